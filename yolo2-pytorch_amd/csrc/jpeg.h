// jpeg.h — the baseline JPEG decoder of the data pipeline, ONE copy for the device kernels (jpeg.hip) and the host functions (host.hip): the marker
// parser behind y2_jpeg_probe_host, the descriptor record it fills, the layout of an image's scratch, the Huffman bit reader, the integer IDCT, the
// chroma upsampling and the colour conversion.  The recipes are stated in include/yolo2_hip.h (libjpeg-turbo's defaults: JDCT_ISLOW, fancy upsampling).
// Integer arithmetic only: device and host give the same bytes and the same status.
//
// Safety rules of this file (the inputs are files from disk): nothing taken from the stream or from a descriptor is used as an index, a size or a
// loop bound before it was clamped or checked - jp_layout() is the one place that turns descriptor fields into geometry, the Src object (byte / bytes4) is the one
// place the stream is read, and a block takes at most 64 coefficients whatever the symbols say.
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef Y2_HD
#define Y2_HD __host__ __device__ inline
#endif

#define JP_MAX_DIM 16384
#define JP_DESC_BYTES 4096

// status of one image (y2_jpeg_decode_images: status[b]); the FIRST thing that went wrong stays
enum { JP_OK = 0, JP_EEND = 1 /* bits consumed past the end of the segment */, JP_ERST = 2 /* no RSTn where the interval ends */,
       JP_ECODE = 3 /* no such Huffman code, or a run past coefficient 63 */, JP_ETRAIL = 4 /* bytes left behind the last MCU */,
       JP_ETABLE = 5 /* the descriptor, its dst_geom row or its extents do not fit: nothing was written */ };

// One Huffman table in decoding form: look[first 8 bits] = length << 8 | symbol for the codes of up to 8 bits (0: longer), maxcode[l] = the largest
// code of l bits (-1: none), valoff[l] = index of its first symbol minus its first code.
struct JpHuff {
    int32_t maxcode[18];
    int32_t valoff[18];
    uint16_t look[256];
    uint8_t sym[256];
};

// The descriptor record of one file (Y2_JPEG_DESC_BYTES).  The first eight int32 are part of the ABI (include/yolo2_hip.h).
struct JpDesc {
    int32_t height, width, ncomp, hmax, vmax, restart, scan_offset, scan_bytes;
    int32_t tq[3], td[3], ta[3];          // per component: quantisation table 0 .. 3, DC table 0 .. 1, AC table 0 .. 1
    int32_t reserved[7];
    uint8_t quant[4][64];                 // natural (row-major) order
    JpHuff huff[4];                       // DC 0, DC 1, AC 0, AC 1
    uint8_t pad[96];
};
static_assert(sizeof(JpHuff) == 912 && sizeof(JpDesc) == JP_DESC_BYTES, "descriptor layout");

// zigzag position -> natural position
Y2_HD int jp_natural(int k) {
    static constexpr uint8_t t[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return t[k & 63];
}

// ---- geometry: everything the decoder indexes with, derived from CHECKED descriptor fields
// Scratch of one image: the coefficient blocks int16 [nmcu][bpm][64] in decoding order (luma blocks of the MCU row-major, then Cb, then Cr), then the
// component planes uint8 [ph][pw] at block-padded sizes.  Component c > 0 is sampled 1 x 1, component 0 hmax x vmax.
struct JpLayout {
    int ok;
    int h, w, ncomp, hmax, vmax, restart, mcux, mcuy, bpm, nmcu;
    int tq[3], td[3], ta[3];
    int pw[3], ph[3];                     // plane sizes (multiples of 8)
    int cw[3], ch[3];                     // the components' downsampled sizes ceil(size * samp / max_samp)
    long long plane[3];                   // byte offsets of the planes behind the coefficients
    long long bytes;                      // the whole scratch (a multiple of 64)
    int scan_offset, scan_bytes;
};

Y2_HD JpLayout jp_layout(const JpDesc* d) {
    JpLayout L;
    L.ok = 0;
    L.h = d->height; L.w = d->width; L.ncomp = d->ncomp; L.hmax = d->hmax; L.vmax = d->vmax; L.restart = d->restart;
    L.scan_offset = d->scan_offset; L.scan_bytes = d->scan_bytes;
    bool good = L.h >= 1 && L.h <= JP_MAX_DIM && L.w >= 1 && L.w <= JP_MAX_DIM && (L.ncomp == 1 || L.ncomp == 3) && (L.hmax == 1 || L.hmax == 2)
                && (L.vmax == 1 || L.vmax == 2) && !(L.vmax == 2 && L.hmax == 1) && !(L.ncomp == 1 && (L.hmax != 1 || L.vmax != 1))
                && L.restart >= 0 && L.restart <= 65535 && L.scan_offset >= 0 && L.scan_bytes >= 0;
    for (int c = 0; c < 3; ++c) {
        L.tq[c] = d->tq[c]; L.td[c] = d->td[c]; L.ta[c] = d->ta[c];
        good = good && L.tq[c] >= 0 && L.tq[c] <= 3 && L.td[c] >= 0 && L.td[c] <= 1 && L.ta[c] >= 0 && L.ta[c] <= 1;
    }
    if (!good) {          // a defined, harmless geometry for a caller that forgets to look at `ok`
        L.h = L.w = L.ncomp = L.hmax = L.vmax = 1; L.restart = 0; L.scan_offset = L.scan_bytes = 0;
        for (int c = 0; c < 3; ++c) L.tq[c] = L.td[c] = L.ta[c] = 0;
    }
    L.mcux = (L.w + 8 * L.hmax - 1) / (8 * L.hmax);
    L.mcuy = (L.h + 8 * L.vmax - 1) / (8 * L.vmax);
    L.nmcu = L.mcux * L.mcuy;                                   // <= 2048 * 2048
    L.bpm = L.ncomp == 1 ? 1 : L.hmax * L.vmax + 2;
    long long at = (long long)L.nmcu * L.bpm * 128;
    for (int c = 0; c < 3; ++c) {
        const int hs = c == 0 ? L.hmax : 1, vs = c == 0 ? L.vmax : 1;
        L.pw[c] = L.mcux * 8 * hs; L.ph[c] = L.mcuy * 8 * vs;
        L.cw[c] = (L.w * hs + L.hmax - 1) / L.hmax; L.ch[c] = (L.h * vs + L.vmax - 1) / L.vmax;
        L.plane[c] = at;
        if (c < L.ncomp) at += (long long)L.pw[c] * L.ph[c];
    }
    L.bytes = at;
    L.ok = good ? 1 : 0;
    return L;
}

// a[c] for c in 0 .. 2 without indexing by a variable (on the device that would move the whole layout from registers into scratch memory)
template <class T>
Y2_HD T jp_of(const T (&a)[3], int c) { return c == 0 ? a[0] : (c == 1 ? a[1] : a[2]); }

// Where block i (decoding order) of the image lands: component, and the top-left sample of the block inside the component's plane.
Y2_HD void jp_block_place(const JpLayout& L, int i, int& comp, int& px, int& py) {
    const int mcu = i / L.bpm, j = i - mcu * L.bpm, my = mcu / L.mcux, mx = mcu - my * L.mcux, nl = L.ncomp == 1 ? 1 : L.hmax * L.vmax;
    if (j < nl) { comp = 0; px = 8 * (mx * L.hmax + j % L.hmax); py = 8 * (my * L.vmax + j / L.hmax); }
    else { comp = j - nl + 1; px = 8 * mx; py = 8 * my; }
}

// The dst_geom row and the extents of image b against its layout: true when every byte the decoder will read and write is inside the buffers.
Y2_HD bool jp_extents_ok(const JpLayout& L, long long src_bytes, long long src_offset, long long dst_bytes, long long dst_offset, const int32_t* geom,
                         long long ws_per_image) {
    const long long stride = geom[0];
    return L.ok && geom[1] == L.h && geom[2] == L.w && stride >= 3LL * L.w && dst_offset >= 0 && dst_offset + (L.h - 1) * stride + 3LL * L.w <= dst_bytes
           && src_offset >= 0 && src_offset <= src_bytes && (long long)L.scan_offset + L.scan_bytes <= src_bytes - src_offset && L.bytes <= ws_per_image;
}

// ---- the bit reader
// Src: `int byte(int i) const`, byte i of the entropy-coded segment, called for 0 <= i < end only; `uint32_t bytes4(int i) const`, bytes i .. i + 3 as one
// big-endian word, called for 0 <= i and i + 3 < end only; `int natural(int k) const`, jp_natural(k) from wherever the table is quick to read.
struct JpBits {
    uint64_t buf;          // the low `bits` bits are unread, oldest first
    int bits, real;        // `real` of them came from the stream (the oldest ones); the rest are the zeros fed behind its end or behind a marker
    int pos, end;          // next byte of the segment
    int err, dead;         // dead: an error happened, every further bit is zero
};

Y2_HD void jp_error(JpBits& s, int code) {
    if (!s.err) s.err = code;
    s.dead = 1; s.buf = 0; s.real = 0;
}

template <class Src>
Y2_HD void jp_fill(JpBits& s, const Src& src) {
    uint32_t c = 0;
    bool real = false;
    if (!s.dead && s.pos < s.end) {
        c = (uint32_t)src.byte(s.pos) & 255u;
        if (c != 0xFF) { s.pos += 1; real = true; }
        else if (s.pos < s.end - 1 && (src.byte(s.pos + 1) & 255) == 0) { s.pos += 2; real = true; }          // FF 00: a stuffed FF
        else c = 0;                                                                                              // a marker: stay in front of it
    }
    s.buf = (s.buf << 8) | c;
    s.bits += 8;
    if (real) s.real += 8;
}

// at least n <= 16 unread bits.  Four bytes at once where none of them is FF (no stuffing, no marker: exactly what four jp_fill calls would append).
template <class Src>
Y2_HD void jp_need(JpBits& s, const Src& src, int n) {
    if (s.bits >= n) return;
    if (!s.dead && s.pos < s.end - 3) {
        const uint32_t w = src.bytes4(s.pos);
        if ((((~w) - 0x01010101u) & w & 0x80808080u) == 0) {          // no byte of w is FF
            s.buf = (s.buf << 32) | w;
            s.bits += 32; s.real += 32; s.pos += 4;
            return;
        }
    }
    while (s.bits < n) jp_fill(s, src);
}

Y2_HD void jp_consume(JpBits& s, int n) {
    s.bits -= n;
    if (s.dead) return;
    if (s.real >= n) s.real -= n;
    else jp_error(s, JP_EEND);
}

template <class Src>
Y2_HD int jp_symbol(JpBits& s, const Src& src, const JpHuff* h) {
    jp_need(s, src, 16);
    const uint32_t code = (uint32_t)(s.buf >> (s.bits - 16)) & 0xffffu;
    const uint32_t e = h->look[code >> 8];
    const int n = (int)(e >> 8);
    if (n >= 1 && n <= 8) { jp_consume(s, n); return (int)(e & 255u); }
    for (int l = 9; l <= 16; ++l) {
        const int c = (int)(code >> (16 - l));
        if (c <= h->maxcode[l]) { jp_consume(s, l); return h->sym[((uint32_t)h->valoff[l] + (uint32_t)c) & 255u]; }
    }
    jp_error(s, JP_ECODE);
    return 0;
}

// n extra bits (0 .. 15), sign-extended: a value below 2^(n-1) stands for value - 2^n + 1
template <class Src>
Y2_HD int jp_extend(JpBits& s, const Src& src, int n) {
    if (n == 0) return 0;
    jp_need(s, src, n);
    const int v = (int)((uint32_t)(s.buf >> (s.bits - n)) & ((1u << n) - 1u));
    jp_consume(s, n);
    return v < (1 << (n - 1)) ? v - (1 << n) + 1 : v;
}

// One block into 64 ZEROED coefficients (natural order); returns the component's new DC prediction.  At most 63 AC symbols.
template <class Src>
Y2_HD int jp_block(JpBits& s, const Src& src, const JpHuff* dc, const JpHuff* ac, int pred, int16_t* coef) {
    int t = jp_symbol(s, src, dc);
    if (t > 15) { jp_error(s, JP_ECODE); t = 0; }
    pred = (int16_t)(pred + jp_extend(s, src, t));
    coef[0] = (int16_t)pred;
    for (int k = 1; k < 64; ++k) {
        const int rs = jp_symbol(s, src, ac), r = rs >> 4, n = rs & 15;
        if (n) {
            k += r;
            if (k > 63) { jp_error(s, JP_ECODE); break; }
            coef[src.natural(k) & 63] = (int16_t)jp_extend(s, src, n);
        } else {
            if (r != 15) break;          // EOB
            k += 15;                     // ZRL
        }
    }
    return pred;
}

struct JpState {
    JpBits b;
    int pred[3];
    int mcu, to_restart, next_rst;
};

Y2_HD void jp_start(JpState& st, const JpLayout& L, int seg_bytes) {
    st.b.buf = 0; st.b.bits = st.b.real = 0; st.b.pos = 0; st.b.end = seg_bytes; st.b.err = 0; st.b.dead = 0;
    st.pred[0] = st.pred[1] = st.pred[2] = 0;
    st.mcu = 0; st.to_restart = L.restart; st.next_rst = 0;
}

// MCUs [st.mcu, mcu_stop) while the reader stands in front of pos_stop at the start of an MCU.  coefs: the image's zeroed coefficient blocks.
template <class Src>
Y2_HD void jp_decode_mcus(JpState& st, const JpLayout& L, const JpHuff* huff, const Src& src, int16_t* coefs, int mcu_stop, int pos_stop) {
    JpBits s = st.b;          // (copies, written back below: the device keeps them in registers)
    int p0 = st.pred[0], p1 = st.pred[1], p2 = st.pred[2];
    const int nl = L.ncomp == 1 ? 1 : L.hmax * L.vmax;
    while (st.mcu < mcu_stop && (s.pos < pos_stop || s.dead)) {
        if (L.restart && st.to_restart == 0) {
            if (!s.dead) {
                const bool marker = s.real < 8 && s.pos < s.end - 1 && (src.byte(s.pos) & 255) == 0xFF && (src.byte(s.pos + 1) & 255) == 0xD0 + st.next_rst;
                if (marker) { s.pos += 2; s.buf = 0; s.bits = s.real = 0; }
                else jp_error(s, JP_ERST);
            }
            st.next_rst = (st.next_rst + 1) & 7;
            p0 = p1 = p2 = 0;
            st.to_restart = L.restart;
        }
        int16_t* c = coefs + (long long)st.mcu * L.bpm * 64;
        for (int j = 0; j < nl; ++j) p0 = jp_block(s, src, huff + L.td[0], huff + 2 + L.ta[0], p0, c + 64 * j);
        if (L.ncomp == 3) {          // (spelled out: a component index that is a variable would put the layout into scratch memory on the device)
            p1 = jp_block(s, src, huff + L.td[1], huff + 2 + L.ta[1], p1, c + 64 * nl);
            p2 = jp_block(s, src, huff + L.td[2], huff + 2 + L.ta[2], p2, c + 64 * (nl + 1));
        }
        st.mcu += 1;
        if (L.restart) st.to_restart -= 1;
    }
    st.b = s;
    st.pred[0] = p0; st.pred[1] = p1; st.pred[2] = p2;
}

// behind the last MCU: less than a byte of padding and nothing but the end of the segment
Y2_HD int jp_finish(JpState& st) {
    if (!st.b.err && (st.b.real >= 8 || st.b.pos < st.b.end)) st.b.err = JP_ETRAIL;
    return st.b.err;
}

// ---- dequantisation + IDCT (jidctint.c, jpeg_idct_islow: CONST_BITS 13, PASS1_BITS 2).  32-bit arithmetic that wraps (unsigned) instead of
// overflowing: exact for every stream whose intermediate values fit int32, defined for the rest.
Y2_HD int jp_descale(uint32_t x, int n) { return (int32_t)(x + (1u << (n - 1))) >> n; }

Y2_HD void jp_idct_1d(const uint32_t in[8], uint32_t out[8]) {
    uint32_t z2 = in[2], z3 = in[6];
    uint32_t z1 = (z2 + z3) * 4433u;
    uint32_t tmp2 = z1 - z3 * 15137u, tmp3 = z1 + z2 * 6270u;
    z2 = in[0]; z3 = in[4];
    uint32_t tmp0 = (z2 + z3) * 8192u, tmp1 = (z2 - z3) * 8192u;
    const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    uint32_t z4 = tmp1 + tmp3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u; tmp1 *= 16819u; tmp2 *= 25172u; tmp3 *= 12299u;
    z1 *= 0u - 7373u; z2 *= 0u - 20995u; z3 *= 0u - 16069u; z4 *= 0u - 3196u;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    out[0] = tmp10 + tmp3; out[7] = tmp10 - tmp3;
    out[1] = tmp11 + tmp2; out[6] = tmp11 - tmp2;
    out[2] = tmp12 + tmp1; out[5] = tmp12 - tmp1;
    out[3] = tmp13 + tmp0; out[4] = tmp13 - tmp0;
}

// coef [64] (natural order), q [64] -> out: 8 rows of 8 levels, `stride` bytes apart, each row written as one 8-byte unit
Y2_HD void jp_idct(const int16_t* coef, const uint8_t* q, uint8_t* out, long long stride) {
    uint32_t ws[64];
#pragma unroll
    for (int x = 0; x < 8; ++x) {          // columns
        uint32_t in[8], o[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) in[y] = (uint32_t)((int)coef[8 * y + x] * (int)q[8 * y + x]);
        jp_idct_1d(in, o);
#pragma unroll
        for (int y = 0; y < 8; ++y) ws[8 * y + x] = (uint32_t)jp_descale(o[y], 11);          // CONST_BITS - PASS1_BITS
    }
#pragma unroll
    for (int y = 0; y < 8; ++y) {          // rows
        uint32_t o[8];
        jp_idct_1d(ws + 8 * y, o);
        uint64_t row = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const int v = jp_descale(o[x], 18) + 128;          // CONST_BITS + PASS1_BITS + 3
            row |= (uint64_t)(v < 0 ? 0 : (v > 255 ? 255 : v)) << (8 * x);
        }
        memcpy(out + y * stride, &row, 8);
    }
}

// ---- upsampling: the level of a 1 x 1 sampled component at full-resolution pixel (x, y) of an image whose luma is sampled hmax x vmax.
// p: the component's plane, `stride` bytes per row; cw, ch: its downsampled size.  Fancy (triangle) filters where cw > 2, replication otherwise.
Y2_HD int jp_upsample(const uint8_t* p, long long stride, int cw, int ch, int hmax, int vmax, int x, int y) {
    if (hmax == 1) return p[y * stride + x];
    const int i = x >> 1;
    if (vmax == 1) {
        const uint8_t* r = p + y * stride;
        if (cw <= 2) return r[i];
        if (x & 1) return i == cw - 1 ? r[i] : (3 * r[i] + r[i + 1] + 2) >> 2;
        return i == 0 ? r[i] : (3 * r[i] + r[i - 1] + 1) >> 2;
    }
    const int j = y >> 1;
    if (cw <= 2) return p[j * stride + i];
    const int jf = (y & 1) ? (j + 1 < ch ? j + 1 : ch - 1) : (j > 0 ? j - 1 : 0);          // the far row; beyond the first / last real row: that row itself
    const uint8_t* n = p + j * stride;
    const uint8_t* f = p + jf * stride;
    const int cur = 3 * n[i] + f[i];
    if (x & 1) return i == cw - 1 ? (4 * cur + 7) >> 4 : (3 * cur + 3 * n[i + 1] + f[i + 1] + 7) >> 4;
    return i == 0 ? (4 * cur + 8) >> 4 : (3 * cur + 3 * n[i - 1] + f[i - 1] + 8) >> 4;
}

Y2_HD int jp_clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Y, Cb, Cr levels -> B | G << 8 | R << 16 (jdcolor.c: 16-bit fixed point, arithmetic shifts)
Y2_HD uint32_t jp_bgr(int y, int cb, int cr) {
    cb -= 128; cr -= 128;
    const int r = jp_clamp255(y + ((91881 * cr + 32768) >> 16));
    const int b = jp_clamp255(y + ((116130 * cb + 32768) >> 16));
    const int g = jp_clamp255(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    return (uint32_t)b | ((uint32_t)g << 8) | ((uint32_t)r << 16);
}

// Pixel (x, y) of the image from its planes (ws: the image's scratch).
Y2_HD uint32_t jp_pixel(const JpLayout& L, const uint8_t* ws, int x, int y) {
    const int lum = ws[L.plane[0] + (long long)y * L.pw[0] + x];
    if (L.ncomp == 1) return (uint32_t)lum * 0x010101u;
    const int cb = jp_upsample(ws + L.plane[1], L.pw[1], L.cw[1], L.ch[1], L.hmax, L.vmax, x, y);
    const int cr = jp_upsample(ws + L.plane[2], L.pw[2], L.cw[2], L.ch[2], L.hmax, L.vmax, x, y);
    return jp_bgr(lum, cb, cr);
}

// ---- one image on the host, the three device kernels in sequence: entropy decoding into the zeroed coefficient blocks, IDCT into the planes, pixels.
// seg: the entropy-coded segment (L.scan_bytes long); w: the image's scratch (L.bytes); out: its first destination row.  Returns the status.
struct JpHostSrc {
    const uint8_t* seg;
    int byte(int i) const { return seg[i]; }
    uint32_t bytes4(int i) const { return ((uint32_t)seg[i] << 24) | ((uint32_t)seg[i + 1] << 16) | ((uint32_t)seg[i + 2] << 8) | (uint32_t)seg[i + 3]; }
    int natural(int k) const { return jp_natural(k); }
};

inline int jp_decode_image_host(const JpDesc* d, const JpLayout& L, const uint8_t* seg, uint8_t* w, uint8_t* out, long long stride) {
    int16_t* coefs = reinterpret_cast<int16_t*>(w);
    const int blocks = L.nmcu * L.bpm;
    memset(coefs, 0, (size_t)blocks * 128);
    JpHostSrc s;
    s.seg = seg;
    JpState st;
    jp_start(st, L, L.scan_bytes);
    jp_decode_mcus(st, L, d->huff, s, coefs, L.nmcu, 0x7fffffff);
    const int status = jp_finish(st);
    for (int i = 0; i < blocks; ++i) {
        int comp, px, py;
        jp_block_place(L, i, comp, px, py);
        const int pw = jp_of(L.pw, comp);
        jp_idct(coefs + 64 * (long long)i, d->quant[jp_of(L.tq, comp)], w + jp_of(L.plane, comp) + (long long)py * pw + px, pw);
    }
    for (int y = 0; y < L.h; ++y)
        for (int x = 0; x < L.w; ++x) {
            const uint32_t p = jp_pixel(L, w, x, y);
            uint8_t* o = out + y * stride + 3 * x;
            o[0] = (uint8_t)p; o[1] = (uint8_t)(p >> 8); o[2] = (uint8_t)(p >> 16);
        }
    return status;
}

// ---- the marker parser (host only): y2_jpeg_probe_host.  Returns 0, -1 (Y2_EINVAL) or -3 (Y2_ENOSUP); reads [data, data + n) only.
inline int jp_be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Exif orientation (tag 0x0112 of IFD0) of an APP1 payload [p, p + n); 0 when there is none
inline int jp_exif_orientation(const uint8_t* p, int n) {
    if (n < 14 || memcmp(p, "Exif\0\0", 6) != 0) return 0;
    const uint8_t* t = p + 6;
    const int tn = n - 6;
    const bool le = t[0] == 'I' && t[1] == 'I', be = t[0] == 'M' && t[1] == 'M';
    if (!le && !be) return 0;
    auto u16 = [&](int o) { return le ? t[o] | (t[o + 1] << 8) : (t[o] << 8) | t[o + 1]; };
    auto u32 = [&](int o) { return le ? (uint32_t)t[o] | ((uint32_t)t[o + 1] << 8) | ((uint32_t)t[o + 2] << 16) | ((uint32_t)t[o + 3] << 24)
                                      : ((uint32_t)t[o] << 24) | ((uint32_t)t[o + 1] << 16) | ((uint32_t)t[o + 2] << 8) | (uint32_t)t[o + 3]; };
    if (u16(2) != 42) return 0;
    const uint32_t ifd = u32(4);
    if (ifd > (uint32_t)tn || tn - (int)ifd < 2) return 0;
    const int count = u16((int)ifd);
    for (int e = 0; e < count; ++e) {
        const long long o = (long long)ifd + 2 + 12LL * e;
        if (o + 12 > tn) return 0;
        if (u16((int)o) == 0x0112) return (u16((int)o + 2) == 3 && u32((int)o + 4) == 1) ? u16((int)o + 8) : 0;
    }
    return 0;
}

inline int jp_probe(const uint8_t* data, long long nbytes, JpDesc* d) {
    const int EINVAL_ = -1, ENOSUP_ = -3;
    memset(d, 0, sizeof(JpDesc));
    if (!data || nbytes < 4 || nbytes > 0x7fffffffLL || data[0] != 0xFF || data[1] != 0xD8) return EINVAL_;
    const int n = (int)nbytes;
    bool have_q[4] = {false, false, false, false}, have_h[4] = {false, false, false, false}, sof = false, jfif = false;
    int comp_id[3] = {0, 0, 0}, comp_h[3] = {1, 1, 1}, comp_v[3] = {1, 1, 1}, adobe = -1, orientation = 0;
    int pos = 2;
    for (;;) {
        if (pos + 2 > n || data[pos] != 0xFF) return EINVAL_;
        while (pos + 1 < n && data[pos + 1] == 0xFF) ++pos;          // fill bytes in front of a marker
        if (pos + 2 > n) return EINVAL_;
        const int m = data[pos + 1];
        pos += 2;
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;        // stand-alone markers
        if (m == 0xD8 || m == 0xD9 || m == 0x00) return EINVAL_;    // a second SOI, EOI in front of a scan
        if (pos + 2 > n) return EINVAL_;
        const int len = jp_be16(data + pos);
        if (len < 2 || pos + len > n) return EINVAL_;
        const uint8_t* p = data + pos + 2;
        const int pn = len - 2;
        if (m == 0xC0) {
            if (sof || pn < 6) return EINVAL_;
            const int prec = p[0], nf = p[5];
            d->height = jp_be16(p + 1); d->width = jp_be16(p + 3);
            if (prec == 12) return ENOSUP_;
            if (prec != 8 || d->height == 0 || d->width == 0 || nf == 0 || pn != 6 + 3 * nf) return EINVAL_;
            if (d->height > JP_MAX_DIM || d->width > JP_MAX_DIM || (nf != 1 && nf != 3)) return ENOSUP_;
            for (int c = 0; c < nf; ++c) {
                comp_id[c] = p[6 + 3 * c]; comp_h[c] = p[7 + 3 * c] >> 4; comp_v[c] = p[7 + 3 * c] & 15; d->tq[c] = p[8 + 3 * c];
                if (comp_h[c] < 1 || comp_h[c] > 4 || comp_v[c] < 1 || comp_v[c] > 4 || d->tq[c] > 3) return EINVAL_;
            }
            d->ncomp = nf;
            sof = true;
        } else if ((m >= 0xC1 && m <= 0xCF) && m != 0xC4 && m != 0xC8) {
            return ENOSUP_;                                         // extended, progressive, lossless, arithmetic (and DAC)
        } else if (m == 0xC4) {
            int at = 0;
            while (at < pn) {
                if (at + 17 > pn) return EINVAL_;
                const int tc = p[at] >> 4, th = p[at] & 15;
                if (tc > 1 || th > 3) return EINVAL_;
                int total = 0;
                for (int l = 1; l <= 16; ++l) total += p[at + l];
                if (total > 256 || at + 17 + total > pn) return EINVAL_;
                if (th > 1) return ENOSUP_;
                JpHuff* h = &d->huff[2 * tc + th];
                memset(h, 0, sizeof(JpHuff));
                memcpy(h->sym, p + at + 17, (size_t)total);
                int code = 0, k = 0;
                for (int l = 1; l <= 16; ++l) {
                    const int cnt = p[at + l];
                    if (code + cnt > (1 << l)) return EINVAL_;     // the counts over-subscribe the code space
                    h->maxcode[l] = cnt ? code + cnt - 1 : -1;
                    h->valoff[l] = k - code;
                    if (l <= 8)
                        for (int i = 0; i < cnt; ++i)
                            for (int f = 0; f < (1 << (8 - l)); ++f) h->look[((code + i) << (8 - l)) + f] = (uint16_t)((l << 8) | h->sym[k + i]);
                    k += cnt; code = (code + cnt) << 1;
                }
                h->maxcode[0] = h->maxcode[17] = -1;
                have_h[2 * tc + th] = true;
                at += 17 + total;
            }
        } else if (m == 0xDB) {
            int at = 0;
            while (at < pn) {
                const int pq = p[at] >> 4, tq = p[at] & 15;
                if (pq > 1 || tq > 3) return EINVAL_;
                if (pq == 1) return ENOSUP_;
                if (at + 65 > pn) return EINVAL_;
                for (int k = 0; k < 64; ++k) d->quant[tq][jp_natural(k)] = p[at + 1 + k];
                have_q[tq] = true;
                at += 65;
            }
        } else if (m == 0xDD) {
            if (pn != 2) return EINVAL_;
            d->restart = jp_be16(p);
        } else if (m == 0xE0) {
            if (pn >= 5 && memcmp(p, "JFIF\0", 5) == 0) jfif = true;
        } else if (m == 0xE1) {
            if (!orientation) orientation = jp_exif_orientation(p, pn);
        } else if (m == 0xEE) {
            if (pn >= 12 && memcmp(p, "Adobe", 5) == 0) adobe = p[11];
        } else if (m == 0xDC) {
            return ENOSUP_;                                         // DNL
        } else if (m == 0xDA) {
            if (!sof || pn < 1) return EINVAL_;
            const int ns = p[0];
            if (ns < 1 || ns > 4 || pn != 4 + 2 * ns) return EINVAL_;
            if (ns != d->ncomp) return ENOSUP_;                     // more than one scan
            for (int c = 0; c < ns; ++c) {
                const int td = p[2 + 2 * c] >> 4, ta = p[2 + 2 * c] & 15;
                if (td > 3 || ta > 3) return EINVAL_;
                if (p[1 + 2 * c] != comp_id[c] || td > 1 || ta > 1) return ENOSUP_;
                if (!have_h[td] || !have_h[2 + ta] || !have_q[d->tq[c]]) return EINVAL_;
                d->td[c] = td; d->ta[c] = ta;
            }
            if (p[1 + 2 * ns] != 0 || p[2 + 2 * ns] != 63 || p[3 + 2 * ns] != 0) return EINVAL_;          // Ss, Se, Ah / Al of a sequential scan
            if (d->ncomp == 3) {
                if (comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1 || comp_h[0] > 2 || comp_v[0] > 2 || (comp_v[0] == 2 && comp_h[0] == 1))
                    return ENOSUP_;
                if (adobe == 0 || (adobe < 0 && !jfif && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B')) return ENOSUP_;          // RGB, not YCbCr
                d->hmax = comp_h[0]; d->vmax = comp_v[0];
            } else {
                d->hmax = d->vmax = 1;                              // the single scan of one component: its sampling factors mean nothing
            }
            if (orientation >= 2 && orientation <= 8) return ENOSUP_;          // cv2.imread would turn the image
            const int start = pos + len;
            int i = start;
            while (i < n && !(data[i] == 0xFF && i + 1 < n && data[i + 1] != 0x00 && !(data[i + 1] >= 0xD0 && data[i + 1] <= 0xD7))) ++i;
            if (i < n && data[i + 1] != 0xD9) return ENOSUP_;       // something other than the end of the image behind the scan
            d->scan_offset = start; d->scan_bytes = i - start;
            return 0;
        }
        pos += len;
    }
}
