// jpeg.hip — baseline JPEG decoding of a whole batch on the device: y2_jpeg_decode_images (include/yolo2_hip.h), the stage in front of
// y2_warp_affine_images / y2_collate_images / y2_collate_jitter_images.  The decoder itself is csrc/jpeg.h, shared with the host function.
//
// Three launches, the image's scratch (coefficients, component planes) between them:
//   A  jpeg_entropy_kernel: Huffman decoding, serial per image - ONE lane of a 64-lane workgroup decodes, with the bit buffer in registers and the
//      four look-ahead tables in LDS; the other 63 lanes stage the stream through LDS in 4-KB chunks (16-byte loads) and zero the coefficient blocks
//      ahead of the decoding lane.  An image is one segment: restart markers are verified as they come.  Images are workgroups, so a batch of 64
//      spreads over 64 CUs.
//   B1 jpeg_idct_kernel: dequantisation + 8x8 integer IDCT, one thread per block, 128 contiguous bytes read and eight 8-byte rows written.
//   B2 jpeg_colour_kernel: chroma upsampling + colour conversion + BGR store, one thread per 4 pixels = ONE 12-byte store (as warp.hip).
// Every index comes out of jp_layout() / jp_extents_ok(): an image whose descriptor, dst_geom row or extents do not fit gets status JP_ETABLE and
// is touched by none of the three kernels.
#include "common.h"
#include "jpeg.h"

namespace {

constexpr int JA_CHUNK = 4096;          // stream bytes staged per round
constexpr int JA_MARGIN = 512;          // the decoding lane starts no MCU this close to the chunk's end (bytes beyond it are read from memory: slow, correct)
constexpr int JA_AHEAD = 128;           // MCUs zeroed ahead per round at most

struct JpegArgs {
    const uint8_t* src; long long src_bytes; const int64_t* src_offset; const uint8_t* desc;
    uint8_t* dst; long long dst_bytes; const int64_t* dst_offset; const int32_t* dst_geom;
    uint8_t* ws; long long per_image; int32_t* status;
};

__device__ inline bool jpeg_image(const JpegArgs& a, int b, JpLayout& L) {
    L = jp_layout(reinterpret_cast<const JpDesc*>(a.desc + (size_t)b * JP_DESC_BYTES));
    return jp_extents_ok(L, a.src_bytes, a.src_offset[b], a.dst_bytes, a.dst_offset[b], a.dst_geom + 8 * (size_t)b, a.per_image);
}

typedef const __attribute__((address_space(3))) uint8_t* LdsBytes;          // spelled out, so that a load is a ds_read and never a flat load of a selected pointer

// the segment as the decoding lane sees it: the staged chunk [cb, ce) from LDS, anything else from memory; the zigzag table from LDS
struct JaSrc {
    const uint8_t* seg; LdsBytes lds; LdsBytes nat; int cb, ce;
    __device__ int byte(int i) const {
        if (i >= cb && i < ce) return lds[i - cb];
        return seg[i];
    }
    __device__ uint32_t bytes4(int i) const {
        if (i >= cb && i + 3 < ce) {
            LdsBytes p = lds + (i - cb);
            return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
        }
        return ((uint32_t)seg[i] << 24) | ((uint32_t)seg[i + 1] << 16) | ((uint32_t)seg[i + 2] << 8) | (uint32_t)seg[i + 3];
    }
    __device__ int natural(int k) const { return nat[k & 63]; }
};

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const JpegArgs a) {
    __shared__ JpHuff huff[4];
    __shared__ uint4 chunk[JA_CHUNK / 16];
    __shared__ JpState st;
    __shared__ uint8_t natural[64];
    const int b = blockIdx.x, t = threadIdx.x;
    JpLayout L;
    if (!jpeg_image(a, b, L)) {          // (uniform per workgroup)
        if (t == 0) a.status[b] = JP_ETABLE;
        return;
    }
    const JpDesc* d = reinterpret_cast<const JpDesc*>(a.desc + (size_t)b * JP_DESC_BYTES);
    {
        const uint32_t* from = reinterpret_cast<const uint32_t*>(d->huff);
        uint32_t* to = reinterpret_cast<uint32_t*>(huff);
        for (int i = t; i < (int)(sizeof(huff) / 4); i += 64) to[i] = from[i];
    }
    const long long seg_at = a.src_offset[b] + L.scan_offset;
    const uint8_t* seg = a.src + seg_at;
    const int len = L.scan_bytes;
    uint4* coefs = reinterpret_cast<uint4*>(a.ws + (size_t)b * a.per_image);
    if (t == 0) jp_start(st, L, len);
    natural[t] = (uint8_t)jp_natural(t);
    int zeroed = 0;
    __syncthreads();
    for (;;) {
        const int pos = st.b.pos, mcu = st.mcu;
        // stage [cb, cb + JA_CHUNK): cb at the 16-byte boundary at or below the reader.  Bytes outside the source buffer are zeros (never consumed:
        // the reader asks for bytes of the segment only).
        const int cb = pos - (int)(reinterpret_cast<uintptr_t>(seg + pos) & 15u);
        const long long at = seg_at + cb;
        for (int i = t; i < JA_CHUNK / 16; i += 64) {
            const long long o = at + 16 * i;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (o >= 0 && o + 16 <= a.src_bytes) v = *reinterpret_cast<const uint4*>(a.src + o);
            else {
                uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (o + k >= 0 && o + k < a.src_bytes) w[k >> 2] |= (uint32_t)a.src[o + k] << (8 * (k & 3));
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            chunk[i] = v;
        }
        const int ahead = min(L.nmcu, mcu + JA_AHEAD);
        if (ahead > zeroed) {
            const long long z0 = (long long)zeroed * L.bpm * 8, z1 = (long long)ahead * L.bpm * 8;          // 16-byte units: a block is 8 of them
            for (long long i = z0 + t; i < z1; i += 64) coefs[i] = make_uint4(0, 0, 0, 0);
            zeroed = ahead;
        }
        __syncthreads();
        if (t == 0) {
            JpState s = st;
            JaSrc src;
            src.seg = seg; src.lds = (LdsBytes)reinterpret_cast<uint8_t*>(chunk); src.nat = (LdsBytes)natural; src.cb = cb; src.ce = cb + JA_CHUNK;
            const int stop = (long long)cb + JA_CHUNK >= len ? 0x7fffffff : cb + JA_CHUNK - JA_MARGIN;
            jp_decode_mcus(s, L, huff, src, reinterpret_cast<int16_t*>(coefs), zeroed, stop);
            st = s;
        }
        __syncthreads();
        if (st.mcu >= L.nmcu) break;
    }
    if (t == 0) a.status[b] = jp_finish(st);
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const JpegArgs a) {
    const int b = blockIdx.y;
    JpLayout L;
    if (!jpeg_image(a, b, L)) return;
    const JpDesc* d = reinterpret_cast<const JpDesc*>(a.desc + (size_t)b * JP_DESC_BYTES);
    uint8_t* ws = a.ws + (size_t)b * a.per_image;
    const int blocks = L.nmcu * L.bpm;          // <= 6 * 2^22
    for (int i = blockIdx.x * 256 + threadIdx.x; i < blocks; i += gridDim.x * 256) {
        int comp, px, py;
        jp_block_place(L, i, comp, px, py);
        const int pw = jp_of(L.pw, comp);
        jp_idct(reinterpret_cast<const int16_t*>(ws) + 64 * (long long)i, d->quant[jp_of(L.tq, comp)], ws + jp_of(L.plane, comp) + (long long)py * pw + px, pw);
    }
}

struct alignas(4) JpDwords { unsigned d[3]; };          // four pixels: 12 bytes, stored as one three-dword store

__global__ __launch_bounds__(256) void jpeg_colour_kernel(const JpegArgs a) {
    const int b = blockIdx.y;
    JpLayout L;
    if (!jpeg_image(a, b, L)) return;
    const uint8_t* ws = a.ws + (size_t)b * a.per_image;
    uint8_t* out = a.dst + a.dst_offset[b];
    const long long stride = a.dst_geom[8 * (size_t)b];
    const bool dwords = ((reinterpret_cast<uintptr_t>(out) | (unsigned long long)stride) & 3u) == 0;
    const int Q = (L.w + 3) >> 2;
    const long long items = (long long)L.h * Q;
    for (long long item = blockIdx.x * 256 + threadIdx.x; item < items; item += (long long)gridDim.x * 256) {
        const int y = (int)(item / Q), x = (int)(item - (long long)y * Q) << 2, n = min(4, L.w - x);
        unsigned px[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) px[j] = j < n ? jp_pixel(L, ws, x + j, y) : 0u;
        uint8_t* o = out + y * stride + 3 * x;
        if (dwords && n == 4) {
            JpDwords v;
            v.d[0] = px[0] | (px[1] << 24);
            v.d[1] = (px[1] >> 8) | (px[2] << 16);
            v.d[2] = (px[2] >> 16) | (px[3] << 8);
            *reinterpret_cast<JpDwords*>(o) = v;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {          // an unaligned layout, or the last 1-3 pixels of a row: nothing beyond 3 * w is written
                if (j < n) {
                    o[3 * j] = (uint8_t)px[j];
                    o[3 * j + 1] = (uint8_t)(px[j] >> 8);
                    o[3 * j + 2] = (uint8_t)(px[j] >> 16);
                }
            }
        }
    }
}

}  // namespace

extern "C" int y2_jpeg_decode_images(const uint8_t* src, int64_t src_bytes, const int64_t* src_offset, const uint8_t* desc,
                                     uint8_t* dst, int64_t dst_bytes, const int64_t* dst_offset, const int32_t* dst_geom,
                                     uint8_t* ws, int64_t ws_bytes, int32_t* status, int32_t B, y2_stream_t stream) {
    if (B < 0 || src_bytes < 0 || dst_bytes < 0 || ws_bytes < 0) return Y2_EINVAL;
    if (B == 0) return Y2_OK;
    if (B > 65535) return Y2_ENOSUP;
    if (!src || !src_offset || !desc || !dst || !dst_offset || !dst_geom || !ws || !status) return Y2_EINVAL;
    if ((reinterpret_cast<uintptr_t>(ws) & 15u) || (reinterpret_cast<uintptr_t>(desc) & 3u)) return Y2_EALIGN;
    JpegArgs a;
    a.src = src; a.src_bytes = src_bytes; a.src_offset = src_offset; a.desc = desc;
    a.dst = dst; a.dst_bytes = dst_bytes; a.dst_offset = dst_offset; a.dst_geom = dst_geom;
    a.ws = ws; a.per_image = (ws_bytes / B) & ~15LL; a.status = status;
    // the grids follow the scratch the caller sized from the descriptors (an image has at most per_image / 192 blocks and per_image / 12 four-pixel
    // items); the kernels stride over whatever is left
    const int gi = (int)std::min<long long>(std::max<long long>(y2_cdiv(a.per_image / 192, 256), 1), 4096);
    const int gc = (int)std::min<long long>(std::max<long long>(y2_cdiv(a.per_image / 12, 1024), 1), 4096);
    Y2_LAUNCH("jpeg_entropy_kernel", 0.0, jpeg_entropy_kernel, dim3(B), dim3(64), 0, y2_s(stream), a);
    Y2_LAUNCH_CHECK();
    Y2_LAUNCH("jpeg_idct_kernel", 0.0, jpeg_idct_kernel, dim3(gi, B), dim3(256), 0, y2_s(stream), a);
    Y2_LAUNCH_CHECK();
    Y2_LAUNCH("jpeg_colour_kernel", 0.0, jpeg_colour_kernel, dim3(gc, B), dim3(256), 0, y2_s(stream), a);
    Y2_LAUNCH_CHECK();
    return Y2_OK;
}
