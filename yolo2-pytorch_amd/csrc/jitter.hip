// jitter.hip — the collate step WITH the colour jitter of the data pipeline (utils/data.py:120-121: resize, then transform_image = RandomBlur, BGR2HSV,
// RandomHue / RandomSaturation / RandomBrightness, HSV2RGB, RandomGamma of transform/image.py; then ToTensor, Normalize) for a whole batch in ONE
// launch: y2_collate_jitter_images (include/yolo2_hip.h).
//
// Everything random but the blur is a per-level map that the workers ship as tables; what runs here is the resize of y2_collate_images (the same
// arithmetic: resample.h), the box blur on the RESIZED image and the two fixed colour-space conversions.  Integer arithmetic, one exactly rounded fp64
// product per blurred value and exactly rounded fp32 operations in HSV2RGB (this file is compiled with -ffp-contract=off like the rest), so
// y2_collate_jitter_images_host (host.hip) is bit-identical.
//
// A workgroup owns one JT_TILE_H x JT_TILE_W tile of one output image.  It stages the image's tables in LDS, computes the resized levels of the tile
// plus the blur's halo (kx - 1 columns, ky - 1 rows: an image with a 1x1 blur has none) into LDS as bytes - halo coordinates are reflected BEFORE the
// resize arithmetic, so a tile reads no other tile's work -, sums rows, then columns, converts colour and writes three fp32 planes, 16 bytes per lane
// and plane where the output allows it.
#include "common.h"
#include "resample.h"

namespace {

constexpr int JT_TILE_H = 32, JT_TILE_W = 32;          // 416 = 13 tiles, 608 = 19: the network's sizes are multiples of 32; one 4-column item per thread
constexpr int JT_HALO = Y2_JITTER_MAX_BLUR - 1;
constexpr int JT_HH = JT_TILE_H + JT_HALO, JT_HW = JT_TILE_W + JT_HALO;
constexpr int JT_PITCH = 40;                           // bytes per level row in LDS: >= JT_HW, a multiple of 4, and the last 4-column group's 12 bytes end inside it
constexpr int JT_GROUPS = JT_TILE_W / 4;
static_assert(JT_TILE_H * JT_GROUPS == 256 && JT_PITCH >= JT_HW && 4 * (JT_GROUPS - 1) + 12 <= JT_PITCH && JT_HH <= 64 && JT_HW <= 64, "tile shape");

struct JitterArgs {
    const uint8_t* src; const int64_t* offset; const int32_t* geom; const int32_t* jitter; const uint8_t* hsv_tab; const float* lut;
    float* out;
    int H, W, swap, vec, tiles_x;
};

// Row sums of one blur width: item (channel, halo row, 4-column group) reads the group's KX + 3 level bytes as aligned dwords and writes four 16-bit
// sums as one 8-byte value.  The width is a template parameter so that every byte is picked with a constant shift.
template <int KX>
__device__ inline void jt_row_sums(const uint32_t* lv, uint64_t* rs, int hh, int groups, int t) {
    constexpr int ND = (KX + 3 + 3) / 4;
    for (int item = t; item < 3 * hh * JT_GROUPS; item += 256) {
        const int q = item & (JT_GROUPS - 1), r = item / JT_GROUPS;
        if (q >= groups) continue;
        const int c = r / hh, hy = r - c * hh;
        const uint32_t* p = lv + (c * JT_HH + hy) * (JT_PITCH / 4) + q;
        uint32_t d[ND];
#pragma unroll
        for (int i = 0; i < ND; ++i) d[i] = p[i];
        uint64_t packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t s = 0;
#pragma unroll
            for (int i = 0; i < KX; ++i) s += (d[(j + i) >> 2] >> (8 * ((j + i) & 3))) & 255u;
            packed |= (uint64_t)s << (16 * j);
        }
        rs[(c * JT_HH + hy) * JT_GROUPS + q] = packed;
    }
}

__global__ __launch_bounds__(256) void collate_jitter_images_kernel(const JitterArgs a) {
    __shared__ float s_lut[768];                                  // the image's output table
    __shared__ __attribute__((aligned(4))) uint8_t s_hsv[768];    // its H, S, V tables
    __shared__ int s_sdiv[256], s_hdiv[256];                      // BGR2HSV's division tables
    __shared__ int s_xo0[JT_HW], s_xo1[JT_HW], s_xc[JT_HW];       // per halo column: byte offsets of the two taps in a source row, coefficients
    __shared__ int s_yr0[JT_HH], s_yr1[JT_HH], s_yc[JT_HH];       // per halo row: the two source rows, coefficients
    __shared__ uint32_t s_lv[3 * JT_HH * (JT_PITCH / 4)];         // resized levels [channel][halo row][JT_PITCH bytes]
    __shared__ uint64_t s_rs[3 * JT_HH * JT_GROUPS];              // row sums [channel][halo row][column] x 16 bit
    const int H = a.H, W = a.W;
    const int b = blockIdx.y, t = threadIdx.x;
    const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
    const int32_t* g = a.geom + 8 * (size_t)b;
    const int stride = g[0], src_h = g[1], src_w = g[2], wy0 = g[3], wx0 = g[4], wh = g[5], ww = g[6], flip = g[7];
    if (src_h <= 0 || src_w <= 0 || wh <= 0 || ww <= 0) return;          // (uniform per workgroup; the wrappers refuse such a table)
    const int32_t* jt = a.jitter + 4 * (size_t)b;
    // a table on the device cannot be refused: a blur size is brought into range, so that every LDS index below is inside its array
    const int kx = cl_clamp(jt[0], 1, Y2_JITTER_MAX_BLUR), ky = cl_clamp(jt[1], 1, Y2_JITTER_MAX_BLUR);
    const bool hsv = jt[2] != 0 && a.hsv_tab != nullptr;
    const bool box = wh == 2 * H && ww == 2 * W;
    const int x_first = tile_x * JT_TILE_W, y_first = tile_y * JT_TILE_H;
    const int cols = min(JT_TILE_W, W - x_first), rows = min(JT_TILE_H, H - y_first);
    const int hw = cols + kx - 1, hh = rows + ky - 1;
    for (int i = t; i < 768; i += 256) s_lut[i] = a.lut[(size_t)b * 768 + i];
    if (hsv) {
        for (int i = t; i < 768; i += 256) s_hsv[i] = a.hsv_tab[(size_t)b * 768 + i];
        s_sdiv[t] = jt_div(JT_SDIV_N, t);
        s_hdiv[t] = jt_div(JT_HDIV_N, t);
    }
    // halo column / row i of the tile is column x_first + i - kx / 2 (row y_first + i - ky / 2) of the resized image, reflected into it
    if (t < hw) cl_col(jt_reflect101(x_first + t - kx / 2, W), box, ww, W, wx0, flip, src_w, s_xo0[t], s_xo1[t], s_xc[t]);
    else if (t >= 64 && t - 64 < hh) cl_row(jt_reflect101(y_first + (t - 64) - ky / 2, H), box, wh, H, wy0, src_h, s_yr0[t - 64], s_yr1[t - 64], s_yc[t - 64]);
    __syncthreads();
    const uint8_t* img = a.src + a.offset[b];
    uint8_t* lvb = reinterpret_cast<uint8_t*>(s_lv);
    for (int item = t; item < hh * hw; item += 256) {
        const int hy = item / hw, hx = item - hy * hw;
        const uint8_t* p0 = img + (long long)s_yr0[hy] * stride;
        const uint8_t* p1 = img + (long long)s_yr1[hy] * stride;
        const int yc = s_yc[hy], b0 = yc & 0xffff, b1 = yc >> 16;
        const int o0 = s_xo0[hx], o1 = s_xo1[hx], xc = s_xc[hx];
#pragma unroll
        for (int c = 0; c < 3; ++c) lvb[(c * JT_HH + hy) * JT_PITCH + hx] = (uint8_t)cl_level(box, p0, p1, o0 + c, o1 + c, xc, b0, b1);
    }
    __syncthreads();
    const int groups = (cols + 3) >> 2;
    switch (kx) {          // (uniform per workgroup)
        case 1: jt_row_sums<1>(s_lv, s_rs, hh, groups, t); break;
        case 2: jt_row_sums<2>(s_lv, s_rs, hh, groups, t); break;
        case 3: jt_row_sums<3>(s_lv, s_rs, hh, groups, t); break;
        case 4: jt_row_sums<4>(s_lv, s_rs, hh, groups, t); break;
        case 5: jt_row_sums<5>(s_lv, s_rs, hh, groups, t); break;
        case 6: jt_row_sums<6>(s_lv, s_rs, hh, groups, t); break;
        default: jt_row_sums<7>(s_lv, s_rs, hh, groups, t); break;
    }
    __syncthreads();
    // one item per thread: row y, columns 4 q .. 4 q + 3 of the tile; a wave's lanes write consecutive 16-byte pieces of 8 plane rows
    const int q = t & (JT_GROUPS - 1), y = t / JT_GROUPS;
    if (y >= rows || q >= groups) return;
    int lev[3][4];          // blurred levels in source channel order (B, G, R)
    const bool blur = kx * ky > 1;
    const double inv = 1.0 / (double)(kx * ky);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        uint64_t s = 0;          // four 16-bit column sums at once: none exceeds 49 * 255
        for (int j = 0; j < ky; ++j) s += s_rs[(c * JT_HH + y + j) * JT_GROUPS + q];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = (int)((s >> (16 * i)) & 0xffffu);
            lev[c][i] = blur ? jt_blur_level(v, inv) : v;
        }
    }
    const size_t plane = (size_t)H * W;
    float* o = a.out + (size_t)b * 3 * plane + (size_t)(y_first + y) * W + x_first + 4 * q;
    f32x4 v[3];
    if (hsv) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int h, s, val, r, gg, bb;
            jt_bgr2hsv(lev[0][i], lev[1][i], lev[2][i], s_sdiv, s_hdiv, h, s, val);
            jt_hsv2rgb(s_hsv[h], s_hsv[256 + s], s_hsv[512 + val], r, gg, bb);
            v[0][i] = s_lut[r];
            v[1][i] = s_lut[256 + gg];
            v[2][i] = s_lut[512 + bb];
        }
    } else {
        // output plane c reads source channel 2 - c with BGR2RGB
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[0][i] = s_lut[a.swap ? lev[2][i] : lev[0][i]];
            v[1][i] = s_lut[256 + lev[1][i]];
            v[2][i] = s_lut[512 + (a.swap ? lev[0][i] : lev[2][i])];
        }
    }
    if (a.vec) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(o + c * plane) = v[c];
    } else {
        const int n = min(4, cols - 4 * q);
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < n) o[c * plane + i] = v[c][i];
    }
}

}  // namespace

extern "C" int y2_collate_jitter_images(const uint8_t* src, const int64_t* offset, const int32_t* geom, const int32_t* jitter, const uint8_t* hsv_tab,
                                        const float* lut, int32_t B, int32_t H, int32_t W, int32_t flags, float* out, y2_stream_t stream) {
    if (B < 0 || H <= 0 || W <= 0 || W > Y2_COLLATE_MAX_W || (flags & ~1)) return Y2_EINVAL;
    if (B == 0) return Y2_OK;
    if (B > 65535) return Y2_ENOSUP;
    if (!src || !offset || !geom || !jitter || !lut || !out) return Y2_EINVAL;
    JitterArgs a;
    a.src = src; a.offset = offset; a.geom = geom; a.jitter = jitter; a.hsv_tab = hsv_tab; a.lut = lut; a.out = out;
    a.H = H; a.W = W; a.swap = flags & 1;
    a.vec = (W % 4 == 0 && y2_aligned16(out)) ? 1 : 0;          // plane and row sizes are then multiples of 16 bytes too
    a.tiles_x = y2_cdiv(W, JT_TILE_W);
    const long long tiles = (long long)a.tiles_x * y2_cdiv(H, JT_TILE_H);
    if (tiles > 2147483647LL) return Y2_ENOSUP;
    Y2_LAUNCH("collate_jitter_images_kernel", 0.0, collate_jitter_images_kernel, dim3((unsigned)tiles, B), dim3(256), 0, y2_s(stream), a);
    Y2_LAUNCH_CHECK();
    return Y2_OK;
}
