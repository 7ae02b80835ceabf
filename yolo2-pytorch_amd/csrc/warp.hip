// warp.hip — the rotation of the data pipeline (transform/augmentation.py:28-75: cv2.warpAffine of the source image with the matrix of
// cv2.getRotationMatrix2D on a grown canvas) for a whole batch in ONE launch: y2_warp_affine_images (include/yolo2_hip.h).
//
// The stage in front of y2_collate_images: every uint8 HWC source image of the packed batch is resampled through its own inverse affine map into
// an intermediate byte buffer whose tables (dst_offset, dst_geom) are the ones y2_collate_images reads next.  The arithmetic is the 8-bit
// INTER_LINEAR / BORDER_CONSTANT recipe of the header: four exactly rounded double products and two sums per coordinate (this file is compiled
// with -ffp-contract=off like the rest), everything after the two roundings to integers is integer, so y2_warp_affine_images_host (host.hip) is
// bit-identical.
//
// A streaming gather: per destination pixel 12 gathered source bytes (served by the caches: a destination row is a straight line through the
// source, neighbouring lanes share taps and cache lines) and 3 bytes stored; a lane owns 4 consecutive pixels = three dwords = ONE 12-byte store.
#include "common.h"

namespace {

constexpr int WP_ROWS = 16;         // destination rows per workgroup: a 375x500 image is 24 workgroups of 2000 four-pixel items, 8 per thread

// rint to an int32 through a saturating clamp: a table the device cannot check (NaN, infinities, huge entries) still gives a defined value
__device__ inline long long wp_round(double v) { return (long long)(int)fmin(fmax(rint(v), -2147483648.0), 2147483647.0); }

__device__ inline int wp_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ inline int wp_clamp16(long long v) { return (int)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }

struct alignas(4) WpDwords { unsigned d[3]; };          // four pixels: 12 bytes, stored as one three-dword store

struct WarpArgs {
    const uint8_t* src; const int64_t* src_offset; const int32_t* src_geom; const double* inv;
    uint8_t* dst; const int64_t* dst_offset; const int32_t* dst_geom;
    int max_h, max_w, fill;
};

// One destination pixel: the three levels packed as b0 | b1 << 8 | b2 << 16.  X, Y: the coordinates in 1/32 pixel.
__device__ inline unsigned wp_pixel(const uint8_t* img, int stride, int src_h, int src_w, int flip, long long X, long long Y, int fill) {
    const int sx = wp_clamp16(X >> 5), sy = wp_clamp16(Y >> 5);
    const int ax = (int)(X & 31), ay = (int)(Y & 31);
    const int w00 = (32 - ax) * (32 - ay), w01 = ax * (32 - ay), w10 = (32 - ax) * ay, w11 = ax * ay;
    // a tap outside the image is the fill level.  Every load is unconditional and goes to the nearest position INSIDE the image the table names (its
    // value is dropped where the tap is outside): the loads of an item are in flight together, adjacent channel bytes paired by the compiler, where a
    // guard per load compiled to 96 branches and measured 37 % slower
    const bool x0 = sx >= 0 && sx < src_w, x1 = sx + 1 >= 0 && sx + 1 < src_w;
    const bool y0 = sy >= 0 && sy < src_h, y1 = sy + 1 >= 0 && sy + 1 < src_h;
    const int k0 = wp_clamp(sx, 0, src_w - 1), k1 = wp_clamp(sx + 1, 0, src_w - 1);
    const int c0 = 3 * (flip ? src_w - 1 - k0 : k0), c1 = 3 * (flip ? src_w - 1 - k1 : k1);
    const uint8_t* r0 = img + (long long)wp_clamp(sy, 0, src_h - 1) * stride;
    const uint8_t* r1 = img + (long long)wp_clamp(sy + 1, 0, src_h - 1) * stride;
    unsigned out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int f = (fill >> (8 * c)) & 255;
        const int v00 = r0[c0 + c], v01 = r0[c1 + c], v10 = r1[c0 + c], v11 = r1[c1 + c];
        const int p00 = (y0 && x0) ? v00 : f, p01 = (y0 && x1) ? v01 : f, p10 = (y1 && x0) ? v10 : f, p11 = (y1 && x1) ? v11 : f;
        out |= (unsigned)((p00 * w00 + p01 * w01 + p10 * w10 + p11 * w11 + 512) >> 10) << (8 * c);
    }
    return out;
}

// Workgroup (blockIdx.x, blockIdx.y) = (block of WP_ROWS destination rows, image).  The threads walk the block's (row, 4-pixel group) items in
// row-major order, so a wave writes 768 consecutive bytes of a destination row.  Every lane computes its own coordinates: two double products per
// column and two products and sums per row (staging the per-column terms in LDS measured the same: DESIGN 3.6c).
__global__ __launch_bounds__(256) void warp_affine_images_kernel(const WarpArgs a) {
    const int b = blockIdx.y, t = threadIdx.x;
    const int32_t* sg = a.src_geom + 4 * (size_t)b;
    const int32_t* dg = a.dst_geom + 8 * (size_t)b;
    const int stride = sg[0], src_h = sg[1], src_w = sg[2], flip = sg[3];
    const int dstride = dg[0], dst_h = min(dg[1], a.max_h), dst_w = min(dg[2], a.max_w);
    const int row_first = blockIdx.x * WP_ROWS;
    if (src_h <= 0 || src_w <= 0 || dst_w <= 0 || row_first >= dst_h) return;          // (uniform per workgroup)
    const int rows = min(WP_ROWS, dst_h - row_first);
    const double* A = a.inv + 6 * (size_t)b;
    const double A0 = A[0], A1 = A[1], A2 = A[2], A3 = A[3], A4 = A[4], A5 = A[5];
    const uint8_t* img = a.src + a.src_offset[b];
    uint8_t* out = a.dst + a.dst_offset[b];
    const bool dwords = ((reinterpret_cast<uintptr_t>(out) | (unsigned)dstride) & 3u) == 0;      // every row, and so every 12-byte item, starts on a dword
    const int Q = (dst_w + 3) >> 2;
    for (int item = t; item < rows * Q; item += 256) {
        const int r = item / Q, x = (item - r * Q) << 2, y = row_first + r;
        const long long X0 = wp_round((A1 * (double)y + A2) * 1024.0) + 16, Y0 = wp_round((A4 * (double)y + A5) * 1024.0) + 16;
        unsigned px[4];
        const int n = min(4, dst_w - x);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            px[j] = 0;
            if (j < n) {
                const double xd = (double)(x + j);
                const long long X = (X0 + wp_round((A0 * xd) * 1024.0)) >> 5, Y = (Y0 + wp_round((A3 * xd) * 1024.0)) >> 5;
                px[j] = wp_pixel(img, stride, src_h, src_w, flip, X, Y, a.fill);
            }
        }
        uint8_t* o = out + (long long)y * dstride + 3 * x;
        if (dwords && n == 4) {
            WpDwords v;
            v.d[0] = px[0] | (px[1] << 24);
            v.d[1] = (px[1] >> 8) | (px[2] << 16);
            v.d[2] = (px[2] >> 16) | (px[3] << 8);
            *reinterpret_cast<WpDwords*>(o) = v;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {          // a caller's unaligned layout, or the last 1-3 pixels of a row: nothing beyond 3 * dst_w is written
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

extern "C" int y2_warp_affine_images(const uint8_t* src, const int64_t* src_offset, const int32_t* src_geom, const double* inv,
                                     uint8_t* dst, const int64_t* dst_offset, const int32_t* dst_geom,
                                     int32_t B, int32_t max_h, int32_t max_w, int32_t fill, y2_stream_t stream) {
    if (B < 0 || max_h < 1 || max_h > Y2_WARP_MAX_DIM || max_w < 1 || max_w > Y2_WARP_MAX_DIM || (fill & ~0xffffff)) return Y2_EINVAL;
    if (B == 0) return Y2_OK;
    if (B > 65535) return Y2_ENOSUP;
    if (!src || !src_offset || !src_geom || !inv || !dst || !dst_offset || !dst_geom) return Y2_EINVAL;
    WarpArgs a;
    a.src = src; a.src_offset = src_offset; a.src_geom = src_geom; a.inv = inv;
    a.dst = dst; a.dst_offset = dst_offset; a.dst_geom = dst_geom;
    a.max_h = max_h; a.max_w = max_w; a.fill = fill;
    Y2_LAUNCH("warp_affine_images_kernel", 0.0, warp_affine_images_kernel, dim3(y2_cdiv(max_h, WP_ROWS), B), dim3(256), 0, y2_s(stream), a);
    Y2_LAUNCH_CHECK();
    return Y2_OK;
}
