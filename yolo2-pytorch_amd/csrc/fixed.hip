// fixed.hip — the test-time `fixed` resize of the data pipeline (transform/resize/image.py:36-46: an aspect-preserving, scale-only cv2.warpAffine into the
// top-left of a zero canvas, INTER_LINEAR when shrinking and INTER_CUBIC otherwise) fused with BGR2RGB, ToTensor and Normalize for a whole batch in ONE
// launch: y2_fixed_images (include/yolo2_hip.h).
//
// A ragged batch of uint8 HWC source images (one packed byte buffer, any byte alignment) becomes the network's fp32 [B][3][H][W] input with no uint8
// intermediate: every output pixel is resampled through its image's inverse affine map (csrc/fixed.h: the coordinates of y2_warp_affine_images, its
// bilinear level in mode 0, the 4 x 4 cubic table of 15-bit weights in mode 1), its channels are swapped and looked up in the level table.  The
// arithmetic is fixed.h's, shared with y2_fixed_images_host (host.hip); this file is compiled with -ffp-contract=off like the rest: bit-identical.
//
// A streaming gather: per output pixel 12 (linear) or 48 (cubic) gathered source bytes, served by the caches (a destination row is a straight line
// through the source, neighbouring lanes share taps and cache lines), and 12 bytes stored; a lane owns 4 consecutive pixels of the three planes =
// three 16-byte stores.
#include "common.h"
#include "fixed.h"

namespace {

constexpr int FX_ROWS = 16;         // output rows per workgroup: 416x416 x 64 images -> 1664 workgroups, 6-7 items of 4 pixels per thread

struct FixedArgs {
    const uint8_t* src; const int64_t* offset; const int32_t* geom; const double* inv; const float* lut;
    float* out;
    int H, W, swap, vec;
};

// Workgroup (blockIdx.x, blockIdx.y) = (block of FX_ROWS output rows, image).  The level table is staged in LDS once per workgroup; then the threads
// walk the block's (row, 4-pixel group) items in row-major order, so a wave's lanes write consecutive 16-byte pieces of one plane row.  The mode is
// the image's: the branch on it is uniform per workgroup.
template <bool CUBIC>
__device__ inline void fixed_rows(const FixedArgs& a, const float* lut, const uint8_t* img, int stride, int src_h, int src_w, const double* A,
                                  float* out, int row_first, int rows) {
    const int W = a.W, t = threadIdx.x;
    const size_t plane = (size_t)a.H * W;
    const int cs = a.swap ? 2 : 0;          // output plane c reads source channel c ^ cs for c in {0, 2}; channel 1 stays
    const int Q = (W + 3) >> 2;
    for (int item = t; item < rows * Q; item += 256) {
        const int r = item / Q, x = (item - r * Q) << 2, y = row_first + r;
        long long X0, Y0;
        fx_row(A, y, X0, Y0);
        const int n = min(4, W - x);
        unsigned px[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            px[j] = 0;
            if (j < n) {
                long long X, Y;
                fx_position(A, x + j, X0, Y0, X, Y);
                px[j] = CUBIC ? fx_cubic(img, stride, src_h, src_w, X, Y) : fx_linear(img, stride, src_h, src_w, X, Y);
            }
        }
        float* o = out + (size_t)y * W + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int sh = 8 * (c == 1 ? 1 : c ^ cs);
            if (a.vec) {          // W % 4 == 0: n == 4, and every item starts on a 16-byte boundary
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = lut[c * 256 + ((px[j] >> sh) & 255)];
                *reinterpret_cast<f32x4*>(o + c * plane) = v;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < n) o[c * plane + j] = lut[c * 256 + ((px[j] >> sh) & 255)];          // nothing beyond column W - 1 is written
            }
        }
    }
}

__global__ __launch_bounds__(256) void fixed_images_kernel(const FixedArgs a) {
    __shared__ float lut[768];          // [3][256]: the level table
    const int b = blockIdx.y, t = threadIdx.x;
    const int32_t* g = a.geom + 4 * (size_t)b;
    const int stride = g[0], src_h = g[1], src_w = g[2], mode = g[3];
    if (src_h <= 0 || src_w <= 0) return;          // (uniform per workgroup; the wrappers refuse such a table)
    const int row_first = blockIdx.x * FX_ROWS;
    const int rows = min(FX_ROWS, a.H - row_first);
    for (int i = t; i < 768; i += 256) lut[i] = a.lut[i];
    __syncthreads();
    const double* Ap = a.inv + 6 * (size_t)b;
    const double A[6] = {Ap[0], Ap[1], Ap[2], Ap[3], Ap[4], Ap[5]};
    const uint8_t* img = a.src + a.offset[b];
    float* out = a.out + (size_t)b * 3 * a.H * a.W;
    if (mode == 1) fixed_rows<true>(a, lut, img, stride, src_h, src_w, A, out, row_first, rows);
    else fixed_rows<false>(a, lut, img, stride, src_h, src_w, A, out, row_first, rows);
}

}  // namespace

extern "C" int y2_fixed_images(const uint8_t* src, const int64_t* offset, const int32_t* geom, const double* inv, const float* lut,
                               int32_t B, int32_t H, int32_t W, int32_t flags, float* out, y2_stream_t stream) {
    if (B < 0 || H < 1 || H > Y2_WARP_MAX_DIM || W < 1 || W > Y2_WARP_MAX_DIM || (flags & ~1)) return Y2_EINVAL;
    if (B == 0) return Y2_OK;
    if (B > 65535) return Y2_ENOSUP;
    if (!src || !offset || !geom || !inv || !lut || !out) return Y2_EINVAL;
    FixedArgs a;
    a.src = src; a.offset = offset; a.geom = geom; a.inv = inv; a.lut = lut; a.out = out;
    a.H = H; a.W = W; a.swap = flags & 1;
    a.vec = (W % 4 == 0 && y2_aligned16(out)) ? 1 : 0;          // plane and row sizes are then multiples of 16 bytes too
    Y2_LAUNCH("fixed_images_kernel", 0.0, fixed_images_kernel, dim3(y2_cdiv(H, FX_ROWS), B), dim3(256), 0, y2_s(stream), a);
    Y2_LAUNCH_CHECK();
    return Y2_OK;
}
