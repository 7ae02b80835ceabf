// collate.hip — the collate step of the data pipeline (utils/data.py:114-133 with transform/resize/label.py:25-74, transform/augmentation.py:88-103,
// BGR2RGB, ToTensor, Normalize) for a whole batch in ONE launch: y2_collate_images (include/yolo2_hip.h).
//
// A ragged batch of uint8 HWC source images (one packed byte buffer, any byte alignment) becomes the network's fp32 [B][3][H][W] input: crop window,
// horizontal flip, 8-bit INTER_LINEAR resize (11-bit integer coefficients; the 2x2 box mean at exactly 2:1 on both axes), channel swap and a
// per-level table for ToTensor + Normalize.  Everything after the tap coefficients is integer arithmetic and the coefficients are exactly rounded
// IEEE operations (this file is compiled with -ffp-contract=off like the rest), so y2_collate_images_host (host.hip) is bit-identical.
//
// A streaming kernel: per output value 4 gathered source bytes (served by the caches: neighbouring outputs share taps) and one 4-byte store; the
// fp32 output is 4/3 .. 4x the bytes of the source, so the 16-byte stores are what has to be right.
#include "common.h"
#include "resample.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int CL_ROWS = 16;         // output rows per workgroup: 416x416 x 64 images -> 1664 workgroups, 6-7 items of 4 pixels per thread

struct CollateArgs {
    const uint8_t* src; const int64_t* offset; const int32_t* geom; const float* lut;
    float* out;
    int H, W, swap, vec;
};

// Workgroup (blockIdx.x, blockIdx.y) = (block of CL_ROWS output rows, image).  LDS: per output column the byte offsets of its two taps inside a source
// row and the packed coefficients (12 bytes per column), per output row of the block the two source rows and coefficients, and the level table.
// The column table depends only on x: it is built once per workgroup, then the threads walk the block's (row, 4-column group) items in row-major
// order, so a wave's lanes write consecutive 16-byte pieces of one plane row.
__global__ __launch_bounds__(256) void collate_images_kernel(const CollateArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cl_smem[];
    const int H = a.H, W = a.W;
    int* x_off0 = reinterpret_cast<int*>(cl_smem);       // [W] byte offset of tap 0 in a source row
    int* x_off1 = x_off0 + W;                            // [W]
    int* x_coef = x_off1 + W;                            // [W] c0 | c1 << 16
    int* y_row0 = x_coef + W;                            // [CL_ROWS] source row of tap 0
    int* y_row1 = y_row0 + CL_ROWS;
    int* y_coef = y_row1 + CL_ROWS;
    float* lut = reinterpret_cast<float*>(y_coef + CL_ROWS);      // [3][256]: the level table, staged once per workgroup
    const int b = blockIdx.y, t = threadIdx.x;
    const int32_t* g = a.geom + 8 * (size_t)b;
    const int stride = g[0], src_h = g[1], src_w = g[2], wy0 = g[3], wx0 = g[4], wh = g[5], ww = g[6], flip = g[7];
    if (src_h <= 0 || src_w <= 0 || wh <= 0 || ww <= 0) return;          // (uniform per workgroup; the wrappers refuse such a table)
    const bool box = wh == 2 * H && ww == 2 * W;
    const int row_first = blockIdx.x * CL_ROWS;
    const int rows = min(CL_ROWS, H - row_first);
    for (int x = t; x < W; x += 256) {
        cl_col(x, box, ww, W, wx0, flip, src_w, x_off0[x], x_off1[x], x_coef[x]);
    }
    for (int r = t; r < rows; r += 256) {
        cl_row(row_first + r, box, wh, H, wy0, src_h, y_row0[r], y_row1[r], y_coef[r]);
    }
    for (int i = t; i < 768; i += 256) lut[i] = a.lut[i];
    __syncthreads();
    const uint8_t* img = a.src + a.offset[b];
    const size_t plane = (size_t)H * W;
    float* out = a.out + (size_t)b * 3 * plane;
    const int cs = a.swap ? 2 : 0;          // output plane c reads source channel c ^ cs for c in {0, 2}; channel 1 stays
    if (a.vec) {
        // W % 4 == 0: the three column tables start on 16-byte boundaries and a lane's 4 columns are ONE 16-byte LDS read per table (a wave reads
        // 1 KB of consecutive addresses: no bank conflict; four 4-byte reads per lane at a stride of 16 bytes would be 4-way conflicts)
        const int Q = W >> 2;
        for (int item = t; item < rows * Q; item += 256) {
            const int r = item / Q, x = (item - r * Q) << 2;
            const uint8_t* p0 = img + (long long)y_row0[r] * stride;
            const uint8_t* p1 = img + (long long)y_row1[r] * stride;
            const int yc = y_coef[r], b0 = yc & 0xffff, b1 = yc >> 16;
            const i32x4 o0 = *reinterpret_cast<const i32x4*>(x_off0 + x), o1 = *reinterpret_cast<const i32x4*>(x_off1 + x);
            const i32x4 xc = *reinterpret_cast<const i32x4*>(x_coef + x);
            float* o = out + (size_t)(row_first + r) * W + x;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int ch = c == 1 ? 1 : c ^ cs;
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = lut[c * 256 + cl_level(box, p0, p1, o0[j] + ch, o1[j] + ch, xc[j], b0, b1)];
                *reinterpret_cast<f32x4*>(o + c * plane) = v;
            }
        }
    } else {
        for (int item = t; item < rows * W; item += 256) {
            const int r = item / W, x = item - r * W;
            const uint8_t* p0 = img + (long long)y_row0[r] * stride;
            const uint8_t* p1 = img + (long long)y_row1[r] * stride;
            const int yc = y_coef[r], b0 = yc & 0xffff, b1 = yc >> 16;
            float* o = out + (size_t)(row_first + r) * W + x;
            const int o0 = x_off0[x], o1 = x_off1[x], xc = x_coef[x];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int ch = c == 1 ? 1 : c ^ cs;
                o[c * plane] = lut[c * 256 + cl_level(box, p0, p1, o0 + ch, o1 + ch, xc, b0, b1)];
            }
        }
    }
}

}  // namespace

extern "C" int y2_collate_images(const uint8_t* src, const int64_t* offset, const int32_t* geom, const float* lut,
                                 int32_t B, int32_t H, int32_t W, int32_t flags, float* out, y2_stream_t stream) {
    if (B < 0 || H <= 0 || W <= 0 || W > Y2_COLLATE_MAX_W || (flags & ~1)) return Y2_EINVAL;
    if (B == 0) return Y2_OK;
    if (B > 65535) return Y2_ENOSUP;
    if (!src || !offset || !geom || !lut || !out) return Y2_EINVAL;
    CollateArgs a;
    a.src = src; a.offset = offset; a.geom = geom; a.lut = lut; a.out = out;
    a.H = H; a.W = W; a.swap = flags & 1;
    a.vec = (W % 4 == 0 && y2_aligned16(out)) ? 1 : 0;          // plane and row sizes are then multiples of 16 bytes too
    const size_t lds = (size_t)(3 * W + 3 * CL_ROWS) * 4 + 768 * 4;
    Y2_LAUNCH("collate_images_kernel", 0.0, collate_images_kernel, dim3(y2_cdiv(H, CL_ROWS), B), dim3(256), lds, y2_s(stream), a);
    Y2_LAUNCH_CHECK();
    return Y2_OK;
}
