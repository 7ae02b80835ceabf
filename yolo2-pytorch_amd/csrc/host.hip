// host.hip — HOST-memory entry points of libyolo2_hip.so (include/yolo2_hip.h: y2_nms_host, y2_iou_matrix_host, y2_iou_pair_host,
// y2_eval_match_host, y2_collate_images_host, y2_warp_affine_images_host, y2_collate_jitter_images_host, y2_jpeg_probe_host,
// y2_jpeg_workspace_bytes, y2_jpeg_decode_images_host, y2_anchor_kmeans_host, y2_anchor_assign_host, y2_fixed_images_host).
//
// The reference calls utils.postprocess.nms on CPU tensors from its summary worker process (train.py:209, a child forked
// after the GPU was initialised, which must never touch the device) and runs the utils.iou.torch unit tests on CPU tensors
// (utils/iou/torch.py:64-113).  These functions are the product's own host implementation of the SAME algorithms as the
// device kernels in detect.hip — rank by (score desc, index asc), L x L suppression bit matrix, serial greedy replay; the
// identical one-rounding-per-operation fp32 IoU sequence (this file is compiled with -ffp-contract=off like the rest) — so
// GPU and CPU callers get bit-identical keep lists.  No HIP call is made here: safe in a forked child.
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "yolo2_hip.h"
#include "resample.h"
#include "jpeg.h"
#include "kmeans.h"
#include "fixed.h"

namespace {

inline float iou_host(float ymin1, float xmin1, float ymax1, float xmax1, float ymin2, float xmin2, float ymax2, float xmax2, float min_union) {
    // utils/iou/torch.py:34-61 (same operation order as common.h: iou_one)
    const float ih = fmaxf(fminf(ymax1, ymax2) - fmaxf(ymin1, ymin2), 0.f);
    const float iw = fmaxf(fminf(xmax1, xmax2) - fmaxf(xmin1, xmin2), 0.f);
    const float inter = ih * iw;
    const float a1 = (ymax1 - ymin1) * (xmax1 - xmin1);
    const float a2 = (ymax2 - ymin2) * (xmax2 - xmin2);
    const float uni = fmaxf((a1 + a2) - inter, min_union);
    return inter / uni;
}

inline float nms_key(float s) { return s != s ? -INFINITY : s; }   // NaN ranks last (detect.hip: nms_key)

// warp.hip: wp_round, wp_clamp16 (rint rounds to nearest even in the default rounding mode, which nothing here changes)
inline long long warp_round(double v) { return (long long)(int)fmin(fmax(rint(v), -2147483648.0), 2147483647.0); }
inline int warp_clamp16(long long v) { return (int)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }

}  // namespace

extern "C" int y2_nms_host(const float* score, const float* yx_min, const float* yx_max, const int32_t* cand, const int32_t* n, int B, int stride,
                           float overlap, int limit, int32_t* keep, int32_t* keep_count) {
    if (!score || !yx_min || !yx_max || !n || !keep || !keep_count) return Y2_EINVAL;
    if (B <= 0 || stride <= 0 || limit <= 0 || limit > 1024) return Y2_EINVAL;
    std::vector<int32_t> order;
    std::vector<float> key, box;
    for (int b = 0; b < B; ++b) {
        const int nb = n[b];
        if (nb < 0 || nb > stride) return Y2_EINVAL;
        const float* s = score + (size_t)b * stride;
        const int32_t* cd = cand ? cand + (size_t)b * stride : nullptr;
        int32_t* kp = keep + (size_t)b * limit;
        // stage 1 (utils/postprocess.py:37-38): the first `limit` of the descending order; ties -> lower index first
        key.resize((size_t)nb);
        order.resize((size_t)nb);
        for (int i = 0; i < nb; ++i) { key[(size_t)i] = nms_key(s[cd ? cd[i] : i]); order[(size_t)i] = i; }
        const int L = nb < limit ? nb : limit;
        std::partial_sort(order.begin(), order.begin() + L, order.end(), [&](int32_t a, int32_t c) {
            const float ka = key[(size_t)a], kc = key[(size_t)c];
            return ka > kc || (ka == kc && a < c);
        });
        // stage 2 (utils/postprocess.py:39-48): the serial greedy loop on a "removed" bit set; row i of the device kernel's
        // suppression matrix is evaluated only when i is kept (the rows of removed boxes are never used there either)
        const int words = (L + 63) >> 6;
        box.resize((size_t)L * 4);
        for (int r = 0; r < L; ++r) {
            const int i = order[(size_t)r];
            const size_t g = ((size_t)b * stride + (size_t)(cd ? cd[i] : i)) * 2;
            box[4 * (size_t)r] = yx_min[g]; box[4 * (size_t)r + 1] = yx_min[g + 1];
            box[4 * (size_t)r + 2] = yx_max[g]; box[4 * (size_t)r + 3] = yx_max[g + 1];
        }
        std::vector<uint64_t> removed((size_t)words, 0ull);
        int kept = 0;
        for (int i = 0; i < L; ++i) {
            if ((removed[(size_t)(i >> 6)] >> (i & 63)) & 1ull) continue;
            kp[kept++] = order[(size_t)i];
            const float y0 = box[4 * (size_t)i], x0 = box[4 * (size_t)i + 1], y1 = box[4 * (size_t)i + 2], x1 = box[4 * (size_t)i + 3];
            for (int j = i + 1; j < L; ++j) {
                const float v = iou_host(y0, x0, y1, x1, box[4 * (size_t)j], box[4 * (size_t)j + 1], box[4 * (size_t)j + 2], box[4 * (size_t)j + 3], 1.1920929e-07f);
                if (!(v <= overlap)) removed[(size_t)(j >> 6)] |= 1ull << (j & 63);     // kept iff iou <= overlap (utils/postprocess.py:48)
            }
        }
        keep_count[b] = kept;
    }
    return Y2_OK;
}

extern "C" int y2_iou_matrix_host(const float* mn1, const float* mx1, const float* mn2, const float* mx2,
                                  int Bt, int N1, int N2, float min_union, int mode, float* out) {
    if (Bt < 0 || N1 < 0 || N2 < 0 || (mode != 0 && mode != 1)) return Y2_EINVAL;
    if ((long long)Bt * N1 * N2 == 0) return Y2_OK;
    if (!mn1 || !mx1 || !mn2 || !mx2 || !out) return Y2_EINVAL;
    for (int b = 0; b < Bt; ++b)
        for (int i = 0; i < N1; ++i) {
            const size_t r = ((size_t)b * N1 + i) * 2;
            for (int j = 0; j < N2; ++j) {
                const size_t c = ((size_t)b * N2 + j) * 2;
                float v;
                if (mode == 0) {
                    v = iou_host(mn1[r], mn1[r + 1], mx1[r], mx1[r + 1], mn2[c], mn2[c + 1], mx2[c], mx2[c + 1], min_union);
                } else {
                    const float ih = fmaxf(fminf(mx1[r], mx2[c]) - fmaxf(mn1[r], mn2[c]), 0.f);
                    const float iw = fmaxf(fminf(mx1[r + 1], mx2[c + 1]) - fmaxf(mn1[r + 1], mn2[c + 1]), 0.f);
                    v = ih * iw;
                }
                out[((size_t)b * N1 + i) * N2 + j] = v;
            }
        }
    return Y2_OK;
}

extern "C" int y2_iou_pair_host(const float* mn1, const float* mx1, const float* mn2, const float* mx2, int n, float min_union, float* out) {
    if (n < 0) return Y2_EINVAL;
    if (n == 0) return Y2_OK;
    if (!mn1 || !mx1 || !mn2 || !mx2 || !out) return Y2_EINVAL;
    for (int i = 0; i < n; ++i)
        out[i] = iou_host(mn1[2 * i], mn1[2 * i + 1], mx1[2 * i], mx1[2 * i + 1], mn2[2 * i], mn2[2 * i + 1], mx2[2 * i], mx2[2 * i + 1], min_union);
    return Y2_OK;
}

// eval.py:278-292 for a batch (evalmatch.hip: eval_match_kernel, serially): per image the valid boxes are counted per class, every participating row takes
// its best valid same-class box (first maximum) and the EARLIEST positive row per box is the true positive.
extern "C" int y2_eval_match_host(const float* det_min, const float* det_max, const long long* det_cls, const int32_t* det_count,
                                  const float* gt_min, const float* gt_max, const long long* gt_cls, const uint8_t* gt_difficult,
                                  int B, int M, int G, int C, float threshold, float min_union, uint8_t* tp, int32_t* cls_num) {
    if (B <= 0 || M < 0 || G < 0 || C <= 0 || !det_count || !cls_num) return Y2_EINVAL;
    if (M > 0 && (!det_min || !det_max || !det_cls || !tp)) return Y2_EINVAL;
    if (G > 0 && (!gt_min || !gt_max || !gt_cls || !gt_difficult)) return Y2_EINVAL;
    if (G > Y2_EVAL_MATCH_MAX_G) return Y2_ENOSUP;
    std::vector<uint8_t> valid((size_t)G), claimed((size_t)G);
    for (int b = 0; b < B; ++b) {
        const size_t g0 = (size_t)b * G, d0 = (size_t)b * M;
        for (int g = 0; g < G; ++g) {
            const size_t o = g0 + g;
            const bool v = gt_min[2 * o] < gt_max[2 * o] && gt_min[2 * o + 1] < gt_max[2 * o + 1] && gt_difficult[o] < 1;
            valid[(size_t)g] = v;
            claimed[(size_t)g] = 0;
            const long long c = gt_cls[o];
            if (v && c >= 0 && c < C) cls_num[c] += 1;
        }
        int count = det_count[b];
        count = count < 0 ? 0 : (count > M ? M : count);
        for (int i = 0; i < M; ++i) {
            const size_t o = d0 + i;
            tp[o] = 0;
            if (i >= count) continue;
            const long long c = det_cls[o];
            float bv = 0.f;
            int bi = -1;
            for (int g = 0; g < G; ++g) {
                if (!valid[(size_t)g] || gt_cls[g0 + g] != c) continue;
                const size_t q = g0 + g;
                const float v = iou_host(det_min[2 * o], det_min[2 * o + 1], det_max[2 * o], det_max[2 * o + 1],
                                         gt_min[2 * q], gt_min[2 * q + 1], gt_max[2 * q], gt_max[2 * q + 1], min_union);
                if (bi < 0 || v > bv) { bv = v; bi = g; }
            }
            if (bi >= 0 && bv > threshold && !claimed[(size_t)bi]) {        // rows in ascending order: the first positive row of a box claims it
                claimed[(size_t)bi] = 1;
                tp[o] = 1;
            }
        }
    }
    return Y2_OK;
}

// y2_collate_images on host memory (collate.hip: collate_images_kernel, serially).  The tables are readable here, so they are checked before
// anything is written: a window outside its image is Y2_EINVAL.
extern "C" int y2_collate_images_host(const uint8_t* src, const int64_t* offset, const int32_t* geom, const float* lut,
                                      int32_t B, int32_t H, int32_t W, int32_t flags, float* out) {
    if (B < 0 || H <= 0 || W <= 0 || W > Y2_COLLATE_MAX_W || (flags & ~1)) return Y2_EINVAL;
    if (B == 0) return Y2_OK;
    if (B > 65535) return Y2_ENOSUP;
    if (!src || !offset || !geom || !lut || !out) return Y2_EINVAL;
    for (int b = 0; b < B; ++b) {
        const int32_t* g = geom + 8 * (size_t)b;
        const long long stride = g[0], src_h = g[1], src_w = g[2], wy0 = g[3], wx0 = g[4], wh = g[5], ww = g[6];
        if (offset[b] < 0 || src_h < 1 || src_w < 1 || stride < 3 * src_w || wh < 1 || ww < 1 || wy0 < 0 || wx0 < 0 || wy0 + wh > src_h || wx0 + ww > src_w
            || (g[7] != 0 && g[7] != 1))
            return Y2_EINVAL;
    }
    const int cs = (flags & 1) ? 2 : 0;
    const size_t plane = (size_t)H * W;
    std::vector<int> off0((size_t)W), off1((size_t)W), xc((size_t)W);
    for (int b = 0; b < B; ++b) {
        const int32_t* g = geom + 8 * (size_t)b;
        const int stride = g[0], src_h = g[1], src_w = g[2], wy0 = g[3], wx0 = g[4], wh = g[5], ww = g[6], flip = g[7];
        const bool box = wh == 2 * H && ww == 2 * W;
        for (int x = 0; x < W; ++x) cl_col(x, box, ww, W, wx0, flip, src_w, off0[(size_t)x], off1[(size_t)x], xc[(size_t)x]);
        const uint8_t* img = src + offset[b];
        float* o = out + (size_t)b * 3 * plane;
        for (int y = 0; y < H; ++y) {
            int r0, r1, yc;
            cl_row(y, box, wh, H, wy0, src_h, r0, r1, yc);
            const uint8_t* p0 = img + (long long)r0 * stride;
            const uint8_t* p1 = img + (long long)r1 * stride;
            for (int c = 0; c < 3; ++c) {
                const int ch = c == 1 ? 1 : c ^ cs;
                float* row = o + c * plane + (size_t)y * W;
                for (int x = 0; x < W; ++x)
                    row[x] = lut[c * 256 + cl_level(box, p0, p1, off0[(size_t)x] + ch, off1[(size_t)x] + ch, xc[(size_t)x], yc & 0xffff, yc >> 16)];
            }
        }
    }
    return Y2_OK;
}

// y2_warp_affine_images on host memory (warp.hip: warp_affine_images_kernel, serially).  The tables are readable here, so they are checked before
// anything is written.
extern "C" int y2_warp_affine_images_host(const uint8_t* src, const int64_t* src_offset, const int32_t* src_geom, const double* inv,
                                          uint8_t* dst, const int64_t* dst_offset, const int32_t* dst_geom,
                                          int32_t B, int32_t max_h, int32_t max_w, int32_t fill) {
    if (B < 0 || max_h < 1 || max_h > Y2_WARP_MAX_DIM || max_w < 1 || max_w > Y2_WARP_MAX_DIM || (fill & ~0xffffff)) return Y2_EINVAL;
    if (B == 0) return Y2_OK;
    if (B > 65535) return Y2_ENOSUP;
    if (!src || !src_offset || !src_geom || !inv || !dst || !dst_offset || !dst_geom) return Y2_EINVAL;
    for (int b = 0; b < B; ++b) {
        const int32_t* sg = src_geom + 4 * (size_t)b;
        const int32_t* dg = dst_geom + 8 * (size_t)b;
        const double* A = inv + 6 * (size_t)b;
        if (src_offset[b] < 0 || sg[1] < 1 || sg[1] > Y2_WARP_MAX_DIM || sg[2] < 1 || sg[2] > Y2_WARP_MAX_DIM || sg[0] < 3 * sg[2] || (sg[3] != 0 && sg[3] != 1))
            return Y2_EINVAL;
        if (dst_offset[b] < 0 || dg[1] < 1 || dg[1] > max_h || dg[2] < 1 || dg[2] > max_w || dg[0] < 3 * dg[2]) return Y2_EINVAL;
        // (negated comparisons: a NaN is refused)
        if (!(fabs(A[0]) <= 4.0 && fabs(A[1]) <= 4.0 && fabs(A[3]) <= 4.0 && fabs(A[4]) <= 4.0 && fabs(A[2]) <= 524288.0 && fabs(A[5]) <= 524288.0))
            return Y2_EINVAL;
    }
    for (int b = 0; b < B; ++b) {
        const int32_t* sg = src_geom + 4 * (size_t)b;
        const int32_t* dg = dst_geom + 8 * (size_t)b;
        const int stride = sg[0], src_h = sg[1], src_w = sg[2], flip = sg[3], dstride = dg[0], dst_h = dg[1], dst_w = dg[2];
        const double* A = inv + 6 * (size_t)b;
        const uint8_t* img = src + src_offset[b];
        for (int y = 0; y < dst_h; ++y) {
            const long long X0 = warp_round((A[1] * (double)y + A[2]) * 1024.0) + 16, Y0 = warp_round((A[4] * (double)y + A[5]) * 1024.0) + 16;
            uint8_t* o = dst + dst_offset[b] + (long long)y * dstride;
            for (int x = 0; x < dst_w; ++x) {
                const long long X = (X0 + warp_round((A[0] * (double)x) * 1024.0)) >> 5, Y = (Y0 + warp_round((A[3] * (double)x) * 1024.0)) >> 5;
                const int sx = warp_clamp16(X >> 5), sy = warp_clamp16(Y >> 5), ax = (int)(X & 31), ay = (int)(Y & 31);
                const int w00 = (32 - ax) * (32 - ay), w01 = ax * (32 - ay), w10 = (32 - ax) * ay, w11 = ax * ay;
                const bool x0 = sx >= 0 && sx < src_w, x1 = sx + 1 >= 0 && sx + 1 < src_w, y0 = sy >= 0 && sy < src_h, y1 = sy + 1 >= 0 && sy + 1 < src_h;
                const long long c0 = 3LL * (flip ? src_w - 1 - sx : sx), c1 = 3LL * (flip ? src_w - 2 - sx : sx + 1);
                const long long r0 = (long long)sy * stride, r1 = r0 + stride;          // (offsets, not pointers: a tap outside the image is never formed)
                for (int c = 0; c < 3; ++c) {
                    const int f = (fill >> (8 * c)) & 255;
                    const int p00 = (y0 && x0) ? (int)img[r0 + c0 + c] : f, p01 = (y0 && x1) ? (int)img[r0 + c1 + c] : f;
                    const int p10 = (y1 && x0) ? (int)img[r1 + c0 + c] : f, p11 = (y1 && x1) ? (int)img[r1 + c1 + c] : f;
                    o[3 * x + c] = (uint8_t)((p00 * w00 + p01 * w01 + p10 * w10 + p11 * w11 + 512) >> 10);
                }
            }
        }
    }
    return Y2_OK;
}

// y2_fixed_images on host memory: csrc/fixed.h's fx_images_host (the table checks, then fixed.hip's kernel serially, the same arithmetic).
static_assert(Y2_WARP_MAX_DIM == FX_MAX_DIM && Y2_OK == 0 && Y2_EINVAL == -1 && Y2_ENOSUP == -3, "include/yolo2_hip.h and csrc/fixed.h disagree");

extern "C" int y2_fixed_images_host(const uint8_t* src, const int64_t* offset, const int32_t* geom, const double* inv, const float* lut,
                                    int32_t B, int32_t H, int32_t W, int32_t flags, float* out) {
    return fx_images_host(src, offset, geom, inv, lut, B, H, W, flags, out);
}

// y2_collate_jitter_images on host memory (jitter.hip: collate_jitter_images_kernel, image by image instead of tile by tile).  The tables are readable
// here, so they are checked before anything is written.
extern "C" int y2_collate_jitter_images_host(const uint8_t* src, const int64_t* offset, const int32_t* geom, const int32_t* jitter, const uint8_t* hsv_tab,
                                             const float* lut, int32_t B, int32_t H, int32_t W, int32_t flags, float* out) {
    if (B < 0 || H <= 0 || W <= 0 || W > Y2_COLLATE_MAX_W || (flags & ~1)) return Y2_EINVAL;
    if (B == 0) return Y2_OK;
    if (B > 65535) return Y2_ENOSUP;
    if (!src || !offset || !geom || !jitter || !lut || !out) return Y2_EINVAL;
    for (int b = 0; b < B; ++b) {
        const int32_t* g = geom + 8 * (size_t)b;
        const int32_t* jt = jitter + 4 * (size_t)b;
        const long long stride = g[0], src_h = g[1], src_w = g[2], wy0 = g[3], wx0 = g[4], wh = g[5], ww = g[6];
        if (offset[b] < 0 || src_h < 1 || src_w < 1 || stride < 3 * src_w || wh < 1 || ww < 1 || wy0 < 0 || wx0 < 0 || wy0 + wh > src_h || wx0 + ww > src_w
            || (g[7] != 0 && g[7] != 1))
            return Y2_EINVAL;
        if (jt[0] < 1 || jt[0] > Y2_JITTER_MAX_BLUR || jt[1] < 1 || jt[1] > Y2_JITTER_MAX_BLUR || (jt[2] != 0 && jt[2] != 1) || jt[3] != 0 || (jt[2] && !hsv_tab))
            return Y2_EINVAL;
    }
    int sdiv[256], hdiv[256];
    for (int i = 0; i < 256; ++i) { sdiv[i] = jt_div(JT_SDIV_N, i); hdiv[i] = jt_div(JT_HDIV_N, i); }
    const size_t plane = (size_t)H * W;
    std::vector<int> off0((size_t)W), off1((size_t)W), xc((size_t)W), rx((size_t)W + Y2_JITTER_MAX_BLUR);
    std::vector<uint8_t> lv(plane * 3);          // the resized image [H][W][3], source channel order
    std::vector<int> rs(plane * 3);              // its row sums
    for (int b = 0; b < B; ++b) {
        const int32_t* g = geom + 8 * (size_t)b;
        const int32_t* jt = jitter + 4 * (size_t)b;
        const int stride = g[0], src_h = g[1], src_w = g[2], wy0 = g[3], wx0 = g[4], wh = g[5], ww = g[6], flip = g[7];
        const int kx = jt[0], ky = jt[1], hsv = jt[2];
        const bool box = wh == 2 * H && ww == 2 * W;
        for (int x = 0; x < W; ++x) cl_col(x, box, ww, W, wx0, flip, src_w, off0[(size_t)x], off1[(size_t)x], xc[(size_t)x]);
        const uint8_t* img = src + offset[b];
        for (int y = 0; y < H; ++y) {
            int r0, r1, yc;
            cl_row(y, box, wh, H, wy0, src_h, r0, r1, yc);
            const uint8_t* p0 = img + (long long)r0 * stride;
            const uint8_t* p1 = img + (long long)r1 * stride;
            for (int x = 0; x < W; ++x)
                for (int c = 0; c < 3; ++c)
                    lv[((size_t)y * W + x) * 3 + c] = (uint8_t)cl_level(box, p0, p1, off0[(size_t)x] + c, off1[(size_t)x] + c, xc[(size_t)x], yc & 0xffff, yc >> 16);
        }
        // the box filter: the window of column x is x - kx / 2 .. x - kx / 2 + kx - 1, reflected into the resized image; rows alike
        for (int i = 0; i < W + kx - 1; ++i) rx[(size_t)i] = jt_reflect101(i - kx / 2, W);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                for (int c = 0; c < 3; ++c) {
                    int s = 0;
                    for (int i = 0; i < kx; ++i) s += lv[((size_t)y * W + rx[(size_t)(x + i)]) * 3 + c];
                    rs[((size_t)y * W + x) * 3 + c] = s;
                }
        const double inv = 1.0 / (double)(kx * ky);
        const float* tab = lut + (size_t)b * 768;
        const uint8_t* ht = hsv ? hsv_tab + (size_t)b * 768 : nullptr;
        float* o = out + (size_t)b * 3 * plane;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                int lev[3];
                for (int c = 0; c < 3; ++c) {
                    int s = 0;
                    for (int j = 0; j < ky; ++j) s += rs[((size_t)jt_reflect101(y + j - ky / 2, H) * W + x) * 3 + c];
                    lev[c] = kx * ky > 1 ? jt_blur_level(s, inv) : s;
                }
                int p[3];          // the levels of the three output planes
                if (hsv) {
                    int h, s, v;
                    jt_bgr2hsv(lev[0], lev[1], lev[2], sdiv, hdiv, h, s, v);
                    jt_hsv2rgb(ht[h], ht[256 + s], ht[512 + v], p[0], p[1], p[2]);
                } else {
                    p[0] = (flags & 1) ? lev[2] : lev[0];
                    p[1] = lev[1];
                    p[2] = (flags & 1) ? lev[0] : lev[2];
                }
                for (int c = 0; c < 3; ++c) o[c * plane + (size_t)y * W + x] = tab[c * 256 + p[c]];
            }
    }
    return Y2_OK;
}

// ---- baseline JPEG (csrc/jpeg.h is the decoder; jpeg.hip runs the same functions on the device)

static_assert(Y2_JPEG_DESC_BYTES == JP_DESC_BYTES && Y2_JPEG_MAX_DIM == JP_MAX_DIM, "include/yolo2_hip.h and csrc/jpeg.h disagree");

extern "C" int y2_jpeg_probe_host(const uint8_t* data, int64_t nbytes, uint8_t* desc) {
    if (!desc) return Y2_EINVAL;
    JpDesc d;
    const int rc = jp_probe(data, nbytes, &d);
    if (rc != 0) memset(&d, 0, sizeof(d));          // a refused file leaves no half-filled record behind
    memcpy(desc, &d, sizeof(d));
    return rc;
}

extern "C" long long y2_jpeg_workspace_bytes(const uint8_t* desc, int32_t B) {
    if (B < 0 || (B > 0 && !desc)) return Y2_EINVAL;
    long long most = 0;
    for (int b = 0; b < B; ++b) {
        JpDesc d;
        memcpy(&d, desc + (size_t)b * JP_DESC_BYTES, sizeof(d));
        const JpLayout L = jp_layout(&d);
        if (!L.ok) return Y2_EINVAL;
        most = std::max(most, L.bytes);
    }
    return B * ((most + 15) & ~15LL);
}

// y2_jpeg_decode_images on host memory (jpeg.hip's three kernels, image by image).  The tables are readable here, so they are checked before anything
// is written.
extern "C" int y2_jpeg_decode_images_host(const uint8_t* src, int64_t src_bytes, const int64_t* src_offset, const uint8_t* desc,
                                          uint8_t* dst, int64_t dst_bytes, const int64_t* dst_offset, const int32_t* dst_geom,
                                          uint8_t* ws, int64_t ws_bytes, int32_t* status, int32_t B) {
    if (B < 0 || src_bytes < 0 || dst_bytes < 0 || ws_bytes < 0) return Y2_EINVAL;
    if (B == 0) return Y2_OK;
    if (B > 65535) return Y2_ENOSUP;
    if (!src || !src_offset || !desc || !dst || !dst_offset || !dst_geom || !ws || !status) return Y2_EINVAL;
    if ((reinterpret_cast<uintptr_t>(ws) & 15u) || (reinterpret_cast<uintptr_t>(desc) & 3u)) return Y2_EALIGN;
    const long long per_image = (ws_bytes / B) & ~15LL;
    for (int b = 0; b < B; ++b) {
        const JpLayout L = jp_layout(reinterpret_cast<const JpDesc*>(desc + (size_t)b * JP_DESC_BYTES));
        if (!jp_extents_ok(L, src_bytes, src_offset[b], dst_bytes, dst_offset[b], dst_geom + 8 * (size_t)b, per_image)) return Y2_EINVAL;
    }
    for (int b = 0; b < B; ++b) {
        const JpDesc* d = reinterpret_cast<const JpDesc*>(desc + (size_t)b * JP_DESC_BYTES);
        const JpLayout L = jp_layout(d);
        status[b] = jp_decode_image_host(d, L, src + src_offset[b] + L.scan_offset, ws + (size_t)b * per_image, dst + dst_offset[b], dst_geom[8 * (size_t)b]);
    }
    return Y2_OK;
}

// ---- anchors by k-means on 1 - IoU (csrc/kmeans.h is the arithmetic and the trial itself; kmeans.hip runs the same functions on the device)

static_assert(Y2_KMEANS_MAX_K == KM_MAX_K, "include/yolo2_hip.h and csrc/kmeans.h disagree");

extern "C" int y2_anchor_kmeans_host(const double* size, int32_t N, int32_t K, const int32_t* init, int32_t R, int32_t max_iter, double conv_test,
                                     double* means, int32_t* iters, int32_t* status, double* cost, int32_t* counts) {
    if (N <= 0 || K <= 0 || R <= 0 || max_iter <= 0) return Y2_EINVAL;
    if (!size || !init || !means || !iters || !status || !cost || !counts) return Y2_EINVAL;
    if (K > Y2_KMEANS_MAX_K || R > 65535) return Y2_ENOSUP;
    if ((reinterpret_cast<uintptr_t>(size) | reinterpret_cast<uintptr_t>(means) | reinterpret_cast<uintptr_t>(cost)) & 7u) return Y2_EALIGN;
    std::vector<double> part((size_t)(2 * K + 1) * KM_LANES);
    for (int r = 0; r < R; ++r)
        km_trial_host(size, N, K, init + (size_t)r * K, max_iter, conv_test, means + 2 * (size_t)r * K, iters + r, status + r, cost + r,
                      counts + (size_t)r * K, part.data());
    return Y2_OK;
}

extern "C" int y2_anchor_assign_host(const double* size, int32_t N, const double* means, int32_t K, int32_t* index, double* iou) {
    if (N <= 0 || K <= 0 || !size || !means) return Y2_EINVAL;
    if (K > Y2_KMEANS_MAX_K) return Y2_ENOSUP;
    if ((reinterpret_cast<uintptr_t>(size) | reinterpret_cast<uintptr_t>(means) | reinterpret_cast<uintptr_t>(iou)) & 7u) return Y2_EALIGN;
    km_assign_host(size, N, means, K, index, iou);
    return Y2_OK;
}
