// fixed.h — the per-pixel arithmetic of y2_fixed_images, ONE copy for the device kernel (fixed.hip) and the host function (host.hip): the coordinates
// of cv2.warpAffine for 8-bit images, its INTER_LINEAR level (the formula of y2_warp_affine_images) and its INTER_CUBIC level (fp32 Keys coefficients,
// A = -0.75, a 4 x 4 table of 15-bit integer weights whose sum is corrected to 32768).  The recipe is stated in include/yolo2_hip.h.  Only exactly
// rounded IEEE operations and integer arithmetic (every file that includes this is compiled with -ffp-contract=off): device and host give the same bits.
//
// Safety: every load goes to a position clamped into the image the caller names (src_h, src_w >= 1 is the caller's to check); a tap outside the image
// contributes nothing because its weight, not its address, is dropped.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef Y2_HD
#define Y2_HD __host__ __device__ inline
#endif

#define FX_MAX_DIM 16384          // Y2_WARP_MAX_DIM

// rint to an int32 through a saturating clamp: a table nobody could check (NaN, infinities, huge entries) still gives a defined value
Y2_HD long long fx_round(double v) { return (long long)(int)fmin(fmax(rint(v), -2147483648.0), 2147483647.0); }
Y2_HD int fx_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
Y2_HD int fx_clamp16(long long v) { return (int)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }

// The row terms of destination row y and the source position of destination pixel (x, y) in 1/32 pixel (sx = X >> 5, ax = X & 31).
Y2_HD void fx_row(const double* A, int y, long long& X0, long long& Y0) {
    X0 = fx_round((A[1] * (double)y + A[2]) * 1024.0) + 16;
    Y0 = fx_round((A[4] * (double)y + A[5]) * 1024.0) + 16;
}
Y2_HD void fx_position(const double* A, int x, long long X0, long long Y0, long long& X, long long& Y) {
    const double xd = (double)x;
    X = (X0 + fx_round((A[0] * xd) * 1024.0)) >> 5;
    Y = (Y0 + fx_round((A[3] * xd) * 1024.0)) >> 5;
}

// Mode 0: the three levels of one destination pixel, packed l0 | l1 << 8 | l2 << 16 in source channel order.  The bilinear formula of
// y2_warp_affine_images with fill 0 and no flip.
Y2_HD unsigned fx_linear(const uint8_t* img, int stride, int src_h, int src_w, long long X, long long Y) {
    const int sx = fx_clamp16(X >> 5), sy = fx_clamp16(Y >> 5);
    const int ax = (int)(X & 31), ay = (int)(Y & 31);
    const bool x0 = sx >= 0 && sx < src_w, x1 = sx + 1 >= 0 && sx + 1 < src_w;
    const bool y0 = sy >= 0 && sy < src_h, y1 = sy + 1 >= 0 && sy + 1 < src_h;
    const int w00 = (y0 && x0) ? (32 - ax) * (32 - ay) : 0, w01 = (y0 && x1) ? ax * (32 - ay) : 0;
    const int w10 = (y1 && x0) ? (32 - ax) * ay : 0, w11 = (y1 && x1) ? ax * ay : 0;
    const int c0 = 3 * fx_clamp(sx, 0, src_w - 1), c1 = 3 * fx_clamp(sx + 1, 0, src_w - 1);
    const uint8_t* r0 = img + (long long)fx_clamp(sy, 0, src_h - 1) * stride;
    const uint8_t* r1 = img + (long long)fx_clamp(sy + 1, 0, src_h - 1) * stride;
    unsigned out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        out |= (unsigned)(((int)r0[c0 + c] * w00 + (int)r0[c1 + c] * w01 + (int)r1[c0 + c] * w10 + (int)r1[c1 + c] * w11 + 512) >> 10) << (8 * c);
    return out;
}

// The four cubic coefficients of the fraction a / 32 (taps at -1, 0, +1, +2), fp32, every operation rounded separately.
Y2_HD void fx_cubic_coeffs(int a, float* c) {
    const float A = -0.75f;
    const float t = (float)a * (1.f / 32.f);
    const float u = t + 1.f, v = 1.f - t;
    c[0] = ((A * u - 5.f * A) * u + 8.f * A) * u - 4.f * A;
    c[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
    c[2] = ((A + 2.f) * v - (A + 3.f)) * v * v + 1.f;
    c[3] = 1.f - c[0] - c[1] - c[2];
}

// The 4 x 4 integer weights of the fractions (ax / 32, ay / 32), w[4 * i + j] for row sy - 1 + i and column sx - 1 + j: each product rounded to
// int16 with saturation, then the difference of their sum to 32768 taken out of one of the four central weights (the scan of the header).  The
// corrected weight is kept as an int: (0, 0) gives 32768 in the centre, an exact copy.
Y2_HD void fx_cubic_weights(int ax, int ay, int* w) {
    float cx[4], cy[4];
    fx_cubic_coeffs(ax, cx);
    fx_cubic_coeffs(ay, cy);
    int sum = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float r = rintf((cy[i] * cx[j]) * 32768.f);
            const int q = (int)fminf(fmaxf(r, -32768.f), 32767.f);
            w[4 * i + j] = q;
            sum += q;
        }
    }
    const int d = sum - 32768;
    const int w5 = w[5], w6 = w[6], w9 = w[9], w10 = w[10];
    // min = max = [1][1]; [1][2], [2][1], [2][2] in turn: strictly below the minimum -> the minimum, else strictly above the maximum -> the maximum
    int lo = 5, hi = 5, vlo = w5, vhi = w5;
    if (w6 < vlo) { lo = 6; vlo = w6; } else if (w6 > vhi) { hi = 6; vhi = w6; }
    if (w9 < vlo) { lo = 9; vlo = w9; } else if (w9 > vhi) { hi = 9; vhi = w9; }
    if (w10 < vlo) { lo = 10; vlo = w10; } else if (w10 > vhi) { hi = 10; vhi = w10; }
    const int at = d < 0 ? hi : lo;          // (d == 0: nothing changes)
    // selects, not an indexed store: the weights stay in registers on the device
    w[5] = at == 5 ? w5 - d : w5;
    w[6] = at == 6 ? w6 - d : w6;
    w[9] = at == 9 ? w9 - d : w9;
    w[10] = at == 10 ? w10 - d : w10;
}

// Mode 1: the three levels of one destination pixel, packed as fx_linear packs them.
Y2_HD unsigned fx_cubic(const uint8_t* img, int stride, int src_h, int src_w, long long X, long long Y) {
    const int sx = fx_clamp16(X >> 5), sy = fx_clamp16(Y >> 5);
    int w[16];
    fx_cubic_weights((int)(X & 31), (int)(Y & 31), w);
    int col[4];
    bool cin[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = sx - 1 + j;
        cin[j] = x >= 0 && x < src_w;
        col[j] = 3 * fx_clamp(x, 0, src_w - 1);
    }
    int acc0 = 0, acc1 = 0, acc2 = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int y = sy - 1 + i;
        const bool rin = y >= 0 && y < src_h;
        const uint8_t* r = img + (long long)fx_clamp(y, 0, src_h - 1) * stride;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int wt = (rin && cin[j]) ? w[4 * i + j] : 0;
            acc0 += (int)r[col[j]] * wt;
            acc1 += (int)r[col[j] + 1] * wt;
            acc2 += (int)r[col[j] + 2] * wt;
        }
    }
    const unsigned l0 = (unsigned)fx_clamp((acc0 + 16384) >> 15, 0, 255), l1 = (unsigned)fx_clamp((acc1 + 16384) >> 15, 0, 255);
    const unsigned l2 = (unsigned)fx_clamp((acc2 + 16384) >> 15, 0, 255);
    return l0 | (l1 << 8) | (l2 << 16);
}

// A geometry row and an inverse matrix the host function accepts: what it (and utils.data.check_fixed) refuse otherwise.  (A NaN fails every
// comparison and is refused.)
inline bool fx_tables_ok(long long offset, const int32_t* g, const double* A) {
    if (offset < 0 || g[1] < 1 || g[1] > FX_MAX_DIM || g[2] < 1 || g[2] > FX_MAX_DIM || (long long)g[0] < 3LL * g[2] || (g[3] != 0 && g[3] != 1)) return false;
    return fabs(A[0]) <= 4.0 && fabs(A[1]) <= 4.0 && fabs(A[3]) <= 4.0 && fabs(A[4]) <= 4.0 && fabs(A[2]) <= 524288.0 && fabs(A[5]) <= 524288.0;
}

// The whole of y2_fixed_images_host (host.hip wraps it; tools/fixed_host_check.cpp drives it under the sanitizers): the argument and table checks,
// then fixed.hip's kernel serially.  Returns Y2_OK (0), Y2_EINVAL (-1: nothing is written) or Y2_ENOSUP (-3).  Beyond what it checks, the caller
// answers for the extent of the buffers: image b occupies offset[b] .. offset[b] + (src_h - 1) * row_stride_bytes + 3 * src_w of src.
inline int fx_images_host(const uint8_t* src, const int64_t* offset, const int32_t* geom, const double* inv, const float* lut,
                          int32_t B, int32_t H, int32_t W, int32_t flags, float* out) {
    if (B < 0 || H < 1 || H > FX_MAX_DIM || W < 1 || W > FX_MAX_DIM || (flags & ~1)) return -1;
    if (B == 0) return 0;
    if (B > 65535) return -3;
    if (!src || !offset || !geom || !inv || !lut || !out) return -1;
    for (int b = 0; b < B; ++b)
        if (!fx_tables_ok(offset[b], geom + 4 * (size_t)b, inv + 6 * (size_t)b)) return -1;
    const int cs = (flags & 1) ? 2 : 0;
    const size_t plane = (size_t)H * W;
    for (int b = 0; b < B; ++b) {
        const int32_t* g = geom + 4 * (size_t)b;
        const int stride = g[0], src_h = g[1], src_w = g[2], mode = g[3];
        const double* A = inv + 6 * (size_t)b;
        const uint8_t* img = src + offset[b];
        float* o = out + (size_t)b * 3 * plane;
        for (int y = 0; y < H; ++y) {
            long long X0, Y0;
            fx_row(A, y, X0, Y0);
            for (int x = 0; x < W; ++x) {
                long long X, Y;
                fx_position(A, x, X0, Y0, X, Y);
                const unsigned px = mode == 1 ? fx_cubic(img, stride, src_h, src_w, X, Y) : fx_linear(img, stride, src_h, src_w, X, Y);
                for (int c = 0; c < 3; ++c) o[c * plane + (size_t)y * W + x] = lut[c * 256 + ((px >> (8 * (c == 1 ? 1 : c ^ cs))) & 255)];
            }
        }
    }
    return 0;
}
