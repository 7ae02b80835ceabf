// resample.h — the per-pixel arithmetic of the collate step, ONE copy for the device kernels (collate.hip, jitter.hip) and the host functions
// (host.hip): the 8-bit INTER_LINEAR resize of y2_collate_images (taps, 11-bit coefficients, the 2x2 box mean, the window / flip / clamp rules) and
// the stages y2_collate_jitter_images puts behind it (BORDER_REFLECT_101, the box filter's rounding, 8-bit BGR2HSV and HSV2RGB).
// The recipes are stated in include/yolo2_hip.h.  Only exactly rounded IEEE operations and integer arithmetic (every file that includes this is
// compiled with -ffp-contract=off): device and host give the same bits.
#pragma once
#include <math.h>
#include <stdint.h>

#define Y2_HD __host__ __device__ inline

// Tap k (first of two; the second is k + 1, both clamped by the caller) and 11-bit coefficients of destination index i on an axis that maps a window
// of s source pixels to d destination pixels.  `edge`: the horizontal axis pins k to the window and zeroes the fraction there; the vertical axis only
// clamps its taps (the two coefficients always sum to 2048, so equal taps give the pixel back).
Y2_HD void cl_axis(int i, int s, int d, bool edge, int& k, int& c0, int& c1) {
    const double scale = (double)s / (double)d;
    float f = (float)(((double)i + 0.5) * scale - 0.5);
    const float fl = floorf(f);
    k = (int)fl;
    f -= fl;
    if (edge) {
        if (k < 0) { k = 0; f = 0.f; }
        if (k >= s - 1) { k = s - 1; f = 0.f; }
    }
    c1 = (int)rintf(f * 2048.f);
    c0 = (int)rintf((1.f - f) * 2048.f);
}

Y2_HD int cl_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Output column x of W reading the window [wx0, wx0 + ww) of a src_w wide image (the frame after the optional flip): the byte offsets of its two taps
// inside a source row and the packed coefficients c0 | c1 << 16.  `box`: the 2:1 box mean (taps 2x and 2x + 1, no coefficients).
// A window inside the image never moves in the last clamp: whatever the table says, no tap leaves the image it names.
Y2_HD void cl_col(int x, bool box, int ww, int W, int wx0, int flip, int src_w, int& off0, int& off1, int& coef) {
    int k, c0, c1;
    if (box) { k = 2 * x; c0 = c1 = 0; }
    else cl_axis(x, ww, W, true, k, c0, c1);
    int s0 = wx0 + cl_clamp(k, 0, ww - 1), s1 = wx0 + cl_clamp(k + 1, 0, ww - 1);
    if (flip) { s0 = src_w - 1 - s0; s1 = src_w - 1 - s1; }
    off0 = 3 * cl_clamp(s0, 0, src_w - 1);
    off1 = 3 * cl_clamp(s1, 0, src_w - 1);
    coef = c0 | (c1 << 16);
}

// Output row y of H reading the window [wy0, wy0 + wh) of a src_h high image: its two source rows and the packed coefficients.
Y2_HD void cl_row(int y, bool box, int wh, int H, int wy0, int src_h, int& row0, int& row1, int& coef) {
    int k, c0, c1;
    if (box) { k = 2 * y; c0 = c1 = 0; }
    else cl_axis(y, wh, H, false, k, c0, c1);
    row0 = cl_clamp(wy0 + cl_clamp(k, 0, wh - 1), 0, src_h - 1);
    row1 = cl_clamp(wy0 + cl_clamp(k + 1, 0, wh - 1), 0, src_h - 1);
    coef = c0 | (c1 << 16);
}

// Level of one output value: taps at byte offsets o0 / o1 (channel included) of the source rows p0 / p1, column coefficients xc (packed), row
// coefficients b0 / b1.
Y2_HD int cl_level(bool box, const uint8_t* p0, const uint8_t* p1, int o0, int o1, int xc, int b0, int b1) {
    if (box) return ((int)p0[o0] + (int)p0[o1] + (int)p1[o0] + (int)p1[o1] + 2) >> 2;
    const int c0 = xc & 0xffff, c1 = xc >> 16;
    const int h0 = (int)p0[o0] * c0 + (int)p0[o1] * c1;
    const int h1 = (int)p1[o0] * c0 + (int)p1[o1] * c1;
    return cl_clamp((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2, 0, 255);
}

// ---- y2_collate_jitter_images

// BORDER_REFLECT_101 (borderInterpolate's loop): position p on an axis of n pixels.
Y2_HD int jt_reflect101(int p, int n) {
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

// The box filter's output for an integer window sum s: inv = 1.0 / (kx * ky).
Y2_HD int jt_blur_level(int s, double inv) {
    const double v = rint((double)s * inv);
    return v < 0.0 ? 0 : (v > 255.0 ? 255 : (int)v);
}

// n / i rounded half to even, 0 for i == 0: sdiv[i] = jt_div(255 << 12, i) and hdiv[i] = jt_div((180 << 12) / 6, i).  (For i <= 255 the exact quotient
// is no closer than 1 / 510 to a half it does not hit, so this is cvRound of the correctly rounded double quotient.)
Y2_HD int jt_div(int n, int i) {
    if (i == 0) return 0;
    const int q = n / i, r = n - q * i;
    return 2 * r > i ? q + 1 : (2 * r == i ? q + (q & 1) : q);
}
#define JT_SDIV_N (255 << 12)
#define JT_HDIV_N ((180 << 12) / 6)

// 8-bit COLOR_BGR2HSV (H in 0 .. 179), integer; sdiv / hdiv: the caller's 256-entry tables (jt_div).
Y2_HD void jt_bgr2hsv(int b, int g, int r, const int* sdiv, const int* hdiv, int& h, int& s, int& v) {
    v = b > g ? b : g;
    v = v > r ? v : r;
    int vmin = b < g ? b : g;
    vmin = vmin < r ? vmin : r;
    const int diff = v - vmin;
    s = (diff * sdiv[v] + 2048) >> 12;
    h = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
    h = (h * hdiv[diff] + 2048) >> 12;
    if (h < 0) h += 180;
    h = cl_clamp(h, 0, 255);
    s = cl_clamp(s, 0, 255);
}

Y2_HD int jt_level_of(float x) {
    const float v = rintf(x * 255.f);
    return v < 0.f ? 0 : (v > 255.f ? 255 : (int)v);
}

Y2_HD float jt_pick(int sector, float a0, float a1, float a2, float a3, float a4, float a5) {
    return sector == 0 ? a0 : sector == 1 ? a1 : sector == 2 ? a2 : sector == 3 ? a3 : sector == 4 ? a4 : a5;
}

// 8-bit COLOR_HSV2RGB (H in units of 2 degrees), fp32: + - x and floorf only.
Y2_HD void jt_hsv2rgb(int h, int s, int v, int& r, int& g, int& b) {
    float hf = (float)h;
    const float sf = (float)s * (1.f / 255.f), vf = (float)v * (1.f / 255.f);
    if (s == 0) {
        r = g = b = jt_level_of(vf);
        return;
    }
    hf *= (6.f / 180.f);
    while (hf >= 6.f) hf -= 6.f;
    int sector = (int)floorf(hf);
    hf -= (float)sector;
    if (sector < 0 || sector > 5) { sector = 0; hf = 0.f; }
    const float t0 = vf, t1 = vf * (1.f - sf), t2 = vf * (1.f - sf * hf), t3 = vf * (1.f - sf * (1.f - hf));
    b = jt_level_of(jt_pick(sector, t1, t1, t3, t0, t0, t2));
    g = jt_level_of(jt_pick(sector, t3, t0, t0, t2, t1, t1));
    r = jt_level_of(jt_pick(sector, t0, t2, t1, t1, t3, t0));
}
