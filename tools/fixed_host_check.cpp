// fixed_host_check.cpp — a stand-alone program (its own main, no HIP, no Python) that drives fx_images_host of csrc/fixed.h - the whole of
// y2_fixed_images_host (host.hip only forwards to it) and, function for function, the arithmetic of fixed.hip's kernel - with random and hostile
// tables, meant to be built with the address and undefined-behaviour sanitizers:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -I yolo2-pytorch_amd/csrc tools/fixed_host_check.cpp -o fixed_host_check
//   ./fixed_host_check [runs]
//
// Every buffer (source bytes, tables, level table, output) is a heap block of exactly the size the contract names - the last image ends where the source
// block ends -, so a read or write one element outside is reported.  Per run: B in 0 .. 6 images of 1 .. 40 rows and columns (1 x 1 regularly), padded
// row strides, odd offsets, modes 0 and 1, matrices that are scales, rotations or anything within the limits; H and W in 1 .. 24.  Hostile runs damage one
// table entry: NaN, infinite and huge matrix entries, modes outside 0 / 1, zero and negative extents, a stride below 3 * src_w, a negative offset.
// Checked: a damaged table is refused (-1) and leaves every output value untouched; an intact one returns 0, writes every value (none keeps the canary)
// from the level table's range, and pixels of the identity map in mode 1 are the source's.  A second pass hands the pixel functions themselves
// positions nobody checked - any 64-bit X and Y - against exact-size images: whatever the coordinates, no load leaves the image.
#define Y2_HD inline
#include "fixed.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>

namespace {

template <class T>
T* block(size_t n) { return (T*)malloc(n ? n * sizeof(T) : 1); }          // exact blocks, not vectors: capacity would hide an overrun

int fail(const char* what, long long run) {
    fprintf(stderr, "run %lld: %s\n", run, what);
    return 1;
}

const float CANARY = -7.f;

}  // namespace

int main(int argc, char** argv) {
    const long long runs = argc > 1 ? atoll(argv[1]) : 20000;
    std::mt19937 rng(29);
    std::uniform_real_distribution<double> unit(0.0, 1.0);
    const double inf = std::numeric_limits<double>::infinity();
    const double hostile_values[] = {std::numeric_limits<double>::quiet_NaN(), inf, -inf, 1e308, -1e300, 524289.0, -1e9, 4.0000001, -4.5};          // the last two: out of range for A0, A1, A3, A4 only
    long long accepted = 0, refused = 0, positions = 0;
    for (long long run = 0; run < runs; ++run) {
        const bool hostile = run % 3 == 0;
        const int B = run % 13 == 0 ? 0 : 1 + (int)(rng() % 6);
        const int H = 1 + (int)(rng() % 24), W = 1 + (int)(rng() % 24);
        int64_t* offset = block<int64_t>(B);
        int32_t* geom = block<int32_t>(4 * (size_t)B);
        double* inv = block<double>(6 * (size_t)B);
        long long pos = 0;
        for (int b = 0; b < B; ++b) {
            const int h = run % 7 == 0 ? 1 : 1 + (int)(rng() % 40), w = run % 7 == 0 ? 1 : 1 + (int)(rng() % 40);
            const int stride = 3 * w + (int)(rng() % 3) * (int)(rng() % 9);
            pos += 1 + (int)(rng() % 4);
            offset[b] = pos;
            pos += (long long)(h - 1) * stride + 3LL * w;          // the image ends where its last pixel ends
            geom[4 * b] = stride; geom[4 * b + 1] = h; geom[4 * b + 2] = w; geom[4 * b + 3] = (int)(rng() % 2);
            double* A = inv + 6 * b;
            const int kind = (int)(rng() % 4);
            if (kind == 0) {          // the `fixed` resize itself: one scale
                const double s = 0.25 + 3.75 * unit(rng);
                A[0] = A[4] = s; A[1] = A[3] = A[2] = A[5] = 0.0;
            } else if (kind == 1) {   // the identity: an exact copy in both modes
                A[0] = A[4] = 1.0; A[1] = A[3] = A[2] = A[5] = 0.0;
            } else if (kind == 2) {   // a rotation with a scale and a shift
                const double t = 6.283185307179586 * unit(rng), s = 0.3 + 2.0 * unit(rng);
                A[0] = s * cos(t); A[1] = s * sin(t); A[3] = -s * sin(t); A[4] = s * cos(t);
                A[2] = 80.0 * unit(rng) - 40.0; A[5] = 80.0 * unit(rng) - 40.0;
            } else {                  // anything within the limits, the limits themselves included
                for (int k = 0; k < 6; ++k) {
                    const double lim = (k == 2 || k == 5) ? 524288.0 : 4.0;
                    A[k] = rng() % 5 == 0 ? (rng() % 2 ? lim : -lim) : lim * (2.0 * unit(rng) - 1.0);
                }
            }
        }
        uint8_t* src = block<uint8_t>((size_t)pos);
        for (long long i = 0; i < pos; ++i) src[i] = (uint8_t)rng();
        float* lut = block<float>(768);
        for (int i = 0; i < 768; ++i) lut[i] = (float)(i % 256) + 1000.f * (float)(i / 256);          // level and plane can be read back
        const size_t n = (size_t)B * 3 * H * W;
        float* out = block<float>(n);
        for (size_t i = 0; i < n; ++i) out[i] = CANARY;
        bool damaged = false;
        if (hostile && B > 0) {
            const int b = (int)(rng() % B);
            damaged = true;
            switch (rng() % 6) {
                case 0: { const int k = (int)(rng() % 6); inv[6 * b + k] = hostile_values[rng() % ((k == 2 || k == 5) ? 7 : 9)]; break; }
                case 1: { const int32_t bad[] = {2, -1, 255, INT32_MIN, INT32_MAX}; geom[4 * b + 3] = bad[rng() % 5]; break; }
                case 2: { const int32_t bad[] = {0, -1, -40, INT32_MIN, FX_MAX_DIM + 1, INT32_MAX}; geom[4 * b + 1 + rng() % 2] = bad[rng() % 6]; break; }
                case 3: geom[4 * b] = 3 * geom[4 * b + 2] - 1 - (int)(rng() % 3); break;
                case 4: { const int64_t bad[] = {-1, INT64_MIN, -pos}; offset[b] = bad[rng() % 3]; break; }
                default: geom[4 * b] = rng() % 2 ? 0 : -geom[4 * b]; break;
            }
        }
        const int flags = (int)(rng() % 2);
        const int code = fx_images_host(src, offset, geom, inv, lut, B, H, W, flags, out);
        if (damaged) {
            if (code != -1) return fail("a damaged table was not refused", run);
            for (size_t i = 0; i < n; ++i)
                if (out[i] != CANARY) return fail("a refused call wrote to out", run);
            ++refused;
        } else {
            if (code != 0) return fail("an intact table was refused", run);
            for (int b = 0; b < B; ++b) {
                const double* A = inv + 6 * b;
                const bool identity = A[0] == 1.0 && A[4] == 1.0 && A[1] == 0.0 && A[3] == 0.0 && A[2] == 0.0 && A[5] == 0.0;
                for (int c = 0; c < 3; ++c)
                    for (int y = 0; y < H; ++y)
                        for (int x = 0; x < W; ++x) {
                            const float v = out[(((size_t)b * 3 + c) * H + y) * W + x] - 1000.f * (float)c;
                            if (!(v >= 0.f && v <= 255.f) || v != floorf(v)) return fail("an output value that is no entry of its plane's table", run);
                            if (identity) {
                                const int ch = c == 1 ? 1 : (flags ? 2 - c : c);
                                const bool in = y < geom[4 * b + 1] && x < geom[4 * b + 2];
                                const int want = in ? src[offset[b] + (long long)y * geom[4 * b] + 3 * x + ch] : 0;
                                if ((int)v != want) return fail("the identity map is no exact copy", run);
                            }
                        }
            }
            ++accepted;
        }
        // the pixel functions at positions nobody checked: any X and Y against the exact-size image of image 0 (or a 1 x 1 image)
        {
            const int h = B ? (damaged ? 1 : geom[1]) : 1, w = B ? (damaged ? 1 : geom[2]) : 1;
            const int stride = 3 * w;
            uint8_t* img = block<uint8_t>((size_t)h * stride);
            memset(img, 200, (size_t)h * stride);
            for (int k = 0; k < 64; ++k) {
                long long X = (long long)(((unsigned long long)rng() << 32) | rng()), Y = (long long)(((unsigned long long)rng() << 32) | rng());
                if (k % 4 == 0) { X = (long long)(rng() % (32 * (w + 4))) - 64; Y = (long long)(rng() % (32 * (h + 4))) - 64; }          // around the image
                if (k % 16 == 1) { X = std::numeric_limits<long long>::max(); Y = std::numeric_limits<long long>::min(); }
                const unsigned a = fx_linear(img, stride, h, w, X, Y), c = fx_cubic(img, stride, h, w, X, Y);
                if ((a | c) >> 24) return fail("a packed pixel beyond 24 bits", run);
                positions += 2;
            }
            free(img);
        }
        free(offset); free(geom); free(inv); free(src); free(lut); free(out);
    }
    printf("%lld runs: %lld accepted, %lld refused, %lld pixels at unchecked positions\n", runs, accepted, refused, positions);
    return 0;
}
