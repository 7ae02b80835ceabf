// Depthwise 3x3 convolution (nn.Conv2d(C, C, 3, stride, 1, groups=C, bias=False), the `dw` half of every unit of the MobileNet
// plugin, model/mobilenet.py): forward, data gradient and weight gradient on NHWC fp32, filter in its state_dict layout [C][1][3][3].
//
// Memory-bound (9 multiply-adds per output element, ~2 flop per compulsory byte): no MFMA, no LDS staging of the input.  Every thread
// owns ONE group of CV channels (CV = 4: one 16-B access per pixel and tap; CV = 1: the scalar path for widths, strides or bases that
// are not 4-aligned) for the whole launch and walks pixels with a grid stride, so the 9*CV filter taps, the epilogue affine and the
// statistics / weight-gradient accumulators stay in registers.  Lanes of a wave cover neighbouring channel groups of one pixel and then
// neighbouring pixels: every wave-wide access is contiguous; the 3x3 halo re-reads hit L1 / L2, HBM sees each input once.
//
// Block = 256 threads = TC channel lanes x TP pixel lanes (TC = the channel-group count rounded up to a power of two, at most 64);
// grid = (pixel blocks, channel blocks), sized from the problem shape alone (never from the device), so the fixed-order reductions of the
// weight gradient are reproducible bit for bit.
#include "common.h"

namespace {

constexpr int DW_THREADS = 256;
constexpr int DW_MAX_BLOCKS = Y2_NUM_CU * 8;

struct DwGrid {
    int CV, Cg, TC, TP, gx, gy;
};

// min_pix: pixels each thread should at least visit (the weight gradient amortises its partial-sum write-out over several pixels)
inline DwGrid dw_grid(long long P, int C, int CV, int min_pix) {
    DwGrid g;
    g.CV = CV;
    g.Cg = C / CV;
    g.TC = 1;
    while (g.TC < g.Cg && g.TC < 64) g.TC *= 2;
    g.TP = DW_THREADS / g.TC;
    g.gy = (g.Cg + g.TC - 1) / g.TC;
    long long gx = (P + (long long)g.TP * min_pix - 1) / ((long long)g.TP * min_pix);
    long long cap = DW_MAX_BLOCKS / g.gy;
    if (cap < 1) cap = 1;
    if (gx > cap) gx = cap;
    if (gx < 1) gx = 1;
    g.gx = (int)gx;
    return g;
}

template <int CV>
struct Vec { float v[CV]; };

template <int CV>
__device__ __forceinline__ Vec<CV> ld_vec(const float* p) {
    Vec<CV> r;
    if (CV == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int e = 0; e < CV; ++e) r.v[e] = t[e];
    } else {
#pragma unroll
        for (int e = 0; e < CV; ++e) r.v[e] = p[e];
    }
    return r;
}

template <int CV>
__device__ __forceinline__ void st_vec(float* p, const float (&v)[CV]) {
    if (CV == 4) {
        f32x4 t;
#pragma unroll
        for (int e = 0; e < CV; ++e) t[e] = v[e];
        *reinterpret_cast<f32x4*>(p) = t;
    } else {
#pragma unroll
        for (int e = 0; e < CV; ++e) p[e] = v[e];
    }
}

// ------------------------------------------------------------------------------------------------ forward
// y[b,yo,xo,c] = act(scale[c] * sum_{ky,kx} x[b, yo*s-1+ky, xo*s-1+kx, c] * w[c][ky][kx] + shift[c]); taps in row-major order.
// stats: per-channel [sum | sum^2] of the raw sum (fp64), reduced over the block's pixel lanes, one atomic per channel and block into
// copy (blockIdx.x mod Y2_STATS_REPL).
template <int CV>
__global__ __launch_bounds__(DW_THREADS) void dwconv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ scale,
                                                                const float* __restrict__ shift, float slope, float* __restrict__ y, double* __restrict__ stats,
                                                                int H, int W, int Ho, int Wo, int C, int ldx, int ldy, int stride, uint32_t P,
                                                                y2_fastdiv fWo, y2_fastdiv fHo, int TC) {
    __shared__ double red[2][DW_THREADS * CV];
    const int cl = threadIdx.x % TC, pl = threadIdx.x / TC, TP = DW_THREADS / TC;
    const int cg = blockIdx.y * TC + cl;
    const bool active = cg * CV < C;
    const int c = active ? cg * CV : 0;
    float wt[9][CV], sc[CV], sh[CV];
#pragma unroll
    for (int e = 0; e < CV; ++e) {
#pragma unroll
        for (int t = 0; t < 9; ++t) wt[t][e] = w[(c + e) * 9 + t];
        sc[e] = scale != nullptr ? scale[c + e] : 1.f;
        sh[e] = shift != nullptr ? shift[c + e] : 0.f;
    }
    double s1[CV], s2[CV];
#pragma unroll
    for (int e = 0; e < CV; ++e) s1[e] = s2[e] = 0.0;
    if (active) {
        for (uint32_t p = blockIdx.x * (uint32_t)TP + pl; p < P; p += gridDim.x * (uint32_t)TP) {
            const uint32_t r = y2_div(p, fWo);
            const int xo = (int)(p - r * (uint32_t)Wo);
            const uint32_t b = y2_div(r, fHo);
            const int yo = (int)(r - b * (uint32_t)Ho);
            float acc[CV];
#pragma unroll
            for (int e = 0; e < CV; ++e) acc[e] = 0.f;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int yy = yo * stride - 1 + ky;
                if ((unsigned)yy >= (unsigned)H) continue;
                const float* row = x + ((long long)b * H + yy) * W * (long long)ldx + c;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int xx = xo * stride - 1 + kx;
                    if ((unsigned)xx >= (unsigned)W) continue;
                    const Vec<CV> v = ld_vec<CV>(row + (long long)xx * ldx);
#pragma unroll
                    for (int e = 0; e < CV; ++e) acc[e] = fmaf(v.v[e], wt[ky * 3 + kx][e], acc[e]);
                }
            }
            float o[CV];
#pragma unroll
            for (int e = 0; e < CV; ++e) {
                if (stats != nullptr) { s1[e] += (double)acc[e]; s2[e] += (double)acc[e] * (double)acc[e]; }
                const float a = acc[e] * sc[e] + sh[e];
                o[e] = a < 0.f ? a * slope : a;
            }
            st_vec<CV>(y + (long long)p * ldy + c, o);
        }
    }
    if (stats == nullptr) return;        // (uniform: a kernel argument)
#pragma unroll
    for (int e = 0; e < CV; ++e) {
        red[0][threadIdx.x * CV + e] = s1[e];
        red[1][threadIdx.x * CV + e] = s2[e];
    }
    __syncthreads();
    if (pl == 0 && active) {
        double* st = stats + (size_t)(blockIdx.x % Y2_STATS_REPL) * 2 * C;
#pragma unroll
        for (int e = 0; e < CV; ++e) {
            double a = 0.0, q = 0.0;
            for (int i = 0; i < TP; ++i) {
                a += red[0][(i * TC + cl) * CV + e];
                q += red[1][(i * TC + cl) * CV + e];
            }
            atomicAdd(st + c + e, a);
            atomicAdd(st + C + c + e, q);
        }
    }
}

// ------------------------------------------------------------------------------------------------ data gradient (gather form)
// dx[b,y,x,c] = sum_{ky,kx} dz[b,(y+1-ky)/s,(x+1-kx)/s,c] * w[c][ky][kx] over the taps whose output position exists (<= 9 at stride 1,
// <= 4 at stride 2), in row-major tap order: no atomics, reproducible by construction.
template <int CV>
__global__ __launch_bounds__(DW_THREADS) void dwconv_dgrad_kernel(const float* __restrict__ dz, const float* __restrict__ w, float* __restrict__ dx,
                                                                  int H, int W, int Ho, int Wo, int C, int ldz, int lddx, int stride, uint32_t P,
                                                                  y2_fastdiv fW, y2_fastdiv fH, int TC) {
    const int cl = threadIdx.x % TC, pl = threadIdx.x / TC, TP = DW_THREADS / TC;
    const int cg = blockIdx.y * TC + cl;
    if (cg * CV >= C) return;
    const int c = cg * CV;
    float wt[9][CV];
#pragma unroll
    for (int e = 0; e < CV; ++e)
#pragma unroll
        for (int t = 0; t < 9; ++t) wt[t][e] = w[(c + e) * 9 + t];
    for (uint32_t p = blockIdx.x * (uint32_t)TP + pl; p < P; p += gridDim.x * (uint32_t)TP) {
        const uint32_t r = y2_div(p, fW);
        const int xi = (int)(p - r * (uint32_t)W);
        const uint32_t b = y2_div(r, fH);
        const int yi = (int)(r - b * (uint32_t)H);
        float acc[CV];
#pragma unroll
        for (int e = 0; e < CV; ++e) acc[e] = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int ty = yi + 1 - ky;
            if (ty < 0 || (stride == 2 && (ty & 1))) continue;
            const int yo = stride == 2 ? ty >> 1 : ty;
            if (yo >= Ho) continue;
            const float* row = dz + ((long long)b * Ho + yo) * Wo * (long long)ldz + c;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int tx = xi + 1 - kx;
                if (tx < 0 || (stride == 2 && (tx & 1))) continue;
                const int xo = stride == 2 ? tx >> 1 : tx;
                if (xo >= Wo) continue;
                const Vec<CV> v = ld_vec<CV>(row + (long long)xo * ldz);
#pragma unroll
                for (int e = 0; e < CV; ++e) acc[e] = fmaf(v.v[e], wt[ky * 3 + kx][e], acc[e]);
            }
        }
        st_vec<CV>(dx + (long long)p * lddx + c, acc);
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient, stage 1
// partial[blockIdx.x][c][t] = sum over this block's output pixels of dz[p][c] * x[tap t of p][c]: per-thread fp32 accumulators over the
// thread's grid-stride pixels, then the block's TP pixel lanes added in lane order through LDS.  Plain stores, no atomics.
template <int CV>
__global__ __launch_bounds__(DW_THREADS) void dwconv_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dz, float* __restrict__ partial,
                                                                  int H, int W, int Ho, int Wo, int C, int ldx, int ldz, int stride, uint32_t P,
                                                                  y2_fastdiv fWo, y2_fastdiv fHo, int TC) {
    constexpr int NA = 9 * CV, LDA = NA + 1;            // +1: the lane-order reads below walk the LDS rows with an odd stride
    __shared__ float red[DW_THREADS * LDA];
    const int cl = threadIdx.x % TC, pl = threadIdx.x / TC, TP = DW_THREADS / TC;
    const int cg = blockIdx.y * TC + cl;
    const bool active = cg * CV < C;
    const int c = active ? cg * CV : 0;
    float acc[9][CV];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < CV; ++e) acc[t][e] = 0.f;
    if (active) {
        for (uint32_t p = blockIdx.x * (uint32_t)TP + pl; p < P; p += gridDim.x * (uint32_t)TP) {
            const uint32_t r = y2_div(p, fWo);
            const int xo = (int)(p - r * (uint32_t)Wo);
            const uint32_t b = y2_div(r, fHo);
            const int yo = (int)(r - b * (uint32_t)Ho);
            const Vec<CV> g = ld_vec<CV>(dz + (long long)p * ldz + c);
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int yy = yo * stride - 1 + ky;
                if ((unsigned)yy >= (unsigned)H) continue;
                const float* row = x + ((long long)b * H + yy) * W * (long long)ldx + c;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int xx = xo * stride - 1 + kx;
                    if ((unsigned)xx >= (unsigned)W) continue;
                    const Vec<CV> v = ld_vec<CV>(row + (long long)xx * ldx);
#pragma unroll
                    for (int e = 0; e < CV; ++e) acc[ky * 3 + kx][e] = fmaf(v.v[e], g.v[e], acc[ky * 3 + kx][e]);
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < CV; ++e) red[threadIdx.x * LDA + e * 9 + t] = acc[t][e];
    __syncthreads();
    // TC * 9 * CV outputs of this block: output j = (channel lane, e*9 + t), summed over the pixel lanes in order
    for (int j = threadIdx.x; j < TC * NA; j += DW_THREADS) {
        const int l = j / NA, k = j - l * NA;
        const int cj = (blockIdx.y * TC + l) * CV;
        if (cj >= C) continue;
        float s = 0.f;
        for (int i = 0; i < TP; ++i) s += red[(i * TC + l) * LDA + k];
        partial[(size_t)blockIdx.x * C * 9 + (size_t)cj * 9 + k] = s;          // k = e*9 + t: channel cj + e, tap t
    }
}

// stage 2: dw[n] = sum_{g < G} partial[g][n] for n < C*9, in fp64, lanes of a row group summing every DW_R-th partial, the DW_R lane sums
// then added in lane order
constexpr int DW_R = 8, DW_N = DW_THREADS / DW_R;
__global__ __launch_bounds__(DW_THREADS) void dwconv_wgrad_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dw, int N, int G) {
    __shared__ double red[DW_R][DW_N];
    const int ln = threadIdx.x % DW_N, r = threadIdx.x / DW_N;
    const int n = blockIdx.x * DW_N + ln;
    double s = 0.0;
    if (n < N)
        for (int g = r; g < G; g += DW_R) s += (double)partial[(size_t)g * N + n];
    red[r][ln] = s;
    __syncthreads();
    if (r == 0 && n < N) {
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < DW_R; ++i) t += red[i][ln];
        dw[n] = (float)t;
    }
}

inline bool dw_vec_ok(int C, int lda, int ldb, const void* a, const void* b) {
    return !(C & 3) && !(lda & 3) && !(ldb & 3) && y2_aligned16(a) && y2_aligned16(b);
}

inline bool dw_shape_ok(int B, int H, int W, int C, int stride, long long* Pin, long long* Pout, int* Ho, int* Wo) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (stride != 1 && stride != 2)) return false;
    *Ho = (H - 1) / stride + 1;
    *Wo = (W - 1) / stride + 1;
    *Pin = (long long)B * H * W;
    *Pout = (long long)B * *Ho * *Wo;
    return *Pin < 0x7fffffffLL;          // pixel indices are 32-bit
}

constexpr int DW_WGRAD_MIN_PIX = 8;

}  // namespace

extern "C" int y2_dwconv_fwd(const float* x, const float* w, const float* scale, const float* shift, float slope, float* y, double* stats,
                             int B, int H, int W, int C, int ldx, int ldy, int stride, y2_stream_t stream) {
    long long Pin, P;
    int Ho, Wo;
    if (!x || !w || !y || !dw_shape_ok(B, H, W, C, stride, &Pin, &P, &Ho, &Wo) || ldx < C || ldy < C) return Y2_EINVAL;
    if (stats != nullptr && y2_det.on) return Y2_ENOSUP;      // deterministic mode: statistics come from y2_colstats_det, not from atomics
    const int CV = dw_vec_ok(C, ldx, ldy, x, y) ? 4 : 1;
    const DwGrid g = dw_grid(P, C, CV, 1);
    const double flops = 2.0 * 9 * (double)P * C;
    if (CV == 4)
        Y2_LAUNCH("dwconv_fwd_kernel", flops, (dwconv_fwd_kernel<4>), dim3(g.gx, g.gy), dim3(DW_THREADS), 0, y2_s(stream), x, w, scale, shift, slope, y, stats,
                  H, W, Ho, Wo, C, ldx, ldy, stride, (uint32_t)P, y2_make_fastdiv(Wo), y2_make_fastdiv(Ho), g.TC);
    else
        Y2_LAUNCH("dwconv_fwd_kernel", flops, (dwconv_fwd_kernel<1>), dim3(g.gx, g.gy), dim3(DW_THREADS), 0, y2_s(stream), x, w, scale, shift, slope, y, stats,
                  H, W, Ho, Wo, C, ldx, ldy, stride, (uint32_t)P, y2_make_fastdiv(Wo), y2_make_fastdiv(Ho), g.TC);
    Y2_LAUNCH_CHECK();
    return Y2_OK;
}

extern "C" int y2_dwconv_dgrad(const float* dz, const float* w, float* dx, int B, int H, int W, int C, int ldz, int lddx, int stride, y2_stream_t stream) {
    long long P, Pout;
    int Ho, Wo;
    if (!dz || !w || !dx || !dw_shape_ok(B, H, W, C, stride, &P, &Pout, &Ho, &Wo) || ldz < C || lddx < C) return Y2_EINVAL;
    const int CV = dw_vec_ok(C, ldz, lddx, dz, dx) ? 4 : 1;
    const DwGrid g = dw_grid(P, C, CV, 1);
    const double flops = 2.0 * 9 * (double)Pout * C;
    if (CV == 4)
        Y2_LAUNCH("dwconv_dgrad_kernel", flops, (dwconv_dgrad_kernel<4>), dim3(g.gx, g.gy), dim3(DW_THREADS), 0, y2_s(stream), dz, w, dx,
                  H, W, Ho, Wo, C, ldz, lddx, stride, (uint32_t)P, y2_make_fastdiv(W), y2_make_fastdiv(H), g.TC);
    else
        Y2_LAUNCH("dwconv_dgrad_kernel", flops, (dwconv_dgrad_kernel<1>), dim3(g.gx, g.gy), dim3(DW_THREADS), 0, y2_s(stream), dz, w, dx,
                  H, W, Ho, Wo, C, ldz, lddx, stride, (uint32_t)P, y2_make_fastdiv(W), y2_make_fastdiv(H), g.TC);
    Y2_LAUNCH_CHECK();
    return Y2_OK;
}

extern "C" long long y2_dwconv_wgrad_workspace_bytes(int B, int H, int W, int C, int stride) {
    long long Pin, P;
    int Ho, Wo;
    if (!dw_shape_ok(B, H, W, C, stride, &Pin, &P, &Ho, &Wo)) return 0;
    long long gx = 0;
    for (int CV = 1; CV <= 4; CV += 3) {          // either path (the vector path needs C % 4 == 0 and aligned operands)
        if (CV == 4 && (C & 3)) continue;
        const DwGrid g = dw_grid(P, C, CV, DW_WGRAD_MIN_PIX);
        if (g.gx > gx) gx = g.gx;
    }
    return gx * C * 9 * (long long)sizeof(float);
}

extern "C" int y2_dwconv_wgrad(const float* x, const float* dz, float* dw, float* workspace, long long workspace_bytes,
                               int B, int H, int W, int C, int ldx, int ldz, int stride, y2_stream_t stream) {
    long long Pin, P;
    int Ho, Wo;
    if (!x || !dz || !dw || !workspace || !dw_shape_ok(B, H, W, C, stride, &Pin, &P, &Ho, &Wo) || ldx < C || ldz < C) return Y2_EINVAL;
    if (!y2_aligned16(workspace)) return Y2_EALIGN;
    const int CV = dw_vec_ok(C, ldx, ldz, x, dz) ? 4 : 1;
    const DwGrid g = dw_grid(P, C, CV, DW_WGRAD_MIN_PIX);
    if ((long long)g.gx * C * 9 * (long long)sizeof(float) > workspace_bytes) return Y2_EINVAL;
    const double flops = 2.0 * 9 * (double)P * C;
    if (CV == 4)
        Y2_LAUNCH("dwconv_wgrad_kernel", flops, (dwconv_wgrad_kernel<4>), dim3(g.gx, g.gy), dim3(DW_THREADS), 0, y2_s(stream), x, dz, workspace,
                  H, W, Ho, Wo, C, ldx, ldz, stride, (uint32_t)P, y2_make_fastdiv(Wo), y2_make_fastdiv(Ho), g.TC);
    else
        Y2_LAUNCH("dwconv_wgrad_kernel", flops, (dwconv_wgrad_kernel<1>), dim3(g.gx, g.gy), dim3(DW_THREADS), 0, y2_s(stream), x, dz, workspace,
                  H, W, Ho, Wo, C, ldx, ldz, stride, (uint32_t)P, y2_make_fastdiv(Wo), y2_make_fastdiv(Ho), g.TC);
    Y2_LAUNCH_CHECK();
    const int N = C * 9;
    Y2_LAUNCH("dwconv_wgrad_reduce_kernel", 0.0, dwconv_wgrad_reduce_kernel, dim3((N + DW_N - 1) / DW_N), dim3(DW_THREADS), 0, y2_s(stream), workspace, dw, N, g.gx);
    Y2_LAUNCH_CHECK();
    return Y2_OK;
}
