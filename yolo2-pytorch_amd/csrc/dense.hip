// Pre-activation kernels of the DenseNet plugin (model/densenet.py; torchvision's _DenseLayer / _Transition: BatchNorm -> ReLU -> conv 1x1
// [-> AvgPool2d(2, 2)]) on NHWC fp32.
//
// Every dense layer normalises the SAME growing concatenation with its own gamma / beta, so the affine + ReLU cannot live in a producer's
// epilogue (the library's conv -> affine -> activation form); it has to sit in front of the consumer's GEMM:
//   y2_preact_conv1x1_fwd  out[m][n] = epi(sum_k act(a[k] * x[m][k] + b[k]) * w[n][k]): the pre-activation runs in the A-operand loader (global ->
//                          VGPR -> mul, add, select -> LDS), the product on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32, accumulators in VGPRs),
//                          the epilogue is y2_conv_params' (per-output-channel affine, LeakyReLU, ldy / coff write-through, fp64 statistics of the
//                          raw product).  pool = 1: the loader averages the 2x2 window of pre-activated inputs and the GEMM runs at half
//                          resolution (a 1x1 convolution and an average pool commute): a quarter of the multiply-adds of conv -> pool.
//   y2_preact_fwd          the materialising form A = act(a * x + b) [2x2-averaged], dense: the operand of the 1x1 weight gradient, and the
//                          unfused A/B leg.
//   y2_preact_bwd          backward of (BatchNorm | frozen BatchNorm | nothing) -> ReLU [-> AvgPool 2x2] on a channel slice of a block buffer,
//                          WRITING or ADDING the input gradient into the block's gradient buffer (a slab has many consumers).
//
// GEMM geometry: 256 threads = 2 x 2 waves, block tile (64 MT) x (64 NT) x 32, MT, NT in {1, 2}: each wave owns MT x NT accumulator tiles of
// 32 x 32.  Both operands are K-contiguous ([pixel][k] with stride ldx, [n][k] with stride K), staged through LDS rows of 36 floats (144 B: the
// 16 lanes of a ds_read_b128 group fall on 16 different 16-B slots).  The sum over k is order-free, so lane half h of the 32x32x2 instruction
// takes k = 16 h + j (not 2 j + h): each lane reads its 16 k-values of a row as four 16-B words.  Next tile global -> VGPR loads are issued
// before the current tile's MFMAs.
#include "common.h"

namespace {

constexpr int PG_THREADS = 256;
constexpr int PG_BK = 32;
constexpr int PG_LDK = 36;

struct PreactGemmArgs {
    const float* x;
    const float* w;
    const float* pre_scale;
    const float* pre_shift;
    const float* scale;
    const float* shift;
    float* y;
    double* stats;
    long long M;             // output pixels
    int H, W, Ho, Wo;        // input / output spatial size (equal unless pooled)
    int K, ldx, N, ldy, coff, gn;
    float pre_slope, slope;
    y2_fastdiv fWo, fHo;
};

__device__ __forceinline__ float pre_act(float v, float sc, float sh, float slope) {
    const float a = v * sc + sh;
    return a < 0.f ? a * slope : a;
}

// 4 consecutive floats at p + k (k .. k+3 < K on the vector path; element-wise bounds on the scalar path); p == nullptr: zeros
template <bool VEC>
__device__ __forceinline__ f32x4 ld4(const float* p, int k, int K, float fill) {
    f32x4 r = {fill, fill, fill, fill};
    if (p == nullptr) return r;
    if (VEC) {
        if (k < K) r = *reinterpret_cast<const f32x4*>(p + k);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k + e < K) r[e] = p[k + e];
    }
    return r;
}

template <int MT, int NT, bool VEC, bool POOL>
__global__ __launch_bounds__(PG_THREADS) void preact_gemm_kernel(const PreactGemmArgs a) {
    constexpr int BM = 64 * MT, BN = 64 * NT, RA = BM / 32, RB = BN / 32, NP = POOL ? 4 : 1;
    __shared__ __attribute__((aligned(16))) float As[BM * PG_LDK];
    __shared__ __attribute__((aligned(16))) float Bs[BN * PG_LDK];
    __shared__ double sred[2][2][BN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int nb = blockIdx.x % a.gn, mb = blockIdx.x / a.gn;
    const long long m0 = (long long)mb * BM;
    const int n0 = nb * BN;
    const int kq = (tid & 7) * 4, r0 = tid >> 3;

    // per-thread row pointers: RA rows of the A tile (top-left pixel of the window when pooled), RB rows of the weight panel
    const float* arow[RA];
    const float* brow[RB];
#pragma unroll
    for (int i = 0; i < RA; ++i) {
        const long long m = m0 + r0 + 32 * i;
        arow[i] = nullptr;
        if (m < a.M) {
            if (POOL) {
                const uint32_t r = y2_div((uint32_t)m, a.fWo);
                const int xo = (int)((uint32_t)m - r * (uint32_t)a.Wo);
                const uint32_t b = y2_div(r, a.fHo);
                const int yo = (int)(r - b * (uint32_t)a.Ho);
                arow[i] = a.x + (((long long)b * a.H + 2 * yo) * a.W + 2 * xo) * (long long)a.ldx;
            } else {
                arow[i] = a.x + m * (long long)a.ldx;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        const int n = n0 + r0 + 32 * i;
        brow[i] = n < a.N ? a.w + (long long)n * a.K : nullptr;
    }
    const long long poff[4] = {0, a.ldx, (long long)a.W * a.ldx, (long long)(a.W + 1) * a.ldx};

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    f32x4 ra[RA][NP], rb[RB], rsc, rsh;
    auto load_tile = [&](int k0) {
        const int k = k0 + kq;
        rsc = ld4<VEC>(a.pre_scale, k, a.K, 1.f);
        rsh = ld4<VEC>(a.pre_shift, k, a.K, 0.f);
#pragma unroll
        for (int i = 0; i < RA; ++i)
#pragma unroll
            for (int q = 0; q < NP; ++q) ra[i][q] = ld4<VEC>(arow[i] != nullptr ? arow[i] + poff[q] : nullptr, k, a.K, 0.f);
#pragma unroll
        for (int i = 0; i < RB; ++i) rb[i] = ld4<VEC>(brow[i], k, a.K, 0.f);
    };
    auto store_tile = [&](int k0) {
        const int k = k0 + kq;
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (arow[i] != nullptr) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (k + e < a.K) {          // (a padded k must stay zero: act(shift) is not)
                        if (POOL) {
                            const float s = (pre_act(ra[i][0][e], rsc[e], rsh[e], a.pre_slope) + pre_act(ra[i][1 % NP][e], rsc[e], rsh[e], a.pre_slope)) +
                                            (pre_act(ra[i][2 % NP][e], rsc[e], rsh[e], a.pre_slope) + pre_act(ra[i][3 % NP][e], rsc[e], rsh[e], a.pre_slope));
                            v[e] = 0.25f * s;
                        } else {
                            v[e] = pre_act(ra[i][0][e], rsc[e], rsh[e], a.pre_slope);
                        }
                    }
                }
            }
            *reinterpret_cast<f32x4*>(&As[(r0 + 32 * i) * PG_LDK + kq]) = v;
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) *reinterpret_cast<f32x4*>(&Bs[(r0 + 32 * i) * PG_LDK + kq]) = rb[i];
    };

    const int nk = (a.K + PG_BK - 1) / PG_BK;
    const int lr = lane & 31, lh = lane >> 5;
    load_tile(0);
    for (int kt = 0; kt < nk; ++kt) {
        store_tile(kt * PG_BK);
        __syncthreads();
        if (kt + 1 < nk) load_tile((kt + 1) * PG_BK);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 fa[MT], fb[NT];
#pragma unroll
            for (int i = 0; i < MT; ++i) fa[i] = *reinterpret_cast<const f32x4*>(&As[(wm * 32 * MT + i * 32 + lr) * PG_LDK + lh * 16 + q * 4]);
#pragma unroll
            for (int j = 0; j < NT; ++j) fb[j] = *reinterpret_cast<const f32x4*>(&Bs[(wn * 32 * NT + j * 32 + lr) * PG_LDK + lh * 16 + q * 4]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][e], fb[j][e], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    // epilogue: accumulator register e of lane (lr, lh) is row (e & 3) + 8 (e >> 2) + 4 lh, column lr of its 32 x 32 tile
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int nl = wn * 32 * NT + j * 32 + lr, n = n0 + nl;
        const bool nok = n < a.N;
        const float sc = (nok && a.scale != nullptr) ? a.scale[n] : 1.f;
        const float sh = (nok && a.shift != nullptr) ? a.shift[n] : 0.f;
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float raw = acc[i][j][e];
                if (a.stats != nullptr) { s1 += (double)raw; s2 += (double)raw * (double)raw; }          // rows >= M are zero rows of A
                const long long m = m0 + wm * 32 * MT + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (nok && m < a.M) {
                    const float v = raw * sc + sh;
                    a.y[m * (long long)a.ldy + a.coff + n] = v < 0.f ? v * a.slope : v;
                }
            }
        }
        if (a.stats != nullptr) {          // (uniform: a kernel argument)
            s1 += __shfl_xor(s1, 32);
            s2 += __shfl_xor(s2, 32);
            if (lh == 0) { sred[wm][0][nl] = s1; sred[wm][1][nl] = s2; }
        }
    }
    if (a.stats == nullptr) return;
    __syncthreads();
    if (tid < BN && n0 + tid < a.N) {
        double* st = a.stats + (size_t)(mb % Y2_STATS_REPL) * 2 * a.N;
        atomicAdd(st + n0 + tid, sred[0][0][tid] + sred[1][0][tid]);
        atomicAdd(st + a.N + n0 + tid, sred[0][1][tid] + sred[1][1][tid]);
    }
}

template <int MT, int NT>
int launch_preact_gemm(const PreactGemmArgs& a, bool vec, bool pool, hipStream_t s) {
    const long long gm = (a.M + 64 * MT - 1) / (64 * MT);
    if (gm * a.gn > 0x7fffffffLL) return Y2_EINVAL;
    const dim3 grid((unsigned)(gm * a.gn)), block(PG_THREADS);
    const double flops = 2.0 * (double)a.M * a.N * a.K;
    if (vec && pool) Y2_LAUNCH("preact_gemm_kernel", flops, (preact_gemm_kernel<MT, NT, true, true>), grid, block, 0, s, a);
    else if (vec) Y2_LAUNCH("preact_gemm_kernel", flops, (preact_gemm_kernel<MT, NT, true, false>), grid, block, 0, s, a);
    else if (pool) Y2_LAUNCH("preact_gemm_kernel", flops, (preact_gemm_kernel<MT, NT, false, true>), grid, block, 0, s, a);
    else Y2_LAUNCH("preact_gemm_kernel", flops, (preact_gemm_kernel<MT, NT, false, false>), grid, block, 0, s, a);
    Y2_LAUNCH_CHECK();
    return Y2_OK;
}

// ------------------------------------------------------------------------------------------------ element-wise kernels
// Thread (cl, pl) of a block owns ONE group of CV channels and walks pixels with a grid stride (the layout of csrc/dwconv.hip): the
// per-channel constants stay in registers, every wave-wide access is contiguous.  The grid depends on the problem shape alone.
constexpr int PE_THREADS = 256;
constexpr int PE_MAX_BLOCKS = Y2_NUM_CU * 8;

struct PeGrid { int Cg, TC, TP, gx, gy; };

inline PeGrid pe_grid(long long P, int C, int CV, int min_pix) {
    PeGrid g;
    g.Cg = C / CV;
    g.TC = 1;
    while (g.TC < g.Cg && g.TC < 64) g.TC *= 2;
    g.TP = PE_THREADS / g.TC;
    g.gy = (g.Cg + g.TC - 1) / g.TC;
    long long gx = (P + (long long)g.TP * min_pix - 1) / ((long long)g.TP * min_pix);
    long long cap = PE_MAX_BLOCKS / g.gy;
    if (cap < 1) cap = 1;
    if (gx > cap) gx = cap;
    if (gx < 1) gx = 1;
    g.gx = (int)gx;
    return g;
}

template <int CV>
__device__ __forceinline__ void ldv(const float* p, float (&v)[CV]) {
    if (CV == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int e = 0; e < CV; ++e) v[e] = t[e];
    } else {
#pragma unroll
        for (int e = 0; e < CV; ++e) v[e] = p[e];
    }
}

template <int CV>
__device__ __forceinline__ void stv(float* p, const float (&v)[CV]) {
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

// out[po][c] = act(sc[c] * x + sh[c]), or the mean of that over the 2x2 input window of output pixel po (same summation order as the GEMM loader)
template <int CV, bool POOL>
__global__ __launch_bounds__(PE_THREADS) void preact_fwd_kernel(const float* __restrict__ x, const float* __restrict__ pre_scale, const float* __restrict__ pre_shift,
                                                                float pre_slope, float* __restrict__ out, int H, int W, int Ho, int Wo, int C, int ldx, int ldo,
                                                                uint32_t P, y2_fastdiv fWo, y2_fastdiv fHo, int TC) {
    const int cl = threadIdx.x % TC, pl = threadIdx.x / TC, TP = PE_THREADS / TC;
    const int c = (blockIdx.y * TC + cl) * CV;
    if (c >= C) return;
    float sc[CV], sh[CV];
#pragma unroll
    for (int e = 0; e < CV; ++e) {
        sc[e] = pre_scale != nullptr ? pre_scale[c + e] : 1.f;
        sh[e] = pre_shift != nullptr ? pre_shift[c + e] : 0.f;
    }
    for (uint32_t p = blockIdx.x * (uint32_t)TP + pl; p < P; p += gridDim.x * (uint32_t)TP) {
        float o[CV];
        if (POOL) {
            const uint32_t r = y2_div(p, fWo);
            const int xo = (int)(p - r * (uint32_t)Wo);
            const uint32_t b = y2_div(r, fHo);
            const int yo = (int)(r - b * (uint32_t)Ho);
            const float* q = x + (((long long)b * H + 2 * yo) * W + 2 * xo) * (long long)ldx + c;
            float v0[CV], v1[CV], v2[CV], v3[CV];
            ldv<CV>(q, v0);
            ldv<CV>(q + ldx, v1);
            ldv<CV>(q + (long long)W * ldx, v2);
            ldv<CV>(q + (long long)(W + 1) * ldx, v3);
#pragma unroll
            for (int e = 0; e < CV; ++e)
                o[e] = 0.25f * ((pre_act(v0[e], sc[e], sh[e], pre_slope) + pre_act(v1[e], sc[e], sh[e], pre_slope)) +
                                (pre_act(v2[e], sc[e], sh[e], pre_slope) + pre_act(v3[e], sc[e], sh[e], pre_slope)));
        } else {
            float v[CV];
            ldv<CV>(x + (long long)p * ldx + c, v);
#pragma unroll
            for (int e = 0; e < CV; ++e) o[e] = pre_act(v[e], sc[e], sh[e], pre_slope);
        }
        stv<CV>(out + (long long)p * ldo + c, o);
    }
}

struct PreactBwdArgs {
    const float* x;
    const float* pre_scale;
    const float* pre_shift;
    const float* mean;
    const float* invstd;
    const float* gamma;
    const float* dA;
    double* sums;            // [2C]: sum g | sum g * xhat
    float* partial;          // deterministic mode: [gridDim.x][2C] block partials instead of atomics
    float* dx;
    int H, W, Ho, Wo, C, ldx, ldda, lddx, has_bn, accumulate, TC;
    uint32_t P;              // input pixels
    float pre_slope;
    double inv_count;
    y2_fastdiv fW, fH;
};

// gradient reaching the pre-activation of input pixel p: dA of its (pooled) output pixel, a quarter of it per window element when pooled, through the
// ReLU mask rebuilt from the forward's affine (torch: zero gradient at pre == 0)
template <int CV, bool POOL>
__device__ __forceinline__ void preact_g(const PreactBwdArgs& a, uint32_t p, int c, const float (&xv)[CV], const float (&sc)[CV], const float (&sh)[CV], float (&g)[CV]) {
    long long po = p;
    if (POOL) {
        const uint32_t r = y2_div(p, a.fW);
        const int xi = (int)(p - r * (uint32_t)a.W);
        const uint32_t b = y2_div(r, a.fH);
        const int yi = (int)(r - b * (uint32_t)a.H);
        po = ((long long)b * a.Ho + (yi >> 1)) * a.Wo + (xi >> 1);
    }
    float d[CV];
    ldv<CV>(a.dA + po * a.ldda + c, d);
#pragma unroll
    for (int e = 0; e < CV; ++e) {
        const float pre = xv[e] * sc[e] + sh[e];
        const float t = POOL ? 0.25f * d[e] : d[e];
        g[e] = pre > 0.f ? t : t * a.pre_slope;
    }
}

template <int CV, bool POOL>
__global__ __launch_bounds__(PE_THREADS) void preact_bwd_sums_kernel(const PreactBwdArgs a) {
    __shared__ double red[2][PE_THREADS * CV];
    const int TC = a.TC, cl = threadIdx.x % TC, pl = threadIdx.x / TC, TP = PE_THREADS / TC;
    const int cg = blockIdx.y * TC + cl;
    const bool active = cg * CV < a.C;
    const int c = active ? cg * CV : 0;
    float sc[CV], sh[CV], mu[CV], is[CV];
#pragma unroll
    for (int e = 0; e < CV; ++e) {
        sc[e] = a.pre_scale != nullptr ? a.pre_scale[c + e] : 1.f;
        sh[e] = a.pre_shift != nullptr ? a.pre_shift[c + e] : 0.f;
        mu[e] = a.has_bn ? a.mean[c + e] : 0.f;
        is[e] = a.has_bn ? a.invstd[c + e] : 1.f;
    }
    double s1[CV], s2[CV];
#pragma unroll
    for (int e = 0; e < CV; ++e) s1[e] = s2[e] = 0.0;
    if (active) {
        for (uint32_t p = blockIdx.x * (uint32_t)TP + pl; p < a.P; p += gridDim.x * (uint32_t)TP) {
            float xv[CV], g[CV];
            ldv<CV>(a.x + (long long)p * a.ldx + c, xv);
            preact_g<CV, POOL>(a, p, c, xv, sc, sh, g);
#pragma unroll
            for (int e = 0; e < CV; ++e) {
                s1[e] += (double)g[e];
                s2[e] += (double)g[e] * (double)((xv[e] - mu[e]) * is[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < CV; ++e) {
        red[0][threadIdx.x * CV + e] = s1[e];
        red[1][threadIdx.x * CV + e] = s2[e];
    }
    __syncthreads();
    if (pl == 0 && active) {
#pragma unroll
        for (int e = 0; e < CV; ++e) {
            double s = 0.0, q = 0.0;
            for (int i = 0; i < TP; ++i) {
                s += red[0][(i * TC + cl) * CV + e];
                q += red[1][(i * TC + cl) * CV + e];
            }
            if (a.partial != nullptr) {
                a.partial[(size_t)blockIdx.x * 2 * a.C + c + e] = (float)s;
                a.partial[(size_t)blockIdx.x * 2 * a.C + a.C + c + e] = (float)q;
            } else {
                atomicAdd(a.sums + c + e, s);
                atomicAdd(a.sums + a.C + c + e, q);
            }
        }
    }
}

template <int CV, bool POOL>
__global__ __launch_bounds__(PE_THREADS) void preact_bwd_dx_kernel(const PreactBwdArgs a) {
    const int TC = a.TC, cl = threadIdx.x % TC, pl = threadIdx.x / TC, TP = PE_THREADS / TC;
    const int c = (blockIdx.y * TC + cl) * CV;
    if (c >= a.C) return;
    float sc[CV], sh[CV], mu[CV], is[CV], gi[CV], m1[CV], m2[CV];
#pragma unroll
    for (int e = 0; e < CV; ++e) {
        sc[e] = a.pre_scale != nullptr ? a.pre_scale[c + e] : 1.f;
        sh[e] = a.pre_shift != nullptr ? a.pre_shift[c + e] : 0.f;
        mu[e] = a.has_bn ? a.mean[c + e] : 0.f;
        is[e] = a.has_bn ? a.invstd[c + e] : 1.f;
        gi[e] = a.has_bn ? a.gamma[c + e] * is[e] : 1.f;
        m1[e] = a.has_bn == 1 ? (float)(a.sums[c + e] * a.inv_count) : 0.f;
        m2[e] = a.has_bn == 1 ? (float)(a.sums[a.C + c + e] * a.inv_count) : 0.f;
    }
    for (uint32_t p = blockIdx.x * (uint32_t)TP + pl; p < a.P; p += gridDim.x * (uint32_t)TP) {
        float xv[CV], g[CV], o[CV];
        ldv<CV>(a.x + (long long)p * a.ldx + c, xv);
        preact_g<CV, POOL>(a, p, c, xv, sc, sh, g);
        float* dst = a.dx + (long long)p * a.lddx + c;
        if (a.accumulate) ldv<CV>(dst, o);
#pragma unroll
        for (int e = 0; e < CV; ++e) {
            const float d = gi[e] * (g[e] - m1[e] - (xv[e] - mu[e]) * is[e] * m2[e]);
            o[e] = a.accumulate ? o[e] + d : d;
        }
        stv<CV>(dst, o);
    }
}

inline bool pe_shape_ok(int B, int H, int W, int C, int pool, long long* Pin, long long* Pout, int* Ho, int* Wo) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (pool != 0 && pool != 1)) return false;
    if (pool && ((H | W) & 1)) return false;
    *Ho = pool ? H / 2 : H;
    *Wo = pool ? W / 2 : W;
    *Pin = (long long)B * H * W;
    *Pout = (long long)B * *Ho * *Wo;
    return *Pin < 0x7fffffffLL;          // pixel indices are 32-bit
}

inline bool vec_ptr_ok(const float* p) { return p == nullptr || y2_aligned16(p); }

}  // namespace

extern "C" int y2_preact_conv1x1_fwd(const float* x, const float* w, const float* pre_scale, const float* pre_shift, float pre_slope,
                                     const float* scale, const float* shift, float slope, float* y, double* stats,
                                     int B, int H, int W, int K, int ldx, int N, int ldy, int coff, int pool, y2_stream_t stream) {
    long long Pin, M;
    int Ho, Wo;
    if (!x || !w || !y || !pe_shape_ok(B, H, W, K, pool, &Pin, &M, &Ho, &Wo) || N <= 0 || ldx < K || coff < 0 || ldy < coff + N) return Y2_EINVAL;
    if (stats != nullptr && y2_det.on) return Y2_ENOSUP;      // deterministic mode: statistics come from y2_colstats_det, not from atomics
    const bool vec = !(K & 3) && !(ldx & 3) && y2_aligned16(x) && y2_aligned16(w) && vec_ptr_ok(pre_scale) && vec_ptr_ok(pre_shift);
    PreactGemmArgs a;
    a.x = x; a.w = w; a.pre_scale = pre_scale; a.pre_shift = pre_shift; a.scale = scale; a.shift = shift; a.y = y; a.stats = stats;
    a.M = M; a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.K = K; a.ldx = ldx; a.N = N; a.ldy = ldy; a.coff = coff;
    a.pre_slope = pre_slope; a.slope = slope;
    a.fWo = y2_make_fastdiv(Wo); a.fHo = y2_make_fastdiv(Ho);
    // tile: 128 output channels per block where the layer has them (the A operand and its pre-activation are then done once per pixel for the
    // dense layers' N = 128); 128-pixel tiles only when they still give every CU a block
    const int NT = N > 64 ? 2 : 1;
    a.gn = (N + 64 * NT - 1) / (64 * NT);
    const int MT = ((M + 127) / 128) * a.gn >= Y2_NUM_CU ? 2 : 1;
    hipStream_t s = y2_s(stream);
    if (MT == 2 && NT == 2) return launch_preact_gemm<2, 2>(a, vec, pool != 0, s);
    if (MT == 2) return launch_preact_gemm<2, 1>(a, vec, pool != 0, s);
    if (NT == 2) return launch_preact_gemm<1, 2>(a, vec, pool != 0, s);
    return launch_preact_gemm<1, 1>(a, vec, pool != 0, s);
}

extern "C" int y2_preact_fwd(const float* x, const float* pre_scale, const float* pre_shift, float pre_slope, float* out,
                             int B, int H, int W, int C, int ldx, int ldo, int pool, y2_stream_t stream) {
    long long Pin, P;
    int Ho, Wo;
    if (!x || !out || !pe_shape_ok(B, H, W, C, pool, &Pin, &P, &Ho, &Wo) || ldx < C || ldo < C) return Y2_EINVAL;
    const int CV = (!(C & 3) && !(ldx & 3) && !(ldo & 3) && y2_aligned16(x) && y2_aligned16(out)) ? 4 : 1;
    const PeGrid g = pe_grid(P, C, CV, 1);
    const dim3 grid(g.gx, g.gy), block(PE_THREADS);
    hipStream_t s = y2_s(stream);
#define Y2_PREACT_FWD(CVV, POOLV)                                                                                                                  \
    Y2_LAUNCH("preact_fwd_kernel", 0.0, (preact_fwd_kernel<CVV, POOLV>), grid, block, 0, s, x, pre_scale, pre_shift, pre_slope, out, H, W, Ho, Wo, C, ldx, ldo, \
              (uint32_t)P, y2_make_fastdiv(Wo), y2_make_fastdiv(Ho), g.TC)
    if (CV == 4 && pool) Y2_PREACT_FWD(4, true);
    else if (CV == 4) Y2_PREACT_FWD(4, false);
    else if (pool) Y2_PREACT_FWD(1, true);
    else Y2_PREACT_FWD(1, false);
#undef Y2_PREACT_FWD
    Y2_LAUNCH_CHECK();
    return Y2_OK;
}

extern "C" int y2_preact_bwd(const float* x, const float* pre_scale, const float* pre_shift, float pre_slope, const float* mean, const float* invstd,
                             const float* gamma, const float* dA, int ldda, double* sums, float* dx, int lddx, int accumulate,
                             int B, int H, int W, int C, int ldx, int pool, int has_bn, y2_stream_t stream) {
    long long P, Pout;
    int Ho, Wo;
    if (!x || !dA || !sums || !dx || !pe_shape_ok(B, H, W, C, pool, &P, &Pout, &Ho, &Wo) || ldx < C || ldda < C || lddx < C) return Y2_EINVAL;
    if (has_bn < 0 || has_bn > 2 || (has_bn && (!mean || !invstd || !gamma))) return Y2_EINVAL;
    const int CV = (!(C & 3) && !(ldx & 3) && !(ldda & 3) && !(lddx & 3) && y2_aligned16(x) && y2_aligned16(dA) && y2_aligned16(dx)) ? 4 : 1;
    const PeGrid g = pe_grid(P, C, CV, 8);
    PreactBwdArgs a;
    a.x = x; a.pre_scale = pre_scale; a.pre_shift = pre_shift; a.mean = mean; a.invstd = invstd; a.gamma = gamma; a.dA = dA; a.sums = sums;
    a.partial = nullptr; a.dx = dx;
    a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.C = C; a.ldx = ldx; a.ldda = ldda; a.lddx = lddx; a.has_bn = has_bn; a.accumulate = accumulate ? 1 : 0; a.TC = g.TC;
    a.P = (uint32_t)P; a.pre_slope = pre_slope; a.inv_count = 1.0 / (double)P;
    a.fW = y2_make_fastdiv(W); a.fH = y2_make_fastdiv(H);
    if (y2_det.on) {
        if ((size_t)g.gx * 2 * C * sizeof(float) > y2_det.bytes) return Y2_EINVAL;
        a.partial = y2_det.ws;
    }
    const dim3 grid(g.gx, g.gy), block(PE_THREADS);
    hipStream_t s = y2_s(stream);
#define Y2_PREACT_BWD(KERN, NAME)                                                                  \
    do {                                                                                           \
        if (CV == 4 && pool) Y2_LAUNCH(NAME, 0.0, (KERN<4, true>), grid, block, 0, s, a);          \
        else if (CV == 4) Y2_LAUNCH(NAME, 0.0, (KERN<4, false>), grid, block, 0, s, a);            \
        else if (pool) Y2_LAUNCH(NAME, 0.0, (KERN<1, true>), grid, block, 0, s, a);                \
        else Y2_LAUNCH(NAME, 0.0, (KERN<1, false>), grid, block, 0, s, a);                         \
        Y2_LAUNCH_CHECK();                                                                         \
    } while (0)
    Y2_PREACT_BWD(preact_bwd_sums_kernel, "preact_bwd_sums_kernel");
    if (a.partial != nullptr) {
        const int rc = y2_det_reduce_f32(a.partial, g.gx, (long long)2 * C, (long long)2 * C, sums, nullptr, s);
        if (rc != Y2_OK) return rc;
    }
    Y2_PREACT_BWD(preact_bwd_dx_kernel, "preact_bwd_dx_kernel");
#undef Y2_PREACT_BWD
    return Y2_OK;
}
