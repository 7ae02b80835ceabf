// kmeans.hip — choosing anchors on the device: y2_anchor_kmeans and y2_anchor_assign (include/yolo2_hip.h).  The arithmetic is csrc/kmeans.h, shared
// with the host functions.
//
// kmeans_kernel: ONE workgroup of KM_LANES = 256 threads per trial, the whole Lloyd loop inside the launch; trials never talk to each other (no
// cooperative launch, no floating-point atomics).  The K means live in LDS and are read as broadcasts; the boxes are re-read from memory every
// iteration (16 bytes per box, lane-contiguous: one 4-KB line set per step of the workgroup, served by the last-level cache after the first pass).
// Thread t IS lane partial t of the contract: it adds the boxes i = t (mod 256) in increasing i into per-cluster registers, PREDICATED - every
// cluster's partial takes the box or +0.0 (km_accumulate) - because a register array indexed by the run-time winner would live in scratch.  The
// kernel is instantiated for KC = 4, 8, 12, 16 clusters' worth of registers and the launcher takes the smallest that holds K.
// The tree of the contract (s = 128, 64 through LDS; s = 32 ... 1 inside wave 0 with lane shuffles: at step s only lanes below 2 s hold partials that
// are still read, and lane l < s reads lane l + s < 2 s) leaves the totals in thread 0, which alone computes the new means, the difference and the
// verdict, and broadcasts the verdict through LDS: every thread takes the same number of trips through every barrier and leaves the loop together.
// Member counts are integers (any order gives the same sum): LDS integer atomics.
#include "common.h"
#include "kmeans.h"

namespace {

struct KmArgs {
    const double* size; const int32_t* init; double* means; int32_t* iters; int32_t* status; double* cost; int32_t* counts;
    double conv_test; int32_t N, K, max_iter;
};

// the contract's tree over the 256 lane partials of Q quantities at once; the totals arrive in thread 0.  red: [Q][128] doubles of LDS, free again
// on return.  Every thread of the workgroup calls it.
template <int Q>
__device__ inline void km_reduce(double (&v)[Q], double* red, int t) {
    if (t >= 128) {
#pragma unroll
        for (int q = 0; q < Q; ++q) red[q * 128 + (t - 128)] = v[q];
    }
    __syncthreads();
    if (t < 128) {
#pragma unroll
        for (int q = 0; q < Q; ++q) v[q] += red[q * 128 + t];
    }
    __syncthreads();
    if (t >= 64 && t < 128) {
#pragma unroll
        for (int q = 0; q < Q; ++q) red[q * 128 + (t - 64)] = v[q];
    }
    __syncthreads();
    if (t < 64) {
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            v[q] += red[q * 128 + t];
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) v[q] += __shfl_down(v[q], s, 64);
        }
    }
    __syncthreads();
}

template <int KC>
__global__ __launch_bounds__(KM_LANES) void kmeans_kernel(const KmArgs a) {
    __shared__ double mean[2 * KM_MAX_K];
    __shared__ double sum[2 * KM_MAX_K];
    __shared__ double red[KC * 128];
    __shared__ int32_t count[KM_MAX_K];
    __shared__ int32_t verdict[2];          // [0]: an initial index is out of range; [1]: what the iteration ended with (0 go on, 1 empty cluster, 2 converged)
    const int r = blockIdx.x, t = threadIdx.x, N = a.N, K = a.K;
    if (t < 2) verdict[t] = 0;
    __syncthreads();
    int idx = 0;
    if (t < K) {
        idx = a.init[(size_t)r * K + t];
        if (idx < 0 || idx >= N) verdict[0] = 1;
    }
    __syncthreads();
    if (verdict[0]) {          // (uniform) nothing of `size` was read
        if (t < K) {
            a.means[2 * ((size_t)r * K + t)] = 0.0;
            a.means[2 * ((size_t)r * K + t) + 1] = 0.0;
            a.counts[(size_t)r * K + t] = 0;
        }
        if (t == 0) { a.iters[r] = 0; a.status[r] = KM_EINDEX; a.cost[r] = 0.0; }
        return;
    }
    if (t < K) {
        mean[2 * t] = a.size[2 * (size_t)idx];
        mean[2 * t + 1] = a.size[2 * (size_t)idx + 1];
    }
    __syncthreads();
    int st = KM_OK, it = 0;
    if (K < N) {          // (uniform) nltk's num_means < len(vectors) guard
        st = KM_EITER;
        while (it < a.max_iter) {
            double sh[KC], sw[KC];
            int32_t cnt[KC];
#pragma unroll
            for (int c = 0; c < KC; ++c) { sh[c] = 0.0; sw[c] = 0.0; cnt[c] = 0; }
            if (t < KM_MAX_K) count[t] = 0;
            long long i = t;
            double h = 0.0, w = 0.0;
            if (i < N) { h = a.size[2 * i]; w = a.size[2 * i + 1]; }
            while (i < N) {          // the next box is on its way while this one is classified
                const long long j = i + KM_LANES;
                double nh = 0.0, nw = 0.0;
                if (j < N) { nh = a.size[2 * j]; nw = a.size[2 * j + 1]; }
                double best;
                const int win = km_classify(h, w, mean, K, best);
                km_accumulate<KC>(sh, sw, cnt, win, h, w);
                h = nh; w = nw; i = j;
            }
            km_reduce<KC>(sh, red, t);
            km_reduce<KC>(sw, red, t);
#pragma unroll
            for (int c = 0; c < KC; ++c)
                if (cnt[c]) atomicAdd(&count[c], cnt[c]);          // (zeroed before the barriers of km_reduce)
            if (t == 0) {
#pragma unroll
                for (int c = 0; c < KC; ++c) { sum[2 * c] = sh[c]; sum[2 * c + 1] = sw[c]; }
            }
            __syncthreads();
            if (t == 0) {
                double difference = 0.0;
                const int rc = km_update(mean, sum, count, K, difference);
                verdict[1] = rc != KM_OK ? 1 : (difference < a.conv_test ? 2 : 0);
            }
            __syncthreads();
            const int v = verdict[1];          // the same value in every thread: the loop is left by all or by none
            if (v == 1) { st = KM_EEMPTY; break; }
            ++it;
            if (v == 2) { st = KM_OK; break; }
        }
    }
    // the final pass: counts and cost against the final means
    double pc[1] = {0.0};
    int32_t cnt[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) cnt[c] = 0;
    if (t < KM_MAX_K) count[t] = 0;
    for (long long i = t; i < N; i += KM_LANES) {
        double best;
        const int win = km_classify(a.size[2 * i], a.size[2 * i + 1], mean, K, best);
        pc[0] += best;
#pragma unroll
        for (int c = 0; c < KC; ++c) cnt[c] += c == win ? 1 : 0;
    }
    km_reduce<1>(pc, red, t);
#pragma unroll
    for (int c = 0; c < KC; ++c)
        if (cnt[c]) atomicAdd(&count[c], cnt[c]);
    __syncthreads();
    if (t < K) {
        a.means[2 * ((size_t)r * K + t)] = mean[2 * t];
        a.means[2 * ((size_t)r * K + t) + 1] = mean[2 * t + 1];
        a.counts[(size_t)r * K + t] = count[t];
    }
    if (t == 0) { a.iters[r] = it; a.status[r] = st; a.cost[r] = pc[0]; }
}

__global__ __launch_bounds__(256) void anchor_assign_kernel(const double* size, int N, const double* means, int K, int32_t* index, double* iou) {
    __shared__ double mean[2 * KM_MAX_K];
    const int t = threadIdx.x;
    if (t < 2 * K) mean[t] = means[t];
    __syncthreads();
    for (long long i = (long long)blockIdx.x * 256 + t; i < N; i += (long long)gridDim.x * 256) {
        double best;
        const double h = size[2 * i], w = size[2 * i + 1];
        const int win = km_classify(h, w, mean, K, best);
        if (index) index[i] = win;
        if (iou) iou[i] = km_iou(h, w, mean[2 * win], mean[2 * win + 1]);
    }
}

}  // namespace

static_assert(Y2_KMEANS_MAX_K == KM_MAX_K, "include/yolo2_hip.h and csrc/kmeans.h disagree");

extern "C" int y2_anchor_kmeans(const double* size, int32_t N, int32_t K, const int32_t* init, int32_t R, int32_t max_iter, double conv_test,
                                double* means, int32_t* iters, int32_t* status, double* cost, int32_t* counts, y2_stream_t stream) {
    if (N <= 0 || K <= 0 || R <= 0 || max_iter <= 0) return Y2_EINVAL;
    if (!size || !init || !means || !iters || !status || !cost || !counts) return Y2_EINVAL;
    if (K > Y2_KMEANS_MAX_K || R > 65535) return Y2_ENOSUP;
    if ((reinterpret_cast<uintptr_t>(size) | reinterpret_cast<uintptr_t>(means) | reinterpret_cast<uintptr_t>(cost)) & 7u) return Y2_EALIGN;
    KmArgs a;
    a.size = size; a.init = init; a.means = means; a.iters = iters; a.status = status; a.cost = cost; a.counts = counts;
    a.conv_test = conv_test; a.N = N; a.K = K; a.max_iter = max_iter;
    if (K <= 4) Y2_LAUNCH("kmeans_kernel<4>", 0.0, kmeans_kernel<4>, dim3(R), dim3(KM_LANES), 0, y2_s(stream), a);
    else if (K <= 8) Y2_LAUNCH("kmeans_kernel<8>", 0.0, kmeans_kernel<8>, dim3(R), dim3(KM_LANES), 0, y2_s(stream), a);
    else if (K <= 12) Y2_LAUNCH("kmeans_kernel<12>", 0.0, kmeans_kernel<12>, dim3(R), dim3(KM_LANES), 0, y2_s(stream), a);
    else Y2_LAUNCH("kmeans_kernel<16>", 0.0, kmeans_kernel<16>, dim3(R), dim3(KM_LANES), 0, y2_s(stream), a);
    Y2_LAUNCH_CHECK();
    return Y2_OK;
}

extern "C" int y2_anchor_assign(const double* size, int32_t N, const double* means, int32_t K, int32_t* index, double* iou, y2_stream_t stream) {
    if (N <= 0 || K <= 0 || !size || !means) return Y2_EINVAL;
    if (K > Y2_KMEANS_MAX_K) return Y2_ENOSUP;
    if ((reinterpret_cast<uintptr_t>(size) | reinterpret_cast<uintptr_t>(means) | reinterpret_cast<uintptr_t>(iou)) & 7u) return Y2_EALIGN;
    if (!index && !iou) return Y2_OK;
    const int grid = std::min(y2_cdiv(N, 256), 4096);
    Y2_LAUNCH("anchor_assign_kernel", 0.0, anchor_assign_kernel, dim3(grid), dim3(256), 0, y2_s(stream), size, (int)N, means, (int)K, index, iou);
    Y2_LAUNCH_CHECK();
    return Y2_OK;
}
