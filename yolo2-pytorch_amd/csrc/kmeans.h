// kmeans.h — k-means on the distance 1 - IoU over box sizes (dimension_cluster.py: choosing a dataset's anchors), ONE copy of the arithmetic for the
// device kernels (kmeans.hip) and the host functions (host.hip).  The contract is stated in include/yolo2_hip.h (y2_anchor_kmeans): fp64, one rounding
// per operation (the library is built with -ffp-contract=off), and a summation order that is fixed independently of how a kernel is launched -
// KM_LANES lane partials, lane l adding the members i = l (mod KM_LANES) in increasing i, then a halving tree.
//
// Safety: a box index comes from a loop bound, an initial index is range-checked before it is used, a winner is an integer in [0, K) whatever the
// values are (NaN compares false and leaves index 0) - no value read from `size` or `means` is ever used as an index.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef Y2_HD
#define Y2_HD __host__ __device__ inline
#endif

#define KM_MAX_K 16
#define KM_LANES 256
#define KM_EPS 2.220446049250313e-16          // DBL_EPSILON: utils/iou/numpy.py's default `min` for float64

// status of one trial (y2_anchor_kmeans: status[r])
enum { KM_OK = 0, KM_EEMPTY = 1 /* a cluster lost all its members */, KM_EITER = 2 /* max_iter iterations without convergence */,
       KM_EINDEX = 3 /* an initial index outside [0, N): nothing was read, the outputs are zero */ };

// np.minimum / np.maximum: a NaN operand is the result
Y2_HD double km_min(double a, double b) { return (a < b || a != a) ? a : b; }
Y2_HD double km_max(double a, double b) { return (a > b || a != a) ? a : b; }

// IoU of two boxes centred on the origin with half-extents (ah, aw) and (bh, bw): utils/iou/numpy.py:iou(-a, a, -b, b) in its operation order.
// min(a, b) - max(-a, -b) is exactly 2 min(a, b), and the extent a - (-a) exactly 2 a.
Y2_HD double km_iou(double ah, double aw, double bh, double bw) {
    const double ih = 2.0 * km_min(ah, bh), iw = 2.0 * km_min(aw, bw);
    const double inter = ih * iw;
    const double area1 = (2.0 * ah) * (2.0 * aw), area2 = (2.0 * bh) * (2.0 * bw);
    const double uni = km_max((area1 + area2) - inter, KM_EPS);
    return inter / uni;
}
Y2_HD double km_dist(double ah, double aw, double bh, double bw) { return 1.0 - km_iou(ah, aw, bh, bw); }

// nltk's classify_vectorspace: mean 0 unconditionally, a later mean only when strictly closer (ties and NaN stay with the lower index).
// means [K][2]; returns the winner in [0, K) for K >= 1 and its distance in `best`.
Y2_HD int km_classify(double h, double w, const double* means, int K, double& best) {
    int win = 0;
    best = km_dist(h, w, means[0], means[1]);
    for (int k = 1; k < K; ++k) {
        const double d = km_dist(h, w, means[2 * k], means[2 * k + 1]);
        if (d < best) { best = d; win = k; }
    }
    return win;
}

// One step of one lane's partials, in the predicated form a kernel keeps in registers: every cluster's partial takes the box or +0.0.  Adding +0.0
// is bit-identical to skipping (a partial starts at +0.0 and can never become -0.0), so code that indexes by the winner instead - the host
// function - gives the same bits.
template <int KC>
Y2_HD void km_accumulate(double (&sh)[KC], double (&sw)[KC], int32_t (&cnt)[KC], int win, double h, double w) {
#pragma unroll
    for (int c = 0; c < KC; ++c) {
        const bool mine = c == win;
        sh[c] += mine ? h : 0.0;
        sw[c] += mine ? w : 0.0;
        cnt[c] += mine ? 1 : 0;
    }
}

// the tree over the lane partials: for s = KM_LANES / 2 ... 1: p[l] += p[l + s] for l < s; the sum is p[0]
Y2_HD double km_tree(double* p) {
    for (int s = KM_LANES / 2; s >= 1; s >>= 1)
        for (int l = 0; l < s; ++l) p[l] += p[l + s];
    return p[0];
}

// The end of one iteration, one thread's work: the verdict on empty clusters, the new means, difference = sum_k dist(old_k, new_k) in increasing k
// from 0.0.  sum [K][2] and count [K] are the reduced totals.  Returns KM_EEMPTY and leaves `means` alone, or KM_OK with the means replaced and
// `difference` set.
Y2_HD int km_update(double* means, const double* sum, const int32_t* count, int K, double& difference) {
    for (int k = 0; k < K; ++k)
        if (count[k] <= 0) return KM_EEMPTY;
    double diff = 0.0;
    for (int k = 0; k < K; ++k) {
        const double nh = sum[2 * k] / (double)count[k], nw = sum[2 * k + 1] / (double)count[k];
        diff += km_dist(means[2 * k], means[2 * k + 1], nh, nw);
        means[2 * k] = nh;
        means[2 * k + 1] = nw;
    }
    difference = diff;
    return KM_OK;
}

// ---- the host functions' bodies (host.hip checks the arguments; tools/kmeans_host_check.cpp calls these directly)

// One trial.  init [K]; means [K][2], counts [K]; the lane partials live in `part` [(2 K + 1) * KM_LANES] doubles of the caller.
inline void km_trial_host(const double* size, int N, int K, const int32_t* init, int max_iter, double conv_test,
                          double* means, int32_t* iters, int32_t* status, double* cost, int32_t* counts, double* part) {
    *iters = 0;
    *cost = 0.0;
    for (int k = 0; k < K; ++k) { means[2 * k] = means[2 * k + 1] = 0.0; counts[k] = 0; }
    for (int k = 0; k < K; ++k)
        if (init[k] < 0 || init[k] >= N) { *status = KM_EINDEX; return; }
    for (int k = 0; k < K; ++k) {
        means[2 * k] = size[2 * (size_t)init[k]];
        means[2 * k + 1] = size[2 * (size_t)init[k] + 1];
    }
    int st = KM_OK, it = 0;
    if (K < N) {
        st = KM_EITER;
        double sum[2 * KM_MAX_K];
        while (it < max_iter) {
            for (int q = 0; q < 2 * K * KM_LANES; ++q) part[q] = 0.0;
            for (int k = 0; k < K; ++k) counts[k] = 0;
            for (int i = 0; i < N; ++i) {          // increasing i: every lane's partial meets its members in increasing i
                double best;
                const double h = size[2 * (size_t)i], w = size[2 * (size_t)i + 1];
                const int win = km_classify(h, w, means, K, best);
                part[(2 * win) * KM_LANES + (i & (KM_LANES - 1))] += h;
                part[(2 * win + 1) * KM_LANES + (i & (KM_LANES - 1))] += w;
                ++counts[win];
            }
            for (int q = 0; q < 2 * K; ++q) sum[q] = km_tree(part + q * KM_LANES);
            double difference;
            if (km_update(means, sum, counts, K, difference) != KM_OK) { st = KM_EEMPTY; break; }
            ++it;
            if (difference < conv_test) { st = KM_OK; break; }
        }
    }
    // the final pass: counts and cost against the final means
    double* pc = part + 2 * K * KM_LANES;
    for (int l = 0; l < KM_LANES; ++l) pc[l] = 0.0;
    for (int k = 0; k < K; ++k) counts[k] = 0;
    for (int i = 0; i < N; ++i) {
        double best;
        const int win = km_classify(size[2 * (size_t)i], size[2 * (size_t)i + 1], means, K, best);
        pc[i & (KM_LANES - 1)] += best;
        ++counts[win];
    }
    *cost = km_tree(pc);
    *iters = it;
    *status = st;
}

inline void km_assign_host(const double* size, int N, const double* means, int K, int32_t* index, double* iou) {
    for (int i = 0; i < N; ++i) {
        double best;
        const double h = size[2 * (size_t)i], w = size[2 * (size_t)i + 1];
        const int win = km_classify(h, w, means, K, best);
        if (index) index[i] = win;
        if (iou) iou[i] = km_iou(h, w, means[2 * win], means[2 * win + 1]);
    }
}
