// kmeans_host_check.cpp — a stand-alone program (its own main, no HIP, no Python) that drives the bodies of both host functions of the anchor
// k-means, km_trial_host and km_assign_host of csrc/kmeans.h (y2_anchor_kmeans_host / y2_anchor_assign_host are argument checks around them), with
// random and hostile input, meant to be built with the address and undefined-behaviour sanitizers:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -I yolo2-pytorch_amd/csrc tools/kmeans_host_check.cpp -o kmeans_host_check
//   ./kmeans_host_check [runs]
//
// Every buffer (sizes, indices, every output, the lane partials) is a heap block of exactly the size the contract names, so a read or write one element
// outside is reported.  Input per run: N in 1 .. 700 (N = 1 and K = 16 are forced regularly), sizes exp(normal) or, in hostile runs, sprinkled with NaN,
// infinities, zeros, negative values and negative zeros; duplicate boxes; initial indices in range, duplicated, or - hostile - anywhere in int32.
// Checked per trial: the status is 0 .. 3; an out-of-range index gives status 3 and zeroed outputs and nothing else does; otherwise every count lies in
// [0, N], the counts add up to N and iters <= max_iter.  Per assignment: every index lies in [0, K).
#define Y2_HD inline
#include "kmeans.h"

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

}  // namespace

int main(int argc, char** argv) {
    const long long runs = argc > 1 ? atoll(argv[1]) : 20000;
    std::mt19937 rng(16);
    std::normal_distribution<double> normal(-1.5, 0.7);
    const double hostile_values[] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity(),
                                     0.0, -0.0, -0.25, 1e308, 5e-324};
    long long trials = 0, assigns = 0, by_status[4] = {0, 0, 0, 0};
    for (long long run = 0; run < runs; ++run) {
        const bool hostile = run % 3 == 0;
        const int N = run % 11 == 0 ? 1 : 1 + (int)(rng() % 700);
        const int K = run % 7 == 0 ? KM_MAX_K : 1 + (int)(rng() % KM_MAX_K);
        const int max_iter = 1 + (int)(rng() % 40);
        double* size = block<double>(2 * (size_t)N);
        for (int i = 0; i < 2 * N; ++i) size[i] = std::fmin(std::fmax(std::exp(normal(rng)), 1e-3), 1.0);
        if (run % 4 == 0)          // duplicate boxes
            for (int i = 0; i < N; ++i) {
                const int j = (int)(rng() % N);
                if (rng() % 3 == 0) { size[2 * i] = size[2 * j]; size[2 * i + 1] = size[2 * j + 1]; }
            }
        if (hostile)
            for (int i = 0; i < 2 * N; ++i)
                if (rng() % 8 == 0) size[i] = hostile_values[rng() % 8];
        int32_t* init = block<int32_t>(K);
        bool in_range = true;
        for (int k = 0; k < K; ++k) {
            init[k] = (int32_t)(rng() % N);
            if (hostile && rng() % 16 == 0) {
                const int32_t bad[] = {-1, N, N + 1, INT32_MIN, INT32_MAX, (int32_t)rng()};
                init[k] = bad[rng() % 6];
            }
            in_range = in_range && init[k] >= 0 && init[k] < N;
        }
        double* means = block<double>(2 * (size_t)K);
        int32_t* counts = block<int32_t>(K);
        int32_t* iters = block<int32_t>(1);
        int32_t* status = block<int32_t>(1);
        double* cost = block<double>(1);
        double* part = block<double>((size_t)(2 * K + 1) * KM_LANES);
        km_trial_host(size, N, K, init, max_iter, 1e-6, means, iters, status, cost, counts, part);
        ++trials;
        if (*status < 0 || *status > 3) return fail("status outside 0 .. 3", run);
        ++by_status[*status];
        if ((*status == KM_EINDEX) != !in_range) return fail("status 3 and the range of the indices disagree", run);
        long long total = 0;
        for (int k = 0; k < K; ++k) {
            if (counts[k] < 0 || counts[k] > N) return fail("a count outside [0, N]", run);
            total += counts[k];
        }
        if (*status == KM_EINDEX) {
            for (int k = 0; k < K; ++k)
                if (means[2 * k] != 0.0 || means[2 * k + 1] != 0.0) return fail("status 3 with a mean that is not zero", run);
            if (total != 0 || *iters != 0 || *cost != 0.0) return fail("status 3 with an output that is not zero", run);
        } else {
            if (total != N) return fail("the counts do not add up to N", run);
            if (*iters < 0 || *iters > max_iter || (K >= N && *iters != 0)) return fail("iters out of range", run);
            if (!hostile && !(*cost >= 0.0 && *cost <= (double)N)) return fail("cost outside [0, N] on valid sizes", run);
        }
        // the assignment against these means (zeros after status 3) and against hostile means
        for (int pass = 0; pass < 2; ++pass) {
            if (pass == 1)
                for (int k = 0; k < 2 * K; ++k)
                    if (rng() % 4 == 0) means[k] = hostile_values[rng() % 8];
            int32_t* index = block<int32_t>(N);
            double* iou = block<double>(N);
            km_assign_host(size, N, means, K, run % 5 == 0 ? nullptr : index, run % 5 == 1 ? nullptr : iou);
            ++assigns;
            if (run % 5 != 0)
                for (int i = 0; i < N; ++i)
                    if (index[i] < 0 || index[i] >= K) return fail("an assigned index outside [0, K)", run);
            free(index); free(iou);
        }
        free(size); free(init); free(means); free(counts); free(iters); free(status); free(cost); free(part);
    }
    printf("%lld trials (status 0: %lld, 1: %lld, 2: %lld, 3: %lld) and %lld assignments\n", trials, by_status[0], by_status[1], by_status[2], by_status[3], assigns);
    return 0;
}
