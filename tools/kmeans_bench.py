#!/usr/bin/env python
"""Timing of the anchor k-means (y2_anchor_kmeans, dimension_cluster.cluster) on one MI355X; prints ONE JSON line.  Nothing is asserted on the numbers.

Workload: seeded synthetic box sizes, exp(N(-1.5, 0.7)) clipped to [1e-3, 1], at a VOC-like size (N = 40 000, K = 5) and a COCO-like size (N = 860 000,
K = 9), with R = 1, 256 and 4096 trials per launch, every trial from its own random sample.  Per shape and R, `--runs` times (default 2) in the process:
  fixed     every trial runs exactly `--iters` Lloyd iterations (conv_test = -1 never holds; status 2), so the work of a launch is known: the median
            HIP-event time over the timed launches, min and max, trials per second, ms per trial and ns per box, mean and iteration (N K distances each)
  converged R = 256 only: the reference's conv_test 1e-6 with max_iter 1000: the iterations the trials took, the failures, ms per trial, the best mean IoU
and once per shape
  host      y2_anchor_kmeans_host, ONE trial of `--iters` iterations on one core of this machine (a host clock)
  python    nltk's inner loop - distance(vector, mean) as a Python call per box and mean - timed on `--python-calls` calls and EXTRAPOLATED to one
            trial of `--iters` iterations (N K calls per iteration); labelled as such
  cluster_s dimension_cluster.cluster(data on the GPU, K, repeats=256) end to end, selection on the host included (a host clock)
The device's outputs for R = 1 are compared with the host function's once per shape (bit for bit).
    python tools/kmeans_bench.py [--shapes 40000x5,860000x9] [--trials 1,256,4096] [--iters 16] [--launches 5] [--runs 2]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'yolo2-pytorch_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

KEYS = ('means', 'iters', 'status', 'cost', 'counts')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='40000x5,860000x9')
    ap.add_argument('--trials', default='1,256,4096')
    ap.add_argument('--iters', type=int, default=16)
    ap.add_argument('--launches', type=int, default=5)
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--python-calls', type=int, default=20000)
    args = ap.parse_args()
    import numpy as np
    import torch

    import _hip
    import dimension_cluster
    assert torch.cuda.is_available(), 'kmeans_bench.py measures on an MI355X'
    dev = torch.device('cuda', 0)
    L = _hip.lib()
    res = dict(device=torch.cuda.get_device_name(0), lib=os.path.basename(_hip.LIB_PATH), iters=args.iters, launches=args.launches)

    def launch(size, init, out, max_iter, conv_test):
        R, K = init.shape
        _hip.check(L.y2_anchor_kmeans(size.data_ptr(), size.size(0), K, init.data_ptr(), R, max_iter, conv_test, *(out[k].data_ptr() for k in KEYS), _hip.stream()), 'y2_anchor_kmeans')

    def outputs(R, K, where):
        return dict(means=torch.empty(R, K, 2, dtype=torch.float64, device=where), iters=torch.empty(R, dtype=torch.int32, device=where),
                    status=torch.empty(R, dtype=torch.int32, device=where), cost=torch.empty(R, dtype=torch.float64, device=where),
                    counts=torch.empty(R, K, dtype=torch.int32, device=where))

    def timed(size, init, out, max_iter, conv_test, launches):
        ms = []
        for _ in range(launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch(size, init, out, max_iter, conv_test)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    for shape in args.shapes.split(','):
        N, K = (int(v) for v in shape.split('x'))
        host_size = np.clip(np.exp(np.random.RandomState(N).normal(-1.5, 0.7, (N, 2))), 1e-3, 1.0)
        size = torch.from_numpy(host_size).to(dev)
        rng = random.Random(N)
        entry = dict(N=N, K=K)
        for R in (int(v) for v in args.trials.split(',')):
            host_init = np.array([rng.sample(range(N), K) for _ in range(R)], np.int32)
            init, out = torch.from_numpy(host_init).to(dev), outputs(R, K, dev)
            launch(size, init, out, 2, -1.0)          # warm-up: the code object, the boxes into the last-level cache
            torch.cuda.synchronize()
            runs = []
            for _ in range(args.runs):
                ms = timed(size, init, out, args.iters, -1.0, args.launches if R < 4096 else max(2, args.launches // 2))
                m = statistics.median(ms)
                done = out['iters'].cpu().numpy()
                run = dict(fixed_ms=round(m, 4), fixed_ms_min_max=[round(min(ms), 4), round(max(ms), 4)], trials_per_s=round(R / m * 1e3, 2),
                           ms_per_trial=round(m / R, 5), ns_per_box_mean_iteration=round(m * 1e6 / (R * float(done.mean()) * N * K), 4),
                           iterations_run=[int(done.min()), int(done.max())])
                if R == 256:
                    ms = timed(size, init, out, 1000, 1e-6, 2)
                    m = statistics.median(ms)
                    it, st, cost = (out[k].cpu().numpy() for k in ('iters', 'status', 'cost'))
                    run['converged'] = dict(ms=round(m, 3), ms_per_trial=round(m / R, 4), trials_per_s=round(R / m * 1e3, 2), iters_min_median_max=[int(it.min()), float(np.median(it)), int(it.max())],
                                            failed=int((st != 0).sum()), best_mean_iou=round(float(1 - cost[st == 0].min() / N), 5) if (st == 0).any() else None)
                runs.append(run)
            entry['R%d' % R] = runs
            if R == 1:          # the same trial on the host: one core, a host clock; and the bytes compared
                want = outputs(1, K, 'cpu')
                t0 = time.perf_counter()
                _hip.check(L.y2_anchor_kmeans_host(host_size.ctypes.data, N, K, host_init.ctypes.data, 1, args.iters, -1.0, *(want[k].data_ptr() for k in KEYS)), 'y2_anchor_kmeans_host')
                entry['host_one_core_ms_per_trial'] = round((time.perf_counter() - t0) * 1e3, 2)
                entry['device_equals_host'] = all(torch.equal(out[k].cpu(), want[k]) for k in KEYS)
        # nltk's inner loop: one Python call of `distance` per box and mean
        means = host_size[:K].copy()
        calls, t0 = 0, time.perf_counter()
        while calls < args.python_calls:
            vector = host_size[calls // K % N]
            for mean in means:
                dimension_cluster.distance(vector, mean)
            calls += K
        per_call = (time.perf_counter() - t0) / calls
        entry['python_us_per_distance_call'] = round(per_call * 1e6, 3)
        entry['python_ms_per_trial_extrapolated'] = round(per_call * N * K * args.iters * 1e3, 1)
        t0 = time.perf_counter()
        got = dimension_cluster.cluster(size, K, repeats=256, seed=N)
        entry['cluster_s'] = round(time.perf_counter() - t0, 3)
        entry['cluster'] = dict(mean_iou=round(float(got['iou']), 5), failed=int((got['status'] != 0).sum()), counts=got['counts'].tolist())
        res[shape] = entry
    print(json.dumps(res))


if __name__ == '__main__':
    main()
