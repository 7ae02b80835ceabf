"""Writes tests/golden/kmeans.npz: for three small cases of tests/kmeans_cases.py the seeded synthetic box sizes (exp(N(-1.5, 0.7)) clipped to
[1e-3, 1]), the initial indices of every trial and what the PLAIN restatement of include/yolo2_hip.h's k-means gives - nltk's shape, a cluster's
members added one after the other (kmeans_cases.lloyd_plain) - as means, iters, status, cost and counts.  numpy only; needs neither the library nor a
GPU.  The library sums in another, fixed order: tests compare within the bound that difference allows (test_kmeans_cpu.py).

    python tools/make_golden_kmeans.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import kmeans_cases as km  # noqa: E402

GOLDEN_CASES = [(1000, 5, 6), (300, 2, 4), (64, 9, 4)]


def main():
    out = {}
    for case in GOLDEN_CASES:
        size, init = km.inputs(case)
        res = km.plain((size, init))
        assert (res['status'] == 0).all(), case
        name = km.case_id(case)
        out[name + '.size'], out[name + '.init'] = size, init
        for k in ('means', 'iters', 'status', 'cost', 'counts'):
            out[name + '.' + k] = res[k]
        print('%s: iters %s, mean IoU %s' % (name, res['iters'].tolist(), np.round(1 - res['cost'] / case[0], 4).tolist()))
    np.savez_compressed(km.GOLDEN, **out)
    print('wrote %s (%d bytes)' % (km.GOLDEN, os.path.getsize(km.GOLDEN)))


if __name__ == '__main__':
    main()
