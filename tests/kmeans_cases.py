"""Shared by test_kmeans_cpu.py, test_gpu_kmeans.py and tools/make_golden_kmeans.py: the case table of y2_anchor_kmeans, its seeded inputs, the host
launch, and two numpy restatements of include/yolo2_hip.h's contract:

  lloyd_fixed   the contract's summation order (lane partials by cumsum over zero-filled non-members, then the tree): bit for bit what the library gives;
  lloyd_plain   nltk's shape - a cluster's members added one after the other - which differs from the library in the summation order only.

Results are computed once per case, shared, never written to."""
import os
import random

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'kmeans.npz')
LANES = 256
EPS = np.finfo(np.float64).eps
MAX_ITER, CONV_TEST = 1000, 1e-6
EINVAL, ENOSUP = -1, -3
# (N, K, R).  (5, 5, 2) and (3, 5, 1): K = N and K > N, no iteration runs; (70 000, 9, 2): every lane has more than one stride of work;
# (300, 2, 300): more workgroups than the chip has CUs
CASES = [(1000, 5, 6), (257, 1, 1), (300, 2, 4), (64, 9, 4), (5, 5, 2), (3, 5, 1), (70000, 9, 2), (300, 2, 300)]
SEED = 20          # the conditions of test_kmeans_cpu.py's comparison with lloyd_plain (best / second-best gaps, distance to conv_test) hold for it


def case_id(case):
    return 'N%d-K%d-R%d' % case


def sizes(N, seed=SEED):
    """Synthetic (height, width) box sizes: exp(N(-1.5, 0.7)) clipped to [1e-3, 1], float64 [N, 2]."""
    return np.clip(np.exp(np.random.RandomState(seed + N).normal(-1.5, 0.7, (N, 2))), 1e-3, 1.0)


def inits(N, K, R, seed=SEED):
    """int32 [R, K]: per trial the sample dimension_cluster.cluster draws; with K > N (no sample exists) any K indices."""
    rng = random.Random(seed * 1000003 + N * 31 + K)
    return np.array([rng.sample(range(N), K) if K <= N else [rng.randrange(N) for _ in range(K)] for _ in range(R)], np.int32).reshape(R, K)


_INPUTS, _HOST, _FIXED = {}, {}, {}


def inputs(case):
    if case not in _INPUTS:
        N, K, R = case
        _INPUTS[case] = (sizes(N), inits(N, K, R))
        for a in _INPUTS[case]:
            a.setflags(write=False)
    return _INPUTS[case]


def frozen(res):
    for a in res.values():
        a.setflags(write=False)
    return res


def host(size, init, max_iter=MAX_ITER, conv_test=CONV_TEST, code=0):
    """y2_anchor_kmeans_host into canary-filled outputs; returns the dict of outputs (the return code must be `code`)."""
    import _hip
    size, init = np.ascontiguousarray(size, np.float64), np.ascontiguousarray(init, np.int32)
    N, (R, K) = len(size), init.shape
    out = dict(means=np.full((R, K, 2), -7.0), iters=np.full(R, -7, np.int32), status=np.full(R, -7, np.int32), cost=np.full(R, -7.0),
               counts=np.full((R, K), -7, np.int32))
    rc = _hip.lib().y2_anchor_kmeans_host(size.ctypes.data, N, K, init.ctypes.data, R, max_iter, conv_test,
                                          *(out[k].ctypes.data for k in ('means', 'iters', 'status', 'cost', 'counts')))
    assert rc == code, rc
    return out


def host_case(case):
    if case not in _HOST:
        _HOST[case] = frozen(host(*inputs(case)))
    return _HOST[case]


def assign_host(size, means):
    import _hip
    size, means = np.ascontiguousarray(size, np.float64), np.ascontiguousarray(means, np.float64)
    index, iou = np.full(len(size), -7, np.int32), np.full(len(size), -7.0)
    rc = _hip.lib().y2_anchor_assign_host(size.ctypes.data, len(size), means.ctypes.data, len(means), index.ctypes.data, iou.ctypes.data)
    assert rc == 0, rc
    return index, iou


# ---- the contract in numpy

def iou(a, b):
    """The contract's IoU of boxes a [..., 2] and b [..., 2] (broadcast), operation by operation."""
    ih, iw = 2.0 * np.minimum(a[..., 0], b[..., 0]), 2.0 * np.minimum(a[..., 1], b[..., 1])
    inter = ih * iw
    area1, area2 = (2.0 * a[..., 0]) * (2.0 * a[..., 1]), (2.0 * b[..., 0]) * (2.0 * b[..., 1])
    return inter / np.maximum((area1 + area2) - inter, EPS)


def classify(size, means):
    """(winner [N], distance to it [N], gap to the second best [N] - inf with one mean).  argmin takes the first minimum: the lower index on a tie."""
    d = 1.0 - iou(size[:, None], means[None])
    win = np.argmin(d, 1)
    best = d[np.arange(len(size)), win]
    gap = np.full(len(size), np.inf)
    if means.shape[0] > 1:
        rest = d.copy()
        rest[np.arange(len(size)), win] = np.inf
        gap = rest.min(1) - best
    return win, best, gap


def lane_tree(values):
    """Sum of values [N] in the contract's order: lane l adds the entries i = l (mod 256) in increasing i (cumsum is sequential), then the tree."""
    pad = np.zeros((-len(values)) % LANES + len(values))
    pad[:len(values)] = values
    p = np.cumsum(pad.reshape(-1, LANES), 0)[-1]
    s = LANES // 2
    while s >= 1:
        p[:s] = p[:s] + p[s:2 * s]
        s //= 2
    return p[0]


def sum_fixed(size, member):
    return np.array([lane_tree(np.where(member, size[:, c], 0.0)) for c in range(2)])


def sum_plain(size, member):
    return np.cumsum(size[member], 0)[-1]          # nltk's _centroid: the members one after the other


def lloyd(size, init, summer, max_iter=MAX_ITER, conv_test=CONV_TEST, cost_sum=lane_tree):
    """One trial.  Returns (means, iters, status, cost, counts, smallest best / second-best gap met, the differences)."""
    N, K = len(size), len(init)
    means = size[init].copy()
    status, iters, min_gap, differences = 0, 0, np.inf, []
    if K < N:
        status = 2
        while iters < max_iter:
            win, _, gap = classify(size, means)
            min_gap = min(min_gap, gap.min())
            counts = np.bincount(win, minlength=K)
            if (counts == 0).any():
                status = 1
                break
            new = np.stack([summer(size, win == k) / float(counts[k]) for k in range(K)])
            difference = 0.0
            for k in range(K):
                difference = difference + (1.0 - iou(means[k], new[k]))
            differences.append(float(difference))
            means = new
            iters += 1
            if difference < conv_test:
                status = 0
                break
    win, best, gap = classify(size, means)
    if K < N:
        min_gap = min(min_gap, gap.min())
    return means, iters, status, cost_sum(best), np.bincount(win, minlength=K).astype(np.int32), min_gap, differences


def run(case_inputs, summer, cost_sum=lane_tree, **kw):
    size, init = case_inputs
    trials = [lloyd(size, row, summer, cost_sum=cost_sum, **kw) for row in init]
    res = dict(means=np.stack([t[0] for t in trials]), iters=np.array([t[1] for t in trials], np.int32), status=np.array([t[2] for t in trials], np.int32),
               cost=np.array([t[3] for t in trials]), counts=np.stack([t[4] for t in trials]), min_gap=np.array([t[5] for t in trials]),
               differences=np.concatenate([t[6] for t in trials] + [np.zeros(0)]))
    return frozen(res)


def fixed_case(case):
    if case not in _FIXED:
        _FIXED[case] = run(inputs(case), sum_fixed)
    return _FIXED[case]


def plain(case_inputs):
    return run(case_inputs, sum_plain, cost_sum=lambda v: np.cumsum(v)[-1])
