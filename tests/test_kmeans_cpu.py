"""Anchor k-means without a GPU: y2_anchor_kmeans_host and y2_anchor_assign_host (the host functions share csrc/kmeans.h with the device kernels)
against the numpy restatements of tests/kmeans_cases.py, the status paths, and the Python layer: dimension_cluster.cluster / get_data / main,
utils.iou.numpy.iou, utils.image_size."""
import configparser
import os
import pickle
import random

import numpy as np
import pytest

import _hip
import dimension_cluster
import jpeg_cases as jp
import kmeans_cases as km
import utils

KEYS = ('means', 'iters', 'status', 'cost', 'counts')
SMALL = [c for c in km.CASES if c[0] <= 1000]


# ---- 1. bit for bit against the fixed summation order

@pytest.mark.parametrize('case', km.CASES, ids=km.case_id)
def test_host_equals_the_fixed_order_restatement(case):
    got, want = km.host_case(case), km.fixed_case(case)
    assert (want['status'] == 0).all()          # the table's cases converge, no cluster runs empty
    assert ((want['iters'] == 0) == (case[1] >= case[0])).all()          # K >= N: no iteration runs
    for k in KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert (got['counts'].sum(1) == case[0]).all()


# ---- 2. against the plain, nltk-shaped restatement (members added one after the other): only the summation order differs

@pytest.mark.parametrize('case', SMALL, ids=km.case_id)
def test_host_against_the_plain_restatement(case):
    """A centroid is a sum of at most N sizes in (0, 1] divided by their number; two summation orders of the same members differ by at most
    2 (N - 1) u sum|x| / n <= 2 N 2^-53 per component (u = 2^-53).  That holds as long as both sides assign every box alike and take the same
    verdicts, which the two conditions on the restatement guarantee: a best / second-best gap above 1e-10 and no difference within 1e-9 of
    conv_test are orders of magnitude beyond what a perturbation of 2 N 2^-53 <= 2.3e-13 of the means can move.
    The cost (a sum of N distances in [0, 1]) differs by the summation order, at most N^2 2^-53, and by the perturbed means: a relative
    perturbation d / m of one component of a mean moves the intersection and the mean's area by at most that factor each, the IoU (<= 1) by at
    most 4 d / m, so the cost by at most N * 4 * (2 N 2^-53) / 1e-3 (no component of a mean is below the smallest size, 1e-3)."""
    N, K, R = case
    want = km.plain(km.inputs(case))
    assert want['min_gap'].min() > 1e-10
    assert len(want['differences']) == 0 or np.abs(want['differences'] - km.CONV_TEST).min() > 1e-9
    got = km.host_case(case)
    np.testing.assert_array_equal(got['iters'], want['iters'])
    np.testing.assert_array_equal(got['status'], want['status'])
    np.testing.assert_array_equal(got['counts'], want['counts'])
    err = np.abs(got['means'] - want['means']).max()
    cost_err = np.abs(got['cost'] - want['cost']).max()
    print('%s: mean error %.3g (bound %.3g), cost error %.3g' % (km.case_id(case), err, 2 * N * 2.0 ** -53, cost_err))
    assert err <= 2 * N * 2.0 ** -53
    assert cost_err <= N * N * 2.0 ** -53 + N * 4 * (2 * N * 2.0 ** -53) / 1e-3


def test_golden_file_holds_the_plain_results_of_today(golden):
    """tests/golden/kmeans.npz (tools/make_golden_kmeans.py) against the inputs the tests generate and the host function, within the same bound."""
    g = golden('kmeans')
    for case in [(1000, 5, 6), (300, 2, 4), (64, 9, 4)]:
        name = km.case_id(case)
        size, init = km.inputs(case)
        np.testing.assert_array_equal(g[name + '.size'], size)
        np.testing.assert_array_equal(g[name + '.init'], init)
        got = km.host_case(case)
        for k in ('iters', 'status', 'counts'):
            np.testing.assert_array_equal(got[k], g[name + '.' + k], err_msg=k)
        assert np.abs(got['means'] - g[name + '.means']).max() <= 2 * case[0] * 2.0 ** -53


# ---- 3. status paths

def test_identical_initial_means_leave_a_cluster_empty():
    size = km.sizes(100).copy()
    size[7] = size[3]
    init = np.array([[3, 7, 11], [3, 11, 20]], np.int32)
    got = km.host(size, init)
    assert got['status'].tolist() == [1, 0] and got['iters'][0] == 0
    np.testing.assert_array_equal(got['means'][0], size[init[0]])          # the means the failing iteration started from
    assert got['counts'][0, 1] == 0 and got['counts'][0].sum() == 100          # the final pass: every tie went to the lower index
    want = km.run((size, init), km.sum_fixed)
    for k in KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_iteration_limit():
    case = (1000, 5, 6)
    size, init = km.inputs(case)
    assert km.host_case(case)['iters'].min() > 3
    got, want = km.host(size, init, max_iter=3), km.run((size, init), km.sum_fixed, max_iter=3)
    assert got['status'].tolist() == [2] * 6 and got['iters'].tolist() == [3] * 6
    for k in KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert km.host(size, init, max_iter=1)['status'].tolist() == [2] * 6


@pytest.mark.parametrize('bad', [-1, 300])
def test_initial_index_out_of_range(bad):
    size, init = km.inputs((300, 2, 4))
    init = init.copy()
    init[2, 1] = bad
    got, want = km.host(size, init), km.host_case((300, 2, 4))
    assert got['status'].tolist() == [0, 0, 3, 0]
    assert not got['means'][2].any() and not got['counts'][2].any() and got['iters'][2] == 0 and got['cost'][2] == 0
    for k in KEYS:          # the other trials are not affected
        np.testing.assert_array_equal(np.delete(got[k], 2, 0), np.delete(want[k], 2, 0), err_msg=k)


def test_argument_errors():
    size = km.sizes(64)
    out = km.host(size, np.zeros((1, 17), np.int32), code=km.ENOSUP)
    assert all((out[k] == -7).all() for k in KEYS)          # nothing was written
    lib, init, m = _hip.lib(), np.zeros((1, 2), np.int32), np.zeros((1, 2, 2))
    i32, f64 = np.zeros(2, np.int32), np.zeros(1)
    args = lambda N, K, R, it, size_p=size.ctypes.data: (size_p, N, K, init.ctypes.data, R, it, 1e-6, m.ctypes.data, i32.ctypes.data, i32.ctypes.data, f64.ctypes.data, i32.ctypes.data)
    assert lib.y2_anchor_kmeans_host(*args(0, 2, 1, 10)) == km.EINVAL
    assert lib.y2_anchor_kmeans_host(*args(64, 0, 1, 10)) == km.EINVAL
    assert lib.y2_anchor_kmeans_host(*args(64, 2, 0, 10)) == km.EINVAL
    assert lib.y2_anchor_kmeans_host(*args(64, 2, 1, 0)) == km.EINVAL
    assert lib.y2_anchor_kmeans_host(*args(64, 2, 1, 10, None)) == km.EINVAL
    assert lib.y2_anchor_kmeans_host(*args(64, 2, 65536, 10)) == km.ENOSUP
    assert lib.y2_anchor_assign_host(size.ctypes.data, 0, m.ctypes.data, 1, None, None) == km.EINVAL
    assert lib.y2_anchor_assign_host(size.ctypes.data, 64, m.ctypes.data, 17, None, None) == km.ENOSUP
    assert _hip.KMEANS_MAX_K == 16


# ---- 4. y2_anchor_assign_host

def test_assign_against_numpy():
    case = (1000, 5, 6)
    size, means = km.inputs(case)[0], km.host_case(case)['means'][0]
    index, iou = km.assign_host(size, means)
    win, best, _ = km.classify(size, means)
    np.testing.assert_array_equal(index, win)
    np.testing.assert_array_equal(iou, km.iou(size, means[win]))
    np.testing.assert_array_equal(1 - iou, best)
    np.testing.assert_array_equal(dimension_cluster.distance(size, means[win]), best)          # utils.iou.numpy.iou: the same operation order
    np.testing.assert_array_equal(np.bincount(index, minlength=5), km.host_case(case)['counts'][0])
    i2, u2 = dimension_cluster.assign(size, means)
    np.testing.assert_array_equal(i2, index)
    np.testing.assert_array_equal(u2, iou)


def test_assign_ties_and_nan_go_to_the_lower_index():
    size = km.sizes(50)
    index, iou = km.assign_host(size, np.array([[0.2, 0.3], [0.2, 0.3]]))
    assert not index.any() and (iou > 0).all()
    index, iou = km.assign_host(size, np.array([[0.9, 0.9], [0.2, 0.3], [0.2, 0.3]]))
    assert set(index.tolist()) <= {0, 1} and (index == 1).any()
    index, iou = km.assign_host(np.array([[np.nan, 0.5], [0.2, 0.3]]), np.array([[0.9, 0.9], [0.2, 0.3]]))
    assert index.tolist() == [0, 1] and np.isnan(iou[0]) and iou[1] == 1.0


# ---- 5. dimension_cluster.cluster

def select(size, init, rule):
    """The selection of dimension_cluster.cluster restated: the trials on the host, nltk's sort and consensus as loops over vectors."""
    res = km.host(size, init)
    good = [r for r in range(len(init)) if res['status'][r] == 0]
    sets = []
    for r in good:
        rows = sorted(range(init.shape[1]), key=lambda k: sum(res['means'][r][k])) if len(init) > 1 else list(range(init.shape[1]))
        sets.append((res['means'][r][rows], res['counts'][r][rows]))
    if rule == 'cost':
        pick = min(range(len(good)), key=lambda i: res['cost'][good[i]])
    else:
        totals = [sum(dimension_cluster.distance(a, b) for j, (other, _) in enumerate(sets) if j != i for a, b in zip(mine, other))
                  for i, (mine, _) in enumerate(sets)]
        pick = min(range(len(good)), key=lambda i: totals[i])
    return res, good[pick], sets[pick]


def draw(N, K, R, seed):
    rng = random.Random(seed)
    return np.array([rng.sample(range(N), K) for _ in range(R)], np.int32)


@pytest.mark.parametrize('rule', ['consensus', 'cost'])
def test_cluster_selection(rule):
    size = km.sizes(300).copy()
    size[:90] = size[0]          # duplicates: a trial that draws two of them loses a cluster (status 1) and must be left out
    res, trial, (means, counts) = select(size, draw(300, 3, 24, 5), rule)
    assert 0 < (res['status'] == 1).sum() < 24
    got = dimension_cluster.cluster(size, 3, repeats=24, seed=5, select=rule)
    for k in ('iters', 'status', 'cost'):
        np.testing.assert_array_equal(got[k], res[k], err_msg=k)
    np.testing.assert_array_equal(got['trial_means'], res['means'])          # the draw order for a seed
    assert got['trial'] == trial and got['status'][trial] == 0 and not got['interrupted']
    np.testing.assert_array_equal(got['means'], means)
    np.testing.assert_array_equal(got['counts'], counts)
    assert got['iou'] == 1 - res['cost'][trial] / 300
    assert (np.diff(got['means'].sum(1)) >= 0).all()          # the sort
    if rule == 'cost':
        assert got['cost'][trial] == res['cost'][res['status'] == 0].min()


def test_cluster_single_trial_is_not_sorted():
    size = km.sizes(300)
    got = dimension_cluster.cluster(torch_cpu(size), 4, repeats=1, seed=11)
    want = km.host(size, draw(300, 4, 1, 11))
    np.testing.assert_array_equal(got['means'], want['means'][0])
    np.testing.assert_array_equal(got['counts'], want['counts'][0])
    assert (np.diff(want['means'][0].sum(1)) < 0).any()          # (this seed's result is not in sorted order)


def torch_cpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))


def test_cluster_chunks_equal_one_piece():
    size = km.sizes(64)
    got = dimension_cluster.cluster(size, 2, repeats=5000, seed=1)
    want = km.host(size, draw(64, 2, 5000, 1))
    assert dimension_cluster.CHUNK == 4096 and len(got['status']) == 5000
    np.testing.assert_array_equal(got['trial_means'], want['means'])
    for k in ('iters', 'status', 'cost'):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_cluster_interrupt_reports_the_chunks_that_finished(monkeypatch):
    size, calls, real = km.sizes(64), [], dimension_cluster.run_trials

    def run_trials(*args):
        if calls:
            raise KeyboardInterrupt
        calls.append(1)
        return real(*args)
    monkeypatch.setattr(dimension_cluster, 'CHUNK', 4)
    monkeypatch.setattr(dimension_cluster, 'run_trials', run_trials)
    got = dimension_cluster.cluster(size, 2, repeats=12, seed=1)
    assert got['interrupted'] and len(got['status']) == 4
    np.testing.assert_array_equal(got['trial_means'], km.host(size, draw(64, 2, 4, 1))['means'])


def test_cluster_rejects_bad_input():
    size = km.sizes(20).copy()
    for bad in (np.nan, 0.0, -0.1, np.inf):
        s = size.copy()
        s[3, 1] = bad
        with pytest.raises(ValueError):
            dimension_cluster.cluster(s, 2, repeats=1, seed=0)
    for num in (0, 17, 21):
        with pytest.raises(ValueError):
            dimension_cluster.cluster(size, num, repeats=1, seed=0)
    with pytest.raises(ValueError):
        dimension_cluster.run_trials(torch_cpu(size), np.array([[0, 20]]))
    with pytest.raises(ValueError):
        dimension_cluster.cluster(size, 2, repeats=1, seed=0, select='best')


# ---- 6. get_data and main on a cache pickle whose entries point at the JPEG fixtures (tests/golden/jpeg: the sizes are in the names)

def cache(tmp_path):
    rng = np.random.RandomState(3)
    samples, want = [], []
    for name, (h, w) in ((n, jp.SUPPORTED[n][:2]) for n in jp.NAMES):
        lo = (rng.uniform(0, 0.4, (3, 2)) * [h, w]).astype(np.float32)
        hi = lo + (rng.uniform(0.1, 0.6, (3, 2)) * [h, w]).astype(np.float32)
        samples.append(dict(path=jp.path(name), yx_min=lo, yx_max=hi, cls=np.zeros(3, np.int64)))
        want.append((hi - lo).astype(np.float64) / [h, w])
    os.makedirs(str(tmp_path / 'cache'))
    with open(str(tmp_path / 'cache' / 'train.pkl'), 'wb') as f:
        pickle.dump(samples, f)
    return str(tmp_path / 'cache' / 'train.pkl'), np.concatenate(want)


def test_image_size():
    assert utils.image_size(jp.path('c420_17x13')) == (13, 17)          # (width, height) from the headers alone
    try:
        import PIL  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match='Pillow'):
            utils.image_size(jp.path('prog_48x40'))
    else:
        assert utils.image_size(jp.path('prog_48x40')) == (40, 48)          # a file the library does not parse: Pillow


def test_get_data_and_main(tmp_path, capsys):
    path, want = cache(tmp_path)
    data = dimension_cluster.get_data([path])
    assert data.dtype == np.float64
    np.testing.assert_array_equal(data, want)
    ini, out = str(tmp_path / 'config.ini'), str(tmp_path / 'anchors.tsv')
    with open(ini, 'w') as f:
        f.write('[config]\nroot = %s\n[cache]\nname = cache\n[model]\nanchors = %s\n' % (tmp_path, out))
    res = dimension_cluster.main(['2', '-c', ini, '-p', 'train', '-r', '8', '--seed', '3', '--device', 'cpu', '--logging', str(tmp_path / 'none.yml'),
                                  '--cells', '13', '19', '--output', out])
    want = dimension_cluster.cluster(data, 2, repeats=8, seed=3)
    np.testing.assert_array_equal(res['means'], want['means'])
    lines = capsys.readouterr().out.strip().split('\n')
    assert len(lines) == 2 and all(line.count('\t') == 1 for line in lines)
    np.testing.assert_array_equal(np.array([[float(v) for v in line.split('\t')] for line in lines]), res['means'])
    config = configparser.ConfigParser()
    utils.load_config(config, [ini])
    np.testing.assert_array_equal(utils.get_anchors(config, np.float64), res['means'] * [13, 19])
    assert open(out).readline() == 'width\theight\n'
