"""The batched evaluation on the library's HOST code (y2_eval_match_host behind eval.match_batch on CPU tensors) and the host mAP arithmetic,
against tests/golden/eval.npz: flags, counts, score lists and AP produced by the reference's own eval.py functions (tools/make_golden_eval.py)."""
import configparser
import importlib

import numpy as np
import pytest
import torch

import _hip

ev = importlib.import_module('eval')


def batch(g, k, device='cpu'):
    t = lambda name: torch.from_numpy(g['b%d_%s' % (k, name)]).to(device)
    data = dict(yx_min=t('gt_min'), yx_max=t('gt_max'), cls=t('gt_cls'), difficult=t('gt_difficult'))
    dets = dict(yx_min=t('det_min'), yx_max=t('det_max'), cls=t('det_cls'), score=t('det_score'), count=t('det_count'))
    return data, dets


def test_match_batch_equals_reference_fixture(golden):
    g = golden('eval')
    C, thr = int(g['num_cls']), float(g['threshold'])
    total = np.zeros(C, np.int64)
    for k in range(2):
        data, dets = batch(g, k)
        tp, cls_num = ev.match_batch(data['yx_min'], data['yx_max'], data['cls'], data['difficult'], dets, thr, C)
        assert tp.dtype == torch.bool and tuple(tp.shape) == g['b%d_tp' % k].shape
        np.testing.assert_array_equal(tp.numpy(), g['b%d_tp' % k])
        total += cls_num.numpy()
    np.testing.assert_array_equal(total, g['cls_num'])
    # the cases the fixture exists for are really in it
    assert g['b0_tp'].sum() >= 3 and g['b1_tp'].sum() >= 3
    assert not g['b0_tp'][1].any() and not g['b0_tp'][2].any()          # no valid ground truth; count = 0


def test_accumulator_equals_reference_ap(golden):
    g = golden('eval')
    C, thr = int(g['num_cls']), float(g['threshold'])
    acc = ev.Accumulator(num_cls=C, iou=thr)
    for k in range(2):
        acc.update(*batch(g, k))
    cls_num, cls_score, cls_tp = acc.collect()
    np.testing.assert_array_equal(cls_num, g['cls_num'])
    for c in range(C):
        order, want = np.argsort(-cls_score[c], kind='stable'), np.argsort(-g['score_%d' % c], kind='stable')      # (distinct scores: the order is unique)
        np.testing.assert_array_equal(cls_score[c][order], g['score_%d' % c][want])
        np.testing.assert_array_equal(cls_tp[c][order], g['tp_%d' % c][want])
    for metric07, name in ((True, 'ap07'), (False, 'ap')):
        got = acc.result(metric07=metric07)
        assert sorted(got) == list(g['ap_keys'])
        for c, want in zip(g['ap_keys'], g[name]):
            assert abs(got[int(c)] - want) <= 1e-12, (name, c, got[int(c)], want)
        assert abs(acc.mean_ap(metric07=metric07) - np.mean(g[name])) <= 1e-12
    # config form, and compaction of the retained tensors at a tiny byte bound gives the same result
    cfg = configparser.ConfigParser()
    cfg.read_dict({'eval': {'iou': str(thr), 'metric07': '1'}})
    acc2 = ev.Accumulator(cfg, num_cls=C, max_bytes=1)
    for k in range(2):
        acc2.update(*batch(g, k))
    assert not acc2._padded and acc2.result() == acc.result(metric07=True)


def test_accumulator_keeps_its_own_counts(golden):
    """A detector that reuses its result buffers (a captured graph) overwrites `count` with the next batch's: what was accumulated stays."""
    g = golden('eval')
    C, thr = int(g['num_cls']), float(g['threshold'])
    acc, ref = ev.Accumulator(num_cls=C, iou=thr), ev.Accumulator(num_cls=C, iou=thr)
    count = torch.zeros(3, dtype=torch.int32)
    for k in range(2):
        data, dets = batch(g, k)
        ref.update(data, dets)
        count.copy_(dets['count'])
        acc.update(data, dict(dets, count=count))
    count.fill_(1)
    assert acc.result() == ref.result() and len(acc.result()) >= 1


def test_accumulator_normalises_like_the_reference(golden):
    """image_size / grid: label boxes / (H, W), predicted boxes / (rows, cols) in fp32 (norm_bbox_data, norm_bbox_pred)."""
    g = golden('eval')
    C, thr = int(g['num_cls']), float(g['threshold'])
    data, dets = batch(g, 1)
    hw, grid = torch.tensor([96.0, 64.0]).view(1, 1, 2), torch.tensor([3.0, 2.0]).view(1, 1, 2)
    want, _ = ev.match_batch(data['yx_min'] / hw, data['yx_max'] / hw, data['cls'], data['difficult'],
                             dict(dets, yx_min=dets['yx_min'] / grid, yx_max=dets['yx_max'] / grid), thr, C)
    got = ev.Accumulator(num_cls=C, iou=thr).update(data, dets, image_size=(96, 64), grid=(3, 2))
    assert torch.equal(got, want)


def test_filter_valid_is_the_boolean_mask():
    yx_min = torch.tensor([[1., 1.], [2., 2.], [0., 0.], [3., 5.], [1., 1.], [4., 4.]])
    yx_max = torch.tensor([[2., 3.], [4., 5.], [0., 0.], [5., 5.], [3., 3.], [6., 7.]])
    cls = torch.tensor([1, 1, 0, 2, 3, 0])
    difficult = torch.tensor([0, 0, 0, 0, 1, 0], dtype=torch.uint8)
    mn, mx, c = ev.filter_valid(yx_min, yx_max, cls, difficult)
    keep = [0, 1, 5]            # padding, the box degenerate in x and the difficult box are dropped
    assert torch.equal(mn, yx_min[keep]) and torch.equal(mx, yx_max[keep]) and c.tolist() == [1, 1, 0]
    mn, mx, c = ev.filter_valid(yx_min[2:4], yx_max[2:4], cls[2:4], difficult[2:4])
    assert tuple(mn.shape) == (0, 2) and tuple(mx.shape) == (0, 2) and c.numel() == 0


def test_average_precision_known_answers():
    cfg = {m: configparser.ConfigParser() for m in (0, 1)}
    for m in cfg:
        cfg[m].read_dict({'eval': {'metric07': str(m)}})
    tp = np.array([True, False, True])
    assert abs(ev.average_precision(cfg[1], tp, 3) - 6.0 / 11.0) <= 1e-12
    assert abs(ev.average_precision(cfg[0], tp, 3) - 5.0 / 9.0) <= 1e-12
    empty = np.zeros(0, bool)
    assert ev.average_precision(cfg[1], empty, 2) == 0 and ev.average_precision(cfg[0], empty, 2) == 0
    # merge_ap: descending score, classes without ground truth left out
    ap = ev.merge_ap(cfg[0], [3, 0], [np.array([0.2, 0.9, 0.5], np.float32), np.array([0.3], np.float32)], [np.array([True, True, False]), np.array([False])])
    assert list(ap) == [0] and abs(ap[0] - 5.0 / 9.0) <= 1e-12


def _host_args(B, M, G, seed=0):
    rng = np.random.RandomState(seed)
    f = lambda *s: torch.from_numpy(rng.uniform(0, 4, s).astype(np.float32))
    d_min, g_min = f(B, M, 2), f(B, G, 2)
    return dict(d_min=d_min, d_max=d_min + 1, d_cls=torch.zeros(B, M, dtype=torch.int64), count=torch.full((B,), M, dtype=torch.int32),
                g_min=g_min, g_max=g_min + 1, g_cls=torch.zeros(B, G, dtype=torch.int64), g_dif=torch.zeros(B, G, dtype=torch.uint8),
                tp=torch.full((B, M), 7, dtype=torch.uint8), cls_num=torch.zeros(3, dtype=torch.int32))


def _call_host(a, B, M, G, C=3, null=None):
    p = lambda k: None if (k == null or a[k].numel() == 0) else a[k].data_ptr()
    return _hip.lib().y2_eval_match_host(p('d_min'), p('d_max'), p('d_cls'), p('count'), p('g_min'), p('g_max'), p('g_cls'), p('g_dif'),
                                         B, M, G, C, 0.5, 1.1920929e-07, p('tp'), p('cls_num'))


def test_eval_match_host_argument_handling():
    EINVAL, ENOSUP = -1, -3
    a = _host_args(2, 5, 3)
    for k in ('d_min', 'd_max', 'd_cls', 'count', 'g_min', 'g_max', 'g_cls', 'g_dif', 'tp', 'cls_num'):
        assert _call_host(a, 2, 5, 3, null=k) == EINVAL, k
    assert _call_host(a, 0, 5, 3) == EINVAL and _call_host(a, -1, 5, 3) == EINVAL
    assert (a['tp'] == 7).all() and (a['cls_num'] == 0).all()            # a refused call writes nothing
    big = _host_args(1, 2, _hip.EVAL_MATCH_MAX_G + 1)
    assert _call_host(big, 1, 2, _hip.EVAL_MATCH_MAX_G + 1) == ENOSUP
    assert (big['tp'] == 7).all() and (big['cls_num'] == 0).all()
    # G == 0: every row is written as 0; M == 0: nothing to write, the counts are still taken
    a = _host_args(2, 5, 0)
    assert _call_host(a, 2, 5, 0) == 0 and (a['tp'] == 0).all() and (a['cls_num'] == 0).all()
    a = _host_args(2, 0, 3)
    assert _call_host(a, 2, 0, 3) == 0 and a['cls_num'].tolist() == [6, 0, 0]
    # a class id outside [0, C) is not counted (and nothing is written out of bounds: cls_num has exactly C slots)
    a = _host_args(1, 4, 3)
    a['g_cls'][0] = torch.tensor([0, 3, -1])
    a['d_cls'][0] = torch.tensor([0, 3, -1, 0])
    assert _call_host(a, 1, 4, 3) == 0 and a['cls_num'].tolist() == [1, 0, 0]


def test_match_batch_refuses_too_many_labels():
    G = _hip.EVAL_MATCH_MAX_G + 1
    z = torch.zeros(1, G, 2)
    dets = dict(yx_min=torch.zeros(1, 2, 2), yx_max=torch.ones(1, 2, 2), cls=torch.zeros(1, 2, dtype=torch.int64), count=torch.tensor([2], dtype=torch.int32))
    with pytest.raises(RuntimeError, match='Y2_ENOSUP'):
        ev.match_batch(z, z, torch.zeros(1, G, dtype=torch.int64), torch.zeros(1, G), dets, 0.5, 3)
