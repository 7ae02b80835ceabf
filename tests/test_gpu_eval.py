"""GPU tests of the batched evaluation (run with -m gpu on an MI355X): y2_eval_match against its host twin bit for bit, detect.expand_batch
against postprocess_batch, and eval.Accumulator end to end against the per-image, per-class path (postprocess_batch + eval.matching)."""
import configparser
import importlib

import numpy as np
import pytest
import torch

import _hip
import utils.iou.torch as iou
from oracle import darknet as odark
from oracle import synth
from oracle.make_golden import NARROW

pytestmark = pytest.mark.gpu

ev = importlib.import_module('eval')
THR = 0.5


def dev():
    return torch.device('cuda:0')


def batch(g, k, device='cpu'):
    """Batch k of tests/golden/eval.npz as (labels, detections) on `device`."""
    t = lambda name: torch.from_numpy(g['b%d_%s' % (k, name)]).to(device)
    data = dict(yx_min=t('gt_min'), yx_max=t('gt_max'), cls=t('gt_cls'), difficult=t('gt_difficult'))
    dets = dict(yx_min=t('det_min'), yx_max=t('det_max'), cls=t('det_cls'), score=t('det_score'), count=t('det_count'))
    return data, dets


def both(data, dets, C, thr=THR):
    """match_batch on the device and on the host for the same CPU inputs -> ((tp, cls_num) device, (tp, cls_num) host) as numpy."""
    d = dev()
    got = ev.match_batch(*(data[k].to(d) for k in ('yx_min', 'yx_max', 'cls', 'difficult')), {k: v.to(d) for k, v in dets.items()}, thr, C)
    want = ev.match_batch(data['yx_min'], data['yx_max'], data['cls'], data['difficult'], dets, thr, C)
    return tuple(t.cpu().numpy() for t in got), tuple(t.numpy() for t in want)


def positives(data, dets, thr=THR):
    """Participating rows whose best IoU over the valid same-class boxes exceeds thr, restated with the IoU matrix (no claim logic)."""
    n = 0
    for b in range(data['cls'].size(0)):
        k = int(dets['count'][b])
        if k == 0:
            continue
        m = iou.iou_matrix(dets['yx_min'][b, :k], dets['yx_max'][b, :k], data['yx_min'][b], data['yx_max'][b])
        valid = (data['yx_min'][b] < data['yx_max'][b]).all(-1) & (data['difficult'][b] < 1)
        ok = valid.view(1, -1) & (dets['cls'][b, :k].view(-1, 1) == data['cls'][b].view(1, -1))
        n += int(((m * ok).max(-1)[0] > thr).sum()) if ok.numel() else 0
    return n


def random_case(B, M, G, C, counts, seed):
    """Boxes the way test_eval_matching_like_reference builds them: per image G ground-truth boxes, detections = jittered copies of the first
    ones (twice: true positives and duplicates) plus strays; with G >= 3 one box is difficult, one degenerate, and the last box carries the class
    id C (outside [0, C): not counted, still matched by its copies); with M >= 3 the last row carries the class id -1."""
    rng = np.random.RandomState(seed)
    c, s = rng.uniform(2, 11, (B, G, 2)).astype(np.float32), rng.uniform(1, 4, (B, G, 2)).astype(np.float32)
    g_min, g_max = c - s / 2, c + s / 2
    g_cls = rng.randint(0, C, (B, G)).astype(np.int64)
    g_dif = np.zeros((B, G), np.uint8)
    if G >= 3:
        g_dif[:, 1] = 1
        g_max[:, 2, 0] = g_min[:, 2, 0]
        g_cls[:, G - 1] = C
    n = min(G, max(1, M // 3))
    pc = rng.uniform(2, 11, (B, M, 2)).astype(np.float32)
    ps = rng.uniform(1, 4, (B, M, 2)).astype(np.float32)
    p_cls = rng.randint(0, C, (B, M)).astype(np.int64)
    for r in range(min(2, M // n)):
        rows = slice(r * n, (r + 1) * n)
        pc[:, rows] = c[:, :n] + rng.uniform(-0.1, 0.1, (B, n, 2)).astype(np.float32) * (r + 1)
        ps[:, rows], p_cls[:, rows] = s[:, :n], g_cls[:, :n]
    if M >= 3:
        p_cls[:, M - 1] = -1
    t = torch.from_numpy
    data = dict(yx_min=t(g_min), yx_max=t(g_max), cls=t(g_cls), difficult=t(g_dif))
    dets = dict(yx_min=t(pc - ps / 2), yx_max=t(pc + ps / 2), cls=t(p_cls), count=torch.tensor(counts, dtype=torch.int32))
    return data, dets


def test_device_equals_host_on_the_fixture(golden):
    g = golden('eval')
    C = int(g['num_cls'])
    for k in range(2):
        data, dets = batch(g, k)
        got, want = both(data, dets, C, float(g['threshold']))
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[0], g['b%d_tp' % k])


# (1,1,1,1); rows wrapping round the 256 threads several times; G over two wavefronts; count = 0 / partial / M
CASES = [(1, 1, 1, 1, [1]), (5, 700, 7, 20, [700, 650, 300, 700, 1]), (2, 40, 130, 80, [40, 33]), (3, 24, 6, 5, [0, 13, 24])]


@pytest.mark.parametrize('B,M,G,C,counts', CASES)
def test_device_equals_host_on_random_cases(B, M, G, C, counts):
    data, dets = random_case(B, M, G, C, counts, seed=B + M + G + C)
    got, want = both(data, dets, C)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    tp = int(got[0].sum())
    assert tp >= 1
    for b in range(B):
        assert not got[0][b, counts[b]:].any()
    if M >= 2:          # (a single detection row cannot hold a duplicate: at M = 1 only the true positive is asserted)
        assert positives(data, dets) - tp >= 1, 'no suppressed duplicate in this case'
    assert got[1].sum() >= 1
    if G >= 3:          # the valid boxes of class C are not counted: the counts hold exactly the valid boxes with a class in [0, C)
        valid = ((data['yx_min'] < data['yx_max']).all(-1) & (data['difficult'] < 1) & (data['cls'] < C)).numpy()
        assert got[1].sum() == valid.sum() and (data['cls'] == C).any() and (dets['cls'] == -1).any()


def test_reproducible_bytes():
    B, M, G, C, counts = CASES[1]
    data, dets = random_case(B, M, G, C, counts, seed=11)
    d = dev()
    args = [data[k].to(d) for k in ('yx_min', 'yx_max', 'cls', 'difficult')] + [{k: v.to(d) for k, v in dets.items()}, THR, C]
    a, b = ev.match_batch(*args), ev.match_batch(*args)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and int(a[0].sum()) >= 1


def test_label_cap():
    d = dev()
    G = _hip.EVAL_MATCH_MAX_G + 1
    z = lambda *s, **kw: torch.zeros(*s, device=d, **kw)
    tp, cls_num = torch.full((1, 4), 7, dtype=torch.uint8, device=d), z(3, dtype=torch.int32)
    g_min, g_max = z(1, G, 2), z(1, G, 2) + 1
    d_min, d_max = z(1, 4, 2), z(1, 4, 2) + 1
    d_cls, g_cls, g_dif = z(1, 4, dtype=torch.int64), z(1, G, dtype=torch.int64), z(1, G, dtype=torch.uint8)
    count = torch.tensor([4], dtype=torch.int32, device=d)
    call = lambda g: _hip.lib().y2_eval_match(_hip.ptr(d_min), _hip.ptr(d_max), _hip.ptr(d_cls), _hip.ptr(count), _hip.ptr(g_min), _hip.ptr(g_max),
                                              _hip.ptr(g_cls), _hip.ptr(g_dif), 1, 4, g, 3, THR, iou.EPS, _hip.ptr(tp), _hip.ptr(cls_num), _hip.stream())
    assert call(G) == -3                                  # Y2_ENOSUP
    torch.cuda.synchronize()
    assert (tp == 7).all() and (cls_num == 0).all()
    assert call(G - 1) == 0                               # the cap itself is served: every label matches every row, the first row claims box 0
    torch.cuda.synchronize()
    assert tp.tolist() == [[1, 0, 0, 0]] and cls_num.tolist() == [G - 1, 0, 0]


# ------------------------------------------------------------------ on a network's detections
def detections(fix, B=4):
    import detect
    import model
    import model.yolo2
    cfg = configparser.ConfigParser()
    cfg.read_dict({'batch_norm': {'enable': '1'}})
    anchors = torch.from_numpy(synth.ANCHORS_VOC)
    sd = odark.init_state_dict(5, 20, seed=0, channels=NARROW, head_scale=1 / 8.0)
    dnn = model.yolo2.Darknet(model.ConfigChannels(cfg, sd), anchors, 20)
    dnn.load_state_dict(sd, strict=False)
    inf = model.Inference(cfg, dnn, anchors).to(dev()).eval()
    with torch.no_grad():
        pred = model._inference(inf, synth.images(B, 96, seed=1).to(dev()))
    feat = pred['feature'].permute(0, 2, 3, 1).contiguous()
    d = detect.detect_batch(feat, anchors, fix=fix, threshold=0.05, threshold_cls=0.005, overlap=0.45)
    return detect, d


@pytest.mark.parametrize('fix', [False, True])
def test_expand_batch_equals_postprocess_batch(fix):
    detect, d = detections(fix)
    res = detect.postprocess_batch(d, fix=fix, threshold_cls=0.005)
    e = detect.expand_batch(d, fix=fix, threshold_cls=0.005)
    B = len(res)
    M = e['cls'].size(1)
    assert tuple(e['yx_min'].shape) == (B, M, 2) and tuple(e['yx_max'].shape) == (B, M, 2) and tuple(e['score'].shape) == (B, M) and tuple(e['count'].shape) == (B,)
    assert e['cls'].dtype == torch.int64 and e['count'].dtype == torch.int32
    total = 0
    for b in range(B):
        m = int(e['count'][b])
        if res[b] is None:
            assert m == 0
            continue
        _, yx_min, yx_max, cls, score = res[b]
        assert m == score.numel()
        assert torch.equal(e['yx_min'][b, :m], yx_min) and torch.equal(e['yx_max'][b, :m], yx_max)
        assert torch.equal(e['cls'][b, :m], cls) and torch.equal(e['score'][b, :m], score)
        total += m
    assert total >= 20, total


def test_accumulator_end_to_end_equals_per_class_path():
    """The device accumulation against a second one built only from what existed before it (postprocess_batch, then eval.matching per image and
    class) with the host merge_ap on top: the same flag per detection, the same AP per class, exactly."""
    detect, d = detections(True)
    C, S, cells = 20, 96.0, 3.0
    res = detect.postprocess_batch(d, fix=True, threshold_cls=0.005)
    e = detect.expand_batch(d, fix=True, threshold_cls=0.005)
    B, G = len(res), 6
    rng = np.random.RandomState(0)
    g_min, g_max = np.zeros((B, G, 2), np.float32), np.zeros((B, G, 2), np.float32)
    g_cls, g_dif = np.zeros((B, G), np.int64), np.zeros((B, G), np.uint8)
    for b in range(B):                  # labels in pixels: jittered copies of detected boxes, one of them difficult, and a degenerate box
        if res[b] is None:
            continue
        _, yx_min, yx_max, cls, _ = (t.cpu().numpy() for t in res[b])
        rows = np.linspace(0, len(cls) - 1, 5).astype(int)
        for j, r in enumerate(rows):
            g_min[b, j] = (yx_min[r] + rng.uniform(-0.03, 0.03, 2)) * (S / cells)
            g_max[b, j] = (yx_max[r] + rng.uniform(-0.03, 0.03, 2)) * (S / cells)
            g_cls[b, j] = cls[r]
        g_dif[b, 4] = 1
        g_min[b, 5], g_max[b, 5], g_cls[b, 5] = (40, 50), (60, 50), cls[0]
    t = lambda a: torch.from_numpy(a).to(dev())
    data = dict(yx_min=t(g_min), yx_max=t(g_max), cls=t(g_cls), difficult=t(g_dif))
    acc = ev.Accumulator(num_cls=C, iou=THR)
    tp = acc.update(data, e, image_size=(S, S), grid=(cells, cells)).cpu().numpy()
    # the per-image, per-class path
    hw = torch.tensor([S, S], device=dev()).view(1, 2)
    grid = torch.tensor([cells, cells], device=dev()).view(1, 2)
    cls_num = [0] * C
    cls_score = [np.zeros(0, np.float32) for _ in range(C)]
    cls_tp = [np.zeros(0, bool) for _ in range(C)]
    n_tp = n_fp = 0
    for b in range(B):
        d_min, d_max = data['yx_min'][b] / hw, data['yx_max'][b] / hw
        valid = (d_min < d_max).all(-1) & (data['difficult'][b] < 1)
        d_min, d_max, d_cls = d_min[valid], d_max[valid], data['cls'][b][valid]
        for c in d_cls.tolist():
            cls_num[c] += 1
        if res[b] is None:
            assert not tp[b].any()
            continue
        _, yx_min, yx_max, cls, score = res[b]
        yx_min, yx_max = yx_min / grid, yx_max / grid
        flags = np.zeros(len(cls), bool)
        for c in sorted(set(cls.tolist())):
            sel = cls == c
            f = ev.matching(d_min[d_cls == c], d_max[d_cls == c], yx_min[sel], yx_max[sel], THR)
            flags[sel.cpu().numpy()] = f
            cls_score[c] = np.append(cls_score[c], score[sel].cpu().numpy())
            cls_tp[c] = np.append(cls_tp[c], f)
        np.testing.assert_array_equal(tp[b, :len(cls)], flags)
        assert not tp[b, len(cls):].any()
        n_tp += int(flags.sum())
        n_fp += int((~flags).sum())
    assert n_tp >= 3 and n_fp >= 1, (n_tp, n_fp)
    for metric07 in (True, False):
        cfg = configparser.ConfigParser()
        cfg.read_dict({'eval': {'metric07': '1' if metric07 else '0'}})
        want = ev.merge_ap(cfg, cls_num, cls_score, cls_tp)
        got = acc.result(metric07=metric07)
        assert got == want and len(got) >= 1
    assert acc.mean_ap() == float(np.mean(list(acc.result().values())))


def test_accumulator_over_graphed_detector_batches():
    """Two batches through ONE GraphedDetector (its static result dict is overwritten by every replay) with fix = 0, where the detection count is
    the detector's own keep_count buffer: what the accumulator holds at the end equals what postprocess_batch gave per batch at the time."""
    import detect
    import model
    import model.yolo2
    cfg = configparser.ConfigParser()
    cfg.read_dict({'batch_norm': {'enable': '1'}})
    anchors = torch.from_numpy(synth.ANCHORS_VOC)
    sd = odark.init_state_dict(5, 20, seed=0, channels=NARROW, head_scale=1 / 8.0)
    dnn = model.yolo2.Darknet(model.ConfigChannels(cfg, sd), anchors, 20)
    dnn.load_state_dict(sd, strict=False)
    dnn = dnn.to(dev()).eval()
    B, C = 4, 20
    xs = [synth.images(B, 96, seed=1).to(dev()), (synth.images(B, 96, seed=7) * 2).to(dev())]
    gd = detect.GraphedDetector(dnn, anchors, xs[0], fix=False, threshold=0.05, overlap=0.45)
    acc = ev.Accumulator(num_cls=C, iou=THR)
    want_score, want_tp, want_num = [[] for _ in range(C)], [[] for _ in range(C)], np.zeros(C, np.int64)
    counts = []
    for x in xs:
        d = gd.run(x)
        res = detect.postprocess_batch(d, fix=False, to_host=True)
        # labels in cells: the first surviving box of every image with its class, and one box far outside
        g_min, g_max, g_cls = torch.zeros(B, 2, 2), torch.zeros(B, 2, 2), torch.zeros(B, 2, dtype=torch.int64)
        for b in range(B):
            if res[b] is not None:
                g_min[b, 0], g_max[b, 0], g_cls[b, 0] = res[b][1][0], res[b][2][0], res[b][3][0]
            g_min[b, 1], g_max[b, 1], g_cls[b, 1] = torch.tensor([50., 50.]), torch.tensor([52., 53.]), 3
        data = dict(yx_min=g_min.to(dev()), yx_max=g_max.to(dev()), cls=g_cls.to(dev()), difficult=torch.zeros(B, 2, dtype=torch.uint8, device=dev()))
        tp = acc.update(data, detect.expand_batch(d, fix=False)).cpu().numpy()
        valid = (g_min < g_max).all(-1)
        for c in g_cls[valid].tolist():
            want_num[c] += 1
        counts.append([0 if r is None else int(r[4].numel()) for r in res])
        for b in range(B):
            if res[b] is None:
                continue
            cls, score = res[b][3].numpy(), res[b][4].numpy()
            for c in range(C):
                want_score[c].append(score[cls == c])
                want_tp[c].append(tp[b, :len(cls)][cls == c])
    assert counts[0] != counts[1], 'the two batches must differ in their detection counts for this test to say anything'
    assert sum(counts[0]) + sum(counts[1]) >= 20
    cls_num, cls_score, cls_tp = acc.collect()
    np.testing.assert_array_equal(cls_num, want_num)
    n_tp = 0
    for c in range(C):
        np.testing.assert_array_equal(cls_score[c], np.concatenate(want_score[c]) if want_score[c] else np.zeros(0, np.float32))
        np.testing.assert_array_equal(cls_tp[c], np.concatenate(want_tp[c]) if want_tp[c] else np.zeros(0, bool))
        n_tp += int(cls_tp[c].sum())
    assert n_tp >= 2          # at least one exact label per batch was claimed


def test_match_batch_is_capturable(golden):
    """No synchronisation inside match_batch: it is captured in a graph on a side stream at the (3, 24, 6, 5) shape; the replay equals the eager result."""
    g = golden('eval')
    C, thr = int(g['num_cls']), float(g['threshold'])
    data, dets = batch(g, 0, dev())
    args = [data[k] for k in ('yx_min', 'yx_max', 'cls', 'difficult')] + [dets, thr, C]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = ev.match_batch(*args)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = (eager[0].clone(), eager[1].clone())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = ev.match_batch(*args)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
    np.testing.assert_array_equal(out[0].cpu().numpy(), g['b0_tp'])
