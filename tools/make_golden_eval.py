"""Generate tests/golden/eval.npz from the REFERENCE eval.py (only where the reference checkout exists).

    python tools/make_golden_eval.py

The reference's eval.py cannot be imported (cv2, tinydb, xlsxwriter, pandas ...): the file is parsed with `ast` and only the function
definitions _matching, matching, voc_ap, average_precision, filter_cls_data, filter_cls_pred and Eval.merge_ap are compiled, unmodified, into a
namespace that holds np, torch and the `utils` shim of oracle.refload (np.bool / np.float are aliased where numpy has dropped them).  The loop of
eval.py:278-292 is restated around them, fed with detection arrays in place of `postprocess`.

NOT taken from the reference as written: filter_valid (eval.py:140-145).  Its mask `torch.prod(yx_min < yx_max, -1) & (difficult < 1)` was a byte
mask on the torch it was written for; on current torch it is an int64 tensor, and `cls[mask]` INDEXES instead of masking (three valid boxes of
classes [1, 1, 0] come back as classes [1, 1, 1] with all-zero boxes).  The generator applies the mask the code intends,
`(yx_min < yx_max).all(-1) & (difficult < 1)`, as a boolean mask.

Two batches of three images, C = 5 classes, G = 6 label slots, M = 24 detection rows, IoU threshold 0.5.  The cases: a difficult box, a degenerate
box (min >= max), zero padding, an image without valid ground truth, an image with count = 0, a partial count with live-looking rows behind it, a
detected class absent from the ground truth, duplicate detections of one box, two identical ground-truth boxes, and a detection whose IoU equals
the threshold exactly ((0,0)-(2,2) against (0,0)-(2,1): 0.5, not positive).  Rows are in seeded random order (array order is not score order) and
scores are distinct within each class (asserted), so the order among equal scores cannot influence a result.  Stored, arrays only:
  threshold, num_cls
  b<k>_gt_min / gt_max / gt_cls / gt_difficult, b<k>_det_min / det_max / det_cls / det_score / det_count      the inputs of batch k
  b<k>_tp [3,24]           true-positive flag per image and row (False at and beyond count)
  cls_num [5]              valid ground-truth boxes per class
  score_<c> / tp_<c>       the reference's concatenated per-class score and flag lists
  ap_keys, ap07, ap        the keys of merge_ap's result and the AP per key with [eval] metric07 = 1 / 0
The archive is written with fixed time stamps: a second run reproduces it byte for byte."""
import ast
import configparser
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refload  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'eval.npz')
C, G, M, THRESHOLD = 5, 6, 24, 0.5
WANTED = ('_matching', 'matching', 'voc_ap', 'average_precision', 'filter_cls_data', 'filter_cls_pred', 'merge_ap')


def load_reference_eval():
    """Namespace with the reference's evaluation functions (see the module docstring)."""
    if not hasattr(np, 'bool'):
        np.bool = bool
    if not hasattr(np, 'float'):
        np.float = float
    path = os.path.join(refload.REF, 'eval.py')
    tree = ast.parse(open(path).read(), path)
    keep = []
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in WANTED:
            keep.append(node)
        elif isinstance(node, ast.ClassDef) and node.name == 'Eval':
            keep += [n for n in node.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(n.name for n in keep) == sorted(WANTED)
    ns = dict(np=np, torch=torch, utils=refload.load().utils)
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, 'exec'), ns)
    return types.SimpleNamespace(**{k: ns[k] for k in WANTED})


def intended_filter_valid(yx_min, yx_max, cls, difficult):
    mask = (yx_min < yx_max).all(-1) & (difficult < 1)
    return yx_min[mask], yx_max[mask], cls[mask]


def make_image(rng, gts, dets, count, shuffle=True):
    """gts: (ymin, xmin, ymax, xmax, cls, difficult); dets: (ymin, xmin, ymax, xmax, cls).  Pads both with zeros; detection rows are shuffled."""
    g_min, g_max, g_cls, g_dif = np.zeros((G, 2), np.float32), np.zeros((G, 2), np.float32), np.zeros(G, np.int64), np.zeros(G, np.uint8)
    for i, (y0, x0, y1, x1, c, d) in enumerate(gts):
        g_min[i], g_max[i], g_cls[i], g_dif[i] = (y0, x0), (y1, x1), c, d
    d_min, d_max, d_cls = np.zeros((M, 2), np.float32), np.zeros((M, 2), np.float32), np.zeros(M, np.int64)
    order = rng.permutation(len(dets)) if shuffle else np.arange(len(dets))
    for i, j in enumerate(order):
        y0, x0, y1, x1, c = dets[j]
        d_min[i], d_max[i], d_cls[i] = (y0, x0), (y1, x1), c
    assert len(gts) <= G and count <= len(dets) <= M
    return g_min, g_max, g_cls, g_dif, d_min, d_max, d_cls, count


def jitter(rng, b, amount):
    y0, x0, y1, x1 = b
    j = rng.uniform(-amount, amount, 4)
    return (y0 + j[0], x0 + j[1], y1 + j[2], x1 + j[3])


def strays(rng, n, classes):
    out = []
    for _ in range(n):
        c = rng.uniform(0, 12, 2)
        s = rng.uniform(0.5, 3, 2)
        out.append((c[0] - s[0] / 2, c[1] - s[1] / 2, c[0] + s[0] / 2, c[1] + s[1] / 2, int(rng.choice(classes))))
    return out


def random_image(rng, n_gt, n_det, extra_gt=()):
    gts = []
    for _ in range(n_gt):
        c = rng.uniform(2, 10, 2)
        s = rng.uniform(1.5, 4, 2)
        gts.append((c[0] - s[0] / 2, c[1] - s[1] / 2, c[0] + s[0] / 2, c[1] + s[1] / 2, int(rng.randint(0, C)), 0))
    dets = []
    for g in gts:
        for amount in (0.1, 0.3):
            dets.append(jitter(rng, g[:4], amount) + (g[4],))
    dets += strays(rng, n_det - len(dets), list(range(C)))
    return gts + list(extra_gt), dets


def batches():
    rng = np.random.RandomState(7)
    a = [(1, 1, 4, 5), (1.5, 1.5, 4.5, 5.5), (6, 6, 9, 10), (2, 7, 5, 11), (7, 1, 10, 4)]
    # batch 0, image 0: four valid boxes (classes 1, 1, 0, 3; the two of class 1 overlap), a difficult box of class 2, one padding slot;
    # jittered copies (true positives), three detections of box 0 (duplicates), one on the difficult box, class 4 (absent), strays; count 20 of 22 rows
    gts = [a[0] + (1, 0), a[1] + (1, 0), a[2] + (0, 0), a[3] + (3, 0), a[4] + (2, 1)]
    dets = [jitter(rng, a[0], 0.15) + (1,) for _ in range(3)] + [jitter(rng, a[1], 0.1) + (1,), jitter(rng, a[2], 0.2) + (0,), jitter(rng, a[2], 0.2) + (3,),
                                                                 jitter(rng, a[3], 0.2) + (3,), jitter(rng, a[4], 0.1) + (2,), jitter(rng, a[2], 0.1) + (4,)]
    dets += strays(rng, 22 - len(dets), [0, 1, 2, 3, 4])
    i00 = make_image(rng, gts, dets, 20)
    # image 1: no valid ground truth (degenerate in y, degenerate in x with equality, a difficult box, padding); detections on all of them
    gts = [(5, 1, 3, 4, 0, 0), (1, 6, 4, 6, 1, 0), a[2] + (2, 1)]
    dets = [(3, 1, 5, 4, 0), (1, 5, 4, 7, 1), jitter(rng, a[2], 0.1) + (2,)] + strays(rng, 7, [0, 1, 2])
    i01 = make_image(rng, gts, dets, 10)
    # image 2: valid ground truth, count = 0 (the rows look like good detections and must not take part)
    gts = [a[0] + (4, 0), a[2] + (0, 0)]
    dets = [jitter(rng, a[0], 0.1) + (4,), jitter(rng, a[2], 0.1) + (0,)] + strays(rng, 6, [0, 4])
    i02 = make_image(rng, gts, dets, 0)
    # batch 1, image 0: two identical boxes of class 2 with two detections (both go to the first: the second is a false positive); the exact-threshold
    # pair of class 4: ground truth (0,0)-(2,1), detection (0,0)-(2,2), IoU 2 / 4 = 0.5, not > 0.5; count = M
    twin = (5, 5, 9, 9)
    gts = [twin + (2, 0), twin + (2, 0), (0, 0, 2, 1, 4, 0), a[3] + (0, 0)]
    dets = [jitter(rng, twin, 0.1) + (2,), jitter(rng, twin, 0.1) + (2,), (0, 0, 2, 2, 4), jitter(rng, a[3], 0.2) + (0,)]
    dets += strays(rng, M - len(dets), [0, 1, 2, 3])
    i10 = make_image(rng, gts, dets, M)
    g, d = random_image(rng, 5, 20)
    i11 = make_image(rng, g, d, 18)
    g, d = random_image(rng, 4, 24, extra_gt=[(3, 3, 3, 8, 1, 0), (0, 0, 0, 0, 0, 0)])
    i12 = make_image(rng, g, d, 24)
    # distinct scores (globally, hence within each class) in an order unrelated to the rows
    scores = (rng.permutation(2 * 3 * M).astype(np.float32) + 1) / np.float32(2 * 3 * M + 1)
    out = []
    for k, imgs in enumerate(((i00, i01, i02), (i10, i11, i12))):
        cols = [np.stack([im[j] for im in imgs]) for j in range(7)]
        out.append(dict(gt_min=cols[0], gt_max=cols[1], gt_cls=cols[2], gt_difficult=cols[3], det_min=cols[4], det_max=cols[5], det_cls=cols[6],
                        det_score=scores[k * 3 * M:(k + 1) * 3 * M].reshape(3, M), det_count=np.array([im[7] for im in imgs], np.int32)))
    return out


def reference_loop(ref, batch_list):
    """eval.py:257-292 (stat_ap) on detection arrays."""
    cls_num = [0 for _ in range(C)]
    cls_score = [np.array([], dtype=np.float32) for _ in range(C)]
    cls_tp = [np.array([], dtype=np.bool) for _ in range(C)]
    tps = []
    t = torch.from_numpy
    for bt in batch_list:
        tp_rows = np.zeros((3, M), bool)
        for b in range(3):
            data_yx_min, data_yx_max, data_cls = intended_filter_valid(t(bt['gt_min'][b]), t(bt['gt_max'][b]), t(bt['gt_cls'][b]), t(bt['gt_difficult'][b]))
            for c in data_cls.cpu().numpy():
                cls_num[c] += 1
            n = int(bt['det_count'][b])
            if n == 0:                  # postprocess returns None
                continue
            yx_min, yx_max, cls, score = t(bt['det_min'][b][:n]), t(bt['det_max'][b][:n]), t(bt['det_cls'][b][:n]), t(bt['det_score'][b][:n])
            for c in set(cls.cpu().numpy()):
                c = int(c)
                d_min, d_max = ref.filter_cls_data(data_yx_min, data_yx_max, data_cls == c)
                p_min, p_max, _score = ref.filter_cls_pred(yx_min, yx_max, score, cls == c)
                tp = ref.matching(d_min, d_max, p_min, p_max, THRESHOLD)
                cls_score[c] = np.append(cls_score[c], _score.cpu().numpy())
                cls_tp[c] = np.append(cls_tp[c], tp)
                tp_rows[b, :n][(cls == c).numpy()] = tp
        tps.append(tp_rows)
    return cls_num, cls_score, cls_tp, tps


def save_npz(path, arrays):
    """np.savez_compressed with fixed time stamps (numpy stamps the members with the current time)."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ref = load_reference_eval()
    bl = batches()
    cls_num, cls_score, cls_tp, tps = reference_loop(ref, bl)
    for c in range(C):
        assert len(np.unique(cls_score[c])) == len(cls_score[c]), 'scores of class %d are not distinct' % c
    out = dict(threshold=np.float32(THRESHOLD), num_cls=np.int64(C))
    for k, bt in enumerate(bl):
        for name, v in bt.items():
            out['b%d_%s' % (k, name)] = v
        out['b%d_tp' % k] = tps[k]
    out['cls_num'] = np.array(cls_num, np.int64)
    for c in range(C):
        out['score_%d' % c] = cls_score[c].astype(np.float32)
        out['tp_%d' % c] = cls_tp[c].astype(bool)
    aps = {}
    for m07 in (1, 0):
        cfg = configparser.ConfigParser()
        cfg.read_dict({'eval': {'metric07': str(m07)}})
        aps[m07] = ref.merge_ap(types.SimpleNamespace(config=cfg), cls_num, cls_score, cls_tp)
    assert sorted(aps[0]) == sorted(aps[1])
    keys = sorted(aps[1])
    out['ap_keys'] = np.array(keys, np.int64)
    out['ap07'] = np.array([aps[1][c] for c in keys], np.float64)
    out['ap'] = np.array([aps[0][c] for c in keys], np.float64)
    # the cases the fixture exists for
    t0, t1 = tps
    assert t0.sum() >= 4 and t1.sum() >= 4 and not t0[1].any() and not t0[2].any()
    exact = [i for i in range(M) if bl[1]['det_cls'][0][i] == 4 and tuple(bl[1]['det_max'][0][i]) == (2.0, 2.0)]
    assert len(exact) == 1 and not t1[0][exact[0]]
    twins = [i for i in range(M) if bl[1]['det_cls'][0][i] == 2 and t1[0][i]]
    assert len(twins) == 1
    save_npz(OUT, out)
    print('wrote %s (%d bytes); cls_num %s, true positives %d + %d, AP07 %s, AP %s' % (OUT, os.path.getsize(OUT), cls_num, t0.sum(), t1.sum(), out['ap07'], out['ap']))


if __name__ == '__main__':
    main()
