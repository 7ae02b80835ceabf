"""`eval` — the matching and mAP arithmetic of the reference's VOC evaluation (eval.py:57-121, 140-162, 278-301).

`matching` / `_matching` mirror the reference per (image, class) on the IoU kernel (y2_iou_rowmax).  `match_batch` is the batch form of the whole
loop eval.py:278-292 - filter_valid, the per-class ground-truth counts, filter_cls_*, matching - as ONE launch (y2_eval_match; CPU tensors:
y2_eval_match_host), and `Accumulator` carries its flags to `voc_ap` / `average_precision` / `merge_ap` (host numpy float64, like the reference)
without host traffic per image or class.  The TinyDB / xlsx reporting, the data loader and the `Eval` class are out of scope."""
import configparser

import numpy as np
import torch

import _hip
import utils.iou.torch


def _matching(positive, index):
    """eval.py:57-64: walking the predictions in descending-score order, a prediction is a true positive when it overlaps a
    ground-truth box enough (`positive`) and that box (`index`) has not been claimed by an earlier prediction."""
    positive, index = np.asarray(positive, bool), np.asarray(index)
    tp = np.zeros(len(positive), bool)
    claimed = set()
    for i in np.flatnonzero(positive):
        gt = int(index[i])
        if gt not in claimed:
            claimed.add(gt)
            tp[i] = True
    return tp


def matching(data_yx_min, data_yx_max, yx_min, yx_max, threshold):
    """eval.py:67-75: predictions of one class in one image (descending score) against that class's ground truth.  The IoU matrix and
    its row arg-max run on the device in one kernel (y2_iou_rowmax); only two n-vectors cross to the host for the sequential claim loop."""
    if data_yx_min.numel() == 0:
        return np.zeros([yx_min.size(0)], bool)
    if not yx_min.is_cuda:
        best, which = utils.iou.torch.iou_matrix(yx_min, yx_max, data_yx_min, data_yx_max).max(-1)      # CPU tensors: the library's host IoU
    else:
        best, which = utils.iou.torch.iou_rowmax(yx_min, yx_max, data_yx_min, data_yx_max)               # one kernel: IoU row + max + first arg-max
    return _matching((best.cpu().numpy() > np.float32(threshold)), which.cpu().numpy())


def filter_valid(yx_min, yx_max, cls, difficult):
    """eval.py:140-145, one image: the boxes with min < max in both coordinates that are not difficult.  The reference builds its mask as
    `torch.prod(yx_min < yx_max, -1) & (difficult < 1)`: a byte mask on the torch it was written for, an int64 tensor on current torch, where
    `cls[mask]` INDEXES instead of masking (three valid boxes of classes [1, 1, 0] come back as classes [1, 1, 1] with all-zero boxes).  This is
    the mask the code intends, applied as a boolean mask."""
    mask = (yx_min < yx_max).all(-1) & (difficult < 1)
    return yx_min[mask], yx_max[mask], cls[mask]


def match_batch(data_yx_min, data_yx_max, data_cls, difficult, dets, threshold, num_cls):
    """eval.py:278-292 for a batch in one launch.  Labels padded to G boxes per image: data_yx_min / data_yx_max [B,G,2], data_cls [B,G],
    difficult [B,G]; dets: the dict of detect.expand_batch (yx_min / yx_max [B,M,2], cls int64 [B,M], count int32 [B]; `score` is not read here).
    Returns (tp bool [B,M], cls_num int32 [num_cls]): tp[b,i] is the reference's true-positive flag of detection row i (False at and beyond
    count[b]), cls_num the valid ground-truth boxes per class.  Device tensors: y2_eval_match on the current stream, no synchronisation (it can be
    captured in a graph); CPU tensors: y2_eval_match_host."""
    dev = data_yx_min.device
    f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
    g_min, g_max, d_min, d_max = f32(data_yx_min), f32(data_yx_max), f32(dets['yx_min']), f32(dets['yx_max'])
    g_cls = data_cls.to(device=dev, dtype=torch.int64).contiguous()
    g_dif = (difficult.to(dev) >= 1).to(torch.uint8).contiguous()          # `difficult < 1` (eval.py:141) for every dtype the labels come in
    d_cls = dets['cls'].to(device=dev, dtype=torch.int64).contiguous()
    count = dets['count'].to(device=dev, dtype=torch.int32).contiguous()
    B, G = g_cls.shape
    M = d_cls.size(1)
    assert d_cls.size(0) == B and count.numel() == B and g_min.shape == (B, G, 2) and d_min.shape == (B, M, 2)
    tp = torch.empty(B, M, dtype=torch.uint8, device=dev)
    cls_num = torch.empty(num_cls, dtype=torch.int32, device=dev)
    p = lambda t: t.data_ptr() if t.numel() else None
    args = (p(d_min), p(d_max), p(d_cls), p(count), p(g_min), p(g_max), p(g_cls), p(g_dif), B, M, G, num_cls, float(threshold), utils.iou.torch.EPS, p(tp), p(cls_num))
    if dev.type == 'cuda':
        _hip.multi([(_hip.MULTI_ZERO, cls_num, None)])
        _hip.check(_hip.lib().y2_eval_match(*args, _hip.stream()), 'y2_eval_match')
    else:
        cls_num.zero_()
        _hip.check(_hip.lib().y2_eval_match_host(*args), 'y2_eval_match_host')
    return tp.view(torch.bool), cls_num


def voc_ap(rec, prec, use_07_metric=False):
    """eval.py:78-109: VOC average precision from recall / precision (float64): the 11-point metric of VOC07 or the area under the precision envelope."""
    rec, prec = np.asarray(rec, np.float64), np.asarray(prec, np.float64)
    if use_07_metric:
        ap = 0.
        for t in np.arange(0., 1.1, 0.1):
            p = 0 if np.sum(rec >= t) == 0 else np.max(prec[rec >= t])
            ap = ap + p / 11.
        return ap
    mrec = np.concatenate(([0.], rec, [1.]))
    mpre = np.concatenate(([0.], prec, [0.]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def average_precision(config, tp, num, dtype=np.float64):
    """eval.py:112-121: tp = the true-positive flags of one class in descending-score order, num = its valid ground-truth boxes."""
    tp = np.asarray(tp, bool)
    fp = np.cumsum(~tp)
    tp = np.cumsum(tp)
    rec = tp / num if num > 0 else np.zeros(len(tp), dtype=dtype)
    prec = tp / np.maximum(tp + fp, np.finfo(dtype).eps)
    return voc_ap(rec, prec, config.getboolean('eval', 'metric07'))


def merge_ap(config, cls_num, cls_score, cls_tp):
    """eval.py:294-301: {class: AP} for the classes with ground truth.  The detections of a class are put in descending-score order with
    `np.argsort(-score, kind='stable')`.  The reference calls np.argsort with its default, unstable kind: for equal scores with different flags
    its own result is not defined by its source; the stable order (accumulation order among equals) is this mirror's choice."""
    cls_ap = {}
    for c, (num, score, tp) in enumerate(zip(cls_num, cls_score, cls_tp)):
        if num > 0:
            indices = np.argsort(-np.asarray(score), kind='stable')
            cls_ap[c] = average_precision(config, np.asarray(tp, bool)[indices], num)
    return cls_ap


def _eval_config(iou, metric07):
    config = configparser.ConfigParser()
    config.read_dict({'eval': {'iou': repr(float(iou)), 'metric07': '1' if metric07 else '0'}})
    return config


class Accumulator(object):
    """mAP of a detection run, batch by batch, with the matching on the device: stat_ap + merge_ap of the reference (eval.py:257-301) without
    its per-image, per-class host traffic.  Accumulator(config, num_cls=C) reads `[eval] iou` and `[eval] metric07`; Accumulator(num_cls=C,
    iou=0.5, metric07=False) needs no config.

    update() launches y2_eval_match and keeps the batch's tp / score / cls tensors where they are (references, not copies: hand it buffers that
    the next batch does not overwrite - every tensor of detect.expand_batch's dict is allocated per call) and a copy of the small `count`.  Nothing crosses to the host until
    result(); only when the padded tensors kept so far exceed `max_bytes` are they compacted (torch boolean indexing, one synchronisation -
    every few hundred batches at the default 256 MB)."""

    def __init__(self, config=None, num_cls=None, iou=0.5, metric07=False, max_bytes=256 << 20):
        if config is not None:
            iou = config.getfloat('eval', 'iou', fallback=iou)
            metric07 = config.getboolean('eval', 'metric07', fallback=metric07)
        if num_cls is None or num_cls < 1:
            raise ValueError('Accumulator: num_cls (the number of categories) is required')
        self.num_cls, self.iou, self.metric07, self.max_bytes = int(num_cls), float(iou), bool(metric07), int(max_bytes)
        self.cls_num = None
        self._padded, self._flat, self._bytes, self._scales = [], [], 0, {}

    def _scale(self, dev, size):
        key = (str(dev), float(size[0]), float(size[1]))
        t = self._scales.get(key)
        if t is None:
            t = self._scales[key] = torch.tensor([float(size[0]), float(size[1])], dtype=torch.float32).view(1, 1, 2).to(dev)
        return t

    def update(self, data, dets, image_size=None, grid=None):
        """data: the batch's labels (yx_min / yx_max [B,G,2], cls [B,G], difficult [B,G]); dets: detect.expand_batch's dict.
        image_size = (H, W): the label boxes are in pixels and are divided by it (norm_bbox_data, eval.py:124-129); grid = (rows, cols): the
        predicted boxes are in cells (norm_bbox_pred, :132-137).  Both divisions are fp32 torch divisions like the reference's."""
        g_min, g_max = data['yx_min'], data['yx_max']
        d_min, d_max = dets['yx_min'], dets['yx_max']
        if image_size is not None:
            s = self._scale(g_min.device, image_size)
            g_min, g_max = g_min.float() / s, g_max.float() / s
        if grid is not None:
            s = self._scale(d_min.device, grid)
            d_min, d_max = d_min.float() / s, d_max.float() / s
        tp, cls_num = match_batch(g_min, g_max, data['cls'], data['difficult'], dict(yx_min=d_min, yx_max=d_max, cls=dets['cls'], count=dets['count']), self.iou, self.num_cls)
        self.cls_num = cls_num.to(torch.int64) if self.cls_num is None else self.cls_num + cls_num
        kept = (tp, dets['score'].to(tp.device), dets['cls'].to(tp.device), dets['count'].to(tp.device).clone())
        self._padded.append(kept)
        self._bytes += sum(t.numel() * t.element_size() for t in kept)
        if self._bytes > self.max_bytes:
            self._compact()
        return tp

    def _compact(self):
        for tp, score, cls, count in self._padded:
            mask = torch.arange(tp.size(1), device=tp.device).view(1, -1) < count.view(-1, 1)
            self._flat.append((tp[mask], score[mask], cls[mask]))
        self._padded, self._bytes = [], 0

    def collect(self):
        """(cls_num, cls_score, cls_tp) like stat_ap (eval.py:257-292), per class in accumulation order: ONE device-to-host copy."""
        if self.cls_num is None:
            return [0] * self.num_cls, [np.zeros(0, np.float32)] * self.num_cls, [np.zeros(0, bool)] * self.num_cls
        self._compact()
        tp, score, cls = (torch.cat([f[i] for f in self._flat]) for i in range(3))
        self._flat = [(tp, score, cls)]
        n = tp.numel()
        packed = torch.cat([score.float().contiguous().view(torch.int32), cls.to(torch.int32), tp.to(torch.int32), self.cls_num.to(torch.int32)]).cpu().numpy()
        score, cls, tp, cls_num = packed[:n].view(np.float32), packed[n:2 * n], packed[2 * n:3 * n].astype(bool), packed[3 * n:]
        sel = [cls == c for c in range(self.num_cls)]
        return [int(v) for v in cls_num], [score[m] for m in sel], [tp[m] for m in sel]

    def result(self, metric07=None):
        """{class: AP} for the classes with valid ground truth (merge_ap)."""
        return merge_ap(_eval_config(self.iou, self.metric07 if metric07 is None else metric07), *self.collect())

    def mean_ap(self, metric07=None):
        return float(np.mean(list(self.result(metric07).values())))
