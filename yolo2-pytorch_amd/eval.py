"""`eval` — the VOC evaluation of the reference (eval.py): the matching and mAP arithmetic, the `Eval` class and the command line.

`matching` / `_matching` mirror the reference per (image, class) on the IoU kernel (y2_iou_rowmax).  `match_batch` is the batch form of the whole
loop eval.py:278-292 - filter_valid, the per-class ground-truth counts, filter_cls_*, matching - as ONE launch (y2_eval_match; CPU tensors:
y2_eval_match_host), and `Accumulator` carries its flags to `voc_ap` / `average_precision` / `merge_ap` (host numpy float64, like the reference)
without host traffic per image or class.

`Eval(args, config)()` is the reference's class around them: the newest checkpoint of the model directory, the `[eval] phase` cache files through
utils.data.Dataset / Collate (`[transform] resize_eval`, the single `[image] size`), and per batch utils.data.to_device -> the network ->
detect.detect_batch / expand_batch -> Accumulator.update, with nothing crossing to the host until the end.  It returns {class index: AP}, logs
`name=AP` and the mean, and appends one row to `[eval] db` as plain JSON in TinyDB's file layout, {"_default": {"1": row, "2": row, ...}}.
`python eval.py -c config.ini [-m section/option=value ...] [-b 64] [--logging logging.yml]` is `main`.  Not here: the xlsx report (xlsxwriter)
and the `[eval] mapper` file that names the reference's columns - the row has fixed keys instead (`save_db`)."""
import argparse
import configparser
import datetime
import json
import logging
import logging.config
import os

import numpy as np
import torch

import _hip
import utils
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


def save_db(path, row):
    """Append `row` (a JSON-serialisable dict) to the evaluation database `path`: {"_default": {"1": row, "2": row, ...}}, the file layout the
    reference reads back with json.load(f)['_default'].  Returns the row's key."""
    table = {}
    if os.path.exists(path):
        with open(path) as f:
            table = json.load(f).get('_default', {})
    key = str(max([int(k) for k in table] + [0]) + 1)
    table[key] = row
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + '.tmp'
    with open(tmp, 'w') as f:
        json.dump({'_default': table}, f)
    os.replace(tmp, path)
    return key


class Eval(object):
    """The reference's class of this name (eval.py:165-347) on the device-resident pieces.  args: `batch_size`; config: `[eval]`, `[detect]`,
    `[image] size`, `[transform] resize_eval` / `image_test` / `tensor`, `[data] workers`.
    detector (tests): an object called with the device batch (the dict of utils.data.to_device) in place of the network and the detection chain; it
    returns a dict like detect.expand_batch's, with the boxes in cells of `grid=(rows, cols)` when it carries that key and as fractions of the image
    otherwise.  With a detector no checkpoint is loaded onto a device (its step and epoch are still read for the database row)."""

    def __init__(self, args, config, detector=None):
        import model
        import utils.train
        self.args, self.config, self.detector = args, config, detector
        self.model_dir = utils.get_model_dir(config)
        self.cache_dir = utils.get_cache_dir(config)
        self.category = utils.get_category(config, self.cache_dir)
        self.anchors = torch.from_numpy(utils.get_anchors(config)).contiguous()
        self.size = tuple(int(v) for v in config.get('image', 'size').split())
        self.fix = config.getboolean('detect', 'fix')
        self.kwargs = dict(fix=self.fix, threshold=config.getfloat('detect', 'threshold'), threshold_cls=config.getfloat('detect', 'threshold_cls'),
                           overlap=config.getfloat('detect', 'overlap'))
        self.loader = self.get_loader()
        self.path, self.step, self.epoch = utils.train.load_model(self.model_dir)
        if detector is None:
            state_dict = torch.load(self.path, map_location='cpu')
            dnn = utils.parse_attr(config.get('model', 'dnn'))(model.ConfigChannels(config, state_dict), self.anchors, len(self.category))
            dnn.load_state_dict(state_dict)
            self.dnn = dnn.eval().cuda()
            self.anchors_device = self.anchors.to(next(self.dnn.parameters()).device, torch.float32).contiguous()
        self.now = datetime.datetime.now()

    def get_loader(self):
        import detect
        import utils.data
        paths = [os.path.join(self.cache_dir, phase + '.pkl') for phase in self.config.get('eval', 'phase').split()]
        dataset = utils.data.Dataset(utils.data.load_pickles(paths))
        logging.info('num_examples=%d' % len(dataset))
        try:
            workers = self.config.getint('data', 'workers')
        except (configparser.NoSectionError, configparser.NoOptionError):
            workers = min(os.cpu_count() or 1, 16)
        swap_rb, normalize = detect.image_options(self.config)
        collate_fn = utils.data.Collate(detect.parse_resize(self.config, self.config.get('transform', 'resize_eval')), [self.size], swap_rb=swap_rb, normalize=normalize)
        return torch.utils.data.DataLoader(dataset, batch_size=self.args.batch_size, num_workers=workers, collate_fn=collate_fn, pin_memory=torch.cuda.is_available())

    def detect(self, data):
        """(detections, grid) of one device batch: the sequence tools/eval_bench.py times."""
        import detect
        if self.detector is not None:
            dets = self.detector(data)
            return dets, dets.get('grid')
        with torch.no_grad():
            feature = self.dnn.forward_nhwc(data['tensor'])
            d = detect.detect_batch(feature, self.anchors_device, **self.kwargs)
            return detect.expand_batch(d, self.fix, self.kwargs['threshold_cls']), tuple(feature.shape[1:3])

    def stat_ap(self):
        import utils.data
        acc = Accumulator(self.config, num_cls=len(self.category))
        for batch in self.loader:
            data = utils.data.to_device(batch)
            dets, grid = self.detect(data)
            acc.update(data, dets, image_size=self.size, grid=grid)
        return acc

    def logging(self, cls_ap):
        for c in cls_ap:
            logging.info('%s=%f' % (self.category[c], cls_ap[c]))
        logging.info(np.mean(list(cls_ap.values())) if cls_ap else 'no class with ground truth')

    def row(self, cls_ap):
        return dict(timestamp=self.now.timestamp(), time=self.now.isoformat(), step=self.step, epoch=self.epoch, dnn=self.config.get('model', 'dnn'),
                    size='%d %d' % self.size, mean_ap=float(np.mean(list(cls_ap.values()))) if cls_ap else None,
                    cls_ap={self.category[c]: float(ap) for c, ap in cls_ap.items()})

    def __call__(self):
        cls_ap = self.stat_ap().result()
        save_db(utils.get_eval_db(self.config), self.row(cls_ap))
        self.logging(cls_ap)
        return cls_ap


def main(argv=None, detector=None):
    args = make_args(argv)
    config = configparser.ConfigParser()
    utils.load_config(config, args.config)
    for cmd in args.modify:
        utils.modify_config(config, cmd)
    if args.logging:
        import yaml
        with open(os.path.expanduser(os.path.expandvars(args.logging)), 'r') as f:
            logging.config.dictConfig(yaml.safe_load(f))
    return Eval(args, config, detector)()


def make_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('-c', '--config', nargs='+', default=['config.ini'], help='config file')
    parser.add_argument('-m', '--modify', nargs='+', default=[], help='modify config')
    parser.add_argument('-b', '--batch_size', default=16, type=int, help='batch size')
    parser.add_argument('--logging', default=None, help='logging config (yaml), optional')
    return parser.parse_args(argv)


if __name__ == '__main__':
    main()
