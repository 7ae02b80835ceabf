"""`detect` — detection post-filter of YOLOv2, MI355X-native mirror of detect.py:43-80.

`filter_visible` / `postprocess` keep the reference's signatures (one image, config-driven thresholds);
`postprocess_batch` is the device-resident form of the same a20 -> a21 -> a22 chain for a whole
batch: decode+softmax+max (y2_decode), threshold compaction (y2_filter_visible), rank + greedy NMS (y2_nms),
with no host round trip between the stages.

`Detector` is the front and the back the reference's `Detect` class (detect.py:83-175) puts around them, for FILES: pictures -> utils.data.collate_images
(`[transform] resize_test`: transform.resize.image, `rescale` or `fixed`) -> utils.data.to_device (one y2_collate_images or y2_fixed_images launch) ->
the network and the chain above in a captured graph -> boxes in the pixels of each source picture (`to_source`).  `main` is the command line: a
file or a directory of pictures in, annotated pictures and detections.tsv out.  Two deliberate deviations from the reference, both in `to_source`:
the reference caches the scale of the FIRST frame (`self.scale`, right for a video and wrong for a directory of pictures) - here it is computed per
picture; and it applies the `rescale` formula under `fixed` as well, which misplaces every box of a letterboxed picture - here the map is the inverse
of the transform that was applied.  Camera and video input, the OpenCV window and the video writer stay out: they need cv2.
"""
import argparse
import configparser
import inspect
import logging
import logging.config
import os

import numpy as np
import torch

import _hip
import model
import utils
import utils.postprocess


def get_logits(pred):
    """detect.py:43-48."""
    if 'logits' in pred:
        return pred['logits'].contiguous()
    else:
        return torch.ones(*pred['iou'].size(), 1, device=pred['iou'].device)


def filter_visible_batch(iou, prob_cls, fix, thr):
    """iou, prob_cls [B,n] -> (count int32 [B], index int32 [B,n]); detect.py:53-62 for every image at once."""
    _hip.require_gpu(iou, prob_cls)
    iou, prob_cls = _hip.f32c(iou), _hip.f32c(prob_cls)
    B, n = iou.shape
    count = torch.empty(B, dtype=torch.int32, device=iou.device)
    index = torch.empty(B, max(n, 1), dtype=torch.int32, device=iou.device)
    _hip.check(_hip.lib().y2_filter_visible(_hip.ptr(iou), None, B, n, 1, int(bool(fix)), float(thr), _hip.ptr(count), _hip.ptr(index),
                                            _hip.ptr(prob_cls), None, _hip.stream()), 'y2_filter_visible')
    return count, index


def filter_visible(config, iou, yx_min, yx_max, prob):
    """detect.py:51-63, one image: iou [n], yx_min/yx_max [n,2], prob [n,C]."""
    _hip.require_gpu(iou, prob)
    iou, prob = _hip.f32c(iou).view(1, -1), _hip.f32c(prob)
    n, C = iou.size(1), prob.size(-1)
    fix = config.getboolean('detect', 'fix')
    thr = config.getfloat('detect', 'threshold_cls') if fix else config.getfloat('detect', 'threshold')
    dev = iou.device
    count = torch.empty(1, dtype=torch.int32, device=dev)
    index = torch.empty(1, max(n, 1), dtype=torch.int32, device=dev)
    prob_cls = torch.empty(1, max(n, 1), dtype=torch.float32, device=dev)
    cls = torch.empty(1, max(n, 1), dtype=torch.int32, device=dev)
    _hip.check(_hip.lib().y2_filter_visible(_hip.ptr(iou), _hip.ptr(prob.view(-1, C)), 1, n, C, int(fix), thr, _hip.ptr(count), _hip.ptr(index),
                                            _hip.ptr(prob_cls), _hip.ptr(cls), _hip.stream()), 'y2_filter_visible')
    idx = index[0, :int(count.item())].long()
    return (iou[0][idx], yx_min.view(-1, 2)[idx], yx_max.view(-1, 2)[idx], prob.view(-1, C)[idx], prob_cls[0][idx], cls[0][idx].long())


def _expand(iou, prob, yx_min, yx_max, cand, keep, keep_count, fix, threshold_cls):
    """y2_expand_classes: survivors of every image gathered and (fix) expanded into (box, class) detections.  iou [B,n], prob [B,n,C],
    yx_min / yx_max [B,n,2], cand int32 [B,n] or None, keep int32 [B,limit], keep_count int32 [B]."""
    B, limit = keep.shape
    n, C = iou.size(1), prob.size(-1)
    dev = iou.device
    new = lambda *s, **kw: torch.empty(*s, device=dev, **kw)
    k_iou, k_min, k_max = new(B, limit), new(B, limit, 2), new(B, limit, 2)
    if fix:
        e_min, e_max, e_score = new(B, limit * C, 2), new(B, limit * C, 2), new(B, limit * C)
        e_cls, e_count = new(B, limit * C, dtype=torch.int64), new(B, dtype=torch.int32)
    else:
        e_min = e_max = e_score = e_cls = e_count = None
    _hip.check(_hip.lib().y2_expand_classes(_hip.ptr(iou), _hip.ptr(prob), _hip.ptr(yx_min), _hip.ptr(yx_max), _hip.ptr(cand), _hip.ptr(keep), _hip.ptr(keep_count),
                                            B, n, C, limit, float(threshold_cls), _hip.ptr(k_iou), _hip.ptr(k_min), _hip.ptr(k_max),
                                            _hip.ptr(e_min), _hip.ptr(e_max), _hip.ptr(e_score), _hip.ptr(e_cls), _hip.ptr(e_count), _hip.stream()), 'y2_expand_classes')
    return k_iou, k_min, k_max, e_min, e_max, e_score, e_cls, e_count


def postprocess(config, iou, yx_min, yx_max, prob):
    """detect.py:66-80, one image: visibility filter -> NMS on objectness -> per-class expansion (`[detect] fix`) or arg-max class.
    Returns (iou, yx_min, yx_max, cls, score) or None when nothing survives."""
    iou, yx_min, yx_max, prob, prob_cls, cls = filter_visible(config, iou, yx_min, yx_max, prob)
    keep = utils.postprocess.nms(iou, yx_min, yx_max, config.getfloat('detect', 'overlap'))
    if not keep:
        return None
    fix = config.getboolean('detect', 'fix')
    k = len(keep)
    dev = iou.device
    keep_t = torch.tensor(keep, dtype=torch.int32, device=dev).view(1, k)
    count = torch.tensor([k], dtype=torch.int32, device=dev)
    k_iou, k_min, k_max, e_min, e_max, e_score, e_cls, e_count = _expand(_hip.f32c(iou).view(1, -1), _hip.f32c(prob).view(1, iou.numel(), -1), _hip.f32c(yx_min).view(1, -1, 2),
                                                                        _hip.f32c(yx_max).view(1, -1, 2), None, keep_t, count, fix, config.getfloat('detect', 'threshold_cls'))
    if fix:
        m = int(e_count.item())
        return k_iou[0], e_min[0, :m], e_max[0, :m], e_cls[0, :m], e_score[0, :m]
    return k_iou[0], k_min[0], k_max[0], cls[keep_t[0].long()], k_iou[0]


def detect_batch(feature_nhwc, anchors, fix=False, threshold=0.3, threshold_cls=0.005, overlap=0.45, limit=200):
    """Device-resident a8 -> a19 -> a20 -> a21: head image [B,rows,cols,A*(5+C)] -> dict of GPU tensors:
    decoded boxes/probabilities, per-image candidate list (count, index) and NMS survivors (keep = positions in the
    candidate list, keep_count).  No host synchronisation."""
    A = anchors.size(0)
    d = model.decode(feature_nhwc, anchors, A, want_prob=True)
    B = feature_nhwc.size(0)
    n = d['iou'].numel() // B
    iou = d['iou'].view(B, n)
    thr = threshold_cls if fix else threshold
    count, index = filter_visible_batch(iou, d['prob_cls'].view(B, n), fix, thr)
    keep, keep_count = utils.postprocess.nms_batch(iou, d['yx_min'].view(B, n, 2), d['yx_max'].view(B, n, 2), count, overlap, limit, cand=index)
    d.update(count=count, index=index, keep=keep, keep_count=keep_count)
    return d


def postprocess_batch(d, fix=False, threshold_cls=0.005, to_host=False):
    """a22 (detect.py:69-79) for every image of a detect_batch result: ONE launch (y2_expand_classes: gather of the survivors and, with
    `fix`, their expansion into (box, class) detections in row-major order) and one host synchronisation for the counts.
    Returns a list (per image) of None or (iou, yx_min, yx_max, cls, score) GPU tensors (views of the batch's result buffers).
    to_host: the tuples hold CPU tensors - the whole batch's result buffers cross PCIe in ONE copy per buffer (six copies, one synchronisation) and are sliced
    on the host, instead of five small copies and a synchronisation per image (what calling .cpu() on the GPU views costs: the consumer of the reference's
    postprocess works on the host, utils/postprocess.py:34-49 returns a Python list)."""
    keep = d['keep']
    B, limit = keep.shape
    n = d['iou'].numel() // B
    k_iou, k_min, k_max, e_min, e_max, e_score, e_cls, e_count = _expand(d['iou'].view(B, n), d['prob'].view(B, n, -1), d['yx_min'].view(B, n, 2), d['yx_max'].view(B, n, 2),
                                                                        d['index'], keep, d['keep_count'], fix, threshold_cls)
    if to_host and fix:
        bufs = [t.to('cpu', non_blocking=True) for t in (torch.stack([d['keep_count'], e_count]), k_iou, e_min, e_max, e_cls, e_score)]
        torch.cuda.current_stream().synchronize()
        counts, h_iou, h_min, h_max, h_cls, h_score = bufs[0].tolist(), bufs[1], bufs[2], bufs[3], bufs[4], bufs[5]
        return [None if counts[0][b] == 0 else (h_iou[b, :counts[0][b]], h_min[b, :counts[1][b]], h_max[b, :counts[1][b]], h_cls[b, :counts[1][b]], h_score[b, :counts[1][b]]) for b in range(B)]
    counts = (torch.stack([d['keep_count'], e_count]) if fix else d['keep_count'].view(1, B)).tolist()      # the one host round trip
    out = []
    for b in range(B):
        k = counts[0][b]
        if k == 0:
            out.append(None)
        elif fix:
            m = counts[1][b]
            out.append((k_iou[b, :k], e_min[b, :m], e_max[b, :m], e_cls[b, :m], e_score[b, :m]))
        else:
            src = d['index'][b].long()[keep[b, :k].long()]
            out.append((k_iou[b, :k], k_min[b, :k], k_max[b, :k], d['cls'].view(B, n)[b][src].long(), k_iou[b, :k]))
    if to_host:
        out = [None if r is None else tuple(t.cpu() for t in r) for r in out]
    return out


def expand_batch(d, fix=False, threshold_cls=0.005):
    """The batch form of postprocess_batch for consumers that stay on the device (eval.match_batch): the result buffers of a detect_batch result
    as a dict of device tensors - yx_min / yx_max [B,M,2], cls int64 [B,M], score [B,M], count int32 [B] - with NO host synchronisation.  Rows
    [0, count[b]) of image b are what postprocess_batch returns for it, in values and order; the rows behind them are not meaningful.
    fix: M = limit * C (the expanded detections); otherwise M = limit (the NMS survivors with their arg-max class).
    Every returned tensor is allocated by this call (count too: without `fix` it is a copy of d['keep_count'], an asynchronous device copy), so a
    consumer may keep the dict while `d` - the static result of a GraphedDetector, say - is overwritten by the next batch."""
    keep = d['keep']
    B, limit = keep.shape
    n = d['iou'].numel() // B
    k_iou, k_min, k_max, e_min, e_max, e_score, e_cls, e_count = _expand(d['iou'].view(B, n), d['prob'].view(B, n, -1), d['yx_min'].view(B, n, 2), d['yx_max'].view(B, n, 2),
                                                                        d['index'], keep, d['keep_count'], fix, threshold_cls)
    if fix:
        return dict(yx_min=e_min, yx_max=e_max, cls=e_cls, score=e_score, count=e_count)
    # cls[b, k] = cls[b, index[b, keep[b, k]]]: keep beyond keep_count (and index beyond count) is whatever the buffers held - clamped, so that no gather leaves its row
    src = d['index'].long().gather(1, keep.long().clamp_(0, n - 1)).clamp_(0, n - 1)
    return dict(yx_min=k_min, yx_max=k_max, cls=d['cls'].view(B, n).long().gather(1, src), score=k_iou, count=d['keep_count'].clone())


class GraphedDetector(object):
    """hipGraph capture of the whole device-resident detect step (conv stack + decode + filter + NMS, ~30 launches) for a
    fixed input shape: one graph launch per batch instead of ~30 kernel launches and ~40 tensor allocations from Python.
    `run(x)` copies x into the static input buffer, replays the graph and returns the static result dict (overwritten
    by the next run).  `static_input=True` captures on `example` itself (no private copy): `run()` then re-reads that tensor.
    The graph bakes in the pointers of the packed / folded weights: after the parameters change (optimizer step, load_state_dict,
    a training forward) a replay would use stale weights, so `run` checks the plugin's cache key and refuses."""

    def __init__(self, dnn, anchors, example, fix=True, threshold=0.3, threshold_cls=0.005, overlap=0.45, limit=200, warmup=2, static_input=False, slot=0):
        """slot: detectors captured in different slots own different intermediate buffers (model.yolo2.Darknet.forward_nhwc) and may be
        replayed concurrently on different streams; detectors of one slot share them and must be replayed one after the other."""
        self.static_x = example if static_input else example.clone()
        self.dnn = dnn
        kw = dict(fix=fix, threshold=threshold, threshold_cls=threshold_cls, overlap=overlap, limit=limit)

        def step():
            with torch.no_grad():
                return detect_batch(dnn.forward_nhwc(self.static_x, slot) if slot else dnn.forward_nhwc(self.static_x), anchors, **kw)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):          # warm-up on a side stream: one-time attribute/symbol calls, plan + weight packing
            for _ in range(warmup):
                step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.result = step()
        # what the captured pointers were derived from: the tensors themselves (kept alive here) with their version counters - the check in
        # run() is one attribute read per tensor, no module-tree walk (it sits in the replay path)
        self._watched = [(t, t.data_ptr(), t._version) for t in list(dnn.parameters()) + list(dnn.buffers())]
        # the graph bakes in the addresses of the plan's intermediate buffers and scratch: hold the plan, so that an eviction from the
        # plugin's plan LRU (a 13th input shape) cannot hand that memory to somebody else while this graph can still be replayed
        plans = getattr(dnn, '_plans', None)
        self._plan = plans.latest() if plans is not None else None

    def run(self, x=None):
        for t, ptr, ver in self._watched:
            if t._version != ver or t.data_ptr() != ptr:
                raise RuntimeError('GraphedDetector: the parameters changed since capture (the graph holds the old packed weights); capture a new one')
        if x is not None and x.data_ptr() != self.static_x.data_ptr():
            self.static_x.copy_(x)
        self.graph.replay()
        return self.result


def to_source(yx, record, rows, cols, height, width):
    """Box corners `yx` [n, 2] in cells of the rows x cols head image -> pixels of the SOURCE picture (float32 numpy, unclipped).  `record`: the
    picture's sample dict after its transform.resize.image transform; (height, width): the network input.
    `rescale` (record['window'] = the whole src_h x src_w picture): yx * (src_h / rows, src_w / cols), the reference's detect.py:160-162.
    `fixed` (record['fixed']): the picture was scaled by `scale` into the top-left of the canvas, so yx * (height / rows, width / cols) / scale - the
    inverse of the transform that was applied (the reference applies the `rescale` formula here too, and caches the scale of its first frame:
    both are deliberately not reproduced)."""
    if 'fixed' in record:
        scale = float(record['fixed']['scale'])
        factor = (height / rows / scale, width / cols / scale)
    else:
        _, _, src_h, src_w = record['window']
        factor = (src_h / rows, src_w / cols)
    return np.asarray(yx, np.float32).reshape(-1, 2) * np.array(factor, np.float32)


def parse_resize(config, method):
    """`[transform] resize_test` -> the transform object, as the reference's transform.parse_transform: the dotted name is resolved with
    utils.parse_attr and called with the config when it takes one argument, without arguments otherwise."""
    if not isinstance(method, str):
        return method
    attr = utils.parse_attr(method)
    return attr(config) if len(inspect.signature(attr).parameters) == 1 else attr()


def image_options(config):
    """(swap_rb, normalize) of `[transform] image_test` and `[transform] tensor`: what utils.data.collate_images takes.  The test path has no
    jitter: a sequence other than nothing or BGR2RGB raises."""
    import transform.image
    jitter = transform.image.get_transform(config, config.get('transform', 'image_test', fallback='transform.image.BGR2RGB').split())
    if jitter.active:
        raise ValueError('[transform] image_test: the test path serves BGR2RGB only')
    normalize = None
    for name in config.get('transform', 'tensor', fallback='torchvision.transforms.ToTensor transform.image.Normalize').split():
        if name == 'transform.image.Normalize':
            plugin = transform.image.Normalize(config)
            normalize = (plugin.mean, plugin.std)
        elif name != 'torchvision.transforms.ToTensor':
            raise ValueError('[transform] tensor: %s is not served by the level table (ToTensor and transform.image.Normalize are)' % name)
    return jitter.swap_rb, normalize


class Detector(object):
    """Pictures in, boxes in source pixels out.  Reads `[image] size`, `[transform] resize_test` (transform.resize.image.Resize / Rescale / Fixed),
    `[transform] image_test` / `tensor` (BGR2RGB, Normalize) and `[detect] fix` / `threshold` / `threshold_cls` / `overlap`.
    dnn: a plugin on the GPU in eval mode with `forward_nhwc`; anchors: the (height, width) table in cells.
    One GraphedDetector is captured per batch size and kept; to_device writes straight into its static input."""

    def __init__(self, config, dnn, anchors, device=None):
        import utils.data
        self.config, self.dnn = config, dnn
        device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device.type == 'cuda' and device.index is None else device
        self.anchors = anchors.to(self.device, torch.float32).contiguous()
        self.height, self.width = (int(v) for v in config.get('image', 'size').split())
        self.resize = parse_resize(config, config.get('transform', 'resize_test'))
        self.swap_rb, self.normalize = image_options(config)
        self.fix = config.getboolean('detect', 'fix')
        self.kwargs = dict(fix=self.fix, threshold=config.getfloat('detect', 'threshold'), threshold_cls=config.getfloat('detect', 'threshold_cls'),
                           overlap=config.getfloat('detect', 'overlap'))
        utils.data.level_table(self.normalize, self.device)          # (its first call copies from pageable memory)
        self._graphs = {}

    def collate(self, images):
        """(samples, batch): the sample dicts after the resize transform and the dict of utils.data.collate_images."""
        import utils.data
        samples = [dict(image=utils.data.read_image(image) if isinstance(image, (str, os.PathLike)) else image) for image in images]
        return samples, utils.data.collate_images(samples, self.resize, self.height, self.width, self.swap_rb, self.normalize)

    def __call__(self, images):
        """images: uint8 [h, w, 3] BGR arrays, utils.data.JpegImage objects or paths.  Returns, per picture, None or (yx_min [n, 2], yx_max [n, 2],
        cls [n], score [n]) as numpy arrays, the corners in pixels of that picture, unclipped, as the reference leaves them."""
        import utils.data
        if not len(images):
            return []
        samples, batch = self.collate(images)
        B = len(samples)
        with torch.cuda.device(self.device):
            entry = self._graphs.get(B)
            if entry is None:
                x = utils.data.to_device(batch, self.device)['tensor']
                with torch.no_grad():
                    rows, cols = self.dnn.forward_nhwc(x).shape[1:3]
                entry = self._graphs[B] = (GraphedDetector(self.dnn, self.anchors, x, static_input=True, **self.kwargs), int(rows), int(cols))
            else:
                utils.data.to_device(batch, self.device, out=entry[0].static_x)
            graphed, rows, cols = entry
            results = postprocess_batch(graphed.run(), self.fix, self.kwargs['threshold_cls'], to_host=True)
        out = []
        for record, result in zip(samples, results):
            if result is None:
                out.append(None)
                continue
            _, yx_min, yx_max, cls, score = result
            out.append((to_source(yx_min.numpy(), record, rows, cols, self.height, self.width), to_source(yx_max.numpy(), record, rows, cols, self.height, self.width),
                        cls.numpy().copy(), score.numpy().copy()))
        return out


PICTURES = ('.jpg', '.jpeg', '.png')
VIDEOS = ('.avi', '.mp4', '.mkv', '.mov', '.mpg', '.mpeg', '.webm', '.flv', '.wmv')


def list_pictures(path):
    """The picture files of `-i`: the file itself, or the .jpg / .jpeg / .png files of a directory in sorted order.  A camera index or a video file
    raises: both need cv2, which this workflow does without."""
    try:
        int(path)
    except ValueError:
        pass
    else:
        raise NotImplementedError('-i %s is a camera: capture needs cv2 (OpenCV), which is not available; give a picture file or a directory of pictures' % path)
    path = os.path.expanduser(os.path.expandvars(path))
    if os.path.splitext(path)[1].lower() in VIDEOS:
        raise NotImplementedError('-i %s is a video: reading it needs cv2 (OpenCV), which is not available; give a picture file or a directory of pictures' % path)
    if os.path.isdir(path):
        return [os.path.join(path, name) for name in sorted(os.listdir(path)) if os.path.splitext(name)[1].lower() in PICTURES]
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    return [path]


def build_detector(config, category):
    """The newest checkpoint of the model directory, its plugin on the current GPU, and the Detector around it (detect.py:84-106)."""
    import utils.train
    anchors = torch.from_numpy(utils.get_anchors(config)).contiguous()
    path, step, epoch = utils.train.load_model(utils.get_model_dir(config))
    state_dict = torch.load(path, map_location='cpu')
    dnn = utils.parse_attr(config.get('model', 'dnn'))(model.ConfigChannels(config, state_dict), anchors, len(category))
    dnn.load_state_dict(state_dict)
    return Detector(config, dnn.eval().cuda(), anchors)


def main(argv=None, detector=None):
    """detect.py -c config.ini -i pictures/ -o out/: every picture of the input, `-b` at a time, through the Detector; per picture the annotated
    copy (rectangles, a colour per class; no text: there is no font renderer without cv2) written with Pillow under its own name, and one
    detections.tsv (file, class name, score, ymin, xmin, ymax, xmax in source pixels).  detector: an object called like Detector (tests)."""
    from PIL import Image

    import utils.data
    import utils.visualize
    args = make_args(argv)
    config = configparser.ConfigParser()
    utils.load_config(config, args.config)
    for cmd in args.modify:
        utils.modify_config(config, cmd)
    if args.logging:
        import yaml
        with open(os.path.expanduser(os.path.expandvars(args.logging)), 'r') as f:
            logging.config.dictConfig(yaml.safe_load(f))
    paths = list_pictures(args.input)
    cache_dir = utils.get_cache_dir(config)
    category = utils.get_category(config, cache_dir if os.path.exists(cache_dir) else None)
    draw_bbox = utils.visualize.DrawBBox(category, colors=args.colors, thickness=args.thickness)
    if detector is None:
        detector = build_detector(config, category)
    output = os.path.expanduser(os.path.expandvars(args.output))
    os.makedirs(output, exist_ok=True)
    with open(os.path.join(output, 'detections.tsv'), 'w') as tsv:
        tsv.write('file\tclass\tscore\tymin\txmin\tymax\txmax\n')
        for first in range(0, len(paths), args.batch_size):
            batch = paths[first:first + args.batch_size]
            for path, result in zip(batch, detector(batch)):
                image = utils.data.imread_host(path)          # the pictures stay on the host: drawing is a few slices per box
                name = os.path.basename(path)
                if result is not None:
                    yx_min, yx_max, cls, score = result
                    image = draw_bbox(image, yx_min.astype(np.int64), yx_max.astype(np.int64), cls)
                    for (ymin, xmin), (ymax, xmax), c, s in zip(yx_min.tolist(), yx_max.tolist(), cls.tolist(), score.tolist()):
                        tsv.write('%s\t%s\t%.6f\t%.2f\t%.2f\t%.2f\t%.2f\n' % (name, category[int(c)], s, ymin, xmin, ymax, xmax))
                Image.fromarray(np.ascontiguousarray(image[..., ::-1])).save(os.path.join(output, name))
            logging.info('%d / %d pictures', min(first + args.batch_size, len(paths)), len(paths))
    return 0


def make_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('-c', '--config', nargs='+', default=['config.ini'], help='config file')
    parser.add_argument('-m', '--modify', nargs='+', default=[], help='modify config')
    parser.add_argument('-i', '--input', required=True, help='a picture file or a directory of .jpg / .jpeg / .png files')
    parser.add_argument('-o', '--output', required=True, help='output directory: the annotated pictures and detections.tsv')
    parser.add_argument('-b', '--batch_size', default=16, type=int)
    parser.add_argument('--thickness', default=3, type=int)
    parser.add_argument('--colors', nargs='+', default=[])
    parser.add_argument('--logging', default=None, help='logging config (yaml), optional')
    args = parser.parse_args(argv)
    if args.batch_size < 1:
        parser.error('--batch_size must be positive')
    return args


if __name__ == '__main__':
    main()
