#!/usr/bin/env python
"""Timing of the collate step WITH the colour jitter on one MI355X; prints ONE JSON line.

Workload: the batches of tools/collate_bench.py (64 seeded source images of VOC-like sizes, one label box each) through RandomFlipHorizontally,
transform.resize.label.RandomCrop and utils.data.Collate with the reference's alternative `image_train` line (RandomBlur, BGR2HSV, RandomHue,
RandomSaturation, RandomBrightness, HSV2RGB, RandomGamma at config.ini's `[augmentation]` values), at 416x416 and 608x608.  Per size, on the same
data in the same process, the medians over the timed batches of the HIP-event times of
  (a) fp32_h2d_ms          one copy of the FINISHED fp32 [64,3,H,W] tensor from pinned memory: what the reference ships after jittering on the CPU
  (b) uint8_jitter_ms      utils.data.to_device on the pinned packed batch: the copies of raw and the tables, then y2_collate_jitter_images
  (c) the library entry points alone (tables and pixels on the device, 8 launches per event pair, the mean per launch), on the SAME pixels and geometry:
      full_ms              y2_collate_jitter_images with the batch's own tables: the full chain
      blur_ms              the batch's blur sizes, the plain colour path, the shared level table repeated per image: blur only
      hsv_ms               1x1 blurs, the batch's HSV and output tables: HSV + gamma only
      plain_ms             1x1 blurs, the plain colour path, the shared table: what y2_collate_images computes, through this kernel's LDS stages
      collate_ms           y2_collate_images: the yardstick (it writes the same bytes)
      *_gbs = (window bytes read + fp32 bytes written) / time
(a) and (b) alternate batch by batch; the five forms of (c) alternate event pair by event pair.  Four different batches rotate, so that neither the
source pixels nor the output of a launch are still in the 256 MB Infinity Cache from the launch before.  The finished tensor of (a) is the host
function's and is compared, once per size, with the device's.  `--runs 2` (the default) measures everything twice in the process and reports both.
    python tools/jitter_bench.py [--batch 64] [--sizes 416,608] [--batches 24] [--warmup 4] [--runs 2] [--blur "5 5"]"""
import argparse
import configparser
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'yolo2-pytorch_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

ROTATE = 4
IMAGE_TRAIN = 'RandomBlur BGR2HSV RandomHue RandomSaturation RandomBrightness HSV2RGB RandomGamma'
AUGMENTATION = {'random_flip_horizontally': '0.5', 'random_crop': '1', 'random_blur': '5 5', 'random_hue': '0 25', 'random_saturation': '0.5 1.5',
                'random_brightness': '0.5 1.5', 'random_gamma': '0.9 1.5'}


def make_batches(B, S, seed, blur='5 5'):
    import numpy as np

    import transform.augmentation
    import transform.image
    import transform.resize.label
    import utils.data
    config = configparser.ConfigParser()
    config.read_dict({'data': {'resize': 'rescale'}, 'augmentation': dict(AUGMENTATION, random_blur=blur)})
    flip = transform.augmentation.RandomFlipHorizontally(config)
    jitter = transform.image.get_transform(config, ['transform.image.' + n for n in IMAGE_TRAIN.split()])
    collate = utils.data.Collate(transform.resize.label.RandomCrop(config), [(S, S)], transform_image=jitter)
    rng = np.random.RandomState(seed)
    random.seed(seed)
    np.random.seed(seed)
    out = []
    for _ in range(ROTATE):
        samples = []
        for i in range(B):
            long_side, short_side = 500, int(rng.randint(333, 401))
            h, w = (short_side, long_side) if i % 3 else (long_side, short_side)
            lo = rng.uniform(0.1, 0.4, 2) * (h, w)
            hi = rng.uniform(0.6, 0.9, 2) * (h, w)
            samples.append(flip(dict(image=rng.randint(0, 256, (h, w, 3)).astype(np.uint8), yx_min=lo.astype(np.float32).reshape(1, 2),
                                     yx_max=hi.astype(np.float32).reshape(1, 2), cls=np.zeros(1, np.int64), difficult=np.zeros(1, np.uint8))))
        out.append(collate(samples))
    return out


def event_ms(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--sizes', default='416,608')
    ap.add_argument('--batches', type=int, default=24)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--blur', default='5 5', help='[augmentation] random_blur: the largest width and height')
    args = ap.parse_args()
    import torch

    import _hip
    import utils.data
    assert torch.cuda.is_available(), 'jitter_bench.py measures on an MI355X'
    dev = torch.device('cuda', 0)
    B = args.batch
    labels = set(utils.data.LABELS)
    res = dict(batch=B, batches=args.batches, image_train=IMAGE_TRAIN, random_blur=args.blur, device=torch.cuda.get_device_name(0), lib=os.path.basename(_hip.LIB_PATH))
    for S in (int(v) for v in args.sizes.split(',')):
        packed = make_batches(B, S, S, args.blur)
        pinned = [{k: (v.pin_memory() if torch.is_tensor(v) else v) for k, v in b.items() if k not in labels} for b in packed]
        finished = [utils.data.to_device(b, 'cpu')['tensor'].pin_memory() for b in pinned]          # what the reference's workers hand over
        on_dev = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()} for b in pinned]
        outs = [torch.empty(B, 3, S, S, dtype=torch.float32, device=dev) for _ in range(ROTATE)]
        utils.data.to_device(pinned[0], dev, out=outs[0])
        assert torch.equal(outs[0].cpu(), finished[0]), 'device and host differ'
        level = utils.data.level_table(packed[0]['normalize'], dev)
        shared = level.view(1, 3, 256).repeat(B, 1, 1).contiguous()
        L, st = _hip.lib(), _hip.stream()
        flags = 1 if packed[0]['swap_rb'] else 0
        keep, forms = [], dict(full=[], blur=[], hsv=[], plain=[], collate=[])
        for d, o in zip(on_dev, outs):
            blur_only, hsv_only, plain = d['jitter'].clone(), d['jitter'].clone(), d['jitter'].clone()
            blur_only[:, 2] = 0
            hsv_only[:, :2] = 1
            plain[:, :2], plain[:, 2] = 1, 0
            keep += [blur_only, hsv_only, plain]
            head, tail = (d['raw'].data_ptr(), d['offset'].data_ptr(), d['geom'].data_ptr()), (B, S, S, flags, o.data_ptr(), st)
            forms['full'].append(head + (d['jitter'].data_ptr(), d['hsv_tab'].data_ptr(), d['lut_b'].data_ptr()) + tail)
            forms['blur'].append(head + (blur_only.data_ptr(), None, shared.data_ptr()) + tail)
            forms['hsv'].append(head + (hsv_only.data_ptr(), d['hsv_tab'].data_ptr(), d['lut_b'].data_ptr()) + tail)
            forms['plain'].append(head + (plain.data_ptr(), None, shared.data_ptr()) + tail)
            forms['collate'].append(head + (level.data_ptr(),) + tail)

        def launches(name):
            fn = L.y2_collate_images if name == 'collate' else L.y2_collate_jitter_images
            for c in forms[name] * 2:
                _hip.check(fn(*c), name)
        window_bytes = statistics.mean(int((d['geom'][:, 5].long() * d['geom'][:, 6].long()).sum()) * 3 for d in pinned)
        out_bytes = B * 3 * S * S * 4
        runs = []
        for _ in range(args.runs):
            a_ms, b_ms, k_ms = [], [], {name: [] for name in forms}
            for i in range(args.warmup + args.batches):
                j = i % ROTATE
                a = event_ms(lambda: outs[j].copy_(finished[j], non_blocking=True))
                b = event_ms(lambda: utils.data.to_device(pinned[j], dev, out=outs[j]))
                if i >= args.warmup:
                    a_ms.append(a)
                    b_ms.append(b)
            for i in range(args.warmup + args.batches):
                for name in forms:
                    ms = event_ms(lambda: launches(name)) / (2 * ROTATE)
                    if i >= args.warmup:
                        k_ms[name].append(ms)
            a, b = statistics.median(a_ms), statistics.median(b_ms)
            mm = lambda v: [round(min(v), 4), round(max(v), 4)]
            run = dict(fp32_h2d_ms=round(a, 4), uint8_jitter_ms=round(b, 4), ratio_a_over_b=round(a / b, 3), fp32_h2d_ms_min_max=mm(a_ms), uint8_jitter_ms_min_max=mm(b_ms))
            for name, v in k_ms.items():
                m = statistics.median(v)
                run.update({name + '_ms': round(m, 4), name + '_gbs': round((window_bytes + out_bytes) / m / 1e6, 1), name + '_ms_min_max': mm(v)})
            run['full_over_collate'] = round(run['full_ms'] / run['collate_ms'], 2)
            runs.append(run)
        res['size%d' % S] = dict(runs=runs, fp32_mbytes=round(out_bytes / 1e6, 2), uint8_mbytes=round(statistics.mean(d['raw'].numel() for d in pinned) / 1e6, 2),
                                 window_mbytes=round(window_bytes / 1e6, 2), blur_sizes=sorted({tuple(r) for d in packed for r in d['jitter'][:, :2].tolist()}))
        del pinned, finished, on_dev, outs, keep, forms
    print(json.dumps(res))


if __name__ == '__main__':
    main()
