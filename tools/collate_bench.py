#!/usr/bin/env python
"""Timing of the collate step on one MI355X; prints ONE JSON line.

Workload: batches of 64 seeded source images of VOC-like sizes (long side 500, short side 333-400, landscape and portrait), each with one label
box, through transform.augmentation.RandomFlipHorizontally, transform.resize.label.RandomCrop and utils.data.Collate, at 416x416 and 608x608.
Per size, on the same data in the same process, the medians over the timed batches of the HIP-event times of
  (a) fp32_h2d_ms       one copy of the FINISHED fp32 [64,3,H,W] tensor from pinned memory to the device: what the reference's pipeline delivers
  (b) uint8_collate_ms  utils.data.to_device on the pinned packed batch: the copies of raw / offset / geom and the y2_collate_images launch
  (c) kernel_ms         the launch alone (y2_collate_images called directly, tables and pixels already on the device, 8 launches per event
                        pair, the mean per launch); kernel_gbs = (window bytes read + fp32 bytes written) / time
(a) and (b) alternate batch by batch.  Four different batches rotate, so that neither the source pixels nor the output of a launch are still in the
256 MB Infinity Cache from the launch before.  The finished tensor of (a) is the host function's (y2_collate_images_host) and is compared, once,
with the device's: the three paths move the same images.
    python tools/collate_bench.py [--batch 64] [--sizes 416,608] [--batches 24] [--warmup 4]"""
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


def make_batches(B, S, seed):
    import numpy as np

    import transform.augmentation
    import transform.resize.label
    import utils.data
    config = configparser.ConfigParser()
    config.read_dict({'data': {'resize': 'rescale'}, 'augmentation': {'random_flip_horizontally': '0.5', 'random_crop': '1'}})
    flip, crop = transform.augmentation.RandomFlipHorizontally(config), transform.resize.label.RandomCrop(config)
    collate = utils.data.Collate(crop, [(S, S)])
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
    args = ap.parse_args()
    import torch

    import _hip
    import utils.data
    assert torch.cuda.is_available(), 'collate_bench.py measures on an MI355X'
    dev = torch.device('cuda', 0)
    B = args.batch
    res = dict(batch=B, batches=args.batches, device=torch.cuda.get_device_name(0), lib=os.path.basename(_hip.LIB_PATH))
    for S in (int(v) for v in args.sizes.split(',')):
        packed = [{k: b[k] for k in ('raw', 'offset', 'geom', 'size', 'swap_rb', 'normalize')} for b in make_batches(B, S, seed=S)]
        pinned = [{k: (v.pin_memory() if torch.is_tensor(v) else v) for k, v in b.items()} for b in packed]
        finished = [utils.data.to_device(b, 'cpu')['tensor'].pin_memory() for b in packed]          # what the reference's workers hand over
        on_dev = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()} for b in packed]
        outs = [torch.empty(B, 3, S, S, dtype=torch.float32, device=dev) for _ in range(ROTATE)]
        utils.data.to_device(pinned[0], dev, out=outs[0])
        assert torch.equal(outs[0].cpu(), finished[0]), 'device and host collate differ'
        a_ms, b_ms, c_ms = [], [], []
        for i in range(args.warmup + args.batches):
            j = i % ROTATE
            a = event_ms(lambda: outs[j].copy_(finished[j], non_blocking=True))
            b = event_ms(lambda: utils.data.to_device(pinned[j], dev, out=outs[j]))
            if i >= args.warmup:
                a_ms.append(a)
                b_ms.append(b)
        # (c): the library entry point itself, 2 * ROTATE launches per event pair (the rotating batches, twice), so that neither Python between the
        # event and the launch nor the resolution of the events is counted as kernel time
        lut = utils.data.level_table(packed[0]['normalize'], dev)
        L, st = _hip.lib(), _hip.stream()
        calls = [(d['raw'].data_ptr(), d['offset'].data_ptr(), d['geom'].data_ptr(), lut.data_ptr(), B, S, S, 1, o.data_ptr(), st) for d, o in zip(on_dev, outs)] * 2

        def launches():
            for c in calls:
                _hip.check(L.y2_collate_images(*c), 'y2_collate_images')
        for i in range(args.warmup + args.batches):
            c = event_ms(launches) / len(calls)
            if i >= args.warmup:
                c_ms.append(c)
        a, b, c = statistics.median(a_ms), statistics.median(b_ms), statistics.median(c_ms)
        raw_bytes = statistics.mean(p['raw'].numel() for p in packed)
        window_bytes = statistics.mean(int((p['geom'][:, 5].long() * p['geom'][:, 6].long()).sum()) * 3 for p in packed)
        out_bytes = B * 3 * S * S * 4
        res['size%d' % S] = dict(fp32_h2d_ms=round(a, 4), uint8_collate_ms=round(b, 4), kernel_ms=round(c, 4), ratio_a_over_b=round(a / b, 3),
                                 kernel_gbs=round((window_bytes + out_bytes) / c / 1e6, 1), fp32_mbytes=round(out_bytes / 1e6, 2),
                                 uint8_mbytes=round(raw_bytes / 1e6, 2), bytes_ratio=round(out_bytes / raw_bytes, 3),
                                 fp32_h2d_ms_min_max=[round(min(a_ms), 4), round(max(a_ms), 4)], uint8_collate_ms_min_max=[round(min(b_ms), 4), round(max(b_ms), 4)],
                                 kernel_ms_min_max=[round(min(c_ms), 4), round(max(c_ms), 4)])
        del pinned, finished, on_dev, outs
    print(json.dumps(res))


if __name__ == '__main__':
    main()
