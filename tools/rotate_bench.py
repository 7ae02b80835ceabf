#!/usr/bin/env python
"""Timing of the collate step WITH rotation on one MI355X; prints ONE JSON line.

Workload: the batches of tools/collate_bench.py (64 seeded source images of VOC-like sizes, one label box each) through
transform.augmentation.RandomRotate (`random_rotate = -5 5`, the reference's config.ini), RandomFlipHorizontally, transform.resize.label.RandomCrop
and utils.data.Collate, at 416x416 and 608x608.  Per size, on the same data in the same process, the medians over the timed batches of the
HIP-event times of
  (a) fp32_h2d_ms          one copy of the FINISHED fp32 [64,3,H,W] tensor from pinned memory: what the reference ships after rotating on the CPU
  (b) uint8_rotate_ms      utils.data.to_device on the pinned packed batch: the copies of raw and the tables, y2_warp_affine_images, y2_collate_images
      uint8_plain_ms       the same call on the SAME images collated without RandomRotate (one launch): (b) minus this is what rotation adds
  (c) warp_ms              y2_warp_affine_images alone (tables and pixels on the device, 8 launches per event pair, the mean per launch);
                           warp_gbs = (source bytes + rotated bytes written) / time
      collate_ms           y2_collate_images alone on the same rotated batch, the same way: the yardstick for (c)
(a), (b) and the plain form alternate batch by batch.  Four different batches rotate, so that neither the source pixels nor the output of a launch
are still in the 256 MB Infinity Cache from the launch before.  The finished tensor of (a) is the host functions' and is compared, once, with the
device's.
    python tools/rotate_bench.py [--batch 64] [--sizes 416,608] [--batches 24] [--warmup 4] [--angles "-5 5"]"""
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


def make_batches(B, S, seed, angles):
    """ROTATE batches; angles=None: the same images without RandomRotate."""
    import numpy as np

    import transform.augmentation
    import transform.resize.label
    import utils.data
    config = configparser.ConfigParser()
    config.read_dict({'data': {'resize': 'rescale'}, 'augmentation': {'random_flip_horizontally': '0.5', 'random_crop': '1', 'random_rotate': angles or '0 0'}})
    rotate, flip = transform.augmentation.RandomRotate(config), transform.augmentation.RandomFlipHorizontally(config)
    collate = utils.data.Collate(transform.resize.label.RandomCrop(config), [(S, S)])
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
            data = dict(image=rng.randint(0, 256, (h, w, 3)).astype(np.uint8), yx_min=lo.astype(np.float32).reshape(1, 2),
                        yx_max=hi.astype(np.float32).reshape(1, 2), cls=np.zeros(1, np.int64), difficult=np.zeros(1, np.uint8))
            samples.append(flip(rotate(data) if angles else data))
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
    ap.add_argument('--angles', default='-5 5')
    args = ap.parse_args()
    import torch

    import _hip
    import utils.data
    assert torch.cuda.is_available(), 'rotate_bench.py measures on an MI355X'
    dev = torch.device('cuda', 0)
    B = args.batch
    labels = set(utils.data.LABELS)
    res = dict(batch=B, batches=args.batches, angles=args.angles, device=torch.cuda.get_device_name(0), lib=os.path.basename(_hip.LIB_PATH))
    pin = lambda batches: [{k: (v.pin_memory() if torch.is_tensor(v) else v) for k, v in b.items() if k not in labels} for b in batches]
    for S in (int(v) for v in args.sizes.split(',')):
        packed = make_batches(B, S, S, args.angles)
        pinned, plain = pin(packed), pin(make_batches(B, S, S, None))
        assert all('warp' in b for b in pinned) and not any('warp' in b for b in plain)
        finished = [utils.data.to_device(b, 'cpu')['tensor'].pin_memory() for b in pinned]          # what the reference's workers hand over
        on_dev = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()} for b in pinned]
        outs = [torch.empty(B, 3, S, S, dtype=torch.float32, device=dev) for _ in range(ROTATE)]
        rots = [torch.empty(b['rot_bytes'], dtype=torch.uint8, device=dev) for b in pinned]
        utils.data.to_device(pinned[0], dev, out=outs[0], rot=rots[0])
        assert torch.equal(outs[0].cpu(), finished[0]), 'device and host differ'
        a_ms, b_ms, p_ms, c_ms, k_ms = [], [], [], [], []
        for i in range(args.warmup + args.batches):
            j = i % ROTATE
            a = event_ms(lambda: outs[j].copy_(finished[j], non_blocking=True))
            b = event_ms(lambda: utils.data.to_device(pinned[j], dev, out=outs[j], rot=rots[j]))
            p = event_ms(lambda: utils.data.to_device(plain[j], dev, out=outs[j]))
            if i >= args.warmup:
                a_ms.append(a)
                b_ms.append(b)
                p_ms.append(p)
        # (c): the two library entry points themselves, 2 * ROTATE launches per event pair (the rotating batches, twice)
        lut = utils.data.level_table(packed[0]['normalize'], dev)
        L, st = _hip.lib(), _hip.stream()
        warps = [(d['raw'].data_ptr(), d['src_offset'].data_ptr(), d['src_geom'].data_ptr(), d['warp'].data_ptr(), r.data_ptr(), d['offset'].data_ptr(),
                  d['geom'].data_ptr(), B) + tuple(d['rot_size']) + (0, st) for d, r in zip(on_dev, rots)] * 2
        collates = [(r.data_ptr(), d['offset'].data_ptr(), d['geom'].data_ptr(), lut.data_ptr(), B, S, S, 1, o.data_ptr(), st) for d, r, o in zip(on_dev, rots, outs)] * 2

        def warp_launches():
            for c in warps:
                _hip.check(L.y2_warp_affine_images(*c), 'y2_warp_affine_images')

        def collate_launches():
            for c in collates:
                _hip.check(L.y2_collate_images(*c), 'y2_collate_images')
        for i in range(args.warmup + args.batches):
            c, k = event_ms(warp_launches) / len(warps), event_ms(collate_launches) / len(collates)
            if i >= args.warmup:
                c_ms.append(c)
                k_ms.append(k)
        a, b, p, c, k = (statistics.median(v) for v in (a_ms, b_ms, p_ms, c_ms, k_ms))
        src_bytes = statistics.mean(d['raw'].numel() for d in pinned)
        rot_bytes = statistics.mean(int((d['geom'][:, 1].long() * d['geom'][:, 2].long()).sum()) * 3 for d in pinned)
        window_bytes = statistics.mean(int((d['geom'][:, 5].long() * d['geom'][:, 6].long()).sum()) * 3 for d in pinned)
        out_bytes = B * 3 * S * S * 4
        mm = lambda v: [round(min(v), 4), round(max(v), 4)]
        res['size%d' % S] = dict(fp32_h2d_ms=round(a, 4), uint8_rotate_ms=round(b, 4), uint8_plain_ms=round(p, 4), rotation_adds_ms=round(b - p, 4),
                                 ratio_a_over_b=round(a / b, 3), warp_ms=round(c, 4), warp_gbs=round((src_bytes + rot_bytes) / c / 1e6, 1),
                                 collate_ms=round(k, 4), collate_gbs=round((window_bytes + out_bytes) / k / 1e6, 1),
                                 fp32_mbytes=round(out_bytes / 1e6, 2), uint8_mbytes=round(src_bytes / 1e6, 2), rotated_mbytes=round(rot_bytes / 1e6, 2),
                                 fp32_h2d_ms_min_max=mm(a_ms), uint8_rotate_ms_min_max=mm(b_ms), uint8_plain_ms_min_max=mm(p_ms),
                                 warp_ms_min_max=mm(c_ms), collate_ms_min_max=mm(k_ms))
        del pinned, plain, finished, on_dev, outs, rots
    print(json.dumps(res))


if __name__ == '__main__':
    main()
