#!/usr/bin/env python
"""Timing of the evaluation's matching stage on one MI355X; prints ONE JSON line.

Workload: seeded Darknet-19 (bench_data), VOC-20, batch 32 at 416x416, 8 synthetic label slots per image (bench_data.labels), `[detect] fix` 0
and 1 with threshold_cls 0.005.  The detections of one batch are computed once; per `fix` two paths turn them into true-positive flags:
  per_class   postprocess_batch, then per image the valid-label filter and per predicted class eval.matching (one y2_iou_rowmax launch, two
              blocking copies, a host claim loop): the loop of eval.py:278-292 as it could be written before eval.match_batch existed
  batched     detect.expand_batch + eval.Accumulator.update (y2_expand_classes + y2_eval_match, no synchronisation)
Reported per path: the median over the timed batches of the HIP-event time and of the wall-clock time (the per-class path is host-bound: its
wall time is the honest figure; the batched path's wall time includes one synchronisation per batch that a real loop would not pay), the
number of eval.matching calls per batch, and detect_ms: the detector's own time per batch (GraphedDetector replays).
    python tools/eval_bench.py [--batch 32] [--size 416] [--batches 20] [--warmup 3]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'yolo2-pytorch_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

IOU, THRESHOLD_CLS = 0.5, 0.005


def timed(fn, batches, warmup):
    """Median (event ms, wall ms) of fn() over `batches` runs after `warmup`; each run ends with a synchronisation."""
    import torch
    ev_ms, wall_ms = [], []
    for i in range(warmup + batches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            wall_ms.append((time.perf_counter() - t0) * 1000.0)
            ev_ms.append(e0.elapsed_time(e1))
    return statistics.median(ev_ms), statistics.median(wall_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('--batches', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    import torch

    import bench_data
    import detect
    ev = importlib.import_module('eval')
    dev = torch.device('cuda', 0)
    B, S, C = args.batch, args.size, 20
    inf, anchors = bench_data.build_model(C, dev)
    net = inf.dnn
    x = bench_data.images(B, S, seed=1).to(dev)
    data = {k: v.to(dev) for k, v in bench_data.labels(B, S, C, nmax=8, seed=2).items()}
    data['difficult'] = torch.zeros(data['cls'].shape, dtype=torch.uint8, device=dev)
    res = dict(batch=B, size=S, batches=args.batches, labels_per_image=data['cls'].size(1), device=torch.cuda.get_device_name(0))
    for fix in (0, 1):
        gd = detect.GraphedDetector(net, anchors, x, fix=bool(fix), threshold_cls=THRESHOLD_CLS, warmup=3)
        for _ in range(3):
            gd.run()
        res['detect_ms_fix%d' % fix] = timed(gd.run, args.batches, args.warmup)[0]
        d = gd.run()
        torch.cuda.synchronize()
        rows = cols = S // 32          # Darknet-19: the head's grid
        hw = torch.tensor([float(S), float(S)], device=dev).view(1, 2)
        grid = torch.tensor([float(rows), float(cols)], device=dev).view(1, 2)
        calls = [0]

        def per_class():
            calls[0] = 0
            flags = []
            out = detect.postprocess_batch(d, fix=bool(fix), threshold_cls=THRESHOLD_CLS)
            for b in range(B):
                g_min, g_max = data['yx_min'][b] / hw, data['yx_max'][b] / hw
                valid = (g_min < g_max).all(-1) & (data['difficult'][b] < 1)
                g_min, g_max, g_cls = g_min[valid], g_max[valid], data['cls'][b][valid]
                if out[b] is None:
                    continue
                _, yx_min, yx_max, cls, score = out[b]
                yx_min, yx_max = yx_min / grid, yx_max / grid
                for c in set(cls.cpu().numpy()):
                    c = int(c)
                    sel = cls == c
                    flags.append(ev.matching(g_min[g_cls == c], g_max[g_cls == c], yx_min[sel], yx_max[sel], IOU))
                    calls[0] += 1
            return flags

        acc = ev.Accumulator(num_cls=C, iou=IOU, max_bytes=1 << 40)

        def batched():
            acc._padded, acc._bytes = [], 0         # (timing the same batch over and over: keep nothing)
            return acc.update(data, detect.expand_batch(d, fix=bool(fix), threshold_cls=THRESHOLD_CLS), image_size=(S, S), grid=(rows, cols))

        # both paths flag the same detections
        tp = batched().cpu().numpy()
        n_a = sum(int(f.sum()) for f in per_class())
        assert int(tp.sum()) == n_a, (int(tp.sum()), n_a)
        a_ev, a_wall = timed(per_class, args.batches, args.warmup)
        b_ev, b_wall = timed(batched, args.batches, args.warmup)
        res['fix%d' % fix] = dict(per_class_event_ms=round(a_ev, 4), per_class_wall_ms=round(a_wall, 4), matching_calls=calls[0],
                                  batched_event_ms=round(b_ev, 4), batched_wall_ms=round(b_wall, 4), true_positives=n_a,
                                  detections=int(detect.expand_batch(d, fix=bool(fix), threshold_cls=THRESHOLD_CLS)['count'].sum()),
                                  wall_ratio=round(a_wall / b_wall, 2), batched_over_detect=round(b_wall / res['detect_ms_fix%d' % fix], 4),
                                  per_class_over_detect=round(a_wall / res['detect_ms_fix%d' % fix], 2))
        res['detect_ms_fix%d' % fix] = round(res['detect_ms_fix%d' % fix], 4)
        del gd
    print(json.dumps(res))


if __name__ == '__main__':
    main()
