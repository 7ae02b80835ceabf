#!/usr/bin/env python
"""Timing of the MobileNet plugin (model.mobilenet) on one MI355X; prints ONE JSON line:
  detect_ips      images/s of GraphedDetector at 416x416, batch 32 (replays after warm-up)
  train_ips       images/s of train.iterate at 416x416, batch 64, 20 classes (captured steps after warm-up)
  kernels         per kernel family: ms per batch (y2_prof event pairs around every library launch, one detect batch and one eager training
                  step after warm-up); for the dwconv_* kernels also the compulsory bytes (input read once, output written once) and TB/s
  dw_layers       the depthwise forward layers of the detect batch: shape, compulsory MB, ms, TB/s
    python tools/mobilenet_bench.py [--detect-batch 32] [--train-batch 64] [--size 416] [--steps 10]"""
import argparse
import configparser
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'yolo2-pytorch_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def build(dev, num_cls=20):
    import torch

    import bench_data
    import model
    import model.mobilenet
    cfg = configparser.ConfigParser()
    cfg.read_dict({'model': {'dnn': 'model.mobilenet.MobileNet'}})
    anchors = torch.from_numpy(bench_data.ANCHORS_VOC)
    torch.manual_seed(0)
    dnn = model.mobilenet.MobileNet(model.ConfigChannels(cfg), anchors, num_cls)
    bench_data.randomize(dnn, 0, 0.25, gamma=(0.25, 0.5))
    return model.Inference(cfg, dnn, anchors).to(dev), anchors


def prof_records(L):
    out = []
    name = ctypes.create_string_buffer(128)
    ms, fl = ctypes.c_float(), ctypes.c_double()
    for i in range(L.y2_prof_count()):
        L.y2_prof_get(i, name, 128, ctypes.byref(ms), ctypes.byref(fl))
        out.append((name.value.decode(), ms.value, fl.value))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--detect-batch', type=int, default=32)
    ap.add_argument('--train-batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('--steps', type=int, default=10)
    args = ap.parse_args()
    import torch

    import _hip
    import bench_data
    import detect
    import train as y2train
    import utils
    dev = torch.device('cuda', 0)
    L = _hip.lib()
    S = args.size
    res = dict(size=S, detect_batch=args.detect_batch, train_batch=args.train_batch)
    inf, anchors = build(dev)
    net = inf.dnn.eval()
    # ---- detect
    x = bench_data.images(args.detect_batch, S, seed=1).to(dev)
    gd = detect.GraphedDetector(net, anchors, x, warmup=3)
    for _ in range(3):
        gd.run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        gd.run()
    e1.record()
    torch.cuda.synchronize()
    res['detect_ms'] = e0.elapsed_time(e1) / args.steps
    res['detect_ips'] = args.detect_batch * 1000.0 / res['detect_ms']
    # per-kernel table of one eager detect batch
    fam = {}
    dw_layers = []
    L.y2_prof_enable(1)
    with torch.no_grad():
        detect.detect_batch(net.forward_nhwc(x), anchors, fix=True)
    torch.cuda.synchronize()
    recs = prof_records(L)
    L.y2_prof_enable(0)
    plan = net._plans.latest()
    dw_steps = [s for s in plan['steps'] if s[0] == 'dw']
    di = 0
    for name, ms, _ in recs:
        f = fam.setdefault('detect:' + name, dict(ms=0.0, n=0))
        f['ms'] += ms
        f['n'] += 1
        if name == 'dwconv_fwd_kernel':
            _, _, _, _, _, B, h, w, c, _, _, s = dw_steps[di]
            ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
            nbytes = 4.0 * B * c * (h * w + ho * wo)
            f['bytes'] = f.get('bytes', 0.0) + nbytes
            dw_layers.append(dict(B=B, H=h, W=w, C=c, stride=s, mb=nbytes / 1e6, ms=ms, tbps=nbytes / ms / 1e9))
            di += 1
    del gd
    # ---- training
    tinf, tanchors = build(dev)
    tinf.train()
    opt = utils.optim.SGD(tinf.parameters(), 0.0)
    d = {k: v.to(dev) for k, v in bench_data.labels(args.train_batch, S, 20, seed=2).items()}
    d['tensor'] = bench_data.images(args.train_batch, S, seed=11).to(dev)
    for _ in range(6):
        y2train.iterate(tinf, opt, d, bench_data.HPARAM, bench_data.THRESHOLD, tanchors)
    torch.cuda.synchronize()
    t0 = time.time()
    e0.record()
    for _ in range(args.steps):
        y2train.iterate(tinf, opt, d, bench_data.HPARAM, bench_data.THRESHOLD, tanchors)
    e1.record()
    torch.cuda.synchronize()
    res['train_ms'] = e0.elapsed_time(e1) / args.steps
    res['train_wall_ms'] = (time.time() - t0) * 1000.0 / args.steps
    res['train_ips'] = args.train_batch * 1000.0 / res['train_ms']
    runner = tinf.__dict__.get('_y2_step_runner')
    res['train_captured'] = bool(runner is not None and runner.captures >= 1 and not runner.broken)
    # per-kernel table of one eager (autograd path) training step
    y2train.PLAN = False
    try:
        import model
        L.y2_prof_enable(1)
        pred = model._inference(tinf, d['tensor'])
        loss, _ = model.loss(tanchors, {k: d[k] for k in ('yx_min', 'yx_max', 'cls')}, pred, bench_data.THRESHOLD)
        sum(loss[k] * bench_data.HPARAM[k] for k in loss).backward()
        torch.cuda.synchronize()
        recs = prof_records(L)
        L.y2_prof_enable(0)
    finally:
        y2train.PLAN = True
    for name, ms, _ in recs:
        f = fam.setdefault('train:' + name, dict(ms=0.0, n=0))
        f['ms'] += ms
        f['n'] += 1
    for k, f in fam.items():
        if 'bytes' in f:
            f['tbps'] = f['bytes'] / f['ms'] / 1e9
    res['kernels'] = {k: {a: (round(b, 4) if isinstance(b, float) else b) for a, b in v.items()} for k, v in sorted(fam.items(), key=lambda kv: -kv[1]['ms'])}
    res['dw_layers'] = [{a: (round(b, 4) if isinstance(b, float) else b) for a, b in l.items()} for l in dw_layers]
    res['device'] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
