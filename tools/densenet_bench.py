#!/usr/bin/env python
"""Timing of the DenseNet plugin (model.densenet, densenet121) on one MI355X; prints ONE JSON line:
  detect_ips      images/s of GraphedDetector at 416x416, batch 32 (replays after warm-up), with the plan's measured per-layer choices
  detect_ips_fused / detect_ips_two_kernel   the same with every pre-activated 1x1 forced to one form (Y2_DENSE_FUSED=1 / 0)
  layers          one row per distinct pre-activated 1x1 shape of the plan: the fused kernel (y2_preact_conv1x1_fwd) against the SAME layer as
                  the two-kernel form (y2_preact_fwd + 1x1 y2_conv_fwd with its measured tile): event pairs around warm executions, median
                  of `--rounds` (>= 20) pairs, both forms interleaved in one process; spread = (max - min) / median of the fused kernel's
                  pairs; compulsory bytes of the fused form (input slice read once, weights, output written once) -> TB/s; fraction of the
                  157.3 TF/s fp32-MFMA peak; `chosen`: what the plan runs for that shape
  bn_act_two_kernel_ms   unpooled shapes: y2_bn_act_fwd + the same 1x1 y2_conv_fwd, the two kernels that existed before csrc/dense.hip
  train_ips       images/s of train.iterate at 416x416, batch 64, 20 classes (captured steps after warm-up)
    python tools/densenet_bench.py [--detect-batch 32] [--train-batch 64] [--size 416] [--steps 10] [--rounds 21]"""
import argparse
import configparser
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'yolo2-pytorch_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_TF = 157.3


def build(dev, num_cls=20):
    import torch

    import bench_data
    import model
    import model.densenet
    cfg = configparser.ConfigParser()
    cfg.read_dict({'model': {'dnn': 'model.densenet.densenet121', 'pretrained': '0'}})
    anchors = torch.from_numpy(bench_data.ANCHORS_VOC)
    torch.manual_seed(0)
    dnn = model.densenet.densenet121(model.ConfigChannels(cfg), anchors, num_cls)
    bench_data.randomize(dnn, 0, 0.25, gamma=(0.25, 0.5))
    return model.Inference(cfg, dnn, anchors).to(dev), anchors


def detect_ips(net, anchors, x, steps):
    import torch

    import detect
    net._plan_cache = None
    gd = detect.GraphedDetector(net, anchors, x, warmup=3)
    for _ in range(3):
        gd.run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        gd.run()
    e1.record()
    torch.cuda.synchronize()
    return x.shape[0] * 1000.0 * steps / e0.elapsed_time(e1)


def run(net, steps, B):
    import _hip
    st = _hip.stream()
    for step in steps:
        if step[0] == 'bnact':
            _, xin, ps, pb, pslope, act, h, w, K, ldx = step
            _hip.check(_hip.lib().y2_bn_act_fwd(_hip.ptr(xin), _hip.ptr(ps), _hip.ptr(pb), pslope, _hip.ptr(act), None, B, h, w, K, ldx, K, 0, 0, 0, 0, st), 'y2_bn_act_fwd')
        else:
            net._run([step], B, st)


def pairs(net, B, steps, rounds):
    import torch
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(net, steps, B)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--detect-batch', type=int, default=32)
    ap.add_argument('--train-batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=21)
    args = ap.parse_args()
    import torch

    import _hip
    import bench_data
    import model.densenet as densenet
    dev = torch.device('cuda', 0)
    S, B = args.size, args.detect_batch
    res = dict(size=S, detect_batch=B, device=torch.cuda.get_device_name(0))
    inf, anchors = build(dev)
    net = inf.dnn.eval()
    x = bench_data.images(B, S, seed=1).to(dev)
    for name, mode in (('detect_ips', None), ('detect_ips_fused', True), ('detect_ips_two_kernel', False)):
        densenet.FUSED = mode
        res[name] = round(detect_ips(net, anchors, x, args.steps), 1)
    # ---- per-layer table: both forms of every distinct pre-activated 1x1 shape, on the buffers of a fused plan
    densenet.FUSED = True
    net._plan_cache = None
    with torch.no_grad():
        net.forward_nhwc(x)
    torch.cuda.synchronize()
    plan = net._plans.latest()
    rows, seen = [], set()
    for step in plan['steps']:
        if step[0] != 'pre':
            continue
        _, xin, wt, ps, pb, pslope, scale, shift, slope, y, h, w, K, ldx, N, ldy, coff, pool = step
        shape = (h, w, K, ldx, N, pool)
        if shape in seen:
            continue
        seen.add(shape)
        ho, wo = (h // 2, w // 2) if pool else (h, w)
        act = torch.empty(B, ho, wo, K, device=dev)
        p = _hip.ConvParams()
        p.x, p.w, p.y = act.data_ptr(), wt.data_ptr(), y.data_ptr()
        p.scale = scale.data_ptr() if scale is not None else None
        p.shift = shift.data_ptr() if shift is not None else None
        p.B, p.H, p.W, p.Cin, p.ldx, p.Cout, p.ksize, p.ldy, p.coff, p.slope, p.stride, p.pad_plus1 = B, ho, wo, K, K, N, 1, ldy, coff, slope, 1, 1
        _hip.autotune_conv(p, dev)
        _hip.conv_workspace(p, dev)
        two = [('act', xin, ps, pb, pslope, act, h, w, K, ldx, pool), ('conv', p)]
        # the two kernels as they existed before csrc/dense.hip: y2_bn_act_fwd (no pooled form: unpooled shapes only) + the same 1x1 y2_conv_fwd
        parent = None if pool else [('bnact', xin, ps, pb, pslope, act, h, w, K, ldx), ('conv', p)]
        for steps in ([step], two) + ((parent,) if parent else ()):          # warm
            run(net, steps, B)
        tf, tt, tp = [], [], []
        for _ in range(3):                   # interleaved rounds
            tf += pairs(net, B, [step], args.rounds // 3 + 1)
            tt += pairs(net, B, two, args.rounds // 3 + 1)
            if parent:
                tp += pairs(net, B, parent, args.rounds // 3 + 1)
        tf.sort()
        tt.sort()
        tp.sort()
        mf, mt = tf[len(tf) // 2], tt[len(tt) // 2]
        nbytes = 4.0 * (B * h * w * K + N * K + B * ho * wo * N)
        flops = 2.0 * B * ho * wo * N * K
        chosen = _hip._TUNE.get(('preact', B, h, w, K, ldx, N, pool, str(dev)))
        rows.append(dict(H=h, W=w, K=K, ldx=ldx, N=N, pool=pool, fused_ms=round(mf, 4), two_kernel_ms=round(mt, 4),
                         bn_act_two_kernel_ms=round(tp[len(tp) // 2], 4) if tp else None, conv_tile=[p.algo, p.tile],
                         spread=round((tf[-1] - tf[0]) / mf, 3), tbps=round(nbytes / mf / 1e9, 3), mfma_frac=round(flops / mf / 1e9 / PEAK_TF, 3),
                         chosen=None if chosen is None else ('fused' if chosen else 'two_kernel')))
    res['layers'] = rows
    # ---- training: captured train.iterate steps after warm-up
    import train as y2train
    import utils
    del net, inf
    torch.cuda.empty_cache()
    densenet.FUSED = None
    tinf, tanchors = build(dev)
    tinf.train()
    opt = utils.optim.SGD(tinf.parameters(), 0.0)
    TB = args.train_batch
    d = {k: v.to(dev) for k, v in bench_data.labels(TB, S, 20, seed=2).items()}
    d['tensor'] = bench_data.images(TB, S, seed=11).to(dev)
    for _ in range(6):
        y2train.iterate(tinf, opt, d, bench_data.HPARAM, bench_data.THRESHOLD, tanchors)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        y2train.iterate(tinf, opt, d, bench_data.HPARAM, bench_data.THRESHOLD, tanchors)
    e1.record()
    torch.cuda.synchronize()
    res['train_batch'] = TB
    res['train_ms'] = round(e0.elapsed_time(e1) / args.steps, 3)
    res['train_ips'] = round(TB * 1000.0 * args.steps / e0.elapsed_time(e1), 1)
    runner = tinf.__dict__.get('_y2_step_runner')
    res['train_captured'] = bool(runner is not None and runner.captures >= 1 and not runner.broken)
    res['fused_wins'] = sum(1 for r in rows if r['fused_ms'] <= r['two_kernel_ms'])
    res['shapes'] = len(rows)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
