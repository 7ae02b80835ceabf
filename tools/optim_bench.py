#!/usr/bin/env python
"""Time of one optimizer step() on Darknet-19's parameter tensors (VOC-20 head: 50.66 M fp32 elements) on one MI355X; prints ONE JSON line.

Compared on the same tensors and gradients, in the same process, alternating:
  fused_rmsprop     utils.optim.RMSprop (y2_opt_rmsprop: one launch per 48 tensors)
  torch_foreach     torch.optim.RMSprop(foreach=True)  - what `lambda params, lr: torch.optim.RMSprop(...)` of the ini picks on a GPU
  torch_loop        torch.optim.RMSprop(foreach=False) - the per-tensor loop
  fused_adam        utils.optim.Adam, as a yardstick
Per optimizer: the median over the timed steps of the HIP-event time and of the wall-clock time of a step that ends in a synchronisation (the
per-tensor loops are host-bound: for them the wall time is the honest figure), for two runs of the whole comparison (`run1`, `run2`: their
difference is the spread), the bytes the plain update must move - RMSprop 3 reads + 2 writes, Adam 4 reads + 3 writes of 4 bytes per element -
and the resulting GB/s of the event time.  `--momentum` / `--centered` time those forms of RMSprop instead of the plain one.
    python tools/optim_bench.py [--steps 50] [--warmup 5] [--momentum 0.9] [--centered]"""
import argparse
import configparser
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'yolo2-pytorch_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def darknet19_shapes(num_cls=20):
    import torch

    import bench_data
    import model
    import model.yolo2
    cfg = configparser.ConfigParser()
    cfg.read_dict({'batch_norm': {'enable': '1'}, 'model': {'pretrained': '0'}})
    dnn = model.yolo2.Darknet(model.ConfigChannels(cfg), torch.from_numpy(bench_data.ANCHORS_VOC), num_cls)
    return [tuple(p.shape) for p in dnn.parameters()]


def timed(step, steps, warmup):
    """Median (event ms, wall ms) of step() over `steps` calls after `warmup`; every call ends with a synchronisation."""
    import torch
    ev_ms, wall_ms = [], []
    for i in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            wall_ms.append((time.perf_counter() - t0) * 1000.0)
            ev_ms.append(e0.elapsed_time(e1))
    return statistics.median(ev_ms), statistics.median(wall_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--momentum', type=float, default=0.0)
    ap.add_argument('--centered', action='store_true')
    args = ap.parse_args()
    import torch

    import utils
    if not torch.cuda.is_available():
        raise SystemExit('tools/optim_bench.py measures on a GPU: none is visible')
    dev = torch.device('cuda', 0)
    shapes = darknet19_shapes()
    elements = sum(int(torch.Size(s).numel()) for s in shapes)
    g = torch.Generator().manual_seed(0)

    def tensors():
        params = [torch.nn.Parameter((torch.randn(*s, generator=g) * 0.05).to(dev)) for s in shapes]
        for p in params:
            p.grad = (torch.randn(p.shape, generator=g) * 0.01).to(dev)
        return params
    kw = dict(alpha=0.99, eps=1e-8, momentum=args.momentum, centered=args.centered)
    rms_floats = 5 + (2 if args.momentum else 0) + (2 if args.centered else 0)
    make = dict(fused_rmsprop=(lambda p: utils.optim.RMSprop(p, 1e-3, **kw), rms_floats),
                torch_foreach=(lambda p: torch.optim.RMSprop(p, 1e-3, foreach=True, **kw), rms_floats),
                torch_loop=(lambda p: torch.optim.RMSprop(p, 1e-3, foreach=False, **kw), rms_floats),
                fused_adam=(lambda p: utils.optim.Adam(p, 1e-3, betas=(0.9, 0.999), eps=1e-8), 7))
    optimizers = {name: (f(tensors()), floats) for name, (f, floats) in make.items()}
    res = dict(device=torch.cuda.get_device_name(0), tensors=len(shapes), elements=elements, steps=args.steps, momentum=args.momentum, centered=args.centered)
    for run in ('run1', 'run2'):
        out = res[run] = {}
        for name, (opt, floats) in optimizers.items():
            ev, wall = timed(opt.step, args.steps, args.warmup)
            nbytes = 4 * floats * elements
            out[name] = dict(event_ms=round(ev, 4), wall_ms=round(wall, 4), bytes=nbytes, event_gb_s=round(nbytes / ev / 1e6, 1))
        out['foreach_over_fused_event'] = round(out['torch_foreach']['event_ms'] / out['fused_rmsprop']['event_ms'], 2)
        out['foreach_over_fused_wall'] = round(out['torch_foreach']['wall_ms'] / out['fused_rmsprop']['wall_ms'], 2)
        out['loop_over_fused_wall'] = round(out['torch_loop']['wall_ms'] / out['fused_rmsprop']['wall_ms'], 2)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
