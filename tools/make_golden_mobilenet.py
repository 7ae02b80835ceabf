"""Generate tests/golden/mobilenet.npz from the REFERENCE model/mobilenet.py (only where the reference checkout exists).

    python tools/make_golden_mobilenet.py

The reference file is loaded by path next to the reference's own `model` package (oracle.refload).  The network is built at the
default widths divided by 8 (a pruned checkpoint through ConfigChannels: every width a multiple of 4) from a seeded state_dict
(kaiming-scaled convolutions, randomised BatchNorm affine / running statistics and head bias: the synthetic-input convention of
oracle/resnet.init_state_dict).  Stored, arrays and names only:
  keys / shapes            state_dict key order and shapes of the narrow model; full_keys / full_shapes: the same at default widths
  sd/<key>                 the narrow state_dict (fp32)
  x64x96 [1,3,64,96]       an input; the other, x96 [2,3,96,96], is oracle.synth.images(2, 96, seed=1) (x96_head: its first 64 values)
  eval_<x>_fp64 / _fp32    eval-mode outputs of the reference in fp64 and in fp32
  train_R                  seeded weights R of the training objective sum(out * R) on x96
  train_out_fp64 / _fp32   training-mode output
  grad/<param>             fp64 gradient (stored as fp32) of sum(out * R) for every parameter; gfloor/<param>: max|fp32 - fp64| / rms(fp64) of the
                           reference's own fp32 gradient
  run/<buffer>             fp64 (stored as fp32) running_mean / running_var after the step (rfloor/<buffer>: the fp32 run's error alike)
"""
import collections
import configparser
import copy
import importlib.util
import logging
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refload, synth  # noqa: E402

WIDTH_DIV = 8
NUM_CLS = 20
OUT = os.path.join(ROOT, 'tests', 'golden', 'mobilenet.npz')


def load_reference_mobilenet(ns):
    sys.modules['model'] = ns.model
    try:
        spec = importlib.util.spec_from_file_location('_ref_mobilenet', os.path.join(refload.REF, 'model/mobilenet.py'))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        sys.modules.pop('model', None)
    return m


def synthetic_state_dict(template, seed=0):
    """Seeded values for every entry of `template` (a state_dict): conv weights ~ N(0, 2/fan_in), BN gamma U(0.25, 0.75), beta
    N(0, 0.1), running mean N(0, 0.1), running var U(0.5, 1.5), head weight scaled by 1/4, head bias N(0, 0.1)."""
    g = torch.Generator().manual_seed(seed)
    sd = collections.OrderedDict()
    for k, v in template.items():
        if k.endswith('num_batches_tracked'):
            sd[k] = torch.zeros_like(v)
        elif k.endswith('running_mean') or (k.endswith('.bias') and v.dim() == 1 and 'bn' in k):
            sd[k] = torch.randn(v.shape, generator=g) * 0.1
        elif k.endswith('running_var'):
            sd[k] = torch.rand(v.shape, generator=g) + 0.5
        elif v.dim() == 1 and k.endswith('.weight'):
            sd[k] = torch.rand(v.shape, generator=g) * 0.5 + 0.25
        elif v.dim() == 4:
            fan_in = v.shape[1] * v.shape[2] * v.shape[3]
            sd[k] = torch.randn(v.shape, generator=g) * math.sqrt(2.0 / fan_in)
        else:                                   # head bias
            sd[k] = torch.randn(v.shape, generator=g) * 0.1
    head = [k for k in sd if sd[k].dim() == 4][-1]
    sd[head] = sd[head] * 0.25
    return sd


def rel(a, ref):
    ref = ref.double()
    return float((a.double() - ref).abs().max() / ref.pow(2).mean().sqrt().clamp_min(1e-30))


def main():
    logging.disable(logging.WARNING)
    ns = refload.load()
    m = load_reference_mobilenet(ns)
    cfg = configparser.ConfigParser()
    cfg.read(os.path.join(refload.REF, 'config.ini'))
    anchors = torch.from_numpy(synth.ANCHORS_VOC)
    torch.manual_seed(0)
    full = m.MobileNet(ns.model.ConfigChannels(cfg), anchors, NUM_CLS)
    fsd = full.state_dict()
    # narrow widths: the default widths / 8, named the way ConfigChannels reads them
    narrow = collections.OrderedDict((k, torch.zeros(v.shape[0] // WIDTH_DIV, *v.shape[1:]) if (k.endswith('conv.weight') and '.dw.' not in k) else v)
                                     for k, v in fsd.items())
    net = m.MobileNet(ns.model.ConfigChannels(cfg, narrow), anchors, NUM_CLS)
    sd = synthetic_state_dict(net.state_dict(), seed=0)
    net.load_state_dict(sd)
    out = collections.OrderedDict()
    out['keys'] = np.array(list(sd.keys()))
    out['shapes'] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], np.int64)
    out['full_keys'] = np.array(list(fsd.keys()))
    out['full_shapes'] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in fsd.values()], np.int64)
    for k, v in sd.items():
        out['sd/' + k] = v.numpy()
    inputs = dict(x96=synth.images(2, 96, seed=1), x64x96=torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(3)))
    nets = {}
    for dt, name in ((torch.float64, 'fp64'), (torch.float32, 'fp32')):
        n = copy.deepcopy(net).to(dt)
        n.eval()
        nets[name] = n
        with torch.no_grad():
            for xn, x in inputs.items():
                out['eval_%s_%s' % (xn, name)] = n(x.to(dt)).numpy()
    out['x64x96'] = inputs['x64x96'].numpy()
    out['x96_head'] = inputs['x96'].reshape(-1)[:64].numpy()      # x96 itself is oracle.synth.images(2, 96, seed=1): its first values pin it
    # one training step on x96: objective sum(out * R)
    x = inputs['x96']
    R = torch.randn(2, 125, 3, 3, generator=torch.Generator().manual_seed(5))
    out['train_R'] = R.numpy()
    res = {}
    for dt, name in ((torch.float64, 'fp64'), (torch.float32, 'fp32')):
        n = copy.deepcopy(net).to(dt)
        n.train()
        y = n(x.to(dt))
        (y * R.to(dt)).sum().backward()
        res[name] = (y.detach(), {k: p.grad.detach() for k, p in n.named_parameters()},
                     {k: b.detach() for k, b in n.named_buffers() if not k.endswith('num_batches_tracked')})
        out['train_out_' + name] = y.detach().numpy()
    y64, g64, b64 = res['fp64']
    _, g32, b32 = res['fp32']
    for k in g64:
        out['grad/' + k] = g64[k].float().numpy()          # (fp32 storage of the fp64 result: 6e-8 relative, far below every bound)
        out['gfloor/' + k] = np.float64(rel(g32[k], g64[k]))
    for k in b64:
        out['run/' + k] = b64[k].float().numpy()
        out['rfloor/' + k] = np.float64(rel(b32[k], b64[k]))
    out['train_floor'] = np.float64(rel(res['fp32'][0], y64))
    for xn in inputs:
        out['eval_floor_' + xn] = np.float64(rel(torch.from_numpy(out['eval_%s_fp32' % xn]), torch.from_numpy(out['eval_%s_fp64' % xn])))
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d bytes, %d keys, %d elements at default width)' % (OUT, os.path.getsize(OUT), len(fsd), sum(v.numel() for v in fsd.values())))


if __name__ == '__main__':
    main()
