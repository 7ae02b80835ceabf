"""Generate tests/golden/densenet.npz from the REFERENCE model/densenet.py (only where the reference checkout exists).

    python tools/make_golden_densenet.py

torchvision is not installed; the reference file takes `_DenseBlock`, `_Transition`, `model_urls` and its base class from
`torchvision.models.densenet` (model/densenet.py:23-24), so a stub module with those four names is injected while the file is loaded by
path next to the reference's own `model` package (the way oracle/make_golden_resnet.py stubs ResNet).  The stub classes below are written
from torchvision's public module structure (Sequential layers `norm1, relu1, conv1, norm2, relu2, conv2` concatenated onto their input;
transitions `norm, relu, conv, pool`).  The narrow network is `growth_rate=16, block_config=(2, 4, 4, 2), num_init_features=32, bn_size=2`
(every width a multiple of 8; blocks with 4 layers: a slab of the concatenation has up to 4 consumers; three transitions) with a seeded
state_dict (tools/make_golden_mobilenet.synthetic_state_dict).  Stored, arrays and names only - the contents of tests/golden/mobilenet.npz:
  keys / shapes            state_dict key order and shapes of the narrow model; full_keys / full_shapes: the same for densenet121
  sd_flat                  the narrow state_dict: its floating-point entries in `keys` order, concatenated (num_batches_tracked are zero)
  x64x96 [1,3,64,96]       an input; the other, x96 [2,3,96,96], is oracle.synth.images(2, 96, seed=1) (x96_head: its first 64 values)
  eval_<x>_fp64 / _fp32    eval-mode outputs of the reference in fp64 and in fp32
  train_R                  seeded weights R of the training objective sum(out * R) on x96
  train_out_fp64 / _fp32   training-mode output
  grad_keys / grad_flat    fp64 gradient (stored as fp32) of sum(out * R) for every parameter, concatenated in grad_keys order (shapes: `shapes`);
                           gfloor[i]: max|fp32 - fp64| / rms(fp64) of the reference's own fp32 gradient of parameter i
  run_keys / run_flat      fp64 (stored as fp32) running_mean / running_var after the step (rfloor[i]: the fp32 run's error alike)
Per-tensor arrays are stored concatenated (one zip member per group instead of ~470: the archive stays below the 1 MiB limit of a committed
file); `unpack(z, group)` gives them back as a dict of name -> array.
"""
import collections
import configparser
import copy
import importlib.util
import logging
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from oracle import refload, synth  # noqa: E402
from make_golden_mobilenet import rel, synthetic_state_dict  # noqa: E402

NARROW = dict(growth_rate=16, block_config=(2, 4, 4, 2), num_init_features=32, bn_size=2)
NUM_CLS = 20
OUT = os.path.join(ROOT, 'tests', 'golden', 'densenet.npz')


class _DenseLayer(nn.Sequential):
    def __init__(self, num_input_features, growth_rate, bn_size, drop_rate):
        nn.Sequential.__init__(self)
        self.add_module('norm1', nn.BatchNorm2d(num_input_features))
        self.add_module('relu1', nn.ReLU(inplace=True))
        self.add_module('conv1', nn.Conv2d(num_input_features, bn_size * growth_rate, kernel_size=1, stride=1, bias=False))
        self.add_module('norm2', nn.BatchNorm2d(bn_size * growth_rate))
        self.add_module('relu2', nn.ReLU(inplace=True))
        self.add_module('conv2', nn.Conv2d(bn_size * growth_rate, growth_rate, kernel_size=3, stride=1, padding=1, bias=False))
        assert drop_rate == 0

    def forward(self, x):
        return torch.cat([x, nn.Sequential.forward(self, x)], 1)


class _DenseBlock(nn.Sequential):
    def __init__(self, num_layers, num_input_features, bn_size, growth_rate, drop_rate):
        nn.Sequential.__init__(self)
        for i in range(num_layers):
            self.add_module('denselayer%d' % (i + 1), _DenseLayer(num_input_features + i * growth_rate, growth_rate, bn_size, drop_rate))


class _Transition(nn.Sequential):
    def __init__(self, num_input_features, num_output_features):
        nn.Sequential.__init__(self)
        self.add_module('norm', nn.BatchNorm2d(num_input_features))
        self.add_module('relu', nn.ReLU(inplace=True))
        self.add_module('conv', nn.Conv2d(num_input_features, num_output_features, kernel_size=1, stride=1, bias=False))
        self.add_module('pool', nn.AvgPool2d(kernel_size=2, stride=2))


def flat(tensors):
    return torch.cat([t.detach().reshape(-1).float() for t in tensors]).numpy()


def load_reference_densenet(ns):
    tv, tvm, tvd = types.ModuleType('torchvision'), types.ModuleType('torchvision.models'), types.ModuleType('torchvision.models.densenet')

    class _D(nn.Module):
        pass
    tvd.DenseNet, tvd._DenseBlock, tvd._Transition, tvd.model_urls = _D, _DenseBlock, _Transition, {}
    tv.models, tvm.densenet = tvm, tvd
    names = {'torchvision': tv, 'torchvision.models': tvm, 'torchvision.models.densenet': tvd, 'model': ns.model}
    sys.modules.update(names)
    if not hasattr(nn.init, 'kaiming_normal'):          # (the reference calls the pre-1.0 name, model/densenet.py:59)
        nn.init.kaiming_normal = nn.init.kaiming_normal_
    try:
        spec = importlib.util.spec_from_file_location('_ref_densenet', os.path.join(refload.REF, 'model/densenet.py'))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        for k in names:
            sys.modules.pop(k, None)
    return m


def unpack(z, group):
    """name -> array of one concatenated group of the fixture: 'sd' (with zero num_batches_tracked), 'grad' or 'run'."""
    shapes = {k: tuple(int(d) for d in s if d) for k, s in zip(z['keys'].tolist(), z['shapes'])}
    if group == 'sd':
        names = [k for k in z['keys'].tolist()]
    else:
        names = z[group + '_keys'].tolist()
    data, out, o = z[group + '_flat'], collections.OrderedDict(), 0
    for k in names:
        if k.endswith('num_batches_tracked'):
            out[k] = np.zeros((), np.int64)
            continue
        n = int(np.prod(shapes[k]))
        out[k] = data[o:o + n].reshape(shapes[k])
        o += n
    assert o == data.size
    return out


def main():
    logging.disable(logging.WARNING)
    import warnings
    warnings.simplefilter('ignore')
    ns = refload.load()
    m = load_reference_densenet(ns)
    cfg = configparser.ConfigParser()
    cfg.read(os.path.join(refload.REF, 'config.ini'))
    cfg.set('model', 'pretrained', '0')
    anchors = torch.from_numpy(synth.ANCHORS_VOC)
    torch.manual_seed(0)
    fsd = m.densenet121(ns.model.ConfigChannels(cfg), anchors, NUM_CLS).state_dict()
    net = m.DenseNet(ns.model.ConfigChannels(cfg), anchors, NUM_CLS, **NARROW)
    sd = synthetic_state_dict(net.state_dict(), seed=0)
    net.load_state_dict(sd)          # (norm*.bias take the rule's last branch: N(0, 0.1), as the BatchNorm biases of the other fixtures)
    out = collections.OrderedDict()
    out['keys'] = np.array(list(sd.keys()))
    out['shapes'] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], np.int64)
    out['full_keys'] = np.array(list(fsd.keys()))
    out['full_shapes'] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in fsd.values()], np.int64)
    out['sd_flat'] = flat(v for v in sd.values() if v.is_floating_point())
    inputs = dict(x96=synth.images(2, 96, seed=1), x64x96=torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(3)))
    for dt, name in ((torch.float64, 'fp64'), (torch.float32, 'fp32')):
        n = copy.deepcopy(net).to(dt)
        n.eval()
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
    out['grad_keys'] = np.array(list(g64))
    out['grad_flat'] = flat(g64.values())          # (fp32 storage of the fp64 result: 6e-8 relative, far below every bound)
    out['gfloor'] = np.array([rel(g32[k], g64[k]) for k in g64], np.float64)
    out['run_keys'] = np.array(list(b64))
    out['run_flat'] = flat(b64.values())
    out['rfloor'] = np.array([rel(b32[k], b64[k]) for k in b64], np.float64)
    out['train_floor'] = np.float64(rel(res['fp32'][0], y64))
    for xn in inputs:
        out['eval_floor_' + xn] = np.float64(rel(torch.from_numpy(out['eval_%s_fp32' % xn]), torch.from_numpy(out['eval_%s_fp64' % xn])))
    np.savez_compressed(OUT, **out)
    gf = sorted(out['gfloor'].tolist())
    print('wrote %s (%d bytes; narrow %d entries / %d elements; densenet121 %d entries / %d elements)' % (
        OUT, os.path.getsize(OUT), len(sd), sum(v.numel() for v in sd.values()), len(fsd), sum(v.numel() for v in fsd.values())))
    print('floors: eval %s, train %.2g, grad median %.2g worst %.2g' % (
        ', '.join('%.2g' % float(out['eval_floor_' + xn]) for xn in inputs), float(out['train_floor']), gf[len(gf) // 2], gf[-1]))


if __name__ == '__main__':
    main()
