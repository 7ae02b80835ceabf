"""The inference plans of the five backbone families through what they share (model/_infer_parts.py): a plan serves a revisited input size
without building anything, and after an in-place parameter update the next forward computes exactly what a freshly constructed network with the
same state_dict computes - Darknet, the ResNets and MobileNet by moving the operand pointers of the plan they have, DenseNet by planning again,
Tiny without a plan."""
import configparser

import numpy as np
import pytest
import torch

from oracle import darknet as odark
from oracle import resnet as ores
from oracle import synth
from oracle.make_golden import NARROW as DARKNET_NARROW
from test_densenet_cpu import NARROW as DENSENET_NARROW, unpack

pytestmark = pytest.mark.gpu

FAMILIES = ['darknet', 'tiny', 'resnet18', 'mobilenet', 'densenet']
REBINDS = ('darknet', 'resnet18', 'mobilenet')          # keep the plan and move its operand pointers on a new parameter version


def make(family, golden, sd=None):
    """One narrow network of `family` (the widths its own test file builds) in eval mode on the GPU; sd: the state_dict to load instead."""
    import model
    import model.densenet
    import model.mobilenet
    import model.resnet
    import model.yolo2
    cfg = configparser.ConfigParser()
    cfg.read_dict({'batch_norm': {'enable': '1'}, 'model': {'pretrained': '0'}})
    anchors = torch.from_numpy(synth.ANCHORS_VOC)
    if family == 'darknet':
        own = odark.init_state_dict(5, 20, seed=0, channels=DARKNET_NARROW, head_scale=1 / 8.0)
        net = model.yolo2.Darknet(model.ConfigChannels(cfg, own), anchors, 20)
    elif family == 'tiny':
        own = odark.init_tiny_state_dict(5, 20, seed=0, div=8, head_scale=0.25)
        net = model.yolo2.Tiny(model.ConfigChannels(cfg, own), anchors, 20)
    elif family == 'resnet18':
        own = ores.init_state_dict(family, 5, 20, seed=0, width=8, head_scale=0.25)
        net = model.resnet.resnet18(model.ConfigChannels(cfg, own), anchors, 20)
    elif family == 'mobilenet':
        g = golden('mobilenet')
        own = {k: torch.from_numpy(g['sd/' + k]) for k in g['keys']}
        net = model.mobilenet.MobileNet(model.ConfigChannels(cfg, own), anchors, 20)
    else:
        own = {k: torch.from_numpy(np.array(v)) for k, v in unpack(golden('densenet'), 'sd').items()}
        net = model.densenet.DenseNet(model.ConfigChannels(cfg), anchors, 20, **DENSENET_NARROW)
    net.load_state_dict(own if sd is None else sd, strict=False)
    return net.to(torch.device('cuda', 0)).eval()


@pytest.mark.parametrize('family', FAMILIES)
def test_plan_serves_a_revisit_and_a_new_parameter_version(family, golden, monkeypatch):
    import _hip
    monkeypatch.setattr(_hip, 'AUTOTUNE', False)         # the static algorithm choice, in this network and in the fresh one
    net = make(family, golden)
    xs = {S: synth.images(2, S, seed=S).to(torch.device('cuda', 0)) for S in (64, 96)}
    with torch.no_grad():
        first = net(xs[64]).clone()
        net(xs[96])
        misses, plan = net._plans.misses, net._plans.d.get(next(iter(net._plans.d), None))
        assert torch.equal(net(xs[64]), first)
        assert net._plans.misses == misses
        for p in net.parameters():
            p.mul_(1.01)
        for name, b in net.named_buffers():
            if name.endswith('running_var'):
                b.mul_(1.1)
        got = net(xs[64]).clone()
        fresh = make(family, golden, sd={k: v.clone() for k, v in net.state_dict().items()})
        want = fresh(xs[64])
    assert not torch.equal(got, first)
    assert torch.equal(got, want)
    if family in REBINDS:
        assert plan is not None and plan['key'][3:5] == (64, 64)
        assert net._plans.misses == misses and net._plans.latest() is plan
