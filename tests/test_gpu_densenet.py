"""The DenseNet plugin on the MI355X (model.densenet, reference model/densenet.py:29-117): the pre-activation kernels of csrc/dense.hip
against fp64 torch (F.conv2d(F.relu(x * a + b), w) [avg_pool2d], and the autograd of BatchNorm2d(train) -> ReLU [-> AvgPool2d(2)]), the
plugin's eval output against the reference fixture tests/golden/densenet.npz (tools/make_golden_densenet.py), densenet121 at 416x416
against an fp64 torch.nn twin built here from the plugin's state_dict, one training step against the fixture, a region-loss step against the
oracle's fp64 autograd, frozen-BatchNorm eval with gradients, deterministic mode, the captured step, and GraphedDetector against eager detection.
Error = max |diff| / rms of the fp64 reference (README)."""
import configparser

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import synth
from test_densenet_cpu import NARROW, unpack

import _hip

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda', 0)


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    rms = ref.pow(2).mean().sqrt().item()
    return (got - ref).abs().max().item() / max(rms, 1e-30)


def L():
    return _hip.lib()


def nhwc(t, ld, off=0):
    """[B,C,H,W] -> a device buffer [B,H,W,ld] holding it in channels [off, off + C) (the rest poison)."""
    B, C, H, W = t.shape
    buf = torch.full((B, H, W, ld), float('nan'), dtype=torch.float32, device=dev())
    buf[..., off:off + C] = t.permute(0, 2, 3, 1).to(dev(), torch.float32)
    return buf


def take(buf, C, off=0):
    return buf[..., off:off + C].permute(0, 3, 1, 2).double().cpu()


def misaligned(t):
    """The same values at an address that is 4 (not 16) bytes aligned."""
    raw = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev())
    raw[1:] = t.reshape(-1)
    return raw[1:].view(t.shape)


# ------------------------------------------------------------------------------------------------ kernel (a)
GEMM_CASES = [  # B, H, W, K, ldx, N, ldy, coff
    (2, 16, 16, 64, 64, 128, 128, 0), (2, 14, 10, 96, 256, 128, 132, 4), (1, 26, 26, 512, 512, 128, 128, 0), (2, 8, 12, 1000, 1024, 125, 125, 0),
    (1, 6, 10, 64, 100, 30, 64, 17), (3, 12, 12, 96, 96, 30, 30, 0), (1, 52, 52, 512, 640, 125, 160, 32), (64, 26, 26, 64, 64, 128, 128, 0),
]


def preact_ref(x, a, b, pre_relu):
    t = x.double()
    if a is not None:
        t = t * a.double().view(1, -1, 1, 1) + b.double().view(1, -1, 1, 1)
    return F.relu(t) if pre_relu else t


def run_gemm(xb, w, a, b, pre_slope, scale, shift, slope, yb, stats, B, H, W, K, ldx, N, ldy, coff, pool):
    return L().y2_preact_conv1x1_fwd(_hip.ptr(xb), _hip.ptr(w), _hip.ptr(a), _hip.ptr(b), pre_slope, _hip.ptr(scale), _hip.ptr(shift), slope, _hip.ptr(yb),
                                     _hip.ptr(stats), B, H, W, K, ldx, N, ldy, coff, pool, _hip.stream())


@pytest.mark.parametrize('case', GEMM_CASES)
@pytest.mark.parametrize('pool', [0, 1])
@pytest.mark.parametrize('form', ['relu_affine_relu', 'plain_bias', 'misaligned'])
def test_preact_conv1x1_matches_fp64(case, pool, form):
    B, H, W, K, ldx, N, ldy, coff = case
    g = torch.Generator().manual_seed(B * 1000 + K + H * 7 + W + N + pool)
    x, w = torch.randn(B, K, H, W, generator=g), torch.randn(N, K, 1, 1, generator=g) / K ** 0.5
    a, b = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.5
    scale, shift = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
    pre_relu = form != 'plain_bias'
    if form == 'plain_bias':                      # the head: BatchNorm affine without ReLU in front, bias behind, no activation
        scale, slope = None, 1.0
    else:
        slope = 0.0
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    xb = nhwc(x, ldx)
    yb = torch.full((B, Ho, Wo, ldy), float('nan'), device=dev())
    wd, ad, bd = w.to(dev()).contiguous(), a.to(dev()), b.to(dev())
    if form == 'misaligned':                      # 4-byte aligned operands: the scalar path
        xb, wd, ad = misaligned(xb), misaligned(wd), misaligned(ad)
    sc = scale.to(dev()) if scale is not None else None
    sh = shift.to(dev())
    stats = torch.zeros(_hip.STATS_REPL * 2 * N, dtype=torch.float64, device=dev())
    assert run_gemm(xb, wd, ad, bd, 0.0 if pre_relu else 1.0, sc, sh, slope, yb, stats, B, H, W, K, ldx, N, ldy, coff, pool) == 0
    torch.cuda.synchronize()
    t = preact_ref(x, a, b, pre_relu)
    raw = F.conv2d(t, w.double())
    if pool:
        raw = F.avg_pool2d(raw, 2)                # the reference order: convolution, then the pool
    ref = raw * scale.double().view(1, -1, 1, 1) if scale is not None else raw
    ref = ref + shift.double().view(1, -1, 1, 1)
    ref = F.relu(ref) if slope == 0.0 else ref
    err = rel(take(yb, N, coff), ref)
    print('preact_conv1x1 %s pool=%d %s: %.2e' % (case, pool, form, err))
    assert err <= 2e-5
    mask = torch.ones(ldy, dtype=torch.bool)
    mask[coff:coff + N] = False
    assert torch.isnan(yb[..., mask.to(dev())]).all()           # nothing outside the slice [coff, coff + N) is written
    st = stats.view(_hip.STATS_REPL, 2, N).sum(0).cpu()
    # the channel sum is signed and can cancel: its 1e-6 is taken relative to the sum of magnitudes (rtol on the sum itself would bound nothing
    # meaningful for a sum near zero); the sum of squares below cannot cancel and keeps the pure relative bound
    np.testing.assert_allclose(st[0].numpy(), raw.sum((0, 2, 3)).numpy(), rtol=1e-6, atol=1e-6 * raw.abs().sum().item() / N)
    np.testing.assert_allclose(st[1].numpy(), raw.pow(2).sum((0, 2, 3)).numpy(), rtol=1e-6)


@pytest.mark.parametrize('case', GEMM_CASES[:4] + GEMM_CASES[6:])
@pytest.mark.parametrize('pool', [0, 1])
def test_fused_form_equals_materialised_preactivation_plus_conv(case, pool):
    """(a) against (b) + the 1x1 y2_conv_fwd, and (b) against fp64."""
    import ctypes
    B, H, W, K, ldx, N, ldy, coff = case
    g = torch.Generator().manual_seed(11 + B * 1000 + K + H * 7 + W + N + pool)
    x, w = torch.randn(B, K, H, W, generator=g), torch.randn(N, K, 1, 1, generator=g) / K ** 0.5
    a, b = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.5
    scale, shift = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    xb, wd, ad, bd, sc, sh = nhwc(x, ldx), w.to(dev()).contiguous(), a.to(dev()), b.to(dev()), scale.to(dev()), shift.to(dev())
    y1 = torch.full((B, Ho, Wo, ldy), float('nan'), device=dev())
    assert run_gemm(xb, wd, ad, bd, 0.0, sc, sh, 0.0, y1, None, B, H, W, K, ldx, N, ldy, coff, pool) == 0
    act = torch.full((B, Ho, Wo, K), float('nan'), device=dev())
    assert L().y2_preact_fwd(_hip.ptr(xb), _hip.ptr(ad), _hip.ptr(bd), 0.0, _hip.ptr(act), B, H, W, K, ldx, K, pool, _hip.stream()) == 0
    y2 = torch.full((B, Ho, Wo, ldy), float('nan'), device=dev())
    p = _hip.ConvParams()
    p.x, p.w, p.scale, p.shift, p.y = act.data_ptr(), wd.data_ptr(), sc.data_ptr(), sh.data_ptr(), y2.data_ptr()
    p.B, p.H, p.W, p.Cin, p.ldx, p.Cout, p.ksize, p.ldy, p.coff, p.slope, p.stride, p.pad_plus1 = B, Ho, Wo, K, K, N, 1, ldy, coff, 0.0, 1, 1
    _hip.conv_workspace(p, dev())
    _hip.check(L().y2_conv_fwd(ctypes.byref(p), _hip.stream()), 'y2_conv_fwd')
    torch.cuda.synchronize()
    t = preact_ref(x, a, b, True)
    if pool:
        t = F.avg_pool2d(t, 2)
    assert rel(take(act, K), t) <= 2e-5
    assert rel(take(y1, N, coff), take(y2, N, coff)) <= 2e-5


def test_preact_conv1x1_refuses_statistics_in_deterministic_mode():
    x = torch.zeros(1, 4, 4, 64, device=dev())
    w = torch.zeros(128, 64, device=dev())
    y = torch.zeros(1, 4, 4, 128, device=dev())
    stats = torch.zeros(_hip.STATS_REPL * 2 * 128, dtype=torch.float64, device=dev())
    _hip.set_deterministic(True, dev())
    try:
        assert run_gemm(x, w, None, None, 0.0, None, None, 1.0, y, stats, 1, 4, 4, 64, 64, 128, 128, 0, 0) == -3
        assert run_gemm(x, w, None, None, 0.0, None, None, 1.0, y, None, 1, 4, 4, 64, 64, 128, 128, 0, 0) == 0
    finally:
        _hip.set_deterministic(False)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ kernels (b), (c)
BWD_CASES = [  # B, C, H, W, ldx, off (channel offset of the slice in the block buffer), lddx
    (2, 64, 12, 12, 96, 0, 96), (2, 32, 8, 6, 160, 64, 160), (1, 256, 26, 26, 256, 0, 256), (4, 16, 14, 10, 48, 16, 64), (2, 6, 8, 8, 11, 3, 9),
    (2, 1000, 4, 6, 1024, 0, 1024),
]


def run_bwd(xb, off, a, b, mean, invstd, gamma, dab, ldda, sums, dxb, dxoff, lddx, acc, B, H, W, C, ldx, pool, has_bn):
    xs = xb.view(-1)[off:]
    ds = dxb.view(-1)[dxoff:]
    return L().y2_preact_bwd(_hip.ptr(xs), _hip.ptr(a), _hip.ptr(b), 0.0, _hip.ptr(mean), _hip.ptr(invstd), _hip.ptr(gamma), _hip.ptr(dab), ldda, _hip.ptr(sums),
                             _hip.ptr(ds), lddx, acc, B, H, W, C, ldx, pool, has_bn, _hip.stream())


@pytest.mark.parametrize('case', BWD_CASES)
@pytest.mark.parametrize('pool', [0, 1])
@pytest.mark.parametrize('has_bn', [1, 2, 0])
def test_preact_bwd_matches_fp64_autograd(case, pool, has_bn):
    B, C, H, W, ldx, off, lddx = case
    g = torch.Generator().manual_seed(3 + B * 1000 + C + H * 7 + W + pool + has_bn)
    x = (torch.randn(B, C, H, W, generator=g) * 1.5 + 0.3).double().requires_grad_()
    gamma = (torch.rand(C, generator=g) + 0.5).double().requires_grad_()
    beta = (torch.randn(C, generator=g) * 0.3).double().requires_grad_()
    rmean, rvar = (torch.randn(C, generator=g) * 0.2).double(), (torch.rand(C, generator=g) + 0.5).double()
    if has_bn == 1:
        mean, var = x.detach().mean((0, 2, 3)), x.detach().var((0, 2, 3), unbiased=False)
        y = F.batch_norm(x, None, None, gamma, beta, True, 0.0, 1e-5)
    elif has_bn == 2:
        mean, var = rmean, rvar
        y = F.batch_norm(x, rmean, rvar, gamma, beta, False, 0.0, 1e-5)
    else:
        mean, var = torch.zeros(C).double(), torch.ones(C).double()
        y = x
    y = F.relu(y)
    if pool:
        y = F.avg_pool2d(y, 2)
    dA = torch.randn(y.shape, generator=g).double()
    y.backward(dA)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    if has_bn:
        a, b = (gamma.detach() * invstd).float().to(dev()), (beta.detach() - mean * gamma.detach() * invstd).float().to(dev())
        md, isd, gd = mean.float().to(dev()), invstd.float().to(dev()), gamma.detach().float().to(dev())
    else:
        a = b = md = isd = gd = None
    xb = nhwc(x.detach(), ldx, off)
    dab = nhwc(dA, C + 4)
    sums = torch.zeros(2 * C, dtype=torch.float64, device=dev())
    dxb = torch.full((B, H, W, lddx), float('nan'), device=dev())
    dxoff = min(off, lddx - C)
    assert run_bwd(xb, off, a, b, md, isd, gd, dab, C + 4, sums, dxb, dxoff, lddx, 0, B, H, W, C, ldx, pool, has_bn) == 0
    torch.cuda.synchronize()
    err = rel(take(dxb, C, dxoff), x.grad)
    s = sums.cpu()
    print('preact_bwd %s pool=%d has_bn=%d: dx %.2e' % (case, pool, has_bn, err))
    assert err <= 8e-5
    mask = torch.ones(lddx, dtype=torch.bool)
    mask[dxoff:dxoff + C] = False
    assert torch.isnan(dxb[..., mask.to(dev())]).all()
    if has_bn:
        assert rel(s[:C], beta.grad) <= 8e-5 and rel(s[C:], gamma.grad) <= 8e-5
    else:
        assert rel(s[:C], x.grad.sum((0, 2, 3))) <= 8e-5
    # accumulate = 1 equals write + add
    base = torch.randn(B, H, W, lddx, generator=g).to(dev())
    acc = base.clone()
    sums2 = torch.zeros_like(sums)
    assert run_bwd(xb, off, a, b, md, isd, gd, dab, C + 4, sums2, acc, dxoff, lddx, 1, B, H, W, C, ldx, pool, has_bn) == 0
    torch.cuda.synchronize()
    want = base[..., dxoff:dxoff + C] + dxb[..., dxoff:dxoff + C]
    assert rel(acc[..., dxoff:dxoff + C], want) <= 1e-6
    assert torch.equal(acc[..., mask.to(dev())], base[..., mask.to(dev())])


@pytest.mark.parametrize('case', BWD_CASES[:4])
def test_preact_bwd_is_bit_reproducible_in_deterministic_mode(case):
    B, C, H, W, ldx, off, lddx = case
    g = torch.Generator().manual_seed(5 + C)
    x, dA = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H // 2, W // 2, generator=g)
    a, b = (torch.rand(C, generator=g) + 0.5).to(dev()), torch.randn(C, generator=g).to(dev())
    md, isd, gd = torch.randn(C, generator=g).to(dev()), (torch.rand(C, generator=g) + 0.5).to(dev()), (torch.rand(C, generator=g) + 0.5).to(dev())
    xb, dab = nhwc(x, ldx, off), nhwc(dA, C)
    _hip.set_deterministic(True, dev())
    try:
        outs = []
        for _ in range(2):
            sums = torch.full((2 * C,), float('nan'), dtype=torch.float64, device=dev())          # written, not accumulated, in this mode
            dxb = torch.zeros(B, H, W, lddx, device=dev())
            assert run_bwd(xb, off, a, b, md, isd, gd, dab, C, sums, dxb, 0, lddx, 0, B, H, W, C, ldx, 1, 1) == 0
            torch.cuda.synchronize()
            outs.append((sums.clone(), dxb.clone()))
    finally:
        _hip.set_deterministic(False)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.isfinite(outs[0][0]).all()


# ------------------------------------------------------------------------------------------------ plugin
def config():
    cfg = configparser.ConfigParser()
    cfg.read_dict({'model': {'dnn': 'model.densenet.densenet121', 'pretrained': '0'}})
    return cfg


def narrow_net(golden):
    import model
    import model.densenet
    g = golden('densenet')
    dnn = model.densenet.DenseNet(model.ConfigChannels(config()), torch.from_numpy(synth.ANCHORS_VOC), 20, **NARROW)
    dnn.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in unpack(g, 'sd').items()}, strict=True)
    return dnn.to(dev()).eval(), g


@pytest.mark.parametrize('xn', ['x96', 'x64x96'])
def test_eval_output_matches_reference_fixture(golden, xn):
    dnn, g = narrow_net(golden)
    x = synth.images(2, 96, seed=1) if xn == 'x96' else torch.from_numpy(g['x64x96'])
    with torch.no_grad():
        out = dnn(x.to(dev()))
    ref = torch.from_numpy(g['eval_%s_fp64' % xn])
    assert out.shape == ref.shape
    err = rel(out, ref)
    print('densenet narrow eval %s: %.2e (reference fp32 floor %.2e)' % (xn, err, float(g['eval_floor_' + xn])))
    assert err <= 2e-5


def test_two_kernel_form_gives_the_same_network_output(golden, monkeypatch):
    import model.densenet
    dnn, g = narrow_net(golden)
    x = synth.images(2, 96, seed=1).to(dev())
    with torch.no_grad():
        monkeypatch.setattr(model.densenet, 'FUSED', True)
        fused = dnn(x).clone()
        assert not any(s[0] == 'act' for s in dnn._plan_cache[1]['steps'])
        monkeypatch.setattr(model.densenet, 'FUSED', False)
        dnn._plan_cache = None
        unfused = dnn(x)
    assert any(s[0] == 'act' for s in dnn._plan_cache[1]['steps'])
    ref = torch.from_numpy(g['eval_x96_fp64'])
    assert rel(unfused, ref) <= 2e-5 and rel(fused, unfused) <= 2e-5


class Twin(nn.Module):
    """fp64 torch.nn twin of the plugin's forward, fed with the plugin's state_dict."""

    def __init__(self, sd, block_config):
        nn.Module.__init__(self)
        self.sd, self.block_config = sd, block_config

    def bn(self, x, name):
        s = self.sd
        return F.batch_norm(x, s[name + '.running_mean'], s[name + '.running_var'], s[name + '.weight'], s[name + '.bias'], False, 0.0, 1e-5)

    def forward(self, x):
        s = self.sd
        x = F.max_pool2d(F.relu(self.bn(F.conv2d(x, s['features.conv0.weight'], stride=2, padding=3), 'features.norm0')), 3, 2, 1)
        for i, n in enumerate(self.block_config):
            for j in range(n):
                p = 'features.denseblock%d.denselayer%d.' % (i + 1, j + 1)
                t = F.conv2d(F.relu(self.bn(x, p + 'norm1')), s[p + 'conv1.weight'])
                t = F.conv2d(F.relu(self.bn(t, p + 'norm2')), s[p + 'conv2.weight'], padding=1)
                x = torch.cat([x, t], 1)
            if i != len(self.block_config) - 1:
                p = 'features.transition%d.' % (i + 1)
                x = F.avg_pool2d(F.conv2d(F.relu(self.bn(x, p + 'norm')), s[p + 'conv.weight']), 2)
        return F.conv2d(self.bn(x, 'features.norm5'), s['features.conv.weight'], s['features.conv.bias'])


def full_net(seed=0):
    import model
    import model.densenet
    torch.manual_seed(seed)
    dnn = model.densenet.densenet121(model.ConfigChannels(config()), torch.from_numpy(synth.ANCHORS_VOC), 20)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in dnn.modules():          # randomised BatchNorm affine / running statistics (the synthetic-input convention of the fixtures)
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 0.5 + 0.75)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.bias.shape, generator=g) + 0.5)
        dnn.features.conv.weight.mul_(0.25)
        dnn.features.conv.bias.copy_(torch.randn(dnn.features.conv.bias.shape, generator=g) * 0.1)
    return dnn


def test_densenet121_at_416_matches_fp64_twin():
    dnn = full_net()
    sd = {k: v.clone() for k, v in dnn.state_dict().items()}
    x = synth.images(2, 416, seed=1)
    with torch.no_grad():
        ref = Twin({k: v.double() for k, v in sd.items()}, dnn.block_config)(x.double())
        floor = rel(Twin(sd, dnn.block_config)(x), ref)
        out = dnn.to(dev()).eval()(x.to(dev()))
    assert out.shape == (2, 125, 13, 13)
    err = rel(out, ref)
    print('densenet121 416x416 B=2: %.2e (the twin\'s own fp32 floor %.2e)' % (err, floor))
    assert err <= max(2e-5, 2.5 * floor)


# ------------------------------------------------------------------------------------------------ training
class _TLayer(nn.Sequential):
    def __init__(self, cin, growth, bn_size):
        nn.Sequential.__init__(self)
        self.add_module('norm1', nn.BatchNorm2d(cin))
        self.add_module('relu1', nn.ReLU())
        self.add_module('conv1', nn.Conv2d(cin, bn_size * growth, 1, bias=False))
        self.add_module('norm2', nn.BatchNorm2d(bn_size * growth))
        self.add_module('relu2', nn.ReLU())
        self.add_module('conv2', nn.Conv2d(bn_size * growth, growth, 3, padding=1, bias=False))

    def forward(self, x):
        return torch.cat([x, nn.Sequential.forward(self, x)], 1)


def twin_module(net):
    """torch.nn twin (fp64) of a plugin instance with the same module tree, so parameters and buffers line up by name."""
    f = nn.Sequential()
    c0 = net.features.conv0.out_channels
    f.add_module('conv0', nn.Conv2d(3, c0, 7, 2, 3, bias=False))
    f.add_module('norm0', nn.BatchNorm2d(c0))
    f.add_module('relu0', nn.ReLU())
    f.add_module('pool0', nn.MaxPool2d(3, 2, 1))
    for i, (block, trans) in enumerate(net.blocks()):
        b = nn.Sequential()
        for j, layer in enumerate(block):
            b.add_module('denselayer%d' % (j + 1), _TLayer(layer.conv1.in_channels, layer.conv2.out_channels, layer.conv1.out_channels // layer.conv2.out_channels))
        f.add_module('denseblock%d' % (i + 1), b)
        if trans is not None:
            t = nn.Sequential()
            t.add_module('norm', nn.BatchNorm2d(trans.conv.in_channels))
            t.add_module('relu', nn.ReLU())
            t.add_module('conv', nn.Conv2d(trans.conv.in_channels, trans.conv.out_channels, 1, bias=False))
            t.add_module('pool', nn.AvgPool2d(2, 2))
            f.add_module('transition%d' % (i + 1), t)
    f.add_module('norm5', nn.BatchNorm2d(net.features.conv.in_channels))
    f.add_module('conv', nn.Conv2d(net.features.conv.in_channels, net.features.conv.out_channels, 1))
    m = nn.Module()
    m.features = f
    m.forward = lambda x: f(x)
    m.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()}, strict=True)
    return m.double()


def build_inference(golden, sd=None):
    import model
    import model.densenet
    g = golden('densenet')
    if sd is None:
        sd = {k: torch.from_numpy(np.array(v)) for k, v in unpack(g, 'sd').items()}
    anchors = torch.from_numpy(synth.ANCHORS_VOC)
    net = model.densenet.DenseNet(model.ConfigChannels(config()), anchors, 20, **NARROW)
    net.load_state_dict(sd, strict=True)
    return model.Inference(config(), net, anchors).to(dev()), anchors


def test_training_step_matches_reference_fixture(golden):
    """Output, every parameter gradient and every running statistic of one step on sum(out * R): within max(2e-4, 4 x the stored fp32 floor of that tensor)."""
    dnn, g = narrow_net(golden)
    dnn.train()
    x = synth.images(2, 96, seed=1).to(dev())
    out = dnn(x)
    (out * torch.from_numpy(g['train_R']).to(dev())).sum().backward()
    e = rel(out, torch.from_numpy(g['train_out_fp64']))
    print('densenet training output: %.2e (floor %.2e)' % (e, float(g['train_floor'])))
    assert e <= max(2e-4, 4 * float(g['train_floor']))
    grads, run = unpack(g, 'grad'), unpack(g, 'run')
    params = dict(dnn.named_parameters())
    assert list(params) == list(grads)
    worst = 0.0
    for (k, ref), floor in zip(grads.items(), g['gfloor']):
        assert params[k].grad is not None, k
        e = rel(params[k].grad, torch.from_numpy(np.array(ref)))
        worst = max(worst, e / max(2e-4, 4 * float(floor)))
        assert e <= max(2e-4, 4 * float(floor)), (k, e, float(floor))
    bufs = dict(dnn.named_buffers())
    for (k, ref), floor in zip(run.items(), g['rfloor']):
        e = rel(bufs[k], torch.from_numpy(np.array(ref)))
        assert e <= max(2e-4, 4 * float(floor)), (k, e, float(floor))
    print('densenet training gradients: worst error / bound = %.2f' % worst)
    assert all(int(b) == 1 for k, b in bufs.items() if k.endswith('num_batches_tracked'))


def test_region_loss_training_step_matches_oracle_autograd(golden):
    import model
    from oracle import head as ohead
    from oracle import loss as oloss
    inf, anchors = build_inference(golden)
    inf.train()
    net = inf.dnn
    S, B, C = 96, 3, 20
    x = synth.images(B, S, seed=1)
    data = synth.norm_data(synth.labels(B, S, C, seed=2), S, S, S // 32, S // 32)
    twins = {dt: twin_module(net).to(dt).train() for dt in (torch.float64, torch.float32)}      # (from the statistics before the step)
    calls = {}
    net.grad_ready_hook = lambda p, g: calls.__setitem__(id(p), calls.get(id(p), 0) + 1)
    pred = model._inference(inf, x.to(dev()))
    loss, _ = model.loss(anchors, data, pred, 0.6)
    sum(loss[k] * oloss.HPARAM[k] for k in loss).backward()
    net.grad_ready_hook = None
    assert sorted(calls.values()) == [1] * len(list(net.parameters())) and set(calls) == {id(p) for p in net.parameters()}
    results = {}
    for dt in (torch.float64, torch.float32):
        t = twins[dt]
        f = t(x.to(dt))
        an = anchors.to(dt)
        lo, _ = oloss.loss(an, {k: (v.to(dt) if v.is_floating_point() else v) for k, v in data.items()}, ohead.decode(f, an), 0.6)
        oloss.total(lo).backward()
        results[dt] = (lo, t)
    lo, t64 = results[torch.float64]
    _, t32 = results[torch.float32]
    for k in lo:
        np.testing.assert_allclose(loss[k].item(), lo[k].item(), rtol=5e-4)
    for (k, a), r, q in zip(net.named_parameters(), t64.parameters(), t32.parameters()):
        floor = rel(q.grad, r.grad)
        assert rel(a.grad, r.grad) <= max(2e-3, 4 * floor), (k, rel(a.grad, r.grad), floor)
    b64 = [b for k, b in t64.state_dict().items() if 'running' in k]
    bours = [b for k, b in net.state_dict().items() if 'running' in k]
    for a, r in zip(bours, b64):
        np.testing.assert_allclose(a.cpu().numpy(), r.numpy(), rtol=1e-4, atol=1e-6)


def test_frozen_bn_eval_with_grad_matches_fp64_twin(golden):
    inf, _ = build_inference(golden)
    net = inf.dnn.eval()
    x = synth.images(2, 96, seed=6)
    xg = x.to(dev()).requires_grad_()
    out = net(xg)
    R = torch.randn(out.shape, generator=torch.Generator().manual_seed(8))
    (out * R.to(dev())).sum().backward()
    results = {}
    for dt in (torch.float64, torch.float32):
        t = twin_module(net).to(dt).eval()
        xr = x.to(dt).requires_grad_()
        o = t(xr)
        (o * R.to(dt)).sum().backward()
        results[dt] = (o, t, xr)
    (o64, t64, x64), (o32, t32, x32) = results[torch.float64], results[torch.float32]
    assert rel(out.detach().cpu(), o64) <= max(2e-5, 4 * rel(o32, o64))
    assert rel(xg.grad.cpu(), x64.grad) <= max(2e-4, 4 * rel(x32.grad, x64.grad))
    for (k, a), r, q in zip(net.named_parameters(), t64.parameters(), t32.parameters()):
        assert rel(a.grad, r.grad) <= max(2e-4, 4 * rel(q.grad, r.grad)), k
    assert all(int(b) == 0 for k, b in net.named_buffers() if k.endswith('num_batches_tracked'))


def test_deterministic_mode_training_steps_are_bit_identical(golden):
    import model
    from oracle import loss as oloss
    S, B, C = 96, 2, 20
    x = synth.images(B, S, seed=1).to(dev())
    data = synth.norm_data(synth.labels(B, S, C, seed=2), S, S, S // 32, S // 32)
    runs = []
    _hip.set_deterministic(True)
    try:
        for _ in range(2):
            inf, anchors = build_inference(golden)
            inf.train()
            pred = model._inference(inf, x)
            loss, _ = model.loss(anchors, data, pred, 0.6)
            sum(loss[k] * oloss.HPARAM[k] for k in loss).backward()
            runs.append(([p.grad.clone() for p in inf.dnn.parameters()], [b.clone() for b in inf.dnn.buffers()], pred['feature'].detach().clone()))
    finally:
        _hip.set_deterministic(False)
    (g1, b1, f1), (g2, b2, f2) = runs
    assert torch.equal(f1, f2)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    assert all(torch.equal(a, b) for a, b in zip(b1, b2))


def test_captured_training_step_equals_autograd_step(golden):
    import train as y2train
    import utils
    from oracle import loss as oloss
    inf, anchors = build_inference(golden)
    inf.train()
    S, B = 96, 3
    data = []
    for seed in (1, 2):
        d = {k: v.to(dev()) for k, v in synth.labels(B, S, 20, nmax=6, seed=10 + seed).items()}
        d['tensor'] = synth.images(B, S, seed=seed).to(dev())
        data.append(d)
    opt = utils.optim.SGD(inf.parameters(), 0.0)
    for i in range(6):                 # 3 eager plan passes, the capture, replays
        r = y2train.iterate(inf, opt, data[i % 2], oloss.HPARAM, 0.6, anchors)
        assert np.isfinite(float(r['loss_total']))
    runner = inf.__dict__['_y2_step_runner']
    assert runner.captures == 1 and not runner.broken
    for i in range(2):
        y2train.PLAN = False
        try:
            wit, _ = build_inference(golden, sd={k: v.clone() for k, v in inf.dnn.state_dict().items()})
            wit.train()
            w = y2train.iterate(wit, utils.optim.SGD(wit.parameters(), 0.0), data[i], oloss.HPARAM, 0.6, anchors)
        finally:
            y2train.PLAN = True
        r = y2train.iterate(inf, opt, data[i], oloss.HPARAM, 0.6, anchors)
        np.testing.assert_allclose(float(r['loss_total']), float(w['loss_total']), rtol=2e-5)
        for (k, a), (_, b) in zip(inf.dnn.named_parameters(), wit.dnn.named_parameters()):
            assert rel(a.grad, b.grad) <= 1e-3, (i, k, rel(a.grad, b.grad))


def test_widths_that_are_not_multiples_of_4_run_in_inference_and_refuse_training():
    import model
    import model.densenet
    torch.manual_seed(3)
    net = model.densenet.DenseNet(model.ConfigChannels(config()), torch.from_numpy(synth.ANCHORS_VOC), 20, growth_rate=6, block_config=(2, 3, 2, 2),
                                  num_init_features=10, bn_size=3)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 0.5 + 0.75)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.bias.shape, generator=g) + 0.5)
    t64 = twin_module(net).eval()
    x = synth.images(2, 128, seed=5)
    with torch.no_grad():
        ref = t64(x.double())
        floor = rel(twin_module(net).float().eval()(x), ref)
        out = net.to(dev()).eval()(x.to(dev()))
    err = rel(out, ref)
    print('densenet growth_rate=6: %.2e (twin fp32 floor %.2e)' % (err, floor))
    assert err <= max(2e-5, 2.5 * floor)
    net.train()
    with pytest.raises(RuntimeError, match='multiples of 4'):
        net(x.to(dev()))


def test_graphed_detector_equals_eager_detection_and_replans(golden):
    import detect
    net, _ = narrow_net(golden)
    anchors = torch.from_numpy(synth.ANCHORS_VOC)
    for S in (416, 320):
        x = synth.images(2, S, seed=S).to(dev())
        gd = detect.GraphedDetector(net, anchors, x)
        got = gd.run(x)
        with torch.no_grad():
            want = detect.detect_batch(net.forward_nhwc(x), anchors, fix=True)
        assert set(got.keys()) == set(want.keys())
        for k in want:
            if not torch.is_tensor(want[k]):
                continue
            if k in ('index', 'keep'):           # candidate / survivor lists: valid up to their per-image counts
                n = want['count' if k == 'index' else 'keep_count'].view(-1).tolist()
                for b, c in enumerate(n):
                    assert torch.equal(got[k][b, :c], want[k][b, :c]), (S, k, b)
            else:
                assert torch.equal(got[k], want[k]), (S, k)
        assert net._plans.latest()['key'][3:5] == (S, S)
