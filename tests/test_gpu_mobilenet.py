"""The MobileNet plugin on the MI355X (model.mobilenet, reference model/mobilenet.py:54-85): the depthwise kernels of csrc/dwconv.hip
against fp64 torch (F.conv2d with groups=C and its autograd), the plugin against the reference fixture tests/golden/mobilenet.npz
(tools/make_golden_mobilenet.py), a default-width network against an fp64 torch.nn twin, a region-loss training step against the
oracle's fp64 autograd, the captured training step against the autograd step, and GraphedDetector against eager detection."""
import configparser
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import head as ohead
from oracle import loss as oloss
from oracle import synth

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


def nhwc(t, ld):
    """[B,C,H,W] -> a device buffer [B,H,W,ld] holding it in channels [0, C) (the rest poison)."""
    B, C, H, W = t.shape
    buf = torch.full((B, H, W, ld), float('nan'), dtype=torch.float32, device=dev())
    buf[..., :C] = t.permute(0, 2, 3, 1).to(dev(), torch.float32)
    return buf


def take(buf, C):
    return buf[..., :C].permute(0, 3, 1, 2).double().cpu()


# ------------------------------------------------------------------------------------------------ kernels
CASES = [  # B, C, H, W, stride, ld
    (2, 4, 13, 13, 1, 4), (2, 32, 13, 13, 2, 32), (1, 36, 7, 9, 1, 40), (3, 36, 7, 9, 2, 36), (2, 1024, 13, 13, 1, 1024),
    (1, 1024, 7, 9, 2, 1028), (2, 6, 13, 13, 1, 6), (1, 6, 7, 9, 2, 7), (2, 32, 1, 1, 1, 32), (2, 32, 1, 1, 2, 36), (1, 4, 16, 12, 2, 8),
    (2, 32, 26, 26, 1, 32),
]


def dw_forward_ref(x, w, stride, scale=None, shift=None, relu=False):
    y = F.conv2d(x.double(), w.double(), stride=stride, padding=1, groups=x.shape[1])
    raw = y
    if scale is not None:
        y = y * scale.double().view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.double().view(1, -1, 1, 1)
    return (F.relu(y) if relu else y), raw


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('epi', ['plain', 'affine_relu'])
def test_dwconv_fwd_matches_fp64(case, epi):
    B, C, H, W, s, ld = case
    g = torch.Generator().manual_seed(B * 1000 + C + H * 7 + W + s)
    x, w = torch.randn(B, C, H, W, generator=g), torch.randn(C, 1, 3, 3, generator=g)
    scale, shift = (torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)) if epi != 'plain' else (None, None)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    xb = nhwc(x, ld)
    yb = torch.full((B, Ho, Wo, ld), float('nan'), device=dev())
    wd = w.to(dev()).contiguous()
    sc = scale.to(dev()) if scale is not None else None
    sh = shift.to(dev()) if shift is not None else None
    stats = torch.zeros(_hip.STATS_REPL * 2 * C, dtype=torch.float64, device=dev())
    rc = L().y2_dwconv_fwd(_hip.ptr(xb), _hip.ptr(wd), _hip.ptr(sc), _hip.ptr(sh), 0.0 if epi != 'plain' else 1.0, _hip.ptr(yb), _hip.ptr(stats),
                           B, H, W, C, ld, ld, s, _hip.stream())
    assert rc == 0
    torch.cuda.synchronize()
    ref, raw = dw_forward_ref(x, w, s, scale, shift, relu=epi != 'plain')
    assert rel(take(yb, C), ref) <= 2e-5
    if ld > C:
        assert torch.isnan(yb[..., C:]).all()           # the channels past C of the output pixels are not written
    st = stats.view(_hip.STATS_REPL, 2, C).sum(0).cpu()
    np.testing.assert_allclose(st[0].numpy(), raw.sum((0, 2, 3)).numpy(), rtol=1e-5, atol=1e-6 * raw.abs().sum().item() / C)
    np.testing.assert_allclose(st[1].numpy(), raw.pow(2).sum((0, 2, 3)).numpy(), rtol=1e-5)


def run_dgrad(dz_b, wd, dxb, B, H, W, C, ldz, lddx, s):
    return L().y2_dwconv_dgrad(_hip.ptr(dz_b), _hip.ptr(wd), _hip.ptr(dxb), B, H, W, C, ldz, lddx, s, _hip.stream())


def run_wgrad(xb, dz_b, B, H, W, C, ldx, ldz, s):
    nws = L().y2_dwconv_wgrad_workspace_bytes(B, H, W, C, s)
    ws = torch.full((nws // 4 + 4,), float('nan'), device=dev())
    dw = torch.full((C, 1, 3, 3), float('nan'), device=dev())
    rc = L().y2_dwconv_wgrad(_hip.ptr(xb), _hip.ptr(dz_b), _hip.ptr(dw), _hip.ptr(ws), ws.numel() * 4, B, H, W, C, ldx, ldz, s, _hip.stream())
    return rc, dw


@pytest.mark.parametrize('case', CASES)
def test_dwconv_gradients_match_fp64_autograd_and_are_reproducible(case):
    B, C, H, W, s, ld = case
    g = torch.Generator().manual_seed(7 + B * 1000 + C + H * 7 + W + s)
    x, w = torch.randn(B, C, H, W, generator=g).double().requires_grad_(), torch.randn(C, 1, 3, 3, generator=g).double().requires_grad_()
    y = F.conv2d(x, w, stride=s, padding=1, groups=C)
    dz = torch.randn(y.shape, generator=g).double()
    y.backward(dz)
    xb, dz_b = nhwc(x.detach(), ld), nhwc(dz, ld + 4)
    wd = w.detach().float().to(dev()).contiguous()
    dxb = torch.full((B, H, W, ld), float('nan'), device=dev())
    assert run_dgrad(dz_b, wd, dxb, B, H, W, C, ld + 4, ld, s) == 0
    rc, dw = run_wgrad(xb, dz_b, B, H, W, C, ld, ld + 4, s)
    assert rc == 0
    torch.cuda.synchronize()
    assert rel(take(dxb, C), x.grad) <= 8e-5
    assert rel(dw.double().cpu(), w.grad) <= 8e-5
    # no atomics: a second launch gives the same bits
    dx2 = torch.full_like(dxb, float('nan'))
    assert run_dgrad(dz_b, wd, dx2, B, H, W, C, ld + 4, ld, s) == 0
    _, dw2 = run_wgrad(xb, dz_b, B, H, W, C, ld, ld + 4, s)
    torch.cuda.synchronize()
    assert torch.equal(dx2[..., :C], dxb[..., :C]) and torch.equal(dw2, dw)


def test_dwconv_misaligned_operands_take_the_scalar_path_and_bad_workspace_is_refused():
    B, C, H, W, s = 2, 8, 9, 9, 1
    g = torch.Generator().manual_seed(11)
    x, w = torch.randn(B, C, H, W, generator=g), torch.randn(C, 1, 3, 3, generator=g)
    base = torch.zeros(B * H * W * C + 1, device=dev())
    xb = base[1:].view(B, H, W, C)                     # 4-byte aligned, not 16-byte
    xb.copy_(x.permute(0, 2, 3, 1))
    yb = torch.empty(B, H, W, C, device=dev())
    wd = w.to(dev())
    assert L().y2_dwconv_fwd(_hip.ptr(xb), _hip.ptr(wd), None, None, 1.0, _hip.ptr(yb), None, B, H, W, C, C, C, s, _hip.stream()) == 0
    torch.cuda.synchronize()
    assert rel(take(yb, C), dw_forward_ref(x, w, s)[0]) <= 2e-5
    nws = L().y2_dwconv_wgrad_workspace_bytes(B, H, W, C, s)
    ws = torch.empty(nws // 4 + 8, device=dev())
    dw = torch.empty(C, 1, 3, 3, device=dev())
    args = (B, H, W, C, C, C, s, _hip.stream())
    assert L().y2_dwconv_wgrad(_hip.ptr(xb), _hip.ptr(yb), _hip.ptr(dw), ws.data_ptr() + 4, nws, *args) == -2          # Y2_EALIGN
    assert L().y2_dwconv_wgrad(_hip.ptr(xb), _hip.ptr(yb), _hip.ptr(dw), _hip.ptr(ws), nws - 4, *args) == -1           # too small
    assert L().y2_dwconv_fwd(_hip.ptr(xb), _hip.ptr(wd), None, None, 1.0, _hip.ptr(yb), None, B, H, W, C, C - 1, C, s, _hip.stream()) == -1
    assert L().y2_dwconv_fwd(_hip.ptr(xb), _hip.ptr(wd), None, None, 1.0, _hip.ptr(yb), None, B, H, W, C, C, C, 3, _hip.stream()) == -1


def test_dwconv_stats_refused_in_deterministic_mode():
    B, C, H, W = 1, 8, 5, 5
    x = torch.randn(B, H, W, C, device=dev())
    w = torch.randn(C, 1, 3, 3, device=dev())
    y = torch.empty_like(x)
    stats = torch.zeros(_hip.STATS_REPL * 2 * C, dtype=torch.float64, device=dev())
    _hip.set_deterministic(True)
    try:
        assert L().y2_dwconv_fwd(_hip.ptr(x), _hip.ptr(w), None, None, 1.0, _hip.ptr(y), _hip.ptr(stats), B, H, W, C, C, C, 1, _hip.stream()) == -3
        assert L().y2_dwconv_fwd(_hip.ptr(x), _hip.ptr(w), None, None, 1.0, _hip.ptr(y), None, B, H, W, C, C, C, 1, _hip.stream()) == 0
    finally:
        _hip.set_deterministic(False)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the plugin against the reference fixture
def cfg():
    c = configparser.ConfigParser()
    c.read_dict({'model': {'dnn': 'model.mobilenet.MobileNet'}})
    return c


def fixture_net(golden, train=False):
    import model
    import model.mobilenet
    g = golden('mobilenet')
    sd = {k: torch.from_numpy(g['sd/' + k]) for k in g['keys']}
    net = model.mobilenet.MobileNet(model.ConfigChannels(cfg(), sd), torch.from_numpy(synth.ANCHORS_VOC), 20)
    net.load_state_dict(sd)
    net = net.to(dev())
    return (net.train() if train else net.eval()), g


def test_eval_output_matches_reference_fixture(golden):
    net, g = fixture_net(golden)
    inputs = dict(x96=synth.images(2, 96, seed=1), x64x96=torch.from_numpy(g['x64x96']))
    for name, x in inputs.items():
        with torch.no_grad():
            out = net(x.to(dev()))
        ref = torch.from_numpy(g['eval_%s_fp64' % name])
        assert out.shape == ref.shape
        assert rel(out.cpu(), ref) <= 2e-5, (name, rel(out.cpu(), ref))


def test_training_step_matches_reference_fixture(golden):
    net, g = fixture_net(golden, train=True)
    x = synth.images(2, 96, seed=1).to(dev())
    out = net(x)
    R = torch.from_numpy(g['train_R']).to(dev())
    (out * R).sum().backward()
    bound = lambda floor: max(2e-4, 4 * float(floor))     # noqa: E731
    assert rel(out.detach().cpu(), torch.from_numpy(g['train_out_fp64'])) <= bound(g['train_floor'])
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        e = rel(p.grad.cpu(), torch.from_numpy(g['grad/' + k]))
        assert e <= bound(g['gfloor/' + k]), (k, e, float(g['gfloor/' + k]))
    bufs = dict(net.named_buffers())
    for k, b in bufs.items():
        if k.endswith('num_batches_tracked'):
            assert int(b) == 1, k
        else:
            e = rel(b.cpu(), torch.from_numpy(g['run/' + k]))
            assert e <= bound(g['rfloor/' + k]), (k, e)


# ------------------------------------------------------------------------------------------------ full width against an fp64 torch.nn twin
def twin(net):
    """fp64 torch.nn copy of a MobileNet plugin (Conv2d with groups, BatchNorm2d, ReLU), from its state_dict."""
    layers = []
    for m in net.layers:
        if isinstance(m, nn.Conv2d):
            layers.append(nn.Conv2d(m.in_channels, m.out_channels, 1))
            continue
        seqs = [m] if hasattr(m, 'conv') else [m.dw, m.pw]
        for sq in seqs:
            c = sq.conv
            layers += [nn.Conv2d(c.in_channels, c.out_channels, c.kernel_size, c.stride, c.padding, groups=c.groups, bias=False),
                       nn.BatchNorm2d(c.out_channels), nn.ReLU()]
    t = nn.Sequential(*layers).double()
    sd = [v for k, v in net.state_dict().items()]
    tsd = t.state_dict()
    assert len(sd) == len(tsd)
    t.load_state_dict({k: v.detach().double().cpu() if v.is_floating_point() else v.cpu() for k, v in zip(tsd.keys(), sd)})
    return t


def default_net(seed=0):
    import model
    import model.mobilenet
    torch.manual_seed(seed)
    net = model.mobilenet.MobileNet(model.ConfigChannels(cfg()), torch.from_numpy(synth.ANCHORS_VOC), 20)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.25)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
        net.layers[14].weight.mul_(0.25)
        net.layers[14].bias.copy_(torch.randn(125, generator=g) * 0.1)
    return net


def test_full_width_eval_matches_fp64_twin():
    net = default_net()
    t64 = twin(net).eval()
    t32 = twin(net).float().eval()
    x = synth.images(2, 416, seed=4)
    net = net.to(dev()).eval()
    with torch.no_grad():
        out = net(x.to(dev())).cpu()
        ref = t64(x.double())
        floor = rel(t32(x), ref)
    assert out.shape == (2, 125, 13, 13)
    assert rel(out, ref) <= max(2e-5, 2.5 * floor), (rel(out, ref), floor)


def test_pruned_odd_widths_run_in_inference_and_refuse_training():
    import model
    import model.mobilenet
    sd = default_net().state_dict()
    odd = {}
    for k, v in sd.items():                 # layers.3.pw -> 30 channels: a width that is not a multiple of 4
        if k == 'layers.3.pw.conv.weight':
            v = v[:30]
        elif k.startswith('layers.3.pw.bn.') and v.dim():
            v = v[:30]
        elif k in ('layers.4.dw.conv.weight',) or (k.startswith('layers.4.dw.bn.') and v.dim()):
            v = v[:30]
        elif k == 'layers.4.pw.conv.weight':
            v = v[:, :30]
        odd[k] = v
    net = model.mobilenet.MobileNet(model.ConfigChannels(cfg(), odd), torch.from_numpy(synth.ANCHORS_VOC), 20)
    net.load_state_dict(odd)
    t64 = twin(net).eval()
    x = synth.images(1, 128, seed=5)
    net = net.to(dev()).eval()
    with torch.no_grad():
        out = net(x.to(dev())).cpu()
        ref = t64(x.double())
        floor = rel(twin(net).float().eval()(x), ref)
    assert rel(out, ref) <= max(2e-5, 2.5 * floor)
    net.train()
    with pytest.raises(RuntimeError, match='layers.3.pw.conv.weight'):
        net(x.to(dev()))


# ------------------------------------------------------------------------------------------------ region-loss training step
def narrow_sd(golden):
    g = golden('mobilenet')
    return {k: torch.from_numpy(g['sd/' + k]).clone() for k in g['keys']}


def build_inference(golden, sd=None):
    import model
    import model.mobilenet
    sd = narrow_sd(golden) if sd is None else sd
    anchors = torch.from_numpy(synth.ANCHORS_VOC)
    net = model.mobilenet.MobileNet(model.ConfigChannels(cfg(), sd), anchors, 20)
    net.load_state_dict(sd)
    c = cfg()
    return model.Inference(c, net, anchors).to(dev()), anchors


def test_region_loss_training_step_matches_oracle_autograd(golden):
    import model
    inf, anchors = build_inference(golden)
    inf.train()
    net = inf.dnn
    S, B, C = 96, 3, 20
    x = synth.images(B, S, seed=1)
    data = synth.norm_data(synth.labels(B, S, C, seed=2), S, S, S // 32, S // 32)
    twins = {dt: twin(net).to(dt).train() for dt in (torch.float64, torch.float32)}      # (from the statistics before the step)
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
    ours = list(net.parameters())
    p64, p32 = list(t64.parameters()), list(t32.parameters())
    names = [k for k, _ in net.named_parameters()]
    for k, a, r, q in zip(names, ours, p64, p32):
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
        t = twin(net).to(dt).eval()
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


# ------------------------------------------------------------------------------------------------ captured training step
def test_captured_training_step_equals_autograd_step(golden):
    import train as y2train
    import utils
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


# ------------------------------------------------------------------------------------------------ detection
def test_graphed_detector_equals_eager_detection_and_replans(golden):
    import detect
    inf, anchors = build_inference(golden)
    net = inf.dnn.eval()
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
