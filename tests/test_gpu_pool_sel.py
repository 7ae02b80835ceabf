"""Pooled blocks keep z_sel, the one pre-activation per 2x2 window that the pool selects: the producer of z_sel against its definition,
the forward over z_sel against the pooled forward over z (bit for bit), pass 1 of the BatchNorm backward from (z_sel, dy_pool) against fp64 autograd,
and a Darknet training step with the path on, off and forced onto the activation kernel's producer.
Every gamma vector has both signs and an exact zero; constructed inputs hold windows with two equal extremes and windows whose extreme is -0 / +0."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import darknet as odark
from oracle import head as ohead
from oracle import loss as oloss
from oracle import synth
from oracle.make_golden import NARROW

pytestmark = pytest.mark.gpu
B, H, W = 3, 8, 12


def dev():
    return torch.device('cuda:0')


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def rel(got, ref):
    ref = ref.double()
    rms = ref.pow(2).mean().sqrt().item()
    return (got.double().cpu() - ref).abs().max().item() / max(rms, 1e-30)


def mixed_gamma(C, g):
    """|gamma| in [0.25, 1.5], signs alternating in pairs, gamma[1] exactly 0."""
    gamma = 0.25 + 1.25 * torch.rand(C, generator=g, dtype=torch.float64)
    gamma[(torch.arange(C) // 2) % 2 == 1] *= -1.0
    gamma[1] = 0.0
    return gamma


def constructed_z(C, g):
    """[B,H,W,C] fp32: random, plus per channel a window with two equal maxima, one with two equal minima and two whose extreme is a -0 / +0 pair."""
    z = torch.randn(B, H, W, C, generator=g, dtype=torch.float64).float()
    z[0, 0, 0] = z[0, 1, 1] = 5.0
    z[0, 2, 3] = z[0, 3, 2] = -5.0
    z[1, 0:2, 0:2] = -1.0
    z[1, 0, 0], z[1, 0, 1] = -0.0, 0.0           # the maximum of its window: the first of the pair is selected where gamma > 0
    z[1, 2:4, 2:4] = 1.0
    z[1, 2, 2], z[1, 2, 3] = 0.0, -0.0           # the minimum of its window: selected where gamma < 0
    return z


def z_sel_definition(z, gamma):
    """The definition: per window (scan order) and channel the FIRST z_q that maximises sign(gamma) * z_q, strict comparison.  z: [B,H,W,C] fp32 numpy."""
    s = np.sign(gamma).astype(np.float32)
    win = [z[:, 0::2, 0::2], z[:, 0::2, 1::2], z[:, 1::2, 0::2], z[:, 1::2, 1::2]]
    best, sel = s * win[0], win[0].copy()
    for q in (1, 2, 3):
        key = s * win[q]
        m = key > best
        best, sel = np.where(m, key, best), np.where(m, win[q], sel)
    return sel


def bits(t):
    return (t.cpu().numpy() if torch.is_tensor(t) else t).view(np.uint32)


def affine(z, gamma, beta):
    """fp32 (scale, shift, mean, invstd) of training-mode BatchNorm over z [B,H,W,C]."""
    z64 = z.double()
    mean = z64.mean((0, 1, 2))
    invstd = 1.0 / torch.sqrt(z64.var((0, 1, 2), unbiased=False) + 1e-5)
    scale = gamma.float() * invstd.float()
    shift = beta.float() - mean.float() * scale
    return scale, shift, mean.float(), invstd.float()


@pytest.fixture(scope='module', params=[32, 6])           # CV = 4 (16-byte accesses) and CV = 1
def case(request):
    C = request.param
    g = torch.Generator().manual_seed(7 + C)
    z = constructed_z(C, g)
    gamma = mixed_gamma(C, g)
    beta = 0.1 + 0.2 * torch.rand(C, generator=g, dtype=torch.float64)            # never 0: the activations of -0 and +0 are the same bits
    scale, shift, mean, invstd = affine(z, gamma, beta)
    assert (torch.sign(scale) == torch.sign(gamma.float())).all()
    d = dev()
    return dict(C=C, z=z, gamma=gamma, beta=beta, zd=z.to(d), scale=scale.to(d), shift=shift.to(d), mean=mean.to(d), invstd=invstd.to(d),
                gd=gamma.float().to(d), want=z_sel_definition(z.numpy(), gamma.numpy()))


def run_fwd_sel(c):
    import _hip
    L, C = _hip.lib(), c['C']
    yp = torch.full((B, H // 2, W // 2, C), 7.0, device=dev())
    zs = torch.full((B, H // 2, W // 2, C), 7.0, device=dev())
    _hip.check(L.y2_bn_act_fwd_sel(_hip.ptr(c['zd']), _hip.ptr(c['scale']), _hip.ptr(c['shift']), 0.1, _hip.ptr(yp), _hip.ptr(zs), B, H, W, C, C, C, 0, C, _hip.stream()), 'fwd_sel')
    return yp, zs


def run_fwd(c, z, h, w, pool):
    import _hip
    L, C = _hip.lib(), c['C']
    out = torch.full((B, h // 2, w // 2, C) if pool else (B, h, w, C), 7.0, device=dev())
    _hip.check(L.y2_bn_act_fwd(_hip.ptr(z), _hip.ptr(c['scale']), _hip.ptr(c['shift']), 0.1, None if pool else _hip.ptr(out), _hip.ptr(out) if pool else None,
                               B, h, w, C, C, C, 0, C, 0, 0, _hip.stream()), 'fwd')
    return out


def test_activation_kernel_writes_the_defined_z_sel(case):
    """Producer (i): z at the first maximal activation.  On these inputs (no two different z of a window round to one activation) that IS the definition,
    exactly; the pooled activation of the same launch is the plain pooled launch's, bit for bit."""
    yp, zs = run_fwd_sel(case)
    assert np.array_equal(bits(zs), bits(case['want']))
    assert np.array_equal(bits(yp), bits(run_fwd(case, case['zd'], H, W, True)))


@pytest.mark.parametrize('Hc,Wc', [(32, 32), (12, 20)])          # every tile inside the image (the straight-line epilogue); the bounds-checked kernel
def test_first_layer_convolution_writes_the_defined_z_sel(Hc, Wc):
    """Producer (ii): z_sel against the definition applied to the SAME launch's z; z and the statistics against the launch without z_sel.  One output
    channel has zero weights: every window of it is a four-way tie."""
    import _hip
    L = _hip.lib()
    d = dev()
    Bc, C = 2, 32
    g = torch.Generator().manual_seed(Hc + Wc)
    x = torch.randn(Bc, 3, Hc, Wc, generator=g).to(d)
    w = 0.3 * torch.randn(C, 3, 3, 3, generator=g)
    w[5] = 0.0
    w = w.to(d)
    gamma = mixed_gamma(C, g).float()
    out = {}
    for form in ('sel', 'plain'):
        z = torch.full((Bc, Hc, Wc, C), 7.0, device=d)
        zs = torch.full((Bc, Hc // 2, Wc // 2, C), 7.0, device=d)
        stats = torch.zeros(32, 2 * C, dtype=torch.float64, device=d)          # Y2_STATS_REPL replicated accumulators
        if form == 'sel':
            gd = gamma.to(d)
            _hip.check(L.y2_conv0_fwd_sel(_hip.ptr(x), _hip.ptr(w), _hip.ptr(gd), _hip.ptr(z), _hip.ptr(zs), _hip.ptr(stats), Bc, Hc, Wc, 3, C, C, C, _hip.stream()), 'conv0_sel')
        else:
            _hip.check(L.y2_conv0_fwd(_hip.ptr(x), _hip.ptr(w), None, None, _hip.ptr(z), None, _hip.ptr(stats), Bc, Hc, Wc, 3, C, C, 0, 1.0, _hip.stream()), 'conv0')
        out[form] = (z.cpu().numpy(), zs.cpu().numpy(), stats.sum(0).cpu().numpy())
    z, zs, st = out['sel']
    assert np.array_equal(bits(zs), bits(z_sel_definition(z, gamma.numpy())))
    assert (z[..., 5] == 0).all()
    assert np.array_equal(z, out['plain'][0])          # (values: the bounds-checked kernel of the plain launch passes z through an identity affine, -0 -> +0)
    np.testing.assert_allclose(st, out['plain'][2], rtol=1e-12, atol=0)


def test_forward_over_z_sel_is_the_pooled_forward_bit_for_bit(case):
    """Consequence (a): the activation is monotone in z per channel, so act(z_sel) is the window's maximal activation (scales of both signs and zero)."""
    zs = torch.from_numpy(case['want']).to(dev())
    got = run_fwd(case, zs, H // 2, W // 2, False)
    assert np.array_equal(bits(got), bits(run_fwd(case, case['zd'], H, W, True)))


@pytest.mark.parametrize('C', [32, 6])
def test_pass1_from_z_sel_matches_fp64_autograd(C):
    """Built as tests/test_gpu_train.py::test_bn_act_forward_backward builds its pooled case, with that test's tolerances."""
    import _hip
    L = _hip.lib()
    d = dev()
    g = torch.Generator().manual_seed(C + 1)
    z = constructed_z(C, g).permute(0, 3, 1, 2).double().requires_grad_(True)          # fp32 values: the fp64 reference sees the same ties
    gamma = mixed_gamma(C, g).requires_grad_(True)
    beta = (0.1 + 0.2 * torch.rand(C, generator=g, dtype=torch.float64)).requires_grad_(True)
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    yp = F.max_pool2d(F.leaky_relu(F.batch_norm(z, rm, rv, gamma, beta, True, 0.01, 1e-5), 0.1), 2)
    dyp = torch.randn(yp.shape, generator=g, dtype=torch.float64)
    (yp * dyp).sum().backward()
    # ---- ours
    zd = nhwc(z.detach().float()).to(d)
    stats = torch.zeros(32, 2 * C, dtype=torch.float64)
    stats[5] = torch.stack([z.detach().sum((0, 2, 3)), (z.detach() ** 2).sum((0, 2, 3))]).reshape(-1)
    stats = stats.reshape(-1).to(d)
    scale, shift, mean, invstd = (torch.empty(C, device=d) for _ in range(4))
    gd, bd = gamma.detach().float().to(d), beta.detach().float().to(d)
    _hip.check(L.y2_bn_finalize(_hip.ptr(stats), float(B * H * W), _hip.ptr(gd), _hip.ptr(bd), None, None, 0.01, 1e-5,
                                _hip.ptr(scale), _hip.ptr(shift), _hip.ptr(mean), _hip.ptr(invstd), C, None, _hip.stream()), 'fin')
    ypo, zs = run_fwd_sel(dict(C=C, zd=zd, scale=scale, shift=shift))
    assert rel(ypo.permute(0, 3, 1, 2), yp.detach()) <= 2e-5
    dypd = nhwc(dyp.float()).to(d)
    got = {}
    for form in ('sel', 'sel_sums_only', 'full'):
        sums = torch.zeros(2 * C, dtype=torch.float64, device=d)
        dz = torch.empty(B, H, W, C, device=d) if form != 'sel_sums_only' else None
        if form == 'full':
            _hip.check(L.y2_bn_act_bwd(_hip.ptr(zd), _hip.ptr(scale), _hip.ptr(shift), _hip.ptr(mean), _hip.ptr(invstd), _hip.ptr(gd), 0.1,
                                       None, 0, 0, 0, _hip.ptr(dypd), C, 0, _hip.ptr(sums), _hip.ptr(dz), C, B, H, W, C, C, 1, _hip.stream()), 'bwd')
        else:
            _hip.check(L.y2_bn_act_bwd_sel(_hip.ptr(zd), _hip.ptr(zs), C, _hip.ptr(scale), _hip.ptr(shift), _hip.ptr(mean), _hip.ptr(invstd), _hip.ptr(gd), 0.1,
                                           _hip.ptr(dypd), C, 0, _hip.ptr(sums), _hip.ptr(dz), C, B, H, W, C, C, _hip.stream()), 'bwd_sel')
        got[form] = sums.cpu().numpy()
        print(form, 'max |sum error|', np.abs(got[form] - np.concatenate([beta.grad.numpy(), gamma.grad.numpy()])).max())
        np.testing.assert_allclose(got[form][:C], beta.grad.numpy(), rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(got[form][C:], gamma.grad.numpy(), rtol=1e-4, atol=1e-4)
        if dz is not None:
            assert rel(dz.permute(0, 3, 1, 2), z.grad) <= 5e-5
    np.testing.assert_allclose(got['sel'], got['full'], rtol=1e-4, atol=1e-4)


def test_bwd_sel_refuses_what_it_does_not_cover():
    import _hip
    L = _hip.lib()
    t = torch.zeros(2 * 2 * 2 * 4, device=dev())
    s = torch.zeros(8, dtype=torch.float64, device=dev())
    p = _hip.ptr(t)
    assert L.y2_bn_act_bwd_sel(p, None, 4, p, p, p, p, p, 0.1, p, 4, 0, _hip.ptr(s), None, 4, 1, 2, 2, 4, 4, _hip.stream()) != 0          # no z_sel
    assert L.y2_bn_act_bwd_sel(p, p, 4, p, p, p, p, p, 0.1, None, 4, 0, _hip.ptr(s), None, 4, 1, 2, 2, 4, 4, _hip.stream()) != 0          # no pooled gradient
    assert L.y2_bn_act_bwd_sel(p, p, 4, p, p, p, p, p, 0.1, p, 4, 0, _hip.ptr(s), None, 4, 1, 3, 2, 4, 4, _hip.stream()) != 0             # odd height
    assert L.y2_bn_act_fwd_sel(p, p, p, 0.1, p, None, 1, 2, 2, 4, 4, 4, 0, 4, _hip.stream()) != 0                                          # no z_sel


# ---------------------------------------------------------------------------------------------------------------- one training step
GRAD_TOL = 2e-4        # tests/test_gpu_train.py: the bound of test_darknet_training_step_matches_oracle_autograd
S, SB = 64, 2


@pytest.fixture(scope='module')
def step_oracle():
    widths = dict(NARROW)
    widths['layers1.5'] = 8
    sd = odark.init_state_dict(5, 20, seed=0, channels=widths, head_scale=1 / 8.0)
    for k, v in sd.items():           # both signs and an exact zero in every BatchNorm weight
        if k.endswith('.bn.weight'):
            v[(torch.arange(v.numel()) // 2) % 2 == 1] *= -1.0
            v[1] = 0.0
    anchors = torch.from_numpy(synth.ANCHORS_VOC)
    x = synth.images(SB, S, seed=1)
    data = synth.norm_data(synth.labels(SB, S, 20, seed=2), S, S, S // 32, S // 32)
    data64 = {k: (v.double() if v.is_floating_point() else v) for k, v in data.items()}
    sd64 = {k: v.double().requires_grad_(v.is_floating_point() and 'running' not in k) for k, v in sd.items()}
    lo, _ = oloss.loss(anchors.double(), data64, ohead.decode(odark.forward(x.double(), sd64, training=True), anchors.double()), 0.6)
    oloss.total(lo).backward()
    sd32 = {k: v.clone().requires_grad_(v.is_floating_point() and 'running' not in k) for k, v in sd.items()}
    l32, _ = oloss.loss(anchors, data, ohead.decode(odark.forward(x, sd32, training=True), anchors), 0.6)
    oloss.total(l32).backward()
    ref = {k: v.grad for k, v in sd64.items() if v.requires_grad}
    bound = {k: max(GRAD_TOL, 2.5 * rel(sd32[k].grad, ref[k])) for k in ref}
    return dict(sd=sd, anchors=anchors, x=x, data=data, loss={k: lo[k].item() for k in lo}, ref=ref, bound=bound)


def test_training_step_with_the_path_on_off_and_forced(step_oracle, monkeypatch):
    import configparser

    import _hip
    import model
    import model.yolo2
    from model import train_graph as tg
    o = step_oracle
    grads = {}
    for mode in (True, False, 'act'):
        monkeypatch.setattr(tg, 'POOL_SEL', mode)
        seen, conv_sel = [], []
        decide = tg._decide_bwd
        L = _hip.lib()
        real = L.y2_conv0_fwd_sel
        monkeypatch.setattr(L, 'y2_conv0_fwd_sel', lambda *a: conv_sel.append(1) or real(*a), raising=False)
        monkeypatch.setattr(tg, '_decide_bwd', lambda *a, **k: seen.append(decide(*a, **k)) or seen[-1])
        cfg = configparser.ConfigParser()
        cfg.read_dict({'batch_norm': {'enable': '1'}})
        dnn = model.yolo2.Darknet(model.ConfigChannels(cfg, o['sd']), o['anchors'], 20)
        dnn.load_state_dict(o['sd'], strict=False)
        inf = model.Inference(cfg, dnn, o['anchors']).to(dev()).train()
        pred = model._inference(inf, o['x'].to(dev()))
        loss, _ = model.loss(o['anchors'], o['data'], pred, 0.6)
        sum(loss[k] * oloss.HPARAM[k] for k in loss).backward()
        monkeypatch.setattr(tg, '_decide_bwd', decide)
        monkeypatch.setattr(L, 'y2_conv0_fwd_sel', real, raising=False)
        assert sum(p.sel for p in seen[-1]) == (4 if mode else 0), mode          # layers1.0, .2, .6, .10
        assert len(conv_sel) == (1 if mode is True else 0), mode                 # the first layer's own producer, unless off or forced onto the activation kernel's
        for k in o['loss']:
            np.testing.assert_allclose(loss[k].item(), o['loss'][k], rtol=1e-4)
        ours = dict(inf.dnn.named_parameters())
        for k, r in o['ref'].items():
            assert ours[k].grad is not None, k
            e = rel(ours[k].grad, r)
            assert e <= o['bound'][k], (mode, k, e, o['bound'][k])
        grads[mode] = {k: ours[k].grad.detach().clone() for k in o['ref']}
    for a, b in ((True, False), ('act', False), (True, 'act')):
        for k in o['ref']:
            e = rel(grads[a][k], grads[b][k].cpu())
            assert e <= o['bound'][k], (a, b, k, e)
