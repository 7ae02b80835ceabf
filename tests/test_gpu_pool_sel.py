"""Pooled blocks keep z_sel, the one pre-activation per 2x2 window that the pool selects: the producer of z_sel against its definition,
the forward over z_sel against the pooled forward over z (bit for bit), pass 1 of the BatchNorm backward from (z_sel, dy_pool) against fp64 autograd,
a Darknet training step with the path on, off and forced onto the activation kernel's producer, and - the second half of the file - every dispatch path of
y2_bn_act_fwd_sel and y2_bn_act_bwd_sel (tests/pool_sel_cases.py) against the definition and fp64 autograd.  The first layer's own producer,
y2_conv0_fwd_sel, has its dispatch paths in tests/test_gpu_conv0_sel.py.
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


# ================================================================================================ every dispatch path of the two streaming entries
# tests/pool_sel_cases.py holds the cases and the mirror of bn_act_fwd_impl / bn_act_bwd_impl (checked on the CPU by tests/test_pool_sel_cases.py).
# Inputs: z is a multiple of 1 / 64 in [-4, 4] (513 values) plus constructed_z's tie and -0 / +0 windows; with |scale| >= 0.25 two different z of a window
# never round to one activation, so `z at the first maximal activation` (what the kernels compute) and the header's definition select the same element in EVERY
# window - the number of windows where they could differ is asserted to be 0; it is a condition of the inputs, not a tolerance.  Every map is a channel window
# of rows of -7.0 between -7.0 guards, its base pointer on or one float off a 16-byte boundary as the case says.
import ctypes
import functools

import pool_sel_cases as pc
from test_gpu_conv0_sel import definition
from test_gpu_streaming import BN_EPS, TOL, TOL_DZ
from test_gpu_wgrad import GUARD, SENT, deterministic, kernels_of

SUM_TOL = dict(rtol=1e-4, atol=1e-4)          # the sums' bound of test_pass1_from_z_sel_matches_fp64_autograd above


class Map(object):
    """rows x ld floats of -7.0 between two guards; the data (or the destination) is the channel window off .. off + C; the base pointer lies `mis` floats
    past a 16-byte boundary."""

    def __init__(self, rows, C, ld, off=0, mis=0, data=None):
        self.flat = torch.full((GUARD + 4 + rows * ld + GUARD,), SENT, dtype=torch.float32, device=dev())
        self.start, self.rows, self.C, self.ld, self.off = GUARD + mis, rows, C, ld, off
        self.view = self.flat[self.start:self.start + rows * ld].view(rows, ld)
        self.win = self.view[:, off:off + C]
        if data is not None:
            self.win.copy_(data.reshape(rows, C))
        self.ptr = ctypes.c_void_p(self.flat.data_ptr() + 4 * self.start)
        assert (self.ptr.value % 16 != 0) == bool(mis)
        self.before = self.flat.clone()

    def unchanged(self):
        return torch.equal(self.flat.view(torch.int32), self.before.view(torch.int32))

    def outside_intact(self):
        """Everything but the channel window still holds the sentinel."""
        m = self.flat.clone()
        m[self.start:self.start + self.rows * self.ld].view(self.rows, self.ld)[:, self.off:self.off + self.C] = SENT
        return bool((m == SENT).all())


def grid_z(Bc, Hc, Wc, C, g):
    """[B,H,W,C] fp32: multiples of 1 / 64 in [-4, 4], with constructed_z's windows: two equal maxima, two equal minima, a -0 / +0 pair at either extreme."""
    z = torch.randint(-256, 257, (Bc, Hc, Wc, C), generator=g).float() / 64
    if Bc >= 2 and Hc >= 4 and Wc >= 4:
        z[0, 0, 0] = z[0, 1, 1] = 4.0
        z[0, 2, 3] = z[0, 3, 2] = -4.0
        z[1, 0:2, 0:2] = -1.0
        z[1, 0, 0], z[1, 0, 1] = -0.0, 0.0
        z[1, 2:4, 2:4] = 1.0
        z[1, 2, 2], z[1, 2, 3] = 0.0, -0.0
    return z


def signed(C, g, lo, hi):
    """|v| in [lo, hi], signs alternating in pairs, v[1] = 0 and v[2] = -0.0: both signs, an exact zero and a -0.0."""
    v = lo + (hi - lo) * torch.rand(C, generator=g, dtype=torch.float64)
    v[(torch.arange(C) // 2) % 2 == 1] *= -1.0
    v[1], v[2] = 0.0, -0.0
    v = v.float()
    assert bool((v > 0).any()) and bool((v < 0).any()) and v[1:3].view(torch.int32).tolist() == [0, -(1 << 31)]
    return v


def windows_where_the_rules_could_differ(z, scale, shift, slope):
    """Windows (per channel with a non-zero scale) in which two DIFFERENT z have the same fp32 activation: there `first maximal activation` may pick another
    element than the definition.  (A zero scale maps every z to one activation: both rules keep the first element.)"""
    v = F.leaky_relu(z * scale + shift, slope)                    # fp32, one rounding per operation, as the kernel
    zq = [z[:, i::2, j::2] for i in (0, 1) for j in (0, 1)]
    vq = [v[:, i::2, j::2] for i in (0, 1) for j in (0, 1)]
    bad = torch.zeros_like(zq[0], dtype=torch.bool)
    for a in range(4):
        for b in range(a + 1, 4):
            bad |= (vq[a] == vq[b]) & (zq[a] != zq[b])
    return int(bad[..., scale != 0].sum())


def pooled(c):
    return c.B * (c.H // 2) * (c.W // 2)


# ------------------------------------------------------------------------------------------------ forward
def fwd_call(c, z, scale, shift, yp, zs, sel=True):
    import _hip
    L = _hip.lib()
    s = pc.strides(c)
    nul = lambda name, p: None if name in c.null else p
    sc, sh = (_hip.ptr(scale), _hip.ptr(shift)) if c.affine else (None, None)
    if sel:
        return L.y2_bn_act_fwd_sel(nul('z', z.ptr), sc, sh, 0.1, nul('y_pool', yp.ptr), nul('z_sel', zs.ptr), c.B, c.H, c.W, c.C, s['ldz'], s['ldp'], c.poff, s['ldzs'], _hip.stream())
    return L.y2_bn_act_fwd(z.ptr, sc, sh, 0.1, None, yp.ptr, c.B, c.H, c.W, c.C, s['ldz'], 0, 0, s['ldp'], c.poff, 0, _hip.stream())


@pytest.mark.parametrize('name', list(pc.FWD_CASES))
def test_bn_act_fwd_sel_paths(name):
    """z_sel bit-equal to the header's definition, y_pool bit-equal to the plain pooled launch's and within TOL of fp64 max_pool2d(leaky_relu(batch_norm))."""
    c = pc.FWD_CASES[name].c
    r = pc.fwd_route(c)
    assert r.rc == pc.OK
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    z = grid_z(c.B, c.H, c.W, c.C, g)
    scale = signed(c.C, g, 0.25, 1.5) if c.affine else torch.ones(c.C)
    shift = (0.1 + 0.2 * torch.rand(c.C, generator=g, dtype=torch.float64)).float() if c.affine else torch.zeros(c.C)
    assert windows_where_the_rules_could_differ(z, scale, shift, 0.1) == 0
    s = pc.strides(c)
    zm = Map(c.B * c.H * c.W, c.C, s['ldz'], 0, c.zmis, z.to(dev()))
    sd, hd = scale.to(dev()), shift.to(dev())
    out = {}
    for sel in (True, False):
        yp = Map(pooled(c), c.C, s['ldp'], c.poff, c.pmis)
        zs = Map(pooled(c), c.C, s['ldzs'], 0, c.smis)
        names = kernels_of(lambda: out.__setitem__('rc', fwd_call(c, zm, sd, hd, yp, zs, sel)))
        assert out['rc'] == 0 and names == ['bn_act_fwd_kernel']
        assert yp.outside_intact() and zs.outside_intact() and zm.unchanged() and (sel or zs.unchanged())
        out[sel] = (yp.win.clone(), zs.win.clone())
    want = definition(z.to(dev()), sd).reshape(-1, c.C)
    assert torch.equal(out[True][1].view(torch.int32), want.view(torch.int32)), 'z_sel is not the definition'
    assert torch.equal(out[True][0].view(torch.int32), out[False][0].view(torch.int32)), 'y_pool differs from the plain pooled launch\'s'
    z64 = z.double().permute(0, 3, 1, 2)
    ref = F.max_pool2d(F.leaky_relu(F.batch_norm(z64, torch.zeros(c.C, dtype=torch.float64), torch.ones(c.C, dtype=torch.float64) - BN_EPS, scale.double(), shift.double(), False, 0.0, BN_EPS), 0.1), 2)          # (running variance 1 - eps: the affine z * scale + shift)
    e = rel(out[True][0].view(c.B, c.H // 2, c.W // 2, c.C).permute(0, 3, 1, 2), ref)
    print('y_pool against fp64: %.3g x rms' % e)
    assert e <= TOL


@pytest.mark.parametrize('name', list(pc.FWD_REFUSALS))
def test_bn_act_fwd_sel_refusals(name):
    """Every pointer is valid but the one under test; a refusal writes nothing."""
    c, rc = pc.FWD_REFUSALS[name]
    assert pc.fwd_route(c).rc == rc
    maps = [Map(64, 8, 16) for _ in range(3)]
    sc = torch.ones(16, device=dev())
    assert fwd_call(c, maps[0], sc, sc, maps[1], maps[2]) == rc
    torch.cuda.synchronize()
    assert all(m.unchanged() for m in maps)


# ------------------------------------------------------------------------------------------------ backward
@functools.lru_cache(maxsize=4)
def bwd_reference(Bc, Hc, Wc, C):
    """Inputs of one geometry and the fp64 autograd of max_pool2d(leaky_relu(batch_norm(z))), shared (read only) by the cases of that geometry."""
    g = torch.Generator().manual_seed(Bc + 3 * Hc + 5 * Wc + 7 * C)
    z = grid_z(Bc, Hc, Wc, C, g)
    gamma = signed(C, g, 0.75, 1.5)
    beta = (0.1 + 0.2 * torch.rand(C, generator=g, dtype=torch.float64)).float()
    dyp = torch.randn(Bc, C, Hc // 2, Wc // 2, generator=g, dtype=torch.float32)
    z64 = z.double().permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        _, mean, invstd = torch.native_batch_norm(z64, gamma.double(), beta.double(), None, None, True, 0.0, BN_EPS)
        zhat = (z64 - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)
        # LeakyReLU's derivative jumps at 0: a channel with a pre-activation within 1e-3 of 0 gets another beta (neighbouring pre-activations lie |scale| / 64 >= 0.004 apart)
        for _ in range(16):
            pre = zhat * gamma.double().view(1, -1, 1, 1) + beta.double().view(1, -1, 1, 1)
            close = (pre.abs() < 1e-3).flatten(2).any(2).any(0)
            if not bool(close.any()):
                break
            beta[close] += 0.002
        assert pre.abs().min().item() >= 1e-3, 'test input: a pre-activation sits on the LeakyReLU kink'
    scale = (gamma.double() * invstd).float()
    shift = (beta.double() - mean * gamma.double() * invstd).float()
    assert float(scale[scale != 0].abs().min()) >= 0.25 and windows_where_the_rules_could_differ(z, scale, shift, 0.1) == 0
    zr = z64.clone().requires_grad_(True)
    ga, be = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    yp = F.max_pool2d(F.leaky_relu(F.batch_norm(zr, None, None, ga, be, True, 0.0, BN_EPS), 0.1), 2)
    (yp * dyp.double()).sum().backward()
    return dict(z=z, gamma=gamma, dyp=dyp, mean=mean.float(), invstd=invstd.float(), scale=scale, shift=shift, dz=zr.grad, dbeta=be.grad.numpy(), dgamma=ga.grad.numpy())


class BwdRun(object):
    """One y2_bn_act_bwd_sel call (sel=False: the pooled-only y2_bn_act_bwd on the same operands) on fresh buffers."""

    def __init__(self, c, ref, sel=True, alloc=None):
        import _hip
        L = _hip.lib()
        d = dev()
        call_c, c = c, alloc or c                                     # (alloc: a refusal - the buffers are built for `alloc`, the call carries c)
        s = pc.strides(c)
        C, rows, prow = c.C, c.B * c.H * c.W, pooled(c)
        self.held = {k: ref[k].to(d) for k in ('scale', 'shift', 'mean', 'invstd', 'gamma')}
        zd = ref['z'].to(d)
        self.z = Map(rows, C, s['ldz'], 0, c.zmis, zd)
        zs = definition(zd, self.held['gamma'])
        self.dyp = Map(prow, C, s['ldp'], c.poff, c.pmis, ref['dyp'].permute(0, 2, 3, 1).to(d))
        if c.dz == 'alias':          # one allocation: z_sel in its first quarter, dz over all of it
            assert s['ldzs'] == C and s['ldd'] == C
            self.dz = Map(rows, C, C, 0, c.smis)
            self.dz.view[:prow].copy_(zs.reshape(prow, C))
            self.zs = None
            zs_ptr = self.dz.ptr
        else:
            self.zs = Map(prow, C, s['ldzs'], 0, c.smis, zs)
            zs_ptr = self.zs.ptr
            self.dz = Map(rows, C, s['ldd'], 0, c.dmis) if c.dz != 'null' else None
        self.sums = torch.full((2 * C + 4,), SENT, dtype=torch.float64, device=d)
        self.sums[:2 * C] = 0.0
        nul = lambda name, p: None if name in c.null else p
        h = {k: _hip.ptr(v) for k, v in self.held.items()}
        dzp = self.dz.ptr if self.dz is not None else None
        c, s, C = call_c, pc.strides(call_c), call_c.C

        def call():
            if sel:
                self.rc = L.y2_bn_act_bwd_sel(nul('z', self.z.ptr), nul('z_sel', zs_ptr), s['ldzs'], h['scale'], h['shift'], nul('mean', h['mean']), nul('invstd', h['invstd']), nul('gamma', h['gamma']),
                                              0.1, nul('dy_pool', self.dyp.ptr), s['ldp'], c.poff, nul('sums', _hip.ptr(self.sums)), dzp, s['ldd'], c.B, c.H, c.W, C, s['ldz'], _hip.stream())
            else:
                self.rc = L.y2_bn_act_bwd(self.z.ptr, h['scale'], h['shift'], h['mean'], h['invstd'], h['gamma'], 0.1, None, 0, 0, 0, self.dyp.ptr, s['ldp'], c.poff,
                                          _hip.ptr(self.sums), dzp, s['ldd'], c.B, c.H, c.W, C, s['ldz'], 1, _hip.stream())
        self.kernels = kernels_of(call)

    def intact(self):
        return (self.z.unchanged() and self.dyp.unchanged() and (self.zs is None or self.zs.unchanged()) and (self.dz is None or self.dz.outside_intact())
                and bool((self.sums[-4:] == SENT).all()))


def check_bwd(c, ref, run):
    C = c.C
    assert run.rc == 0 and run.intact()
    got = run.sums[:2 * C].cpu().numpy()
    print('max |sum error| %.3g' % np.abs(got - np.concatenate([ref['dbeta'], ref['dgamma']])).max())
    np.testing.assert_allclose(got[:C], ref['dbeta'], **SUM_TOL)
    np.testing.assert_allclose(got[C:], ref['dgamma'], **SUM_TOL)
    if run.dz is not None:
        e = rel(run.dz.win.view(c.B, c.H, c.W, C).permute(0, 3, 1, 2), ref['dz'])
        print('dz against fp64: %.3g x rms' % e)
        assert e <= TOL_DZ


@pytest.mark.parametrize('name', list(pc.BWD_CASES))
def test_bn_act_bwd_sel_paths(name):
    """Sums and dz against fp64 autograd, and the reduction form the mirror names, observed by kernel name: the block-reduce kernel exactly when the partial
    sums are parked, the det-reduce kernel exactly in deterministic mode.  Deterministic mode: a second run is bit-identical, and the sums are those of the
    pooled-only y2_bn_act_bwd bit for bit (the same grid, the same loop order, a sum that differs only by zero terms: DESIGN.md 3.4)."""
    import _hip
    c = pc.BWD_CASES[name].c
    r = pc.bwd_route(c)
    assert r.rc == pc.OK
    ref = bwd_reference(c.B, c.H, c.W, c.C)
    want = ['bn_act_bwd_kernel'] + {'atomics': [], 'parked': ['bn_bwd_block_reduce_kernel'], 'det': ['det_reduce_rows_kernel']}[r.form] + (['bn_act_bwd_kernel'] if c.dz != 'null' else [])
    if not c.det:
        run = BwdRun(c, ref)
        assert run.kernels == want, (run.kernels, r)
        check_bwd(c, ref, run)
        return
    with deterministic():
        a, b, full = BwdRun(c, ref), BwdRun(c, ref), BwdRun(c, ref, sel=False)
    assert not _hip.lib().y2_get_deterministic()
    assert a.kernels == b.kernels == full.kernels == want, (a.kernels, full.kernels)
    for run in (a, b, full):
        check_bwd(c, ref, run)
    assert torch.equal(a.sums.view(torch.int64), b.sums.view(torch.int64)) and (a.dz is None or torch.equal(a.dz.flat.view(torch.int32), b.dz.flat.view(torch.int32))), 'two deterministic runs differ'
    assert torch.equal(a.sums.view(torch.int64), full.sums.view(torch.int64)), 'deterministic sums from z_sel are not the pooled-only backward\'s, bit for bit'
    assert a.dz is None or torch.equal(a.dz.flat.view(torch.int32), full.dz.flat.view(torch.int32))


@pytest.mark.parametrize('name', list(pc.BWD_REFUSALS))
def test_bn_act_bwd_sel_refusals(name):
    """Every pointer is valid but the one under test; a refusal writes nothing."""
    import _hip
    c, rc = pc.BWD_REFUSALS[name]
    assert pc.bwd_route(c).rc == rc
    if c.det_small:
        with deterministic(pc.DET_SMALL_BYTES):
            run = BwdRun(c, bwd_reference(c.B, c.H, c.W, c.C))
        assert not _hip.lib().y2_get_deterministic()
    else:
        alloc = pc.K()                                                 # what the buffers are built for; the call carries c's sizes, strides and NULLs
        run = BwdRun(c, bwd_reference(alloc.B, alloc.H, alloc.W, alloc.C), alloc=alloc)
    assert run.rc == rc and run.kernels == []
    assert run.intact() and (run.dz is None or run.dz.unchanged()) and not bool(run.sums[:-4].any())
