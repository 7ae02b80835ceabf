"""GPU parity tests of the raw epilogue of wino_fused3_kernel (csrc/wino.hip: OUT bit 3) and of y2_conv_fwd_sel, the same launch as the
producer of z_sel, one instantiation at a time: the explicit and the implicit loader, the one-slab variants (Cin 32), the half-unit
variant (Cout 32, implicit), units with missing channels (Cout 96), whole and ragged tile rows, odd maps (raw only), rows wider than Cout with a channel
offset.  algo / tile are set in the parameters, as in tests/test_gpu_fwd.py.

y and z_sel are channel windows of rows of -7.0 between -7.0 guards; x, the filter and gamma are NaN-guarded; the workspace is NaN-filled.  Two regimes:

  exact    x = k / 4, w = k / 8 with |k| <= 4 and one all-zero output channel.  The filter transform (halves and quarters of sums of three w) gives multiples of
           1 / 32 no larger than 9 / 8, the input transform multiples of 1 / 4 no larger than 4, a product is a multiple of 1 / 128 and all 16 * Cin of them sum
           below 2^24 / 128; the output transform only adds.  Every sum is exact in fp32 in ANY order: z must equal the fp64 F.conv2d bit for bit (-0 == +0),
           z_sel the header's definition applied to it, and the statistics the fp64 sums (|z| <= 36 * Cin / 32 on a grid of 1 / 32, so z^2 is a multiple of
           1 / 1024 below 5184 and a lane's 32 terms per unit sum exactly in fp32 as well).
  random   z of the raw launch == z of the same launch with scale = ones, shift = zeros (the instantiation without bit 3: the epilogue this one replaces);
           z_sel == the definition applied to that z; statistics against fp64 sums at the tolerance of tests/test_gpu_fwd.py for this kernel (WINO_STATS).

gamma has both signs, +0 and -0 within any seven neighbours.  The definition is written with torch.where, not as the kernel's loop."""
import collections
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_wgrad import GUARD, NAN, SENT, Dest, Operand, dev, kernels_of, nhwc, rel

pytestmark = pytest.mark.gpu
OK, EINVAL, ENOSUP = 0, -1, -3
WINO_TOL = 8e-5                 # tests/test_gpu_fwd.py: x rms of the fp64 reference, both Winograd forms
WINO_STATS = (1e-5, 2e-5, 2e-5)  # ibid.: (relative on the sum, absolute x sqrt(max sum of squares), relative on the sum of squares)
GAMMA = (1.5, -0.75, 0.0, -0.0, -2.0, 0.25, 3.0)
FUSED, IMPLICIT = 2, 3          # Y2_ALGO_WINOGRAD_FUSED, Y2_ALGO_WINOGRAD_IMPLICIT

Case = collections.namedtuple('Case', 'cin cout H W algo')
# name -> case.  8x8 at B = 2: 32 tiles, one whole unit; 12x20: 120 tiles, three whole units and a ragged one; 7x9: odd, 40 tiles
SEL_CASES = {
    'cin32-explicit-8x8': Case(32, 64, 8, 8, FUSED),              # VAR 8
    'cin32-implicit-12x20': Case(32, 64, 12, 20, IMPLICIT),       # VAR 12
    'cin64-explicit-12x20': Case(64, 64, 12, 20, FUSED),          # VAR 0
    'cin64-implicit-8x8': Case(64, 64, 8, 8, IMPLICIT),           # VAR 4
    'cin64-implicit-12x20': Case(64, 64, 12, 20, IMPLICIT),
    'cout96-explicit-8x8': Case(64, 96, 8, 8, FUSED),             # the second channel unit has 32 of 64 channels
    'cout96-implicit-12x20': Case(64, 96, 12, 20, IMPLICIT),
    'cout32-implicit-12x20': Case(64, 32, 12, 20, IMPLICIT),      # VAR 20
}
RAW_CASES = dict(SEL_CASES, **{
    'cin32-explicit-7x9': Case(32, 64, 7, 9, FUSED),
    'cin32-implicit-7x9': Case(32, 64, 7, 9, IMPLICIT),
    'cin64-explicit-7x9': Case(64, 96, 7, 9, FUSED),
    'cin64-implicit-7x9': Case(64, 64, 7, 9, IMPLICIT),
    'cout32-implicit-7x9': Case(64, 32, 7, 9, IMPLICIT),
    'cout32-implicit-8x8': Case(64, 32, 8, 8, IMPLICIT),
})
B = 2
LAYOUTS = {'dense': (0, 0), 'wide': (8, 4)}          # (floats a row is wider than Cout, channel offset of the window): y's ldy / coff, z_sel's ldzs / pointer


def zero_channel(cout):
    return 5


def gamma_of(cout):
    g = torch.tensor([GAMMA[i % len(GAMMA)] for i in range(cout)], dtype=torch.float32)
    bits = g.view(torch.int32)
    assert bool((g > 0).any()) and bool((g < 0).any()) and bool((bits == 0).any()) and bool((bits == -(1 << 31)).any())
    return g


def definition(z, gamma):
    """The header's z_sel of z [n,H,W,C]: per window and channel the FIRST z_q in scan order that maximises sign(gamma) * z_q under a strict comparison."""
    s = (gamma > 0).to(z.dtype) - (gamma < 0).to(z.dtype)
    win = [z[:, 0::2, 0::2], z[:, 0::2, 1::2], z[:, 1::2, 0::2], z[:, 1::2, 1::2]]
    best, sel = s * win[0], win[0]
    for q in (1, 2, 3):
        key = s * win[q]
        m = key > best
        best, sel = torch.where(m, key, best), torch.where(m, win[q], sel)
    return sel


@functools.lru_cache(maxsize=None)
def reference(c, regime):
    """x [B,cin,H,W], w [cout,cin,3,3] in fp32 and z = the fp64 convolution [B,H,W,cout], on the CPU.  Shared by every test of a case: read only."""
    g = torch.Generator().manual_seed(11 + 10007 * c.cin + 101 * c.cout + 13 * c.H + 7 * c.W + c.algo)
    if regime == 'exact':
        x = torch.randint(-4, 5, (B, c.cin, c.H, c.W), generator=g).float() / 4
        w = torch.randint(-4, 5, (c.cout, c.cin, 3, 3), generator=g).float() / 8
    else:
        x = torch.randn(B, c.cin, c.H, c.W, generator=g)
        w = torch.randn(c.cout, c.cin, 3, 3, generator=g) * (2.0 / (9 * c.cin)) ** 0.5
    w[zero_channel(c.cout)] = 0.0
    z = F.conv2d(x.double(), w.double(), padding=1)
    if regime == 'exact':
        assert torch.equal(F.conv2d(x, w, padding=1).double(), z), 'the exact regime is not exact: fp32 and fp64 convolutions differ'
    return x, w, nhwc(z)


Ops = collections.namedtuple('Ops', 'x u gamma ones zeros keep')


@functools.lru_cache(maxsize=4)
def operands(c, regime):
    import _hip
    L, st = _hip.lib(), _hip.stream()
    x, w, _ = reference(c, regime)
    wd = w.to(dev()).contiguous()
    n = w.numel()
    pbuf = torch.full((GUARD + n + GUARD,), NAN, dtype=torch.float32, device=dev())
    ubuf = torch.full((GUARD + 16 * c.cout * c.cin + GUARD,), NAN, dtype=torch.float32, device=dev())
    wp, u = pbuf[GUARD:GUARD + n], ubuf[GUARD:GUARD + 16 * c.cout * c.cin]
    _hip.check(L.y2_pack_weight(_hip.ptr(wd), _hip.ptr(wp), c.cout, c.cin, 3, 0, st), 'pack')
    _hip.check(L.y2_wino_weight(_hip.ptr(wp), _hip.ptr(u), c.cout, c.cin, st), 'filter transform')
    torch.cuda.synchronize()
    assert bool(torch.isfinite(u).all())
    one = lambda v: Operand(torch.full((1, c.cout), v))
    return Ops(Operand(nhwc(x), 8, 4), u, Operand(gamma_of(c.cout).view(1, -1)), one(1.0), one(0.0), [pbuf, ubuf])


Result = collections.namedtuple('Result', 'rc names y zs stats')


def launch(c, ops, lay, entry='plain', stats=True, forced=False, algo=None, tile=3, scale=False, pool=False, gamma=True, zsel=True, ldzs=None, H=None):
    """One y2_conv_fwd ('plain') or y2_conv_fwd_sel ('sel') call.  forced: scale = ones, shift = zeros - the same values from the epilogue without bit 3.
    The keywords behind it build the refusals."""
    import _hip
    L = _hip.lib()
    pad, off = LAYOUTS[lay]
    H = c.H if H is None else H
    q = _hip.ConvParams()
    q.x, q.ldx, q.w = ops.x.ptr.value, ops.x.ld, ops.u.data_ptr()
    q.B, q.H, q.W, q.Cin, q.Cout, q.ksize = B, H, c.W, c.cin, c.cout, 3
    q.slope, q.tile, q.algo = 1.0, tile, c.algo if algo is None else algo
    if forced or scale:
        q.scale, q.shift = ops.ones.ptr.value, ops.zeros.ptr.value
    y = Dest(B * H * c.W * (c.cout + pad))
    q.y, q.ldy, q.coff = y.ptr.value, c.cout + pad, off
    zs = Dest(B * (H // 2) * (c.W // 2) * (c.cout + pad)) if entry == 'sel' or pool else None
    if pool:
        q.y_pool, q.ldp, q.poff = zs.ptr.value, c.cout + pad, off
    st = torch.zeros(32 * 2 * c.cout, dtype=torch.float64, device=dev()) if stats else None
    q.stats = st.data_ptr() if stats else None
    need = L.y2_conv_fwd_workspace_bytes(ctypes.byref(q))
    assert need >= 0, need
    ws = torch.full((need // 4 + 4,), NAN, dtype=torch.float32, device=dev())
    q.workspace, q.workspace_bytes = ws.data_ptr(), need
    rc = []
    if entry == 'sel':
        call = lambda: rc.append(L.y2_conv_fwd_sel(ctypes.byref(q), ops.gamma.ptr if gamma else None, ctypes.c_void_p(zs.ptr.value + 4 * off) if zsel else None,
                                                   c.cout + pad if ldzs is None else ldzs, _hip.stream()))
    else:
        call = lambda: rc.append(L.y2_conv_fwd(ctypes.byref(q), _hip.stream()))
    names = kernels_of(call)
    return Result(rc[0], names, y, zs, st)


def window(d, c, lay, H, W):
    """The channel window of a destination as a device tensor [B,H,W,cout]; everything around it must still be the sentinel."""
    pad, off = LAYOUTS[lay]
    assert d.guards_intact()
    full = d.t.view(-1, c.cout + pad)
    assert bool((full[:, :off] == SENT).all()) and bool((full[:, off + c.cout:] == SENT).all()), 'wrote outside its channel window'
    got = full[:, off:off + c.cout].reshape(B, H, W, c.cout)
    assert bool(torch.isfinite(got).all()), 'the result depends on memory outside the operands (or on what the workspace held)'
    return got


def where_wrong(bad):
    """The images, rows, columns and channels of the wrong elements of a [B,H,W,C] mask, for the failure message."""
    idx = bad.nonzero().cpu()
    return '%d of %d wrong; images %s rows %s columns %s channels %s' % ((len(idx), bad.numel()) + tuple(sorted(set(idx[:, i].tolist()))[:24] for i in range(4)))


def check_stats(r, z64, cout, exact):
    got = r.stats.cpu().view(32, 2 * cout).sum(0)
    assert bool(torch.isfinite(got).all())
    s1, s2 = z64.sum((0, 1, 2)), (z64 * z64).sum((0, 1, 2))
    rt1, at1, rt2 = (1e-12, 0.0, 1e-12) if exact else WINO_STATS
    e1 = ((got[:cout] - s1).abs() - rt1 * s1.abs()).max().item()
    print('statistics: sum off by at most %.3g, sum of squares by %.3g relative' % ((got[:cout] - s1).abs().max().item(), ((got[cout:] - s2).abs() / s2.clamp_min(1e-300)).max().item()))
    assert e1 <= at1 * float(s2.max().sqrt()), 'sum'
    assert bool(((got[cout:] - s2).abs() <= rt2 * s2.abs()).all()), 'sum of squares'


def check(c, lay, regime, entry, stats):
    ops = operands(c, regime)
    _, _, z64 = reference(c, regime)
    r = launch(c, ops, lay, entry, stats)
    assert r.rc == OK, r.rc
    assert r.names[-1] == ('wino_fused3_kernel[implicit]' if c.algo == IMPLICIT else 'wino_fused3_kernel'), r.names
    z = window(r.y, c, lay, c.H, c.W)
    zd = z64.to(dev())
    if regime == 'exact':
        assert torch.equal(z.double(), zd), 'z is not the fp64 convolution: ' + where_wrong(z.double() != zd)
    else:
        f = launch(c, ops, lay, 'plain', stats, forced=True)
        assert f.rc == OK and f.names == r.names
        assert torch.equal(z, window(f.y, c, lay, c.H, c.W)), 'z differs from the epilogue without bit 3'
        e = rel(z, z64)
        print('z against fp64: %.3g x rms' % e)
        assert e <= WINO_TOL, e
    assert bool((z[..., zero_channel(c.cout)] == 0).all())
    if entry == 'sel':
        gd = gamma_of(c.cout).to(dev())
        zs = window(r.zs, c, lay, c.H // 2, c.W // 2)
        assert torch.equal(definition(z, gd).view(torch.int32), zs.view(torch.int32)), 'z_sel is not the definition applied to the launch\'s own z'
        if regime == 'exact':
            assert torch.equal(zs.double(), definition(zd, gd.double())), 'z_sel is not the definition applied to the fp64 convolution'
    if stats:
        check_stats(r, z64, c.cout, regime == 'exact')


@pytest.mark.parametrize('lay', list(LAYOUTS))
@pytest.mark.parametrize('name', list(RAW_CASES))
def test_raw_exact(name, lay):
    check(RAW_CASES[name], lay, 'exact', 'plain', True)


@pytest.mark.parametrize('stats', [True, False])
@pytest.mark.parametrize('name', list(RAW_CASES))
def test_raw_random(name, stats):
    check(RAW_CASES[name], 'wide', 'random', 'plain', stats)


@pytest.mark.parametrize('lay', list(LAYOUTS))
@pytest.mark.parametrize('name', list(SEL_CASES))
def test_sel_exact(name, lay):
    check(SEL_CASES[name], lay, 'exact', 'sel', True)


@pytest.mark.parametrize('stats', [True, False])
@pytest.mark.parametrize('name', list(SEL_CASES))
def test_sel_random(name, stats):
    check(SEL_CASES[name], 'wide', 'random', 'sel', stats)


def test_sel_writes_the_z_and_statistics_of_the_plain_launch():
    c = SEL_CASES['cin64-implicit-12x20']
    ops = operands(c, 'random')
    a, b = launch(c, ops, 'wide', 'sel'), launch(c, ops, 'wide', 'plain')
    assert a.rc == OK and b.rc == OK
    assert torch.equal(window(a.y, c, 'wide', c.H, c.W), window(b.y, c, 'wide', c.H, c.W))
    sa, sb = a.stats.view(32, -1).sum(0), b.stats.view(32, -1).sum(0)
    assert bool(((sa - sb).abs() <= 1e-12 * sb.abs() + 1e-12).all())          # (the same fp32 partial sums; their fp64 atomics arrive in any order)


REFUSALS = {
    'direct': (dict(algo=0, tile=0), ENOSUP),
    'three-kernel': (dict(algo=1), ENOSUP),
    'tile-0': (dict(tile=0), ENOSUP),
    'tile-5': (dict(tile=5), ENOSUP),
    'odd-height': (dict(H=11), ENOSUP),
    'scale': (dict(scale=True), ENOSUP),
    'pool': (dict(pool=True), ENOSUP),
    'narrow-rows': (dict(ldzs=60), ENOSUP),
    'no-gamma': (dict(gamma=False), EINVAL),
    'no-z_sel': (dict(zsel=False), EINVAL),
}


@pytest.mark.parametrize('name', list(REFUSALS))
def test_sel_refusals_launch_nothing_and_write_nothing(name):
    kw, rc = REFUSALS[name]
    c = SEL_CASES['cin64-explicit-12x20']
    ops = operands(c, 'exact')
    r = launch(c, ops, 'dense', 'sel', **kw)
    assert r.rc == rc, r.rc
    assert r.names == [], r.names
    assert r.y.untouched() and r.zs.untouched() and not bool(r.stats.any())


# ---------------------------------------------------------------------------------------------------------------- one training step
def test_training_step_takes_the_producer_where_the_fused_kernel_runs(monkeypatch):
    """A narrow Darknet whose pooled blocks are wide enough for the fused kernel (32 channels in, 32 out), the fused kernel of tile 3 forced on every layer
    that accepts it: Y2_POOL_SEL=1 against =act - same loss and gradients within what two runs of =act differ by (statistics and weight gradients are
    accumulated with atomics; z, z_sel and the pooled activation are the same values on both paths), and under =1 no pooled block launches the pooling
    activation kernel.  "Within": the largest element difference of a tensor between two runs is itself a sample of that noise, so the bound is 4 x the
    measured difference plus a floor of 1e-6 x the tensor's rms (a few fp32 roundings) for the tensors two runs happen to agree on."""
    import configparser

    import _hip
    import model
    import model.yolo2
    from model import train_graph as tg
    from oracle import darknet as odark
    from oracle import loss as oloss
    from oracle import synth
    from oracle.make_golden import NARROW
    S, SB = 64, 2
    widths = dict(NARROW)
    widths['layers1.5'] = 8
    for k in ('layers1.0', 'layers1.2', 'layers1.5', 'layers1.6', 'layers1.9', 'layers1.10'):
        widths[k] = 32
    sd = odark.init_state_dict(5, 20, seed=0, channels=widths, head_scale=1 / 8.0)
    for k, v in sd.items():           # both signs and an exact zero in every BatchNorm weight
        if k.endswith('.bn.weight'):
            v[(torch.arange(v.numel()) // 2) % 2 == 1] *= -1.0
            v[1] = 0.0
    anchors = torch.from_numpy(synth.ANCHORS_VOC)
    x = synth.images(SB, S, seed=1)
    data = synth.norm_data(synth.labels(SB, S, 20, seed=2), S, S, S // 32, S // 32)
    monkeypatch.setattr(_hip, 'FORCE_ALGO', 'implicit3')
    L = _hip.lib()
    real, real_act = L.y2_conv_fwd_sel, L.y2_bn_act_fwd_sel

    def step(mode):
        monkeypatch.setattr(tg, 'POOL_SEL', mode)
        served, pooled = [], []
        monkeypatch.setattr(L, 'y2_conv_fwd_sel', lambda *a: served.append(real(*a)) or served[-1], raising=False)
        monkeypatch.setattr(L, 'y2_bn_act_fwd_sel', lambda *a: pooled.append(1) or real_act(*a), raising=False)          # the one launcher of bn_act_fwd_kernel<true, ., true>
        cfg = configparser.ConfigParser()
        cfg.read_dict({'batch_norm': {'enable': '1'}})
        dnn = model.yolo2.Darknet(model.ConfigChannels(cfg, sd), anchors, 20)
        dnn.load_state_dict(sd, strict=False)
        inf = model.Inference(cfg, dnn, anchors).to(dev()).train()
        out = {}

        def run():
            pred = model._inference(inf, x.to(dev()))
            loss, _ = model.loss(anchors, data, pred, 0.6)
            sum(loss[k] * oloss.HPARAM[k] for k in loss).backward()
            out['loss'] = {k: loss[k].item() for k in loss}
        names = kernels_of(run)
        monkeypatch.setattr(L, 'y2_conv_fwd_sel', real, raising=False)
        monkeypatch.setattr(L, 'y2_bn_act_fwd_sel', real_act, raising=False)
        names = [n for n in names if n.startswith(('bn_act_fwd', 'wino_fused3'))] + ['pooled-sel'] * len(pooled)
        grads = {k: p.grad.detach().clone() for k, p in inf.dnn.named_parameters() if p.grad is not None}
        return out['loss'], grads, names, served

    la, ga, na, sa = step('act')
    lb, gb, nb, sb = step('act')
    l1, g1, n1, s1 = step(True)
    assert sa == [] and s1 == [OK, OK, OK], (sa, s1)          # layers1.2, .6, .10: asked and served
    # the library's launch hooks name a kernel without its template arguments: the instantiation <true, ., true> is told by its only launcher, y2_bn_act_fwd_sel
    count = lambda names, what: sum(n.startswith(what) for n in names)
    print('act:', {w: count(na, w) for w in ('pooled-sel', 'bn_act_fwd_kernel', 'wino_fused3_kernel')}, ' 1:', {w: count(n1, w) for w in ('pooled-sel', 'bn_act_fwd_kernel', 'wino_fused3_kernel')})
    assert count(na, 'pooled-sel') == 4 and count(n1, 'pooled-sel') == 0          # =act: layers1.0, .2, .6, .10; =1: conv0's producer and this one
    assert count(na, 'bn_act_fwd_kernel') == count(n1, 'bn_act_fwd_kernel') and count(na, 'wino_fused3_kernel') == count(n1, 'wino_fused3_kernel') >= 3
    for k in la:
        spread = abs(la[k] - lb[k])
        assert abs(l1[k] - la[k]) <= 4 * spread + 1e-6 * abs(la[k]), (k, l1[k], la[k], spread)
    for k in ga:
        rms = ga[k].double().pow(2).mean().sqrt().item()
        spread = (ga[k].double() - gb[k].double()).abs().max().item()
        d = (g1[k].double() - ga[k].double()).abs().max().item()
        assert d <= 4 * spread + 1e-6 * rms, (k, d, spread, rms)
