"""GPU parity tests of the pre-activation kernels of csrc/dense.hip, one launch path at a time: the tables of tests/dense_cases.py (all sixteen
preact_gemm_kernel instantiations with a ragged last row tile, K that is no multiple of 4 in one slab and in several, every single reason for the
element-wise loader; the element-wise kernels at CV x POOL x channel blocks x steps per thread, under the grid cap, for every single reason for
the scalar path; y2_preact_bwd for every has_bn, writing and adding, and in deterministic mode), each case proved on the CPU to reach what it
names (tests/test_dense_cases.py).

Ground rules: the operands are drawn in fp32 from a seeded generator and upcast for the reference, which is torch-CPU fp64 (F.conv2d of the
pre-activated input, F.avg_pool2d, F.batch_norm / relu and their autograd) - never another run of the kernels.  Every operand, the filter and the
per-channel vectors of the loader included, is a window of a NaN-filled buffer (tests/test_gpu_dwconv.py Window) with its own pixel stride and
offset from a 16-byte boundary; destinations start as NaN, everything outside their channel window must keep its bits, the inputs must keep theirs.
Bounds: rel() <= 2e-5 forward, 8e-5 gradients and backward sums (rel = max |diff| / rms of the reference), the GEMM statistics within the bounds of
tests/test_gpu_densenet.py.  Every test prints its error and the worst of its kernel so far; the module prints the worst error per kernel at its end
(pytest -s, or -rP).

The backward's ReLU mask is discontinuous at pre == 0: the inputs are built so that the fp64 pre-activation is at least 1e-3 from zero at every
element (the few that are not are moved; asserted before the launch), and no element is left out of any comparison."""
import functools
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_cases as dn
from test_gpu_densenet import rel
from test_gpu_dwconv import NAN, OK, Window, dev, hip, rows, worst_errors
from test_gpu_wgrad import deterministic

pytestmark = pytest.mark.gpu
TOL_FWD, TOL_GRAD = 2e-5, 8e-5
EINVAL = -1
record, _report_worst = worst_errors({})
MARGIN = 1e-3                   # |pre-activation| of every element of the backward tests


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def signs(n, g):
    return (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()


def leaky(t, slope):
    return t if slope == 1.0 else F.leaky_relu(t, slope)


def preact(x, a, b, slope):
    t = x.double()
    if a is not None:
        t = t * a.double().view(1, -1, 1, 1)
    if b is not None:
        t = t + b.double().view(1, -1, 1, 1)
    return leaky(t, slope)


def vector(t, off=0):
    """A per-channel vector (or the filter) in a guarded window; None stays NULL."""
    return None if t is None else Window(1, t.numel(), t.numel(), off, t.reshape(1, -1).float())


def vptr(w):
    return None if w is None else w.ptr


# ------------------------------------------------------------------------------------------------ y2_preact_conv1x1_fwd
@functools.lru_cache(maxsize=None)
def gemm_operands(name):
    B, H, W, K, N, pool = dn.GEMM_CASES[name].shape
    g = gen('gemm', name)
    x, w = torch.randn(B, K, H, W, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    a, b = (torch.rand(K, generator=g) + 0.5) * signs(K, g), torch.randn(K, generator=g) * 0.5
    scale, shift = (torch.rand(N, generator=g) + 0.5) * signs(N, g), torch.randn(N, generator=g)
    return x, w, a, b, scale, shift


def gemm(name, form):
    c = dn.GEMM_CASES[name]
    B, H, W, K, N, pool = c.shape
    s = dn.pe_shape_ok(B, H, W, K, pool)
    x, w, a, b, scale, shift = gemm_operands(name)
    a, b, pre_slope, scale, shift, slope = {
        'plain': (None, None, 1.0, None, None, 1.0), 'affine-relu': (a, b, 0.0, scale, shift, 0.0), 'affine-slope0.1': (a, b, 0.1, scale, shift, 0.1),
        'scale-only': (a, b, 0.0, scale, None, 0.1), 'shift-only': (a, b, 0.0, None, shift, 0.0), 'null-pre': (None, None, 0.0, scale, shift, 0.1)}[form]
    xb = Window(s.Pin, K, K + c.xpad, c.off['x'], rows(x))
    yb = Window(s.Pout, N, c.ldy, 0, None, c.coff)
    wb, ab, bb = vector(w, c.off['w']), vector(a, c.off['pre_scale']), vector(b, c.off['pre_shift'])
    scb, shb = vector(scale), vector(shift)
    _hip = hip()
    stats = torch.zeros(_hip.STATS_REPL * 2 * N, dtype=torch.float64, device=dev())
    rc = _hip.lib().y2_preact_conv1x1_fwd(xb.ptr, wb.ptr, vptr(ab), vptr(bb), pre_slope, vptr(scb), vptr(shb), slope, yb.ptr, _hip.ptr(stats),
                                          B, H, W, K, xb.ld, N, yb.ld, c.coff, pool, _hip.stream())
    assert rc == OK
    torch.cuda.synchronize()
    raw = F.conv2d(preact(x, a, b, pre_slope), w.double().view(N, K, 1, 1))
    if pool:
        raw = F.avg_pool2d(raw, 2)                  # the reference order: convolution, then the pool
    ref = raw
    if scale is not None:
        ref = ref * scale.double().view(1, -1, 1, 1)
    if shift is not None:
        ref = ref + shift.double().view(1, -1, 1, 1)
    err = rel(yb.view(), rows(leaky(ref, slope)))
    record('preact_gemm_kernel', '%s %s' % (name, form), err)
    assert err <= TOL_FWD, err
    assert yb.outside_untouched()
    assert all(v is None or v.unchanged() for v in (xb, wb, ab, bb, scb, shb))
    copies = stats.view(_hip.STATS_REPL, 2, N).cpu()
    st = copies.sum(0)
    np.testing.assert_allclose(st[0].numpy(), raw.sum((0, 2, 3)).numpy(), rtol=1e-6, atol=1e-6 * raw.abs().sum().item() / N)
    np.testing.assert_allclose(st[1].numpy(), raw.pow(2).sum((0, 2, 3)).numpy(), rtol=1e-6)
    # row tile mb adds into copy mb mod Y2_STATS_REPL: below 32 row tiles - the mt1 cases - the copies in use tell their number and with it MT (the
    # mirror's, observed on the device); every mt2 case has 128 row tiles or more and fills all 32 copies with either tile, so that an mt2 case ran a
    # <2, *> kernel rests on the mirror being pinned to the source text (tests/test_dense_cases.py)
    assert int((copies[:, 1].sum(1) > 0).sum()) == min(dn.gemm_derive(c)[1].gm, _hip.STATS_REPL)


@pytest.mark.parametrize('name', list(dn.GEMM_CASES))
def test_preact_conv1x1(name):
    """Affine + LeakyReLU(0.1) in front and behind, with statistics, on every case."""
    gemm(name, 'affine-slope0.1')


@pytest.mark.parametrize('form', [f for f in dn.GEMM_FORMS if f != 'affine-slope0.1'])
@pytest.mark.parametrize('name', dn.GEMM_FORM_CASES)
def test_preact_conv1x1_forms(name, form):
    gemm(name, form)


# ------------------------------------------------------------------------------------------------ y2_preact_fwd
def preact_fwd(name, form):
    c = dn.FWD_CASES[name]
    B, C, H, W, pool = c.shape
    s = dn.pe_shape_ok(B, H, W, C, pool)
    g = gen('fwd', name)
    x = torch.randn(B, C, H, W, generator=g)
    a, b = (torch.rand(C, generator=g) + 0.5) * signs(C, g), torch.randn(C, generator=g) * 0.5
    a, b, slope = {'affine-relu': (a, b, 0.0), 'affine-slope0.1': (a, b, 0.1), 'null-pre-relu': (None, None, 0.0), 'scale-only': (a, None, 0.0),
                   'shift-only': (None, b, 0.1), 'identity': (None, None, 1.0)}[form]
    xb, ob = Window(s.Pin, C, dn.ld(c, 'x'), c.off['x'], rows(x)), Window(s.Pout, C, dn.ld(c, 'out'), c.off['out'])
    ab, bb = vector(a), vector(b)
    _hip = hip()
    rc = _hip.lib().y2_preact_fwd(xb.ptr, vptr(ab), vptr(bb), slope, ob.ptr, B, H, W, C, xb.ld, ob.ld, pool, _hip.stream())
    assert rc == OK
    torch.cuda.synchronize()
    ref = preact(x, a, b, slope)
    if pool:
        ref = F.avg_pool2d(ref, 2)
    err = rel(ob.view(), rows(ref))
    record('preact_fwd_kernel', '%s %s' % (name, form), err)
    assert err <= TOL_FWD, err
    assert ob.outside_untouched() and all(v is None or v.unchanged() for v in (xb, ab, bb))


@pytest.mark.parametrize('name', list(dn.FWD_CASES))
def test_preact_fwd(name):
    preact_fwd(name, 'affine-relu')


@pytest.mark.parametrize('form', [f for f in dn.FWD_FORMS if f != 'affine-relu'])
@pytest.mark.parametrize('name', dn.FWD_FORM_CASES)
def test_preact_fwd_forms(name, form):
    preact_fwd(name, form)


# ------------------------------------------------------------------------------------------------ y2_preact_bwd
class BwdRef(object):
    pass


@functools.lru_cache(maxsize=None)
def bwd_reference(name, has_bn):
    """Operands in fp32 and the fp64 autograd of (BatchNorm | frozen BatchNorm | nothing) -> ReLU [-> AvgPool2d(2)].  Read only."""
    B, C, H, W, pool = dn.BWD_CASES[name].shape
    g = gen('bwd', name, has_bn)
    x = torch.randn(B, C, H, W, generator=g) * 1.5 + 0.3
    gamma = ((torch.rand(C, generator=g) + 0.5) * signs(C, g)).double()
    beta = (torch.randn(C, generator=g) * 0.3).double()
    rmean, rvar = (torch.randn(C, generator=g) * 0.2).double(), (torch.rand(C, generator=g) + 0.5).double()
    v = lambda t: t.view(1, -1, 1, 1)          # noqa: E731

    def affine(x):
        xd = x.double()
        if has_bn == 1:
            mean, var = xd.mean((0, 2, 3)), xd.var((0, 2, 3), unbiased=False)
        elif has_bn == 2:
            mean, var = rmean, rvar
        else:
            return xd, None, None, None, None
        invstd = 1.0 / torch.sqrt(var + 1e-5)
        a = gamma * invstd
        return xd * v(a) + v(beta - mean * a), a, beta - mean * a, mean, invstd

    for _ in range(50):                          # move the few elements whose pre-activation is within 2 * MARGIN of zero away from it
        pre, a = affine(x)[:2]
        close = pre.abs() < 2 * MARGIN
        if not close.any():
            break
        step = torch.where(pre >= 0, 1.0, -1.0) * 8 * MARGIN / (v(a) if a is not None else 1.0)
        x = torch.where(close, (x.double() + step).float(), x)
    r = BwdRef()
    pre, a, b, mean, invstd = affine(x)
    r.min_pre = pre.abs().min().item()
    xd, gd, bd = x.double().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    if has_bn == 1:
        y = F.batch_norm(xd, None, None, gd, bd, True, 0.0, 1e-5)
    elif has_bn == 2:
        y = F.batch_norm(xd, rmean, rvar, gd, bd, False, 0.0, 1e-5)
    else:
        y = xd
    y = F.relu(y)
    if pool:
        y = F.avg_pool2d(y, 2)
    r.dA = torch.randn(y.shape, generator=g)
    y.backward(r.dA.double())
    r.x, r.dx = x, xd.grad
    r.sum_g, r.sum_gx = (bd.grad, gd.grad) if has_bn else (xd.grad.sum((0, 2, 3)), None)
    r.params = [None if t is None else t.float() for t in (a, b, mean, invstd, gamma if has_bn else None)]
    r.base = torch.randn(B * H * W, C, generator=g)
    return r


def launch_bwd(c, r, xb, dab, dxb, sums, has_bn, accumulate, vecs):
    B, C, H, W, pool = c.shape
    _hip = hip()
    a, b, mean, invstd, gamma = [vptr(t) for t in vecs]
    return _hip.lib().y2_preact_bwd(xb.ptr, a, b, 0.0, mean, invstd, gamma, dab.ptr, dab.ld, _hip.ptr(sums), dxb.ptr, dxb.ld, accumulate,
                                    B, H, W, C, xb.ld, pool, has_bn, _hip.stream())


def bwd_windows(c, r):
    B, C, H, W, pool = c.shape
    s = dn.pe_shape_ok(B, H, W, C, pool)
    xb = Window(s.Pin, C, dn.ld(c, 'x'), c.off['x'], rows(r.x))
    dab = Window(s.Pout, C, dn.ld(c, 'dA'), c.off['dA'], rows(r.dA))
    return s, xb, dab, [vector(t) for t in r.params]


def check_sums(name, has_bn, sums, r, what):
    C = sums.numel() // 2
    s = sums.cpu()
    e1 = rel(s[:C], r.sum_g)
    e2 = rel(s[C:], r.sum_gx) if has_bn else 0.0
    record('preact_bwd_sums_kernel sum g', '%s has_bn=%d %s' % (name, has_bn, what), e1)
    if has_bn:
        record('preact_bwd_sums_kernel sum g xhat', '%s has_bn=%d %s' % (name, has_bn, what), e2)
    assert e1 <= TOL_GRAD and e2 <= TOL_GRAD, (e1, e2)


@pytest.mark.parametrize('has_bn', dn.HAS_BN)
@pytest.mark.parametrize('name', list(dn.BWD_CASES))
def test_preact_bwd(name, has_bn):
    c = dn.BWD_CASES[name]
    C = c.shape[1]
    r = bwd_reference(name, has_bn)
    assert r.min_pre >= MARGIN                      # no element sits on the ReLU's kink
    s, xb, dab, vecs = bwd_windows(c, r)
    got = {}
    for accumulate in dn.ACCUMULATE:
        dxb = Window(s.Pin, C, dn.ld(c, 'dx'), c.off['dx'], r.base if accumulate else None)
        sums = torch.zeros(2 * C, dtype=torch.float64, device=dev())
        assert launch_bwd(c, r, xb, dab, dxb, sums, has_bn, accumulate, vecs) == OK
        torch.cuda.synchronize()
        got[accumulate] = dxb.view().double().cpu()
        delta = got[accumulate] - r.base.double() if accumulate else got[accumulate]
        err = rel(delta, rows(r.dx))
        record('preact_bwd_dx_kernel', '%s has_bn=%d accumulate=%d' % (name, has_bn, accumulate), err)
        assert err <= TOL_GRAD, err
        check_sums(name, has_bn, sums, r, 'accumulate=%d' % accumulate)
        assert dxb.outside_untouched()
    assert rel(got[1], r.base.double() + got[0]) <= 1e-6                    # accumulate = 1 equals write + add
    assert xb.unchanged() and dab.unchanged() and all(t is None or t.unchanged() for t in vecs)


@pytest.mark.parametrize('name', dn.DET_CASES)
def test_preact_bwd_deterministic(name):
    """Block partial sums in fp32 through y2_det_reduce_f32: the sums are WRITTEN (they start as NaN here), held to the same fp64 reference, and a
    second run gives the same bits."""
    c = dn.BWD_CASES[name]
    C, has_bn = c.shape[1], 1
    r = bwd_reference(name, has_bn)
    assert r.min_pre >= MARGIN
    s, xb, dab, vecs = bwd_windows(c, r)
    runs = []
    with deterministic():
        for _ in range(2):
            dxb = Window(s.Pin, C, dn.ld(c, 'dx'), c.off['dx'])
            sums = torch.full((2 * C,), NAN, dtype=torch.float64, device=dev())
            assert launch_bwd(c, r, xb, dab, dxb, sums, has_bn, 0, vecs) == OK
            torch.cuda.synchronize()
            runs.append((sums, dxb))
    (s1, d1), (s2, d2) = runs
    assert torch.equal(s1, s2) and torch.equal(d1.buf.view(torch.int32), d2.buf.view(torch.int32))
    err = rel(d1.view(), rows(r.dx))
    record('preact_bwd_dx_kernel', '%s deterministic' % name, err)
    assert err <= TOL_GRAD, err
    check_sums(name, has_bn, s1, r, 'deterministic')
    assert d1.outside_untouched() and xb.unchanged() and dab.unchanged()


def test_preact_bwd_refuses_a_deterministic_workspace_one_byte_short():
    B, C, H, W, pool = dn.DET_TOO_SMALL
    P = B * H * W
    need = dn.det_need_bytes(P, C, 4)
    assert need > dn.DET_MIN_BYTES and need % 16 == 0
    _hip = hip()
    L = _hip.lib()
    x, dA = torch.ones(P * C, device=dev()), torch.ones(P * C, device=dev())
    dxb = Window(P, C, C)
    sums = torch.full((2 * C,), -7.0, dtype=torch.float64, device=dev())
    ws = torch.empty(need // 4, dtype=torch.float32, device=dev())
    call = lambda: L.y2_preact_bwd(_hip.ptr(x), None, None, 0.0, None, None, None, _hip.ptr(dA), C, _hip.ptr(sums), dxb.ptr, C, 0,          # noqa: E731
                                   B, H, W, C, C, pool, 0, _hip.stream())
    try:
        _hip.check(L.y2_set_deterministic(1, _hip.ptr(ws), need - 1), 'y2_set_deterministic')
        assert call() == EINVAL
        torch.cuda.synchronize()
        assert dxb.unchanged() and bool((sums == -7.0).all())
        _hip.check(L.y2_set_deterministic(1, _hip.ptr(ws), need), 'y2_set_deterministic')
        assert call() == OK                          # exactly the mirror's need
        torch.cuda.synchronize()
    finally:
        _hip.set_deterministic(False)
        torch.cuda.synchronize()
    assert bool((sums[:C] == float(P)).all()) and bool((dxb.view() == 1.0).all()) and dxb.outside_untouched()


def test_refusals_leave_every_buffer_alone():
    """Every refusal of the three entry points on real buffers (a check that regressed would launch inside them): bad sizes, an odd map with pool = 1, a
    pixel stride below the channel count, N = 0, coff < 0, ldy < coff + N, a missing operand, has_bn out of range or without its vectors."""
    from test_dense_cases import BAD_PLACEMENTS, BAD_SHAPES
    B, H, W, C = 2, 6, 8, 5
    n = B * H * W
    g = gen('refusals')
    xb, ab = Window(n, C, C, 0, torch.randn(n, C, generator=g)), Window(n, C, C, 0, torch.randn(n, C, generator=g))
    wb, vb = vector(torch.randn(8, C, generator=g)), vector(torch.rand(C, generator=g) + 0.5)
    yb, db = Window(n, 8, 8), Window(n, C, C)
    sums = torch.full((2 * C,), -7.0, dtype=torch.float64, device=dev())
    _hip = hip()
    L, st = _hip.lib(), _hip.stream()

    def gemm(b, h, w, k, ldx, N, ldy, coff, pool, x=xb.ptr, wp=wb.ptr, y=yb.ptr):
        return L.y2_preact_conv1x1_fwd(x, wp, None, None, 0.0, None, None, 1.0, y, None, b, h, w, k, ldx, N, ldy, coff, pool, st)

    def fwd(b, h, w, c, ldx, ldo, pool, x=xb.ptr, out=db.ptr):
        return L.y2_preact_fwd(x, None, None, 0.0, out, b, h, w, c, ldx, ldo, pool, st)

    def bwd(b, h, w, c, ldx, ldda, lddx, pool, has_bn=0, stat=None, x=xb.ptr, dA=ab.ptr, sm=_hip.ptr(sums), dx=db.ptr):
        return L.y2_preact_bwd(x, None, None, 0.0, stat, stat, stat, dA, ldda, sm, dx, lddx, 0, b, h, w, c, ldx, pool, has_bn, st)

    for bad in BAD_SHAPES:
        if max(bad) > 100:
            continue                                    # (no real buffer holds 2^32 pixels: that refusal is checked from the source text)
        b, h, w, c, pool = bad
        assert gemm(b, h, w, c, c, 4, 4, 0, pool) == EINVAL, bad
        assert fwd(b, h, w, c, c, c, pool) == EINVAL, bad
        assert bwd(b, h, w, c, c, c, c, pool) == EINVAL, bad
    for ldx, N, ldy, coff in BAD_PLACEMENTS:
        assert gemm(B, H, W, C, ldx, N, ldy, coff, 1) == EINVAL, (ldx, N, ldy, coff)
    for k in ('x', 'wp', 'y'):
        assert gemm(B, H, W, C, C, 4, 4, 0, 1, **{k: None}) == EINVAL, k
    assert fwd(B, H, W, C, C - 1, C, 0) == EINVAL and fwd(B, H, W, C, C, C - 1, 0) == EINVAL
    assert fwd(B, H, W, C, C, C, 0, x=None) == EINVAL and fwd(B, H, W, C, C, C, 0, out=None) == EINVAL
    assert bwd(B, H, W, C, C - 1, C, C, 0) == EINVAL and bwd(B, H, W, C, C, C - 1, C, 0) == EINVAL and bwd(B, H, W, C, C, C, C - 1, 0) == EINVAL
    for k in ('x', 'dA', 'sm', 'dx'):
        assert bwd(B, H, W, C, C, C, C, 0, **{k: None}) == EINVAL, k
    assert bwd(B, H, W, C, C, C, C, 0, has_bn=3, stat=vb.ptr) == EINVAL and bwd(B, H, W, C, C, C, C, 0, has_bn=-1, stat=vb.ptr) == EINVAL
    assert bwd(B, H, W, C, C, C, C, 0, has_bn=1) == EINVAL and bwd(B, H, W, C, C, C, C, 0, has_bn=2) == EINVAL
    torch.cuda.synchronize()
    assert all(t.unchanged() for t in (xb, ab, wb, vb, yb, db)) and bool((sums == -7.0).all())
