"""GPU parity tests of y2_bn_act_bwd_wino6 (csrc/train.hip: BatchNorm / LeakyReLU backward fused with both 4x4-tile Winograd transforms of the gradient it
forms) and of its two consumers - y2_conv_fwd with Y2_ALGO_WINOGRAD_F43_PRE (algo 7: the data gradient from V6) and y2_wino_wgrad_ex with bit 2 of
native_layout (modes 6 / 7: the weight gradient from M6) - one dispatch path at a time.  tests/bnwino6_cases.py holds the case table and the mirror of
the dispatch, tests/test_bnwino6_cases.py proves on the CPU what the table reaches and that the fp64 statement of V6 / M6 used here reproduces the
gradients of conv2d.

Ground rules (those of tests/test_gpu_streaming.py): inputs are drawn in fp32 from a seeded generator and upcast to fp64 for the reference, so kernel and
reference see bit-identical inputs; the reference is torch-CPU fp64 autograd of leaky_relu(batch_norm(z)) under the upstream gradient dy (dz is z.grad,
never the kernel's formula restated) and of conv2d; z, dy and x live in channel windows of NaN-filled buffers; every destination sits between -7.0
sentinels; dz, V6 and M6 are pre-filled with NaN, so a pixel or tile that is not written surfaces in every consumer."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

if __name__ == '__main__':          # the child process of test_per_image_grid_in_a_fresh_process: what conftest.py does for the suite
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (os.path.join(_ROOT, 'tests'), os.path.join(_ROOT, 'yolo2-pytorch_amd'), _ROOT):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import bnwino6_cases as bc
from test_gpu_wgrad import GUARD, NAN, SENT, deterministic, dev, kernels_of, nhwc, randn32, rel

pytestmark = pytest.mark.gpu
TOL = 2e-5                      # the project's bound (tests/test_gpu_train.py)
TOL_WINO = 4 * TOL              # both Winograd forms (ibid.)
TOL_DZ = 5e-5                   # dz (tests/test_gpu_streaming.py)
EPS32 = float(torch.finfo(torch.float32).eps)
BN_EPS = 1e-5


class Window(object):
    """Rows of ld floats between two guards, all `fill`; channels off .. off + C of every row are the window (`inside`: a tensor [..., C] or a number).
    ptr points at row 0, channel 0 (the callee adds its own offset) - or, with ptr_at_window, at the window's first element."""

    def __init__(self, prefix, C, ld, off, fill, inside, ptr_at_window=False):
        rows = int(np.prod(prefix))
        assert ld >= off + C
        flat = torch.full((GUARD + rows * ld + GUARD,), fill, dtype=torch.float32)
        body = flat[GUARD:GUARD + rows * ld].view(rows, ld)
        if isinstance(inside, torch.Tensor):
            body[:, off:off + C] = inside.reshape(rows, C)
        else:
            body[:, off:off + C] = inside
        self.buf = flat.to(dev())
        self.ld, self.off, self.C, self.rows, self.fill, self.prefix = ld, off, C, rows, fill, tuple(prefix)
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + (GUARD + (off if ptr_at_window else 0)) * 4)

    def body(self):
        return self.buf[GUARD:GUARD + self.rows * self.ld].view(self.rows, self.ld)

    def window(self):
        return self.body()[:, self.off:self.off + self.C].reshape(self.prefix + (self.C,))

    def guards_intact(self):
        b = self.body()
        parts = (self.buf[:GUARD], self.buf[GUARD + self.rows * self.ld:], b[:, :self.off], b[:, self.off + self.C:])
        return all(bool((torch.isnan(p) if self.fill != self.fill else p == self.fill).all()) for p in parts)


class Flat(object):
    """n floats holding `fill` between two guards of sentinels; off = 1 starts them one float off 16-byte alignment."""

    def __init__(self, n, fill, off=0):
        self.buf = torch.full((GUARD + off + n + GUARD,), SENT, dtype=torch.float32, device=dev())
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.t = self.buf[self.lo:self.hi]
        self.t.fill_(fill)
        self.ptr = ctypes.c_void_p(self.t.data_ptr())
        assert self.t.data_ptr() % 16 == 4 * off

    def guards_intact(self):
        return bool((self.buf[:self.lo] == SENT).all()) and bool((self.buf[self.hi:] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())


# ================================================================================================ the reference
@functools.lru_cache(maxsize=None)
def reference(name, regime='randn', tall_allowed=True):
    """Everything the tests of one case compare with, computed once on the CPU and left unchanged: the inputs (fp32), fp64 autograd's dz, the sums and
    the size of their summands, V6 / M6 of that dz by the fp64 layout contract, the error of the same chain in torch-CPU fp32 (the floor), and for
    the consumers x, w and fp64 autograd's x.grad / w.grad of conv2d under dz."""
    c = bc.CASES[name]
    r = bc.route(c, tall_allowed)
    B, H, W, C = c.B, c.H, c.W, c.C
    g = torch.Generator().manual_seed(sum(map(ord, name)) * 7 + (1 if regime != 'randn' else 0))
    z = randn32(g, B, C, H, W)
    dy = randn32(g, B, C, H, W)
    if regime == 'mean-positive':               # the operands of the MEANPOS_* tables (tests/wgrad_cases.py): a gradient with a common sign on a positive mean
        z = z * 0.5 + 1.0
        dy = dy * 0.1 + 0.05
    if c.has_bn:
        sign = torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)     # a third of the channels scale negatively: yv > 0 and zv > mean disagree
        gamma = ((torch.rand(C, generator=g, dtype=torch.float32) + 0.5) * sign).double()
    else:
        gamma = torch.ones(C, dtype=torch.float64)
    beta = (randn32(g, C) * 0.3).double() if c.affine else torch.zeros(C, dtype=torch.float64)
    rm = (randn32(g, C) * 0.3).double()
    rv = (torch.rand(C, generator=g, dtype=torch.float32) + 0.5).double()

    def bn(zz, ga, be):
        k = dict(dtype=zz.dtype)
        if c.has_bn == 1:
            return F.batch_norm(zz, None, None, ga.to(**k), be.to(**k), True, 0.0, BN_EPS)
        if c.has_bn == 2:
            return F.batch_norm(zz, rm.to(**k), rv.to(**k), ga.to(**k), be.to(**k), False, 0.0, BN_EPS)
        return zz * ga.to(**k).view(1, -1, 1, 1) + be.to(**k).view(1, -1, 1, 1)

    # LeakyReLU's derivative jumps at 0: inputs whose pre-activation is within rounding of 0 are moved, so that fp32 and fp64 take the same side
    with torch.no_grad():
        for _ in range(8):
            pre = bn(z.double(), gamma, beta)
            if pre.abs().min().item() >= 1e-3:
                break
            z = torch.where(pre.abs() < 1e-3, z + 0.5, z)
        assert pre.abs().min().item() > 1e-4, 'test input: a pre-activation sits on the LeakyReLU kink'
    z64 = z.double().requires_grad_(True)
    ga, be = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    u = bn(z64, ga, be)
    u.retain_grad()
    (F.leaky_relu(u, c.slope) * dy.double()).sum().backward()
    z32 = z.clone().requires_grad_(True)
    (F.leaky_relu(bn(z32, gamma, beta), c.slope) * dy).sum().backward()
    with torch.no_grad():
        if c.has_bn == 1:
            _, mean, invstd = torch.native_batch_norm(z.double(), gamma, beta, None, None, True, 0.0, BN_EPS)
        elif c.has_bn == 2:
            mean, invstd = rm, 1.0 / torch.sqrt(rv + BN_EPS)
        else:
            mean, invstd = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
        zhat = (z.double() - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)
        abs1, abs2 = u.grad.abs().sum((0, 2, 3)), (u.grad * zhat).abs().sum((0, 2, 3))       # only the SIZE of the summation bound comes from these
    dz64 = nhwc(z64.grad)
    v6, m6 = map(torch.from_numpy, bc.v6_m6_reference(dz64.numpy(), r))
    v6f, m6f = map(torch.from_numpy, bc.v6_m6_reference(nhwc(z32.grad).numpy(), r, np.float32))
    ref = dict(c=c, r=r, z=z, dy=dy, gamma=gamma.float(), mean=mean.float(), invstd=invstd.float(), scale=(gamma * invstd).float(),
               shift=(beta - mean * gamma * invstd).float(), dz=dz64, dbeta=be.grad, dgamma=ga.grad, abs1=abs1, abs2=abs2,
               v6=v6, m6=m6, floor_v6=rel(v6f, v6), floor_m6=rel(m6f, m6), floor_dz=rel(nhwc(z32.grad), dz64),
               zeros=tuple(torch.from_numpy(m) for m in bc.structural_zeros(B, H, W, r)))
    if c.cin:
        x = randn32(g, B, c.cin, H, W)
        if regime == 'mean-positive':
            x = F.leaky_relu(x + 1, 0.1)
        w = randn32(g, C, c.cin, 3, 3) * 0.1        # forward weight [C][cin]: its data gradient maps C -> cin channels
        x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
        F.conv2d(x64, w64, padding=1).backward(z64.grad)
        x32, w32 = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        F.conv2d(x32, w32, padding=1).backward(z32.grad)
        ref.update(x=x, w=w, dx=nhwc(x64.grad), dw=w64.grad, floor_dx=rel(nhwc(x32.grad), nhwc(x64.grad)), floor_dw=rel(w32.grad, w64.grad))
    return ref


# ================================================================================================ one call
class Run(object):
    pass


def fused(ref, expect=bc.OK, **override):
    """One y2_bn_act_bwd_wino6 call on fresh buffers.  `override` replaces arguments for the refusal tests (ldz, ldf, ldd, mean, drop = both operands NULL)."""
    import _hip
    L, d = _hip.lib(), dev()
    c, r = ref['c'], ref['r']
    B, H, W, C = c.B, c.H, c.W, c.C
    ldz, ldf, ldd = bc.strides(c)
    o = Run()
    o.z = Window((B, H, W), C, ldz, 0, NAN, nhwc(ref['z']))
    o.dy = Window((B, H, W), C, ldf, c.foff, NAN, nhwc(ref['dy']))
    o.dz = Window((B, H, W), C, ldd, 0, SENT, NAN) if c.dz != 'null' else None
    n = 36 * r.T * C
    o.v6 = Flat(n, NAN, c.park_off if c.out != 'm6' else 0) if c.out in ('v6', 'both') else None
    o.m6 = Flat(n, NAN, c.park_off if c.out == 'm6' else 0) if c.out in ('m6', 'both') else None
    if expect != bc.OK:             # a refused call must leave everything as it was: all sentinels
        for f in (o.v6, o.m6):
            if f is not None:
                f.t.fill_(SENT)
        if o.dz is not None:
            o.dz.buf.fill_(SENT)
    o.base = 0.0 if c.has_bn == 1 else 3.0      # (with batch statistics pass 2 reads the sums as this call's own: they start at zero)
    o.sums = torch.full((2 * C + 4,), SENT, dtype=torch.float64, device=d)
    if expect == bc.OK:
        o.sums[:2 * C] = o.base
    o.held = {k: ref[k].to(d) for k in ('mean', 'invstd', 'gamma', 'scale', 'shift')}
    bnp = [_hip.ptr(o.held[k]) if c.has_bn else None for k in ('mean', 'invstd', 'gamma')]
    if 'mean' in override:
        bnp[0] = override['mean']
    sc, sh = (_hip.ptr(o.held['scale']), _hip.ptr(o.held['shift'])) if c.affine else (None, None)
    drop = override.get('drop', False)
    before = (o.z.buf.clone(), o.dy.buf.clone())
    rc = []
    o.names = kernels_of(lambda: rc.append(L.y2_bn_act_bwd_wino6(
        o.z.ptr, sc, sh, *bnp, c.slope, o.dy.ptr, override.get('ldf', ldf), c.foff, _hip.ptr(o.sums),
        o.v6.ptr if o.v6 is not None and not drop else None, o.m6.ptr if o.m6 is not None and not drop else None,
        o.dz.ptr if o.dz is not None else None, override.get('ldd', ldd), B, H, W, C, override.get('ldz', ldz), c.has_bn, _hip.stream())))
    assert rc == [expect], rc
    # torch.equal treats NaN as unequal: compare the bits
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip((o.z.buf, o.dy.buf), before)), 'an input buffer was written'
    return o


def check_fused(ref, o, label):
    """Sums, dz, V6, M6 and the launch list of one call; prints every figure before it asserts."""
    c, r = ref['c'], ref['r']
    C = c.C
    K = r.items + 256
    want = ['bn_act_bwd_kernel'] + (['bn_bwd_block_reduce_kernel'] if r.sums.startswith('parked') else []) + ['bn_bwd_wino6_kernel']
    assert o.names == want, (r.sums, o.names)
    assert bool((o.sums[2 * C:] == SENT).all()), 'sums written past 2C'
    sums = o.sums[:2 * C].cpu() - o.base
    e1, e2 = (sums[:C] - ref['dbeta']).abs(), (sums[C:] - ref['dgamma']).abs()
    b1, b2 = K * EPS32 * ref['abs1'], K * EPS32 * ref['abs2']
    line = '%s [%s %s %s]: sums %.3g / %.3g of K * eps32 * sum|.|, K = %d' % (label, r.form, r.pass1, r.sums, (e1 / b1).max().item(), (e2 / b2).max().item(), K)
    err = {}
    if o.dz is not None:
        err['dz'] = rel(o.dz.window(), ref['dz'])
        line += '; dz %.3g (fp32 floor %.3g)' % (err['dz'], ref['floor_dz'])
    for key, f in (('v6', o.v6), ('m6', o.m6)):
        if f is not None:
            err[key] = rel(f.t.view(36, r.T, C), ref[key])
            bound = max(TOL, 4 * ref['floor_' + key])
            line += '; %s %.3g (fp32 floor %.3g, bound %.3g)' % (key.upper(), err[key], ref['floor_' + key], bound)
    print(line)
    assert bool((e1 <= b1).all()), 'sum g outside K * eps32 * sum |g|: worst %.3g x the bound' % (e1 / b1).max().item()
    assert bool((e2 <= b2).all()), 'sum g*zhat outside K * eps32 * sum |g*zhat|: worst %.3g x the bound' % (e2 / b2).max().item()
    if o.dz is not None:
        assert o.dz.guards_intact(), 'dz written outside its channel window'
        assert bool(torch.isfinite(o.dz.window()).all()), 'a pixel of dz was not written (or depends on memory outside the windows)'
        assert err['dz'] <= TOL_DZ, err['dz']
    for key, f, zeros in (('v6', o.v6, ref['zeros'][0]), ('m6', o.m6, ref['zeros'][1])):
        if f is None:
            continue
        assert f.guards_intact(), key + ' written outside [36][T][C]'
        got = f.t.view(36, r.T, C).cpu()
        assert bool(torch.isfinite(got).all()), 'a tile of %s was not written (or depends on memory outside the windows)' % key
        assert err[key] <= max(TOL, 4 * ref['floor_' + key]), (key, err[key], ref['floor_' + key])
        assert bool((got[zeros] == 0).all()), key + ': not zero where no pixel of an image contributes'
    assert o.z.guards_intact() and o.dy.guards_intact()
    return err


# ================================================================================================ the consumers
def data_gradient(ref, v6):
    """y2_conv_fwd, algo 7, on V6 with U6 = y2_wino6_weight(y2_pack_weight mode 1 of w) -> (dx window [B, H, W, cin], launch list)."""
    import _hip
    L, d = _hip.lib(), dev()
    c = ref['c']
    w = ref['w'].to(d).contiguous()
    wd = torch.empty(w.numel(), device=d)
    _hip.check(L.y2_pack_weight(_hip.ptr(w), _hip.ptr(wd), c.C, c.cin, 3, 1, _hip.stream()), 'y2_pack_weight')
    u6 = _hip.wino6_weight(wd, c.cin, c.C)
    dx = Window((c.B, c.H, c.W), c.cin, c.cin + 8, 4, SENT, NAN)
    p = _hip.ConvParams()
    p.x, p.w, p.y = v6.ptr.value, u6.data_ptr(), dx.ptr.value
    p.B, p.H, p.W, p.Cin, p.ldx, p.Cout, p.ksize, p.ldy, p.coff, p.slope, p.algo, p.tile = c.B, c.H, c.W, c.C, c.C, c.cin, 3, dx.ld, dx.off, 1.0, 7, 0
    need = L.y2_conv_fwd_workspace_bytes(ctypes.byref(p))
    assert need > 0
    ws = Flat(need // 4, NAN)                   # exactly what the library asks for, poisoned
    p.workspace, p.workspace_bytes = ws.ptr.value, need
    rc = []
    names = kernels_of(lambda: rc.append(L.y2_conv_fwd(ctypes.byref(p), _hip.stream())))
    assert rc == [bc.OK]
    assert dx.guards_intact() and ws.guards_intact()
    return dx.window(), names


def weight_gradient(ref, m6, mode, x=None, expect=bc.OK):
    """y2_wino_wgrad_ex, mode 6 (packed) or 7 (native), on (x, M6) into a destination full of 5.0 with a NaN workspace -> (dW [C][cin][3][3], launch list)."""
    import _hip
    L = _hip.lib()
    c = ref['c']
    x = Window((c.B, c.H, c.W), c.cin, c.cin + 8, 4, NAN, nhwc(ref['x']), ptr_at_window=True) if x is None else x
    need = L.y2_wino_wgrad_workspace_bytes_ex(c.B, c.H, c.W, c.cin, c.C, mode)
    assert need > 0 and need % 16 == 0
    ws = Flat(need // 4, NAN)
    dw = Flat(c.C * c.cin * 9, 5.0 if expect == bc.OK else SENT)
    rc = []
    names = kernels_of(lambda: rc.append(L.y2_wino_wgrad_ex(x.ptr if x else None, m6.ptr, dw.ptr, c.B, c.H, c.W, c.cin, x.ld if x else c.cin, c.C, c.C, None,
                                                              ws.ptr, need, mode, _hip.stream())))
    assert rc == [expect], rc
    if expect != bc.OK:
        assert dw.untouched() and names == []
        return None, names
    assert dw.guards_intact() and ws.guards_intact()
    assert bool(torch.isfinite(dw.t).all()), 'the weight gradient depends on memory outside the operand windows (or on what the workspace held)'
    got = dw.t.view(c.C, c.cin, 3, 3) if mode & 1 else dw.t.view(c.C, 3, 3, c.cin).permute(0, 3, 1, 2)      # packed: [cout][tap][cin]
    return got, names


def check_consumers(ref, o, label, bound_dx=TOL_WINO, bound_dw=TOL_WINO):
    c = ref['c']
    if o.v6 is not None and not c.park_off:     # (algo 7 takes a 16-byte aligned operand: the misaligned-park case has no data-gradient consumer)
        dx, names = data_gradient(ref, o.v6)
        assert 'wino6_in_kernel' not in names and names[-1] == 'wino6_out_kernel', names
        assert bool(torch.isfinite(dx).all()), 'a tile of V6 was not written'
        e = rel(dx, ref['dx'])
        print('%s: data gradient from V6 %.3g (fp32 floor %.3g)' % (label, e, ref['floor_dx']))
        assert e <= bound_dx, e
    if o.m6 is not None:
        for mode in (6, 7):
            dw, names = weight_gradient(ref, o.m6, mode)
            assert 'wino6_in_kernel[dz]' not in names and 'wino6_in_kernel' in names and names[-1] == 'wino6_dw_kernel', names
            e = rel(dw, ref['dw'])
            print('%s: weight gradient from M6, mode %d: %.3g (fp32 floor %.3g)' % (label, mode, e, ref['floor_dw']))
            assert e <= bound_dw, (mode, e)


# ================================================================================================ the tests
@pytest.mark.parametrize('name', list(bc.CASES))
def test_sums_dz_and_both_transforms(name):
    """Every case of the table: sums within K * eps32 * sum |summand| (K = items per thread + 256), dz within 5e-5 x rms with every pixel written and the
    guards intact, V6 and M6 against the fp64 transforms of autograd's dz within max(2e-5, 4 x the error of the same chain in torch-CPU fp32), exactly
    zero where no pixel contributes, and the launch list: bn_bwd_block_reduce_kernel exactly on the parked routes."""
    ref = reference(name)
    check_fused(ref, fused(ref), name)


CONSUMER_CASES = [n for n, c in bc.CASES.items() if c.cin]


@pytest.mark.parametrize('name', CONSUMER_CASES)
def test_gradients_from_the_transformed_operands(name):
    """y2_conv_fwd algo 7 on the V6 and y2_wino_wgrad_ex modes 6 / 7 on the M6 that the call wrote, against fp64 autograd of conv2d: 8e-5 x rms.  No
    wino6_in_kernel may run in the algo-7 call and no wino6_in_kernel[dz] in modes 6 / 7."""
    ref = reference(name)
    check_consumers(ref, fused(ref), name)


@pytest.mark.parametrize('name', bc.MEANPOS)
def test_mean_positive(name):
    """A gradient with a common sign on pre-activations of positive mean: the subtraction of the two means in pass 2 cancels.  V6 / M6 keep their
    max(2e-5, 4 x floor) rule; the gradients are held to max(8e-5, 4 x the error of torch-CPU fp32 autograd against the same fp64 reference)."""
    ref = reference(name, 'mean-positive')
    o = fused(ref)
    check_fused(ref, o, 'mean-positive ' + name)
    check_consumers(ref, o, 'mean-positive ' + name, max(TOL_WINO, 4 * ref['floor_dx']), max(TOL_WINO, 4 * ref['floor_dw']))


REFUSALS = {
    'both operands NULL': (dict(drop=True), bc.EINVAL),
    'ldz < C': (dict(ldz=15), bc.EINVAL),
    'ldf < foff + C': (dict(ldf=19), bc.EINVAL),
    'dz with ldd < C': (dict(ldd=15), bc.EINVAL),
    'has_bn = 1 without mean': (dict(mean=None), bc.EINVAL),
}


@pytest.mark.parametrize('what', list(REFUSALS))
def test_refusals_leave_every_buffer_untouched(what):
    override, rc = REFUSALS[what]
    ref = reference('b2-7x9-mosaic')            # C = 16, foff = 4, dense dz, batch statistics
    assert (ref['c'].C, ref['c'].foff, ref['c'].dz, ref['c'].has_bn) == (16, 4, 'dense', 1)
    o = fused(ref, expect=rc, **override)
    assert o.names == []
    assert o.v6.untouched() and o.m6.untouched() and bool((o.dz.buf == SENT).all()) and bool((o.sums == SENT).all())


def test_deterministic_mode_is_refused_with_nothing_written():
    ref = reference('b2-7x9-mosaic')
    with deterministic():
        o = fused(ref, expect=bc.ENOSUP)
    assert o.names == []
    assert o.v6.untouched() and o.m6.untouched() and bool((o.dz.buf == SENT).all()) and bool((o.sums == SENT).all())
    check_fused(ref, fused(ref), 'after deterministic mode')


def test_weight_gradient_refusals():
    """Bit 2 of native_layout without bit 1 (modes 4 and 5), and modes 6 / 7 without x: Y2_EINVAL, nothing launched, the destination untouched."""
    import _hip
    L = _hip.lib()
    ref = reference('b2-7x9-mosaic')
    c = ref['c']
    m6 = Flat(36 * ref['r'].T * c.C, 0.0)
    for mode in (4, 5):
        weight_gradient(ref, m6, mode, expect=bc.EINVAL)
    for mode in (6, 7):
        weight_gradient(ref, m6, mode, x=False, expect=bc.EINVAL)
        need = L.y2_wino_wgrad_workspace_bytes_ex(c.B, c.H, c.W, c.cin, c.C, mode)
        ws, dw, v = Flat(need // 4, NAN), Flat(c.C * c.cin * 9, SENT), Flat(36 * ref['r'].T * c.cin, 0.0)
        # ... nor does a transformed input stand in for x
        assert L.y2_wino_wgrad_ex(None, m6.ptr, dw.ptr, c.B, c.H, c.W, c.cin, c.cin, c.C, c.C, v.ptr, ws.ptr, need, mode, _hip.stream()) == bc.EINVAL
        torch.cuda.synchronize()
        assert dw.untouched()
    assert m6.guards_intact()


def run_child(name):
    """One case on the per-image grid: the process was started with Y2_WINO6_TALL=0, which the library reads once."""
    import _hip
    c = bc.CASES[name]
    assert os.environ.get('Y2_WINO6_TALL') == '0'
    assert bc.route(c).form != 'per-image'
    ref = reference(name, 'randn', False)
    assert ref['r'].form == 'per-image' and _hip.lib().y2_wino6_tiles(c.B, c.H, c.W) == ref['r'].T == c.B * ((c.H + 3) // 4) * ((c.W + 3) // 4)
    o = fused(ref)
    check_fused(ref, o, 'per-image ' + name)
    check_consumers(ref, o, 'per-image ' + name)
    print('child ok')


def test_per_image_grid_in_a_fresh_process():
    """Y2_WINO6_TALL=0 keeps the per-image grid for a batch that would take the mosaic.  The switch is read once per process, so the case runs in a
    child process started for it (this process keeps its GPU and its program)."""
    env = dict(os.environ, Y2_WINO6_TALL='0')
    out = subprocess.run([sys.executable, os.path.abspath(__file__), bc.CHILD], env=env, capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and 'child ok' in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


if __name__ == '__main__':
    run_child(sys.argv[1])
