"""GPU parity tests of the depthwise kernels of csrc/dwconv.hip, one launch path at a time: the table of tests/dw_cases.py (vector width x
channel blocks x steps per thread, the grid cap, every single reason for the scalar path, both strides, odd / even / 1x1 maps), each case
proved on the CPU to reach what it names (tests/test_dw_cases.py).

Ground rules: the operands are drawn in fp32 from a seeded generator and upcast for the reference, which is torch-CPU fp64 F.conv2d(groups=C) and
its autograd - never another run of the kernels.  Every operand is a window [pixels][ld] of a NaN-filled buffer with its own pixel stride (no two
operands of an entry point share one), its own offset from a 16-byte boundary and GUARD NaNs in front and behind; destinations start as NaN, and
everything but the C channels of each pixel - pad channels, guards - must keep its bits; the inputs must keep theirs.  Bounds: rel() <= 2e-5 for
the forward, 8e-5 for the gradients (rel = max |diff| / rms of the reference, README), the statistics within the bounds of
tests/test_gpu_mobilenet.py.  Every test prints its error and the worst of its kernel so far; the module prints the worst error per kernel at
its end (pytest -s, or -rP)."""
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dw_cases as dc
from test_gpu_mobilenet import rel

pytestmark = pytest.mark.gpu
TOL_FWD, TOL_GRAD = 2e-5, 8e-5
GUARD = 64                      # floats in front of and behind every window (256 B: keeps the 16-B phase of the base)
NAN = float('nan')
OK, EINVAL, EALIGN = 0, -1, -2


def dev():
    return torch.device('cuda', 0)


def hip():
    import _hip
    return _hip


def worst_errors(table):
    """(record, fixture): record(kernel, what, err) prints the error and keeps the running maximum per kernel; the module-scoped autouse fixture prints the
    maxima when the module's last test is done."""
    def record(kernel, what, err):
        table[kernel] = max(table.get(kernel, 0.0), err)
        print('%s %s: %.2e (worst %s so far %.2e)' % (kernel, what, err, kernel, table[kernel]))

    @pytest.fixture(scope='module', autouse=True)
    def report():
        table.clear()
        yield
        for kernel in sorted(table):
            print('WORST %s: %.2e' % (kernel, table[kernel]))
    return record, report


record, _report_worst = worst_errors({})


def rows(t):
    """[B,C,H,W] -> [B*H*W, C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


class Window(object):
    """[pixels][ld] floats with the data in channels [coff, coff + C) of every pixel, `off` floats past a 16-byte boundary, inside a NaN-filled buffer
    with GUARD NaNs in front and behind; `ptr` is the first pixel's channel 0.  data = None: a destination (all NaN)."""

    def __init__(self, pixels, C, ld, off=0, data=None, coff=0):
        assert coff + C <= ld
        self.pixels, self.C, self.ld, self.lo, self.coff = pixels, C, ld, GUARD + off, coff
        host = torch.full((self.lo + pixels * ld + GUARD,), NAN, dtype=torch.float32)
        if data is not None:
            assert data.shape == (pixels, C) and data.dtype == torch.float32
            host[self.lo:self.lo + pixels * ld].view(pixels, ld)[:, coff:coff + C] = data
        self.buf = host.to(dev())
        self.before = self.buf.clone()
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 4 * self.lo)

    def view(self, buf=None):
        buf = self.buf if buf is None else buf
        return buf[self.lo:self.lo + self.pixels * self.ld].view(self.pixels, self.ld)[:, self.coff:self.coff + self.C]

    def unchanged(self):
        return torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32))

    def outside_untouched(self):
        """Bit for bit: the guards and the channels outside [coff, coff + C) of every pixel."""
        a, b = self.buf.view(torch.int32).clone(), self.before.view(torch.int32).clone()
        self.view(a).zero_()
        self.view(b).zero_()
        return torch.equal(a, b)


def param(t):
    """A small read-only parameter on the device with its before-image."""
    d = t.to(dev(), torch.float32).contiguous()
    return d, d.clone()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(x, w, dz in fp32; raw forward output, dx, dw in fp64 by torch-CPU autograd).  Shared by every test of a case: read only."""
    B, C, H, W, stride = dc.CASES[name].shape
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    x, w = torch.randn(B, C, H, W, generator=g), torch.randn(C, 1, 3, 3, generator=g)
    xd, wd = x.double().requires_grad_(), w.double().requires_grad_()
    raw = F.conv2d(xd, wd, stride=stride, padding=1, groups=C)
    dz = torch.randn(raw.shape, generator=g)
    raw.backward(dz.double())
    return x, w, dz, raw.detach(), xd.grad, wd.grad


def geometry(name):
    c = dc.CASES[name]
    B, C, H, W, stride = c.shape
    return c, B, C, H, W, stride, dc.dw_shape_ok(B, H, W, C, stride)


def window(c, s, operand, data=None):
    pixels = s.Pin if operand in ('x', 'dx') else s.Pout
    return Window(pixels, c.shape[1], dc.ld(c, operand), c.off[operand], None if data is None else rows(data))


def forward(name, form):
    c, B, C, H, W, stride, s = geometry(name)
    x, w, _, raw, _, _ = reference(name)
    g = torch.Generator().manual_seed(zlib.crc32((name + form).encode()))
    scale = (torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
    shift = torch.randn(C, generator=g)
    scale, shift, slope = {'plain': (None, None, 1.0), 'affine-relu': (scale, shift, 0.0), 'affine-slope0.1': (scale, shift, 0.1),
                           'scale-only': (scale, None, 0.1), 'shift-only': (None, shift, 0.0)}[form]
    xb, yb = window(c, s, 'x', x), window(c, s, 'y')
    (wd, w0) = param(w)
    sc, sc0 = param(scale) if scale is not None else (None, None)
    sh, sh0 = param(shift) if shift is not None else (None, None)
    _hip = hip()
    stats = torch.zeros(_hip.STATS_REPL * 2 * C, dtype=torch.float64, device=dev())
    rc = _hip.lib().y2_dwconv_fwd(xb.ptr, _hip.ptr(wd), _hip.ptr(sc), _hip.ptr(sh), slope, yb.ptr, _hip.ptr(stats), B, H, W, C, xb.ld, yb.ld, stride, _hip.stream())
    assert rc == OK
    torch.cuda.synchronize()
    ref = raw
    if scale is not None:
        ref = ref * scale.double().view(1, -1, 1, 1)
    if shift is not None:
        ref = ref + shift.double().view(1, -1, 1, 1)
    ref = F.leaky_relu(ref, slope) if slope != 1.0 else ref
    err = rel(yb.view(), rows(ref))
    record('dwconv_fwd', '%s %s' % (name, form), err)
    assert err <= TOL_FWD, err
    assert yb.outside_untouched()
    assert xb.unchanged() and torch.equal(wd, w0) and (sc is None or torch.equal(sc, sc0)) and (sh is None or torch.equal(sh, sh0))
    # statistics of the RAW sum, whatever the epilogue: all copies added, against the fp64 sums
    copies = stats.view(_hip.STATS_REPL, 2, C).cpu()
    st = copies.sum(0)
    np.testing.assert_allclose(st[0].numpy(), raw.sum((0, 2, 3)).numpy(), rtol=1e-5, atol=1e-6 * raw.abs().sum().item() / C)
    np.testing.assert_allclose(st[1].numpy(), raw.pow(2).sum((0, 2, 3)).numpy(), rtol=1e-5)
    # workgroup b adds into copy b mod Y2_STATS_REPL: below 32 pixel blocks the copies in use tell the grid's width (the mirror's gx, observed on the
    # device); from 32 on - every capped case - all copies are in use whatever the width, and gx rests on the mirror being pinned to the source text
    gx = dc.derive(c, 'fwd')[1].gx
    assert int((copies[:, 1].sum(1) > 0).sum()) == min(gx, _hip.STATS_REPL)


@pytest.mark.parametrize('name', list(dc.CASES))
def test_forward(name):
    """Affine + LeakyReLU(0.1) epilogue with statistics on every case.  Measured worst error: see README (tests/test_gpu_dwconv.py)."""
    forward(name, 'affine-slope0.1')


@pytest.mark.parametrize('form', [f for f in dc.FORMS if f != 'affine-slope0.1'])
@pytest.mark.parametrize('name', dc.FORM_CASES)
def test_forward_epilogue_forms(name, form):
    forward(name, form)


@pytest.mark.parametrize('name', list(dc.CASES))
def test_dgrad(name):
    c, B, C, H, W, stride, s = geometry(name)
    _, w, dz, _, dx, _ = reference(name)
    zb, db = window(c, s, 'dz', dz), window(c, s, 'dx')
    wd, w0 = param(w)
    _hip = hip()
    assert _hip.lib().y2_dwconv_dgrad(zb.ptr, _hip.ptr(wd), db.ptr, B, H, W, C, zb.ld, db.ld, stride, _hip.stream()) == OK
    torch.cuda.synchronize()
    err = rel(db.view(), rows(dx))
    record('dwconv_dgrad', name, err)
    assert err <= TOL_GRAD, err
    assert db.outside_untouched() and zb.unchanged() and torch.equal(wd, w0)


@pytest.mark.parametrize('name', list(dc.CASES))
def test_wgrad(name):
    """The workspace holds exactly the bytes the mirror derives for the launch's vector width (never more than the query's answer): a grid wider than the
    mirror's would be refused, a write past it would hit the guard."""
    c, B, C, H, W, stride, s = geometry(name)
    x, _, dz, _, _, dw = reference(name)
    xb, zb = window(c, s, 'x', x), window(c, s, 'dz', dz)
    _hip = hip()
    need = dc.wgrad_need_bytes(B, H, W, C, stride, dc.derive(c, 'wgrad')[1].CV)
    assert 0 < need <= _hip.lib().y2_dwconv_wgrad_workspace_bytes(B, H, W, C, stride)
    ws, out = Window(1, need // 4, need // 4), Window(1, C * 9, C * 9)
    assert _hip.lib().y2_dwconv_wgrad(xb.ptr, zb.ptr, out.ptr, ws.ptr, need, B, H, W, C, xb.ld, zb.ld, stride, _hip.stream()) == OK
    torch.cuda.synchronize()
    err = rel(out.view().reshape(C, 1, 3, 3), dw)
    record('dwconv_wgrad', name, err)
    assert err <= TOL_GRAD, err
    assert out.outside_untouched() and ws.outside_untouched() and xb.unchanged() and zb.unchanged()


def test_refusals_leave_every_buffer_alone():
    """Every refusal of the three entry points on real buffers (a check that regressed would launch inside them): bad sizes and strides, a pixel stride
    below C, a missing operand, a misaligned or too small workspace."""
    from test_dw_cases import BAD_SHAPES
    B, H, W, C = 2, 5, 7, 8
    n = B * H * W
    g = torch.Generator().manual_seed(3)
    xb, zb = Window(n, C, C, 0, torch.randn(n, C, generator=g)), Window(n, C, C, 0, torch.randn(n, C, generator=g))
    yb, out = Window(n, C, C), Window(1, C * 9, C * 9)
    wd, w0 = param(torch.randn(C, 1, 3, 3, generator=g))
    need = dc.wgrad_workspace_bytes(B, H, W, C, 1)
    ws = Window(1, need // 4 + 4, need // 4 + 4)
    _hip = hip()
    L, st, w = _hip.lib(), _hip.stream(), _hip.ptr(wd)
    fwd = lambda x, w, y, *a: L.y2_dwconv_fwd(x, w, None, None, 1.0, y, None, *a, st)          # noqa: E731
    dgrad = lambda dz, w, dx, *a: L.y2_dwconv_dgrad(dz, w, dx, *a, st)          # noqa: E731
    wgrad = lambda x, dz, dw, wsp, nbytes, *a: L.y2_dwconv_wgrad(x, dz, dw, wsp, nbytes, *a, st)          # noqa: E731
    for bad in BAD_SHAPES:
        if max(bad) > 100:
            continue                                    # (no real buffer holds 2^32 pixels: that refusal is checked from the source text)
        b, h, w_, c, stride = bad
        assert fwd(xb.ptr, w, yb.ptr, b, h, w_, c, c, c, stride) == EINVAL, bad
        assert dgrad(zb.ptr, w, yb.ptr, b, h, w_, c, c, c, stride) == EINVAL, bad
        assert wgrad(xb.ptr, zb.ptr, out.ptr, ws.ptr, need, b, h, w_, c, c, c, stride) == EINVAL, bad
    for lda, ldb in ((C - 1, C), (C, C - 1)):
        assert fwd(xb.ptr, w, yb.ptr, B, H, W, C, lda, ldb, 1) == EINVAL
        assert dgrad(zb.ptr, w, yb.ptr, B, H, W, C, lda, ldb, 1) == EINVAL
        assert wgrad(xb.ptr, zb.ptr, out.ptr, ws.ptr, need, B, H, W, C, lda, ldb, 1) == EINVAL
    for x, ww, y in ((None, w, yb.ptr), (xb.ptr, None, yb.ptr), (xb.ptr, w, None)):
        assert fwd(x, ww, y, B, H, W, C, C, C, 1) == EINVAL and dgrad(x, ww, y, B, H, W, C, C, C, 1) == EINVAL
    for x, dz, dw, wsp in ((None, zb.ptr, out.ptr, ws.ptr), (xb.ptr, None, out.ptr, ws.ptr), (xb.ptr, zb.ptr, None, ws.ptr), (xb.ptr, zb.ptr, out.ptr, None)):
        assert wgrad(x, dz, dw, wsp, need, B, H, W, C, C, C, 1) == EINVAL
    assert wgrad(xb.ptr, zb.ptr, out.ptr, ctypes.c_void_p(ws.ptr.value + 4), need, B, H, W, C, C, C, 1) == EALIGN
    assert wgrad(xb.ptr, zb.ptr, out.ptr, ws.ptr, dc.wgrad_need_bytes(B, H, W, C, 1, 4) - 1, B, H, W, C, C, C, 1) == EINVAL
    torch.cuda.synchronize()
    assert all(b.unchanged() for b in (xb, zb, yb, out, ws)) and torch.equal(wd, w0)
