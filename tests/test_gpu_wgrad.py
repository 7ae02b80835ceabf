"""GPU parity tests of the weight-gradient kernels, one dispatch path at a time: conv_wgrad_kernel (csrc/conv_wgrad.hip: five tile variants, general /
LIN / DZRAW loaders, spread / checked inner loops, store / atomic / deterministic epilogues), the Winograd drivers of csrc/wino.hip (2x2 and 4x4
tiles, packed / native output, in-loader or three-step gradient operand, v_transformed), the first layer's two kernels and _hip.conv_wgrad.

Ground rules of every test here: inputs are drawn in fp32 from a seeded generator and upcast to fp64 for the reference, so kernel and reference see
bit-identical inputs; the reference is torch-CPU fp64 autograd of F.conv2d (never the kernel's formula restated); operands live in windows of wider
buffers whose pad channels and whose memory in front of and behind the window are NaN, so a result that depends on anything outside the window is
not finite; every destination sits between -7.0 guards that must survive.  tests/wgrad_cases.py holds the case tables and the mirror of the host
code's dispatch (checked on the CPU by tests/test_wgrad_cases.py); the tests here observe the dispatch on the device.

What the NaN pads can and cannot show: a pad channel that the loader fetches as operand column Cout + n (or taps*Cin + n) lands in accumulator row
(column) Cout + n alone - the rows and columns of an MFMA product are independent - and the epilogue never stores those, so the a_ok / b_ok masks of
conv_wgrad_kernel change no output (a build with a_ok forced to true passes every test here, as it must).  The pads do catch every address that is
formed with the wrong stride or base (Cout for ldz, Cin for ldx, a window's offset dropped) and rows past the last pixel that are not zero."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import wgrad_cases as wc

pytestmark = pytest.mark.gpu
TOL = 2e-5                      # direct kernels (the project's bound, tests/test_gpu_train.py)
TOL_WINO = 4 * TOL              # both Winograd forms (ibid.)
SENT = -7.0
NAN = float('nan')
GUARD = 64                      # floats in front of and behind every operand and destination (256 B: keeps 16-B alignment)
OK, EINVAL, EALIGN, ENOSUP = 0, -1, -2, -3      # include/yolo2_hip.h


def dev():
    return torch.device('cuda:0')


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def rel(got, ref):
    ref = ref.double()
    rms = ref.pow(2).mean().sqrt().item()
    return (got.double().cpu() - ref).abs().max().item() / max(rms, 1e-30)


def randn32(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


class Operand(object):
    """A channels-last tensor [..., C] as the kernels see it: rows of `C + pad` floats with the data in channels off .. off + C of a NaN-filled buffer that
    also has GUARD NaNs in front and behind.  `ptr` points at the first data element, `ld` is the row stride."""

    def __init__(self, t, pad=0, off=0):
        C = t.shape[-1]
        assert off <= pad
        self.ld = C + pad
        rows = t.numel() // C
        flat = torch.full((GUARD + rows * self.ld + GUARD,), NAN, dtype=torch.float32)
        flat[GUARD:GUARD + rows * self.ld].view(rows, self.ld)[:, off:off + C] = t.reshape(rows, C)
        self.buf = flat.to(dev())
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + (GUARD + off) * 4)


class Dest(object):
    """n floats holding `fill` between two guards of GUARD sentinels."""

    def __init__(self, n, fill=SENT):
        self.buf = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.float32, device=dev())
        self.t = self.buf[GUARD:GUARD + n]
        self.t.fill_(fill)
        self.ptr = ctypes.c_void_p(self.t.data_ptr())

    def guards_intact(self):
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[-GUARD:] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())


def kernels_of(fn):
    """Names of the library kernels `fn` launches (the per-launch event hooks of include/yolo2_hip.h: y2_prof_*)."""
    import _hip
    L = _hip.lib()
    torch.cuda.synchronize()
    L.y2_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.y2_prof_enable(0)
    name, ms, fl = ctypes.create_string_buffer(96), ctypes.c_float(), ctypes.c_double()
    return [name.value.decode() for i in range(L.y2_prof_count()) if L.y2_prof_get(i, name, 96, ctypes.byref(ms), ctypes.byref(fl)) == 0]


def reference(shape, stride=1, pad=None, regime='randn'):
    return _reference(tuple(shape), stride, pad, regime)


@functools.lru_cache(maxsize=None)
def _reference(shape, stride, pad, regime):
    """(x [B,cin,H,W] fp32, dz [B,cout,Ho,Wo] fp32, dW fp64 by autograd, rel of fp32 autograd against it).  Shared by every test of a shape: read only."""
    B, cin, cout, H, W, k = shape
    pad = (k - 1) // 2 if pad is None else pad
    g = torch.Generator().manual_seed(1000003 * B + 10007 * cin + 101 * cout + 13 * H + 7 * W + k + 31 * stride + (5 if regime != 'randn' else 0))
    x = randn32(g, B, cin, H, W)
    dz = randn32(g, B, cout, wc.out_size(H, k, stride, pad), wc.out_size(W, k, stride, pad))
    if regime == 'mean-positive':                                   # post-LeakyReLU activations, a gradient with a common sign
        x = F.leaky_relu(x + 1, 0.1)
        dz = dz * 0.1 + 0.05
    w = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, stride=stride, padding=pad).backward(dz.double())
    floor = None
    if regime == 'mean-positive':
        w32 = torch.zeros(cout, cin, k, k, dtype=torch.float32, requires_grad=True)
        F.conv2d(x, w32, stride=stride, padding=pad).backward(dz)
        floor = rel(w32.grad, w.grad)
    return x, dz, w.grad, floor


def operands(shape, layout, stride=1, pad=None, regime='randn'):
    x, dz, want, floor = reference(shape, stride, pad, regime)
    px, pz, ox, oz = wc.LAYOUTS[layout]
    return Operand(nhwc(x), px, ox), Operand(nhwc(dz), pz, oz), want, floor


def reindex(packed, cout, cin, k):
    """[cout][tap][cin] -> [cout][cin][ky][kx] in Python: the witness of y2_unpack_weight_grad."""
    return packed.view(cout, k, k, cin).permute(0, 3, 1, 2).contiguous()


def unpack(packed, cout, cin, k):
    import _hip
    out = Dest(cout * cin * k * k)
    _hip.check(_hip.lib().y2_unpack_weight_grad(ctypes.c_void_p(packed.data_ptr()), out.ptr, cout, cin, k, _hip.stream()), 'unpack')
    assert out.guards_intact()
    return out.t.view(cout, cin, k, k)


def direct(xo, zo, dw, shape, stride=None, pad=None):
    """y2_conv_wgrad, or y2_conv_wgrad_ex when a stride is given; returns the return code."""
    import _hip
    B, cin, cout, H, W, k = shape
    L = _hip.lib()
    if stride is None:
        return L.y2_conv_wgrad(xo.ptr, zo.ptr, dw.ptr, B, H, W, cin, xo.ld, cout, zo.ld, k, _hip.stream())
    return L.y2_conv_wgrad_ex(xo.ptr, zo.ptr, dw.ptr, B, H, W, cin, xo.ld, cout, zo.ld, k, stride, pad, _hip.stream())


def check_direct(shape, layout, plan, bound=TOL, stride=None, pad=None, regime='randn'):
    """Parity into a zeroed destination, then the observable split decision: into a destination full of 3.0 an unsplit launch stores the gradient and a
    split one adds to what is there."""
    B, cin, cout, H, W, k = shape
    xo, zo, want, floor = operands(shape, layout, 1 if stride is None else stride, pad, regime)
    dw = Dest(want.numel(), 0.0)
    assert direct(xo, zo, dw, shape, stride, pad) == OK
    got = unpack(dw.t, cout, cin, k)
    assert bool(torch.isfinite(dw.t).all()), 'the result depends on memory outside the operand windows'
    assert dw.guards_intact()
    err = rel(got, want)
    if layout == 'dense':
        assert torch.equal(got, reindex(dw.t, cout, cin, k))
    d3 = Dest(want.numel(), 3.0)
    assert direct(xo, zo, d3, shape, stride, pad) == OK
    assert d3.guards_intact() and bool(torch.isfinite(d3.t).all())
    base = 3.0 if plan.splits > 1 else 0.0
    err3 = rel(reindex(d3.t, cout, cin, k).double().cpu() - base, want)
    assert err3 <= bound, ('split' if base else 'unsplit', err3)
    return err, floor


# ================================================================================================ 1. direct kernel
@pytest.mark.parametrize('layout', list(wc.LAYOUTS))
@pytest.mark.parametrize('name', list(wc.DIRECT_CASES))
def test_direct(name, layout):
    c = wc.DIRECT_CASES[name]
    err, _ = check_direct(c.shape, layout, wc.direct_plan(*c.shape))
    assert err <= TOL, err


@pytest.mark.parametrize('layout', list(wc.LAYOUTS))
@pytest.mark.parametrize('name', list(wc.EX_CASES))
def test_direct_strided(name, layout):
    B, cin, cout, H, W, k, stride, pad = wc.EX_CASES[name]
    shape = (B, cin, cout, H, W, k)
    err, _ = check_direct(shape, layout, wc.direct_plan(*shape, stride=stride, pad=pad), stride=stride, pad=pad)
    assert err <= TOL, err


@pytest.mark.parametrize('name', wc.MEANPOS_DIRECT)
def test_direct_mean_positive(name):
    """Post-LeakyReLU activations and a gradient with a common sign: every product of the K-split partial sums has the same sign, so the sums grow
    instead of cancelling.  Bound: the project's, or 4 x the error of torch-CPU fp32 autograd against the same fp64 reference (the factor the
    training-step tests use over their fp32 floor)."""
    c = wc.DIRECT_CASES[name]
    floor = reference(c.shape, 1, None, 'mean-positive')[3]
    bound = max(TOL, 4 * floor)
    err, _ = check_direct(c.shape, 'both-offset', wc.direct_plan(*c.shape), bound=bound, regime='mean-positive')
    print('mean-positive %s: kernel %.3g, fp32 floor %.3g, bound %.3g' % (name, err, floor, bound))
    assert err <= bound, (err, floor)


# ================================================================================================ 2. Winograd forms
def wino_workspace(shape, mode):
    import _hip
    B, cin, cout, H, W = shape
    need = _hip.lib().y2_wino_wgrad_workspace_bytes_ex(B, H, W, cin, cout, mode)
    assert need > 0 and need % 16 == 0
    return torch.full((need // 4,), NAN, dtype=torch.float32, device=dev()), need          # exactly what the library asks for, poisoned


def wino(xo, zo, dw, shape, mode, ws, ws_bytes, v=None):
    import _hip
    B, cin, cout, H, W = shape
    return _hip.lib().y2_wino_wgrad_ex(xo.ptr if xo is not None else None, zo.ptr, dw.ptr, B, H, W, cin, xo.ld if xo is not None else cin, cout, zo.ld,
                                       _hip.ptr(v), _hip.ptr(ws), ws_bytes, mode, _hip.stream())


def wino_result(dw, shape, mode):
    B, cin, cout, H, W = shape
    return dw.t.view(cout, cin, 3, 3) if mode & 1 else unpack(dw.t, cout, cin, 3)


def check_wino(shape, layout, mode, regime='randn'):
    """One y2_wino_wgrad_ex call into a destination full of 5.0 with a NaN-filled workspace; returns (error, launch list)."""
    B, cin, cout, H, W = shape
    xo, zo, want, floor = operands(shape + (3,), layout, regime=regime)
    ws, need = wino_workspace(shape, mode)
    dw = Dest(want.numel(), 5.0)
    rc = []
    names = kernels_of(lambda: rc.append(wino(xo, zo, dw, shape, mode, ws, need)))
    assert rc == [OK]
    assert bool(torch.isfinite(dw.t).all()), 'the result depends on memory outside the operand windows (or on what the workspace held)'
    assert dw.guards_intact()
    got = wino_result(dw, shape, mode)
    if layout == 'dense' and not mode & 1:
        assert torch.equal(got, reindex(dw.t, cout, cin, 3))
    return rel(got, want), names


@pytest.mark.parametrize('layout', list(wc.LAYOUTS))
@pytest.mark.parametrize('name', list(wc.WINO_CASES))
def test_winograd_2x2(name, layout):
    c = wc.WINO_CASES[name]
    plan = wc.wino_plan(*c.shape)
    for mode in (0, 1):                                             # packed, native
        err, names = check_wino(c.shape, layout, mode)
        assert err <= TOL_WINO, (mode, err)
        assert ('zero_fill_kernel' in names) == (plan.splits > 1), names
        assert 'wino_input_kernel' in names and ('wino_dw_kernel' in names)
        if c.form == 'dzraw':
            assert 'conv_wgrad_kernel[grouped,dz]' in names and 'wino_tile_table_kernel' in names, names
            assert 'wino_dz_kernel' not in names and 'conv_wgrad_kernel[grouped]' not in names, names
        else:
            assert 'wino_dz_kernel' in names and 'conv_wgrad_kernel[grouped]' in names, names
            assert 'conv_wgrad_kernel[grouped,dz]' not in names and 'wino_tile_table_kernel' not in names, names


@pytest.mark.parametrize('layout', list(wc.LAYOUTS))
@pytest.mark.parametrize('name', list(wc.WINO6_CASES))
def test_winograd_4x4(name, layout):
    c = wc.WINO6_CASES[name]
    plan = wc.wino6_plan(*c.shape)
    for mode in (2, 3):
        err, names = check_wino(c.shape, layout, mode)
        assert err <= TOL_WINO, (mode, err)
        assert ('zero_fill_kernel' in names) == (plan.splits > 1), names
        assert [n for n in names if n != 'zero_fill_kernel'] == ['wino6_in_kernel', 'wino6_in_kernel[dz]', 'conv_wgrad_kernel[grouped]', 'wino6_dw_kernel'], names


@pytest.mark.parametrize('layout', ['dense', 'both-offset'])
@pytest.mark.parametrize('name', wc.WINO_V_CASES)
def test_winograd_from_the_transformed_input_of_a_forward(name, layout):
    """x = NULL: V is what a Winograd forward left at the head of its workspace.  The gradient operand still comes through its window."""
    import _hip
    L = _hip.lib()
    c = wc.WINO_CASES[name]
    B, cin, cout, H, W = c.shape
    x, dz, want, _ = reference(c.shape + (3,))
    zo = Operand(nhwc(dz), *wc.LAYOUTS[layout][1::2])
    xd = nhwc(x).to(dev())
    wp = torch.zeros(cout * 9 * cin, device=dev())
    uf = _hip.wino_weight(wp, cout, cin)
    yf = torch.empty(B, H, W, cout, device=dev())
    pf = _hip.ConvParams()
    pf.x, pf.w, pf.y, pf.algo = xd.data_ptr(), uf.data_ptr(), yf.data_ptr(), 1
    pf.B, pf.H, pf.W, pf.Cin, pf.ldx, pf.Cout, pf.ksize, pf.ldy, pf.slope = B, H, W, cin, cin, cout, 3, cout, 1.0
    wsf = torch.empty(L.y2_conv_fwd_workspace_bytes(ctypes.byref(pf)) // 4 + 4, device=dev())
    pf.workspace, pf.workspace_bytes = wsf.data_ptr(), wsf.numel() * 4
    _hip.check(L.y2_conv_fwd(ctypes.byref(pf), _hip.stream()), 'wino fwd')
    plan = wc.wino_plan(*c.shape)
    for mode in (0, 1):
        ws, need = wino_workspace(c.shape, mode)
        dw = Dest(want.numel(), 5.0)
        rc = []
        names = kernels_of(lambda: rc.append(wino(None, zo, dw, c.shape, mode, ws, need, v=wsf)))
        assert rc == [OK]
        assert 'wino_input_kernel' not in names and 'conv_wgrad_kernel[grouped,dz]' in names, names
        assert ('zero_fill_kernel' in names) == (plan.splits > 1), names
        assert bool(torch.isfinite(dw.t).all()) and dw.guards_intact()
        err = rel(wino_result(dw, c.shape, mode), want)
        assert err <= TOL_WINO, (mode, err)


@pytest.mark.parametrize('name,mode', [(n, 0) for n in wc.MEANPOS_WINO] + [(n, 2) for n in wc.MEANPOS_WINO6])
def test_winograd_mean_positive(name, mode):
    c = (wc.WINO6_CASES if mode & 2 else wc.WINO_CASES)[name]
    floor = reference(c.shape + (3,), 1, None, 'mean-positive')[3]
    bound = max(TOL_WINO, 4 * floor)
    err, _ = check_wino(c.shape, 'both-offset', mode, regime='mean-positive')
    print('mean-positive %s mode %d: kernel %.3g, fp32 floor %.3g, bound %.3g' % (name, mode, err, floor, bound))
    assert err <= bound, (err, floor)


# ================================================================================================ 3. deterministic mode
class deterministic(object):
    """y2_set_deterministic for the block: the project's scratch, or `nbytes` of a private one."""

    def __init__(self, nbytes=None):
        self.ws = None if nbytes is None else torch.empty(nbytes // 4, dtype=torch.float32, device=dev())

    def __enter__(self):
        import _hip
        if self.ws is None:
            _hip.set_deterministic(True)
        else:
            _hip.check(_hip.lib().y2_set_deterministic(1, _hip.ptr(self.ws), self.ws.numel() * 4), 'y2_set_deterministic')
        return self

    def __exit__(self, *exc):
        import _hip
        _hip.set_deterministic(False)
        torch.cuda.synchronize()
        return False


@pytest.mark.parametrize('layout', ['dense', 'both-offset'])
@pytest.mark.parametrize('name', wc.DET_DIRECT)
def test_deterministic_direct(name, layout):
    c = wc.DIRECT_CASES[name]
    B, cin, cout, H, W, k = c.shape
    xo, zo, want, _ = operands(c.shape, layout)
    with deterministic():
        runs = [Dest(want.numel()) for _ in range(2)]              # sentinel-filled: the fixed-order reduction writes, it does not accumulate
        for dw in runs:
            assert direct(xo, zo, dw, c.shape) == OK
        torch.cuda.synchronize()
    assert torch.equal(runs[0].t, runs[1].t)
    assert all(dw.guards_intact() for dw in runs) and bool(torch.isfinite(runs[0].t).all())
    err = rel(reindex(runs[0].t, cout, cin, k), want)
    assert err <= TOL, err


@pytest.mark.parametrize('layout', ['dense', 'both-offset'])
@pytest.mark.parametrize('name', wc.DET_WINO)
def test_deterministic_winograd(name, layout):
    c = wc.WINO_CASES[name]
    B, cin, cout, H, W = c.shape
    xo, zo, want, _ = operands(c.shape + (3,), layout)
    with deterministic():
        for mode in (0, 1):
            runs, rc = [Dest(want.numel()) for _ in range(2)], []
            for dw in runs:
                ws, need = wino_workspace(c.shape, mode)
                names = kernels_of(lambda: rc.append(wino(xo, zo, dw, c.shape, mode, ws, need)))
            assert rc == [OK, OK]
            assert 'wino_dz_kernel' in names and 'conv_wgrad_kernel[grouped]' in names and 'zero_fill_kernel' not in names, names      # three-step, no atomics
            assert torch.equal(runs[0].t, runs[1].t)
            assert all(dw.guards_intact() for dw in runs) and bool(torch.isfinite(runs[0].t).all())
            err = rel(wino_result(runs[0], c.shape, mode), want)
            assert err <= TOL_WINO, (mode, err)


def test_deterministic_refusals_leave_the_destination_alone():
    c = wc.WINO6_CASES['f-unsplit-13x14']
    xo, zo, want, _ = operands(c.shape + (3,), 'dense')
    with deterministic():
        for mode in (2, 3):                                         # the 4x4-tile form has no fixed-order reduction
            ws, need = wino_workspace(c.shape, mode)
            dw = Dest(want.numel())
            assert wino(xo, zo, dw, c.shape, mode, ws, need) == ENOSUP
            torch.cuda.synchronize()
            assert dw.untouched()
    c = wc.DIRECT_CASES[wc.DET_TOO_SMALL]
    xo, zo, want, _ = operands(c.shape, 'dense')
    with deterministic(wc.DET_MIN_BYTES):                           # the minimum scratch: this case's partial rows need 2.25 MiB
        dw = Dest(want.numel())
        assert direct(xo, zo, dw, c.shape) == EINVAL
        torch.cuda.synchronize()
        assert dw.untouched()


# ================================================================================================ 4. first layer
def conv0_operands(B, cin, cout, H, W, ldz, seed):
    g = torch.Generator().manual_seed(seed)
    x = randn32(g, B, cin, H, W)
    dz = randn32(g, B, cout, H, W)
    w = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, padding=1).backward(dz.double())
    return Operand(x.reshape(-1, 1)), Operand(nhwc(dz), ldz - cout), w.grad            # x is NCHW and dense: NaN guards only


def conv0(xo, zo, dw, B, cin, cout, H, W):
    import _hip
    return _hip.lib().y2_conv0_wgrad(xo.ptr, zo.ptr, dw.ptr, B, H, W, cin, cout, zo.ld, _hip.stream())


@pytest.mark.parametrize('cin,cout,W,ldz', wc.conv0_cases())
def test_first_layer(cin, cout, W, ldz):
    B, H = 2, 5
    xo, zo, want = conv0_operands(B, cin, cout, H, W, ldz, 17 * cout + W + cin)
    dw = Dest(want.numel(), 0.0)
    assert conv0(xo, zo, dw, B, cin, cout, H, W) == OK
    assert bool(torch.isfinite(dw.t).all()) and dw.guards_intact()
    err = rel(dw.t.view(cout, cin, 3, 3), want)
    assert err <= TOL, err


def test_first_layer_row_walk():
    """B*H >= 4096 rows: the grid stops growing and every wave walks more than one row."""
    B, cin, cout, H, W = wc.CONV0_ROW_WALK
    assert wc.conv0_rows_per_wave(B * H) > 1
    xo, zo, want = conv0_operands(B, cin, cout, H, W, cout + 4, 5)
    dw = Dest(want.numel(), 0.0)
    assert conv0(xo, zo, dw, B, cin, cout, H, W) == OK
    assert bool(torch.isfinite(dw.t).all()) and dw.guards_intact()
    err = rel(dw.t.view(cout, cin, 3, 3), want)
    assert err <= TOL, err


def fused_operands(B, cin, cout, H, W, has_bn, seed):
    """The construction of test_first_layer_weight_gradient_without_a_materialised_dz (tests/test_gpu_round3.py): the two-pass y2_bn_act_bwd on dense
    tensors writes the dz that the fused kernel forms in its loader (same arithmetic per element, same pass-1 sums); the reduction over pixels
    that follows is then taken in fp64 by autograd of F.conv2d, so the bound is the one of every other weight gradient against fp64.  The fused
    kernel reads z and dy_pool through NaN-padded windows."""
    import _hip
    L, st, d = _hip.lib(), _hip.stream(), dev()
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, H, W, generator=g)
    z = torch.randn(B, H, W, cout, generator=g)
    z[:, ::2, 1::2] = z[:, ::2, ::2]                                # ties inside pooling windows: the first maximum must win
    dyp = torch.randn(B, H // 2, W // 2, cout, generator=g)
    gamma = (torch.rand(cout, generator=g) + 0.5).to(d)
    mean, invstd = (torch.randn(cout, generator=g) * 0.1).to(d), (torch.rand(cout, generator=g) + 0.5).to(d)
    scale, shift = gamma * invstd, (torch.randn(cout, generator=g) * 0.1).to(d)
    xd, zd, pd = x.to(d), z.to(d), dyp.to(d)
    bn = (_hip.ptr(mean) if has_bn else None, _hip.ptr(invstd) if has_bn else None, _hip.ptr(gamma) if has_bn else None)
    sums = torch.zeros(2 * cout, dtype=torch.float64, device=d)
    dz = torch.empty(B, H, W, cout, device=d)
    _hip.check(L.y2_bn_act_bwd(_hip.ptr(zd), _hip.ptr(scale), _hip.ptr(shift), *bn, 0.1, None, 0, 0, 0, _hip.ptr(pd), cout, 0, _hip.ptr(sums), _hip.ptr(dz),
                               cout, B, H, W, cout, cout, has_bn, st), 'two-pass')
    torch.cuda.synchronize()
    w = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, padding=1).backward(dz.cpu().permute(0, 3, 1, 2).double())
    keep = (scale, shift, mean, invstd, gamma, sums)
    return Operand(x.reshape(-1, 1)), Operand(z, 4), Operand(dyp, 8), keep, bn, w.grad


def conv0_fused(xo, zo, po, keep, bn, dw, B, cin, cout, H, W, has_bn):
    import _hip
    scale, shift, mean, invstd, gamma, sums = keep
    return _hip.lib().y2_conv0_wgrad_fused(xo.ptr, zo.ptr, _hip.ptr(scale), _hip.ptr(shift), *bn, 0.1, po.ptr, po.ld, _hip.ptr(sums), dw.ptr,
                                           B, H, W, cin, cout, zo.ld, has_bn, _hip.stream())


def test_first_layer_fused_row_walk():
    """B*H/2 >= 4096 row pairs: every wave walks more than one; z and dy_pool in windows."""
    B, cin, cout, H, W = wc.CONV0_FUSED_ROW_WALK
    cout = 8
    assert wc.conv0_rows_per_wave(B * H // 2) > 1
    xo, zo, po, keep, bn, want = fused_operands(B, cin, cout, H, W, 1, 11)
    dw = Dest(want.numel(), 0.0)
    assert conv0_fused(xo, zo, po, keep, bn, dw, B, cin, cout, H, W, 1) == OK
    assert bool(torch.isfinite(dw.t).all()) and dw.guards_intact()
    err = rel(dw.t.view(cout, cin, 3, 3), want)
    assert err <= TOL, err


def test_first_layer_deterministic():
    B, cin, cout, H, W = 3, 3, 40, 12, 16
    xo, zo, want = conv0_operands(B, cin, cout, H, W, cout + 5, 23)
    fx, fz, fp, keep, bn, fwant = fused_operands(B, cin, cout, H, W, 1, 29)
    with deterministic():
        runs = [Dest(want.numel()) for _ in range(2)]
        for dw in runs:
            assert conv0(xo, zo, dw, B, cin, cout, H, W) == OK
        fruns = [Dest(want.numel()) for _ in range(2)]
        for dw in fruns:
            assert conv0_fused(fx, fz, fp, keep, bn, dw, B, cin, cout, H, W, 1) == OK
        torch.cuda.synchronize()
    assert torch.equal(runs[0].t, runs[1].t) and torch.equal(fruns[0].t, fruns[1].t)
    assert all(dw.guards_intact() for dw in runs + fruns)
    assert rel(runs[0].t.view(cout, cin, 3, 3), want) <= TOL
    assert rel(fruns[0].t.view(cout, cin, 3, 3), fwant) <= TOL
    # partial rows of one workgroup per 4 rows (row pairs): 160 workgroups x 64 x 27 floats do not fit the 1 MiB minimum scratch
    import _hip
    B, cout, H = 20, 64, 64
    xo = Operand(torch.zeros(B * cin * H * W, 1))
    zo = Operand(torch.zeros(B * H * W, cout), 4)
    po = Operand(torch.zeros(B * H * W // 4, cout), 8)
    assert wc.conv0_grid(B * H // 2) * cout * cin * 9 * 4 > wc.DET_MIN_BYTES
    with deterministic(wc.DET_MIN_BYTES):
        dw = Dest(cout * cin * 9)
        assert conv0(xo, zo, dw, B, cin, cout, H, W) == EINVAL
        assert _hip.lib().y2_conv0_wgrad_fused(xo.ptr, zo.ptr, None, None, None, None, None, 0.1, po.ptr, po.ld, None, dw.ptr, B, H, W, cin, cout, zo.ld, 0,
                                               _hip.stream()) == EINVAL
        torch.cuda.synchronize()
        assert dw.untouched()


# ================================================================================================ 5. refusals
def test_refusals_return_their_code_and_leave_the_destination_alone():
    """Argument checks that return before any launch."""
    import _hip
    L, st = _hip.lib(), _hip.stream()
    B, H, W = 2, 6, 6
    buf = torch.zeros(1 << 16, device=dev())
    p, p1 = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(buf.data_ptr() + 4)
    dw = Dest(4096)
    wgrad = lambda x, z, cin, ldx, cout, ldz, k=3: L.y2_conv_wgrad(x, z, dw.ptr, B, H, W, cin, ldx, cout, ldz, k, st)
    wgrad_ex = lambda x, z, cin, ldx, cout, ldz, k=3: L.y2_conv_wgrad_ex(x, z, dw.ptr, B, H, W, cin, ldx, cout, ldz, k, 1, (k - 1) // 2, st)
    need = L.y2_wino_wgrad_workspace_bytes(B, H, W, 8, 12)
    wino_ex = lambda x, z, cin, ldx, cout, ldz, mode=0, ws=need: L.y2_wino_wgrad_ex(x, z, dw.ptr, B, H, W, cin, ldx, cout, ldz, None, p, ws, mode, st)
    for fn in (wgrad, wgrad_ex, wino_ex):
        assert fn(p, p, 6, 8, 12, 12) == EALIGN                     # Cin
        assert fn(p, p, 8, 8, 10, 12) == EALIGN                     # Cout
        assert fn(p, p, 8, 10, 12, 12) == EALIGN                    # ldx
        assert fn(p, p, 8, 8, 12, 14) == EALIGN                     # ldz
        assert fn(p1, p, 8, 8, 12, 12) == EALIGN                    # x one float off
        assert fn(p, p1, 8, 8, 12, 12) == EALIGN                    # dz one float off
        assert fn(p, p, 8, 4, 12, 12) == EINVAL                     # ldx < Cin
        assert fn(p, p, 8, 8, 12, 8) == EINVAL                      # ldz < Cout
    assert wgrad_ex(p, p, 8, 8, 12, 12, 9) == ENOSUP
    assert wgrad(p, p, 8, 8, 12, 12, 5) == ENOSUP
    for mode in (0, 1, 2, 3):
        short = L.y2_wino_wgrad_workspace_bytes_ex(B, H, W, 8, 12, mode) - 1
        assert wino_ex(p, p, 8, 8, 12, 12, mode, short) == EINVAL   # workspace one byte short
    assert wino_ex(p, p, 8, 8, 12, 12, 4) == EINVAL                 # a transformed gradient exists for the 4x4-tile form only
    assert wino_ex(p, p, 8, 8, 12, 12, 5) == EINVAL
    conv0 = lambda cin, cout: L.y2_conv0_wgrad(p, p, dw.ptr, B, H, W, cin, cout, cout, st)
    assert conv0(4, 32) == ENOSUP and conv0(3, 68) == ENOSUP
    fused = lambda h, w: L.y2_conv0_wgrad_fused(p, p, None, None, None, None, None, 0.1, p, 32, None, dw.ptr, B, h, w, 3, 32, 32, 0, st)
    assert fused(7, 16) == EINVAL                                   # odd H
    assert fused(6, 18) == ENOSUP                                   # W % 16
    torch.cuda.synchronize()
    assert dw.untouched()


# ================================================================================================ 6. _hip.conv_wgrad
def test_python_wrapper_choices_and_destinations():
    import _hip
    d = dev()
    small, large = (1, 32, 32, 6, 6, 3), (2, 32, 64, 13, 12, 3)
    assert all(_hip.eligible_wino(s[2], s[1], 3, s[1], s[2]) for s in (small, large))
    torch.cuda.synchronize()
    _hip._cache(_hip._WGRAD_WS).pop(str(d), None)                   # the scratch grows from nothing: small shape first, then the larger one
    sizes = []
    for shape in (small, large):
        B, cin, cout, H, W, k = shape
        x, dz, want, _ = reference(shape)
        xd, zd = nhwc(x).to(d), nhwc(dz).to(d)
        n = want.numel()
        for choice in (0, 1, 2):
            bound = TOL if choice == 0 else TOL_WINO
            call = lambda **kw: _hip.conv_wgrad(xd, zd, B, H, W, cin, cin, cout, cout, 3, choice=choice, **kw)
            fresh = call()
            assert fresh.numel() == n and rel(reindex(fresh, cout, cin, 3), want) <= bound, choice
            out = torch.full((n,), SENT, device=d)
            assert call(out=out) is out and rel(reindex(out, cout, cin, 3), want) <= bound, choice
            out = torch.zeros(n, device=d)
            assert call(out=out, zeroed=True) is out and rel(reindex(out, cout, cin, 3), want) <= bound, choice
            native, out = torch.full((cout, cin, 3, 3), SENT, device=d), torch.full((n,), SENT, device=d)
            got = call(out=out, native=native)
            assert (got is native) == (choice in (1, 2))
            if choice == 0:
                assert got is out and rel(reindex(out, cout, cin, 3), want) <= bound and bool((native == SENT).all())
            else:
                assert rel(native, want) <= bound and bool((out == SENT).all()), choice
        sizes.append(_hip._cache(_hip._WGRAD_WS)[str(d)].numel())
    assert sizes[1] > sizes[0]
    assert sizes[1] * 4 >= _hip.lib().y2_wino_wgrad_workspace_bytes_ex(*[large[i] for i in (0, 3, 4, 1, 2)], 0)
    # not eligible (1x1; a 3x3 whose ldx is no multiple of 4 cannot reach the library at all): the direct kernel, and the table is neither read nor written
    shape = (2, 32, 64, 9, 7, 1)
    B, cin, cout, H, W, k = shape
    x, dz, want, _ = reference(shape)
    table, misses = dict(_hip._TUNE), list(_hip.TUNE_MISSES)
    got = _hip.conv_wgrad(nhwc(x).to(d), nhwc(dz).to(d), B, H, W, cin, cin, cout, cout, 1)
    assert rel(reindex(got, cout, cin, 1), want) <= TOL
    assert _hip._TUNE == table and _hip.TUNE_MISSES == misses
