"""GPU parity tests of y2_conv_fwd, one dispatch path at a time: the LDS-DMA kernel of csrc/conv_fwd.hip (seven tiles; whole, K-sliced and mixed
launches; CTAIL, POOLORD, GEN, persistent, grouped), the wave-private kernel, the register-staged kernel with and without VEC, both epilogues in
every output combination, and the forward Winograd drivers of csrc/wino.hip (three-kernel form, the three generations of the fused kernel in every
variant and output mask, F(4x4,3x3) with and without its input transform).

Ground rules of every test here: inputs are drawn in fp32 from a seeded generator and upcast to fp64 for the reference, so kernel and reference see
bit-identical inputs; the reference is torch-CPU F.conv2d (F.conv_transpose2d for the transposed form) in fp64, never the kernel's formula restated;
x lives in a window of a wider buffer whose pad channels and whose memory in front of and behind the window are NaN, the filter, scale, shift and the
residual are NaN-guarded, the workspace is NaN-filled (and sentinel-guarded when it has exactly the queried size), so a result that depends on
anything outside an operand is not finite; every destination is a channel window of rows of -7.0 between -7.0 guards, and all of that must survive.
tests/fwd_cases.py holds the case tables and the mirror of the host code's dispatch (checked on the CPU by tests/test_fwd_cases.py, against the
library's own workspace answers too); the tests here observe the dispatch on the device: the kernel family by name, and conv_splitk_fixup_kernel
exactly when the mirror says the launch splits."""
import collections
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import fwd_cases as fc
from test_gpu_wgrad import GUARD, NAN, SENT, Dest, Operand, dev, kernels_of, nhwc, rel

pytestmark = pytest.mark.gpu
CONV_TOL = 2e-5                 # x rms of the fp64 reference: direct kernels (the project's bound, tests/test_gpu_kernels.py)
WINO_TOL = 4 * CONV_TOL         # both Winograd forms (ibid.)
OK, EINVAL, ENOSUP = fc.OK, fc.EINVAL, fc.ENOSUP
ALL_LAYOUTS = dict(fc.LAYOUTS, **fc.NONVEC_LAYOUTS)
SLOPE32 = torch.tensor(0.1, dtype=torch.float32).double().item()           # the slope the kernels see
YPAD, YOFF = 8, 4               # destination rows: 4 sentinel floats, the channel window, 4 more (multiples of 4: the Winograd stores are 16-byte)
DMA_NAMES = ('conv_fwd_dma_kernel', 'conv_fwd_dma_kernel[persistent]', 'conv_fwd_dma_kernel[grouped]', 'conv_fwd_wave_kernel', 'conv_fwd_kernel')


def key_of(p):
    return (p.B, p.cin, p.cout, p.H, p.W, p.k, p.stride, p.pad, p.transposed, p.out_hw)


@functools.lru_cache(maxsize=None)
def reference(key, regime='randn'):
    """x [B,cin,H,W], w (the forward filter), z = the raw convolution in fp64 [B,cout,Ho,Wo], scale, shift, residual [B,Ho,Wo,cout], and in the
    mean-positive regime the error of torch-CPU fp32 against z.  Shared by every test of a shape: read only."""
    B, cin, cout, H, W, k, stride, pad, transposed, ohw = key
    g = torch.Generator().manual_seed(1000003 * B + 10007 * cin + 101 * cout + 13 * H + 7 * W + k + 31 * stride + 3 * pad + (5 if regime != 'randn' else 0))
    x = torch.randn(B, cin, H, W, generator=g)
    wshape = (cin, cout, k, k) if transposed else (cout, cin, k, k)          # transposed: w is the filter of the conv whose data gradient this is
    w = torch.randn(*wshape, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    if regime == 'mean-positive':                                           # post-LeakyReLU activations, filters with a positive mean
        x = F.leaky_relu(x + 1, 0.1)
        w = w + 0.5 * (2.0 / (cin * k * k)) ** 0.5

    def conv(a, b):
        if transposed:
            op = (ohw[0] - ((H - 1) * stride - 2 * pad + k), ohw[1] - ((W - 1) * stride - 2 * pad + k))
            return F.conv_transpose2d(a, b, stride=stride, padding=pad, output_padding=op)
        return F.conv2d(a, b, stride=stride, padding=pad)
    z = conv(x.double(), w.double())
    floor = rel(conv(x, w), z) if regime == 'mean-positive' else None
    scale = torch.randn(cout, generator=g)                                  # both signs: negative scales in front of the pool
    shift = torch.randn(cout, generator=g) * 0.1
    res = torch.randn(B, z.shape[2], z.shape[3], cout, generator=g)
    return x, w, z, scale, shift, res, floor


def guarded(n):
    """n floats of NaN between NaN guards, 16-byte aligned: the place of a packed or transformed filter."""
    buf = torch.full((GUARD + n + GUARD,), NAN, dtype=torch.float32, device=dev())
    return buf, buf[GUARD:GUARD + n]


Ops = collections.namedtuple('Ops', 'x w scale shift res keep')


@functools.lru_cache(maxsize=6)
def operands(key, regime, layout, wform=0):
    """Device operands.  wform 0: y2_pack_weight (mode 1 for the transposed form), 1: + y2_wino_weight, 6: + y2_wino6_weight."""
    import _hip
    L, st = _hip.lib(), _hip.stream()
    B, cin, cout, H, W, k, stride, pad, transposed, ohw = key
    x, w, z, scale, shift, res, _ = reference(key, regime)
    lpad, loff = ALL_LAYOUTS[layout]
    wd = w.to(dev()).contiguous()
    buf, wp = guarded(w.numel())
    if transposed:
        _hip.check(L.y2_pack_weight(_hip.ptr(wd), _hip.ptr(wp), cin, cout, k, 1, st), 'pack1')
    else:
        _hip.check(L.y2_pack_weight(_hip.ptr(wd), _hip.ptr(wp), cout, cin, k, 0, st), 'pack')
    keep = [buf]
    if wform:
        n = (16 if wform == 1 else 36) * cout * cin
        buf2, u = guarded(n)
        fn = L.y2_wino_weight if wform == 1 else L.y2_wino6_weight
        _hip.check(fn(_hip.ptr(wp), _hip.ptr(u), cout, cin, st), 'filter transform')
        keep.append(buf2)
        wp = u
    torch.cuda.synchronize()
    assert bool(torch.isfinite(wp).all())
    return Ops(Operand(nhwc(x), lpad, loff), wp, Operand(scale.view(1, -1)), Operand(shift.view(1, -1)), Operand(res, 8, 4), keep)


class Workspace(object):
    """`need` bytes in one of four states.  'none': no workspace.  'exact': exactly the queried bytes, NaN, between sentinel guards.  'short': 4 bytes
    less.  'misaligned': the full size, 4 bytes off a 16-byte boundary (the library then treats it as absent)."""

    def __init__(self, need, state):
        self.state, n = state, need // 4
        self.buf = torch.full((GUARD + n + 4 + GUARD,), SENT, dtype=torch.float32, device=dev())
        self.buf[GUARD:GUARD + n + (1 if state == 'misaligned' else 0)] = NAN
        self.ptr = None if state == 'none' else self.buf.data_ptr() + 4 * GUARD + (4 if state == 'misaligned' else 0)
        self.bytes = 0 if state == 'none' else max(need - 4, 0) if state == 'short' else need
        self.n = n

    def offered(self):
        """Bytes the library can use, as the mirror counts them."""
        return self.bytes if self.state in ('exact', 'short') else 0

    def guards_intact(self):
        tail = GUARD + self.n + (1 if self.state == 'misaligned' else 0)
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[tail:] == SENT).all())


WS_STATES = ('none', 'exact', 'short', 'misaligned')
Result = collections.namedtuple('Result', 'rc names y yp stats ws need')


def conv(p, ops, ws='exact', scale=True, shift=True, slope=0.1, algo=0, residual=None, x=None, ldx=None, ws_bytes=None, fill=SENT):
    """One y2_conv_fwd call as problem p describes it; destinations that p does not name are not given.  fill: what y holds before the call."""
    import _hip
    L = _hip.lib()
    Ho, Wo = fc.out_hw(p)
    q = _hip.ConvParams()
    q.x, q.ldx = (ops.x.ptr.value, ops.x.ld) if x is None else (x, ldx)
    q.w = ops.w.data_ptr()
    q.scale = ops.scale.ptr.value if scale else None
    q.shift = ops.shift.ptr.value if shift else None
    y = yp = st = None
    if 'y' in p.outs:
        rows, width = (p.B * Ho * Wo // 4, 4 * p.cout) if p.out_mode else (p.B * Ho * Wo, p.cout)
        q.ldy, q.coff = width + YPAD, YOFF
        y = Dest(rows * q.ldy, fill)
        q.y = y.ptr.value
    if 'p' in p.outs:
        q.ldp, q.poff = p.cout + YPAD, YOFF
        yp = Dest(p.B * (p.H // 2) * (p.W // 2) * q.ldp)
        q.y_pool = yp.ptr.value
    if 's' in p.outs:
        st = torch.zeros(32 * 2 * p.cout, dtype=torch.float64, device=dev())      # Y2_STATS_REPL copies
        q.stats = st.data_ptr()
    if p.residual if residual is None else residual:
        q.residual, q.ldr = ops.res.ptr.value, ops.res.ld
    q.B, q.H, q.W, q.Cin, q.Cout, q.ksize = p.B, p.H, p.W, p.cin, p.cout, p.k
    q.out_mode, q.slope, q.tile, q.algo = p.out_mode, slope, p.tile, algo
    if p.stride != 1 or p.pad != (p.k - 1) // 2 or p.transposed:
        q.stride, q.pad_plus1 = p.stride, p.pad + 1
    if p.transposed:
        q.transposed, q.out_h, q.out_w = 1, p.out_hw[0], p.out_hw[1]
    need = L.y2_conv_fwd_workspace_bytes(ctypes.byref(q))
    w = Workspace(max(need, 0) if ws_bytes is None else ws_bytes, ws)
    q.workspace, q.workspace_bytes = w.ptr, w.bytes
    rc = []
    names = kernels_of(lambda: rc.append(L.y2_conv_fwd(ctypes.byref(q), _hip.stream())))
    return Result(rc[0], names, y, yp, st, w, need)


def window(d, cout):
    """The channel window of a destination as a CPU tensor [rows, cout]; everything around it must still be the sentinel."""
    assert d.guards_intact()
    full = d.t.view(-1, cout + YPAD).cpu()
    assert bool((full[:, :YOFF] == SENT).all()) and bool((full[:, YOFF + cout:] == SENT).all()), 'wrote outside its channel window'
    got = full[:, YOFF:YOFF + cout]
    assert bool(torch.isfinite(got).all()), 'the result depends on memory outside the operands (or on what the workspace held)'
    return got


def expected(p, z, scale, shift, slope, res=None):
    """(full output NCHW, pooled output NCHW) in fp64 from the raw convolution z."""
    u = z
    if scale is not None:
        u = u * scale.double().view(1, -1, 1, 1)
    if shift is not None:
        u = u + shift.double().view(1, -1, 1, 1)
    if res is not None:
        u = u + res.double().permute(0, 3, 1, 2)
    s = SLOPE32 if slope == 0.1 else slope
    a = torch.where(u > 0, u, u * s)
    return a, (F.max_pool2d(a, 2) if 'p' in p.outs else None)


def check(p, r, key, tol, scale=True, shift=True, slope=0.1, regime='randn', stats_tol=(1e-5, 1e-5, 1e-5), residual=None):
    """Everything a successful call promises; returns the largest relative error."""
    x, w, z, sc, sh, res, _ = reference(key, regime)
    assert r.rc == OK, r.rc
    assert r.ws.guards_intact()
    has_res = p.residual if residual is None else residual
    full, pooled = expected(p, z, sc if scale else None, sh if shift else None, slope, res if has_res else None)
    B, C, Ho, Wo = z.shape
    err = 0.0
    if r.y is not None:
        if p.out_mode == 1:                                                 # reorg: y[b, y/2, x/2, ((y&1)*2 + (x&1))*Cout + n]
            got = window(r.y, 4 * C).view(B, Ho // 2, Wo // 2, 2, 2, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, Ho, Wo)
        else:
            got = window(r.y, C).view(B, Ho, Wo, C).permute(0, 3, 1, 2)
        err = max(err, rel(got, full))
    if r.yp is not None:
        err = max(err, rel(window(r.yp, C).view(B, Ho // 2, Wo // 2, C).permute(0, 3, 1, 2), pooled))
    if r.stats is not None:
        got = r.stats.cpu().view(32, 2 * C).sum(0)
        assert bool(torch.isfinite(got).all())
        s1, s2 = z.sum((0, 2, 3)), (z * z).sum((0, 2, 3))
        rt1, at1, rt2 = stats_tol
        assert bool(((got[:C] - s1).abs() <= at1 * float(s2.max().sqrt()) + rt1 * s1.abs()).all()), 'sum'
        assert bool(((got[C:] - s2).abs() <= rt2 * s2.abs()).all()), 'sum of squares'
    assert err <= tol, err
    return err


def check_dispatch(p, r, lay, family=None):
    """The launch list against the mirror: the family's name, and the fixup kernel exactly when the mirror's plan for the offered workspace splits."""
    m = fc.route(p, *ALL_LAYOUTS[lay])
    assert m.rc == OK
    assert [n for n in r.names if n in DMA_NAMES] == [family or m.family], r.names
    full, ks = fc.splits(m, r.ws.offered())
    assert ('conv_splitk_fixup_kernel' in r.names) == (ks > 1), (r.ws.state, r.names, full, ks)
    assert r.need == fc.workspace_bytes(p, *ALL_LAYOUTS[lay])
    return ks


def four_states(p, lay, tol=CONV_TOL):
    """A split-capable case: unsplit without workspace, split with exactly the queried bytes (guards intact), unsplit when 4 bytes are missing or the
    pointer is 4 bytes off - the same launch as without workspace, so those two must repeat its (verified) result bit for bit."""
    key = key_of(p)
    ops = operands(key, 'randn', lay)
    seen, first = {}, None
    for state in WS_STATES:
        r = conv(p, ops, ws=state)
        seen[state] = check_dispatch(p, r, lay)
        if state in ('none', 'exact'):
            check(p, r, key, tol)
        else:
            assert r.rc == OK and r.ws.guards_intact() and bool(torch.isnan(r.ws.buf[GUARD:GUARD + r.ws.n]).all())
            assert all(a is None or torch.equal(a.buf, b.buf) for a, b in ((first.y, r.y), (first.yp, r.yp)))
        first = first or r
    assert seen['none'] == seen['short'] == seen['misaligned'] == 1
    return seen['exact']


# ================================================================================================ 1. LDS-DMA kernel
@pytest.mark.parametrize('lay', list(fc.LAYOUTS))
@pytest.mark.parametrize('name', list(fc.DMA_CASES))
def test_dma_tiles(name, lay):
    c = fc.DMA_CASES[name]
    assert four_states(c.p, lay) > 1


@pytest.mark.parametrize('name', list(fc.XCD_CASES))
def test_dma_grids_of_every_residue(name):
    assert four_states(fc.XCD_CASES[name].p, 'both') in (2, 3)


@pytest.mark.parametrize('lay', list(fc.LAYOUTS))
@pytest.mark.parametrize('name', list(fc.GEN_CASES))
def test_general_form(name, lay):
    c = fc.GEN_CASES[name]
    assert (four_states(c.p, lay) > 1) == ('split-all' in c.claims)


@pytest.mark.parametrize('lay', list(fc.LAYOUTS))
@pytest.mark.parametrize('name', list(fc.WAVE_CASES))
def test_wave_kernel_and_its_fallback(name, lay):
    c = fc.WAVE_CASES[name]
    assert (four_states(c.p, lay) > 1) == ('unsplit' not in c.claims)


@pytest.mark.parametrize('name,lay', [(n, l) for n in fc.PERSIST_CASES for l in fc.LAYOUTS if 'walk' not in n or l in ('dense', 'both')])      # (the 33280-pixel walks: two layouts)
def test_persistent_tiles_against_plain_tiles(name, lay):
    """The walk of a persistent workgroup adds the slabs of a tile in the order the one-tile workgroup does, so the outputs are bit-identical."""
    c = fc.PERSIST_CASES[name]
    key = key_of(c.p)
    ops = operands(key, 'randn', lay)
    r = conv(c.p, ops, ws='exact')                                          # (the size query answers for the plain tile; a persistent launch leaves the scratch alone)
    assert check_dispatch(c.p, r, lay) == 1
    assert bool(torch.isnan(r.ws.buf[GUARD:GUARD + r.ws.n]).all())
    check(c.p, r, key, CONV_TOL)
    plain = c.p._replace(tile=fc.PERSIST_OF[c.p.tile])
    q = conv(plain, ops, ws='none')
    assert check_dispatch(plain, q, lay) == 1
    assert torch.equal(r.y.buf, q.y.buf)


# ================================================================================================ 2. register-staged kernel
@pytest.mark.parametrize('tid', fc.REG_IDS)
@pytest.mark.parametrize('name', list(fc.REG_SHAPES))
def test_register_staged_kernel(name, tid):
    shape, outs = fc.REG_SHAPES[name]
    key = key_of(fc.P(*shape))
    for lay, (pad, off) in ALL_LAYOUTS.items():
        vec = fc.route(fc.P(*shape, outs=outs), pad, off).vec
        ops = operands(key, 'randn', lay)
        for t in (fc.reg_tile_id(tid, vec),) + (() if vec or tid != 3 else (0,)):       # tile = 0 on everything that is not VEC (once per shape and layout)
            p = fc.P(*shape, tile=t, outs=outs)
            m = fc.route(p, pad, off)
            assert m.family == 'conv_fwd_kernel' and m.vec == vec
            r = conv(p, ops, ws='exact')
            assert check_dispatch(p, r, lay) == 1
            check(p, r, key, CONV_TOL)


# ================================================================================================ 3. epilogue forms
@pytest.mark.parametrize('name', list(fc.FAMILY_CASES))
def test_epilogue_forms(name):
    """Every output combination the API accepts, the reorg output, the residual, missing scale / shift with and without an activation - on split
    launches wherever the family splits."""
    base = fc.FAMILY_CASES[name]
    key, lay = key_of(base), 'both'
    ops = operands(key, 'randn', lay)
    ran = 0
    for outs in fc.OUTS:
        for sc, sh, slope in fc.AFFINE:
            p = base._replace(outs=outs)
            if fc.route(p, *ALL_LAYOUTS[lay]).rc != OK:
                r = conv(p, ops, scale=sc, shift=sh, slope=slope)
                assert r.rc == fc.route(p, *ALL_LAYOUTS[lay]).rc and all(d is None or d.untouched() for d in (r.y, r.yp))
                break
            r = conv(p, ops, scale=sc, shift=sh, slope=slope)
            check_dispatch(p, r, lay)
            check(p, r, key, CONV_TOL, scale=sc, shift=sh, slope=slope)
            ran += 1
    for kw in (dict(out_mode=1), dict(out_mode=1, outs='ys'), dict(residual=True), dict(residual=True, outs='ys')):
        p = base._replace(**kw)
        m = fc.route(p, *ALL_LAYOUTS[lay])
        r = conv(p, ops)
        if m.rc != OK:
            assert r.rc == m.rc and r.y.untouched()
            continue
        check_dispatch(p, r, lay)
        check(p, r, key, CONV_TOL)
        ran += 1
    assert ran >= (14 if name in ('persistent', 'gen') else 51)


@pytest.mark.parametrize('name', list(fc.FAMILY_CASES))
def test_mean_positive(name):
    """Post-LeakyReLU inputs and filters with a positive mean: the products of a K-slice have a common sign, so partial sums grow instead of
    cancelling.  Bound: the project's, or 4 x the error of torch-CPU fp32 conv2d against the same fp64 reference (the rule of tests/test_gpu_wgrad.py)."""
    p = fc.FAMILY_CASES[name]._replace(outs='yps' if name not in ('persistent', 'gen') else 'ys')
    key = key_of(p)
    floor = reference(key, 'mean-positive')[6]
    bound = max(CONV_TOL, 4 * floor)
    r = conv(p, operands(key, 'mean-positive', 'both'))
    check_dispatch(p, r, 'both')
    err = check(p, r, key, bound, regime='mean-positive')
    print('mean-positive %s: kernel %.3g, fp32 floor %.3g, bound %.3g' % (name, err, floor, bound))


# ================================================================================================ 4. Winograd
def wino_conv(p, algo, lay, regime='randn', ws='exact', **kw):
    ops = operands(key_of(p), regime, lay, 6 if algo in (6, 7) else 1)
    return conv(p, ops, ws=ws, algo=algo, **kw)


WINO_STATS = (1e-5, 2e-5, 2e-5)


@pytest.mark.parametrize('lay', list(fc.LAYOUTS))
@pytest.mark.parametrize('where', list(fc.WINO_MAPS))
@pytest.mark.parametrize('variant', list(fc.WINO_VARIANTS))
def test_winograd_variants_and_output_masks(variant, where, lay, monkeypatch):
    """Family x variant x out_mask.  Masks 4 (statistics only) and 6 (pool + statistics) run the OUT = 7 instantiation with a null y."""
    for mask in fc.wino_masks(where):
        p, algo, env = fc.wino_case(variant, where, mask)
        if env is not None:
            monkeypatch.setenv('Y2_WF_VARIANT', str(env))
        m = fc.wino_route(p, algo, *fc.LAYOUTS[lay], variant=env)
        r = wino_conv(p, algo, lay)
        assert r.rc == OK and r.need == m.ws_bytes
        assert tuple(n for n in r.names if n != 'conv_splitk_fixup_kernel') == m.names, (mask, r.names)
        check(p, r, key_of(p), WINO_TOL, stats_tol=WINO_STATS)


@pytest.mark.parametrize('variant', list(fc.WINO_WALKS))
def test_winograd_persistent_walks(variant, monkeypatch):
    """More units than resident workgroups: some workgroups take a second unit, the last column of units is ragged."""
    algo, tile, env, _, _ = fc.WINO_VARIANTS[variant]
    B, cin, cout, H, W = fc.WINO_WALKS[variant]
    if env is not None:
        monkeypatch.setenv('Y2_WF_VARIANT', str(env))
    p = fc.P(B, cin, cout, H, W, 3, tile=tile, outs='yps')
    r = wino_conv(p, algo, 'both')
    assert tuple(r.names) == fc.wino_route(p, algo, variant=env).names
    check(p, r, key_of(p), WINO_TOL, stats_tol=WINO_STATS)


@pytest.mark.parametrize('cout', fc.WINO_OUTPUT_COUTS)
def test_winograd_output_transform_widths(cout):
    p = fc.P(2, 32, cout, 7, 10, 3, outs='ys')
    r = wino_conv(p, 1, 'both')
    assert 'wino_output_kernel' in r.names
    check(p, r, key_of(p), WINO_TOL, stats_tol=WINO_STATS)
    p = fc.P(2, 32, cout, 8, 10, 3, outs='yps')
    check(p, wino_conv(p, 1, 'both'), key_of(p), WINO_TOL, stats_tol=WINO_STATS)


@pytest.mark.parametrize('name', list(fc.CHUNK_CASES))
def test_winograd_batch_chunks(name, monkeypatch):
    algo, tile, B, cin, cout, H, W = fc.CHUNK_CASES[name]
    monkeypatch.setenv('Y2_WINO_CHUNK_MB', str(fc.CHUNK_MB))
    p = fc.P(B, cin, cout, H, W, 3, tile=tile, outs='yps')
    m = fc.wino_route(p, algo, *fc.LAYOUTS['both'], chunk_mb=fc.CHUNK_MB)
    r = wino_conv(p, algo, 'both')
    assert r.need == m.ws_bytes and tuple(n for n in r.names if n != 'conv_splitk_fixup_kernel') == m.names * m.nchunks, r.names
    check(p, r, key_of(p), WINO_TOL, stats_tol=WINO_STATS)


@pytest.mark.parametrize('lay', ['dense', 'both'])
@pytest.mark.parametrize('name', list(fc.GROUPED_CASES))
def test_grouped_gemm_of_the_three_kernel_forms(name, lay):
    """16 groups (algo 1) and 36 groups (algo 6): whole and K-sliced; the 36-group form again from the transformed input the first call left (algo 7)."""
    algo, B, cin, cout, H, W = fc.GROUPED_CASES[name]
    p = fc.P(B, cin, cout, H, W, 3)
    m = fc.wino_route(p, algo, *fc.LAYOUTS[lay])
    split = fc.splits(m.inner, None)[1] > 1
    inner = fc.workspace_bytes(fc.P(1, cin, cout, 1, m.T, 1, groups=16 if algo == 1 else 36))
    for state in ('exact', 'short') if split else ('exact',):               # (4 bytes short of a size without split scratch is short of V + M: refused)
        r = wino_conv(p, algo, lay, ws=state)
        assert r.need == m.ws_bytes and tuple(n for n in r.names if n != 'conv_splitk_fixup_kernel') == m.names, r.names
        assert ('conv_splitk_fixup_kernel' in r.names) == (split and state == 'exact'), (state, r.names)
        check(p, r, key_of(p), WINO_TOL)
    assert (inner > 0) == split
    if algo == 6:
        v = r.ws.buf[GUARD:GUARD + 36 * m.T * cin].clone()                  # V = B^T d B of every tile: the head of the workspace
        assert bool(torch.isfinite(v).all())
        m7 = fc.wino_route(p, 7)
        r7 = wino_conv(p, 7, lay, x=v.data_ptr(), ldx=cin)
        assert r7.need == m7.ws_bytes and tuple(n for n in r7.names if n != 'conv_splitk_fixup_kernel') == m7.names, r7.names
        check(p, r7, key_of(p), WINO_TOL)
        assert torch.equal(r7.y.buf, conv(p, operands(key_of(p), 'randn', lay, 6), ws='exact', algo=6).y.buf)


@pytest.mark.parametrize('variant,algo', [('three-kernel', 1), ('gen1', 2), ('gen2-v3', 2), ('gen2-v5', 3), ('gen3-v0', 2), ('gen3-v4', 3), ('f43', 6)])
def test_winograd_mean_positive(variant, algo, monkeypatch):
    if variant == 'f43':
        p, env = fc.P(3, 64, 72, 12, 14, 3), None
    else:
        p, _, env = fc.wino_case(variant, 'even', 7)
    if env is not None:
        monkeypatch.setenv('Y2_WF_VARIANT', str(env))
    key = key_of(p)
    floor = reference(key, 'mean-positive')[6]
    bound = max(WINO_TOL, 4 * floor)
    r = wino_conv(p, algo, 'both', regime='mean-positive')
    err = check(p, r, key, bound, regime='mean-positive', stats_tol=WINO_STATS)
    print('mean-positive %s: kernel %.3g, fp32 floor %.3g, bound %.3g' % (variant, err, floor, bound))


# ================================================================================================ 5. refusals, deterministic mode
@pytest.mark.parametrize('name', list(fc.REFUSALS))
def test_refusals_return_their_code_and_leave_the_destinations_alone(name):
    f = fc.REFUSALS[name]
    ops = operands(key_of(f.p._replace(k=3 if f.p.k > 7 else f.p.k)), 'randn', f.layout)
    r = conv(f.p, ops, ws='exact', algo=f.algo, ws_bytes=1 << 20)
    torch.cuda.synchronize()
    assert r.rc == f.rc == fc.refusal_code(f)
    # (the three-kernel Winograd forms learn of their grouped GEMM's refusal after the input transform has run: it writes the workspace only)
    assert [n for n in r.names if n not in ('wino_input_kernel', 'wino6_in_kernel') or not name.startswith('grouped')] == []
    assert all(d is None or d.untouched() for d in (r.y, r.yp)) and (r.stats is None or not bool(r.stats.any()))
    assert (r.names != [] or bool(torch.isnan(r.ws.buf[GUARD:GUARD + r.ws.n]).all())) and r.ws.guards_intact()


@pytest.mark.parametrize('tid', [t + h for h in (0, 100) for t in fc.ABLATIONS])
def test_removed_ablation_ids_are_refused(tid):
    """Tile ids 91 - 93 (191 - 193) used to launch timing ablations of the register-staged kernel that compute wrong results.  They are unknown ids now:
    Y2_ENOSUP, nothing launched, a NaN-filled y bit for bit as it was - on the operands that tile 1 (and 101, the tile they were forms of) convolves."""
    shape = fc.P(*fc.REFUSED_TILE_SHAPE)
    key = key_of(shape)
    ops = operands(key, 'randn', 'dense')
    r = conv(shape._replace(tile=tid), ops, fill=NAN)
    torch.cuda.synchronize()
    assert r.rc == ENOSUP == fc.route(shape._replace(tile=tid)).rc and r.names == []
    assert torch.equal(r.y.buf.view(torch.int32), Dest(r.y.t.numel(), NAN).buf.view(torch.int32)) and r.ws.guards_intact()
    for good in (1, 101):
        check(shape, conv(shape._replace(tile=good), ops), key, CONV_TOL)


@pytest.mark.parametrize('name', list(fc.FAMILY_CASES))
def test_deterministic_mode(name):
    """Statistics from epilogue atomics are refused; everything else - K-sliced launches and their fixup included - repeats bit for bit."""
    import _hip
    from test_gpu_wgrad import deterministic
    base = fc.FAMILY_CASES[name]
    key = key_of(base)
    ops = operands(key, 'randn', 'both')
    with deterministic():
        r = conv(base._replace(outs='ys'), ops)
        assert r.rc == ENOSUP and r.names == [] and r.y.untouched() and not bool(r.stats.any())
        for outs in ('y', 'yp'):
            p = base._replace(outs=outs)
            if fc.route(p, *ALL_LAYOUTS['both']).rc != OK:
                continue
            a, b = conv(p, ops), conv(p, ops)
            check_dispatch(p, a, 'both')
            check(p, a, key, CONV_TOL)
            assert torch.equal(a.y.buf, b.y.buf) and (a.yp is None or torch.equal(a.yp.buf, b.yp.buf))
    assert not _hip.lib().y2_get_deterministic()
