"""GPU parity tests of the first layer's forward kernel, one dispatch path at a time: y2_conv0_fwd (csrc/conv0_fwd.hip: the eight straight-line
variants and the general kernel with NBLK 1 and 2, the tap tables of Cin 1 .. 4, the persistent walk from one tile per workgroup to the steady state of
its three LDS buffers, ragged tiles, channel masks, outputs written through into wider rows) and the three small kernels at the same boundary,
y2_nchw_to_nhwc, y2_maxpool2_fwd and y2_bn_fold (csrc/misc.hip).

Ground rules of every test here: inputs are drawn in fp32 from a seeded generator and upcast to fp64 for the reference, so kernel and reference see
bit-identical inputs; the reference is torch-CPU fp64 F.conv2d -> affine -> LeakyReLU -> F.max_pool2d, never the kernel's formula restated, built a
chunk of images at a time (no full-batch fp64 tensor of a large case exists; small shapes keep theirs for the tests that share it); x is a window of
a larger allocation with NaN on both sides, and so are the filter, scale and shift, so a result that depends on anything outside an operand is not
finite; y and y_pool are channel windows of rows of -7.0 with -7.0 pixels in front of and behind the tensor, and all of that must survive;
statistics go into Y2_STATS_REPL rows.  tests/conv0_cases.py holds the case tables and the mirror of the host code's dispatch (checked on the CPU by
tests/test_conv0_cases.py).  Every variant launches as `conv0_kernel`, so the dispatch cannot be observed here; the README's mutation table shows
which tests fail when the code a case claims to reach is changed."""
import collections
import ctypes
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import conv0_cases as cc
from test_gpu_wgrad import GUARD, NAN, SENT, Dest, Operand, deterministic, dev, nhwc

pytestmark = pytest.mark.gpu
CONV_TOL = 2e-5                 # x rms of the fp64 reference: the project's bound for direct convolutions (tests/test_gpu_kernels.py)
SUM_RTOL = 1e-5                 # statistics: relative, the sum with the absolute allowance of tests/test_gpu_mobilenet.py (1e-6 x sum|z| / C) on top
PACKED_RTOL = 2e-6              # statistics of the packed (straight-line) form against the general kernel's
REPL = 32                       # Y2_STATS_REPL
OK, EINVAL, ENOSUP = cc.OK, cc.EINVAL, cc.ENOSUP
CACHE_ELEMS = 1 << 22           # a raw fp64 convolution of up to 32 MB is kept for the tests that share its shape
CHUNK_ELEMS = 1 << 23           # larger ones are built in chunks of about 64 MB


def f32(v):
    """The value a float argument has inside the library."""
    return torch.tensor(v, dtype=torch.float32).double().item()


def key_of(c):
    return (min(max(c.B, 1), 1 << 20), max(c.cin, 1), max(c.cout, 1), max(c.H, 1), max(c.W, 1))


@functools.lru_cache(maxsize=3)
def inputs(key, regime='randn'):
    """x [B,cin,H,W], w [cout,cin,3,3], scale, shift in fp32.  Shared by every test of a shape: read only."""
    B, cin, cout, H, W = key
    g = torch.Generator().manual_seed(1000003 * (B % 1009) + 10007 * cin + 101 * cout + 13 * H + 7 * W + (5 if regime != 'randn' else 0))
    x = torch.randn(B, cin, H, W, generator=g)
    std = (2.0 / (9 * cin)) ** 0.5
    w = torch.randn(cout, cin, 3, 3, generator=g) * std
    if regime == 'mean-positive':                                           # an image after normalisation to [0, 1]-like values, filters with a positive mean
        x = F.leaky_relu(x + 1, 0.1)
        w = w + 0.5 * std
    scale = torch.randn(cout, generator=g)                                  # both signs: negative scales in front of the pool
    shift = torch.randn(cout, generator=g) * 0.1
    return x, w, scale, shift


_Z = {}


def z_chunks(key, regime='randn'):
    """(b0, b1, raw fp64 convolution of images b0 .. b1) over the batch, image chunk by image chunk."""
    B, cin, cout, H, W = key
    if (key, regime) in _Z:
        yield 0, B, _Z[(key, regime)]
        return
    x, w = inputs(key, regime)[:2]
    w64 = w.double()
    if B * cout * H * W <= CACHE_ELEMS:
        _Z[(key, regime)] = F.conv2d(x.double(), w64, padding=1)
        yield 0, B, _Z[(key, regime)]
        return
    nb = max(1, CHUNK_ELEMS // (cout * H * W))
    for b0 in range(0, B, nb):
        yield b0, min(B, b0 + nb), F.conv2d(x[b0:b0 + nb].double(), w64, padding=1)


def guarded(t):
    """A contiguous fp32 tensor as the kernel sees it: NaN in front of it and behind it.  (buffer, device pointer of the first element)"""
    buf = torch.full((GUARD + t.numel() + GUARD,), NAN, dtype=torch.float32)
    buf[GUARD:GUARD + t.numel()] = t.reshape(-1)
    buf = buf.to(dev())
    return buf, ctypes.c_void_p(buf.data_ptr() + 4 * GUARD)


Ops = collections.namedtuple('Ops', 'x w scale shift keep')


@functools.lru_cache(maxsize=2)
def operands(key, regime='randn', special=False):
    """Device operands.  special: the affine of the pool-first identity test - scales of both signs, some exactly 0 and some -0.0, and shifts large
    enough that whole windows saturate to one sign."""
    x, w, scale, shift = inputs(key, regime)
    if special:
        scale, shift = special_affine(scale, shift)
    parts = [guarded(t) for t in (x, w, scale, shift)]
    return Ops(parts[0][1], parts[1][1], parts[2][1], parts[3][1], [p[0] for p in parts])


def special_affine(scale, shift):
    scale, shift = scale.clone(), shift.clone()
    scale[3::5] = 0.0
    scale[1::7] = -0.0
    shift[2::4] = 30.0
    shift[0::6] = -30.0
    return scale, shift


Result = collections.namedtuple('Result', 'rc c y yp stats')


class Out(object):
    """A destination of `rows` pixels: rows of cout + pad floats, the kernel is given the address of channel `off` of the first one."""

    def __init__(self, rows, cout, pad, off):
        self.rows, self.cout, self.ld, self.off = rows, cout, cout + max(pad, 0), off
        self.d = Dest(rows * self.ld)
        self.ptr = ctypes.c_void_p(self.d.t.data_ptr() + 4 * off)

    def window(self):
        """The channel window [rows, cout] on the device; everything around it must still be the sentinel."""
        assert self.d.guards_intact(), 'wrote in front of or behind the tensor'
        full = self.d.t.view(self.rows, self.ld)
        assert bool((full[:, :self.off] == SENT).all()) and bool((full[:, self.off + self.cout:] == SENT).all()), 'wrote outside its channel window'
        got = full[:, self.off:self.off + self.cout]
        assert bool(torch.isfinite(got).all()), 'the result depends on memory outside the operands'
        return got

    def untouched(self):
        return self.d.untouched()


def run(c, ops, stats=None):
    """One y2_conv0_fwd call as c describes it; destinations that c does not name are not given.  stats: accumulate into this buffer."""
    import _hip
    L = _hip.lib()
    assert 'Y2_CONV0_WGS' not in os.environ, 'the mirror (conv0_cases.WGS_PER_CU) and every walk length here assume launch0\'s default grid'
    B, cin, cout, H, W = key_of(c)
    B = min(B, 4) if c.B > 1 << 20 else B                                   # (a refusal by size: the destinations are never reached)
    y = yp = st = None
    if 'y' in c.outs:
        y = Out(B * H * W, cout, c.ypad, c.yoff)
    if 'p' in c.outs:
        yp = Out(B * max(H // 2, 1) * max(W // 2, 1), cout, c.ppad, c.poff)
    if 's' in c.outs:
        st = torch.zeros(REPL, 2 * cout, dtype=torch.float64, device=dev()) if stats is None else stats
    rc = L.y2_conv0_fwd(None if c.nox else ops.x, None if c.now else ops.w, ops.scale if c.scale else None, ops.shift if c.shift else None,
                        y.ptr if y else None, yp.ptr if yp else None, _hip.ptr(st), c.B, c.H, c.W, c.cin, c.cout,
                        c.cout + c.ypad if y else 0, c.cout + c.ppad if yp else 0, c.slope, _hip.stream())
    return Result(rc, c, y, yp, st)


class Acc(object):
    """max |got - expected| and the rms of `expected` over the chunks of a tensor."""

    def __init__(self):
        self.err, self.sq, self.n = 0.0, 0.0, 0

    def add(self, got, exp64):
        """got: device fp32 [nb, h, w, C] (a view of the destination), exp64: CPU fp64 [nb, C, h, w]."""
        e = exp64.to(dev())
        self.err = max(self.err, (got.double().permute(0, 3, 1, 2) - e).abs().max().item())
        self.sq += e.pow(2).sum().item()
        self.n += e.numel()

    def rel(self):
        return self.err / max((self.sq / max(self.n, 1)) ** 0.5, 1e-30)


def verify(runs, regime='randn', tol=CONV_TOL, special=False):
    """Everything successful calls on the same operands promise, against one pass over the fp64 reference; returns the largest relative error."""
    key = key_of(runs[0].c)
    B, cin, cout, H, W = key
    _, _, scale, shift = inputs(key, regime)
    if special:
        scale, shift = special_affine(scale, shift)
    sc64, sh64 = scale.double().view(1, -1, 1, 1), shift.double().view(1, -1, 1, 1)
    torch.cuda.synchronize()
    wins = []
    for r in runs:
        assert r.rc == OK and key_of(r.c) == key, r.rc
        wins.append((r.y.window().view(B, H, W, cout) if r.y else None, r.yp.window().view(B, H // 2, W // 2, cout) if r.yp else None, Acc(), Acc()))
    s1, s2, sabs = torch.zeros(cout, dtype=torch.float64), torch.zeros(cout, dtype=torch.float64), 0.0
    want_stats = any(r.stats is not None for r in runs)
    for b0, b1, z in z_chunks(key, regime):
        if want_stats:
            s1 += z.sum((0, 2, 3))
            s2 += (z * z).sum((0, 2, 3))
            sabs += z.abs().sum().item()
        made = {}
        for r, (wy, wp, ay, ap) in zip(runs, wins):
            form = (r.c.scale, r.c.shift, f32(r.c.slope))
            if form not in made:
                u = z * sc64 if r.c.scale else z
                if r.c.shift:
                    u = u + sh64 if u is z else u.add_(sh64)
                made[form] = [u if form[2] == 1.0 else F.leaky_relu(u, form[2], inplace=u is not z), None]       # (u > 0 ? u : u * slope, for every slope)
            if wy is not None:
                ay.add(wy[b0:b1], made[form][0])
            if wp is not None:
                if made[form][1] is None:
                    made[form][1] = F.max_pool2d(made[form][0], 2)
                ap.add(wp[b0:b1], made[form][1])
    err = 0.0
    for r, (wy, wp, ay, ap) in zip(runs, wins):
        if wy is not None:
            assert ay.rel() <= tol, ('y', cc.variant_name(cc.route(r.c)), ay.rel())
            err = max(err, ay.rel())
        if wp is not None:
            assert ap.rel() <= tol, ('y_pool', cc.variant_name(cc.route(r.c)), ap.rel())
            err = max(err, ap.rel())
        if r.stats is not None:
            got = r.stats.cpu().sum(0)
            assert bool(torch.isfinite(got).all())
            assert bool(((got[:cout] - s1).abs() <= SUM_RTOL * s1.abs() + 1e-6 * sabs / cout).all()), ('sum', (got[:cout] - s1).abs().max().item())
            assert bool(((got[cout:] - s2).abs() <= SUM_RTOL * s2).all()), ('sum of squares', ((got[cout:] - s2).abs() / s2).max().item())
    return err


def parity(c, **kw):
    return verify([run(c, operands(key_of(c)))], **kw)


# ================================================================================================ 1. the general kernel
@pytest.mark.parametrize('name', list(cc.TAP_CASES))
def test_tap_tables_of_every_cin(name):
    parity(cc.TAP_CASES[name].c)


@pytest.mark.parametrize('name', list(cc.MASK_CASES))
def test_channel_masks_dense_and_written_through(name):
    parity(cc.MASK_CASES[name].c)


@pytest.mark.parametrize('name', list(cc.GEOMETRY_CASES))
def test_edge_geometry(name):
    parity(cc.GEOMETRY_CASES[name].c)


@pytest.mark.parametrize('outs', cc.OUTS)
@pytest.mark.parametrize('shape', list(cc.OUTSET_SHAPES))
def test_output_sets_of_the_general_kernel(shape, outs):
    cases = [c.c for n, c in cc.OUTSET_CASES.items() if n.startswith('%s-%s-' % (shape, outs))]
    assert len(cases) == len(cc.AFFINE)
    ops = operands(key_of(cases[0]))
    verify([run(c, ops) for c in cases])


@pytest.mark.parametrize('name', list(cc.FALL_CASES))
def test_aligned_looking_calls_that_fall_to_the_general_kernel(name):
    parity(cc.FALL_CASES[name].c)


@pytest.mark.parametrize('name', list(cc.GEN_WALK_CASES))
def test_general_kernel_walks(name):
    parity(cc.GEN_WALK_CASES[name].c)


# ================================================================================================ 2. the straight-line variants
@pytest.mark.parametrize('size,cout', [(s, co) for s in cc.ALIGNED_SIZES for co in (32, 64) if any(cc.STRAIGHT[v][0] == co for v in cc.STRAIGHT_AT[s])])
def test_straight_line_variants(size, cout):
    """Every variant of one width at one aligned size against one pass over the reference."""
    cases = [cc.straight_call(v, size) for v in cc.STRAIGHT_AT[size] if cc.STRAIGHT[v][0] == cout]
    ops = operands(key_of(cases[0]))
    verify([run(c, ops) for c in cases])


@pytest.mark.parametrize('name', list(cc.RAW_EDGE_CASES))
def test_statistics_calls_at_the_edge_of_raw(name):
    parity(cc.RAW_EDGE_CASES[name].c)


def test_pooled_only_walk_of_seven_tiles():
    parity(cc.STRAIGHT_CASES['sl1-o2-walk7'].c)


def equal(a, b):
    return torch.equal(a.d.buf, b.d.buf)


@pytest.mark.parametrize('cout', [32, 64])
@pytest.mark.parametrize('size', list(cc.ALIGNED_SIZES))
def test_straight_line_variants_equal_the_general_kernel(size, cout):
    """At every aligned size every straight-line variant repeats, bit for bit, the matching outputs of the out-mask-7 call (the general kernel) on the same
    operands: the pool taken before affine + activation with the scale's sign folded into the filter is exact, for slopes 0, 0.1 and 1, scales of both
    signs, 0 and -0.0, and shifts that saturate whole windows; slopes -0.5 and 1.5 are the fall-through.  The packed statistics add the same values
    to the same fp32 partial sums in the same order as the general kernel's; the sums of squares use a fused multiply-add where the general kernel rounds the
    product first, and the fp64 atomics arrive in another order: both are held at PACKED_RTOL relative.
    At Cout 64 the 'yp' and the affine 'ys' calls have no straight-line variant: those rows compare the general kernel with itself and show only that the
    call falls through (the route assertion); they are no cover of a variant."""
    B, H, W = cc.ALIGNED_SIZES[size][0]
    base = cc.C(B, 3, cout, H, W, 'yps')
    key = key_of(base)
    assert cc.route(base).kernel == 'general'
    for special in (False, True):
        ops = operands(key, 'randn', special)
        for slope in (0.1, 0.0, 1.0, -0.5, 1.5) if special else (0.1,):
            ref = run(base._replace(slope=slope), ops)
            assert ref.rc == OK
            for outs in ('p',) if special else ('p', 'y', 'yp', 'ys'):
                c = base._replace(outs=outs, slope=slope)
                m = cc.route(c)
                assert (m.kernel == 'straight') == (0.0 <= slope <= 1.0 and (cout == 32 or outs in ('p', 'y')))
                r = run(c, ops)
                assert r.rc == OK
                assert r.y is None or equal(r.y, ref.y), (outs, slope)
                assert r.yp is None or equal(r.yp, ref.yp), (outs, slope, special)
                if r.stats is not None:
                    close_stats(r.stats, ref.stats, cout, key)
            if special and size == 'small' and 0.0 <= slope <= 1.0:
                verify([ref], special=True)                                  # (the general kernel itself against fp64 with this affine, at the small size)
    # the training forward: raw z + statistics
    ops = operands(key)
    raw = base._replace(scale=False, shift=False, slope=1.0)
    ref, r = run(raw, ops), run(raw._replace(outs='ys'), ops)
    assert cc.variant_name(cc.route(r.c)) == 'sl%d-o5-raw' % (cout // 32) and ref.rc == OK and r.rc == OK
    assert equal(r.y, ref.y)
    close_stats(r.stats, ref.stats, cout, key)


def close_stats(got, ref, cout, key):
    """Packed against general statistics: sums and sums of squares PACKED_RTOL relative, no absolute allowance."""
    g, r = got.cpu().sum(0), ref.cpu().sum(0)
    d = ((g - r).abs() / r.abs()).view(2, cout).max(1)[0]
    print('packed against general statistics %s: sum %.3g, sum of squares %.3g relative' % (key, d[0].item(), d[1].item()))
    assert bool(((g[cout:] - r[cout:]).abs() <= PACKED_RTOL * r[cout:]).all()), d[1].item()
    assert bool(((g[:cout] - r[:cout]).abs() <= PACKED_RTOL * r[:cout].abs()).all()), d[0].item()


# ================================================================================================ 3. the mean-positive regime
@pytest.mark.parametrize('form', list(cc.MEAN_POSITIVE))
def test_mean_positive(form):
    """Inputs and filters with a positive mean: the 9 Cin products of an output have a common sign, so partial sums grow instead of cancelling.  Bound: the
    project's, or 4 x the error of torch-CPU fp32 conv2d against the same fp64 reference (the rule of tests/test_gpu_fwd.py)."""
    calls = cc.MEAN_POSITIVE[form]
    key = key_of(calls[0])
    x, w = inputs(key, 'mean-positive')[:2]
    z = next(z_chunks(key, 'mean-positive'))[2]
    floor = ((F.conv2d(x, w, padding=1).double() - z).abs().max() / z.pow(2).mean().sqrt()).item()
    bound = max(CONV_TOL, 4 * floor)
    ops = operands(key, 'mean-positive')
    err = 0.0
    for c in calls:                                                          # one at a time: the error of each against its own bound, printed before it is asserted
        e = verify([run(c, ops)], regime='mean-positive', tol=float('inf'))
        print('mean-positive %s %s: kernel %.3g, fp32 floor %.3g, bound %.3g' % (form, cc.variant_name(cc.route(c)), e, floor, bound))
        err = max(err, e)
    assert err <= bound, (err, floor)
    verify([run(c, ops) for c in calls], regime='mean-positive', tol=bound)  # (and the statistics, sentinels and finiteness at the bound itself)


# ================================================================================================ 4. statistics, deterministic mode, refusals
@pytest.mark.parametrize('name', ['general', 'packed'])
def test_statistics_accumulate(name):
    """The kernel adds to what the buffer holds: a pre-filled buffer keeps its contents, and a second call doubles the first call's contribution."""
    c = cc.C(3, 3, 20, 20, 36, 'ys') if name == 'general' else cc.C(2, 3, 32, 32, 64, 'ys', scale=False, shift=False, slope=1.0)
    assert cc.route(c).kernel == ('general' if name == 'general' else 'straight')
    key = key_of(c)
    ops = operands(key)
    pre = torch.arange(REPL * 2 * c.cout, dtype=torch.float64, device=dev()).view(REPL, -1) * 0.25 - 100.0
    st = pre.clone()
    r1 = run(c, ops, stats=st)
    torch.cuda.synchronize()
    one = (st - pre).clone()
    r1 = r1._replace(stats=one)
    verify([r1])                                                             # what the first call added is the statistics
    r2 = run(c, ops, stats=st)
    torch.cuda.synchronize()
    assert r2.rc == OK
    n = c.B * c.H * c.W
    two, want = (st - pre).sum(0).cpu(), 2 * one.sum(0).cpu()
    s2 = want[c.cout:]
    # fp64 atomics in another order: 1e-12 of sum|z| <= sqrt(N sum z^2) (and of sum z^2), far above 2^-53 x the 3,200 added to every entry
    assert bool(((two[c.cout:] - s2).abs() <= 1e-12 * s2 + 1e-9).all()), 'sum of squares'
    assert bool(((two[:c.cout] - want[:c.cout]).abs() <= 1e-12 * (s2 * n).sqrt() + 1e-9).all()), 'sum'
    assert int((one.abs().sum(1) > 0).sum()) == min(REPL, cc.route(c).grid), 'the replicated rows: workgroup index mod Y2_STATS_REPL'


@pytest.mark.parametrize('name', ['general', 'straight'])
def test_deterministic_mode(name):
    """Statistics from atomics are refused (-3) and nothing is written; the same call without statistics is bit-identical to default mode; the mode is off
    afterwards."""
    import _hip
    c = cc.C(2, 3, 20, 18, 34, 'yps') if name == 'general' else cc.C(2, 3, 32, 32, 64, 'ys', scale=False, shift=False, slope=1.0)
    ops = operands(key_of(c))
    plain = [run(c._replace(outs=o), ops) for o in ('y', 'p', 'yp')]
    torch.cuda.synchronize()
    with deterministic():
        r = run(c, ops)
        torch.cuda.synchronize()
        assert r.rc == ENOSUP == cc.route(c._replace(det=True)).rc
        assert all(d is None or d.untouched() for d in (r.y, r.yp)) and not bool(r.stats.any())
        again = [run(c._replace(outs=o), ops) for o in ('y', 'p', 'yp')]
        torch.cuda.synchronize()
    for a, b in zip(plain, again):
        assert a.rc == b.rc == OK and (a.y is None or equal(a.y, b.y)) and (a.yp is None or equal(a.yp, b.yp))
    verify([again[2]])
    assert not _hip.lib().y2_get_deterministic()


@pytest.mark.parametrize('name', list(cc.REFUSALS))
def test_refusals_return_their_code_and_leave_the_destinations_alone(name):
    import _hip
    c, rc = cc.REFUSALS[name]
    ops = operands(key_of(c._replace(B=min(c.B, 4))))
    if c.det:
        with deterministic():
            r = run(c, ops)
            torch.cuda.synchronize()
        assert not _hip.lib().y2_get_deterministic()
    else:
        r = run(c, ops)
        torch.cuda.synchronize()
    assert r.rc == rc == cc.route(c).rc
    assert all(d is None or d.untouched() for d in (r.y, r.yp)) and (r.stats is None or not bool(r.stats.any()))


# ================================================================================================ 5. the small kernels at the same boundary
@pytest.mark.parametrize('B,C,H,W,ld', [(2, 3, 9, 7, 3), (2, 3, 9, 7, 4), (1, 1, 5, 6, 1), (2, 4, 6, 5, 7), (3, 3, 300, 300, 4)])      # the last: 1,080,000 elements, the grid-stride loop's third pass
def test_nchw_to_nhwc(B, C, H, W, ld):
    import _hip
    assert (B * H * W * ld > 2 * 524288) == (H == 300)
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(C + H + ld))
    keep, xp = guarded(x)
    y = Dest(B * H * W * ld)
    assert _hip.lib().y2_nchw_to_nhwc(xp, y.ptr, B, C, H, W, ld, _hip.stream()) == OK
    torch.cuda.synchronize()
    got = y.t.view(B, H, W, ld).cpu()
    assert y.guards_intact()
    assert torch.equal(got[..., :C], x.permute(0, 2, 3, 1))
    assert torch.equal(got[..., C:].contiguous().view(torch.int32), torch.zeros(B, H, W, ld - C, dtype=torch.int32))       # pad channels: +0.0 exactly
    bad = Dest(16)
    assert _hip.lib().y2_nchw_to_nhwc(xp, bad.ptr, B, C, H, W, C - 1, _hip.stream()) == EINVAL and bad.untouched()


POOL_CASES = collections.OrderedDict([
    # name: (B, H, W, C, pad and offset of x's rows, ldy - C, floats y is off its 16-byte boundary, vector path)
    ('vector', (2, 8, 12, 16, (8, 4), 4, 0, True)),
    ('vector-dense', (3, 2, 2, 4, (0, 0), 0, 0, True)),
    ('scalar-C%4', (2, 8, 12, 6, (2, 0), 2, 0, False)),
    ('scalar-ldx%4', (2, 8, 12, 8, (2, 0), 4, 0, False)),
    ('scalar-ldy%4', (2, 8, 12, 8, (4, 0), 1, 0, False)),
    ('scalar-x-off-by-one', (2, 8, 12, 8, (4, 1), 4, 0, False)),
    ('scalar-y-off-by-one', (2, 8, 12, 8, (4, 0), 4, 1, False)),
    ('vector-above-the-grid-cap', (2, 130, 130, 256, (4, 4), 4, 0, True)),             # 540,800 threads' worth of work on 524,288 threads
    ('scalar-above-the-grid-cap', (2, 130, 130, 63, (1, 0), 1, 0, False)),             # 532,350
])


@pytest.mark.parametrize('name', list(POOL_CASES))
def test_maxpool2(name):
    import _hip
    B, H, W, C, (pad, off), ypad, yshift, vec = POOL_CASES[name]
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(H + C))
    xo = Operand(nhwc(x), pad, off)
    ldy = C + ypad
    rows = B * (H // 2) * (W // 2)
    y = Dest(rows * ldy + 4)
    yptr = ctypes.c_void_p(y.t.data_ptr() + 4 * yshift)
    assert vec == (C % 4 == 0 and xo.ld % 4 == 0 and ldy % 4 == 0 and xo.ptr.value % 16 == 0 and yptr.value % 16 == 0)
    assert ('cap' in name) == (rows * (C // 4 if vec else C) > 524288)
    assert _hip.lib().y2_maxpool2_fwd(xo.ptr, yptr, B, H, W, C, xo.ld, ldy, _hip.stream()) == OK
    torch.cuda.synchronize()
    assert y.guards_intact() and bool((y.t[:yshift] == SENT).all()) and bool((y.t[yshift + rows * ldy:] == SENT).all())
    got = y.t[yshift:yshift + rows * ldy].view(B, H // 2, W // 2, ldy).cpu()
    assert bool((got[..., C:] == SENT).all()), 'wrote past C'
    assert torch.equal(got[..., :C].permute(0, 3, 1, 2), F.max_pool2d(x, 2))


@pytest.mark.parametrize('H,W', [(7, 12), (8, 11)])
def test_maxpool2_refuses_odd_sizes(H, W):
    import _hip
    xo = Operand(torch.randn(2, H, W, 8))
    y = Dest(2 * 4 * 6 * 8)
    assert _hip.lib().y2_maxpool2_fwd(xo.ptr, y.ptr, 2, H, W, 8, 8, 8, _hip.stream()) == EINVAL
    torch.cuda.synchronize()
    assert y.untouched()


@pytest.mark.parametrize('C', [1, 255, 257])
def test_bn_fold(C):
    """scale = gamma / sqrt(var + eps), shift = beta - mean * scale in fp32: an addition, a square root, a division (1.5 ulp together: 1.8e-7 on the scale), a
    product and a subtraction (half an ulp each of |mean * scale| and of the result): about 3e-7 in all, held at 1e-6.  Variances of 0 and 1e-12: eps alone."""
    import _hip
    g = torch.Generator().manual_seed(C)
    gamma, beta, mean = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g) * 3
    var = torch.rand(C, generator=g) * 4 + 1e-3
    var[0] = 0.0
    if C > 1:
        var[1], var[C - 1] = 1e-12, 0.0
    eps = 1e-5
    bufs = [guarded(t) for t in (gamma, beta, mean, var)]
    scale, shift = Dest(C), Dest(C)
    assert _hip.lib().y2_bn_fold(bufs[0][1], bufs[1][1], bufs[2][1], bufs[3][1], eps, scale.ptr, shift.ptr, C, _hip.stream()) == OK
    torch.cuda.synchronize()
    assert scale.guards_intact() and shift.guards_intact()
    s64 = gamma.double() / (var.double() + f32(eps)).sqrt()
    h64 = beta.double() - mean.double() * s64
    s, h = scale.t.cpu().double(), shift.t.cpu().double()
    assert bool(torch.isfinite(s).all()) and bool(torch.isfinite(h).all())
    assert bool(((s - s64).abs() <= 1e-6 * s64.abs()).all()), ((s - s64).abs() / s64.abs()).max().item()
    assert bool(((h - h64).abs() <= 1e-6 * (beta.double().abs() + (mean.double() * s64).abs())).all())
    none = Dest(C)
    assert _hip.lib().y2_bn_fold(bufs[0][1], bufs[1][1], bufs[2][1], None, eps, none.ptr, none.ptr, C, _hip.stream()) == EINVAL and none.untouched()
