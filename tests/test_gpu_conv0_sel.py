"""GPU parity tests of y2_conv0_fwd_sel, the first layer's training forward as the producer of z_sel (csrc/conv0_fwd.hip), one dispatch
path at a time: the ninth straight-line variant <3, 1, 7, FULL, RAW>, and the general kernel with a.pool_sign for every other call - without
statistics (the call of a deterministic-mode user), Cout 64, rows wider than Cout, every Cin, every channel mask, ragged tiles, a persistent walk.
tests/conv0_cases.py holds the cases (SEL_CASES, SEL_REFUSALS) and the mirror of the dispatch; tests/test_conv0_cases.py checks them on the CPU.

Ground rules as in tests/test_gpu_conv0.py: x, the filter and gamma are windows of NaN-guarded allocations; z and z_sel are channel windows of rows of
-7.0 between -7.0 guards, and all of that must survive.  Two input regimes:

  exact    x = k / 4, w = k / 8 with |k| <= 4 and one all-zero output channel: every product is a multiple of 1 / 32 and every partial sum stays below 2^24 / 32,
           so each sum is exact in fp32 in ANY order.  z must equal the fp64 F.conv2d bit for bit (-0 and +0 counted equal), z_sel the header's
           definition applied to that reference, and the statistics the reference's fp64 sums (z^2 is a multiple of 1 / 1024 below 183: a tile's 32 terms per
           lane are exact in fp32 as well).  That torch-CPU fp32 F.conv2d equals the fp64 one is asserted on every chunk, so the regime cannot stop being
           exact unnoticed.  Windows whose extreme is held by two elements are 1 - 3 % of all here (their presence is asserted), so the first-extreme rule is
           exercised in every case.
  random   (the small cases) z against fp64 within the bound of tests/test_gpu_conv0.py; z_sel against the definition applied to the launch's own z.

In both, z_sel is ALSO compared bit for bit with the definition applied to the launch's own z, and z and the statistics with those of the plain
y2_conv0_fwd(x, w, NULL, NULL, z, NULL, stats, ..., 1.0) launch.  Every gamma vector has both signs, an exact zero and a -0.0 (Cout 1: one launch each).
The definition is written with torch.where on the device, not as the kernel's loop."""
import collections
import functools

import pytest
import torch
import torch.nn.functional as F

import conv0_cases as cc
from test_gpu_conv0 import CHUNK_ELEMS, CONV_TOL, PACKED_RTOL, REPL, Acc, Out, guarded, inputs, key_of
from test_gpu_wgrad import deterministic, dev

pytestmark = pytest.mark.gpu
OK = cc.OK
GAMMA = (1.5, -0.75, 0.0, -0.0, -2.0, 0.25, 3.0)          # repeated over the channels: both signs, +0 and -0 within any four neighbours


def zero_channel(cout):
    """The output channel whose filter is all zero (every window of it a four-way tie); a one-channel layer has none."""
    return None if cout == 1 else min(5, cout - 1)


def gamma_of(cout, rot=0):
    g = torch.tensor([GAMMA[(i + rot) % len(GAMMA)] for i in range(cout)], dtype=torch.float32)
    if cout >= 4:
        bits = g.view(torch.int32)
        assert bool((g > 0).any()) and bool((g < 0).any()) and bool((bits == 0).any()) and bool((bits == -(1 << 31)).any())
    return g


@functools.lru_cache(maxsize=2)
def operands_of(key, regime):
    """(x, w) in fp32 on the CPU, read only."""
    B, cin, cout, H, W = key
    if regime == 'exact':
        g = torch.Generator().manual_seed(7 + 1000003 * (B % 1009) + 10007 * cin + 101 * cout + 13 * H + 7 * W)
        x = torch.randint(-4, 5, (B, cin, H, W), generator=g).float() / 4
        w = torch.randint(-4, 5, (cout, cin, 3, 3), generator=g).float() / 8
    else:
        x, w = inputs(key)[:2]
        w = w.clone()
    if zero_channel(cout) is not None:
        w[zero_channel(cout)] = 0.0
    return x, w


def reference_chunks(key, regime):
    """(b0, b1, fp64 convolution of images b0 .. b1 [n,C,H,W] on the CPU)."""
    B, cin, cout, H, W = key
    x, w = operands_of(key, regime)
    nb = max(1, CHUNK_ELEMS // (cout * H * W))
    for b0 in range(0, B, nb):
        z = F.conv2d(x[b0:b0 + nb].double(), w.double(), padding=1)
        if regime == 'exact':
            assert torch.equal(F.conv2d(x[b0:b0 + nb], w, padding=1).double(), z), 'the exact regime is not exact: fp32 and fp64 convolutions differ'
        yield b0, min(B, b0 + nb), z


def definition(z, gamma):
    """The header's z_sel of z [n,H,W,C] (any float type, on the device): per window and channel the FIRST z_q in scan order that maximises sign(gamma) * z_q
    under a strict comparison."""
    s = (gamma > 0).to(z.dtype) - (gamma < 0).to(z.dtype)
    win = [z[:, 0::2, 0::2], z[:, 0::2, 1::2], z[:, 1::2, 0::2], z[:, 1::2, 1::2]]
    best, sel = s * win[0], win[0]
    for q in (1, 2, 3):
        key = s * win[q]
        m = key > best
        best, sel = torch.where(m, key, best), torch.where(m, win[q], sel)
    return sel


def tie_fraction(z, gamma, cout):
    """Share of the (window, channel) pairs, over the channels with gamma != 0 and a filter, whose extreme is held by two or more elements."""
    sel = definition(z, gamma)
    n = sum((z[:, i::2, j::2] == sel).int() for i in (0, 1) for j in (0, 1))
    use = gamma != 0
    if zero_channel(cout) is not None:
        use[zero_channel(cout)] = False
    return (n[..., use] >= 2).float().mean().item()


Sel = collections.namedtuple('Sel', 'rc z zs stats')


def launch(c, ptrs, sel=True):
    """y2_conv0_fwd_sel as c describes it, or (sel=False) the plain launch the header names: y2_conv0_fwd(x, w, NULL, NULL, z, NULL, stats, ..., ldz, 0, 1.0)."""
    import _hip
    L = _hip.lib()
    x, w, gm = ptrs
    B, cin, cout, H, W = key_of(c)
    B = min(B, 4) if c.B > 1 << 20 else B                                   # (a refusal by size: the destinations are never reached)
    z = Out(B * H * W, cout, c.ypad, c.yoff) if 'y' in c.outs else None
    zs = Out(B * max(H // 2, 1) * max(W // 2, 1), cout, c.ppad, c.poff) if 'p' in c.outs and sel else None
    st = torch.zeros(REPL, 2 * cout, dtype=torch.float64, device=dev()) if 's' in c.outs else None
    if sel:
        rc = L.y2_conv0_fwd_sel(None if c.nox else x, None if c.now else w, None if c.nog else gm, z.ptr if z else None, zs.ptr if zs else None, _hip.ptr(st),
                                c.B, c.H, c.W, c.cin, c.cout, c.cout + c.ypad, c.cout + c.ppad, _hip.stream())
    else:
        rc = L.y2_conv0_fwd(x, w, None, None, z.ptr, None, _hip.ptr(st), c.B, c.H, c.W, c.cin, c.cout, c.cout + c.ypad, 0, 1.0, _hip.stream())
    return Sel(rc, z, zs, st)


def same_statistics_form(c):
    """Whether the sel launch and the plain one sum their statistics in the same form (packed fp32 pairs with a fused multiply-add in the straight-line
    variants, one rounded product at a time in the general kernel: tests/test_gpu_conv0.py holds the two forms together at PACKED_RTOL)."""
    return cc.route(c).kernel == cc.route(c._replace(sel=False, outs=c.outs.replace('p', ''))).kernel


def check(c, regime):
    assert cc.route(c).rc == OK and c.sel
    key = key_of(c)
    B, cin, cout, H, W = key
    x, w = operands_of(key, regime)
    keep = [guarded(x), guarded(w)]
    for rot in range(4 if cout < 4 else 1):
        gamma = gamma_of(cout, rot)
        gkeep, gptr = guarded(gamma)
        gd = gamma.to(dev())
        ptrs = (keep[0][1], keep[1][1], gptr)
        r, plain = launch(c, ptrs), launch(c, ptrs, sel=False)
        torch.cuda.synchronize()
        assert r.rc == OK and plain.rc == OK, (r.rc, plain.rc)
        z, zs = r.z.window().view(B, H, W, cout), r.zs.window().view(B, H // 2, W // 2, cout)
        # ---- z_sel is one of the launch's own four z, the defined one: bit for bit
        assert torch.equal(definition(z, gd).view(torch.int32), zs.view(torch.int32)), 'z_sel is not the definition applied to the launch\'s own z'
        # ---- z and the statistics are the plain launch's (values: the plain launch's general kernel passes z through an identity affine, -0 -> +0)
        assert torch.equal(z, plain.z.window().view(B, H, W, cout)), 'z differs from the plain launch\'s'
        if zero_channel(cout) is not None:
            assert bool((z[..., zero_channel(cout)] == 0).all())
        if r.stats is not None:
            got, ref = r.stats.sum(0).cpu(), plain.stats.sum(0).cpu()
            assert bool(torch.isfinite(got).all())
            rtol = 1e-12 if regime == 'exact' or same_statistics_form(c) else PACKED_RTOL
            print('statistics against the plain launch: %.3g relative (bound %g)' % (((got - ref).abs() / ref.abs().clamp_min(1e-300)).max().item(), rtol))
            assert bool(((got - ref).abs() <= rtol * ref.abs()).all()), 'statistics differ from the plain launch\'s'
        # ---- against the fp64 reference
        if regime == 'exact' and B <= cc.SEL_RANDOM_MAX_B and B * (H // 2) * (W // 2) >= 100 and cout >= 4:
            t = tie_fraction(z, gd, cout)
            print('windows with a tie at the extreme: %.1f %%' % (100 * t))
            assert t >= 0.005, 'the exact regime no longer ties'          # (1.3 - 3 % on these shapes: z lies on a grid of 1 / 32 a few hundred values wide; asked: present in number)
        acc = Acc()
        s1, s2 = torch.zeros(cout, dtype=torch.float64), torch.zeros(cout, dtype=torch.float64)
        for b0, b1, z64 in reference_chunks(key, regime):
            if regime == 'exact':
                e = z64.to(dev()).permute(0, 2, 3, 1)
                assert torch.equal(z[b0:b1].double(), e), 'z is not the fp64 convolution'
                assert torch.equal(zs[b0:b1].double(), definition(e, gd.double())), 'z_sel is not the definition applied to the fp64 convolution'
                s1 += z64.sum((0, 2, 3))
                s2 += (z64 * z64).sum((0, 2, 3))
            else:
                acc.add(z[b0:b1], z64)
        if regime == 'exact' and r.stats is not None:
            got = r.stats.sum(0).cpu()
            assert bool(((got[:cout] - s1).abs() <= 1e-12 * s1.abs()).all()) and bool(((got[cout:] - s2).abs() <= 1e-12 * s2).all()), 'statistics are not the reference\'s sums'
        if regime != 'exact':
            print('z against fp64: %.3g x rms' % acc.rel())
            assert acc.rel() <= CONV_TOL, acc.rel()


@pytest.mark.parametrize('name', list(cc.SEL_CASES))
def test_sel_exact(name):
    check(cc.SEL_CASES[name].c, 'exact')


@pytest.mark.parametrize('name', [n for n, c in cc.SEL_CASES.items() if c.c.B <= cc.SEL_RANDOM_MAX_B])
def test_sel_random(name):
    check(cc.SEL_CASES[name].c, 'random')


@pytest.mark.parametrize('name', ['sel-nostats-aligned', 'sel-nostats-ragged'])
def test_sel_without_statistics_in_deterministic_mode(name):
    """What a deterministic-mode user of the ABI calls (statistics are refused there, so stats is NULL): accepted, and everything check() asks."""
    import _hip
    c = cc.SEL_CASES[name].c
    assert 's' not in c.outs and cc.route(c._replace(det=True)).rc == OK and cc.route(c._replace(det=True, outs='yps')).rc == cc.ENOSUP
    with deterministic():
        check(c, 'exact')
    assert not _hip.lib().y2_get_deterministic()


@pytest.mark.parametrize('name', list(cc.SEL_REFUSALS))
def test_sel_refusals_return_their_code_and_leave_the_destinations_alone(name):
    """Every pointer is valid but the one under test."""
    import _hip
    c, rc = cc.SEL_REFUSALS[name]
    key = key_of(c._replace(B=min(c.B, 4)))
    x, w = operands_of(key, 'exact')
    keep = [guarded(x), guarded(w), guarded(gamma_of(key[2]))]
    ptrs = tuple(k[1] for k in keep)
    if c.det:
        with deterministic():
            r = launch(c, ptrs)
            torch.cuda.synchronize()
        assert not _hip.lib().y2_get_deterministic()
    else:
        r = launch(c, ptrs)
        torch.cuda.synchronize()
    assert r.rc == rc == cc.route(c).rc
    assert all(d is None or d.untouched() for d in (r.z, r.zs)) and (r.stats is None or not bool(r.stats.any()))
