"""CPU check of the case table of the fused BatchNorm-backward + 4x4-tile transform tests (tests/bnwino6_cases.py): the table reaches every route the
mirror knows, the mirror's tile counts are those of the built library (y2_wino6_tiles), its constants are the source text of csrc/train.hip and
csrc/common.h, and the fp64 statement of the V6 / M6 layout contract that the GPU tests (tests/test_gpu_bnwino6.py) compare the kernel with reproduces
torch's fp64 data and weight gradients of conv2d when it is pushed through the rest of the two Winograd algorithms - with matrices derived here
from the interpolation points, not taken from the kernels."""
import os
import random
import re
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bnwino6_cases as bc
import wgrad_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'yolo2-pytorch_amd', 'csrc')


# ------------------------------------------------------------------------------------------------ the table
def test_table_reaches_every_route():
    missing = set(bc.REQUIRED) - bc.reached()
    assert not missing, 'no case reaches: %s' % sorted(missing)


def test_removing_a_sole_case_is_noticed():
    """Each of these routes hangs on one case: without it the set difference names the route."""
    for name, routes in (('park16-b16-26x26-c400', {'parked in v6, 16 slices'}), ('grid17', {'parked at 17 workgroups'}), ('grid16', {'atomics at 16 workgroups'}),
                         ('misaligned-park-m6', {'atomics>16 by misalignment of m6'}),
                         ('park1-scalar', {'parked, scalar pass 1'}), ('scalar-ldz', {'scalar by ldz alone'}), ('b2-4x12-v6', {'v6 only'})):
        rest = {n: c for n, c in bc.CASES.items() if n != name}
        missing = set(bc.REQUIRED) - bc.reached(rest)
        assert routes <= missing, (name, sorted(missing))


@pytest.mark.parametrize('name', list(bc.CASES))
def test_case_reaches_what_its_name_says(name):
    c, r = bc.CASES[name], bc.route(bc.CASES[name])
    words = name.split('-')
    for word, ok in (('tall', r.form == 'tall'), ('mosaic', r.form == 'mosaic'), ('phantom', r.phantom), ('scalar', r.pass1 == 'scalar'), ('c6', c.C == 6 and r.pass1 == 'scalar'),
                     ('park1', r.sums.startswith('parked') and r.sums.endswith(':1')), ('park4', r.sums.endswith(':4')), ('park16', r.sums.endswith(':16')),
                     ('misaligned', r.sums == 'atomics>16'), ('m6', c.out == 'm6'), ('v6', c.out == 'v6'), ('grid16', r.grid == 16 and r.sums == 'atomics'),
                     ('grid17', r.grid == 17 and r.sums == 'parked-v6:1'), ('bn0', c.has_bn == 0)):
        if word in words:
            assert ok, (word, r)
    assert bc.refusal(c) == bc.OK
    assert c.affine or c.has_bn == 0                                 # scale / shift may be NULL without BatchNorm only
    assert c.cin % 4 == 0 and (c.cin == 0 or c.C % 4 == 0)           # the consumers take multiples of 4 channels
    assert (r.grid * bc.THREADS) % (c.C // 4 if r.pass1 == 'vector' else c.C) == 0
    assert r.items <= bc.ITEMS                                       # no case on the capped grid: K = items + 256 <= 264
    # small enough for a test of a few seconds: only the 16-slice case is megabytes large
    assert c.B * c.H * c.W * c.C <= (1 << 20) or name.startswith('park16')
    assert (36 * r.T * c.C * 4 <= 64 << 20)


def test_mirror_known_answers():
    assert bc.act_grid(1, 1) == 1 and bc.act_grid(2049, 1) == 2 and bc.act_grid(10 ** 9, 32) == 2048
    assert bc.act_grid(1521 * 6, 6) == 6 and bc.act_grid(100, 6) == 3 and bc.act_grid(16 * 26 * 26 * 100, 100) == 550
    # common.h: 64 images of 13x13 as 8 x 8 -> 28 x 28 = 784 tiles instead of 1024; 26x26: 3136 -> 2916
    assert wc.wino6_grid(64, 13, 13).T == 784 and wc.wino6_grid(64, 26, 26).T == 2916
    r = bc.route(bc.Case(9, 13, 13, 32))
    assert (r.form, r.phantom, r.gx, r.gy, r.th, r.tw, r.T) == ('mosaic', False, 3, 3, 11, 11, 121)
    r = bc.route(bc.Case(11, 13, 13, 32))
    assert (r.form, r.phantom, r.gx * r.gy) == ('mosaic', True, 12)
    assert bc.route(bc.Case(11, 13, 13, 32), tall_allowed=False).T == 11 * 16
    assert bc.route(bc.Case(1, 13, 13, 32)).form == 'per-image' and bc.route(bc.Case(2, 8, 8, 8)).form == 'per-image'
    # the refusals of the entry point
    assert bc.refusal(bc.Case(2, 8, 8, 8, ldz=-1)) == bc.EINVAL and bc.refusal(bc.Case(2, 8, 8, 8, fpad=-1)) == bc.EINVAL
    assert bc.refusal(bc.Case(2, 8, 8, 8, out='none')) == bc.EINVAL and bc.refusal(bc.Case(2, 8, 8, 8), deterministic=True) == bc.ENOSUP


# ------------------------------------------------------------------------------------------------ the mirror against the library and the sources
def library():
    import _hip
    try:
        return _hip.lib()
    except _hip.HipLibraryMissing:
        pytest.skip('libyolo2_hip.so is not built')


def test_tile_counts_are_the_library_s():
    L = library()
    for name, c in bc.CASES.items():
        assert L.y2_wino6_tiles(c.B, c.H, c.W) == bc.route(c).T, name
    rnd = random.Random(5)
    for _ in range(4000):
        B, H, W = rnd.randint(1, 70), rnd.randint(1, 60), rnd.randint(1, 60)
        assert L.y2_wino6_tiles(B, H, W) == wc.wino6_grid(B, H, W).T, (B, H, W)
    for args in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        assert L.y2_wino6_tiles(*args) == bc.EINVAL


def test_mirror_constants_are_the_sources():
    """Literal matches against the text of train.hip and common.h.  They fail on any edit of the matched lines; when this test fails, re-read route() in
    bnwino6_cases.py against act_grid, bn_act_bwd_impl and y2_bn_act_bwd_wino6 before updating the strings here."""
    common = open(os.path.join(CSRC, 'common.h')).read()
    src = open(os.path.join(CSRC, 'train.hip')).read()
    header = open(os.path.join(ROOT, 'include', 'yolo2_hip.h')).read()
    assert int(re.search(r'constexpr int Y2_NUM_CU = (\d+);', common).group(1)) == bc.NUM_CU
    # act_grid: 256 threads, 8 items per thread, at most 8 workgroups per CU
    grid_fn = src[src.index('inline int act_grid(long long total, int Cg) {'):]
    grid_fn = grid_fn[:grid_fn.index('\n}\n')]
    assert 'int g = %d, r = Cg;' % bc.THREADS in grid_fn
    assert 'long long want = (total + %d * %d - 1) / (%d * %d);' % (bc.THREADS, bc.ITEMS, bc.THREADS, bc.ITEMS) in grid_fn
    assert 'const long long cap = (long long)Y2_NUM_CU * %d;' % bc.WG_PER_CU in grid_fn
    assert 'return (int)(((want + unit - 1) / unit) * unit);' in grid_fn
    impl = src[src.index('static int bn_act_bwd_impl('):src.index('extern "C" int y2_bn_act_bwd_ex(')]
    assert '(bn_act_bwd_kernel<POOL, CV, false>), dim3(grid), dim3(%d), lds, s, a, total);' % bc.THREADS in impl
    # vector pass 1
    assert '!(C & 3) && !(ldz & 3) && (!dz || (!(ldd & 3) && y2_aligned16(dz))) && y2_aligned16(z) &&' in impl
    assert '(!dy_full || (!(ldf & 3) && !(foff & 3) && y2_aligned16(dy_full)))' in impl
    assert 'const int Cg = vec ? C / 4 : C;' in impl and 'const int grid = act_grid(total, Cg);' in impl
    # where the partial sums go
    assert ('if (dz == nullptr && park != nullptr && !y2_det.on && grid > %d && (long long)grid * 2 * C <= park_floats && y2_aligned16(park)) a.block_partial = park;'
            % bc.PARK_MIN_GRID) in impl
    assert '(unsigned)(grid >= %d ? 16 : (grid >= %d ? 4 : 1))' % (bc.SLICE_16, bc.SLICE_4) in impl
    entry = src[src.index('extern "C" int y2_bn_act_bwd_wino6('):src.index('extern "C" int y2_bn_act_fwd(')]
    assert 'float* park = v6 != nullptr ? v6 : m6;' in entry and 'sums, nullptr, 0, B, H, W, C, ldz, has_bn, stream, park, 36LL * g6.T * C)) return rc;' in entry
    assert 'bn_bwd_wino6_kernel, dim3((unsigned)y2_cdiv(g6.T * C, %d)), dim3(%d), 0, y2_s(stream), a);' % (bc.THREADS, bc.THREADS) in entry
    # the refusals, in order
    returns = re.findall(r'if \((.*)\) return (Y2_E\w+);', entry)
    assert [r[1] for r in returns[:3]] == ['Y2_EINVAL', 'Y2_EINVAL', 'Y2_ENOSUP']
    assert returns[0][0] == '!z || !dy_full || !sums || (v6 == nullptr && m6 == nullptr) || B <= 0 || H <= 0 || W <= 0 || C <= 0 || ldz < C || ldf < foff + C'
    assert returns[1][0] == 'dz != nullptr && ldd < C' and returns[2][0] == 'y2_det.on'
    assert 'if (has_bn < 0 || has_bn > 2 || (has_bn && (!mean || !invstd || !gamma))) return Y2_EINVAL;' in impl
    for name, val in (('Y2_OK', bc.OK), ('Y2_EINVAL', bc.EINVAL), ('Y2_EALIGN', bc.EALIGN), ('Y2_ENOSUP', bc.ENOSUP)):
        assert int(re.search(r'%s\s*=?\s*\(?(-?\d+)' % name, header).group(1)) == val, name


# ------------------------------------------------------------------------------------------------ the layout contract against conv2d
POINTS = [Fraction(0), Fraction(1), Fraction(-1), Fraction(2), Fraction(-1, 2)]          # and infinity


def toom_cook(m, r):
    """A^T [m x 6] and G [6 x r] of F(m, r), m + r - 1 = 6, on POINTS and infinity (Lavin & Gray's construction): A^T[k][i] = p_i^k,
    G[i][k] = p_i^k / prod_{j != i} (p_i - p_j); the column / row of infinity picks the highest power."""
    assert m + r - 1 == 6
    at = np.zeros((m, 6))
    g = np.zeros((6, r))
    for i, p in enumerate(POINTS):
        n = Fraction(1)
        for j, q in enumerate(POINTS):
            if j != i:
                n *= p - q
        for k in range(m):
            at[k][i] = float(p ** k)
        for k in range(r):
            g[i][k] = float(p ** k / n)
    at[m - 1][5] = 1.0
    g[5][r - 1] = 1.0
    return at, g


def test_transform_matrices_follow_from_the_interpolation_points():
    """B^T is determined by A^T and G: sum_i A^T[k][i] G[i][j] B^T[i][l] = [l == k + j] for every output k, tap j and input l.  Solved here for both
    algorithms, the solutions agree with each other and with the table's B^T; the table's G (6 x 4) is the G of F(3, 4)."""
    for m, r in ((4, 3), (3, 4)):
        at, g = toom_cook(m, r)
        rows = np.array([[at[k][i] * g[i][j] for i in range(6)] for k in range(m) for j in range(r)])          # [m * r, 6]
        rhs = np.array([[1.0 if l == k + j else 0.0 for l in range(6)] for k in range(m) for j in range(r)])   # [m * r, 6]
        bt, res, rank, _ = np.linalg.lstsq(rows, rhs, rcond=None)
        assert rank == 6 and np.abs(rows @ bt - rhs).max() < 1e-12
        np.testing.assert_allclose(bt, bc.BT, rtol=0, atol=1e-12)
    np.testing.assert_allclose(toom_cook(3, 4)[1], bc.GM, rtol=0, atol=1e-15)


def untile(tiles, r, B, H, W):
    """[T, 4, 4, C] output tiles of route r's grid -> [B, H, W, C] (the inverse of the tile -> pixel map of bc.patches)."""
    C = tiles.shape[-1]
    n = B if r.form == 'per-image' else 1
    canvas = tiles.reshape(n, r.th, r.tw, 4, 4, C).transpose(0, 1, 3, 2, 4, 5).reshape(n, 4 * r.th, 4 * r.tw, C)
    if r.form == 'per-image':
        return canvas[:, :H, :W]
    out = np.empty((B, H, W, C))
    for b in range(B):
        by, bx = divmod(b, r.gx)
        out[b] = canvas[0, by * (H + 1):by * (H + 1) + H, bx * (W + 1):bx * (W + 1) + W]
    return out


CONTRACT_SHAPES = [(1, 1, 1, True), (1, 5, 7, True), (2, 8, 8, True), (3, 1, 1, True), (3, 5, 4, True), (2, 7, 9, True), (5, 6, 5, True), (9, 13, 13, True), (11, 13, 13, True),
                   (2, 3, 2, True), (4, 6, 6, True), (5, 6, 5, False), (11, 13, 13, False)]


@pytest.mark.parametrize('B,H,W,tall_allowed', CONTRACT_SHAPES)
def test_layout_contract_reproduces_the_gradients_of_conv2d(B, H, W, tall_allowed):
    """V6 and M6 as bc.v6_m6_reference states them, pushed through the rest of F(4x4, 3x3) and F(3x3, 4x4): sum over channels of V6 * U6 and the
    inverse transform give x.grad of conv2d, sum over tiles of M6 * (B^T x B) and the inverse transform give w.grad, both in fp64 to 1e-12.  A V6 / M6
    with anything but zero at the separators, outside the images or in a phantom image, or with another tile order, fails this."""
    cin, cout = 3, 4
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + W)
    x = torch.randn(B, cin, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    dz = torch.randn(B, cout, H, W, generator=g, dtype=torch.float64)
    F.conv2d(x, w, padding=1).backward(dz)
    r = bc.route(bc.Case(B, H, W, cout), tall_allowed=tall_allowed)
    assert (r.form == 'per-image') or tall_allowed
    dz_nhwc = dz.permute(0, 2, 3, 1).numpy()
    v6, m6 = bc.v6_m6_reference(dz_nhwc, r)
    assert v6.shape == m6.shape == (36, r.T, cout)
    # ---- data gradient: correlation of dz with k[ci][co][a][b] = w[co][ci][2 - a][2 - b]
    at4, g3 = toom_cook(4, 3)
    k = w.detach().numpy()[:, :, ::-1, ::-1].transpose(1, 0, 2, 3)                                # [ci, co, 3, 3]
    u6 = np.einsum('ua,ioab,vb->uvio', g3, k, g3).reshape(36, cin, cout)
    mo = np.einsum('ptc,pic->pti', v6, u6).reshape(6, 6, r.T, cin)
    tiles = np.einsum('yu,uvti,xv->tyxi', at4, mo, at4)
    dx = untile(tiles, r, B, H, W)
    np.testing.assert_allclose(dx, x.grad.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-12)
    # ---- weight gradient
    at3, g4 = toom_cook(3, 4)
    vx = bc.v6_m6_reference(x.detach().permute(0, 2, 3, 1).numpy(), bc.route(bc.Case(B, H, W, cin), tall_allowed=tall_allowed))[0]
    du = np.einsum('pto,pti->poi', m6, vx).reshape(6, 6, cout, cin)
    dw = np.einsum('au,uvoi,bv->oiab', at3, du, at3)
    np.testing.assert_allclose(dw, w.grad.numpy(), rtol=0, atol=1e-11)
    # ---- structural zeros: exactly where no pixel of an image contributes
    zv, zm = bc.structural_zeros(B, H, W, r)
    assert (v6[zv] == 0).all() and (m6[zm] == 0).all()
    if (B, H, W, tall_allowed) == (11, 13, 13, True):
        assert zv.all(0).sum() >= 3 and zm.all(0).sum() >= 3     # the place of the twelfth image: tiles without any pixel
    ones = bc.v6_m6_reference(np.ones((B, H, W, 1)), r)
    assert (ones[1][0][~zm[0]] != 0).all()                       # (position (0, 0) of M6 is the tile's first pixel itself)


def test_fp32_statement_is_the_fp64_one_rounded():
    """The floor of the GPU tests is the same chain in fp32: same function, dtype float32."""
    r = bc.route(bc.Case(5, 6, 5, 4))
    d = np.random.RandomState(3).randn(5, 6, 5, 4).astype(np.float32)
    v64, m64 = bc.v6_m6_reference(d, r)
    v32, m32 = bc.v6_m6_reference(d, r, np.float32)
    assert v32.dtype == m32.dtype == np.float32
    assert np.abs(v32 - v64).max() < 1e-5 and np.abs(m32 - m64).max() < 1e-5
    assert np.abs(v32 - v64).max() > 0
