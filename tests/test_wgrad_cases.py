"""CPU check of the weight-gradient case tables (tests/wgrad_cases.py): the mirror of the host code's dispatch agrees with what every case
claims to reach, and the tables as a whole cover the dispatch matrix of csrc/conv_wgrad.hip and the Winograd drivers of csrc/wino.hip.  The GPU
tests (tests/test_gpu_wgrad.py) keep the mirror itself honest: they observe the split decision and the launch list on the device."""
import os
import re

import pytest

import wgrad_cases as wc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'yolo2-pytorch_amd', 'csrc')


def _loader(k):
    return 'LIN' if k == 1 else 'general'


def _M(shape):
    B, cin, cout, H, W, k = shape
    return B * H * W


def test_mirror_constants_are_the_sources():
    common = open(os.path.join(CSRC, 'common.h')).read()
    wgrad = open(os.path.join(CSRC, 'conv_wgrad.hip')).read()
    wino = open(os.path.join(CSRC, 'wino.hip')).read()
    assert int(re.search(r'constexpr int Y2_NUM_CU = (\d+);', common).group(1)) == wc.NUM_CU
    assert int(re.search(r'constexpr int KS = (\d+);', wgrad).group(1)) == wc.KS
    assert re.search(r'!y2_det\.on && Cout <= (\d+)\)', wino).group(1) == str(wc.DZRAW_MAX_COUT)
    assert 'p128 * 100 >= p64 * 115' in wgrad and 'TI * TJ >= 128 * 128 ? 2 : (TI * TJ >= 128 * 64 ? 3 : 4)' in wgrad
    assert wgrad.count('a.rows_total < 4 * 4 * Y2_NUM_CU') == 1 and wgrad.count('a.pairs_total < 4 * 4 * Y2_NUM_CU') == 1
    launched = set(re.findall(r'Y2_WGRAD_LAUNCH\((\d+), \d, (\d+)\);', wgrad))
    assert launched == {(str(ti), str(tj)) for ti, tj in wc.VARIANTS}


def test_mirror_on_the_shapes_of_the_flagship_step():
    """Known answers of the host code for shapes whose launch the project's profiles record (416x416, batch 64)."""
    assert wc.wgrad_tj(288, 64) == 64 and wc.wgrad_tj(64, 128) == 64 and wc.wgrad_tj(1152, 256) == 128 and wc.wgrad_tj(288, 32) == 128
    p = wc.direct_plan(64, 32, 64, 208, 208, 3)                    # the 208x208 layer: 64x64 tiles, 5 column tiles
    assert (p.TI, p.TJ, p.tiles) == (64, 64, 5) and p.splits == wc.cdiv(4 * 256, 5)
    p = wc.wino_plan(64, 512, 1024, 13, 13)                        # deep layer: the 16 groups alone fill the chip
    assert (p.TI, p.TJ, p.splits) == (128, 128, 1)
    assert wc.wino_plan(11, 16, 24, 13, 13).splits > 1             # the one split grouped case of tests/test_gpu_train.py
    g = wc.wino6_grid(64, 13, 13)                                  # csrc/common.h: 784 tiles instead of 1024 (the first gx that reaches them wins)
    assert (g.T, g.th * g.tw, g.tall, g.wide) == (784, 784, 14, 14) and wc.cdiv(64, g.gx) * 14 - 1 <= 4 * g.th and g.gx * 14 - 1 <= 4 * g.tw
    assert wc.wino6_grid(1, 13, 13) == wc.Wino6Grid(4, 4, 0, 0, 1, 16)


@pytest.mark.parametrize('name', sorted(wc.DIRECT_CASES))
def test_direct_case_reaches_what_it_claims(name):
    c = wc.DIRECT_CASES[name]
    B, cin, cout, H, W, k = c.shape
    p = wc.direct_plan(*c.shape)
    assert (p.TI, p.TJ) == c.tile
    assert ('split' if p.splits > 1 else 'unsplit') == c.split
    assert c.grid in wc.grid_shapes(p, k * k * cin, cout)
    assert name[0] == ('l' if k == 1 else 'g')
    assert B * H * W * (cin + cout) * 4 <= 4 << 20                 # operands of a few MB at the most


def test_direct_table_covers_the_matrix():
    seen = {(c.tile, _loader(c.shape[5]), c.split) for c in wc.DIRECT_CASES.values()}
    assert seen == {(v, l, s) for v in wc.VARIANTS for l in ('general', 'LIN') for s in ('split', 'unsplit')}
    for v in wc.VARIANTS:
        grids = {c.grid for c in wc.DIRECT_CASES.values() if c.tile == v}
        assert 'full' in grids and grids & {'ragged-rows', 'ragged-cols'}, v
        # compute_slab_spread needs a second slab, and it must be reached with the atomic epilogue too
        assert any(c.grid == 'full' and c.split == 'split' for c in wc.DIRECT_CASES.values() if c.tile == v), v
    for edge, name in wc.DIRECT_EDGES.items():
        c = wc.DIRECT_CASES[name]
        assert edge in wc.split_edges(wc.direct_plan(*c.shape), _M(c.shape), c.shape[1], c.shape[2], c.shape[5]), (edge, name)
    assert {wc.DIRECT_CASES[n].shape[1] for n in wc.TAP_CASES} == {20, 36, 100}
    for n in wc.TAP_CASES:
        c = wc.DIRECT_CASES[n]
        assert 'tap-in-tile' in wc.split_edges(wc.direct_plan(*c.shape), _M(c.shape), c.shape[1], c.shape[2], c.shape[5]), n
    shape = {k: wc.DIRECT_CASES[n].shape for k, n in wc.GEOMETRY.items()}
    assert all(s[5] == 3 for s in shape.values())
    assert shape['W<32'][4] < 32 and shape['W==32'][4] == 32 and shape['W>32'][4] > 32 and shape['W==1'][4] == 1
    assert shape['H*W<32'][3] * shape['H*W<32'][4] < 32 and shape['H*W<32'][0] * shape['H*W<32'][3] * shape['H*W<32'][4] > 3 * 32
    for tables in (wc.MEANPOS_DIRECT, wc.DET_DIRECT[:5], wc.DET_DIRECT[5:]):
        assert [wc.DIRECT_CASES[n].tile for n in tables] == list(wc.VARIANTS)
        assert all(wc.DIRECT_CASES[n].split == 'split' for n in tables)
    assert all(wc.DIRECT_CASES[n].shape[5] == 3 for n in wc.DET_DIRECT[:5]) and all(wc.DIRECT_CASES[n].shape[5] == 1 for n in wc.DET_DIRECT[5:])
    B, cin, cout, H, W, k = wc.DIRECT_CASES[wc.DET_TOO_SMALL].shape
    assert wc.direct_plan(B, cin, cout, H, W, k).splits * cout * k * k * cin * 4 > wc.DET_MIN_BYTES


def test_strided_cases():
    ks = {(s[5], s[6], s[7]) for s in wc.EX_CASES.values()}
    assert {(5, 1, 2), (3, 2, 0), (7, 2, 3), (1, 2, 0), (3, 2, 1), (3, 1, 1)} <= ks
    B, cin, cout, H, W, k, stride, pad = wc.EX_CASES['ex-3x3s2p0-unread-edge']
    assert (wc.out_size(H, k, stride, pad) - 1) * stride + k - 1 - pad < H - 1 and (wc.out_size(W, k, stride, pad) - 1) * stride + k - 1 - pad < W - 1


@pytest.mark.parametrize('name', sorted(wc.WINO_CASES))
def test_winograd_case_reaches_what_it_claims(name):
    c = wc.WINO_CASES[name]
    B, cin, cout, H, W = c.shape
    p = wc.wino_plan(*c.shape)
    assert (p.TI, p.TJ) == c.tile
    assert ('split' if p.splits > 1 else 'unsplit') == c.split
    assert wc.wino_form(cout) == c.form
    assert wc.wino_form(cout, deterministic=True) == 'three-step'
    assert 16 * wc.wino_tiles(B, H, W) * (cin + cout) * 4 <= 24 << 20          # transformed operands in the workspace


def test_winograd_table_covers_the_matrix():
    dz = {(c.tile, c.split) for c in wc.WINO_CASES.values() if c.form == 'dzraw'}
    assert dz == {(v, s) for v in wc.VARIANTS for s in ('split', 'unsplit')}
    assert {c.split for c in wc.WINO_CASES.values() if c.form == 'three-step'} == {'split', 'unsplit'}
    par = {k: wc.WINO_CASES[n].shape[3:] for k, n in wc.WINO_PARITY.items()}
    assert [tuple(v % 2 for v in par[k]) for k in ('even,even', 'odd,odd', 'odd,even', 'even,odd')] == [(0, 0), (1, 1), (1, 0), (0, 1)]
    assert par['1x1'] == (1, 1) and par['1x3'] == (1, 3)
    assert {wc.WINO_CASES[n].split for n in wc.WINO_V_CASES} == {'split', 'unsplit'}
    assert [wc.WINO_CASES[n].tile for n in wc.DET_WINO] == list(wc.VARIANTS) and all(wc.WINO_CASES[n].split == 'split' for n in wc.DET_WINO)
    assert {wc.WINO_CASES[n].form for n in wc.MEANPOS_WINO} == {'dzraw', 'three-step'} and all(wc.WINO_CASES[n].split == 'split' for n in wc.MEANPOS_WINO)


@pytest.mark.parametrize('name', sorted(wc.WINO6_CASES))
def test_wino6_case_reaches_what_it_claims(name):
    c = wc.WINO6_CASES[name]
    B, cin, cout, H, W = c.shape
    p, g = wc.wino6_plan(*c.shape), wc.wino6_grid(B, H, W)
    assert (p.TI, p.TJ) == c.tile
    assert ('split' if p.splits > 1 else 'unsplit') == c.split
    assert bool(g.tall) == c.mosaic
    assert g.T <= B * wc.cdiv(H, 4) * wc.cdiv(W, 4)


def test_wino6_table_covers_the_matrix():
    assert {(c.split, c.mosaic) for c in wc.WINO6_CASES.values()} == {(s, m) for s in ('split', 'unsplit') for m in (False, True)}
    assert {c.shape[3] % 4 for c in wc.WINO6_CASES.values()} == {0, 1, 2, 3} == {c.shape[4] % 4 for c in wc.WINO6_CASES.values()}
    assert all(wc.WINO6_CASES[n].split == 'split' for n in wc.MEANPOS_WINO6)


def test_first_layer_cases_cover_the_row_walk():
    B, cin, cout, H, W = wc.CONV0_ROW_WALK
    assert B * H >= wc.ROW_WALK and wc.conv0_grid(B * H) == 4 * wc.NUM_CU and wc.conv0_rows_per_wave(B * H) == 2
    B, cin, cout, H, W = wc.CONV0_FUSED_ROW_WALK
    assert B * H // 2 >= wc.ROW_WALK and wc.conv0_rows_per_wave(B * H // 2) == 2 and W % 16 == 0 and H % 2 == 0
    assert wc.conv0_rows_per_wave(wc.ROW_WALK - 1) == 1
    cases = wc.conv0_cases()
    assert len(set(cases)) == len(cases) == 3 * 6 * 4 * 2
    assert {(c[0], c[1], c[2], c[3] - c[1]) for c in cases} == {(ci, co, w, p) for ci in (1, 2, 3) for co in (4, 6, 32, 33, 40, 64) for w in (5, 16, 17, 33) for p in (0, 5)}


def test_layouts_keep_the_operands_aligned():
    assert set(wc.LAYOUTS) == {'dense', 'ldx-window', 'ldz-window', 'both-offset'}
    for dx, dz, ox, oz in wc.LAYOUTS.values():
        assert dx % 4 == dz % 4 == ox % 4 == oz % 4 == 0 and ox <= dx and oz <= dz
    assert wc.LAYOUTS['both-offset'] == (8, 12, 4, 8)
