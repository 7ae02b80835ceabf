"""CPU check of the forward-convolution case tables (tests/fwd_cases.py): the mirror of the host code's dispatch agrees with what every case claims
to reach, the tables as a whole cover the dispatch matrix of csrc/conv_fwd.hip and the forward Winograd drivers of csrc/wino.hip, and the mirror
itself agrees with the built library wherever the library answers without a device: y2_conv_fwd_workspace_bytes runs conv_fwd_impl up to the launch
(classification, choose_tile, plan_split), so its answer pins the mirror to the real host code rather than to itself.  The GPU tests
(tests/test_gpu_fwd.py) observe the rest on the device: the launch list and whether a launch split."""
import ctypes
import os
import random
import re

import pytest

import fwd_cases as fc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'yolo2-pytorch_amd', 'csrc')
ALL_LAYOUTS = dict(fc.LAYOUTS, **fc.NONVEC_LAYOUTS)
DIRECT_TABLES = (fc.DMA_CASES, fc.XCD_CASES, fc.GEN_CASES, fc.WAVE_CASES, fc.PERSIST_CASES)
DIRECT = [(n, c) for t in DIRECT_TABLES for n, c in t.items()]


def query(p, pad=0, off=0, algo=0):
    """y2_conv_fwd_workspace_bytes of the built library for problem p with dummy pointers (the size query touches no memory and no device)."""
    import _hip
    q = _hip.ConvParams()
    base = 1 << 20
    q.x, q.w, q.scale, q.shift = base + 4 * off, base, base, base
    q.y = base if 'y' in p.outs else None
    q.y_pool = base if 'p' in p.outs else None
    q.stats = base if 's' in p.outs else None
    q.B, q.H, q.W, q.Cin, q.ldx, q.Cout, q.ksize = p.B, p.H, p.W, p.cin, p.cin + pad, p.cout, p.k
    q.ldy, q.ldp, q.out_mode, q.slope, q.tile, q.algo = (4 if p.out_mode else 1) * p.cout, p.cout, p.out_mode, 0.1, p.tile, algo
    if p.residual:
        q.residual, q.ldr = base, p.cout
    if p.stride != 1 or p.pad != (p.k - 1) // 2 or p.transposed:
        q.stride, q.pad_plus1 = p.stride, p.pad + 1
    if p.transposed:
        q.transposed, q.out_h, q.out_w = 1, p.out_hw[0], p.out_hw[1]
    return _hip.lib().y2_conv_fwd_workspace_bytes(ctypes.byref(q))


# ------------------------------------------------------------------------------------------------ the mirror against the sources and the library
def test_mirror_constants_are_the_sources():
    common = open(os.path.join(CSRC, 'common.h')).read()
    fwd = open(os.path.join(CSRC, 'conv_fwd.hip')).read()
    wino = open(os.path.join(CSRC, 'wino.hip')).read()
    assert int(re.search(r'constexpr int Y2_NUM_CU = (\d+);', common).group(1)) == fc.NUM_CU
    assert int(re.search(r'constexpr int Y2_NUM_XCD = (\d+);', common).group(1)) == fc.NUM_XCD
    cands = re.search(r'const Cand cands\[\] = \{(.*)\};', fwd).group(1)
    assert [tuple(float(v) for v in c.split(',')) for c in re.findall(r'\{([^{}]*)\}', cands)] == [tuple(float(v) for v in c) for c in fc.CANDIDATES]
    dma = {int(i): (int(bm), int(bn), int(nth or 256)) for i, bm, bn, nth in
           re.findall(r'case (\d+): (?:if \(!GEN(?: && !POOLORD)?\) )?return launch_dma<(\d+), (\d+), \d, \w+, \w+(?:, (\d+|NT))?(?:, true)?>', fwd.replace('NT,', '256,').replace('NT>', '256>'))}
    dma[7] = (64, 64, 64)
    assert dma == fc.DMA_TILES
    reg = {int(i): (int(bm), int(bn), int(bk)) for i, bm, bn, bk in re.findall(r'case (\d+): return launch<(\d+), (\d+), \d, (\d+), POOLORD, VEC>', fwd)}
    assert reg == fc.REG_TILES
    dispatch_tile = re.search(r'\nint dispatch_tile\(.*?\n\}\n', fwd, re.S).group(0)
    assert len(re.findall(r'case \d+:', dispatch_tile)) == len(fc.REG_TILES) and 'default: return Y2_ENOSUP;' in dispatch_tile
    assert not re.findall(r'case 9\d:', dispatch_tile) and not set(fc.ABLATIONS) & set(fc.REG_TILES)       # the ablation ids fall to the default
    assert int(re.search(r'constexpr int F3_TM = (\d+);', wino).group(1)) == fc.F3_TM
    assert int(re.search(r'constexpr int WF2_DEFAULT_VARIANT = (-?\d+);', wino).group(1)) == fc.WF2_DEFAULT_VARIANT
    assert 'constexpr size_t WF_DUMP_BYTES = %d; ' % fc.WF_DUMP_BYTES in wino


def test_mirror_known_answers():
    assert fc.plan_split(282, 9, 64 * 64, None) == (256, 2)                     # B=5, 32 -> 64 channels, 60x60, 3x3 on 64x64 tiles: 256 whole + 26 split in 2
    assert fc.plan_split(282, 9, 64 * 64, 26 * 2 * 64 * 64 * 4 - 4) == (282, 1)
    assert fc.plan_split(512, 9, 64 * 64, None) == (512, 1) and fc.plan_split(100, 7, 64 * 64, None) == (100, 1)
    assert fc.plan_split(1040, 9, 64 * 64, None, 1024) == (1024, 2)
    assert [fc.kslice(9, i, 2) for i in range(2)] == [(0, 4), (4, 9)] and [fc.kslice(18, i, 4) for i in range(4)] == [(0, 4), (4, 9), (9, 13), (13, 18)]
    for nk, ks in ((9, 2), (18, 4), (27, 6), (8, 2), (12, 3), (72, 16)):        # the K-slices tile [0, nk) and every slice has a slab
        b = [fc.kslice(nk, i, ks) for i in range(ks)]
        assert b[0][0] == 0 and b[-1][1] == nk and all(b[i][1] == b[i + 1][0] for i in range(ks - 1)) and all(e > s for s, e in b)
    # narrow outputs from about 8256 pixels on: 128x32, the one candidate dispatch_tile has no case for - tile = 0 is refused there when the operands
    # rule out the LDS-DMA kernel (the mirror says so too; a known defect of the library, see the README)
    assert fc.choose_tile(2 * 65 * 64, 20, 9) == 6 and fc.choose_tile(5 * 58 * 58, 20, 1) == 6 and fc.choose_tile(8192, 20, 9) != 6
    assert fc.route(fc.P(2, 6, 20, 65, 64, 3)).rc == fc.ENOSUP and fc.route(fc.P(5, 8, 20, 58, 58, 1), 4, 1).rc == fc.ENOSUP
    assert fc.route(fc.P(2, 6, 20, 64, 64, 3)).tile in fc.REG_TILES
    assert fc.out_size(4, 5, 2, 0) == 1                                          # C division truncates towards zero


def test_mirror_agrees_with_the_library_on_every_case():
    for name, c in DIRECT:
        for lay, (pad, off) in fc.LAYOUTS.items():
            assert query(c.p, pad, off) == fc.workspace_bytes(c.p, pad, off), (name, lay)
    for name, (shape, outs) in fc.REG_SHAPES.items():
        for tid in fc.REG_IDS:
            for lay, (pad, off) in ALL_LAYOUTS.items():
                for t in (tid, tid + 100, 0):
                    p = fc.P(*shape, tile=t, outs=outs)
                    assert query(p, pad, off) == fc.workspace_bytes(p, pad, off), (name, t, lay)
    for name, p in fc.FAMILY_CASES.items():
        for outs in fc.OUTS:
            for kw in (dict(), dict(out_mode=1), dict(residual=True)):
                q = p._replace(outs=outs, **kw)
                assert query(q) == fc.workspace_bytes(q), (name, outs, kw)
    for name, r in fc.REFUSALS.items():
        pad, off = ALL_LAYOUTS[r.layout]
        want = fc.workspace_bytes(r.p, pad, off) if r.algo == 0 else fc.wino_route(r.p, r.algo, pad, off).ws_bytes
        assert query(r.p, pad, off, r.algo) == want, name


def test_tile_choice_is_the_library_s_where_the_workspace_tells_tiles_apart():
    """tile = 0: the size query answers (tiles - full_tiles) * ksplit * BM * BN * 4 of the tile choose_tile took.  Wherever that number differs between
    the five candidates, the library's answer identifies its choice."""
    told, took = set(), set()
    for name, c in DIRECT:
        if c.p.tile != 0:
            continue
        r = fc.route(c.p)
        by_tile = {t: fc.workspace_bytes(c.p._replace(tile=t)) for t in fc.GEN_TILES}
        assert query(c.p) == by_tile[r.tile], name
        if sum(v == by_tile[r.tile] for v in by_tile.values()) == 1:
            told.add(r.tile)
    rnd = random.Random(7)
    for _ in range(3000):
        p = fc.P(rnd.randint(1, 64), rnd.choice((32, 64, 96, 160, 256, 512)), rnd.choice((20, 32, 64, 72, 125, 128, 200, 256, 512, 1024)), rnd.randint(1, 104), rnd.randint(1, 104), rnd.choice((1, 3)))
        r = fc.route(p)
        by_tile = {t: fc.workspace_bytes(p._replace(tile=t)) for t in fc.GEN_TILES}
        assert query(p) == by_tile[r.tile], p
        took.add(r.tile)
        if sum(v == by_tile[r.tile] for v in by_tile.values()) == 1:
            told.add(r.tile)
    assert told == took and {3, 5, 6} <= told                                    # every candidate the sample's problems take was identified at least once


def test_mirror_agrees_with_the_library_on_random_problems():
    rnd = random.Random(1)
    for _ in range(6000):
        k, stride = rnd.choice((1, 3, 3, 5, 7)), rnd.choice((1, 1, 1, 2))
        p = fc.P(rnd.randint(1, 40), rnd.choice((4, 6, 8, 12, 13, 16, 20, 32, 40, 48, 64, 96, 128, 256, 512)), rnd.choice((8, 20, 24, 32, 33, 64, 72, 125, 128, 200, 256, 512)),
                 rnd.randint(1, 70), rnd.randint(1, 70), k, tile=rnd.choice((0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 15, 21, 23, 101, 103, 111, 113, 121, 123, 106, 10)),
                 stride=stride, pad=rnd.choice((None, None, 0, 1)), outs=rnd.choice(fc.OUTS), out_mode=rnd.choice((0, 0, 0, 1)), residual=rnd.choice((False, False, False, True)))
        pad, off = rnd.choice(list(ALL_LAYOUTS.values()))
        assert query(p, pad, off) == fc.workspace_bytes(p, pad, off), (p, pad, off)
    for _ in range(3000):
        algo = rnd.choice((1, 2, 3, 6, 7))
        p = fc.P(rnd.randint(1, 40), rnd.choice((4, 8, 16, 20, 32, 64, 96, 128, 256, 512)), rnd.choice((4, 20, 32, 64, 72, 128, 256, 260, 512)), rnd.randint(1, 60), rnd.randint(1, 60), 3,
                 tile=rnd.choice((0, 0, 1, 2, 3, 5, 6)), outs=rnd.choice(fc.OUTS))
        pad, off = (0, 0) if algo == 7 else rnd.choice(list(fc.LAYOUTS.values()))
        assert query(p, pad, off, algo) == fc.wino_route(p, algo, pad, off).ws_bytes, (algo, p, pad, off)


# ------------------------------------------------------------------------------------------------ claims
@pytest.mark.parametrize('name', [n for n, _ in DIRECT])
def test_direct_case_reaches_what_it_claims(name):
    c = dict(DIRECT)[name]
    for lay, (pad, off) in fc.LAYOUTS.items():
        got = fc.claims_of(c.p, pad, off)
        assert c.claims <= got, (lay, sorted(c.claims - got), sorted(got))
    r = fc.route(c.p)
    assert r.rc == fc.OK and r.vec and c.p.tile not in fc.ABLATIONS
    Ho, Wo = fc.out_hw(c.p)
    assert c.p.B * (c.p.H * c.p.W * c.p.cin + Ho * Wo * c.p.cout) * 4 <= 32 << 20        # operands and result of a few MB
    assert 2 * r.M * c.p.cout * c.p.k * c.p.k * c.p.cin < 3e9                             # ... and a reference of a second at the most


def test_dma_table_covers_every_cell_of_every_tile():
    for t in fc.DMA_TILE_IDS:
        cells, unsplit_nk8 = set(), False
        for n, c in fc.DMA_CASES.items():
            r = fc.route(c.p)
            if r.tile != t:
                continue
            assert r.family == 'conv_fwd_dma_kernel' and not r.gen and (r.bm, r.bn) == fc.DMA_TILES[t][:2]
            cells |= fc.claims_of(c.p) & c.claims
            unsplit_nk8 |= r.nk >= 8 and fc.splits(r, 0) == (r.tiles, 1) and fc.splits(r, None)[1] > 1      # the same case without workspace: whole-tile K loops of 8+ slabs
        assert set(fc.DMA_CELLS) <= cells and unsplit_nk8, (t, sorted(set(fc.DMA_CELLS) - cells))
    c = fc.DMA_CASES['dma3-mixed']
    r = fc.route(c.p)
    assert (r.tiles,) + fc.splits(r, None) == (282, 256, 2)                      # 256 whole tiles and 26 split in two
    # a mixed launch of the 512-thread tiles and of the 128x32 tile too
    assert all('split-mixed' in fc.DMA_CASES['dma%d-mixed' % t].claims for t in fc.DMA_TILE_IDS)


def test_xcd_remap_sees_every_residue_in_both_grids():
    whole, split, even = set(), set(), set()
    for tab in DIRECT_TABLES:
        for n, c in tab.items():
            r = fc.route(c.p)
            if r.family in ('conv_fwd_dma_kernel', 'conv_fwd_wave_kernel'):
                full, ks = fc.splits(r, None)
                whole.add(r.tiles % 8)                                           # the launch without workspace
                if ks > 1:
                    split.add((r.tiles - full) * ks % 8)
                    even.add(r.nk % ks == 0)
    assert whole == split == set(range(8)) and even == {True, False}


def test_gen_wave_and_persistent_tables_cover_their_forms():
    for form in fc.GEN_FORMS:
        got = {s for c in fc.GEN_CASES.values() if form in c.claims for s in ('split-all', 'unsplit') if s in c.claims}
        assert got == {'split-all', 'unsplit'}, form
    assert {fc.route(c.p).tile for c in fc.GEN_CASES.values()} == set(fc.GEN_TILES)
    wave = [c for c in fc.WAVE_CASES.values() if 'wave' in c.claims]
    assert all(fc.route(c.p).procs == 4 * fc.NUM_CU for c in wave)
    assert any({'cin%32==16', 'split-all'} <= c.claims for c in wave) and any('split-mixed' in c.claims for c in wave) and any('poolord' in c.claims for c in wave)
    r = fc.route(fc.WAVE_CASES['wave-mixed'].p)
    assert r.tiles > 1024 and fc.splits(r, None)[0] == 1024
    assert {frozenset(c.claims & {'dma', 'gen'}) for c in fc.WAVE_CASES.values() if 'wave-fallback' in c.claims} == {frozenset(['dma']), frozenset(['gen'])}
    for t in fc.PERSIST_OF:
        cells = set()
        for c in fc.PERSIST_CASES.values():
            if c.p.tile == t:
                cells |= c.claims
                plain = fc.route(c.p._replace(tile=fc.PERSIST_OF[t]))
                assert (plain.bm, plain.bn, plain.nk, plain.family) == fc.route(c.p)[3:5] + (fc.route(c.p).nk, 'conv_fwd_dma_kernel')
                # the oddity the module docstring describes: the size query of a persistent id answers for the plain tile
                assert fc.workspace_bytes(c.p) == fc.workspace_bytes(c.p._replace(tile=fc.PERSIST_OF[t]))
        assert set(fc.PERSIST_CELLS) <= cells, (t, sorted(set(fc.PERSIST_CELLS) - cells))
        assert {'more-than-slots', 'odd-slabs'} <= fc.PERSIST_CASES['p%d-walk-3slabs' % t].claims       # the LDS buffer parity carries over from tile to tile


def test_register_staged_table_reaches_every_id_with_and_without_vec():
    seen = set()
    for name, (shape, outs) in fc.REG_SHAPES.items():
        for tid in fc.REG_IDS:
            for lay, (pad, off) in ALL_LAYOUTS.items():
                pre = fc.route(fc.P(*shape, outs=outs), pad, off)
                p = fc.P(*shape, tile=fc.reg_tile_id(tid, pre.vec), outs=outs)
                r = fc.route(p, pad, off)
                assert r.rc == fc.OK and r.family == 'conv_fwd_kernel' and r.tile == tid and (r.bm, r.bn) == fc.REG_TILES[tid][:2], (name, tid, lay)
                seen.add((tid, r.vec, r.poolord))
                if not r.vec:                                                    # every non-vec problem also runs with tile = 0
                    r0 = fc.route(p._replace(tile=0), pad, off)
                    assert r0.rc == fc.OK and r0.family == 'conv_fwd_kernel' and r0.tile in fc.REG_TILES
    assert seen == {(t, v, q) for t in fc.REG_IDS for v in (False, True) for q in (False, True)}
    assert {101, 103, 111, 113, 121, 123} <= {fc.reg_tile_id(t, True) for t in fc.REG_IDS}
    # blocks: more than one in each direction, ragged in both, for the largest tile too
    assert any(s[0] * s[3] * s[4] > 256 and s[0] * s[3] * s[4] % 64 for s, _ in fc.REG_SHAPES.values()) and any(s[2] > 128 for s, _ in fc.REG_SHAPES.values())
    assert {s[1] % 4 for s, _ in fc.REG_SHAPES.values()} >= {0, 1, 2}


def test_family_cases_and_refusals():
    fam = {n: fc.route(p) for n, p in fc.FAMILY_CASES.items()}
    assert [r.family for r in fam.values()] == ['conv_fwd_dma_kernel', 'conv_fwd_dma_kernel', 'conv_fwd_wave_kernel', 'conv_fwd_dma_kernel[persistent]', 'conv_fwd_dma_kernel',
                                                'conv_fwd_kernel']
    assert fam['gen'].gen and fam['dma-512'].tile == 8 and fam['dma'].ctail and fam['reg'].vec
    assert all(fc.splits(r, None)[1] > 1 for n, r in fam.items() if n not in ('persistent', 'reg'))       # split launches under every epilogue form
    assert all(p.H % 2 == 0 and p.W % 2 == 0 for p in fc.FAMILY_CASES.values())
    for name, r in fc.REFUSALS.items():
        assert fc.refusal_code(r) == r.rc != fc.OK, name
        assert r.p.tile not in fc.ABLATIONS
    assert {r.algo for r in fc.REFUSALS.values()} == {0, 1, 2, 3, 6}
    names = ' '.join(fc.REFUSALS)
    for cell in ('persistent+pool', 'persistent+cin%32', 'strided+nonvec', 'residual+pool', 'grouped-16', 'grouped-36+pool', 'grouped-36+stats', 'tile-without-kernel', 'fused+cin%32',
                 'implicit+cin<32'):
        assert cell in names, cell


def test_nothing_uses_the_ablation_ids():
    ps = [c.p for _, c in DIRECT] + list(fc.FAMILY_CASES.values()) + [r.p for r in fc.REFUSALS.values()]
    assert not {p.tile for p in ps} & ({*fc.ABLATIONS} | {100 + a for a in fc.ABLATIONS})
    assert not set(fc.REG_IDS) & set(fc.ABLATIONS)
    for t in fc.ABLATIONS:                                                       # ... and the library refuses them where they used to launch
        for tid in (t, t + 100):
            for outs in ('y', 'p'):
                assert fc.route(fc.P(*fc.REFUSED_TILE_SHAPE, tile=tid, outs=outs)).rc == fc.ENOSUP
    r = fc.route(fc.P(*fc.REFUSED_TILE_SHAPE, tile=101))
    assert r.rc == fc.OK and r.family == 'conv_fwd_kernel' and r.vec and not r.poolord      # the shape does reach dispatch_tile<false, true>


# ------------------------------------------------------------------------------------------------ Winograd
def test_winograd_table_covers_family_x_variant_x_mask():
    seen = set()
    for v in fc.WINO_VARIANTS:
        for where in fc.WINO_MAPS:
            for m in fc.wino_masks(where):
                p, algo, env = fc.wino_case(v, where, m)
                r = fc.wino_route(p, algo, variant=env)
                assert r.rc == fc.OK and (r.family, r.variant) == fc.WINO_FAMILY[v] and r.out_mask == m, (v, where, m)
                assert r.out_inst == (None if v in ('three-kernel', 'gen1') else m if m in (1, 2, 3, 5) else 7)
                assert r.nchunks == 1 and all(g % fc.NUM_XCD == 0 for g in r.grids)
                seen.add((r.family, r.variant, m))
    want = {(f, v, m) for f, vs in (('wino', (None,)), ('wino_fused_kernel', (-1,)), ('wino_fused2_kernel', (3, 5, 11, 13)), ('wino_fused3_kernel', (0, 4, 8, 12, 20)))
            for v in vs for m in range(1, 8)}
    assert seen == want
    B, H, W = fc.WINO_MAPS['ragged']
    assert H % 2 == 1 and W % 2 == 1 and all(v % 2 == 0 for v in fc.WINO_MAPS['even'][1:])


def test_winograd_walks_chunks_and_grouped_gemms():
    for v, (B, cin, cout, H, W) in fc.WINO_WALKS.items():
        algo, tile, env, _, _ = fc.WINO_VARIANTS[v]
        r = fc.wino_route(fc.P(B, cin, cout, H, W, 3, tile=tile), algo, variant=env)
        slots = 2 * fc.NUM_CU if r.family == 'wino_fused3_kernel' else fc.NUM_CU
        units = fc.cdiv(r.T, fc.F3_TM if r.family == 'wino_fused3_kernel' else 64) * fc.cdiv(cout, 64)
        assert (r.family, r.variant) == fc.WINO_FAMILY[v] and r.grids == (slots,) and slots < units < 2 * slots and cout % 64       # some workgroups take a second unit
    assert {fc.WINO_FAMILY[v][0] for v in fc.WINO_WALKS} == {'wino_fused_kernel', 'wino_fused2_kernel', 'wino_fused3_kernel'}
    assert [fc.output_block(c) for c in fc.WINO_OUTPUT_COUTS] == [(16, 16), (16, 16), (32, 8), (64, 4), (64, 4), (64, 4)]
    assert [fc.cdiv(c // 4, fc.output_block(c)[0]) for c in fc.WINO_OUTPUT_COUTS] == [1, 1, 1, 1, 1, 2]
    got = {}
    for name, (algo, B, cin, cout, H, W) in fc.GROUPED_CASES.items():
        r = fc.wino_route(fc.P(B, cin, cout, H, W, 3), algo)
        assert r.rc == fc.OK and r.inner.family == 'conv_fwd_dma_kernel[grouped]' and r.inner.tiles % (16 if algo == 1 else 36) == 0
        got[name] = fc.splits(r.inner, None)[1] > 1
    assert got == {n: 'split' in n and 'unsplit' not in n for n in fc.GROUPED_CASES}
    assert fc.wino6_grid(*[fc.GROUPED_CASES['g36-mosaic'][i] for i in (1, 4, 5)]).tall
    for name, (algo, tile, B, cin, cout, H, W) in fc.CHUNK_CASES.items():
        r = fc.wino_route(fc.P(B, cin, cout, H, W, 3, tile=tile), algo, chunk_mb=fc.CHUNK_MB)
        assert r.nchunks >= 2 and B % r.cb and r.cb > 1, name                    # two or more chunks, the last one shorter
    assert {fc.wino_route(fc.P(c[2], c[3], c[4], c[5], c[6], 3, tile=c[1]), c[0]).family for c in fc.CHUNK_CASES.values()} == {'wino', 'wino_fused2_kernel', 'wino_fused3_kernel'}


def test_layouts_keep_or_break_the_alignment_as_named():
    assert list(fc.LAYOUTS) == ['dense', 'padded', 'offset', 'both']
    assert all(pad % 4 == 0 and off % 4 == 0 and off <= pad for pad, off in fc.LAYOUTS.values())
    assert [(pad > 0, off > 0) for pad, off in fc.LAYOUTS.values()] == [(False, False), (True, False), (True, True), (True, True)]
    assert fc.LAYOUTS['both'][0] > fc.LAYOUTS['both'][1] and fc.LAYOUTS['offset'][0] == fc.LAYOUTS['offset'][1]
    assert all((pad % 4 or off % 4) and off <= pad for pad, off in fc.NONVEC_LAYOUTS.values())
    assert any(pad % 4 == 0 and off % 4 for pad, off in fc.NONVEC_LAYOUTS.values())      # a misaligned x whose stride is fine
