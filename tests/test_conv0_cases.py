"""CPU check of the first-layer forward case tables (tests/conv0_cases.py): the mirror of y2_conv0_fwd / launch0 agrees with what every case claims to
reach, and the tables as a whole reach every straight-line variant, the general kernel with every Cin x NBLK, every walk length of the persistent
grid for both kernel forms, ragged-right / ragged-bottom / ragged-both tiles and every refusal.
The same for y2_conv0_fwd_sel (SEL_CASES, SEL_REFUSALS; tests/test_gpu_conv0_sel.py runs them): the ninth straight-line variant, which is launched
outside the Y2_C0 list, the general kernel with `sel` through every way a call with gamma misses that variant, and the entry's refusals.

Unlike fwd_cases, this mirror cannot be pinned to the built library: all variants launch as `conv0_kernel` and the entry point answers no size query,
so nothing exported tells which variant ran.  What can be pinned is pinned to the source text below (the constants and the list of straight-line
launches); the README's mutation table shows that the GPU tests (tests/test_gpu_conv0.py) see the code the tables claim to reach."""
import os
import re

import pytest

import conv0_cases as cc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'yolo2-pytorch_amd', 'csrc')
ALL = [(n, c) for t in cc.PARITY_TABLES + (cc.SEL_CASES,) for n, c in t.items()]


def reached(cell, tables=cc.PARITY_TABLES, also=()):
    """Names of the cases whose claim AND whose mirror answer both contain every word of `cell` ('general' / 'straight' are implied by a claimed variant:
    they are looked up in the mirror's answer alone)."""
    cell = set(cell.split()) | set(also)
    return [n for t in tables for n, c in t.items() if cell - {'general', 'straight'} <= c.claims and cell <= cc.claims_of(c.c)]


# ------------------------------------------------------------------------------------------------ the mirror against the sources
def test_mirror_constants_are_the_sources():
    """Literal matches against the text of conv0_fwd.hip, the declared substitute for a pin to the library.  They fail on any edit of the matched lines - the
    FULL condition, the grid expression, `mono` / `raw`, the Y2_C0 launch list, the refusing `if (...) return` lines - including one that changes only a name or
    the spacing.  When this test fails, re-read route() in conv0_cases.py against launch0 and y2_conv0_fwd before updating the strings here."""
    common = open(os.path.join(CSRC, 'common.h')).read()
    src = open(os.path.join(CSRC, 'conv0_fwd.hip')).read()
    header = open(os.path.join(os.path.dirname(CSRC), '..', 'include', 'yolo2_hip.h')).read()
    assert int(re.search(r'constexpr int Y2_NUM_CU = (\d+);', common).group(1)) == cc.NUM_CU
    assert re.search(r'constexpr int TH = (\d+), TW = (\d+);', src).groups() == (str(cc.TH), str(cc.TW))
    assert int(re.search(r'atoi\(getenv\("Y2_CONV0_WGS"\)\) : (\d+);', src).group(1)) == cc.WGS_PER_CU
    assert 'tiles > (long long)Y2_NUM_CU * per_cu ? (long long)Y2_NUM_CU * per_cu : tiles' in src
    # the straight-line launches, Cout 32 first: exactly the mirror's list, in launch0's order
    got = [(int(nb), int(out), raw == 'true') for nb, out, raw in re.findall(r'Y2_C0\((\d), (\d), (true|false)\);', src)]
    assert got == list(cc.VARIANTS)
    assert 'if (CIN == 3 && (a.H % TH) == 0 && (a.W % TW) == 0 && (a.Cout == 32 || a.Cout == 64) && (a.y == nullptr || a.ldy == a.Cout) && (a.y_pool == nullptr || a.ldp == a.Cout))' in src
    # the ninth straight-line launch stands outside the Y2_C0 list: its condition, its instantiation (named once), and the rule that no other call with pool_sign
    # takes a straight-line variant
    assert 'if (a.pool_sign != nullptr && a.Cout == 32 && out == 7 && raw) {' in src and cc.SEL_VARIANT == (1, 7, True)
    assert re.findall(r'\(conv0_kernel<3, (\d), (\d), true, (true|false)>\), dim3', src) == [('1', '7', 'true')]
    assert src.index('if (a.pool_sign != nullptr && a.Cout == 32') < src.index('if (a.pool_sign != nullptr) done = false;') < src.index('else if (a.Cout == 32) {') < src.index('if (done) {')
    assert 'const bool sel = (OUT == 7 && RAW) ? true : (OUT < 0 ? a.pool_sign != nullptr : false);' in src          # which kernels select: <.., 7, .., RAW> and the general one
    assert ('return (gamma != nullptr && z != nullptr && z_sel != nullptr) ? conv0_fwd_impl(x_nchw, w, nullptr, nullptr, z, z_sel, stats, B, H, W, Cin, Cout, ldz, ldzs, 1.f, stream, gamma)'
            in src and list(cc.SEL_REFUSAL_RETURNS)[0] == 'gamma != nullptr && z != nullptr && z_sel != nullptr' and list(cc.SEL_REFUSAL_RETURNS)[1:] == list(cc.REFUSAL_RETURNS))
    assert 'stats may be NULL' in header
    assert 'const bool mono = a.slope >= 0.f && a.slope <= 1.f;' in src and 'a.scale == nullptr && a.shift == nullptr && a.slope == 1.f;' in src
    for name, val in (('Y2_OK', cc.OK), ('Y2_EINVAL', cc.EINVAL), ('Y2_EALIGN', cc.EALIGN), ('Y2_ENOSUP', cc.ENOSUP)):
        assert re.search(r'%s\s*=?\s*\(?(-?\d+)' % name, header) and int(re.search(r'%s\s*=?\s*\(?(-?\d+)' % name, header).group(1)) == val, name
    # every `return` that refuses, in order: the five of the entry point and launch0's own
    entry = src[src.index('extern "C" int y2_conv0_fwd'):]
    returns = re.findall(r'if \((.*)\) return (Y2_E\w+);', entry)
    assert [r[1] for r in returns] == ['Y2_EINVAL', 'Y2_ENOSUP', 'Y2_EINVAL', 'Y2_EINVAL', 'Y2_ENOSUP']
    keys = list(cc.REFUSAL_RETURNS)
    assert all(cond.startswith(k) for (cond, _), k in zip(returns, keys[:5]))
    assert 'if (tiles <= 0 || tiles > 0x7fffffffLL) return Y2_EINVAL;' in src and keys[5] == 'tiles <= 0'


def test_mirror_known_answers():
    r = cc.route(cc.C(32, 3, 32, 416, 416, 'p'))                   # detect at batch 32: 26 x 13 tiles per image, 5.3 tiles per workgroup
    assert (r.tiles_y, r.tiles_x, r.ntiles, r.grid, r.walk_max, r.walk_min) == (26, 13, 10816, 2048, 6, 5) and cc.variant_name(r) == 'sl1-o2'
    r = cc.route(cc.C(64, 3, 32, 416, 416, 'ys', scale=False, shift=False, slope=1.0))
    assert r.ntiles == 21632 and r.walk_max == 11
    # the three shapes of test_conv0_persistent_workgroups_walk_several_tiles (tests/test_gpu_kernels.py): two walks of two tiles, and one that does not walk
    assert [cc.route(cc.C(B, 3, co, H, W, 'p')).ntiles for B, H, W, co in ((9, 416, 416, 32), (40, 208, 224, 32), (3, 330, 500, 16))] == [3042, 3640, 1008]
    assert [cc.route(cc.C(B, 3, co, H, W, 'p')).walk_max for B, H, W, co in ((9, 416, 416, 32), (40, 208, 224, 32), (3, 330, 500, 16))] == [2, 2, 1]
    assert cc.route(cc.C(1, 3, 20, 1, 1)).ntiles == 1 and cc.route(cc.C(3, 3, 20, 17, 33)).ntiles == 12
    assert cc.variant_name(cc.route(cc.C(2, 3, 32, 32, 64, 'p', slope=1.0))) == 'sl1-o2' and cc.variant_name(cc.route(cc.C(2, 3, 32, 32, 64, 'p', slope=0.0))) == 'sl1-o2'
    assert cc.variant_name(cc.route(cc.C(2, 3, 32, 32, 64, 'p', slope=1.0001))) == 'gen1'
    assert cc.variant_name(cc.route(cc.C(2, 3, 32, 32, 64, 'ys', scale=False, shift=False, slope=0.1))) == 'sl1-o5'          # no affine but an activation: not RAW
    assert cc.variant_name(cc.route(cc.C(2, 3, 32, 32, 64, 'ys', scale=True, shift=False, slope=1.0))) == 'sl1-o5'
    assert cc.variant_name(cc.route(cc.C(2, 3, 64, 32, 64, 'ys', scale=True, shift=False, slope=1.0))) == 'gen2'
    assert cc.variant_name(cc.route(cc.C(2, 3, 32, 32, 64, 'p', ypad=4))) == 'sl1-o2'                                        # ldy of an absent y does not count
    assert cc.variant_name(cc.route(cc.C(2, 3, 32, 32, 64, 'y', ppad=4))) == 'sl1-o1'
    assert cc.variant_name(cc.route(cc.C(2, 3, 32, 32, 65, 'y'))) == 'gen1' and cc.variant_name(cc.route(cc.C(2, 2, 32, 32, 64, 'y'))) == 'gen1'
    # y2_conv0_fwd_sel: the training forward at batch 64 takes the ninth variant; without statistics, at Cout 64 or into wider rows it is the general kernel
    r = cc.route(cc.S(64, 3, 32, 416, 416))
    assert cc.variant_name(r) == 'sl1-o7-raw-sel' and (r.ntiles, r.walk_max, r.full, r.raw, r.sel) == (21632, 11, True, True, True)
    assert cc.variant_name(cc.route(cc.S(64, 3, 32, 416, 416, 'yp'))) == 'gen1-sel' and cc.variant_name(cc.route(cc.S(64, 3, 64, 416, 416))) == 'gen2-sel'
    assert cc.variant_name(cc.route(cc.S(64, 3, 32, 416, 416, ppad=32))) == 'gen1-sel' and cc.variant_name(cc.route(cc.S(64, 3, 32, 418, 416))) == 'gen1-sel'
    # the same call through the plain entry (no gamma) keeps its straight-line form
    assert cc.variant_name(cc.route(cc.S(2, 3, 32, 32, 64, 'yp')._replace(sel=False))) == 'sl1-o3'


# ------------------------------------------------------------------------------------------------ claims
@pytest.mark.parametrize('name', [n for n, _ in ALL])
def test_case_reaches_what_it_claims(name):
    c = dict(ALL)[name]
    got = cc.claims_of(c.c)
    assert c.claims <= got, (sorted(c.claims - got), sorted(got))
    r = cc.route(c.c)
    assert r.rc == cc.OK
    # operands and results small enough for a test of a few seconds: at most 1 GB of fp32 output on the device, and no case that walks 7+ tiles writes a full-resolution map
    # at the straight-line widths
    full = c.c.B * c.c.H * c.c.W * c.c.cout * 4
    assert (full if 'y' in c.c.outs else full // 4) <= 1 << 30
    assert not ('walk7+' in got and 'y' in c.c.outs and c.c.cout >= 32)
    assert 0 <= c.c.yoff <= max(c.c.ypad, 0) and 0 <= c.c.poff <= max(c.c.ppad, 0)


def test_tables_reach_every_variant_at_a_small_and_at_a_walking_size():
    for v in cc.VARIANTS:
        name = cc.variant_name(cc.Route(cc.OK, 'straight', v[0], v[1], v[2], True, 0, 0, 0, 0, 0, 0))
        assert reached(name + ' walk1', (cc.STRAIGHT_CASES,)), name
        assert reached(name + ' walk4 steady-state buffer-reuse uneven-walk', (cc.STRAIGHT_CASES,)), name
    assert {cc.variant_name(cc.route(c.c)) for c in cc.STRAIGHT_CASES.values()} == {'sl%d-o%d%s' % (a, b, '-raw' if r else '') for a, b, r in cc.VARIANTS}
    assert len(cc.STRAIGHT) == len(cc.VARIANTS) == 8
    # the forms the shipped plans launch: at every walk length
    for v in ('sl1-o2', 'sl1-o5-raw'):
        for w in ('walk1', 'walk2', 'walk3', 'walk4'):
            assert reached('%s %s' % (v, w), (cc.STRAIGHT_CASES,)), (v, w)
    assert reached('sl1-o2 walk7+ buffers-rewritten-twice', (cc.STRAIGHT_CASES,))
    # both general kernels
    for g in ('gen1', 'gen2'):
        assert reached(g), g


def test_tables_reach_every_cin_with_both_nblk():
    for cin in (1, 2, 3, 4):
        for nb in (1, 2):
            assert reached('cin%d gen%d' % (cin, nb), (cc.TAP_CASES,)), (cin, nb)
        assert reached('cin%d walk4 buffer-reuse' % cin, (cc.GEN_WALK_CASES,)), cin          # every tap table in the steady state of the walk
    assert {c.c.cout for c in cc.MASK_CASES.values()} == set(cc.MASK_COUTS) == {1, 31, 32, 33, 63, 64}
    for cout in cc.MASK_COUTS:
        assert reached('ragged-both', ({n: c for n, c in cc.MASK_CASES.items() if c.c.cout == cout and 'ld>cout' in c.claims},))
        assert reached('ragged-both', ({n: c for n, c in cc.MASK_CASES.items() if c.c.cout == cout and 'ld>cout' not in c.claims},))
    w = cc.claims_of(cc.MASK_CASES['mask-cout32-window'].c)
    assert {'ld%4', 'channel-offset', 'ld>cout'} <= w


def test_tables_reach_every_walk_length_with_both_kernel_forms():
    for w in cc.WALKS:
        assert reached('straight ' + w, also=() if w == 'walk1' else ('uneven-walk',)), w
        assert reached('general ' + w, also=() if w == 'walk1' else ('uneven-walk',)), w
    for form in ('straight', 'general'):
        assert reached(form + ' steady-state') and reached(form + ' buffer-reuse') and reached(form + ' buffers-rewritten-twice'), form
    assert reached('gen2 walk4') and reached('general walk4 multi-tile-image ragged-right ragged-bottom')
    # the thresholds themselves: 4,097 tiles is the first with a tile from the in-loop staging, 6,145 the first that reuses a buffer, 14,337 rewrites each twice
    for tiles, word, has in ((4096, 'steady-state', False), (4097, 'steady-state', True), (6144, 'buffer-reuse', False), (6145, 'buffer-reuse', True),
                             (14336, 'buffers-rewritten-twice', False), (14337, 'buffers-rewritten-twice', True)):
        assert (word in cc.claims_of(cc.C(tiles, 3, 16, 10, 20))) == has, tiles
    r = cc.route(cc.STRAIGHT_CASES['sl1-o2-walk4'].c)
    assert (r.ntiles, r.grid, r.walk_max, r.walk_min) == (6400, 2048, 4, 3)


def test_tables_reach_every_kind_of_ragged_tile_and_the_geometry_list():
    for word in ('ragged-right', 'ragged-bottom', 'ragged-both', 'whole-tile'):
        assert reached(word, (cc.GEOMETRY_CASES,)), word
    sizes = {(c.c.H, c.c.W) for c in cc.GEOMETRY_CASES.values()}
    assert sizes == {(1, 1), (1, 40), (17, 1), (2, 2), (16, 32), (16, 33), (17, 32), (20, 36), (15, 31)}
    for H, W in sizes:
        assert {c.c.B for c in cc.GEOMETRY_CASES.values() if (c.c.H, c.c.W) == (H, W)} == {1, 3}
    assert 'p' in cc.GEOMETRY['2x2'][2] and cc.GEOMETRY['15x31'][2] == 'y'
    assert all(('p' in c.c.outs) == (c.c.H % 2 == 0 and c.c.W % 2 == 0) for c in cc.GEOMETRY_CASES.values())
    assert reached('batch one-tile-image', (cc.GEOMETRY_CASES,)) and reached('batch multi-tile-image', (cc.GEOMETRY_CASES,))


def test_output_sets_and_fallthroughs():
    for g in cc.OUTSET_SHAPES:
        seen = {(c.c.outs, c.c.scale, c.c.shift, c.c.slope) for n, c in cc.OUTSET_CASES.items() if n.startswith(g)}
        assert seen == {(o, a, b, s) for o in cc.OUTS for a, b, s in cc.AFFINE}
        assert all(cc.variant_name(cc.route(c.c)) == g for n, c in cc.OUTSET_CASES.items() if n.startswith(g))
    assert sorted(cc.OUTS) == sorted(cc.MASKS.values())
    assert {(a, b) for a, b, _ in cc.AFFINE} == {(True, True), (False, False), (True, False), (False, True)}
    for cell in ('gen2 out3', 'gen2 out5', 'gen1 out6', 'gen1 out7', 'gen1 out4', 'gen1 out1 ld>cout', 'gen1 out2 ld>cout', 'gen1 out2', 'gen2 out2'):
        assert reached(cell, (cc.FALL_CASES,), also=('fallthrough',)), cell
    slopes = {(c.c.cout, c.c.slope) for c in cc.FALL_CASES.values() if c.c.outs == 'p' and c.c.ppad == 0 and c.c.cin == 3}
    assert slopes == {(32, -0.5), (32, 1.5), (64, -0.5), (64, 1.5)}
    # each fall-through differs from a straight-line call in one respect only
    assert cc.route(cc.FALL_CASES['fall-cout32-ldy'].c._replace(ypad=0)).kernel == 'straight'
    assert cc.route(cc.FALL_CASES['fall-cout32-slope1.5'].c._replace(slope=1.0)).kernel == 'straight'
    assert cc.route(cc.FALL_CASES['fall-cout64-o5-affine'].c._replace(scale=False, shift=False, slope=1.0)).kernel == 'straight'
    assert cc.route(cc.FALL_CASES['fall-cin4'].c._replace(cin=3)).kernel == 'straight'
    # the edge of RAW: each case lacks exactly one of RAW's three conditions, and all three are lacked by some case
    lacks = set()
    for n, c in cc.RAW_EDGE_CASES.items():
        assert cc.route(c.c._replace(scale=False, shift=False, slope=1.0)).raw and not cc.route(c.c).raw, n
        lacks.add((c.c.scale, c.c.shift, c.c.slope != 1.0))
    assert lacks == {(True, False, False), (False, True, False), (False, False, True)}
    for n, calls in cc.MEAN_POSITIVE.items():
        assert {cc.route(c).kernel + str(cc.route(c).nblk) for c in calls} == {{'straight': 'straight1', 'gen1': 'general1', 'gen2': 'general2'}[n]}
    assert {cc.variant_name(cc.route(c)) for c in cc.MEAN_POSITIVE['straight']} == {'sl1-o3', 'sl1-o5-raw', 'sl1-o2'}


def test_refusals_one_per_return_in_the_entry_point_s_order():
    listed = [n for names in cc.REFUSAL_RETURNS.values() for n in names]
    assert listed == list(cc.REFUSALS)                                       # every refusal belongs to a return, in order
    for i, (key, names) in enumerate(cc.REFUSAL_RETURNS.items()):
        assert names, key
        for n in names:
            c, rc = cc.REFUSALS[n]
            assert cc.route(c).rc == rc != cc.OK, n
            assert cc.first_refusing_test(c) == i, n                         # ... and is refused by that return, not by an earlier one
    # each differs from an accepted call in the one respect it names
    base = cc.C(2, 3, 20, 18, 34, 'yps')
    assert cc.route(base).rc == cc.OK
    for n, (c, rc) in cc.REFUSALS.items():
        diff = [f for f in c._fields if getattr(c, f) != getattr(base, f)]
        assert 1 <= len(diff) <= (2 if 'odd' in n or n in ('height-0', 'width-0', 'stats+deterministic') else 8 if n in ('tiles>=2^31', 'stats+deterministic-aligned') else 1), (n, diff)
    assert cc.route(cc.REFUSALS['stats+deterministic'][0]._replace(det=False)).rc == cc.OK
    assert cc.route(cc.REFUSALS['stats+deterministic-aligned'][0]._replace(det=False)).kernel == 'straight'
    assert cc.route(cc.REFUSALS['tiles>=2^31'][0]._replace(B=(1 << 30) - 1)).rc == cc.OK
    # a call refused for two reasons answers the earlier one: Cin 5 with an ld below Cout is ENOSUP, an odd pooled map in deterministic mode is EINVAL
    assert cc.route(cc.C(2, 5, 20, 18, 34, 'yps', ypad=-1)).rc == cc.ENOSUP and cc.route(cc.C(2, 3, 20, 17, 34, 'yps', det=True)).rc == cc.EINVAL


def test_removing_a_sole_case_is_noticed():
    """The coverage tests above fail when a case that alone reaches a cell is taken out: shown here for one cell of each kind."""
    def without(table, name):
        return ({n: c for n, c in table.items() if n != name},)
    assert reached('sl1-o3 walk4', (cc.STRAIGHT_CASES,)) == ['sl1-o3-walk4'] and not reached('sl1-o3 walk4', without(cc.STRAIGHT_CASES, 'sl1-o3-walk4'))
    assert reached('cin1 gen2', (cc.TAP_CASES,)) == ['tap-cin1-cout40'] and not reached('cin1 gen2', without(cc.TAP_CASES, 'tap-cin1-cout40'))
    assert reached('straight walk7+') == ['sl1-o2-walk7'] and reached('general walk7+') == ['gwalk7-cin3']
    assert reached('cin2 walk4', (cc.GEN_WALK_CASES,)) == ['gwalk4-cin2']
    assert all(len(v) >= 1 for v in cc.REFUSAL_RETURNS.values()) and len(cc.REFUSAL_RETURNS['y != nullptr && ldy < Cout']) == 1


# ------------------------------------------------------------------------------------------------ y2_conv0_fwd_sel
def sel_reached(cell, without=None):
    return reached(cell, ({n: c for n, c in cc.SEL_CASES.items() if n != without},))


def test_sel_tables_reach_every_selecting_kernel_and_every_way_to_it():
    assert len(cc.VARIANTS) == 8 and cc.SEL_VARIANT not in cc.VARIANTS          # the macro list, and the ninth variant counted separately
    assert {cc.variant_name(cc.route(c.c)) for c in cc.SEL_CASES.values()} == {'sl1-o7-raw-sel', 'gen1-sel', 'gen2-sel'}
    assert all(c.c.sel and 'sel' in cc.claims_of(c.c) for c in cc.SEL_CASES.values())
    assert sel_reached('sl1-o7-raw-sel walk1 whole-tile') == ['sel-sl-small'] and sel_reached('sl1-o7-raw-sel walk3 steady-state uneven-walk') == ['sel-sl-walk3']
    assert cc.SEL_CASES['sel-sl-small'].c[:5] + cc.SEL_CASES['sel-sl-walk3'].c[:5] == tuple(x for s in ('small', 'walk3') for x in (cc.ALIGNED_SIZES[s][0][0], 3, 32) + cc.ALIGNED_SIZES[s][0][1:])
    # the stats-less aligned call: the shipped first layer on whole tiles, dense rows; with statistics it is the ninth variant, without gamma sl1-o3
    bug = cc.SEL_CASES['sel-nostats-aligned'].c
    assert (bug.B, bug.cin, bug.cout, bug.H, bug.W, bug.outs, bug.ypad, bug.ppad) == (1, 3, 32, 16, 32, 'yp', 0, 0) and cc.looks_aligned(bug)
    assert sel_reached('gen1-sel fallthrough out3') == ['sel-nostats-aligned']
    assert cc.variant_name(cc.route(bug._replace(outs='yps'))) == 'sl1-o7-raw-sel' and cc.variant_name(cc.route(bug._replace(sel=False))) == 'sl1-o3'
    # each fall-through differs from the ninth variant's call in one respect
    for name, field, value in (('sel-fall-cout64', 'cout', 32), ('sel-fall-ldz', 'ypad', 0), ('sel-fall-ldzs', 'ppad', 0), ('sel-fall-cin4', 'cin', 3), ('sel-nostats-aligned', 'outs', 'yps')):
        c = cc.SEL_CASES[name].c
        assert cc.route(c).kernel == 'general' and cc.variant_name(cc.route(c._replace(**{field: value}))) == 'sl1-o7-raw-sel', name
    assert sel_reached('gen2-sel fallthrough out7') == ['sel-fall-cout64'] and sel_reached('gen2-sel out3') == ['sel-fall-cout64-nostats']
    assert [n for n in sel_reached('gen1-sel fallthrough ld>cout')] == ['sel-fall-ldz', 'sel-fall-ldzs']
    assert sel_reached('gen1-sel cin4 whole-tile') == ['sel-fall-cin4']
    # the general kernel: channel masks, tap tables, geometry, the window form, a persistent walk
    assert [c.c.cout for n, c in cc.SEL_CASES.items() if n.startswith('sel-mask-')] == list(cc.MASK_COUTS) == [1, 31, 32, 33, 63, 64]
    for cout in cc.MASK_COUTS:
        c = cc.SEL_CASES['sel-mask-cout%d' % cout].c
        assert c[:5] == (2, 3, cout, 18, 34) and cc.route(c).nblk == (1 if cout <= 32 else 2) and c.outs == 'yps'
    for cin in (1, 2, 3, 4):
        assert 'sel-tap-cin%d' % cin in sel_reached('cin%d ragged-both out7' % cin)
        assert cin == 3 or sel_reached('cin%d ragged-both' % cin, without='sel-tap-cin%d' % cin) == []          # (Cin 3 is everywhere; the others have this case alone)
        assert cc.SEL_CASES['sel-tap-cin%d' % cin].c[3:5] == (18, 34)
    assert {cc.route(cc.SEL_CASES['sel-tap-cin%d' % cin].c).nblk for cin in (1, 2, 3, 4)} == {1, 2}
    assert cc.SEL_CASES['sel-geo-2x2'].c[3:5] == (2, 2) and cc.SEL_CASES['sel-geo-20x36'].c[3:5] == (20, 36)
    assert sel_reached('gen1-sel one-tile-image ragged-both', without='sel-geo-2x2') == [] and sel_reached('gen1-sel ragged-bottom ragged-right whole-tile', without='sel-geo-20x36') == []
    w = cc.SEL_CASES['sel-window'].c
    assert (w.ypad, w.yoff, w.ppad, w.poff) == (5, 3, 6, 1) and sel_reached('gen1-sel channel-offset ld%4') == ['sel-window']
    assert sel_reached('gen1-sel walk4 buffer-reuse uneven-walk') == ['sel-gwalk4-cin3'] and cc.SEL_CASES['sel-gwalk4-cin3'].c[:5] == cc.GEN_WALK_CASES['gwalk4-cin3'].c[:5]
    # the random regime runs what is small; only the two walks are not
    assert [n for n, c in cc.SEL_CASES.items() if c.c.B > cc.SEL_RANDOM_MAX_B] == ['sel-sl-walk3', 'sel-gwalk4-cin3']


def test_sel_refusals_one_per_return_in_the_entry_point_s_order():
    listed = [n for names in cc.SEL_REFUSAL_RETURNS.values() for n in names]
    assert listed == list(cc.SEL_REFUSALS)
    base = cc.S(2, 3, 20, 18, 34)
    assert cc.route(base).rc == cc.OK and cc.variant_name(cc.route(base)) == 'gen1-sel'
    for i, (key, names) in enumerate(cc.SEL_REFUSAL_RETURNS.items()):
        assert names, key
        for n in names:
            c, rc = cc.SEL_REFUSALS[n]
            assert cc.is_sel_entry(c) and cc.route(c).rc == rc != cc.OK, n
            assert cc.sel_first_refusing_test(c) == i, n
            diff = [f for f in c._fields if getattr(c, f) != getattr(base, f)]
            assert 1 <= len(diff) <= (5 if n in ('sel-tiles>=2^31', 'sel-stats+deterministic-aligned') else 2 if n == 'sel-gamma-null' else 1), (n, diff)
    assert {n for n in listed if 'odd' in n} == {'sel-odd-height', 'sel-odd-width'} and 'sel-ldzs<cout' in listed and 'sel-stats+deterministic' in listed
    assert cc.route(cc.SEL_REFUSALS['sel-stats+deterministic'][0]._replace(det=False)).rc == cc.OK
    assert cc.route(cc.SEL_REFUSALS['sel-stats+deterministic'][0]._replace(outs='yp')).rc == cc.OK          # deterministic mode without statistics: accepted
    assert cc.variant_name(cc.route(cc.SEL_REFUSALS['sel-stats+deterministic-aligned'][0]._replace(det=False))) == 'sl1-o7-raw-sel'
    assert cc.route(cc.SEL_REFUSALS['sel-tiles>=2^31'][0]._replace(B=(1 << 30) - 1)).rc == cc.OK
    # the entry's own refusal comes first: gamma NULL with x NULL, Cin 5 or an odd height is still EINVAL
    assert cc.route(cc.S(2, 5, 20, 18, 34, nog=True)).rc == cc.EINVAL and cc.route(cc.S(2, 5, 20, 18, 34)).rc == cc.ENOSUP
