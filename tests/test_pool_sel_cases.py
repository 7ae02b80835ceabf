"""CPU check of the z_sel streaming case tables (tests/pool_sel_cases.py): the mirror of bn_act_fwd_impl / bn_act_bwd_impl behind y2_bn_act_fwd_sel and
y2_bn_act_bwd_sel agrees with what every case claims, and the tables reach the vector and the scalar kernel through every single cause, every reduction form
of pass 1 with every gridDim.y of the block-reduce kernel, the cases that must keep atomics, deterministic mode and every refusal.  The mirror's constants
and conditions are pinned to the text of csrc/train.hip; the GPU tests (tests/test_gpu_pool_sel.py) observe the reduction form by kernel name."""
import os
import re

import pytest

import pool_sel_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'yolo2-pytorch_amd', 'csrc')
TABLES = {False: pc.FWD_CASES, True: pc.BWD_CASES}
ALL = [(('bwd-' if b else 'fwd-') + n, b, c) for b, t in TABLES.items() for n, c in t.items()]


def reached(cell, backward, without=None):
    cell = set(cell.split())
    return [n for n, c in TABLES[backward].items() if n != without and cell <= c.claims and cell <= pc.claims_of(c.c, backward)]


def test_mirror_constants_are_the_sources():
    """Literal matches against train.hip: they fail on any edit of the matched lines.  When this fails, re-read fwd_route / bwd_route / the vec terms in
    pool_sel_cases.py against the source before updating the strings."""
    src = open(os.path.join(CSRC, 'train.hip')).read()
    common = open(os.path.join(CSRC, 'common.h')).read()
    assert int(re.search(r'constexpr int Y2_NUM_CU = (\d+);', common).group(1)) == pc.NUM_CU
    # act_grid
    for line in ('int g = 256, r = Cg;', 'const int unit = Cg / g;', 'long long want = (total + 256 * 8 - 1) / (256 * 8);', 'const long long cap = (long long)Y2_NUM_CU * 8;',
                 'return (int)(((want + unit - 1) / unit) * unit);'):
        assert line in src, line
    # the two entries: what they pass on
    assert 'return bn_act_fwd_impl(z, scale, shift, slope, nullptr, 0, nullptr, y_pool, B, H, W, C, ldz, 0, 0, ldp, poff, 0, stream, z_sel, ldzs);' in src
    assert ('return bn_act_bwd_impl(z, scale, shift, mean, invstd, gamma, slope, nullptr, 0, 0, 0, dy_pool, ldp, poff, nullptr, 0, nullptr, 0, nullptr, 0,\n'
            '                           sums, dz, ldd, B, H, W, C, ldz, 1, stream, nullptr, 0, z_sel, ldzs);') in src
    # the refusals, in order, from each entry on
    for entry, impl, table in (('extern "C" int y2_bn_act_fwd_sel', 'static int bn_act_fwd_impl(const float* z, const float* scale, const float* shift, float slope, const float* residual, int ldr, float* y, float* y_pool,\n', pc.FWD_REFUSAL_RETURNS),
                               ('extern "C" int y2_bn_act_bwd_sel', 'static int bn_act_bwd_impl(', pc.BWD_REFUSAL_RETURNS)):
        body = src[src.index(impl):]
        body = body[:body.index('\n}\n')]
        own = src[src.index(entry):]
        own = own[:own.index('\n}\n')]
        returns = re.findall(r'if \((.*)\) return (Y2_E\w+);', own) + re.findall(r'if \((.*)\) return (Y2_E\w+);', body)
        # (returns that no call of these entries can reach: a residual's stride, a dres without dz)
        returns = [r for r in returns if not r[0].startswith('residual != nullptr && ldr < C') and not r[0].startswith('dz == nullptr && dres != nullptr')]
        assert all(r[0].startswith(k) for k, r in zip(table, returns)) and len(returns) == len(table)
        codes = {k: {pc.OK: None, pc.EINVAL: 'Y2_EINVAL', pc.ENOSUP: 'Y2_ENOSUP'}[(pc.BWD_REFUSALS if table is pc.BWD_REFUSAL_RETURNS else pc.FWD_REFUSALS)[names[0]][1]] for k, names in table.items()}
        assert [r[1] for r in returns] == [codes[k] for k in table]
    # vec, term by term
    assert ('const bool vec = (!residual || (!(ldr & 3) && y2_aligned16(residual))) && !(C & 3) && !(ldz & 3) && (!y || (!(ldy & 3) && !(coff & 3) && y2_aligned16(y))) && '
            '(!pool || (!(ldp & 3) && !(poff & 3) && y2_aligned16(y_pool))) && y2_aligned16(z) &&\n                     (!z_sel || (!(ldzs & 3) && y2_aligned16(z_sel)));') in src
    assert ('!(C & 3) && !(ldz & 3) && (!dz || (!(ldd & 3) && y2_aligned16(dz))) && y2_aligned16(z) &&\n'
            '                     (!dy_full || (!(ldf & 3) && !(foff & 3) && y2_aligned16(dy_full))) && (!pool || (!(ldp & 3) && !(poff & 3) && y2_aligned16(dy_pool))) &&\n'
            '                     (!z_sel || (!(ldzs & 3) && y2_aligned16(z_sel)));') in src
    assert 'const int grid = act_grid(total, vec ? C / 4 : C);' in src and 'const int Cg = vec ? C / 4 : C;' in src and 'const int grid = act_grid(total, Cg);' in src
    # the three reductions of pass 1
    assert 'a.block_partial = (dz != nullptr && !aliased && !y2_det.on && ldd == C && grid > 16 && (long long)grid * 2 * C <= npix * ldd) ? dz : nullptr;' in src
    assert 'overlaps(z_sel, opix * ldzs));' in src
    assert 'if (dz == nullptr && park != nullptr' in src          # (the park buffer: NULL from both ABI entries)
    assert 'const long long prow = (long long)grid * 256 / Cg;' in src
    assert 'dim3((unsigned)y2_cdiv(2 * C, 64), (unsigned)(grid >= 512 ? 16 : (grid >= 64 ? 4 : 1))), dim3(1024), 0, s, a.block_partial, grid, 2 * C, sums);' in src
    assert 'const int rc_ = y2_det_reduce_f32(a.partial, (int)prow, (long long)2 * C, (long long)2 * C, sums, nullptr, s);' in src
    assert 'Y2_LAUNCH("det_reduce_rows_kernel", 0.0, det_reduce_rows_kernel<float>' in open(os.path.join(CSRC, 'det.hip')).read()


def test_mirror_known_answers():
    assert pc.act_grid(648 * 64, 64) == 21 and pc.act_grid(2880, 10) == 5 and pc.act_grid(1, 7) == 7 and pc.act_grid(1 << 40, 64) == 2048
    # the four pooled blocks of a Darknet step at batch 64, 416 x 416 (C 32, 64, 128, 256): the capped grid, 16 slices
    for C, H in ((32, 416), (64, 208), (128, 104), (256, 52)):
        r = pc.bwd_route(pc.K(64, H, H, C))
        assert (r.vec, r.form, r.slices) == (True, 'parked', 16) and r.grid == (2048 if H > 52 else 1352), (C, r)
    r = pc.bwd_route(pc.K(*pc.PARK))
    assert (r.grid, r.form, r.slices, r.loops, r.prow) == (21, 'parked', 1, 8, 84)
    assert pc.bwd_route(pc.K(2, 34, 34, 256)).grid == 19 and pc.bwd_route(pc.K(2, 32, 32, 256)).form == 'atomics'
    assert pc.BWD_CASES['parked4'].c.H == 64 and pc.bwd_route(pc.BWD_CASES['parked4'].c).grid == 64
    assert pc.bwd_route(pc.BWD_CASES['parked16-scalar'].c).grid >= 512 and pc.bwd_route(pc.K(4, pc.BWD_CASES['parked16-scalar'].c.H - 2, pc.BWD_CASES['parked16-scalar'].c.W - 2, 30)).slices == 4


@pytest.mark.parametrize('name', [n for n, _, _ in ALL])
def test_case_reaches_what_it_claims(name):
    _, backward, c = [a for a in ALL if a[0] == name][0]
    got = pc.claims_of(c.c, backward)
    assert c.claims <= got, (sorted(c.claims - got), sorted(got))
    assert c.c.B * c.c.H * c.c.W * (c.c.C + max(c.c.zpad, c.c.dpad)) <= 5 << 20          # a test of seconds: at most 20 MB per full-resolution map
    if c.c.dz == 'alias':
        assert c.c.dpad == 0 and c.c.dmis == 0
    assert (c.c.dz == 'strided') == (c.c.dpad > 0) and not c.c.null


def test_tables_reach_both_kernels_through_every_single_cause():
    for backward, terms in ((False, pc.fwd_vec_terms), (True, pc.bwd_vec_terms)):
        every = terms(pc.K(C=6, zpad=1, ppad=2, poff=1, spad=1, dpad=1, zmis=1, pmis=1, smis=1, dmis=1, dz='strided'))
        assert len(every) == (10 if backward else 8)
        for t in every:
            names = reached('single-cause scalar:' + t, backward)
            assert len(names) == 1, (t, names)                       # one case per cause, every other term aligned
            assert not reached('single-cause scalar:' + t, backward, without=names[0])
            c = TABLES[backward][names[0]].c
            assert terms(c) == [t] and (pc.bwd_route if backward else pc.fwd_route)(c).vec is False
        assert reached('vec', backward) and reached('vec ldz>C ldp>C poff>0 ldzs>C', backward) and reached('scalar ldz>C ldp>C poff>0 ldzs>C loops', backward)
        assert reached('vec cg-not-dividing-256 multi-block', backward) and reached('vec loops multi-block', backward)
    assert reached('vec affine-null', False) and reached('scalar affine-null', False)
    assert pc.FWD_CASES['vec-cg10'].c.C == 40 and pc.fwd_route(pc.FWD_CASES['vec-cg10'].c).grid % 5 == 0


def test_tables_reach_every_reduction_form():
    for form in ('atomics', 'parked1', 'parked4', 'parked16', 'det'):
        assert reached(form, True), form
    for form in ('parked1', 'parked4', 'parked16'):
        names = reached(form, True)
        assert len(names) == 1 and not reached(form, True, without=names[0])          # removing a sole case is noticed
    # the thresholds themselves
    g = {n: pc.bwd_route(pc.BWD_CASES[n].c).grid for n in pc.BWD_CASES}
    assert g['parked1'] == 21 and g['parked4'] == 64 and 512 <= g['parked16-scalar'] and g['atomics-grid16'] == 16
    # the cases that must keep atomics differ from the parked one in the one respect they name
    park = pc.BWD_CASES['parked1'].c
    for name, change in (('atomics-sums-only', dict(dz='null')), ('atomics-strided-dz', dict(dz='strided', dpad=4)), ('atomics-dz-aliases-z_sel', dict(dz='alias')), ('det-vec', dict(det=True))):
        assert pc.BWD_CASES[name].c == park._replace(**change) and pc.bwd_route(pc.BWD_CASES[name].c).form != 'parked', name
    assert reached('atomics grid>16 ldd!=C', True) == ['atomics-strided-dz'] and reached('atomics grid>16 dz-alias', True) == ['atomics-dz-aliases-z_sel']
    assert pc.bwd_route(pc.BWD_CASES['atomics-grid16'].c._replace(H=34)).grid > 16
    assert reached('dz-null', True) and reached('dz-dense', True) and reached('det dz-null scalar', True) and reached('det dz-dense vec grid>16', True)


@pytest.mark.parametrize('backward', [False, True])
def test_refusals_one_per_condition_in_the_source_s_order(backward):
    refusals, returns, route = (pc.BWD_REFUSALS, pc.BWD_REFUSAL_RETURNS, pc.bwd_route) if backward else (pc.FWD_REFUSALS, pc.FWD_REFUSAL_RETURNS, pc.fwd_route)
    assert [n for names in returns.values() for n in names] == list(refusals)
    base = pc.K()
    assert route(base).rc == pc.OK
    for n, (c, rc) in refusals.items():
        assert route(c).rc == rc != pc.OK, n
        diff = [f for f in c._fields if getattr(c, f) != getattr(base, f)]
        assert 1 <= len(diff) <= (3 if n == 'windows>=2^31' else 5 if n == 'deterministic-scratch-too-small' else 1), (n, diff)
    # the order, where the codes tell it: an odd size or a missing pointer with C > 8192 is EINVAL, C > 8192 with too many windows or too small a scratch ENOSUP
    assert route(pc.K(C=pc.MAX_C + 4, H=7)).rc == pc.EINVAL and route(pc.K(C=pc.MAX_C + 4, spad=-1)).rc == pc.EINVAL and route(pc.K(B=pc.MAX_PIX, H=2, W=2, null=('z',))).rc == pc.EINVAL
    assert route(pc.K(B=pc.MAX_PIX, H=2, W=2, C=pc.MAX_C + 4)).rc == pc.ENOSUP
    if backward:
        assert route(pc.K(C=pc.MAX_C + 4, null=('gamma',))).rc == pc.EINVAL and route(pc.K(C=pc.MAX_C + 4, det_small=True)).rc == pc.ENOSUP
        small = pc.BWD_REFUSALS['deterministic-scratch-too-small'][0]
        assert route(small._replace(det_small=False, det=True)).form == 'det' and route(small._replace(det_small=False)).form == 'parked' and route(pc.K(det_small=True)).rc == pc.OK
        assert 'workspace_bytes < (1ll << 20)' in open(os.path.join(CSRC, 'det.hip')).read() and pc.DET_SMALL_BYTES == 1 << 20
    assert len(returns) == (8 if backward else 5)
