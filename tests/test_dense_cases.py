"""CPU check of the pre-activation case tables (tests/dense_cases.py): the mirror of the host code of csrc/dense.hip agrees with what every case
claims to reach, the tables cover all sixteen preact_gemm_kernel instantiations with a ragged last row tile, a K that is no multiple of 4 with one
slab and with several, every single reason for the element-wise loader and for the scalar element-wise kernels, and CV x POOL x has_bn x
accumulate of y2_preact_bwd; the mirror's refusals are the source text's (the library is called with refused arguments in tests/test_gpu_dense.py)."""
import os
import re

import pytest

import dense_cases as dn
import dw_cases as dc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'yolo2-pytorch_amd', 'csrc')


def body(src, start, end):
    return src[src.index(start):src.index(end, src.index(start))]


def test_mirror_constants_are_the_sources():
    dense = open(os.path.join(CSRC, 'dense.hip')).read()
    dw = open(os.path.join(CSRC, 'dwconv.hip')).read()
    det = open(os.path.join(CSRC, 'det.hip')).read()
    assert int(re.search(r'constexpr int PE_THREADS = (\d+);', dense).group(1)) == dn.PE_THREADS == dc.DW_THREADS
    assert 'constexpr int PE_MAX_BLOCKS = Y2_NUM_CU * 8;' in dense and dn.PE_MAX_BLOCKS == dc.DW_MAX_BLOCKS
    assert int(re.search(r'constexpr int PG_BK = (\d+);', dense).group(1)) == dn.PG_BK
    # pe_grid is dw_grid: the same statements on the same constants
    norm = lambda s: re.sub(r'\s+', ' ', s.replace('PE_', 'DW_').replace('PeGrid', 'DwGrid').replace('g.CV = CV;', ''))          # noqa: E731
    assert norm(body(dense, 'g.Cg = C / CV;', 'return g;')) == norm(body(dw, 'g.Cg = C / CV;', 'return g;'))
    assert 'const int NT = N > 64 ? 2 : 1;' in dense and 'a.gn = (N + 64 * NT - 1) / (64 * NT);' in dense
    assert 'const int MT = ((M + 127) / 128) * a.gn >= Y2_NUM_CU ? 2 : 1;' in dense
    assert 'const bool vec = !(K & 3) && !(ldx & 3) && y2_aligned16(x) && y2_aligned16(w) && vec_ptr_ok(pre_scale) && vec_ptr_ok(pre_shift);' in dense
    assert 'const int CV = (!(C & 3) && !(ldx & 3) && !(ldo & 3) && y2_aligned16(x) && y2_aligned16(out)) ? 4 : 1;' in dense
    assert ('const int CV = (!(C & 3) && !(ldx & 3) && !(ldda & 3) && !(lddx & 3) && y2_aligned16(x) && y2_aligned16(dA) && y2_aligned16(dx)) ? 4 : 1;'
            in dense)
    assert 'pe_grid(P, C, CV, 1)' in dense and 'pe_grid(P, C, CV, %d)' % dn.PE_BWD_MIN_PIX in dense
    assert '(size_t)g.gx * 2 * C * sizeof(float) > y2_det.bytes' in dense
    assert 'workspace_bytes < (1ll << 20)' in det and dn.DET_MIN_BYTES == 1 << 20
    launches = re.findall(r'launch_preact_gemm<(\d), (\d)>\(a, vec, pool != 0, s\)', dense)
    assert sorted(launches) == [('1', '1'), ('1', '2'), ('2', '1'), ('2', '2')]


def test_mirror_on_the_shapes_of_the_real_workload():
    # DenseNet-121 at 416: transition 1 (K = 256 -> N = 128, pooled, M = B * 52 * 52) takes the 128-row tile from batch 13 on
    assert dn.gemm_plan(12 * 52 * 52, 128).MT == 1 and dn.gemm_plan(13 * 52 * 52, 128).MT == 2
    assert dn.gemm_plan(64 * 26 * 26, 128) == dn.GemmPlan(2, 2, 1, 338, 338)        # the one MT = 2 case of tests/test_gpu_densenet.py: whole tiles
    assert dn.gemm_plan(126, 30) == dn.GemmPlan(1, 1, 1, 2, 2) and dn.gemm_plan(297, 200) == dn.GemmPlan(1, 2, 2, 5, 10)
    assert dn.det_need_bytes(2 * 12 * 12, 64, 4) == 3 * 2 * 64 * 4                   # Cg 16, TP 16: ceil(288 / 128) pixel blocks


@pytest.mark.parametrize('name', list(dn.GEMM_CASES))
def test_gemm_case_reaches_what_it_claims(name):
    c = dn.GEMM_CASES[name]
    B, H, W, K, N, pool = c.shape
    got, p = dn.gemm_derive(c)
    assert set(c.claims) <= got, (sorted(set(c.claims) - got), p)
    assert dn.gemm_accepts(B, H, W, K, K + c.xpad, N, c.ldy, c.coff, pool)
    s = dn.pe_shape_ok(B, H, W, K, pool)
    assert max(s.Pin * (K + c.xpad), s.Pout * c.ldy) <= dn.MAX_ELEMENTS
    assert all(0 <= v < 4 for v in c.off.values())


def test_gemm_table_covers_the_matrix():
    cells = set()
    for c in dn.GEMM_CASES.values():
        cl = set(c.claims)
        if 'ragged-M' in cl and {'mt1', 'mt2'} & cl and {'nt1', 'nt2'} & cl:
            cells.add(('mt2' in cl, 'nt2' in cl, 'vec' in cl, 'pool' in cl))
            assert ('vec' in cl) != any(x.startswith('nonvec-by-') for x in cl) and ('pool' in cl) != ('nopool' in cl)
    assert len(cells) == 16
    claimed = lambda *cl: any(set(cl) <= set(c.claims) for c in dn.GEMM_CASES.values())          # noqa: E731
    assert claimed('k-quad-tail', 'one-slab') and claimed('k-quad-tail', 'many-slabs')
    assert claimed('vec', 'k-tail', 'one-slab') and claimed('vec', 'k-tail', 'many-slabs') and claimed('gn>1', 'mt1') and claimed('gn>1', 'mt2')
    assert claimed('coff>0', 'ldy>coff+N') and claimed('ragged-N', 'nt1') and claimed('ragged-N', 'nt2')
    assert {c.shape[3] for c in dn.GEMM_CASES.values()} >= {1, 3, 30, 33, 61}
    assert dn.GEMM_CASES['g11-nonvec'].shape[3] % dn.PG_BK == 1                                  # a second slab of a single k
    alone = [next(iter(r)) for r in (dn.gemm_nonvec_reasons(c) for c in dn.GEMM_CASES.values()) if len(r) == 1]
    for reason in ['nonvec-by-K', 'nonvec-by-stride'] + ['nonvec-by-ptr:' + o for o in dn.GEMM_OPERANDS]:
        assert reason in alone and claimed(reason), reason
    assert [('vec' in dn.GEMM_CASES[n].claims) for n in dn.GEMM_FORM_CASES] == [True, False]
    assert set(dn.GEMM_FORMS) == {'plain', 'affine-relu', 'affine-slope0.1', 'scale-only', 'shift-only', 'null-pre'}


def test_gemm_vec_decision_term_by_term():
    ok = dict(x=0, w=4, pre_scale=None, pre_shift=0)
    assert dn.gemm_vec(8, 12, ok)
    assert not dn.gemm_vec(6, 12, ok) and not dn.gemm_vec(8, 13, ok)
    for o in dn.GEMM_OPERANDS:
        assert not dn.gemm_vec(8, 12, dict(ok, **{o: 1})), o
    assert dn.gemm_vec(8, 12, dict(ok, pre_shift=None))


@pytest.mark.parametrize('entry,name', [('fwd', n) for n in dn.FWD_CASES] + [('bwd', n) for n in dn.BWD_CASES])
def test_elementwise_case_reaches_what_it_claims(entry, name):
    c = (dn.FWD_CASES if entry == 'fwd' else dn.BWD_CASES)[name]
    B, C, H, W, pool = c.shape
    got, g = dn.pe_derive(c, entry)
    assert set(c.claims) <= got, (sorted(set(c.claims) - got), g)
    s = dn.pe_shape_ok(B, H, W, C, pool)
    lds = [dn.ld(c, o) for o in c.pad]
    assert len(set(lds)) == len(lds)                       # no two operands share a pixel stride
    assert s.Pin * max(lds) <= dn.MAX_ELEMENTS and all(0 <= v < 4 for v in c.off.values())


def test_elementwise_tables_cover_the_matrix():
    claimed = lambda table, *cl: any(set(cl) <= set(c.claims) for c in table.values())          # noqa: E731
    for cv in ('cv4', 'cv1'):
        for pool in ('pool', 'nopool'):
            assert claimed(dn.FWD_CASES, cv, pool, 'capped', 'walk>=2') and claimed(dn.FWD_CASES, cv, pool, 'walk1', 'gy1')
            assert claimed(dn.FWD_CASES, cv, pool, 'gy>1', 'ragged-channel-block', 'walk1')
            assert claimed(dn.BWD_CASES, cv, pool, 'gy1') and claimed(dn.BWD_CASES, cv, pool, 'gy>1', 'ragged-channel-block')
    for table, entry, ops in ((dn.FWD_CASES, 'fwd', dn.FWD_OPERANDS), (dn.BWD_CASES, 'bwd', dn.BWD_OPERANDS)):
        alone = [next(iter(r)) for r in (dn.pe_scalar_reasons(c, entry) for c in table.values()) if len(r) == 1]
        for reason in ['cv1-by-C'] + ['cv1-by-%s:%s' % (k, o) for k in ('ptr', 'stride') for o in ops]:
            assert reason in alone, (entry, reason)
            assert claimed(table, reason), (entry, reason)
    # y2_preact_bwd: CV x POOL x has_bn x accumulate - the GPU test runs every case with every has_bn and both accumulate values
    assert dn.HAS_BN == (1, 2, 0) and dn.ACCUMULATE == (0, 1)
    det = {(('cv4' in dn.BWD_CASES[n].claims), ('pool' in dn.BWD_CASES[n].claims)) for n in dn.DET_CASES}
    assert len(det) == 4 and all('gy>1' in dn.BWD_CASES[n].claims for n in dn.DET_CASES)
    assert [('cv4' in dn.FWD_CASES[n].claims) for n in dn.FWD_FORM_CASES] == [True, False]
    assert {('pool' in dn.FWD_CASES[n].claims) for n in dn.FWD_FORM_CASES} == {True, False}


def test_deterministic_workspace_need():
    B, C, H, W, pool = dn.DET_TOO_SMALL
    need = dn.det_need_bytes(B * H * W, C, 4)
    assert need > dn.DET_MIN_BYTES and need == 133 * 2 * 1024 * 4
    # the scalar path's partial sums never outgrow the minimum scratch: gx <= 2048 / gy rows of 8 C bytes, gy >= C / 64
    for Cs in (1, 6, 64, 65, 1000, 1024, 1028, 4100):
        assert dn.det_need_bytes(10 ** 9, Cs, 1) <= dn.DET_MIN_BYTES, Cs
    for n in dn.DET_CASES:
        c = dn.BWD_CASES[n]
        assert dn.det_need_bytes(c.shape[0] * c.shape[2] * c.shape[3], c.shape[1], dn.pe_derive(c, 'bwd')[1].CV) < dn.DET_MIN_BYTES


# ------------------------------------------------------------------------------------------------ the refusals: mirror and source text
BAD_SHAPES = ((0, 6, 8, 5, 0), (2, 0, 8, 5, 0), (2, 6, 0, 5, 0), (2, 6, 8, 0, 0), (2, 6, 8, 5, 2), (2, 6, 8, 5, -1), (2, 7, 8, 5, 1), (2, 6, 9, 5, 1),
              (2, 46341, 46341, 1, 0))
BAD_PLACEMENTS = ((4, 4, 4, 0), (5, 0, 4, 0), (5, 4, 4, -1), (5, 4, 3, 0), (5, 4, 6, 3))          # (ldx, N, ldy, coff) for K = 5: ldx < K, N = 0, coff < 0, ldy < N, ldy < coff + N


def test_refusals():
    """The mirror's refusals and the source text they mirror.  No entry point of csrc/dense.hip answers without a launch, so the library is called
    with refused arguments only in tests/test_gpu_dense.py, on real buffers."""
    assert dn.pe_shape_ok(2, 6, 8, 5, 1) == dc.Shape(96, 24, 3, 4) and dn.pe_shape_ok(2, 7, 9, 5, 0) == dc.Shape(126, 126, 7, 9)
    for bad in BAD_SHAPES:
        B, H, W, C, pool = bad
        assert dn.pe_shape_ok(*bad) is None, bad
        assert not dn.gemm_accepts(B, H, W, C, C, 4, 4, 0, pool)
    good = (2, 6, 8, 5)
    for ldx, N, ldy, coff in BAD_PLACEMENTS:
        assert not dn.gemm_accepts(*good, ldx, N, ldy, coff, 1)
    assert dn.gemm_accepts(*good, 5, 4, 7, 3, 1)
    dense = open(os.path.join(CSRC, 'dense.hip')).read()
    assert 'if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (pool != 0 && pool != 1)) return false;' in dense
    assert 'if (pool && ((H | W) & 1)) return false;' in dense and 'return *Pin < 0x7fffffffLL;' in dense
    assert ('if (!x || !w || !y || !pe_shape_ok(B, H, W, K, pool, &Pin, &M, &Ho, &Wo) || N <= 0 || ldx < K || coff < 0 || ldy < coff + N) return Y2_EINVAL;'
            in dense)
    assert 'if (!x || !out || !pe_shape_ok(B, H, W, C, pool, &Pin, &P, &Ho, &Wo) || ldx < C || ldo < C) return Y2_EINVAL;' in dense
    assert ('if (!x || !dA || !sums || !dx || !pe_shape_ok(B, H, W, C, pool, &P, &Pout, &Ho, &Wo) || ldx < C || ldda < C || lddx < C) return Y2_EINVAL;'
            in dense)
    assert 'if (has_bn < 0 || has_bn > 2 || (has_bn && (!mean || !invstd || !gamma))) return Y2_EINVAL;' in dense
