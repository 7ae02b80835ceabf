"""CPU check of the depthwise-convolution case table (tests/dw_cases.py): the mirror of the host code of csrc/dwconv.hip agrees with what every
case claims to reach, the table as a whole covers vector width x channel blocks x steps per thread for every entry point and every reason for
the scalar path, and the mirror agrees with the built library where the library answers without touching memory (the workspace query) and with
the source text of the refusals; the launching entry points are only called on real buffers, in tests/test_gpu_dwconv.py."""
import os
import random
import re

import pytest

import dw_cases as dc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'yolo2-pytorch_amd', 'csrc')


def test_mirror_constants_are_the_sources():
    common = open(os.path.join(CSRC, 'common.h')).read()
    dw = open(os.path.join(CSRC, 'dwconv.hip')).read()
    hdr = open(os.path.join(os.path.dirname(CSRC), '..', 'include', 'yolo2_hip.h')).read()
    assert int(re.search(r'constexpr int Y2_NUM_CU = (\d+);', common).group(1)) == dc.NUM_CU
    assert int(re.search(r'constexpr int DW_THREADS = (\d+);', dw).group(1)) == dc.DW_THREADS
    assert 'constexpr int DW_MAX_BLOCKS = Y2_NUM_CU * 8;' in dw and dc.DW_MAX_BLOCKS == dc.NUM_CU * 8
    assert int(re.search(r'constexpr int DW_WGRAD_MIN_PIX = (\d+);', dw).group(1)) == dc.DW_WGRAD_MIN_PIX
    assert int(re.search(r'#define Y2_STATS_REPL (\d+)', hdr).group(1)) == dc.STATS_REPL
    assert 'while (g.TC < g.Cg && g.TC < 64) g.TC *= 2;' in dw and 'long long cap = DW_MAX_BLOCKS / g.gy;' in dw
    assert 'return !(C & 3) && !(lda & 3) && !(ldb & 3) && y2_aligned16(a) && y2_aligned16(b);' in dw
    # the operands each entry point hands to dw_vec_ok, and the pixel count and min_pix it hands to dw_grid
    assert 'dw_vec_ok(C, ldx, ldy, x, y)' in dw and 'dw_vec_ok(C, ldz, lddx, dz, dx)' in dw and 'dw_vec_ok(C, ldx, ldz, x, dz)' in dw
    assert dw.count('dw_grid(P, C, CV, 1)') == 2 and dw.count('dw_grid(P, C, CV, DW_WGRAD_MIN_PIX)') == 2


def test_mirror_on_the_shapes_of_the_real_workload():
    g = dc.dw_grid(64 * 13 * 13, 1024, 4, 1)              # MobileNet at 416, batch 64: the last units
    assert (g.TC, g.TP, g.gy, g.gx, g.capped, g.steps) == (64, 4, 4, 512, True, 6)
    g = dc.dw_grid(2 * 13 * 13, 1024, 4, 1)               # the largest shape of tests/test_gpu_mobilenet.py: one pixel per thread
    assert (g.gy, g.capped, g.steps, g.ragged) == (4, False, 1, False)
    assert dc.dw_grid(1, 1, 1, 1) == dc.Grid(1, 1, 1, 256, 1, 1, False, 1, False)
    assert dc.dw_grid(10 ** 9, 8192, 1, 1).gx == 16 and dc.dw_grid(10 ** 9, 1 << 20, 1, 1).gx == 1          # cap = max(2048 / gy, 1)


@pytest.mark.parametrize('entry', list(dc.ENTRIES))
@pytest.mark.parametrize('name', list(dc.CASES))
def test_case_reaches_what_it_claims(name, entry):
    c = dc.CASES[name]
    got, g = dc.derive(c, entry)
    assert set(c.claims[entry]) <= got, (sorted(set(c.claims[entry]) - got), g)
    assert {'cv4', 'cv1'} & set(c.claims[entry])           # every case says which width it is there for


@pytest.mark.parametrize('name', list(dc.CASES))
def test_case_layout(name):
    c = dc.CASES[name]
    B, C, H, W, stride = c.shape
    s = dc.dw_shape_ok(B, H, W, C, stride)
    assert s is not None
    assert max((s.Pin if o in ('x', 'dx') else s.Pout) * dc.ld(c, o) for o in dc.OPERANDS) <= dc.MAX_ELEMENTS
    for entry, ((a, b), _, _) in dc.ENTRIES.items():
        assert dc.ld(c, a) != dc.ld(c, b), (entry, a, b)   # a stride taken from the other operand addresses the wrong element
    assert all(0 <= v < 4 for v in c.off.values())


def test_table_covers_the_matrix():
    for entry in dc.ENTRIES:
        seen = set()
        for c in dc.CASES.values():
            cl = set(c.claims[entry])
            cv = 'cv4' if 'cv4' in cl else 'cv1'
            gy = 'gy1' if 'gy1' in cl else ('gy>1+ragged' if {'gy>1', 'ragged-channel-block'} <= cl else None)
            walk = 'walk1' if 'walk1' in cl else ('walk>=2' if 'walk>=2' in cl else None)
            seen.add((cv, gy))
            seen.add((cv, gy, walk))
        want = {(cv, gy) for cv in ('cv4', 'cv1') for gy in ('gy1', 'gy>1+ragged')}
        if entry != 'wgrad':
            want |= {(cv, gy, walk) for cv, gy in want for walk in ('walk1', 'walk>=2')}
        assert want <= seen, (entry, sorted(want - seen, key=str))
        if entry != 'wgrad':                                # a capped grid is what makes a min_pix = 1 thread walk
            assert all('capped' in c.claims[entry] for c in dc.CASES.values() if 'walk>=2' in c.claims[entry])
    assert any({'capped', 'gy>1', 'cv4'} <= set(c.claims['fwd']) and 'ragged-channel-block' not in c.claims['fwd'] for c in dc.CASES.values())
    assert sum('stats-copies>32' in c.claims['fwd'] for c in dc.CASES.values()) >= 2
    for claim in ('stride1', 'stride2', 'odd-map', 'even-map', '1x1-map', 'TC1', 'TC2', 'TC8', 'TC16', 'TC64'):
        assert any(claim in c.claims['fwd'] for c in dc.CASES.values()), claim
    for entry in ('fwd', 'dgrad'):                          # both strides capped
        assert {s for c in dc.CASES.values() for s in ('stride1', 'stride2') if {s, 'capped'} <= dc.derive(c, entry)[0]} == {'stride1', 'stride2'}


def test_every_reason_for_the_scalar_path_stands_alone_once():
    for entry, ((a, b), _, _) in dc.ENTRIES.items():
        alone = [next(iter(r)) for r in (dc.scalar_reasons(c, entry) for c in dc.CASES.values()) if len(r) == 1]
        for reason in ['cv1-by-C'] + ['cv1-by-%s:%s' % (k, o) for k in ('ptr', 'stride') for o in (a, b)]:
            assert reason in alone, (entry, reason)
        claimed = {cl for c in dc.CASES.values() for cl in c.claims[entry] if cl.startswith('cv1-by-')}
        assert {'cv1-by-C', 'cv1-by-stride', 'cv1-by-ptr:' + a, 'cv1-by-ptr:' + b} <= claimed, entry
    # the cases named after an operand leave the entry points that do not read it on the 16-B path
    for name, entries in {'ptr-x': 'fwd wgrad', 'ptr-y': 'fwd', 'ptr-dz': 'dgrad wgrad', 'ptr-dx': 'dgrad',
                          'stride-x': 'fwd wgrad', 'stride-y': 'fwd', 'stride-dz': 'dgrad wgrad', 'stride-dx': 'dgrad'}.items():
        assert {e for e in dc.ENTRIES if 'cv1' in dc.derive(dc.CASES[name], e)[0]} == set(entries.split()), name


def test_vec_decision_term_by_term():
    assert dc.dw_vec_ok(8, 8, 12, 0, 4)
    for bad in ((6, 8, 12, 0, 0), (8, 9, 12, 0, 0), (8, 8, 14, 0, 0), (8, 8, 12, 1, 0), (8, 8, 12, 0, 3)):
        assert not dc.dw_vec_ok(*bad), bad


def test_form_cases():
    assert [('cv4' if 'cv4' in dc.CASES[n].claims['fwd'] else 'cv1') for n in dc.FORM_CASES] == ['cv4', 'cv1']
    assert all('gy>1' in dc.CASES[n].claims['fwd'] for n in dc.FORM_CASES)
    assert set(dc.FORMS) == {'plain', 'affine-relu', 'affine-slope0.1', 'scale-only', 'shift-only'}


# ------------------------------------------------------------------------------------------------ the mirror against the built library
def lib():
    import _hip
    return _hip.lib()


def test_workspace_query_is_the_mirror_and_covers_either_width():
    L = lib()
    rnd = random.Random(5)
    shapes = [(B, H, W, C, stride) for B, C, H, W, stride in (c.shape for c in dc.CASES.values())]          # the entry points' order: B, H, W, C, stride
    shapes += [(rnd.randint(1, 9), rnd.randint(1, 300), rnd.randint(1, 300), rnd.choice((1, 3, 4, 6, 36, 70, 130, 256, 288, 1024, 4100)), rnd.choice((1, 2)))
               for _ in range(3000)]
    shapes += [(64, 13, 13, 1024, 1), (64, 208, 208, 32, 1), (64, 208, 208, 64, 2), (1, 4096, 4096, 4, 1), (1, 3000, 3000, 1, 2)]
    for s in shapes:
        want = dc.wgrad_workspace_bytes(*s)
        assert L.y2_dwconv_wgrad_workspace_bytes(*s) == want, s
        for CV in (1, 4):
            if CV == 1 or s[3] % 4 == 0:
                assert want >= dc.wgrad_need_bytes(*s, CV=CV) > 0, (s, CV)


BAD_SHAPES = ((0, 5, 7, 8, 1), (2, 0, 7, 8, 1), (2, 5, 0, 8, 1), (2, 5, 7, 0, 1), (2, 5, 7, 8, 0), (2, 5, 7, 8, 3), (2, 5, 7, 8, -1), (2, 46341, 46341, 1, 1))


def test_refusals():
    """The mirror's refusals, the source text they mirror, and the one entry point that answers without touching memory (the workspace query).  The
    launching entry points are called with refused arguments in tests/test_gpu_dwconv.py, on real buffers."""
    good = (2, 5, 7, 8)
    assert dc.dw_shape_ok(*good, stride=1) == dc.Shape(70, 70, 5, 7) and dc.dw_shape_ok(*good, stride=2) == dc.Shape(70, 24, 3, 4)
    for bad in BAD_SHAPES:
        assert dc.dw_shape_ok(*bad) is None, bad
        assert lib().y2_dwconv_wgrad_workspace_bytes(*bad) == 0 == dc.wgrad_workspace_bytes(*bad)
    assert dc.dw_shape_ok(1, 46340, 46340, 1, 1) is not None           # 2147395600 < 2^31 - 1
    dw = open(os.path.join(CSRC, 'dwconv.hip')).read()
    assert 'if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (stride != 1 && stride != 2)) return false;' in dw and 'return *Pin < 0x7fffffffLL;' in dw
    assert 'if (!x || !w || !y || !dw_shape_ok(B, H, W, C, stride, &Pin, &P, &Ho, &Wo) || ldx < C || ldy < C) return Y2_EINVAL;' in dw
    assert 'if (!dz || !w || !dx || !dw_shape_ok(B, H, W, C, stride, &P, &Pout, &Ho, &Wo) || ldz < C || lddx < C) return Y2_EINVAL;' in dw
    assert 'if (!x || !dz || !dw || !workspace || !dw_shape_ok(B, H, W, C, stride, &Pin, &P, &Ho, &Wo) || ldx < C || ldz < C) return Y2_EINVAL;' in dw
    assert 'if (!y2_aligned16(workspace)) return Y2_EALIGN;' in dw
    assert 'if ((long long)g.gx * C * 9 * (long long)sizeof(float) > workspace_bytes) return Y2_EINVAL;' in dw
