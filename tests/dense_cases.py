"""Case tables of the pre-activation kernel tests (tests/test_gpu_dense.py runs them on the GPU, tests/test_dense_cases.py proves on the CPU that
every case reaches what it claims), and the Python mirror of the host code of csrc/dense.hip that shapes a launch:

    pe_grid                  the element-wise grid (the function of csrc/dwconv.hip: tests/dw_cases.py dw_grid)
    pe_shape_ok              the refusals, Ho / Wo, the pixel counts
    y2_preact_conv1x1_fwd    NT, gn, MT, the workgroup count, the `vec` decision over K, ldx and the bases of x, w, pre_scale, pre_shift
    y2_preact_fwd            the CV decision over C, ldx, ldo and the bases of x, out
    y2_preact_bwd            the CV decision over C, ldx, ldda, lddx and the bases of x, dA, dx; the deterministic-workspace need

Plain integer arithmetic in the host code's order.  Every case names the claims it is there for; a claim the mirror does not confirm fails the
CPU test.

Left out on purpose: a CAPPED grid of the min_pix = 8 kernels (preact_bwd_sums_kernel, preact_bwd_dx_kernel).  Their threads already take 8
steps at the shapes below (the cap only lengthens the same loop), and reaching it needs operands of 4 M (CV = 1) to 17 M (CV = 4) elements."""
import collections

from dw_cases import NUM_CU, STATS_REPL, Shape, dw_grid as pe_grid          # pe_grid of csrc/dense.hip is dw_grid of csrc/dwconv.hip, line by line

PE_THREADS = 256                # csrc/dense.hip PE_THREADS
PE_MAX_BLOCKS = NUM_CU * 8      # csrc/dense.hip PE_MAX_BLOCKS
PE_BWD_MIN_PIX = 8              # csrc/dense.hip y2_preact_bwd: pe_grid(P, C, CV, 8)
PG_BK = 32                      # csrc/dense.hip PG_BK: k per slab
PIX_LIMIT = 0x7fffffff
DET_MIN_BYTES = 1 << 20         # y2_set_deterministic refuses a smaller scratch (csrc/det.hip)

GemmPlan = collections.namedtuple('GemmPlan', 'MT NT gn gm workgroups')


def cdiv(a, b):
    return (a + b - 1) // b


def pe_shape_ok(B, H, W, C, pool):
    """None where the entry points answer Y2_EINVAL."""
    if B <= 0 or H <= 0 or W <= 0 or C <= 0 or pool not in (0, 1):
        return None
    if pool and ((H | W) & 1):
        return None
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    Pin, Pout = B * H * W, B * Ho * Wo
    return Shape(Pin, Pout, Ho, Wo) if Pin < PIX_LIMIT else None


def gemm_accepts(B, H, W, K, ldx, N, ldy, coff, pool):
    return pe_shape_ok(B, H, W, K, pool) is not None and N > 0 and ldx >= K and coff >= 0 and ldy >= coff + N


def gemm_plan(M, N):
    NT = 2 if N > 64 else 1
    gn = cdiv(N, 64 * NT)
    MT = 2 if cdiv(M, 128) * gn >= NUM_CU else 1
    gm = cdiv(M, 64 * MT)
    return GemmPlan(MT, NT, gn, gm, gm * gn)


def _aligned(off):
    """off: floats past a 16-byte boundary, None: a NULL pointer (vec_ptr_ok)."""
    return off is None or not (off & 3)


def gemm_vec(K, ldx, off):
    return not (K & 3) and not (ldx & 3) and not (off['x'] & 3) and not (off['w'] & 3) and _aligned(off['pre_scale']) and _aligned(off['pre_shift'])


def fwd_cv(C, ldx, ldo, offx, offo):
    return 4 if not (C & 3) and not (ldx & 3) and not (ldo & 3) and not (offx & 3) and not (offo & 3) else 1


def bwd_cv(C, ldx, ldda, lddx, offx, offda, offdx):
    return 4 if not (C & 3) and not (ldx & 3) and not (ldda & 3) and not (lddx & 3) and not (offx & 3) and not (offda & 3) and not (offdx & 3) else 1


def det_need_bytes(Pin, C, CV):
    """y2_preact_bwd in deterministic mode: one row of 2C fp32 partial sums per pixel block."""
    return pe_grid(Pin, C, CV, PE_BWD_MIN_PIX).gx * 2 * C * 4


# ------------------------------------------------------------------------------------------------ y2_preact_conv1x1_fwd
GEMM_OPERANDS = ('x', 'w', 'pre_scale', 'pre_shift')
# shape (B, H, W, K, N, pool); ldx = K + xpad; the output window [coff, coff + N) of rows of ldy floats; off: floats past a 16-B boundary per operand
GemmCase = collections.namedtuple('GemmCase', 'shape xpad ldy coff off claims')


def _gemm(shape, xpad, ldy, coff, off, claims):
    return GemmCase(shape, xpad, ldy, coff, dict(zip(GEMM_OPERANDS, off)), claims.split())


A4 = (0, 0, 0, 0)
GEMM_CASES = collections.OrderedDict((n, _gemm(*v)) for n, v in [
    # ---- 128-row tiles (M = 181 * 181 = 255 * 128 + 121): every <2, NT, VEC, POOL>, each with a ragged last row tile
    ('g21-vec', ((1, 181, 181, 8, 30, 0), 4, 34, 3, A4, 'mt2 nt1 vec nopool ragged-M ragged-N k-tail one-slab coff>0 ldy>coff+N')),
    ('g21-vec-pool', ((1, 362, 362, 8, 30, 1), 0, 30, 0, A4, 'mt2 nt1 vec pool ragged-M ragged-N k-tail one-slab')),
    ('g22-vec', ((1, 181, 181, 8, 128, 0), 0, 128, 0, A4, 'mt2 nt2 vec nopool ragged-M k-tail one-slab')),
    ('g22-vec-pool', ((1, 362, 362, 8, 128, 1), 4, 128, 0, A4, 'mt2 nt2 vec pool ragged-M k-tail one-slab')),
    ('g21-nonvec', ((1, 181, 181, 6, 30, 0), 2, 30, 0, A4, 'mt2 nt1 nonvec-by-K nopool ragged-M k-quad-tail one-slab')),
    ('g21-nonvec-pool', ((1, 362, 362, 6, 30, 1), 1, 35, 5, A4, 'mt2 nt1 nonvec-by-K pool ragged-M k-quad-tail one-slab coff>0')),
    ('g22-nonvec', ((1, 181, 181, 3, 65, 0), 0, 65, 0, A4, 'mt2 nt2 nonvec-by-K nopool ragged-M ragged-N k-quad-tail one-slab')),
    ('g22-nonvec-pool', ((1, 362, 362, 5, 65, 1), 0, 70, 2, A4, 'mt2 nt2 nonvec-by-K pool ragged-M ragged-N k-quad-tail one-slab coff>0 ldy>coff+N')),
    ('g22-gn2', ((1, 129, 127, 8, 129, 0), 0, 129, 0, A4, 'mt2 nt2 gn>1 vec nopool ragged-M ragged-N')),
    # ---- 64-row tiles (M = 126), K of one slab and of several
    ('g11-vec', ((2, 7, 9, 40, 30, 0), 4, 40, 6, A4, 'mt1 nt1 vec nopool ragged-M ragged-N k-tail many-slabs coff>0 ldy>coff+N')),
    ('g11-vec-pool', ((2, 14, 18, 64, 30, 1), 0, 30, 0, A4, 'mt1 nt1 vec pool ragged-M many-slabs')),
    ('g12-vec', ((2, 7, 9, 36, 128, 0), 0, 128, 0, A4, 'mt1 nt2 vec nopool ragged-M k-tail many-slabs')),
    ('g12-vec-pool', ((2, 14, 18, 8, 100, 1), 8, 101, 1, A4, 'mt1 nt2 vec pool ragged-M ragged-N k-tail one-slab coff>0')),
    ('g12-gn2', ((3, 9, 11, 40, 200, 0), 0, 200, 0, A4, 'mt1 nt2 gn>1 vec nopool ragged-M ragged-N many-slabs')),
    ('g11-nonvec', ((2, 7, 9, 33, 30, 0), 3, 30, 0, A4, 'mt1 nt1 nonvec-by-K nopool ragged-M k-quad-tail many-slabs')),          # the second slab holds one k
    ('g11-nonvec-pool', ((2, 14, 18, 3, 30, 1), 2, 33, 2, A4, 'mt1 nt1 nonvec-by-K pool ragged-M k-quad-tail one-slab')),
    ('g12-nonvec', ((2, 7, 9, 61, 100, 0), 0, 100, 0, A4, 'mt1 nt2 nonvec-by-K nopool ragged-M k-quad-tail many-slabs')),
    ('g12-nonvec-pool', ((2, 14, 18, 30, 128, 1), 0, 128, 0, A4, 'mt1 nt2 nonvec-by-K pool ragged-M k-quad-tail one-slab')),
    ('g11-k1', ((2, 7, 9, 1, 30, 0), 0, 30, 0, A4, 'mt1 nt1 nonvec-by-K k-quad-tail one-slab')),
    # ---- the element-wise loader for exactly one reason (K = 40 and ldx = 44 could go 16-B)
    ('g-ptr-x', ((2, 7, 9, 40, 30, 0), 4, 30, 0, (1, 0, 0, 0), 'nonvec-by-ptr:x many-slabs k-tail')),
    ('g-ptr-w', ((2, 14, 18, 40, 100, 1), 4, 100, 0, (0, 2, 0, 0), 'nonvec-by-ptr:w pool')),
    ('g-ptr-pre_scale', ((2, 7, 9, 40, 30, 0), 4, 30, 0, (0, 0, 3, 0), 'nonvec-by-ptr:pre_scale')),
    ('g-ptr-pre_shift', ((2, 7, 9, 40, 30, 0), 4, 30, 0, (0, 0, 0, 1), 'nonvec-by-ptr:pre_shift')),
    ('g-stride', ((2, 14, 18, 40, 30, 1), 1, 30, 0, A4, 'nonvec-by-stride pool')),
])
GEMM_FORM_CASES = ('g11-vec', 'g11-nonvec')
GEMM_FORMS = ('plain', 'affine-relu', 'affine-slope0.1', 'scale-only', 'shift-only', 'null-pre')


def gemm_nonvec_reasons(c):
    B, H, W, K, N, pool = c.shape
    out = set()
    if K & 3:
        out.add('nonvec-by-K')
    if (K + c.xpad) & 3:
        out.add('nonvec-by-stride')
    return out | {'nonvec-by-ptr:' + o for o in GEMM_OPERANDS if not _aligned(c.off[o])}


def gemm_derive(c):
    B, H, W, K, N, pool = c.shape
    s = pe_shape_ok(B, H, W, K, pool)
    p = gemm_plan(s.Pout, N)
    out = {'mt%d' % p.MT, 'nt%d' % p.NT, 'pool' if pool else 'nopool', 'one-slab' if K <= PG_BK else 'many-slabs'}
    vec = gemm_vec(K, K + c.xpad, c.off)
    out |= {'vec'} if vec else gemm_nonvec_reasons(c)
    assert vec == (not gemm_nonvec_reasons(c))
    for claim, true in (('ragged-M', s.Pout % (64 * p.MT)), ('ragged-N', N % (64 * p.NT)), ('k-tail', K % PG_BK), ('k-quad-tail', K % 4), ('coff>0', c.coff > 0),
                        ('ldy>coff+N', c.ldy > c.coff + N), ('gn>1', p.gn > 1)):
        if true:
            out.add(claim)
    return out, p


# ------------------------------------------------------------------------------------------------ y2_preact_fwd, y2_preact_bwd
# shape (B, C, H, W, pool); pad: ld - C per operand; off: floats past a 16-B boundary per operand
FWD_OPERANDS = ('x', 'out')
BWD_OPERANDS = ('x', 'dA', 'dx')
PeCase = collections.namedtuple('PeCase', 'shape pad off claims')


def _pe(operands):
    return lambda shape, pad, off, claims: PeCase(shape, dict(zip(operands, pad)), dict(zip(operands, off)), claims.split())


A2, A3 = (0, 0), (0, 0, 0)
FWD_CASES = collections.OrderedDict((n, _pe(FWD_OPERANDS)(*v)) for n, v in [
    # ---- the grid cap: two pixels per thread, two channel blocks, the second with idle lanes (Cg = 65)
    ('f4-capped', ((1, 260, 65, 65, 0), (4, 0), A2, 'cv4 gy>1 ragged-channel-block capped walk>=2 nopool TC64')),
    ('f4-capped-pool', ((1, 260, 130, 130, 1), (0, 4), A2, 'cv4 gy>1 ragged-channel-block capped walk>=2 pool')),
    ('f1-capped', ((1, 65, 65, 65, 0), (1, 0), A2, 'cv1 gy>1 ragged-channel-block capped walk>=2 nopool')),
    ('f1-capped-pool', ((1, 65, 130, 130, 1), (0, 2), A2, 'cv1 gy>1 ragged-channel-block capped walk>=2 pool')),
    # ---- one pixel per thread
    ('f4-gy2', ((2, 288, 6, 10, 0), (0, 4), A2, 'cv4 gy>1 ragged-channel-block walk1 nopool')),
    ('f4-gy2-pool', ((2, 288, 6, 10, 1), (8, 0), A2, 'cv4 gy>1 ragged-channel-block walk1 pool')),
    ('f1-gy3', ((2, 130, 6, 10, 0), (0, 3), A2, 'cv1 cv1-by-C gy>1 ragged-channel-block walk1 nopool')),
    ('f1-gy3-pool', ((2, 130, 6, 10, 1), (1, 0), A2, 'cv1 cv1-by-C gy>1 ragged-channel-block walk1 pool')),
    ('f4-gy1', ((2, 36, 6, 10, 0), (4, 0), A2, 'cv4 gy1 walk1 nopool TC16')),
    ('f4-gy1-pool', ((2, 36, 6, 10, 1), (0, 4), A2, 'cv4 gy1 walk1 pool')),
    ('f1-gy1', ((2, 6, 6, 10, 0), (2, 6), A2, 'cv1 cv1-by-C gy1 walk1 nopool TC8')),
    ('f1-gy1-pool', ((2, 6, 6, 10, 1), (6, 2), A2, 'cv1 cv1-by-C gy1 walk1 pool')),
    # ---- the scalar path for exactly one reason
    ('f-ptr-x', ((2, 40, 6, 10, 1), (0, 4), (1, 0), 'cv1 cv1-by-ptr:x pool')),
    ('f-ptr-out', ((2, 40, 6, 10, 0), (0, 4), (0, 2), 'cv1 cv1-by-ptr:out nopool')),
    ('f-stride-x', ((2, 40, 6, 10, 0), (3, 4), A2, 'cv1 cv1-by-stride cv1-by-stride:x')),
    ('f-stride-out', ((2, 40, 6, 10, 1), (0, 1), A2, 'cv1 cv1-by-stride cv1-by-stride:out pool')),
])
FWD_FORM_CASES = ('f4-gy2-pool', 'f1-gy3')
FWD_FORMS = ('affine-relu', 'affine-slope0.1', 'null-pre-relu', 'scale-only', 'shift-only', 'identity')

BWD_CASES = collections.OrderedDict((n, _pe(BWD_OPERANDS)(*v)) for n, v in [
    ('b4-gy2', ((2, 288, 6, 10, 0), (0, 4, 8), A3, 'cv4 gy>1 ragged-channel-block walk>=2 nopool')),
    ('b4-gy2-pool', ((2, 288, 6, 10, 1), (8, 0, 4), A3, 'cv4 gy>1 ragged-channel-block walk>=2 pool')),
    ('b1-gy3', ((2, 130, 6, 10, 0), (0, 3, 1), A3, 'cv1 cv1-by-C gy>1 ragged-channel-block walk>=2 nopool')),
    ('b1-gy3-pool', ((2, 130, 6, 10, 1), (1, 0, 2), A3, 'cv1 cv1-by-C gy>1 ragged-channel-block walk>=2 pool')),
    ('b4-gy1', ((2, 36, 8, 6, 0), (4, 0, 8), A3, 'cv4 gy1 nopool TC16')),
    ('b4-gy1-pool', ((3, 36, 8, 6, 1), (0, 8, 4), A3, 'cv4 gy1 pool')),
    ('b1-gy1', ((2, 6, 8, 6, 0), (2, 6, 10), A3, 'cv1 cv1-by-C gy1 nopool TC8')),
    ('b1-gy1-pool', ((2, 6, 8, 6, 1), (6, 10, 2), A3, 'cv1 cv1-by-C gy1 pool')),
    ('b-ptr-x', ((2, 40, 6, 10, 0), (0, 4, 8), (3, 0, 0), 'cv1 cv1-by-ptr:x')),
    ('b-ptr-dA', ((2, 40, 6, 10, 1), (0, 4, 8), (0, 1, 0), 'cv1 cv1-by-ptr:dA pool')),
    ('b-ptr-dx', ((2, 40, 6, 10, 0), (0, 4, 8), (0, 0, 2), 'cv1 cv1-by-ptr:dx')),
    ('b-stride-x', ((2, 40, 6, 10, 1), (1, 4, 8), A3, 'cv1 cv1-by-stride cv1-by-stride:x pool')),
    ('b-stride-dA', ((2, 40, 6, 10, 0), (0, 3, 8), A3, 'cv1 cv1-by-stride cv1-by-stride:dA')),
    ('b-stride-dx', ((2, 40, 6, 10, 1), (0, 4, 9), A3, 'cv1 cv1-by-stride cv1-by-stride:dx pool')),
])
HAS_BN = (1, 2, 0)              # batch statistics, frozen, none (y2_bn_act_bwd's convention)
ACCUMULATE = (0, 1)
DET_CASES = ('b4-gy2', 'b4-gy2-pool', 'b1-gy3', 'b1-gy3-pool')          # deterministic mode: CV x POOL
# the smallest kind of problem whose partial sums outgrow the 1 MiB minimum scratch: CV = 1 never does (its need is at most 1 MiB exactly)
DET_TOO_SMALL = (1, 1024, 65, 65, 0)
MAX_ELEMENTS = 4500000          # the largest operand of the tables (the pooled capped forward's input), in floats


def ld(c, operand):
    return c.shape[1] + c.pad[operand]


def pe_derive(c, entry):
    """entry 'fwd' (walks the output pixels, min_pix 1) or 'bwd' (the input pixels, min_pix 8)."""
    B, C, H, W, pool = c.shape
    s = pe_shape_ok(B, H, W, C, pool)
    ops = FWD_OPERANDS if entry == 'fwd' else BWD_OPERANDS
    CV = (fwd_cv if entry == 'fwd' else bwd_cv)(C, *([ld(c, o) for o in ops] + [c.off[o] for o in ops]))
    g = pe_grid(s.Pout, C, CV, 1) if entry == 'fwd' else pe_grid(s.Pin, C, CV, PE_BWD_MIN_PIX)
    out = {'cv%d' % CV, 'TC%d' % g.TC, 'pool' if pool else 'nopool', 'gy1' if g.gy == 1 else 'gy>1', 'walk1' if g.steps == 1 else 'walk>=2'}
    if CV == 1:
        out |= pe_scalar_reasons(c, entry) | ({'cv1-by-stride'} if any(ld(c, o) & 3 for o in ops) else set())
    if g.capped:
        out.add('capped')
    if g.gy > 1 and g.ragged:
        out.add('ragged-channel-block')
    return out, g


def pe_scalar_reasons(c, entry):
    ops = FWD_OPERANDS if entry == 'fwd' else BWD_OPERANDS
    out = {'cv1-by-C'} if c.shape[1] & 3 else set()
    return out | {'cv1-by-stride:' + o for o in ops if ld(c, o) & 3} | {'cv1-by-ptr:' + o for o in ops if c.off[o] & 3}
