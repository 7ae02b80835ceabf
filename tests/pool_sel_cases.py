"""Case tables of the z_sel streaming tests (tests/test_gpu_pool_sel.py runs them on the GPU, tests/test_pool_sel_cases.py proves on the CPU that they reach
what they claim), and the Python mirror of the host code of csrc/train.hip behind the two entries:

    y2_bn_act_fwd_sel -> bn_act_fwd_impl    the refusals in order; the `vec` condition term by term; act_grid; how often a thread loops
    y2_bn_act_bwd_sel -> bn_act_bwd_impl    the same, and which of the three pass-1 reductions a call gets: fp64 atomics, per-workgroup partial rows parked in
                                            dz and added by bn_bwd_block_reduce_kernel (gridDim.y 1, 4 or 16), or - deterministic mode - per-thread rows
                                            added by det_reduce_rows_kernel

No torch and no library: integer arithmetic in the host code's order.  tests/test_pool_sel_cases.py pins the constants and conditions to the source text; the
GPU tests observe the reduction form by kernel name.  Every case names what it is there for; a claim the mirror does not confirm fails the CPU test."""
import collections
import math

NUM_CU = 256                    # Y2_NUM_CU (csrc/common.h)
OK, EINVAL, EALIGN, ENOSUP = 0, -1, -2, -3      # include/yolo2_hip.h
MAX_C = 8192
MAX_PIX = 0x7fffffff
DET_SMALL_BYTES = 1 << 20       # the smallest scratch y2_set_deterministic accepts: the scratch of a det_small call

# One call of either entry.  Rows: z has ldz = C + zpad floats; the pooled map (y_pool forward, dy_pool backward) ldp = poff + C + ppad and starts at channel
# poff; z_sel ldzs = C + spad; dz ldd = C + dpad.  zmis / pmis / smis / dmis: floats by which the base pointer is off its 16-byte boundary.
# dz (backward): 'dense' | 'null' | 'strided' (dpad > 0) | 'alias' (dz starts where z_sel starts).  det: deterministic mode; det_small: with the smallest scratch.
# null: the pointer arguments given as NULL.  affine: scale and shift given (forward).
_K = collections.namedtuple('K', 'B H W C zpad ppad poff spad dpad zmis pmis smis dmis dz det det_small null affine')


def K(B=2, H=6, W=10, C=8, zpad=0, ppad=0, poff=0, spad=0, dpad=0, zmis=0, pmis=0, smis=0, dmis=0, dz='dense', det=False, det_small=False, null=(), affine=True):
    return _K(B, H, W, C, zpad, ppad, poff, spad, dpad, zmis, pmis, smis, dmis, dz, det, det_small, tuple(null), affine)


def act_grid(total, Cg):
    """csrc/train.hip: workgroups of 256 threads, 8 items per thread, at most 8 per CU, a thread count that is a multiple of Cg."""
    unit = Cg // math.gcd(256, Cg)
    want = min(max((total + 256 * 8 - 1) // (256 * 8), 1), NUM_CU * 8)
    return (want + unit - 1) // unit * unit


def strides(c):
    return dict(ldz=c.C + c.zpad, ldp=c.poff + c.C + c.ppad, ldzs=c.C + c.spad, ldd=c.C + c.dpad)


def fwd_vec_terms(c):
    """The terms of bn_act_fwd_impl's `vec` a y2_bn_act_fwd_sel call can fail, by name, in the source's order."""
    s = strides(c)
    return [n for n, bad in (('C%4', c.C & 3), ('ldz%4', s['ldz'] & 3), ('ldp%4', s['ldp'] & 3), ('poff%4', c.poff & 3), ('pooled-base', c.pmis), ('z-base', c.zmis),
                             ('ldzs%4', s['ldzs'] & 3), ('z_sel-base', c.smis)) if bad]


def bwd_vec_terms(c):
    s = strides(c)
    has_dz = c.dz != 'null'
    return [n for n, bad in (('C%4', c.C & 3), ('ldz%4', s['ldz'] & 3), ('ldd%4', has_dz and s['ldd'] & 3), ('dz-base', has_dz and (c.smis if c.dz == 'alias' else c.dmis)), ('z-base', c.zmis),
                             ('ldp%4', s['ldp'] & 3), ('poff%4', c.poff & 3), ('pooled-base', c.pmis), ('ldzs%4', s['ldzs'] & 3), ('z_sel-base', c.smis)) if bad]


Route = collections.namedtuple('Route', 'rc vec Cg grid loops form slices prow', defaults=(None, 0, 0))


def _refuse(rc):
    return Route(rc, False, 0, 0, 0)


def _geometry(c, terms):
    vec = not terms
    Cg = c.C // 4 if vec else c.C
    pix = c.B * (c.H // 2) * (c.W // 2)
    grid = act_grid(pix * Cg, Cg)
    assert (grid * 256) % Cg == 0
    pstep = grid * 256 // Cg
    return vec, Cg, pix, grid, (pix + pstep - 1) // pstep


def fwd_route(c):
    """y2_bn_act_fwd_sel, then bn_act_fwd_impl."""
    if 'y_pool' in c.null or 'z_sel' in c.null:
        return _refuse(EINVAL)
    if 'z' in c.null or c.B <= 0 or c.H <= 0 or c.W <= 0 or c.C <= 0:
        return _refuse(EINVAL)
    if c.spad < 0:
        return _refuse(EINVAL)
    if c.H & 1 or c.W & 1:
        return _refuse(EINVAL)
    if c.B * (c.H // 2) * (c.W // 2) >= MAX_PIX or c.C > MAX_C:
        return _refuse(ENOSUP)
    vec, Cg, pix, grid, loops = _geometry(c, fwd_vec_terms(c))
    return Route(OK, vec, Cg, grid, loops)


def bwd_route(c):
    """y2_bn_act_bwd_sel, then bn_act_bwd_impl (has_bn = 1, a pooled gradient only, no park buffer)."""
    if 'z_sel' in c.null:
        return _refuse(EINVAL)
    if 'z' in c.null or 'dy_pool' in c.null or 'sums' in c.null or c.B <= 0 or c.H <= 0 or c.W <= 0 or c.C <= 0:
        return _refuse(EINVAL)
    if c.spad < 0:
        return _refuse(EINVAL)
    if 'mean' in c.null or 'invstd' in c.null or 'gamma' in c.null:
        return _refuse(EINVAL)
    if c.H & 1 or c.W & 1:
        return _refuse(EINVAL)
    if c.C > MAX_C:
        return _refuse(ENOSUP)
    if c.B * (c.H // 2) * (c.W // 2) >= MAX_PIX:
        return _refuse(ENOSUP)
    vec, Cg, pix, grid, loops = _geometry(c, bwd_vec_terms(c))
    ldd = c.C + c.dpad
    npix = c.B * c.H * c.W
    prow = grid * 256 // Cg
    if c.det or c.det_small:
        if c.det_small and prow * 2 * c.C * 4 > DET_SMALL_BYTES:
            return _refuse(EINVAL)
        return Route(OK, vec, Cg, grid, loops, 'det', 0, prow)
    if c.dz in ('dense', 'strided') and ldd == c.C and grid > 16 and grid * 2 * c.C <= npix * ldd:
        return Route(OK, vec, Cg, grid, loops, 'parked', 16 if grid >= 512 else (4 if grid >= 64 else 1), prow)
    return Route(OK, vec, Cg, grid, loops, 'atomics', 0, prow)


def claims_of(c, backward):
    r = (bwd_route if backward else fwd_route)(c)
    if r.rc != OK:
        return {'refused'}
    terms = (bwd_vec_terms if backward else fwd_vec_terms)(c)
    out = {'vec' if r.vec else 'scalar'} | {'scalar:' + t for t in terms}
    if len(terms) == 1:
        out.add('single-cause')
    if r.loops > 1:
        out.add('loops')
    if r.grid > 1:
        out.add('multi-block')
    if r.grid > 16:
        out.add('grid>16')
    if 256 % r.Cg:
        out.add('cg-not-dividing-256')
    s = strides(c)
    for n, over in (('ldz>C', c.zpad > 0), ('ldp>C', c.ppad > 0 or c.poff > 0), ('poff>0', c.poff > 0), ('ldzs>C', c.spad > 0)):
        if over:
            out.add(n)
    if not c.affine:
        out.add('affine-null')
    if backward:
        out.add(r.form if r.form != 'parked' else 'parked%d' % r.slices)
        out.add('dz-' + c.dz)
        if c.dz != 'null' and s['ldd'] != c.C:
            out.add('ldd!=C')
    return out


def smallest_parked(B, C, vec, slices):
    """The smallest even square size H = W at which a dense-dz call of batch B parks its partial sums and the block-reduce kernel gets `slices` row slices."""
    for H in range(2, 4096, 2):
        r = bwd_route(K(B, H, H, C))
        assert r.vec == vec
        if r.form == 'parked' and r.slices == slices:
            return H
    raise AssertionError


Case = collections.namedtuple('Case', 'c claims')
WIN = dict(zpad=4, ppad=4, poff=4, spad=4)          # every map a channel window of wider rows, all of it 16-byte aligned
LOOP = dict(B=3, H=16, W=24)                        # 288 windows: two workgroups (vector, C = 32) whose threads walk 5 windows each

# ---- forward: y2_bn_act_fwd_sel
FWD_CASES = collections.OrderedDict([
    ('vec-dense', Case(K(), {'vec'})),
    ('vec-windows', Case(K(**WIN), {'vec', 'ldz>C', 'ldp>C', 'poff>0', 'ldzs>C'})),
    ('vec-loops', Case(K(C=32, **LOOP), {'vec', 'loops', 'multi-block'})),
    ('vec-cg10', Case(K(C=40, **LOOP), {'vec', 'cg-not-dividing-256', 'multi-block', 'loops'})),
    ('vec-affine-null', Case(K(affine=False, **WIN), {'vec', 'affine-null'})),
    ('scalar-C%4', Case(K(C=6, zpad=2, ppad=2, spad=2), {'scalar:C%4', 'single-cause'})),
    ('scalar-ldz%4', Case(K(zpad=2), {'scalar:ldz%4', 'single-cause', 'ldz>C'})),
    ('scalar-ldp%4', Case(K(ppad=2), {'scalar:ldp%4', 'single-cause', 'ldp>C'})),
    ('scalar-poff%4', Case(K(poff=2, ppad=2), {'scalar:poff%4', 'single-cause', 'poff>0'})),
    ('scalar-ldzs%4', Case(K(spad=2), {'scalar:ldzs%4', 'single-cause', 'ldzs>C'})),
    ('scalar-z-base', Case(K(zmis=1), {'scalar:z-base', 'single-cause'})),
    ('scalar-pooled-base', Case(K(pmis=1), {'scalar:pooled-base', 'single-cause'})),
    ('scalar-z_sel-base', Case(K(smis=1), {'scalar:z_sel-base', 'single-cause'})),
    ('scalar-windows-loops', Case(K(C=6, zpad=1, ppad=1, poff=3, spad=5, **LOOP), {'scalar', 'loops', 'ldz>C', 'ldp>C', 'poff>0', 'ldzs>C', 'cg-not-dividing-256'})),
    ('scalar-affine-null', Case(K(C=6, affine=False), {'scalar', 'affine-null'})),
])
FWD_REFUSALS = collections.OrderedDict([
    ('y_pool-null', (K(null=('y_pool',)), EINVAL)), ('z_sel-null', (K(null=('z_sel',)), EINVAL)),
    ('z-null', (K(null=('z',)), EINVAL)), ('batch-0', (K(B=0), EINVAL)), ('height-0', (K(H=0), EINVAL)), ('width-0', (K(W=0), EINVAL)), ('channels-0', (K(C=0), EINVAL)),
    ('ldzs<C', (K(spad=-1), EINVAL)),
    ('odd-height', (K(H=7), EINVAL)), ('odd-width', (K(W=9), EINVAL)),
    ('windows>=2^31', (K(B=MAX_PIX, H=2, W=2), ENOSUP)), ('channels>8192', (K(C=MAX_C + 4), ENOSUP)),
])
# which `return` (by its first words in the source, from the entry on) each refusal is there for
FWD_REFUSAL_RETURNS = collections.OrderedDict([
    ('!y_pool || !z_sel', ('y_pool-null', 'z_sel-null')),
    ('!z || (!y && !y_pool) || B <= 0', ('z-null', 'batch-0', 'height-0', 'width-0', 'channels-0')),
    ('z_sel != nullptr && (!pool || residual != nullptr || ldzs < C)', ('ldzs<C',)),
    ('(pool || out_mode == 1) && ((H & 1) || (W & 1))', ('odd-height', 'odd-width')),
    ('pix >= 0x7fffffffLL || C > 8192', ('windows>=2^31', 'channels>8192')),
])

# ---- backward: y2_bn_act_bwd_sel
PARK = (2, 36, 36, 256)          # the smallest vector call that parks: 648 windows x 64 channel groups = 21 workgroups
BWD_CASES = collections.OrderedDict([
    ('vec-dense', Case(K(), {'vec', 'atomics', 'dz-dense'})),
    ('vec-windows', Case(K(**WIN), {'vec', 'ldz>C', 'ldp>C', 'poff>0', 'ldzs>C', 'atomics'})),
    ('vec-sums-only', Case(K(dz='null', **WIN), {'vec', 'dz-null', 'atomics'})),
    ('vec-loops', Case(K(C=32, **LOOP), {'vec', 'loops', 'multi-block', 'atomics'})),
    ('vec-cg10', Case(K(C=40, **LOOP), {'vec', 'cg-not-dividing-256', 'multi-block', 'loops'})),
    ('scalar-C%4', Case(K(C=6, zpad=2, ppad=2, spad=2, dpad=2, dz='strided'), {'scalar:C%4', 'single-cause'})),
    ('scalar-ldz%4', Case(K(zpad=2), {'scalar:ldz%4', 'single-cause'})),
    ('scalar-ldp%4', Case(K(ppad=2), {'scalar:ldp%4', 'single-cause'})),
    ('scalar-poff%4', Case(K(poff=2, ppad=2), {'scalar:poff%4', 'single-cause'})),
    ('scalar-ldzs%4', Case(K(spad=2), {'scalar:ldzs%4', 'single-cause'})),
    ('scalar-ldd%4', Case(K(dpad=2, dz='strided'), {'scalar:ldd%4', 'single-cause', 'ldd!=C'})),
    ('scalar-z-base', Case(K(zmis=1), {'scalar:z-base', 'single-cause'})),
    ('scalar-pooled-base', Case(K(pmis=1), {'scalar:pooled-base', 'single-cause'})),
    ('scalar-z_sel-base', Case(K(smis=1), {'scalar:z_sel-base', 'single-cause'})),
    ('scalar-dz-base', Case(K(dmis=1), {'scalar:dz-base', 'single-cause'})),
    ('scalar-sums-only-windows-loops', Case(K(C=6, zpad=1, ppad=1, poff=3, spad=5, dz='null', **LOOP), {'scalar', 'loops', 'dz-null', 'cg-not-dividing-256', 'ldz>C', 'ldp>C', 'poff>0', 'ldzs>C'})),
    ('parked1', Case(K(*PARK), {'vec', 'parked1', 'grid>16', 'dz-dense', 'loops'})),
    ('atomics-sums-only', Case(K(*PARK, dz='null'), {'vec', 'atomics', 'grid>16', 'dz-null'})),
    ('atomics-strided-dz', Case(K(*PARK, dpad=4, dz='strided'), {'vec', 'atomics', 'grid>16', 'ldd!=C'})),
    ('atomics-dz-aliases-z_sel', Case(K(*PARK, dz='alias'), {'vec', 'atomics', 'grid>16', 'dz-alias'})),
    ('atomics-grid16', Case(K(2, 32, 32, 256), {'vec', 'atomics', 'dz-dense', 'multi-block'})),          # 512 windows: exactly 16 workgroups, one below the parking threshold
    ('det-vec', Case(K(*PARK, det=True), {'vec', 'det', 'grid>16', 'dz-dense'})),
    ('det-scalar-sums-only', Case(K(C=6, zpad=1, ppad=1, poff=3, spad=5, dz='null', det=True, **LOOP), {'scalar', 'det', 'dz-null', 'loops'})),
])
BWD_CASES['parked4'] = Case(K(2, smallest_parked(2, 256, True, 4), smallest_parked(2, 256, True, 4), 256), {'vec', 'parked4', 'dz-dense'})
# the 16-slice bucket on the scalar path (C = 30): the same 512 workgroups hold a quarter of the vector path's data
BWD_CASES['parked16-scalar'] = Case(K(4, smallest_parked(4, 30, False, 16), smallest_parked(4, 30, False, 16), 30), {'scalar', 'scalar:C%4', 'parked16', 'dz-dense'})
BWD_REFUSALS = collections.OrderedDict([
    ('z_sel-null', (K(null=('z_sel',)), EINVAL)),
    ('z-null', (K(null=('z',)), EINVAL)), ('dy_pool-null', (K(null=('dy_pool',)), EINVAL)), ('sums-null', (K(null=('sums',)), EINVAL)),
    ('batch-0', (K(B=0), EINVAL)), ('height-0', (K(H=0), EINVAL)), ('width-0', (K(W=0), EINVAL)), ('channels-0', (K(C=0), EINVAL)),
    ('ldzs<C', (K(spad=-1), EINVAL)),
    ('mean-null', (K(null=('mean',)), EINVAL)), ('invstd-null', (K(null=('invstd',)), EINVAL)), ('gamma-null', (K(null=('gamma',)), EINVAL)),
    ('odd-height', (K(H=7), EINVAL)), ('odd-width', (K(W=9), EINVAL)),
    ('channels>8192', (K(C=MAX_C + 4), ENOSUP)),
    ('windows>=2^31', (K(B=MAX_PIX, H=2, W=2), ENOSUP)),
])
BWD_REFUSALS['deterministic-scratch-too-small'] = (BWD_CASES['parked16-scalar'].c._replace(det_small=True), EINVAL)          # 4,480 rows of 60 floats: 1,075,200 B
BWD_REFUSAL_RETURNS = collections.OrderedDict([
    ('!z_sel', ('z_sel-null',)),
    ('!z || (!dy_full && !dy_pool) || !sums || B <= 0', ('z-null', 'dy_pool-null', 'sums-null', 'batch-0', 'height-0', 'width-0', 'channels-0')),
    ('z_sel != nullptr && (!dy_pool || dy_full || dy_full2 || residual || has_bn != 1 || ldzs < C)', ('ldzs<C',)),
    ('has_bn < 0 || has_bn > 2 || (has_bn && (!mean || !invstd || !gamma))', ('mean-null', 'invstd-null', 'gamma-null')),
    ('(pool || fmode == 1) && ((H & 1) || (W & 1))', ('odd-height', 'odd-width')),
    ('C > 8192', ('channels>8192',)),
    ('pix >= 0x7fffffffLL', ('windows>=2^31',)),
    ('(size_t)prow * 2 * C * sizeof(float) > y2_det.bytes || prow > 0x7fffffffLL', ('deterministic-scratch-too-small',)),
])
