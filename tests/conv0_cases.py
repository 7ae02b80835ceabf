"""Case tables of the first-layer forward tests (tests/test_gpu_conv0.py runs them on the GPU, tests/test_conv0_cases.py proves on the CPU that they
reach what they claim), and the Python mirror of the host code of csrc/conv0_fwd.hip:

    y2_conv0_fwd        the refusals with their codes, in the entry point's order; tiles_y, tiles_x, ntiles
    y2_conv0_fwd_sel    its own refusal (gamma, z or z_sel NULL), then the shared body with no affine, slope 1 and pool_sign = gamma
    launch0             the persistent grid (Y2_NUM_CU * 8 workgroups or one per tile), how many tiles the busiest and the idlest workgroup walk, the
                        FULL condition, which of the eight straight-line (NBLK, OUT, RAW) variants a call gets or the general kernel with NBLK 1 / 2 -
                        a pooled-only call whose slope lies outside [0, 1] falls through to the general kernel; a call with pool_sign gets the ninth
                        straight-line variant (1, 7, RAW, launched outside the Y2_C0 list) when it asks for z, z_sel and statistics at Cout 32, and the
                        general kernel - the only other code that selects - in every other case

No torch and no library: plain integer arithmetic in the host code's order.

The mirror is NOT pinned to the built library: every variant launches under the one name conv0_kernel and the entry point has no size query, so
nothing the library exports tells which variant a call ran (fwd_cases is pinned through y2_conv_fwd_workspace_bytes; there is no such answer here).
tests/test_conv0_cases.py pins the mirror's constants and its variant list to the source text; that the GPU tests see the code they claim to reach is
shown by the mutation table in the README instead.

Every case names the path it is there for.  A case whose claim the mirror does not confirm fails the CPU test."""
import collections

NUM_CU = 256                    # Y2_NUM_CU (csrc/common.h)
WGS_PER_CU = 8                  # launch0's default; the library reads Y2_CONV0_WGS from the environment - every walk length here assumes it is unset (test_gpu_conv0.run asserts that)
TH, TW = 16, 32                 # output pixels of a tile
OK, EINVAL, EALIGN, ENOSUP = 0, -1, -2, -3      # include/yolo2_hip.h
MASKS = {1: 'y', 2: 'p', 3: 'yp', 4: 's', 5: 'ys', 6: 'ps', 7: 'yps'}
# (Cout / 32, out mask, RAW) of the straight-line instantiations launch0 has
VARIANTS = ((1, 2, False), (1, 5, True), (1, 5, False), (1, 1, False), (1, 3, False), (2, 2, False), (2, 5, True), (2, 1, False))

SEL_VARIANT = (1, 7, True)      # ... and the one launched outside the Y2_C0 list: y2_conv0_fwd_sel's z + z_sel + statistics

_C = collections.namedtuple('C', 'B cin cout H W outs scale shift slope ypad yoff ppad poff det nox now sel nog')


def C(B, cin, cout, H, W, outs='y', scale=True, shift=True, slope=0.1, ypad=0, yoff=0, ppad=0, poff=0, det=False, nox=False, now=False, sel=False, nog=False):
    """A y2_conv0_fwd call, or (sel or nog: see S) a y2_conv0_fwd_sel call.  outs: the destinations given, a subset of 'y' (full), 'p' (2x2-pooled), 's' (statistics).  y has rows of ldy = cout + ypad
    floats and is passed as y + yoff (ppad / poff: the same for y_pool; a negative pad is an ld below Cout).  det: deterministic mode is on.
    nox / now: x / w is NULL."""
    return _C(B, cin, cout, H, W, outs, scale, shift, slope, ypad, yoff, ppad, poff, det, nox, now, sel, nog)


def S(B, cin, cout, H, W, outs='yps', nog=False, **kw):
    """A y2_conv0_fwd_sel call: 'y' is z (rows of ldz = cout + ypad floats, passed as z + yoff), 'p' is z_sel (ldzs = cout + ppad, z_sel + poff), 's' the
    statistics.  sel: gamma is given (nog: the entry is called with gamma NULL).  The entry passes no affine and slope 1 on."""
    return C(B, cin, cout, H, W, outs, scale=False, shift=False, slope=1.0, sel=not nog, nog=nog, **kw)


def is_sel_entry(c):
    return c.sel or c.nog


def cdiv(a, b):
    return (a + b - 1) // b


def out_mask(outs):
    return ('y' in outs) * 1 + ('p' in outs) * 2 + ('s' in outs) * 4


Route = collections.namedtuple('Route', 'rc kernel nblk out raw full tiles_y tiles_x ntiles grid walk_max walk_min sel', defaults=(False,))


def _refuse(rc):
    return Route(rc, None, 0, 0, False, False, 0, 0, 0, 0, 0, 0)


def route(c):
    """What y2_conv0_fwd (y2_conv0_fwd_sel for a call made by S) and launch0 do with call c."""
    if is_sel_entry(c):
        assert not c.scale and not c.shift and c.slope == 1.0, 'y2_conv0_fwd_sel has no affine to pass'
        if c.nog or 'y' not in c.outs or 'p' not in c.outs:
            return _refuse(EINVAL)
    if c.nox or c.now or not c.outs:
        return _refuse(EINVAL)
    if c.B <= 0 or c.H <= 0 or c.W <= 0 or c.cin < 1 or c.cin > 4 or c.cout < 1 or c.cout > 64:
        return _refuse(ENOSUP)
    if 'y' in c.outs and c.cout + c.ypad < c.cout:
        return _refuse(EINVAL)
    if 'p' in c.outs and (c.cout + c.ppad < c.cout or c.H & 1 or c.W & 1):
        return _refuse(EINVAL)
    if 's' in c.outs and c.det:
        return _refuse(ENOSUP)
    ty, tx = cdiv(c.H, TH), cdiv(c.W, TW)
    tiles = c.B * ty * tx
    if tiles <= 0 or tiles > 0x7fffffff:
        return _refuse(EINVAL)
    cap = NUM_CU * WGS_PER_CU
    grid = cap if tiles > cap else tiles
    walk = (cdiv(tiles, grid), tiles // grid)
    out = out_mask(c.outs)
    full = (c.cin == 3 and c.H % TH == 0 and c.W % TW == 0 and c.cout in (32, 64) and ('y' not in c.outs or c.ypad == 0) and ('p' not in c.outs or c.ppad == 0))
    if full:
        raw = not c.scale and not c.shift and c.slope == 1.0
        mono = 0.0 <= c.slope <= 1.0
        nb = c.cout // 32
        if c.sel and (nb, out, raw) == SEL_VARIANT:
            return Route(OK, 'straight', nb, out, raw, True, ty, tx, tiles, grid, walk[0], walk[1], True)
        if c.sel:
            v = None                                # no instantiation of the Y2_C0 list selects: the general kernel
        elif out == 2 and mono:
            v = (nb, 2, False)
        elif out == 5 and raw:
            v = (nb, 5, True)
        elif nb == 1 and out in (5, 1, 3):
            v = (nb, out, False)
        elif nb == 2 and out == 1:
            v = (nb, 1, False)
        else:
            v = None
        if v is not None:
            return Route(OK, 'straight', v[0], v[1], v[2], True, ty, tx, tiles, grid, walk[0], walk[1])
    return Route(OK, 'general', 1 if c.cout <= 32 else 2, out, False, False, ty, tx, tiles, grid, walk[0], walk[1], c.sel)


def variant_name(r):
    return ('sl%d-o%d%s' % (r.nblk, r.out, '-raw' if r.raw else '') if r.kernel == 'straight' else 'gen%d' % r.nblk) + ('-sel' if r.sel else '')


def looks_aligned(c):
    """The part of launch0's condition a reader sees first: the shipped first layer on whole tiles."""
    return c.cin == 3 and c.H % TH == 0 and c.W % TW == 0 and c.cout in (32, 64)


def claims_of(c):
    """Everything the mirror says about the launch of c: the vocabulary of the case tables."""
    r = route(c)
    if r.rc != OK:
        return {'refused'}
    out = {variant_name(r), r.kernel, 'cin%d' % c.cin, 'nblk%d' % r.nblk, 'out%d' % out_mask(c.outs)}
    if r.sel:
        out.add('sel')
    out.add('walk%d' % r.walk_max if r.walk_max <= 4 else 'walk7+' if r.walk_max >= 7 else 'walk5-6')
    if r.walk_min == r.walk_max - 1:
        out.add('uneven-walk')
    if r.ntiles > 2 * r.grid:
        out.add('steady-state')                 # `more` is true somewhere: a tile is taken from the in-loop staging
    if r.ntiles > 3 * r.grid:
        out.add('buffer-reuse')                 # ... and the first LDS buffer is written a second time
    if r.ntiles > 7 * r.grid:
        out.add('buffers-rewritten-twice')
    rw, rh = c.W % TW != 0, c.H % TH != 0
    if rw and (r.tiles_y > 1 or not rh):
        out.add('ragged-right')
    if rh and (r.tiles_x > 1 or not rw):
        out.add('ragged-bottom')
    if rw and rh:
        out.add('ragged-both')
    if (r.tiles_x > 1 or not rw) and (r.tiles_y > 1 or not rh):
        out.add('whole-tile')
    out.add('one-tile-image' if r.tiles_x * r.tiles_y == 1 else 'multi-tile-image')
    if c.B > 1:
        out.add('batch')
    if looks_aligned(c) and r.kernel == 'general':
        out.add('fallthrough')
    if c.cout % 32:
        out.add('channel-mask')
    if ('y' in c.outs and c.ypad > 0) or ('p' in c.outs and c.ppad > 0):
        out.add('ld>cout')
    if ('y' in c.outs and (c.cout + c.ypad) % 4) or ('p' in c.outs and (c.cout + c.ppad) % 4):
        out.add('ld%4')
    if ('y' in c.outs and c.yoff) or ('p' in c.outs and c.poff):
        out.add('channel-offset')
    return out


# ================================================================================================ case tables
# name: (call, what it is there for).  The claims are in the vocabulary of claims_of.
Case = collections.namedtuple('Case', 'c claims')
WINDOW = dict(ypad=5, yoff=3, ppad=6, poff=1)          # the concat write-through form: ldy = Cout + 5 (for Cout 32: 37, no multiple of 4), y + 3, ldp = Cout + 6, y_pool + 1

# ---- tap tables: StepTap<CIN> is different code for each Cin (1: empty group 2 + padded group 3, 2 and 4: no group 3, 3: both), with NBLK 1 and 2
TAP_CASES = collections.OrderedDict()
for _cin in (1, 2, 3, 4):
    for _cout in (7, 40):
        TAP_CASES['tap-cin%d-cout%d' % (_cin, _cout)] = Case(C(2, _cin, _cout, 18, 34, 'yps'), {'cin%d' % _cin, 'gen%d' % (1 if _cout <= 32 else 2), 'ragged-both', 'ragged-right',
                                                                                              'ragged-bottom', 'whole-tile', 'channel-mask', 'out7'})

# ---- channel masks: n < Cout with NBLK 1 and 2, dense and as a window of wider rows
MASK_COUTS = (1, 31, 32, 33, 63, 64)
MASK_CASES = collections.OrderedDict()
for _cout in MASK_COUTS:
    _nb = 'gen%d' % (1 if _cout <= 32 else 2)
    MASK_CASES['mask-cout%d-dense' % _cout] = Case(C(2, 3, _cout, 18, 34, 'yps'), {_nb, 'ragged-both', 'out7'} | ({'channel-mask'} if _cout % 32 else set()))
    MASK_CASES['mask-cout%d-window' % _cout] = Case(C(2, 3, _cout, 18, 34, 'yps', **WINDOW), {_nb, 'ragged-both', 'out7', 'ld>cout', 'channel-offset'} | ({'channel-mask'} if _cout % 32 else set()))

# ---- geometry: (H, W, outs) with batch 1 and 3 (origin decodes a batch index with tiles_x and tiles_y of 1 and of more)
GEOMETRY = collections.OrderedDict([
    ('1x1', (1, 1, 'ys', {'one-tile-image', 'ragged-both'})),              # every tap but one is padding
    ('1x40', (1, 40, 'ys', {'multi-tile-image', 'ragged-both'})),
    ('17x1', (17, 1, 'ys', {'multi-tile-image', 'ragged-both'})),
    ('2x2', (2, 2, 'yps', {'one-tile-image', 'ragged-both'})),
    ('16x32', (16, 32, 'yps', {'one-tile-image', 'whole-tile'})),
    ('16x33', (16, 33, 'ys', {'multi-tile-image', 'ragged-right', 'whole-tile'})),      # a tile holding one column
    ('17x32', (17, 32, 'ys', {'multi-tile-image', 'ragged-bottom', 'whole-tile'})),
    ('20x36', (20, 36, 'yps', {'multi-tile-image', 'ragged-both', 'ragged-right', 'ragged-bottom', 'whole-tile'})),
    ('15x31', (15, 31, 'y', {'one-tile-image', 'ragged-both', 'out1'})),    # odd, y only
])
GEOMETRY_COUT = 20
GEOMETRY_CASES = collections.OrderedDict()
for _n, (_H, _W, _outs, _cl) in GEOMETRY.items():
    for _B in (1, 3):
        GEOMETRY_CASES['geo-%s-b%d' % (_n, _B)] = Case(C(_B, 3, GEOMETRY_COUT, _H, _W, _outs), _cl | {'gen1', 'walk1'} | ({'batch'} if _B > 1 else set()))

# ---- output sets of the general kernel: every mask x (scale given, shift given, slope), NBLK 1 and 2
OUTS = ('y', 'p', 'yp', 's', 'ys', 'ps', 'yps')
AFFINE = ((True, True, 0.1), (False, False, 0.1), (False, True, 0.1), (True, False, 0.1), (False, False, 1.0), (True, True, 0.0))
OUTSET_SHAPES = collections.OrderedDict([('gen1', (2, 3, 24, 18, 34)), ('gen2', (2, 3, 40, 18, 34))])
OUTSET_CASES = collections.OrderedDict()
for _n, _s in OUTSET_SHAPES.items():
    for _outs in OUTS:
        for _sc, _sh, _slope in AFFINE:
            OUTSET_CASES['%s-%s-%d%d-%g' % (_n, _outs, _sc, _sh, _slope)] = Case(C(*_s, outs=_outs, scale=_sc, shift=_sh, slope=_slope), {_n, 'out%d' % out_mask(_outs)})

# ---- the straight-line variants: (Cout, outs, affine given, slope) of each
STRAIGHT = collections.OrderedDict([
    ('sl1-o2', (32, 'p', True, 0.1)), ('sl1-o5-raw', (32, 'ys', False, 1.0)), ('sl1-o5', (32, 'ys', True, 0.1)), ('sl1-o1', (32, 'y', True, 0.1)), ('sl1-o3', (32, 'yp', True, 0.1)),
    ('sl2-o2', (64, 'p', True, 0.1)), ('sl2-o5-raw', (64, 'ys', False, 1.0)), ('sl2-o1', (64, 'y', True, 0.1)),
])
# aligned sizes (B, H, W): one tile per workgroup, and walks of the production grid whose busiest workgroup takes exactly 2, 3, 4 tiles while others take one fewer
ALIGNED_SIZES = collections.OrderedDict([
    ('small', ((2, 32, 64), {'walk1', 'whole-tile', 'multi-tile-image'})),
    ('walk2', ((9, 256, 512), {'walk2', 'uneven-walk'})),                                   # 2,304 tiles
    ('walk3', ((273, 64, 128), {'walk3', 'uneven-walk', 'steady-state'})),                  # 4,368 tiles: the first tiles taken from the in-loop staging
    ('walk4', ((25, 256, 512), {'walk4', 'uneven-walk', 'steady-state', 'buffer-reuse'})),  # 6,400 tiles: the first buffer is reused
])
# every variant runs at 'small' and at 'walk4'; the forms the shipped plans launch (pooled-only: inference, raw + statistics: training) at every walk
STRAIGHT_AT = {'small': tuple(STRAIGHT), 'walk2': ('sl1-o2', 'sl1-o5-raw'), 'walk3': ('sl1-o2', 'sl1-o5-raw', 'sl2-o2'), 'walk4': tuple(STRAIGHT)}


def straight_call(variant, size, **kw):
    cout, outs, affine, slope = STRAIGHT[variant]
    B, H, W = ALIGNED_SIZES[size][0]
    return C(B, 3, cout, H, W, outs, scale=affine, shift=affine, slope=slope, **kw)


STRAIGHT_CASES = collections.OrderedDict(('%s-%s' % (v, s), Case(straight_call(v, s), ALIGNED_SIZES[s][1] | {v, 'straight'}))
                                         for s in ALIGNED_SIZES for v in STRAIGHT_AT[s])
# the deepest walk: pooled-only (what detect runs), so no case holds a full-resolution fp64 map in host memory
STRAIGHT_CASES['sl1-o2-walk7'] = Case(C(57, 3, 32, 256, 512, 'p'), {'sl1-o2', 'walk7+', 'uneven-walk', 'buffers-rewritten-twice'})          # 14,592 tiles

# ---- combinations that look aligned but must fall to the general kernel (B, H, W of 'small')
FALL_CASES = collections.OrderedDict([
    ('fall-cout64-o3', Case(C(2, 3, 64, 32, 64, 'yp'), {'fallthrough', 'gen2', 'out3'})),
    ('fall-cout64-o5-affine', Case(C(2, 3, 64, 32, 64, 'ys'), {'fallthrough', 'gen2', 'out5'})),
    ('fall-cout32-o6', Case(C(2, 3, 32, 32, 64, 'ps'), {'fallthrough', 'gen1', 'out6'})),
    ('fall-cout32-o7', Case(C(2, 3, 32, 32, 64, 'yps'), {'fallthrough', 'gen1', 'out7'})),
    ('fall-cout32-o4', Case(C(2, 3, 32, 32, 64, 's'), {'fallthrough', 'gen1', 'out4'})),
    ('fall-cout32-ldy', Case(C(2, 3, 32, 32, 64, 'y', ypad=4), {'fallthrough', 'gen1', 'out1', 'ld>cout'})),
    ('fall-cout32-ldp', Case(C(2, 3, 32, 32, 64, 'p', ppad=4), {'fallthrough', 'gen1', 'out2', 'ld>cout'})),
    ('fall-cout32-slope-0.5', Case(C(2, 3, 32, 32, 64, 'p', slope=-0.5), {'fallthrough', 'gen1', 'out2'})),
    ('fall-cout32-slope1.5', Case(C(2, 3, 32, 32, 64, 'p', slope=1.5), {'fallthrough', 'gen1', 'out2'})),
    ('fall-cout64-slope-0.5', Case(C(2, 3, 64, 32, 64, 'p', slope=-0.5), {'fallthrough', 'gen2', 'out2'})),
    ('fall-cout64-slope1.5', Case(C(2, 3, 64, 32, 64, 'p', slope=1.5), {'fallthrough', 'gen2', 'out2'})),
    ('fall-cin4', Case(C(2, 4, 32, 32, 64, 'p'), {'gen1', 'cin4', 'out2', 'whole-tile'})),              # (not `looks aligned`: the straight-line forms are Cin 3 only)
])

# ---- the edge of RAW (no scale, no shift AND slope 1): a statistics call that lacks one of the three keeps its affine + activation epilogue
RAW_EDGE_CASES = collections.OrderedDict([
    ('sl1-o5-activation-only', Case(C(2, 3, 32, 32, 64, 'ys', scale=False, shift=False, slope=0.1), {'sl1-o5', 'out5'})),
    ('sl1-o5-scale-only', Case(C(2, 3, 32, 32, 64, 'ys', scale=True, shift=False, slope=1.0), {'sl1-o5', 'out5'})),
    ('sl1-o5-shift-only', Case(C(2, 3, 32, 32, 64, 'ys', scale=False, shift=True, slope=1.0), {'sl1-o5', 'out5'})),
    ('fall-cout64-o5-activation-only', Case(C(2, 3, 64, 32, 64, 'ys', scale=False, shift=False, slope=0.1), {'fallthrough', 'gen2', 'out5'})),
])

# ---- walks of the general kernel: thousands of small ragged images (one tile each), every Cin at the 4-tile walk; one walk over multi-tile images
GEN_WALK_CASES = collections.OrderedDict([
    ('gwalk2-cin3', Case(C(3000, 3, 16, 10, 20, 'yps'), {'gen1', 'walk2', 'uneven-walk', 'ragged-both'})),
    ('gwalk3-cin3', Case(C(4200, 3, 16, 10, 20, 'yps'), {'gen1', 'walk3', 'uneven-walk', 'steady-state'})),
    ('gwalk4-cin1', Case(C(6200, 1, 16, 10, 20, 'yps'), {'gen1', 'cin1', 'walk4', 'uneven-walk', 'buffer-reuse'})),
    ('gwalk4-cin2', Case(C(6200, 2, 16, 10, 20, 'yps'), {'gen1', 'cin2', 'walk4', 'uneven-walk', 'buffer-reuse'})),
    ('gwalk4-cin3', Case(C(6200, 3, 16, 10, 20, 'yps'), {'gen1', 'cin3', 'walk4', 'uneven-walk', 'buffer-reuse'})),
    ('gwalk4-cin4', Case(C(6200, 4, 16, 10, 20, 'yps'), {'gen1', 'cin4', 'walk4', 'uneven-walk', 'buffer-reuse'})),
    ('gwalk4-nblk2', Case(C(6200, 3, 40, 10, 20, 'yps'), {'gen2', 'walk4', 'uneven-walk', 'buffer-reuse'})),
    ('gwalk4-multi-tile', Case(C(700, 3, 16, 40, 70, 'yps'), {'gen1', 'walk4', 'uneven-walk', 'multi-tile-image', 'ragged-right', 'ragged-bottom', 'ragged-both', 'whole-tile'})),
    ('gwalk7-cin3', Case(C(14400, 3, 16, 10, 20, 'yps'), {'gen1', 'walk7+', 'uneven-walk', 'buffers-rewritten-twice'})),
])

PARITY_TABLES = (TAP_CASES, MASK_CASES, GEOMETRY_CASES, OUTSET_CASES, STRAIGHT_CASES, FALL_CASES, RAW_EDGE_CASES, GEN_WALK_CASES)
WALKS = ('walk1', 'walk2', 'walk3', 'walk4', 'walk7+')

# ---- the mean-positive regime: one call per kernel form
MEAN_POSITIVE = collections.OrderedDict([
    ('straight', (C(2, 3, 32, 32, 64, 'yp'), C(2, 3, 32, 32, 64, 'ys', scale=False, shift=False, slope=1.0), C(2, 3, 32, 32, 64, 'p'))),
    ('gen1', (C(2, 3, 24, 18, 34, 'yps'),)),
    ('gen2', (C(2, 3, 40, 18, 34, 'yps'),)),
])

# ---- refusals: one case per `return` of y2_conv0_fwd (and per condition of a return that has several), in the entry point's order.
# (call, code): what the library promises to answer, touching no destination
REFUSALS = collections.OrderedDict([
    ('x-null', (C(2, 3, 20, 18, 34, 'yps', nox=True), EINVAL)),
    ('w-null', (C(2, 3, 20, 18, 34, 'yps', now=True), EINVAL)),
    ('nothing-to-write', (C(2, 3, 20, 18, 34, ''), EINVAL)),
    ('batch-0', (C(0, 3, 20, 18, 34, 'yps'), ENOSUP)),
    ('height-0', (C(2, 3, 20, 0, 34, 'ys'), ENOSUP)),
    ('width-0', (C(2, 3, 20, 18, 0, 'ys'), ENOSUP)),
    ('cin-0', (C(2, 0, 20, 18, 34, 'yps'), ENOSUP)),
    ('cin-5', (C(2, 5, 20, 18, 34, 'yps'), ENOSUP)),
    ('cout-0', (C(2, 3, 0, 18, 34, 'yps'), ENOSUP)),
    ('cout-65', (C(2, 3, 65, 18, 34, 'yps'), ENOSUP)),
    ('ldy<cout', (C(2, 3, 20, 18, 34, 'yps', ypad=-1), EINVAL)),
    ('ldp<cout', (C(2, 3, 20, 18, 34, 'yps', ppad=-1), EINVAL)),
    ('pool+odd-height', (C(2, 3, 20, 17, 34, 'yps'), EINVAL)),
    ('pool+odd-width', (C(2, 3, 20, 18, 33, 'p'), EINVAL)),
    ('stats+deterministic', (C(2, 3, 20, 18, 34, 'ys', det=True), ENOSUP)),
    ('stats+deterministic-aligned', (C(2, 3, 32, 32, 64, 'ys', scale=False, shift=False, slope=1.0, det=True), ENOSUP)),
    ('tiles>=2^31', (C((1 << 30) + 1, 3, 20, 17, 1, 'ys'), EINVAL)),       # 2 tiles per image: launch0's own refusal (answered before anything is read)
])
# which `return` of the entry point (by its first words in the source) each refusal is there for
REFUSAL_RETURNS = collections.OrderedDict([
    ('x_nchw == nullptr', ('x-null', 'w-null', 'nothing-to-write')),
    ('B <= 0', ('batch-0', 'height-0', 'width-0', 'cin-0', 'cin-5', 'cout-0', 'cout-65')),
    ('y != nullptr && ldy < Cout', ('ldy<cout',)),
    ('y_pool != nullptr', ('ldp<cout', 'pool+odd-height', 'pool+odd-width')),
    ('stats != nullptr && y2_det.on', ('stats+deterministic', 'stats+deterministic-aligned')),
    ('tiles <= 0', ('tiles>=2^31',)),
])


def first_refusing_test(c):
    """Index into REFUSAL_RETURNS of the first test that refuses c when the tests before it are taken away one by one: the order of the entry point."""
    tests = (c.nox or c.now or not c.outs,
             c.B <= 0 or c.H <= 0 or c.W <= 0 or c.cin < 1 or c.cin > 4 or c.cout < 1 or c.cout > 64,
             'y' in c.outs and c.ypad < 0,
             'p' in c.outs and (c.ppad < 0 or bool(c.H & 1) or bool(c.W & 1)),
             's' in c.outs and c.det,
             c.B * cdiv(max(c.H, 0), TH) * cdiv(max(c.W, 0), TW) > 0x7fffffff)
    return [i for i, t in enumerate(tests) if t][0]


# ================================================================================================ y2_conv0_fwd_sel
# ---- every path a call with gamma can take: the ninth straight-line variant, and the general kernel wherever that variant does not apply
SEL_SMALL = (2, 18, 34)          # (B, H, W) of the general kernel's mask and tap cases: the size of MASK_CASES and TAP_CASES
SEL_CASES = collections.OrderedDict()
for _s in ('small', 'walk3'):    # walk3: the first aligned size with tiles from the in-loop staging (290 MB of z)
    _B, _H, _W = ALIGNED_SIZES[_s][0]
    SEL_CASES['sel-sl-%s' % _s] = Case(S(_B, 3, 32, _H, _W), ALIGNED_SIZES[_s][1] | {'sl1-o7-raw-sel', 'straight', 'sel', 'out7'})
# the call of a deterministic-mode user: no statistics, everything else as the shipped first layer has it.  launch0 once sent it to <3, 1, 3, true, false>,
# which ignores pool_sign and writes the window maximum for every channel
SEL_CASES['sel-nostats-aligned'] = Case(S(1, 3, 32, 16, 32, 'yp'), {'gen1-sel', 'fallthrough', 'out3', 'whole-tile', 'one-tile-image'})
SEL_CASES['sel-nostats-ragged'] = Case(S(2, 3, 20, 18, 34, 'yp'), {'gen1-sel', 'out3', 'ragged-both'})
SEL_CASES['sel-fall-cout64'] = Case(S(2, 3, 64, 32, 64), {'gen2-sel', 'fallthrough', 'out7'})
SEL_CASES['sel-fall-cout64-nostats'] = Case(S(2, 3, 64, 32, 64, 'yp'), {'gen2-sel', 'fallthrough', 'out3'})
SEL_CASES['sel-fall-ldz'] = Case(S(2, 3, 32, 32, 64, ypad=4), {'gen1-sel', 'fallthrough', 'out7', 'ld>cout'})
SEL_CASES['sel-fall-ldzs'] = Case(S(2, 3, 32, 32, 64, ppad=4), {'gen1-sel', 'fallthrough', 'out7', 'ld>cout'})
SEL_CASES['sel-fall-cin4'] = Case(S(2, 4, 32, 32, 64), {'gen1-sel', 'cin4', 'out7', 'whole-tile'})          # (not `looks aligned`, as FALL_CASES' fall-cin4)
for _cout in MASK_COUTS:
    SEL_CASES['sel-mask-cout%d' % _cout] = Case(S(SEL_SMALL[0], 3, _cout, SEL_SMALL[1], SEL_SMALL[2]),
                                                 {'gen%d-sel' % (1 if _cout <= 32 else 2), 'ragged-both', 'out7'} | ({'channel-mask'} if _cout % 32 else set()))
for _cin in (1, 2, 3, 4):
    SEL_CASES['sel-tap-cin%d' % _cin] = Case(S(SEL_SMALL[0], _cin, 7 if _cin % 2 else 40, SEL_SMALL[1], SEL_SMALL[2]),
                                              {'cin%d' % _cin, 'gen%d-sel' % (1 if _cin % 2 else 2), 'ragged-both', 'channel-mask', 'out7'})
SEL_CASES['sel-geo-2x2'] = Case(S(1, 3, GEOMETRY_COUT, 2, 2), {'gen1-sel', 'one-tile-image', 'ragged-both'})          # one window per channel
SEL_CASES['sel-geo-20x36'] = Case(S(3, 3, GEOMETRY_COUT, 20, 36), {'gen1-sel', 'batch', 'multi-tile-image', 'ragged-both', 'ragged-right', 'ragged-bottom', 'whole-tile'})
SEL_CASES['sel-window'] = Case(S(SEL_SMALL[0], 3, 32, SEL_SMALL[1], SEL_SMALL[2], **WINDOW), {'gen1-sel', 'ld>cout', 'ld%4', 'channel-offset', 'ragged-both'})
SEL_CASES['sel-gwalk4-cin3'] = Case(GEN_WALK_CASES['gwalk4-cin3'].c._replace(scale=False, shift=False, slope=1.0, sel=True),
                                    {'gen1-sel', 'cin3', 'walk4', 'uneven-walk', 'buffer-reuse'})
SEL_RANDOM_MAX_B = 4             # the random regime runs the small cases: those of at most this batch

# ---- refusals of the sel entry: one case per `return` (and per condition of a return that has several), in order - the entry's own, then the shared body's
SEL_REFUSALS = collections.OrderedDict([
    ('sel-gamma-null', (S(2, 3, 20, 18, 34, nog=True), EINVAL)),
    ('sel-z-null', (S(2, 3, 20, 18, 34, 'ps'), EINVAL)),
    ('sel-zsel-null', (S(2, 3, 20, 18, 34, 'ys'), EINVAL)),
    ('sel-x-null', (S(2, 3, 20, 18, 34, nox=True), EINVAL)),
    ('sel-w-null', (S(2, 3, 20, 18, 34, now=True), EINVAL)),
    ('sel-batch-0', (S(0, 3, 20, 18, 34), ENOSUP)),
    ('sel-cin-5', (S(2, 5, 20, 18, 34), ENOSUP)),
    ('sel-cout-65', (S(2, 3, 65, 18, 34), ENOSUP)),
    ('sel-ldz<cout', (S(2, 3, 20, 18, 34, ypad=-1), EINVAL)),
    ('sel-ldzs<cout', (S(2, 3, 20, 18, 34, ppad=-1), EINVAL)),
    ('sel-odd-height', (S(2, 3, 20, 17, 34), EINVAL)),
    ('sel-odd-width', (S(2, 3, 20, 18, 33), EINVAL)),
    ('sel-stats+deterministic', (S(2, 3, 20, 18, 34, det=True), ENOSUP)),
    ('sel-stats+deterministic-aligned', (S(2, 3, 32, 32, 64, det=True), ENOSUP)),
    ('sel-tiles>=2^31', (S((1 << 30) + 1, 3, 20, 18, 2), EINVAL)),          # 2 tiles per image, H and W even
])
SEL_REFUSAL_RETURNS = collections.OrderedDict([
    ('gamma != nullptr && z != nullptr && z_sel != nullptr', ('sel-gamma-null', 'sel-z-null', 'sel-zsel-null')),
    ('x_nchw == nullptr', ('sel-x-null', 'sel-w-null')),                      # (`nothing to write` cannot be asked of this entry: z is required)
    ('B <= 0', ('sel-batch-0', 'sel-cin-5', 'sel-cout-65')),
    ('y != nullptr && ldy < Cout', ('sel-ldz<cout',)),
    ('y_pool != nullptr', ('sel-ldzs<cout', 'sel-odd-height', 'sel-odd-width')),
    ('stats != nullptr && y2_det.on', ('sel-stats+deterministic', 'sel-stats+deterministic-aligned')),
    ('tiles <= 0', ('sel-tiles>=2^31',)),
])


def sel_first_refusing_test(c):
    """first_refusing_test for a y2_conv0_fwd_sel call: index into SEL_REFUSAL_RETURNS."""
    if c.nog or 'y' not in c.outs or 'p' not in c.outs:
        return 0
    return 1 + first_refusing_test(c)
