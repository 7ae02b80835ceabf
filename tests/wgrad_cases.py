"""Case tables of the weight-gradient tests (tests/test_gpu_wgrad.py runs them on the GPU, tests/test_wgrad_cases.py proves on the CPU that
they reach what they claim), and the Python mirror of the host code that picks a kernel for a problem:

    csrc/conv_wgrad.hip   wgrad_tj, wgrad_splits, the tile choice of wgrad_impl, the grids of y2_conv0_wgrad / y2_conv0_wgrad_fused
    csrc/wino.hip         y2_wino_wgrad_ex: in-loader gradient (DZRAW) against the three-step form
    csrc/common.h         wino6_grid

Every case names the dispatch path it is there for: tile variant (TI, TJ), loader, 'split' / 'unsplit', and the shape of the tile grid.  A case whose
claim the mirror does not confirm fails the CPU test, so a change of the heuristics that silently moves a case to another path is noticed there."""
import collections

NUM_CU = 256                    # Y2_NUM_CU (csrc/common.h)
KS = 32                         # pixels per slab (csrc/conv_wgrad.hip)
VARIANTS = ((32, 128), (64, 64), (64, 128), (128, 64), (128, 128))
DZRAW_MAX_COUT = 256            # y2_wino_wgrad_ex builds the gradient operand in the loader up to this width
ROW_WALK = 4 * 4 * NUM_CU       # first layer: rows (row pairs) from which a wave walks more than one

Plan = collections.namedtuple('Plan', 'TI TJ splits slabs_per_split slabs tiles')


def cdiv(a, b):
    return (a + b - 1) // b


def wgrad_tj(ncols, cout):
    if cout <= 32:
        return 128
    p128, p64 = cdiv(ncols, 128) * 128, cdiv(ncols, 64) * 64
    return 64 if p128 * 100 >= p64 * 115 else 128


def wgrad_plan(M, ncols, cout, groups=1):
    """wgrad_splits and the tile choice of wgrad_impl (default mode)."""
    TI = 32 if cout <= 32 else (64 if cout <= 64 else 128)
    TJ = wgrad_tj(ncols, cout)
    tiles = cdiv(cout, TI) * cdiv(ncols, TJ)
    slabs = cdiv(M, KS)
    fill = 2 if TI * TJ >= 128 * 128 else (3 if TI * TJ >= 128 * 64 else 4)
    splits = cdiv(fill * NUM_CU, tiles * groups)
    splits = max(min(splits, max(slabs // 8, 1)), 1)
    sps = cdiv(slabs, splits)
    return Plan(TI, TJ, cdiv(slabs, sps), sps, slabs, tiles)


def out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def direct_plan(B, cin, cout, H, W, k, stride=1, pad=None):
    pad = (k - 1) // 2 if pad is None else pad
    return wgrad_plan(B * out_size(H, k, stride, pad) * out_size(W, k, stride, pad), k * k * cin, cout)


def wino_tiles(B, H, W):
    return B * cdiv(H, 2) * cdiv(W, 2)


def wino_plan(B, cin, cout, H, W):
    """The 16 grouped reductions of the 2x2-tile form."""
    return wgrad_plan(wino_tiles(B, H, W), cin, cout, 16)


def wino_form(cout, deterministic=False):
    return 'dzraw' if cout <= DZRAW_MAX_COUT and not deterministic else 'three-step'


Wino6Grid = collections.namedtuple('Wino6Grid', 'th tw tall wide gx T')


def wino6_grid(B, H, W):
    """csrc/common.h: per-image 4x4 tiles, or the batch as one mosaic of gx images per row when that takes fewer tiles."""
    th, tw, tall, wide, best_gx = cdiv(H, 4), cdiv(W, 4), 0, 0, 1
    T = B * th * tw
    for gx in range(1, min(B, 4096) + 1):
        gy = cdiv(B, gx)
        rows, cols = gy * (H + 1) - 1, gx * (W + 1) - 1
        h, w = cdiv(rows, 4), cdiv(cols, 4)
        if h * w < T:
            T, th, tw, tall, wide, best_gx = h * w, h, w, H + 1, (W + 1 if gx > 1 else 0), gx
    return Wino6Grid(th, tw, tall, wide, best_gx, T)


def wino6_plan(B, cin, cout, H, W):
    """The 36 grouped reductions of the 4x4-tile form."""
    return wgrad_plan(wino6_grid(B, H, W).T, cin, cout, 36)


def grid_shapes(plan, ncols, cout):
    """Which inner loops a launch runs.  'full': every tile is whole - only compute_slab_spread (given two slabs per split).  'ragged-rows' / 'ragged-cols':
    some wave owns a 32x32 block that lies completely outside the output in that direction - compute_slab_checked.  'ragged-edge': the last block
    is cut inside (masked loads and stores, but still the spread loop)."""
    out = set()
    if cdiv(cout, 32) * 32 < cdiv(cout, plan.TI) * plan.TI:
        out.add('ragged-rows')
    if cdiv(ncols, 32) * 32 < cdiv(ncols, plan.TJ) * plan.TJ:
        out.add('ragged-cols')
    if cout % 32 or ncols % 32:
        out.add('ragged-edge')
    if not out and plan.slabs_per_split >= 2:
        out.add('full')
    return out


def split_edges(plan, M, cin, cout, k):
    """Edges of a split launch that a case may claim."""
    out = set()
    if plan.splits > 1:
        if plan.splits * plan.slabs_per_split > plan.slabs:
            out.add('short-last-split')
        if M % KS:
            out.add('M%32')
        if k > 1 and any((t * cin) % plan.TJ for t in range(1, k * k)):
            out.add('tap-in-tile')
        if cout % plan.TI:
            out.add('cout%TI')
    return out


def conv0_grid(rows):
    """Workgroups (4 waves each) of y2_conv0_wgrad over `rows` image rows, or of y2_conv0_wgrad_fused over `rows` row pairs."""
    return cdiv(rows, 4) if rows < ROW_WALK else 4 * NUM_CU


def conv0_rows_per_wave(rows):
    return cdiv(rows, 4 * conv0_grid(rows))


# ------------------------------------------------------------------------------------------------ direct kernel
# name: (B, cin, cout, H, W, k), (TI, TJ), 'split' | 'unsplit', shape of the tile grid.  k = 1 is the LIN loader, k = 3 the general one.
DirectCase = collections.namedtuple('DirectCase', 'shape tile split grid')
DIRECT_CASES = {n: DirectCase(*v) for n, v in {
    # general loader
    'g-32x128-unsplit': ((1, 8, 12, 5, 7, 3), (32, 128), 'unsplit', 'ragged-cols'),
    'g-32x128-split3': ((3, 12, 32, 17, 19, 3), (32, 128), 'split', 'ragged-edge'),
    'g-32x128-split-tap20': ((2, 20, 8, 23, 21, 3), (32, 128), 'split', 'ragged-cols'),
    'g-64x64-unsplit': ((2, 32, 64, 8, 12, 3), (64, 64), 'unsplit', 'ragged-cols'),
    'g-64x64-split3': ((2, 32, 64, 20, 19, 3), (64, 64), 'split', 'ragged-cols'),
    'g-64x128-unsplit': ((1, 128, 64, 7, 9, 3), (64, 128), 'unsplit', 'full'),
    'g-64x128-split2': ((2, 128, 48, 17, 16, 3), (64, 128), 'split', 'ragged-edge'),
    'g-64x128-ragged-cols': ((1, 8, 48, 9, 9, 3), (64, 128), 'unsplit', 'ragged-cols'),
    'g-128x128-unsplit': ((1, 64, 128, 9, 9, 3), (128, 128), 'unsplit', 'ragged-cols'),
    'g-128x64-split2': ((2, 32, 100, 18, 17, 3), (128, 64), 'split', 'ragged-cols'),
    'g-128x64-unsplit': ((1, 32, 100, 6, 5, 3), (128, 64), 'unsplit', 'ragged-cols'),
    'g-128x128-unsplit-rows': ((1, 128, 132, 6, 5, 3), (128, 128), 'unsplit', 'ragged-rows'),
    'g-128x128-split2': ((2, 128, 256, 17, 17, 3), (128, 128), 'split', 'full'),
    'g-128x128-split-tap36': ((2, 36, 132, 17, 16, 3), (128, 128), 'split', 'ragged-rows'),
    'g-128x128-split-tap100': ((2, 100, 68, 17, 17, 3), (128, 128), 'split', 'ragged-rows'),
    # LIN loader
    'l-32x128-split2': ((3, 64, 8, 13, 13, 1), (32, 128), 'split', 'ragged-cols'),
    'l-64x64-split3': ((2, 32, 64, 23, 21, 1), (64, 64), 'split', 'ragged-cols'),
    'l-64x128-split3': ((2, 128, 64, 23, 21, 1), (64, 128), 'split', 'full'),
    'l-128x64-split2': ((2, 64, 128, 19, 17, 1), (128, 64), 'split', 'full'),
    'l-128x128-split2': ((2, 100, 132, 19, 17, 1), (128, 128), 'split', 'ragged-rows'),
    'l-128x64-unsplit': ((1, 36, 132, 3, 5, 1), (128, 64), 'unsplit', 'ragged-rows'),
    'l-32x128-unsplit': ((1, 64, 8, 3, 5, 1), (32, 128), 'unsplit', 'ragged-cols'),
    'l-64x64-unsplit': ((1, 32, 64, 5, 7, 1), (64, 64), 'unsplit', 'ragged-cols'),
    'l-64x128-unsplit': ((1, 128, 48, 5, 7, 1), (64, 128), 'unsplit', 'ragged-edge'),
    'l-64x128-ragged-cols': ((2, 96, 48, 16, 16, 1), (64, 128), 'split', 'ragged-cols'),
    'l-128x128-unsplit': ((1, 100, 132, 5, 7, 1), (128, 128), 'unsplit', 'ragged-rows'),
    # whole tiles, split: compute_slab_spread on every wave, atomic epilogue
    'l-64x128-full': ((2, 128, 64, 16, 16, 1), (64, 128), 'split', 'full'),
    'l-128x64-full': ((2, 64, 128, 16, 16, 1), (128, 64), 'split', 'full'),
    'l-128x128-full': ((2, 128, 128, 16, 16, 1), (128, 128), 'split', 'full'),
    'l-64x64-full': ((2, 64, 64, 16, 16, 1), (64, 64), 'split', 'full'),
    'l-32x128-full': ((2, 128, 32, 16, 16, 1), (32, 128), 'split', 'full'),
    # coordinate stepping of the general loader (q32 / r32): W < 32, == 32, > 32, 1, and a slab that spans several images
    'g-geom-w32': ((1, 8, 12, 3, 32, 3), (32, 128), 'unsplit', 'ragged-cols'),
    'g-geom-w45': ((1, 8, 12, 3, 45, 3), (32, 128), 'unsplit', 'ragged-cols'),
    'g-geom-w1': ((2, 8, 12, 37, 1, 3), (32, 128), 'unsplit', 'ragged-cols'),
    'g-geom-hw<32': ((13, 8, 12, 3, 3, 3), (32, 128), 'unsplit', 'ragged-cols'),
    'g-geom-w70-split': ((1, 8, 12, 9, 70, 3), (32, 128), 'split', 'ragged-cols'),
}.items()}
GEOMETRY = {'W<32': 'g-32x128-unsplit', 'W==32': 'g-geom-w32', 'W>32': 'g-geom-w45', 'W==1': 'g-geom-w1', 'H*W<32': 'g-geom-hw<32'}
# the split launches that carry the edges the split bookkeeping can get wrong
DIRECT_EDGES = {'short-last-split': 'g-32x128-split3', 'M%32': 'g-64x64-split3', 'tap-in-tile': 'g-128x128-split-tap36', 'cout%TI': 'g-128x64-split2'}
TAP_CASES = ('g-32x128-split-tap20', 'g-128x128-split-tap36', 'g-128x128-split-tap100')      # Cin = 20, 36, 100: a tap boundary inside a column tile

# y2_conv_wgrad_ex: name: (B, cin, cout, H, W, k, stride, pad) - the five shapes of test_strided_wgrad_and_transposed_dgrad, 5x5 / 1 / 2, and 3x3 / 2 / 0
# on an even map (the last input row and column are never read)
EX_CASES = {
    'ex-3x3s2p1': (2, 16, 32, 19, 19, 3, 2, 1),
    'ex-1x1s2': (2, 32, 64, 20, 20, 1, 2, 0),
    'ex-7x7s2p3': (1, 4, 64, 32, 40, 7, 2, 3),
    'ex-3x3s2p1-64': (2, 64, 64, 10, 10, 3, 2, 1),
    'ex-3x3s1p1': (2, 8, 16, 9, 9, 3, 1, 1),
    'ex-5x5s1p2': (2, 8, 12, 9, 11, 5, 1, 2),
    'ex-3x3s2p0-unread-edge': (2, 8, 12, 10, 12, 3, 2, 0),
}

# ------------------------------------------------------------------------------------------------ Winograd, 2x2 tiles
# name: (B, cin, cout, H, W), (TI, TJ), 'dzraw' | 'three-step', 'split' | 'unsplit'
WinoCase = collections.namedtuple('WinoCase', 'shape tile form split')
WINO_CASES = {n: WinoCase(*v) for n, v in {
    'w-32x128-split': ((2, 8, 12, 32, 32), (32, 128), 'dzraw', 'split'),
    'w-64x64-split': ((2, 32, 64, 33, 31), (64, 64), 'dzraw', 'split'),
    'w-64x128-split': ((3, 128, 48, 27, 29), (64, 128), 'dzraw', 'split'),
    'w-128x64-split': ((2, 32, 100, 32, 33), (128, 64), 'dzraw', 'split'),
    'w-128x128-split': ((2, 128, 132, 32, 32), (128, 128), 'dzraw', 'split'),
    'w-32x128-unsplit': ((2, 8, 12, 15, 17), (32, 128), 'dzraw', 'unsplit'),
    'w-64x64-unsplit': ((1, 32, 64, 9, 7), (64, 64), 'dzraw', 'unsplit'),
    'w-64x128-unsplit': ((1, 128, 48, 7, 9), (64, 128), 'dzraw', 'unsplit'),
    'w-128x64-unsplit': ((1, 32, 100, 8, 8), (128, 64), 'dzraw', 'unsplit'),
    'w-128x128-unsplit': ((1, 128, 132, 7, 7), (128, 128), 'dzraw', 'unsplit'),
    'w3-128x64-split': ((2, 4, 260, 32, 32), (128, 64), 'three-step', 'split'),
    'w3-128x128-split': ((2, 128, 260, 32, 32), (128, 128), 'three-step', 'split'),
    'w3-128x128-unsplit': ((1, 128, 260, 7, 9), (128, 128), 'three-step', 'unsplit'),
    # tile raggedness: a tile without a second row / column (table bits 30 / 31), the smallest maps
    'w-h-odd': ((2, 8, 12, 7, 6), (32, 128), 'dzraw', 'unsplit'),
    'w-w-odd': ((2, 8, 12, 6, 7), (32, 128), 'dzraw', 'unsplit'),
    'w-1x1': ((3, 8, 12, 1, 1), (32, 128), 'dzraw', 'unsplit'),
    'w-1x3': ((3, 8, 12, 1, 3), (32, 128), 'dzraw', 'unsplit'),
    'w3-h-odd': ((1, 8, 260, 5, 4), (128, 64), 'three-step', 'unsplit'),
    'w3-w-odd': ((1, 8, 260, 4, 5), (128, 64), 'three-step', 'unsplit'),
}.items()}
WINO_PARITY = {'even,even': 'w-32x128-split', 'odd,odd': 'w-32x128-unsplit', 'odd,even': 'w-h-odd', 'even,odd': 'w-w-odd', '1x1': 'w-1x1', '1x3': 'w-1x3'}
WINO_V_CASES = ('w-64x128-split', 'w-64x128-unsplit')          # the v_transformed route (x = NULL)

# ------------------------------------------------------------------------------------------------ Winograd, 4x4 tiles (36 groups)
# name: (B, cin, cout, H, W), (TI, TJ), 'split' | 'unsplit', mosaic tiling or per-image tiling
Wino6Case = collections.namedtuple('Wino6Case', 'shape tile split mosaic')
WINO6_CASES = {n: Wino6Case(*v) for n, v in {
    'f-split-64x64': ((2, 8, 12, 64, 64), (32, 128), 'split', False),
    'f-split-mosaic': ((9, 8, 12, 29, 30), (32, 128), 'split', True),
    'f-unsplit-13x14': ((1, 8, 12, 13, 14), (32, 128), 'unsplit', False),
    'f-unsplit-7x9-mosaic': ((2, 16, 8, 7, 9), (32, 128), 'unsplit', True),
    'f-unsplit-6x7': ((1, 8, 8, 6, 7), (32, 128), 'unsplit', False),
    'f-unsplit-11x12-wide': ((1, 128, 132, 11, 12), (128, 128), 'unsplit', False),
}.items()}

# ------------------------------------------------------------------------------------------------ first layer
CONV0_CIN = (1, 2, 3)
CONV0_COUT = (4, 6, 32, 33, 40, 64)
CONV0_W = (5, 16, 17, 33)
CONV0_ROW_WALK = (65, 3, 32, 64, 16)                 # B, cin, cout, H, W: B*H = 4160 rows
CONV0_FUSED_ROW_WALK = (129, 3, 32, 64, 16)          # B*H/2 = 4128 row pairs


def conv0_cases():
    """(cin, cout, W, ldz): the whole matrix - 144 launches of a few microseconds."""
    return [(cin, cout, W, cout + pad) for cin in CONV0_CIN for cout in CONV0_COUT for W in CONV0_W for pad in (0, 5)]


# ------------------------------------------------------------------------------------------------ operand layouts
# name: (ldx - Cin, ldz - Cout, x offset, dz offset) in floats
LAYOUTS = {'dense': (0, 0, 0, 0), 'ldx-window': (12, 0, 0, 0), 'ldz-window': (0, 8, 0, 0), 'both-offset': (8, 12, 4, 8)}

# mean-positive operands: one split case per tile variant (direct) and per Winograd form
MEANPOS_DIRECT = ('g-32x128-split3', 'g-64x64-split3', 'g-64x128-split2', 'g-128x64-split2', 'g-128x128-split2')
MEANPOS_WINO = ('w-64x128-split', 'w3-128x128-split')
MEANPOS_WINO6 = ('f-split-64x64',)
# deterministic mode: one split case per tile variant and loader (direct), one split grouped case per variant
DET_DIRECT = ('g-32x128-split3', 'g-64x64-split3', 'g-64x128-split2', 'g-128x64-split2', 'g-128x128-split2',
              'l-32x128-split2', 'l-64x64-split3', 'l-64x128-split3', 'l-128x64-split2', 'l-128x128-split2')
DET_WINO = ('w-32x128-split', 'w-64x64-split', 'w-64x128-split', 'w-128x64-split', 'w-128x128-split')
DET_TOO_SMALL = 'g-128x128-split2'                   # 2 splits x 256 x 1152 floats = 2.25 MiB of partial rows: more than the 1 MiB minimum scratch
DET_MIN_BYTES = 1 << 20
