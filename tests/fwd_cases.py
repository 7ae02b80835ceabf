"""Case tables of the forward-convolution tests (tests/test_gpu_fwd.py runs them on the GPU, tests/test_fwd_cases.py proves on the CPU that they
reach what they claim), and the Python mirror of the host code that picks a kernel for a problem:

    csrc/conv_fwd.hip   conv_fwd_impl (standard / vec / dma_ok / gen / ctail / persist, the tile-7 fallback), choose_tile with effective_rounds,
                        plan_split, the K-slice bounds of a split tile, the workspace size, the epilogue a tile runs, the refusals
    csrc/wino.hip       y2_internal_wino_conv / y2_internal_wino6_conv: tiles, batch chunks, kernel family and variant, out_mask, fused_grid

No torch and no library: plain integer (and, where the host code uses them, double) arithmetic in the host code's order.

The workspace size is mirrored exactly as y2_conv_fwd_workspace_bytes answers, including one oddity that is kept on purpose: launch_dma answers
the size query before it looks at PERSIST, so a persistent tile id (11 / 12 / 13 / 15) reports the split scratch of the plain tile of its shape
although a persistent launch never splits and never touches the workspace.

Every case names the path it is there for.  A case whose claim the mirror does not confirm fails the CPU test."""
import collections

from wgrad_cases import cdiv, wino6_grid

NUM_CU = 256                    # Y2_NUM_CU (csrc/common.h)
NUM_XCD = 8                     # Y2_NUM_XCD
OK, EINVAL, EALIGN, ENOSUP = 0, -1, -2, -3      # include/yolo2_hip.h
WF_DUMP_BYTES = 1024            # csrc/wino.hip
WF2_DEFAULT_VARIANT = 3
F3_TM = 32

# tile id -> (BM, BN, threads) of dispatch_dma; 7 is the wave kernel (64 threads own a 64x64 tile)
DMA_TILES = {1: (128, 128, 256), 2: (128, 64, 256), 3: (64, 64, 256), 5: (64, 128, 256), 6: (128, 32, 256), 8: (256, 128, 512), 9: (128, 256, 512),
             7: (64, 64, 64), 11: (128, 128, 256), 12: (128, 64, 256), 13: (64, 64, 256), 15: (64, 128, 256)}
PERSIST_OF = {11: 1, 12: 2, 13: 3, 15: 5}       # persistent id -> the plain id of the same tile shape
GEN_TILES = (1, 2, 3, 5, 6)
# tile id -> (BM, BN, BK) of dispatch_tile (the register-staged kernel)
REG_TILES = {1: (128, 128, 32), 2: (128, 64, 32), 3: (64, 64, 32), 4: (256, 64, 32), 5: (64, 128, 32), 11: (128, 128, 16), 13: (64, 64, 16),
             21: (128, 128, 64), 23: (64, 64, 64)}
ABLATIONS = (91, 92, 93)        # ids of the removed timing ablations of dispatch_tile (wrong results by design): the library must refuse them, and 191 - 193 with them
REFUSED_TILE_SHAPE = (1, 4, 4, 4, 4, 3)        # B, Cin, Cout, H, W, k: the smallest problem whose unknown tile id reaches dispatch_tile<false, true>'s default

# x as the kernels see it: (pad, off) = extra floats per pixel row and where in the row the Cin channels start.  Multiples of 4 keep the LDS-DMA
# and Winograd paths; the NONVEC layouts break ldx % 4 or the 16-byte alignment of x and so force conv_fwd_kernel<VEC = false>.
LAYOUTS = collections.OrderedDict([('dense', (0, 0)), ('padded', (8, 0)), ('offset', (4, 4)), ('both', (12, 4))])
NONVEC_LAYOUTS = collections.OrderedDict([('odd-ld', (3, 0)), ('misaligned', (4, 1)), ('odd-both', (5, 2))])

_P = collections.namedtuple('P', 'B cin cout H W k tile stride pad transposed out_hw outs out_mode residual groups')


def P(B, cin, cout, H, W, k, tile=0, stride=1, pad=None, transposed=False, out_hw=None, outs='y', out_mode=0, residual=False, groups=1):
    """A y2_conv_fwd problem.  outs: which destinations are given, a subset of 'y' (full), 'p' (2x2-pooled), 's' (statistics)."""
    return _P(B, cin, cout, H, W, k, tile, stride, (k - 1) // 2 if pad is None else pad, transposed, out_hw, outs, out_mode, residual, groups)


def out_size(n, k, stride, pad):
    d = n + 2 * pad - k
    return (d // stride if d >= 0 else -(-d // stride)) + 1         # C division truncates towards zero


def out_hw(p):
    if p.transposed:
        return p.out_hw
    return out_size(p.H, p.k, p.stride, p.pad), out_size(p.W, p.k, p.stride, p.pad)


def plan_split(tiles, nk, tile_elems, ws_bytes, procs=NUM_CU):
    """(full_tiles, ksplit).  ws_bytes None = unlimited (the size query)."""
    rem = tiles % procs
    if rem == 0 or nk < 8:
        return tiles, 1
    best, bs = 1.0, 1
    s = 2
    while s <= 16 and nk // s >= 4:
        t = float(cdiv(rem * s, procs)) / s * 1.02 + 0.01
        if t < best - 1e-9:
            best, bs = t, s
        s += 1
    if bs == 1:
        return tiles, 1
    before, after = float(cdiv(tiles, procs)), float(tiles // procs) + best
    if after > before * 0.97:
        return tiles, 1
    if ws_bytes is not None and rem * bs * tile_elems * 4 > ws_bytes:
        return tiles, 1
    return tiles - rem, bs


def kslice(nk, part, ksplit):
    """[ks0, ks1): the slabs K-slice `part` of a split tile adds up."""
    return nk * part // ksplit, nk * (part + 1) // ksplit


def effective_rounds(tiles, nk):
    rem = tiles % NUM_CU
    frac = 1.0 if rem else 0.0
    if rem and nk >= 8:
        s = 2
        while s <= 16 and nk // s >= 4:
            t = float(cdiv(rem * s, NUM_CU)) / s * 1.02 + 0.01
            if t < frac:
                frac = t
            s += 1
    return float(tiles // NUM_CU) + frac


CANDIDATES = ((5, 64, 128, 0.80), (3, 64, 64, 0.78), (2, 128, 64, 0.775), (1, 128, 128, 0.74), (6, 128, 32, 0.60))


def choose_tile(M, cout, nk):
    best, best_cost = 3, 1e300
    for tid, bm, bn, eff in CANDIDATES:
        cost = effective_rounds(cdiv(M, bm) * cdiv(cout, bn), nk) * bm * bn / eff
        if cost < best_cost:
            best, best_cost = tid, cost
    return best


Route = collections.namedtuple('Route', 'rc family tile bm bn poolord vec standard dma_ok gen ctail persist nk nk_choice tiles procs fast_epi M chosen')


def _refuse(rc):
    return Route(rc, None, 0, 0, 0, False, False, False, False, False, False, False, 0, 0, 0, 0, False, 0, False)


def route(p, pad=0, off=0, w_aligned=True, query=False):
    """What conv_fwd_impl does with problem p whose x has row stride cin + pad and starts `off` floats into a 16-byte aligned row.  query: the size
    query's view - it answers "no scratch" for every problem of the register-staged kernel before that path's own refusals are looked at."""
    if not p.outs:
        return _refuse(EINVAL)
    if p.k < 1 or p.k > 7:
        return _refuse(ENOSUP)
    ldx = p.cin + pad
    Ho, Wo = out_hw(p)
    if p.transposed and (Ho <= 0 or Wo <= 0 or out_size(Ho, p.k, p.stride, p.pad) != p.H or out_size(Wo, p.k, p.stride, p.pad) != p.W):
        return _refuse(EINVAL)
    if Ho <= 0 or Wo <= 0:
        return _refuse(EINVAL)
    standard = not p.transposed and p.stride == 1 and p.pad == (p.k - 1) // 2 and p.k in (1, 3)
    if 'y' in p.outs and p.out_mode == 1 and (p.H & 1 or p.W & 1):
        return _refuse(EINVAL)
    if p.out_mode not in (0, 1):
        return _refuse(EINVAL)
    pool = 'p' in p.outs
    if pool and (p.H & 1 or p.W & 1):
        return _refuse(EINVAL)
    if p.residual and (pool or p.out_mode != 0):
        return _refuse(ENOSUP)
    Min, M = p.B * p.H * p.W, p.B * Ho * Wo
    taps = p.k * p.k
    K = taps * p.cin
    fast_epi = not p.residual and p.out_mode == 0 and ((pool and p.outs == 'p') or (not pool and 'y' in p.outs))
    vec = p.cin % 4 == 0 and ldx % 4 == 0 and off % 4 == 0 and w_aligned
    nk_choice = taps * cdiv(p.cin, 32) if standard else cdiv(K, 32)
    chosen = p.tile <= 0
    tile = p.tile if p.tile > 0 else choose_tile(M * p.groups, p.cout, nk_choice)
    if tile == 7 and (not standard or p.cin % 16 or p.groups > 1):
        tile = 3
    persist = tile in PERSIST_OF
    if persist and (not standard or p.groups > 1 or pool or p.cin % 32 or not vec):
        return _refuse(ENOSUP)
    dma_tile = tile in DMA_TILES
    dma_ok = vec and Min * ldx * 4 < 0x7fffffff and p.cout * K * 4 < 0x7fffffff and dma_tile
    gen = not standard or (p.groups == 1 and dma_ok and tile not in (7, 8, 9) and not persist and p.cin < 32 and not pool and p.out_mode == 0)
    if p.groups > 1 and (not dma_ok or gen or pool or p.out_mode != 0 or 's' in p.outs or p.residual):
        return _refuse(ENOSUP)

    def made(family, bm, bn, poolord, ctail, nk, procs):
        return Route(OK, family, tile, bm, bn, poolord, vec, standard, dma_ok, gen, ctail, persist, nk, nk_choice, cdiv(M, bm) * cdiv(p.cout, bn) * p.groups, procs, fast_epi, M,
                     chosen)
    if gen:
        if not dma_ok or pool or p.out_mode != 0 or tile not in GEN_TILES:
            return _refuse(ENOSUP)
        bm, bn, _ = DMA_TILES[tile]
        return made('conv_fwd_dma_kernel', bm, bn, False, False, cdiv(K, 32), NUM_CU)
    if dma_ok:
        bm, bn, _ = DMA_TILES[tile]
        if tile == 7:
            return made('conv_fwd_wave_kernel', bm, bn, pool, False, taps * (p.cin // 16), 4 * NUM_CU)
        family = 'conv_fwd_dma_kernel[persistent]' if persist else 'conv_fwd_dma_kernel[grouped]' if p.groups > 1 else 'conv_fwd_dma_kernel'
        return made(family, bm, bn, pool, p.cin % 32 != 0, taps * cdiv(p.cin, 32), NUM_CU)
    if query:
        return made('conv_fwd_kernel', 64, 64, pool, False, 0, NUM_CU)
    if p.residual:
        return _refuse(ENOSUP)
    if tile > 100:
        tile -= 100
    if tile not in REG_TILES:                                   # dispatch_tile's default: ABLATIONS are unknown ids like any other
        return _refuse(ENOSUP)
    bm, bn, bk = REG_TILES[tile]
    return made('conv_fwd_kernel', bm, bn, pool, False, taps * cdiv(p.cin, bk), NUM_CU)


def splits(r, ws_bytes):
    """(full_tiles, ksplit) of a launch that is offered ws_bytes of aligned workspace (None: as much as it asks for, 0: none)."""
    if r.rc != OK or r.family in ('conv_fwd_kernel', 'conv_fwd_dma_kernel[persistent]'):
        return r.tiles, 1
    return plan_split(r.tiles, r.nk, r.bm * r.bn, ws_bytes, r.procs)


def workspace_bytes(p, pad=0, off=0):
    """y2_conv_fwd_workspace_bytes (algo 0): a refusal's code, else the bytes of the largest split (see the module docstring on persistent ids)."""
    r = route(p, pad, off, query=True)
    if r.rc != OK:
        return r.rc
    if r.family == 'conv_fwd_kernel':
        return 0
    full, ks = plan_split(r.tiles, r.nk, r.bm * r.bn, None, r.procs)
    return (r.tiles - full) * ks * r.bm * r.bn * 4


def epilogues(r, cout):
    """Which of conv_epilogue_fast / conv_epilogue_general the tiles of a launch run."""
    out = set()
    if r.fast_epi and r.M >= r.bm and cout >= r.bn:
        out.add('fast')
    if not r.fast_epi or r.M % r.bm or cout % r.bn:
        out.add('general')
    return out


def max_slots(r):
    """Upper bound of the workgroup slots of a persistent launch: the occupancy query on the device decides, capped at 4 per CU; the two LDS stages of
    (BM + BN) x 32 floats out of a CU's 160 KB bound it from above.  A persistent launch has min(tiles, slots) workgroups, so more tiles than this
    bound means some workgroup walks several tiles, and fewer tiles than CUs means none does."""
    return NUM_CU * min(4, (160 << 10) // (2 * (r.bm + r.bn) * 32 * 4))


def claims_of(p, pad=0, off=0):
    """Everything the mirror says about the launch of p when it is offered all the workspace it asks for: the vocabulary of the case tables."""
    r = route(p, pad, off)
    if r.rc != OK:
        return {'refused'}
    out = {'tile%d' % r.tile} | epilogues(r, p.cout)
    full, ks = splits(r, None)
    out.add('unsplit' if ks == 1 else 'split-all' if full == 0 else 'split-mixed')
    if ks > 1:
        out.add('ksplit-ragged' if r.nk % ks else 'ksplit-even')
    if r.nk >= 8:
        out.add('nk>=8')
    out.update(t for t, on in (('ctail', r.ctail), ('poolord', r.poolord), ('gen', r.gen), ('chosen', r.chosen)) if on)
    if r.family == 'conv_fwd_kernel':
        out.add('reg-vec' if r.vec else 'reg-nonvec')
    elif r.family == 'conv_fwd_wave_kernel':
        out.add('wave')
        if p.cin % 32 == 16:
            out.add('cin%32==16')
    elif r.persist:
        out.add('persistent')
        out.add('more-than-slots' if r.tiles > max_slots(r) else 'fewer-than-slots' if r.tiles < NUM_CU else 'about-slots')
        out.add('one-slab' if r.nk == 1 else 'odd-slabs' if r.nk & 1 else 'even-slabs')
    elif r.gen:
        out.add('transposed' if p.transposed else 'linear-k' if r.standard else 'k%d' % p.k if p.k > 3 else 'strided' if p.stride > 1 else 'padded')
    else:
        out.add('dma')
    if p.tile == 7 and r.tile == 3:
        out.add('wave-fallback')
    return out


# ------------------------------------------------------------------------------------------------ Winograd drivers
WinoRoute = collections.namedtuple('WinoRoute', 'rc family variant out_mask out_inst cb nchunks T th tw grids ws_bytes names inner')


def align256(b):
    return (b + 255) & ~255


def out_mask(outs):
    return ('y' in outs) * 1 + ('p' in outs) * 2 + ('s' in outs) * 4


def wino_route(p, algo, pad=0, off=0, variant=None, chunk_mb=None, ldy=None, ldp=None):
    """y2_internal_wino_conv (algo 1, 2, 3) and y2_internal_wino6_conv (6, 7).  variant: Y2_WF_VARIANT, chunk_mb: Y2_WINO_CHUNK_MB (None = unset)."""
    def refuse(rc):
        return WinoRoute(rc, None, None, out_mask(p.outs), None, 0, 0, 0, 0, 0, (), rc, (), None)
    ldx = p.cin + pad
    if algo in (6, 7):
        if p.outs != 'y' or p.residual or p.out_mode != 0:
            return refuse(ENOSUP)
        if p.k != 3 or p.stride != 1 or p.pad != 1 or p.transposed:
            return refuse(ENOSUP)
        if p.cin % 4 or p.cout % 4:
            return refuse(ENOSUP)
        g = wino6_grid(p.B, p.H, p.W)
        vbytes, mbytes = align256(36 * g.T * p.cin * 4), align256(36 * g.T * p.cout * 4)
        q = P(1, p.cin, p.cout, 1, g.T, 1, tile=p.tile, groups=36)
        inner = route(q)
        if inner.rc != OK:
            return refuse(inner.rc)
        if algo == 7 and (pad or off % 4):
            return refuse(EINVAL)
        ws = (0 if algo == 7 else vbytes) + mbytes + workspace_bytes(q)
        names = ([] if algo == 7 else ['wino6_in_kernel']) + ['conv_fwd_dma_kernel[grouped]', 'wino6_out_kernel']
        return WinoRoute(OK, 'wino6', None, 1, None, p.B, 1, g.T, g.th, g.tw, (), ws, tuple(names), inner)
    if not p.outs:
        return refuse(EINVAL)
    if p.k != 3 or p.stride != 1 or p.pad != 1 or p.transposed:
        return refuse(ENOSUP)
    if p.residual or p.out_mode != 0:
        return refuse(ENOSUP)
    if p.cin % 4 or p.cout % 4 or ldx % 4 or off % 4:
        return refuse(ENOSUP)
    if 'p' in p.outs and (p.H & 1 or p.W & 1):
        return refuse(EINVAL)
    implicit, fused = algo == 3, algo in (2, 3)
    if fused and p.cin % 32:
        return refuse(ENOSUP)
    if implicit and p.cin < 32:
        return refuse(ENOSUP)
    th, tw = (p.H + 1) // 2, (p.W + 1) // 2
    img_bytes = th * tw * 4 if implicit else 16 * th * tw * (p.cin + (0 if fused else p.cout)) * 4
    cb = ((chunk_mb if chunk_mb else 4096) << 20) // max(img_bytes, 1)
    cb = min(max(cb, 1), p.B)
    nchunks = cdiv(p.B, cb)
    cb = cdiv(p.B, nchunks)
    T = cb * th * tw
    vbytes = 0 if implicit else align256(16 * T * p.cin * 4)
    mbytes = align256((T + 63) * 4) + WF_DUMP_BYTES + 256 if fused else align256(16 * T * p.cout * 4)
    mask = out_mask(p.outs)
    if not fused:
        q = P(1, p.cin, p.cout, 1, T, 1, tile=p.tile, groups=16)
        inner = route(q)
        if inner.rc != OK:
            return refuse(inner.rc)
        names = ('wino_input_kernel', 'conv_fwd_dma_kernel[grouped]', 'wino_output_kernel')
        return WinoRoute(OK, 'wino', None, mask, None, cb, nchunks, T, th, tw, (), vbytes + mbytes + workspace_bytes(q), names, inner)
    variant = WF2_DEFAULT_VARIANT if variant is None else variant
    ldy, ldp = p.cout if ldy is None else ldy, p.cout if ldp is None else ldp
    small_out = p.B * p.H * p.W * max(ldy if 'y' in p.outs else 0, ldp if 'p' in p.outs else 0) * 4 < 0x80000000
    gen3 = (variant >= 32 or p.tile == 3) and small_out
    unit_m, slots = (F3_TM, 2 * NUM_CU) if gen3 else (64, NUM_CU)
    grids = []
    for b0 in range(0, p.B, cb):
        Tc = min(p.B - b0, cb) * th * tw
        tiles = cdiv(Tc, unit_m) * cdiv(p.cout, 64)
        grids.append(cdiv(tiles, NUM_XCD) * NUM_XCD if tiles < slots else slots)
    inst = mask if mask in (1, 2, 3, 5) else 7
    if gen3:
        fam, var = 'wino_fused3_kernel', (12 if implicit else 8) if p.cin == 32 else 20 if implicit and p.cout <= 32 else 4 if implicit else 0
    elif implicit:
        if not small_out:
            return refuse(ENOSUP)
        fam, var = 'wino_fused2_kernel', 13 if p.cin == 32 else 5
    elif variant >= 0 and small_out:
        fam, var = 'wino_fused2_kernel', 11 if p.cin == 32 else {0: 0, 1: 1}.get(variant, 3)
    else:
        fam, var, inst = 'wino_fused_kernel', -1, None
    name = fam + ('[implicit]' if implicit else '')
    names = ('wino_tile_table_kernel', name) if implicit else ('wino_input_kernel', name)
    return WinoRoute(OK, fam, var, mask, inst, cb, nchunks, T, th, tw, tuple(grids), vbytes + mbytes, names, None)


def output_block(cout):
    """(nx, ny) of wino_output_kernel: nx channel quads by ny tiles per workgroup; grid.y = cdiv(cout / 4, nx)."""
    n4n, nx = cout // 4, 64
    while nx > 4 and nx // 2 >= n4n:
        nx //= 2
    return nx, 256 // nx


# ================================================================================================ case tables
# name: (problem, what it is there for).  The claims are in the vocabulary of claims_of and must hold in every layout of LAYOUTS.
Case = collections.namedtuple('Case', 'p claims')
BIG = (2, 92, 92)               # 16928 pixels: more than 256 tiles of 128 rows x 2 column tiles
HUGE = (2, 128, 130)            # 33280 pixels: more than 256 tiles of 256 rows, more than 1024 tiles of 64 rows


def _dma(tile, wide, one, fast_pool):
    """The three cases of one LDS-DMA tile id.  wide: a Cout of two column tiles (the second ragged), one: pixels (B, H, W) of the mixed case,
    fast_pool: a Cout with a whole column tile and a ragged one."""
    B, H, W = one
    return {
        'dma%d-mixed' % tile: Case(P(B, 32, wide, H, W, 3, tile=tile), {'dma', 'split-mixed', 'ksplit-ragged', 'nk>=8', 'fast', 'general'}),
        'dma%d-all-ctail' % tile: Case(P(2, 40, wide, 13, 12, 3, tile=tile), {'dma', 'split-all', 'ksplit-ragged', 'ctail', 'nk>=8', 'general'}),
        'dma%d-pool' % tile: Case(P(2, 32, fast_pool, 16, 16, 3, tile=tile, outs='p'), {'dma', 'split-all', 'poolord', 'nk>=8', 'fast', 'general'}),
    }


DMA_CASES = collections.OrderedDict()
for _t, _wide, _one, _fp in ((1, 136, BIG, 160), (2, 72, BIG, 96), (3, 64, (5, 60, 60), 96), (5, 136, (1, 92, 92), 160), (6, 40, BIG, 48), (8, 136, HUGE, 160),
                             (9, 264, BIG, 288)):
    DMA_CASES.update(_dma(_t, _wide, _one, _fp))
DMA_TILE_IDS = (1, 2, 3, 5, 6, 8, 9)
DMA_CELLS = ('nk>=8', 'split-all', 'split-mixed', 'ksplit-ragged', 'ctail', 'poolord', 'fast', 'general')

# tile counts 1 .. 8 of 64x64 tiles, K of 8 slabs (two K-slices) and of 12 slabs (three): whole-tile grids of every residue mod 8 (run without
# workspace) and split grids 2, 4, .. 16 and 3, 6, .. 24 = every residue mod 8 again; y2_xcd_remap is applied to each grid separately
XCD_CASES = collections.OrderedDict(('xcd-%dx%d' % (t, s), Case(P(1, 128 * s, 64, 1, 64 * t - 5, 1, tile=3), {'dma', 'split-all', 'ksplit-even'})) for s in (2, 3) for t in range(1, 9))

GEN_CASES = collections.OrderedDict([
    ('gen-linear-split', Case(P(2, 28, 40, 11, 13, 3), {'gen', 'linear-k', 'split-all', 'nk>=8', 'chosen'})),
    ('gen-linear-unsplit', Case(P(2, 8, 24, 9, 7, 3), {'gen', 'linear-k', 'unsplit'})),
    ('gen-linear-1x1', Case(P(2, 12, 24, 9, 7, 1, tile=6), {'gen', 'linear-k', 'unsplit', 'tile6'})),
    ('gen-strided-split', Case(P(2, 32, 48, 15, 17, 3, stride=2, pad=1, tile=5), {'gen', 'strided', 'split-all', 'tile5'})),
    ('gen-strided-unsplit', Case(P(2, 16, 72, 9, 9, 3, stride=2, pad=1, tile=2), {'gen', 'strided', 'unsplit', 'tile2'})),
    ('gen-strided-1x1', Case(P(2, 64, 40, 10, 12, 1, stride=2, pad=0), {'gen', 'strided', 'unsplit'})),
    ('gen-unpadded-3x3', Case(P(2, 32, 40, 9, 10, 3, pad=0, tile=3), {'gen', 'padded', 'split-all', 'tile3'})),
    ('gen-5x5-split', Case(P(1, 12, 40, 9, 11, 5, tile=1), {'gen', 'k5', 'split-all', 'tile1'})),
    ('gen-5x5-unsplit', Case(P(1, 4, 40, 9, 11, 5), {'gen', 'k5', 'unsplit'})),
    ('gen-7x7-unsplit', Case(P(1, 4, 64, 12, 10, 7, stride=2, pad=3), {'gen', 'k7', 'unsplit'})),
    ('gen-7x7-split', Case(P(1, 8, 40, 11, 9, 7, stride=2, pad=3), {'gen', 'k7', 'split-all'})),
    ('gen-transposed-split', Case(P(2, 32, 24, 7, 6, 3, stride=2, pad=1, transposed=True, out_hw=(13, 11)), {'gen', 'transposed', 'split-all'})),
    ('gen-transposed-unsplit', Case(P(2, 16, 24, 7, 6, 3, stride=2, pad=1, transposed=True, out_hw=(14, 12), tile=3), {'gen', 'transposed', 'unsplit'})),
    ('gen-transposed-1x1', Case(P(2, 64, 32, 5, 6, 1, stride=2, pad=0, transposed=True, out_hw=(10, 11)), {'gen', 'transposed', 'unsplit'})),
])
GEN_FORMS = ('linear-k', 'strided', 'k5', 'k7', 'transposed')

WAVE_CASES = collections.OrderedDict([
    ('wave-cin48-split', Case(P(2, 48, 72, 13, 12, 3, tile=7), {'wave', 'cin%32==16', 'split-all', 'ksplit-ragged', 'general'})),
    ('wave-mixed', Case(P(2, 16, 72, 128, 130, 3, tile=7), {'wave', 'cin%32==16', 'split-mixed', 'fast', 'general'})),
    ('wave-pool', Case(P(2, 32, 96, 16, 16, 3, tile=7, outs='p'), {'wave', 'poolord', 'split-all', 'fast', 'general'})),
    ('wave-1x1-unsplit', Case(P(2, 64, 125, 9, 7, 1, tile=7), {'wave', 'unsplit'})),
    ('wave-fallback-cin40', Case(P(2, 40, 72, 13, 12, 3, tile=7), {'dma', 'wave-fallback', 'tile3', 'ctail'})),
    ('wave-fallback-strided', Case(P(2, 32, 48, 15, 17, 3, stride=2, pad=1, tile=7), {'gen', 'wave-fallback', 'tile3'})),
])

# persistent ids against the plain id of the same tile on the same operands (bit-identical by reading: the K order per accumulator is the same)
PERSIST_SHAPES = collections.OrderedDict([
    ('walk-1slab', ((2, 32, 136, 128, 130, 1), {'more-than-slots', 'one-slab'})),
    ('walk-2slabs', ((2, 64, 136, 128, 130, 1), {'more-than-slots', 'even-slabs'})),
    ('walk-3slabs', ((2, 96, 136, 128, 130, 1), {'more-than-slots', 'odd-slabs'})),
    ('few-1slab', ((2, 32, 136, 13, 12, 1), {'fewer-than-slots', 'one-slab'})),
    ('few-2slabs', ((2, 64, 136, 13, 12, 1), {'fewer-than-slots', 'even-slabs'})),
    ('few-9slabs', ((2, 32, 72, 9, 7, 3), {'fewer-than-slots', 'odd-slabs'})),
])
PERSIST_CASES = collections.OrderedDict(('p%d-%s' % (t, n), Case(P(*s, tile=t), c | {'persistent', 'unsplit'})) for t in PERSIST_OF for n, (s, c) in PERSIST_SHAPES.items())
PERSIST_CELLS = ('more-than-slots', 'fewer-than-slots', 'odd-slabs', 'even-slabs', 'one-slab')

# the register-staged kernel: (shape, outs) x tile id x layout.  Cin = 20 is VEC with the aligned layouts (forced there by id + 100) and not VEC with
# NONVEC_LAYOUTS; Cin = 6 and 13 never are.  Every non-vec problem also runs with tile = 0 (at these sizes choose_tile takes a tile the kernel has; from
# about 8256 pixels on it takes 128x32 for Cout <= 32, which dispatch_tile lacks - the library then answers Y2_ENOSUP: a known defect, see the README).
REG_SHAPES = collections.OrderedDict([
    ('3x3-cin20', ((2, 20, 72, 12, 11, 3), 'y')),
    ('3x3-cin20-pool', ((2, 20, 72, 12, 10, 3), 'yp')),
    ('3x3-cin6', ((2, 6, 20, 8, 9, 3), 'ys')),
    ('1x1-cin13', ((1, 13, 33, 5, 7, 1), 'y')),
    ('1x1-cin8-wide', ((3, 8, 136, 10, 9, 1), 'y')),
])
REG_IDS = tuple(sorted(REG_TILES))


def reg_tile_id(tid, vec):
    """The id that reaches dispatch_tile's case `tid`: + 100 for VEC operands (the plain ids 1, 2, 3, 5 would select the LDS-DMA kernel) and for 11 and 13
    (which name the persistent form first, and that refuses what is not VEC); operands that are not VEC take the plain ids otherwise."""
    return tid + 100 if vec or tid in PERSIST_OF else tid


# one case per kernel family for the epilogue forms, the mean-positive regime and deterministic mode (even H and W: pool and reorg apply)
FAMILY_CASES = collections.OrderedDict([
    ('dma', P(2, 40, 72, 12, 14, 3, tile=3)),
    ('dma-512', P(2, 64, 136, 12, 14, 3, tile=8)),
    ('wave', P(2, 48, 72, 12, 14, 3, tile=7)),
    ('persistent', P(2, 64, 72, 12, 14, 3, tile=13)),
    ('gen', P(2, 28, 40, 12, 14, 3, tile=2)),
    ('reg', P(2, 20, 72, 12, 14, 3, tile=104)),
])
OUTS = ('y', 'p', 'yp', 'ys', 'ps', 'yps', 's')
# (scale given, shift given, slope)
AFFINE = ((True, True, 0.1), (False, False, 0.1), (False, True, 0.1), (True, False, 0.1), (False, False, 1.0), (True, False, 1.0), (False, True, 1.0))

# ------------------------------------------------------------------------------------------------ refusals
# (name, problem, layout, algo, code): what the library promises to answer, touching no destination
Refusal = collections.namedtuple('Refusal', 'p layout algo rc')
REFUSALS = collections.OrderedDict([
    ('persistent+pool', Refusal(P(2, 64, 72, 12, 14, 3, tile=13, outs='p'), 'dense', 0, ENOSUP)),
    ('persistent+cin%32', Refusal(P(2, 48, 72, 12, 14, 3, tile=11), 'dense', 0, ENOSUP)),
    ('persistent+nonvec', Refusal(P(2, 64, 72, 12, 14, 3, tile=12), 'misaligned', 0, ENOSUP)),
    ('persistent+strided', Refusal(P(2, 64, 72, 12, 14, 3, tile=15, stride=2, pad=1), 'dense', 0, ENOSUP)),
    ('strided+nonvec', Refusal(P(2, 6, 20, 12, 14, 3, stride=2, pad=1), 'dense', 0, ENOSUP)),
    ('5x5+misaligned', Refusal(P(2, 8, 20, 12, 14, 5), 'misaligned', 0, ENOSUP)),
    ('strided+pool', Refusal(P(2, 32, 20, 12, 14, 3, stride=2, pad=0, outs='p'), 'dense', 0, ENOSUP)),
    ('strided+reorg', Refusal(P(2, 32, 20, 13, 15, 3, stride=2, pad=0, out_mode=1), 'dense', 0, EINVAL)),
    ('strided+512-thread-tile', Refusal(P(2, 32, 20, 12, 14, 3, stride=2, pad=1, tile=8), 'dense', 0, ENOSUP)),
    ('residual+pool', Refusal(P(2, 32, 72, 12, 14, 3, outs='p', residual=True), 'dense', 0, ENOSUP)),
    ('residual+reorg', Refusal(P(2, 32, 72, 12, 14, 3, out_mode=1, residual=True), 'dense', 0, ENOSUP)),
    ('residual+nonvec', Refusal(P(2, 6, 20, 12, 14, 3, residual=True), 'dense', 0, ENOSUP)),
    ('tile-without-kernel-dma', Refusal(P(2, 32, 72, 12, 14, 3, tile=10), 'dense', 0, ENOSUP)),
    ('tile-without-kernel-reg', Refusal(P(2, 6, 20, 12, 14, 3, tile=6), 'dense', 0, ENOSUP)),
    ('tile-without-kernel-reg-106', Refusal(P(2, 32, 72, 12, 14, 3, tile=106), 'dense', 0, ENOSUP)),
    ('tile-without-kernel-reg-wave', Refusal(P(2, 32, 72, 12, 14, 3, tile=7), 'odd-ld', 0, ENOSUP)),
    ('pool+odd-map', Refusal(P(2, 32, 72, 13, 14, 3, outs='p'), 'dense', 0, EINVAL)),
    ('reorg+odd-map', Refusal(P(2, 32, 72, 12, 13, 3, out_mode=1), 'dense', 0, EINVAL)),
    ('no-destination', Refusal(P(2, 32, 72, 12, 14, 3, outs=''), 'dense', 0, EINVAL)),
    ('9x9', Refusal(P(2, 32, 72, 12, 14, 9), 'dense', 0, ENOSUP)),
    ('grouped-16+cin%4', Refusal(P(2, 6, 20, 12, 14, 3), 'dense', 1, ENOSUP)),
    ('grouped-16+odd-ld', Refusal(P(2, 8, 20, 12, 14, 3), 'odd-ld', 1, ENOSUP)),
    ('grouped-16+tile-without-kernel', Refusal(P(2, 32, 72, 12, 14, 3, tile=4), 'dense', 1, ENOSUP)),
    ('grouped-16+persistent', Refusal(P(2, 32, 72, 12, 14, 3, tile=13), 'dense', 1, ENOSUP)),
    ('grouped-16+reorg', Refusal(P(2, 32, 72, 12, 14, 3, out_mode=1), 'dense', 1, ENOSUP)),
    ('grouped-16+residual', Refusal(P(2, 32, 72, 12, 14, 3, residual=True), 'dense', 1, ENOSUP)),
    ('grouped-36+pool', Refusal(P(2, 32, 72, 12, 14, 3, outs='yp'), 'dense', 6, ENOSUP)),
    ('grouped-36+stats', Refusal(P(2, 32, 72, 12, 14, 3, outs='ys'), 'dense', 6, ENOSUP)),
    ('grouped-36+pool-only', Refusal(P(2, 32, 72, 12, 14, 3, outs='p'), 'dense', 6, ENOSUP)),
    ('grouped-36+tile-without-kernel', Refusal(P(2, 32, 72, 12, 14, 3, tile=21), 'dense', 6, ENOSUP)),
    ('fused+cin%32', Refusal(P(2, 48, 72, 12, 14, 3), 'dense', 2, ENOSUP)),
    ('implicit+cin%32', Refusal(P(2, 48, 72, 12, 14, 3), 'dense', 3, ENOSUP)),
    ('implicit+cin<32', Refusal(P(2, 16, 72, 12, 14, 3), 'dense', 3, ENOSUP)),
    ('winograd+1x1', Refusal(P(2, 32, 72, 12, 14, 1), 'dense', 1, ENOSUP)),
    ('winograd+pool+odd-map', Refusal(P(2, 32, 72, 13, 14, 3, outs='yp'), 'dense', 2, EINVAL)),
])


def refusal_code(r):
    pad, off = dict(LAYOUTS, **NONVEC_LAYOUTS)[r.layout]
    return route(r.p, pad, off).rc if r.algo == 0 else wino_route(r.p, r.algo, pad, off).rc


# ------------------------------------------------------------------------------------------------ Winograd
# family x variant: (algo, tile, Y2_WF_VARIANT or None, Cin, Cout)
WINO_VARIANTS = collections.OrderedDict([
    ('three-kernel', (1, 0, None, 32, 72)),
    ('gen1', (2, 0, -1, 64, 72)),
    ('gen2-v3', (2, 0, None, 64, 72)),
    ('gen2-v5', (3, 0, None, 64, 72)),
    ('gen2-v11', (2, 0, None, 32, 72)),
    ('gen2-v13', (3, 0, None, 32, 72)),
    ('gen3-v0', (2, 3, None, 64, 72)),
    ('gen3-v4', (3, 3, None, 64, 72)),
    ('gen3-v8', (2, 3, None, 32, 72)),
    ('gen3-v12', (3, 3, None, 32, 72)),
    ('gen3-v20', (3, 3, None, 64, 20)),
])
WINO_FAMILY = {'three-kernel': ('wino', None), 'gen1': ('wino_fused_kernel', -1), 'gen2-v3': ('wino_fused2_kernel', 3), 'gen2-v5': ('wino_fused2_kernel', 5),
               'gen2-v11': ('wino_fused2_kernel', 11), 'gen2-v13': ('wino_fused2_kernel', 13), 'gen3-v0': ('wino_fused3_kernel', 0),
               'gen3-v4': ('wino_fused3_kernel', 4), 'gen3-v8': ('wino_fused3_kernel', 8), 'gen3-v12': ('wino_fused3_kernel', 12), 'gen3-v20': ('wino_fused3_kernel', 20)}
WINO_MAPS = collections.OrderedDict([('even', (3, 12, 14)), ('ragged', (2, 13, 11))])      # (B, H, W): 'ragged' has a last tile row and column of one pixel
MASKS = {1: 'y', 2: 'p', 3: 'yp', 4: 's', 5: 'ys', 6: 'ps', 7: 'yps'}


def wino_case(variant, where, mask):
    algo, tile, env, cin, cout = WINO_VARIANTS[variant]
    B, H, W = WINO_MAPS[where]
    return P(B, cin, cout, H, W, 3, tile=tile, outs=MASKS[mask]), algo, env


def wino_masks(where):
    return (1, 4, 5) if where == 'ragged' else tuple(MASKS)         # a pooled output needs an even map


# walks of the persistent fused kernels: more 64 x 64 units than 256 workgroups (generations 1, 2), more 32 x 64 units than 512 (generation 3)
WINO_WALKS = collections.OrderedDict([('gen1', (9, 64, 136, 52, 50)), ('gen2-v3', (9, 64, 136, 52, 50)), ('gen2-v13', (9, 32, 136, 52, 50)), ('gen3-v0', (9, 64, 136, 52, 50)),
                                      ('gen3-v12', (9, 32, 136, 52, 50))])
# wino_output_kernel: Cout below / equal to / above 64 and 256 (its nx and grid.y)
WINO_OUTPUT_COUTS = (60, 64, 68, 252, 256, 260)
# the grouped GEMMs: (algo, B, Cin, Cout, H, W) - split needs 8 slabs, Cin >= 256
GROUPED_CASES = collections.OrderedDict([
    ('g16-split', (1, 2, 256, 72, 13, 11)), ('g16-unsplit', (1, 2, 64, 72, 13, 11)), ('g16-ctail', (1, 2, 40, 72, 12, 14)),
    ('g36-split', (6, 2, 256, 72, 13, 11)), ('g36-unsplit', (6, 2, 64, 72, 13, 11)), ('g36-mosaic', (6, 9, 32, 40, 5, 6)),
])
# batch chunks under Y2_WINO_CHUNK_MB = 1: (algo, tile, B, Cin, Cout, H, W) -> two or more chunks, the last one shorter
CHUNK_MB = 1
CHUNK_CASES = collections.OrderedDict([('three-kernel', (1, 0, 5, 64, 72, 14, 12)), ('fused', (2, 0, 5, 128, 72, 14, 12)), ('fused-gen3', (2, 3, 5, 128, 72, 14, 12))])      # (an implicit launch's chunk holds a tile table only: no small batch exceeds 1 MB)
