"""Case table of the fused BatchNorm-backward + 4x4-tile transform tests (tests/test_gpu_bnwino6.py runs it on the GPU, tests/test_bnwino6_cases.py
proves on the CPU that it reaches what it claims), the Python mirror of what decides the path of one y2_bn_act_bwd_wino6 call:

    csrc/common.h    wino6_grid (tests/wgrad_cases.py holds that mirror; it is reused here)
    csrc/train.hip   act_grid, and bn_act_bwd_impl with dz == NULL and a park buffer: vector or scalar pass 1, where its partial sums go

and a plain fp64 statement of the layout contract of the two operands the call writes (v6_m6_reference).

A route has four fields: the grid form ('per-image', 'tall': gx == 1 and wide == 0, 'mosaic': gx > 1), whether the mosaic has phantom images
(gx * gy > B), the pass-1 form ('vector' / 'scalar') and the pass-1 sum path ('atomics': at most 16 workgroups; 'parked-v6:N' / 'parked-m6:N':
per-workgroup partial rows parked in the transform buffer and added by bn_bwd_block_reduce_kernel with N = 1 / 4 / 16 row slices; 'atomics>16': a
larger grid whose park buffer is one float off 16-byte alignment, or too small)."""
import collections
import math

import numpy as np

import wgrad_cases as wc

NUM_CU = 256                    # Y2_NUM_CU (csrc/common.h)
THREADS = 256                   # workgroup size of the streaming kernels and of bn_bwd_wino6_kernel
ITEMS = 8                       # act_grid: items per thread the grid is sized for
WG_PER_CU = 8                   # act_grid: cap
PARK_MIN_GRID = 16              # bn_act_bwd_impl parks only with grid > 16
SLICE_4, SLICE_16 = 64, 512     # grid >= 64: 4 row slices of bn_bwd_block_reduce_kernel, >= 512: 16
OK, EINVAL, EALIGN, ENOSUP = 0, -1, -2, -3

Case = collections.namedtuple('Case', 'B H W C ldz fpad foff dz out has_bn slope affine park_off cin')
Case.__new__.__defaults__ = (0, 0, 0, 'null', 'both', 1, 0.1, True, 0, 8)
# ldz:      floats added to the pixel stride of z (ldz = C + ldz)
# fpad/foff: dy is the channel window foff .. foff + C of rows of ldf = foff + C + fpad floats
# dz:       'null' | 'dense' | 'window' (ldd = C + 4)
# out:      'v6' | 'm6' | 'both'
# affine:   scale / shift given (False: NULL, has_bn = 0 only)
# park_off: 1 = the buffer pass 1 parks in (v6, or m6 without v6) starts one float off 16-byte alignment
# cin:      input channels of the 3x3 convolution whose gradients the consumers compute (0: sums, dz, V6 and M6 only)

Route = collections.namedtuple('Route', 'form phantom pass1 sums grid items T th tw tall wide gx gy')


def act_grid(total, Cg):
    """csrc/train.hip: workgroups of 256 threads sized for 8 items per thread, at most 8 per CU, total thread count a multiple of Cg."""
    unit = Cg // math.gcd(THREADS, Cg)
    want = min(max((total + THREADS * ITEMS - 1) // (THREADS * ITEMS), 1), NUM_CU * WG_PER_CU)
    return (want + unit - 1) // unit * unit


def strides(c):
    """(ldz, ldf, ldd) of a case."""
    return c.C + c.ldz, c.foff + c.C + c.fpad, {'null': 0, 'dense': c.C, 'window': c.C + 4}[c.dz]


def route(c, tall_allowed=True):
    ldz, ldf, _ = strides(c)
    g = wc.wino6_grid(c.B, c.H, c.W) if tall_allowed else wc.Wino6Grid(wc.cdiv(c.H, 4), wc.cdiv(c.W, 4), 0, 0, 1, c.B * wc.cdiv(c.H, 4) * wc.cdiv(c.W, 4))
    form = 'per-image' if not g.tall else ('mosaic' if g.gx > 1 else 'tall')
    assert bool(g.wide) == (g.gx > 1)
    gy = wc.cdiv(c.B, g.gx)
    # bn_act_bwd_impl, dz == NULL, one un-pooled gradient source (the operands of the tests are 16-byte aligned)
    vec = c.C % 4 == 0 and ldz % 4 == 0 and ldf % 4 == 0 and c.foff % 4 == 0
    Cg = c.C // 4 if vec else c.C
    npix = c.B * c.H * c.W
    grid = act_grid(npix * Cg, Cg)
    pstep = grid * THREADS // Cg
    items = wc.cdiv(npix, pstep)
    park = 'v6' if c.out in ('v6', 'both') else 'm6'
    if grid <= PARK_MIN_GRID:
        sums = 'atomics'
    elif c.park_off or grid * 2 * c.C > 36 * g.T * c.C:
        sums = 'atomics>16'
    else:
        sums = 'parked-%s:%d' % (park, 16 if grid >= SLICE_16 else (4 if grid >= SLICE_4 else 1))
    return Route(form, form != 'per-image' and g.gx * gy > c.B, 'vector' if vec else 'scalar', sums, grid, items, g.T, g.th, g.tw, g.tall, g.wide, g.gx, gy)


def refusal(c, deterministic=False):
    """Return code of y2_bn_act_bwd_wino6 for the strides and pointers of c (every refusing test of the entry point and of bn_act_bwd_impl, in order)."""
    ldz, ldf, ldd = strides(c)
    if c.out not in ('v6', 'm6', 'both') or min(c.B, c.H, c.W, c.C) <= 0 or ldz < c.C or ldf < c.foff + c.C:
        return EINVAL
    if c.dz != 'null' and ldd < c.C:
        return EINVAL
    if deterministic:
        return ENOSUP
    if c.has_bn < 0 or c.has_bn > 2:
        return EINVAL
    return OK


# ------------------------------------------------------------------------------------------------ the layout contract
# Toom-Cook F(4,3) / F(3,4) on the points 0, 1, -1, 2, -1/2, infinity: the input transform B^T (6 x 6) and the transform G (6 x 4) of the 4-tap operand.
BT = np.array([[1, 1.5, -2, -1.5, 1, 0], [0, -1, -2.5, -0.5, 1, 0], [0, 1, 0.5, -2.5, 1, 0], [0, -0.5, -1, 0.5, 1, 0], [0, 2, -1, -2, 1, 0], [0, 1, 1.5, -2, -1.5, 1]], dtype=np.float64)
GM = np.array([[1, 0, 0, 0], [-1 / 3, -1 / 3, -1 / 3, -1 / 3], [1 / 3, -1 / 3, 1 / 3, -1 / 3], [1 / 15, 2 / 15, 4 / 15, 8 / 15], [-16 / 15, 8 / 15, -4 / 15, 2 / 15], [0, 0, 0, 1]],
              dtype=np.float64)


def patches(d, r):
    """d [B, H, W, C] -> [T, 6, 6, C]: the 6x6 patch at (4 ty - 1, 4 tx - 1) of every tile of route r's grid, tile t = (b * th + ty) * tw + tx on the per-image
    grid and ty * tw + tx on the mosaic - gy rows of gx images, image b = by * gx + bx at (by * (H + 1), bx * (W + 1)), one zero line between neighbours.
    Whatever is no pixel of an image (the separators, outside the mosaic, the places of images B .. gx * gy - 1) is zero."""
    B, H, W, C = d.shape
    if r.form == 'per-image':
        canvas = np.zeros((B, 4 * r.th + 2, 4 * r.tw + 2, C), dtype=d.dtype)
        canvas[:, 1:H + 1, 1:W + 1] = d
    else:
        canvas = np.zeros((1, 4 * r.th + 2, 4 * r.tw + 2, C), dtype=d.dtype)
        for b in range(B):
            by, bx = divmod(b, r.gx)
            y0, x0 = by * (H + 1) + 1, bx * (W + 1) + 1
            canvas[0, y0:y0 + H, x0:x0 + W] = d[b]
    out = np.empty((canvas.shape[0], r.th, r.tw, 6, 6, C), dtype=d.dtype)
    for ty in range(r.th):
        for tx in range(r.tw):
            out[:, ty, tx] = canvas[:, 4 * ty:4 * ty + 6, 4 * tx:4 * tx + 6]
    out = out.reshape(-1, 6, 6, C)
    assert out.shape[0] == r.T
    return out


def v6_m6_reference(d, r, dtype=np.float64):
    """The two operands y2_bn_act_bwd_wino6 writes, from the gradient d [B, H, W, C]: V6[6u + v][t][c] = (B^T p B)[u][v] on the 6x6 patch p of tile t and
    M6[6u + v][t][c] = (G q G^T)[u][v] on the 4x4 tile q = p[1:5, 1:5] inside it; each [36, T, C] in `dtype`."""
    p = patches(np.asarray(d, dtype=dtype), r)
    bt, gm = BT.astype(dtype), GM.astype(dtype)
    return _two_sided(bt, p), _two_sided(gm, p[:, 1:5, 1:5])


def _two_sided(m, p):
    """[36, T, C]: (m q m^T)[u][v] at row 6u + v for every q = p[t, :, :, c]."""
    rows = np.tensordot(m, p, axes=(1, 1))                          # [u, t, j, c]
    both = np.tensordot(m, rows, axes=(1, 2))                       # [v, u, t, c]
    return np.ascontiguousarray(both.transpose(1, 0, 2, 3)).reshape(36, p.shape[0], p.shape[3])


def structural_zeros(B, H, W, r):
    """Boolean [36, T] each for V6 and M6: positions every contributing pixel of which is no pixel of an image - there the kernel must write +0.0 or -0.0."""
    p = patches(np.ones((B, H, W, 1)), r)
    return _two_sided(np.abs(BT), p)[:, :, 0] == 0, _two_sided(np.abs(GM), p[:, 1:5, 1:5])[:, :, 0] == 0


# ------------------------------------------------------------------------------------------------ the table
# name: Case(B, H, W, C, ...).  Defaults: dense z and dy, no dz, both operands, batch statistics, slope 0.1, 8 input channels for the consumers.
CASES = {
    # ---- grid forms and sizes (all on the atomics path: at most 16 workgroups)
    'b1-1x1': Case(1, 1, 1, 8, dz='dense', has_bn=2),                                # (batch statistics need more than one value per channel)
    'b1-5x7': Case(1, 5, 7, 8, dz='window'),
    'b3-1x1-mosaic-phantom': Case(3, 1, 1, 8, dz='dense'),
    'b2-3x2': Case(2, 3, 2, 12, dz='window', has_bn=2),
    'b2-8x8': Case(2, 8, 8, 8, dz='dense'),
    'b2-4x12-v6': Case(2, 4, 12, 16, out='v6', dz='dense', slope=0.0),
    'b3-5x4-tall': Case(3, 5, 4, 8, dz='dense', ldz=4),
    'b4-6x6-tall-m6': Case(4, 6, 6, 8, out='m6', dz='window', slope=1.0),
    'b2-7x9-mosaic': Case(2, 7, 9, 16, dz='dense', fpad=4, foff=4),
    'b3-2x3-tall': Case(3, 2, 3, 8, dz='dense'),
    'b5-6x5-mosaic-phantom': Case(5, 6, 5, 8, dz='window', has_bn=2, slope=0.0),
    'b9-13x11-tall': Case(9, 13, 11, 12, dz='dense', has_bn=0, affine=False),
    'b7-10x14-tall': Case(7, 10, 14, 8, dz='dense', slope=1.0, has_bn=2),
    # ---- scalar pass 1: C = 6 (no consumers), and C % 4 == 0 with one stride or offset that is no multiple of 4
    'c6-b2-7x9': Case(2, 7, 9, 6, dz='dense', cin=0),
    'c6-b9-13x13-windows': Case(9, 13, 13, 6, dz='window', ldz=1, fpad=2, foff=3, cin=0, has_bn=2),
    'c6-b1-8x8-bn0': Case(1, 8, 8, 6, dz='dense', has_bn=0, affine=False, cin=0, out='m6'),
    'scalar-ldz': Case(3, 5, 4, 8, ldz=1, dz='dense'),
    'scalar-foff': Case(2, 7, 9, 8, fpad=1, foff=3),
    'scalar-ldf': Case(2, 8, 8, 8, fpad=2, dz='window'),
    # ---- the production mosaics, and the sum paths through the park buffer
    'b9-13x13-c32': Case(9, 13, 13, 32, dz='dense'),                                 # 3 x 3 images, atomics
    'b11-13x13-c32-phantom': Case(11, 13, 13, 32, fpad=8, foff=8, ldz=4),            # 4 x 3 places for 11 images, atomics
    'grid16': Case(12, 13, 13, 64, cin=4),                                         # 16 workgroups: the last size on the atomics
    'grid17': Case(11, 14, 14, 64, cin=4),                                         # 17: the first that parks
    'park1-b9-13x13-c128': Case(9, 13, 13, 128, dz='dense'),
    'park1-m6-b11-13x13-c128': Case(11, 13, 13, 128, out='m6', has_bn=2),
    'park1-scalar': Case(9, 13, 13, 24, foff=2, fpad=2, cin=4),
    'park4-b6-26x26-c128': Case(6, 26, 26, 128, cin=4),                              # exactly 64 workgroups
    'park4-m6-dz-window': Case(10, 29, 30, 64, out='m6', dz='window', cin=4, has_bn=0),
    'misaligned-park': Case(9, 13, 13, 128, park_off=1),                             # v6 one float off: more than 16 workgroups on the atomics
    'misaligned-park-m6': Case(11, 13, 13, 128, out='m6', park_off=1, cin=0),
    'park16-b16-26x26-c400': Case(16, 26, 26, 400, cin=0),                           # 550 workgroups; sums, V6 and M6 only
}
MEANPOS = ('b9-13x13-c32', 'park1-b9-13x13-c128')
CHILD = 'b9-13x13-c32'          # the case the Y2_WINO6_TALL=0 child process runs on the per-image grid

# what the table must reach (tests/test_bnwino6_cases.py): name -> predicate over (Case, Route)
REQUIRED = collections.OrderedDict([
    ('per-image B == 1', lambda c, r: r.form == 'per-image' and c.B == 1),
    ('per-image B > 1', lambda c, r: r.form == 'per-image' and c.B > 1),
    ('tall', lambda c, r: r.form == 'tall' and not r.phantom),
    ('mosaic without phantom images', lambda c, r: r.form == 'mosaic' and not r.phantom),
    ('mosaic with phantom images', lambda c, r: r.form == 'mosaic' and r.phantom),
    ('1x1', lambda c, r: (c.H, c.W) == (1, 1)),
    ('H < 4', lambda c, r: c.H < 4 and c.H * c.W > 1),
    ('W < 4', lambda c, r: c.W < 4 and c.H * c.W > 1),
    ('13x13 B = 9', lambda c, r: (c.B, c.H, c.W) == (9, 13, 13) and r.form == 'mosaic' and not r.phantom),
    ('13x13 B = 11', lambda c, r: (c.B, c.H, c.W) == (11, 13, 13) and r.form == 'mosaic' and r.phantom),
    ('T * C a multiple of 256', lambda c, r: r.T * c.C % THREADS == 0),
    ('T * C no multiple of 256, more than one workgroup', lambda c, r: r.T * c.C % THREADS != 0 and r.T * c.C > THREADS),
    ('C % 4 == 0', lambda c, r: c.C % 4 == 0),
    ('C = 6', lambda c, r: c.C == 6),
    ('ldz > C', lambda c, r: c.ldz > 0),
    ('dy window, 4-aligned', lambda c, r: c.foff > 0 and c.foff % 4 == 0 and c.fpad % 4 == 0 and r.pass1 == 'vector'),
    ('dy window, unaligned', lambda c, r: c.foff % 4 != 0 and r.pass1 == 'scalar'),
    ('scalar by ldz alone', lambda c, r: c.C % 4 == 0 and c.ldz % 4 != 0 and c.foff % 4 == 0 and c.fpad % 4 == 0),
    ('scalar by foff alone', lambda c, r: c.C % 4 == 0 and c.ldz % 4 == 0 and c.foff % 4 != 0 and (c.foff + c.fpad) % 4 == 0),
    ('scalar by ldf alone', lambda c, r: c.C % 4 == 0 and c.ldz % 4 == 0 and c.foff % 4 == 0 and c.fpad % 4 != 0),
    ('dz NULL', lambda c, r: c.dz == 'null'),
    ('dz dense', lambda c, r: c.dz == 'dense'),
    ('dz window', lambda c, r: c.dz == 'window'),
    ('v6 only', lambda c, r: c.out == 'v6'),
    ('m6 only', lambda c, r: c.out == 'm6'),
    ('v6 and m6', lambda c, r: c.out == 'both'),
    ('has_bn 0', lambda c, r: c.has_bn == 0 and c.affine),
    ('has_bn 0, scale / shift NULL', lambda c, r: c.has_bn == 0 and not c.affine),
    ('has_bn 1', lambda c, r: c.has_bn == 1),
    ('has_bn 2', lambda c, r: c.has_bn == 2),
    ('slope 0.1', lambda c, r: c.slope == 0.1),
    ('slope 0', lambda c, r: c.slope == 0.0),
    ('slope 1', lambda c, r: c.slope == 1.0),
    ('vector pass 1', lambda c, r: r.pass1 == 'vector'),
    ('scalar pass 1', lambda c, r: r.pass1 == 'scalar'),
    ('atomics', lambda c, r: r.sums == 'atomics'),
    ('atomics at 16 workgroups', lambda c, r: r.sums == 'atomics' and r.grid == PARK_MIN_GRID),
    ('parked at 17 workgroups', lambda c, r: r.sums.startswith('parked') and r.grid == PARK_MIN_GRID + 1),
    ('parked in v6, 1 slice', lambda c, r: r.sums == 'parked-v6:1'),
    ('parked in v6, 4 slices', lambda c, r: r.sums == 'parked-v6:4'),
    ('parked in v6, 16 slices', lambda c, r: r.sums == 'parked-v6:16'),
    ('parked at exactly 64 workgroups', lambda c, r: r.sums.endswith(':4') and r.grid == SLICE_4),
    ('parked in m6 because v6 is NULL', lambda c, r: r.sums.startswith('parked-m6')),
    ('parked, scalar pass 1', lambda c, r: r.sums.startswith('parked') and r.pass1 == 'scalar'),
    ('atomics>16 by misalignment', lambda c, r: r.sums == 'atomics>16' and c.park_off == 1),
    ('atomics>16 by misalignment of m6', lambda c, r: r.sums == 'atomics>16' and c.park_off == 1 and c.out == 'm6'),
] + [('H %% 4 == %d' % k, (lambda k: lambda c, r: c.H % 4 == k and c.H >= 4)(k)) for k in range(4)]
  + [('W %% 4 == %d' % k, (lambda k: lambda c, r: c.W % 4 == k and c.W >= 4)(k)) for k in range(4)]
  + [('mosaic or tall, (H + 1) %% 4 == %d' % k, (lambda k: lambda c, r: r.form != 'per-image' and (c.H + 1) % 4 == k)(k)) for k in (0, 2, 3)]
  + [('mosaic, (W + 1) %% 4 == %d' % k, (lambda k: lambda c, r: r.form == 'mosaic' and (c.W + 1) % 4 == k)(k)) for k in (2, 3)])


def reached(cases=None):
    """Names of REQUIRED that some case of `cases` reaches."""
    cases = CASES if cases is None else cases
    routes = [(c, route(c)) for c in cases.values()]
    return {name for name, pred in REQUIRED.items() if any(pred(c, r) for c, r in routes)}
