"""Shared by test_fixed_cpu.py and test_gpu_fixed.py: the numpy restatement of y2_fixed_images' contract (include/yolo2_hip.h) - written from the
header, independently of csrc/fixed.h -, an fp64 Keys cubic convolution, and the seeded case groups - one launch each - at the smallest shapes where
each path can go wrong."""
import numpy as np

import collate_cases as cc
import rotate_cases as rc

SENTINEL = np.float32(-7.0)
PAD = 64          # sentinel floats on either side of `out` (a multiple of 4: the buffer's alignment is the output's)

f32 = np.float32


# ---- the recipe, restated

def cubic_coeffs(a):
    """float32 [.., 4]: the four coefficients of the fractions a / 32 (int array), every operation rounded to fp32."""
    A = f32(-0.75)
    t = a.astype(f32) * (f32(1) / f32(32))
    u, v = t + f32(1), f32(1) - t
    c0 = ((A * u - f32(5) * A) * u + f32(8) * A) * u - f32(4) * A
    c1 = ((A + f32(2)) * t - (A + f32(3))) * t * t + f32(1)
    c2 = ((A + f32(2)) * v - (A + f32(3))) * v * v + f32(1)
    c3 = f32(1) - c0 - c1 - c2
    out = np.stack([c0, c1, c2, c3], -1)
    assert out.dtype == np.float32
    return out


def weight_table():
    """int64 [32 (ay), 32 (ax), 4 (row), 4 (column)]: the corrected integer weights of every pair of fractions."""
    c = cubic_coeffs(np.arange(32))
    prod = (c[:, None, :, None] * c[None, :, None, :]) * f32(32768)
    assert prod.dtype == np.float32
    w = np.clip(np.rint(prod), -32768, 32767).astype(np.int64)
    for ay in range(32):
        for ax in range(32):
            t = w[ay, ax]
            d = int(t.sum()) - 32768
            lo = hi = (1, 1)
            for at in ((1, 1), (1, 2), (2, 1), (2, 2)):
                if t[at] < t[lo]:
                    lo = at
                elif t[at] > t[hi]:
                    hi = at
            if d < 0:
                t[hi] -= d
            elif d > 0:
                t[lo] -= d
    return w


_TABLE = []


def table():
    if not _TABLE:
        _TABLE.append(weight_table())
    return _TABLE[0]


def levels(img, A, mode, H, W):
    """int64 [H, W, 3] in source channel order: the level of every output pixel."""
    X, Y = rc.positions(A, H, W)
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    ax, ay = X & 31, Y & 31
    if mode == 0:
        ax, ay = ax[..., None], ay[..., None]
        return (rc.taps(img, sy, sx, 0, 0) * (32 - ax) * (32 - ay) + rc.taps(img, sy, sx + 1, 0, 0) * ax * (32 - ay)
                + rc.taps(img, sy + 1, sx, 0, 0) * (32 - ax) * ay + rc.taps(img, sy + 1, sx + 1, 0, 0) * ax * ay + 512) >> 10
    w = table()[ay, ax]          # [H, W, 4, 4]
    acc = np.zeros((H, W, 3), np.int64)
    for i in range(4):
        for j in range(4):
            acc += rc.taps(img, sy - 1 + i, sx - 1 + j, 0, 0) * w[..., i, j, None]
    return np.clip((acc + 16384) >> 15, 0, 255)


def all_outside(img, A, mode, H, W):
    """bool [H, W]: every tap of the pixel lies outside the source."""
    sh, sw = img.shape[:2]
    X, Y = rc.positions(A, H, W)
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    lo, hi = (0, 1) if mode == 0 else (-1, 2)
    cols_out = (sx + hi < 0) | (sx + lo >= sw)
    rows_out = (sy + hi < 0) | (sy + lo >= sh)
    return cols_out | rows_out


def keys64(img, A, H, W):
    """fp64 Keys cubic convolution (a = -0.75, zero outside the image) at the QUANTISED positions sx + ax / 32, sy + ay / 32, clamped to 0 .. 255:
    float64 [H, W, 3]."""
    X, Y = rc.positions(A, H, W)
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    tx, ty = (X & 31) / 32.0, (Y & 31) / 32.0

    def kernel(d):
        d, a = np.abs(d), -0.75
        return np.where(d <= 1, ((a + 2) * d - (a + 3)) * d * d + 1, np.where(d < 2, ((a * d - 5 * a) * d + 8 * a) * d - 4 * a, 0.0))
    acc = np.zeros((H, W, 3), np.float64)
    for i in range(-1, 3):
        for j in range(-1, 3):
            acc += rc.taps(img, sy + i, sx + j, 0, 0) * (kernel(ty - i) * kernel(tx - j))[..., None]
    return np.clip(acc, 0, 255)


# ---- the case groups

def scale_map(sh, sw, H, W):
    """(inverse matrix, mode) of the reference's rule for a sh x sw source and an H x W canvas, through numpy's general inversion."""
    scale = H / sh if sh / sw > H / W else W / sw
    return rc.inverse(np.array([[scale, 0, 0], [0, scale, 0]], np.float64)), 0 if scale < 1 else 1


def make_group(rng, items, H, W, flags=1, lut=None, misalign=0):
    """items: (image, inverse matrix, mode, source row padding).  The sources are packed by collate_cases.pack (odd byte offsets, random bytes in every
    gap and behind the rows).  misalign: `out` starts that many floats behind a 16-byte boundary."""
    src, offset, g8 = cc.pack(rng, [(img, None, 0, rowpad) for img, _, _, rowpad in items])
    geom = np.ascontiguousarray(g8[:, [0, 1, 2, 2]])
    geom[:, 3] = [mode for _, _, mode, _ in items]
    return dict(src=src, offset=offset, geom=geom.reshape(-1, 4), inv=np.array([it[1] for it in items], np.float64).reshape(-1, 6), H=H, W=W, flags=flags,
                lut=rc.reference_lut() if lut is None else lut, misalign=misalign)


def groups():
    """name -> group (make_group); every group is one launch."""
    rng = np.random.RandomState(41)
    im = lambda h, w: rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    item = lambda h, w, H, W, pad=0: (im(h, w),) + scale_map(h, w, H, W) + (pad,)
    g = {}
    # source widths and heights 1 .. 5 on a 12 x 12 canvas: every cubic tap pattern against the border (all upscales: mode 1); then the same sources
    # in mode 0 with the same maps
    small = [item(h, w, 12, 12) for h in (1, 2, 3, 4, 5) for w in (1, 2, 3, 4, 5)]
    g['tiny_cubic'] = make_group(rng, small, 12, 12)
    g['tiny_linear'] = make_group(rng, [(img, A, 0, pad) for img, A, _, pad in small], 12, 12, flags=0)
    # a wide and a tall source (one for each branch of the scale rule), shrinking (mode 0) and growing (mode 1), scale == 1 exactly (mode 1: a copy);
    # more than one row block; padded rows; a batch that mixes modes
    g['scales'] = make_group(rng, [item(50, 90, 40, 40), item(90, 50, 40, 40, 5), item(13, 30, 40, 40), item(30, 13, 40, 40, 2), item(40, 25, 40, 40),
                                   item(17, 40, 40, 40, 7), item(40, 40, 40, 40)], 40, 40)
    # a general rotation in each mode, the image partly off the canvas
    rot = lambda h, w, angle, shift, mode: (im(h, w), rc.rotation(h, w, angle, shift)[0], mode, 0)
    g['rotations'] = make_group(rng, [rot(30, 37, 30, (0, 0), 0), rot(30, 37, 30, (0, 0), 1), rot(21, 33, -5, (-9.5, 4.25), 1), rot(21, 33, 175, (6, -7), 0)], 36, 44,
                                lut=cc.random_lut())
    # W % 4 != 0 (the scalar stores and the 1-3 pixel tail), BGR2RGB off, a table that differs per plane
    g['w30'] = make_group(rng, [item(50, 33, 21, 30), item(9, 41, 21, 30), item(10, 14, 21, 30, 3), item(21, 30, 21, 30)], 21, 30, flags=0, lut=cc.random_lut(6))
    g['w1'] = make_group(rng, [item(5, 3, 19, 1), item(40, 3, 19, 1), item(3, 1, 19, 1)], 19, 1, lut=cc.random_lut(7))
    # W % 4 == 0 with `out` one float off a 16-byte boundary: the scalar stores again
    g['unaligned'] = make_group(rng, [item(23, 31, 20, 28), item(60, 31, 20, 28), item(10, 14, 20, 28)], 20, 28, misalign=1, lut=cc.random_lut(8))
    g['b0'] = make_group(rng, [], 16, 16)
    return g


GROUP_NAMES = ['tiny_cubic', 'tiny_linear', 'scales', 'rotations', 'w30', 'w1', 'unaligned', 'b0']


def source(group, b):
    g = group['geom'][b]
    return cc.image_view(group['src'], int(group['offset'][b]), (g[0], g[1], g[2]))


def numel(group):
    return len(group['geom']) * 3 * group['H'] * group['W']


def new_out(group):
    """The sentinel-filled output buffer and the index of out[0] in it."""
    return np.full(numel(group) + 2 * PAD, SENTINEL, np.float32), PAD + group['misalign']


def restate(group):
    """The whole output buffer as the contract says the launch leaves it."""
    buf, at = new_out(group)
    H, W, lut = group['H'], group['W'], group['lut']
    out = buf[at:at + numel(group)].reshape(-1, 3, H, W)
    for b, g in enumerate(group['geom']):
        lv = levels(source(group, b), group['inv'][b], int(g[3]), H, W)
        for c in range(3):
            out[b, c] = lut[c][lv[..., 2 - c if group['flags'] & 1 else c]]
    return buf


def host(group, buf=None, **change):
    """y2_fixed_images_host into a sentinel-filled buffer (or `buf`); `change` replaces tables of the group.  Returns (rc, buffer)."""
    import _hip
    g = dict(group, **change)
    at = PAD + g['misalign']
    if buf is None:
        buf = new_out(g)[0]
    arrays = [np.ascontiguousarray(g[k]) for k in ('src', 'offset', 'geom', 'inv', 'lut')]
    p = lambda a: a.ctypes.data if a.size else None
    code = _hip.lib().y2_fixed_images_host(p(arrays[0]), p(arrays[1]), p(arrays[2]), p(arrays[3]), p(arrays[4]), len(g['geom']), g['H'], g['W'], g['flags'],
                                           buf[at:].ctypes.data)
    return code, buf


# ---- generated pictures for the workflow tests

def picture(rng, h, w):
    """A BGR uint8 [h, w, 3] picture with structure at several scales: smooth gradients, rectangles and noise."""
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(255 * y / max(h - 1, 1)), (255 * x / max(w - 1, 1)), 128 + 100 * np.sin(x / 5.0) * np.cos(y / 7.0)], -1)
    for _ in range(4):
        y0, x0 = rng.randint(0, h), rng.randint(0, w)
        img[y0:y0 + rng.randint(2, h), x0:x0 + rng.randint(2, w)] = rng.randint(0, 256, 3)
    return np.clip(img + rng.normal(0, 8, img.shape), 0, 255).astype(np.uint8)
