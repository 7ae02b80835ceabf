"""Shared by test_rotate_cpu.py and test_gpu_rotate.py: the numpy restatement of y2_warp_affine_images' resampling contract (include/yolo2_hip.h),
an fp64 bilinear interpolation with a constant border, and the case groups - one launch each - at the smallest shapes where each path can go wrong."""
import configparser
import math
import random

import numpy as np

import collate_cases as cc

SENTINEL = np.uint8(0xA5)
PAD = 64          # sentinel bytes on either side of the destination buffer (a multiple of 16: the buffer's alignment is the destination's)


def positions(A, dh, dw):
    """X, Y int64 [dh, dw]: the source position of every destination pixel in 1/32 pixel (sx = X >> 5, ax = X & 31)."""
    A = np.asarray(A, np.float64)
    x, y = np.arange(dw, dtype=np.float64), np.arange(dh, dtype=np.float64)
    adelta, bdelta = np.rint((A[0] * x) * 1024).astype(np.int64), np.rint((A[3] * x) * 1024).astype(np.int64)
    X0, Y0 = np.rint((A[1] * y + A[2]) * 1024).astype(np.int64) + 16, np.rint((A[4] * y + A[5]) * 1024).astype(np.int64) + 16
    return (X0[:, None] + adelta[None, :]) >> 5, (Y0[:, None] + bdelta[None, :]) >> 5


def taps(img, sy, sx, fill, flip):
    """int64 [.., 3]: img at (sy, sx), the fill level where that is outside; with flip an inside tap reads column src_w - 1 - sx."""
    sh, sw = img.shape[:2]
    inside = (sy >= 0) & (sy < sh) & (sx >= 0) & (sx < sw)
    col = sw - 1 - sx if flip else sx
    value = img[np.clip(sy, 0, sh - 1), np.clip(col, 0, sw - 1)].astype(np.int64)
    return np.where(inside[..., None], value, np.array([(fill >> (8 * c)) & 255 for c in range(3)], np.int64))


def warp_image(img, A, dh, dw, fill=0, flip=0):
    """uint8 [dh, dw, 3]: the recipe, restated."""
    X, Y = positions(A, dh, dw)
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    ax, ay = (X & 31)[..., None], (Y & 31)[..., None]
    level = (taps(img, sy, sx, fill, flip) * (32 - ax) * (32 - ay) + taps(img, sy, sx + 1, fill, flip) * ax * (32 - ay)
             + taps(img, sy + 1, sx, fill, flip) * (32 - ax) * ay + taps(img, sy + 1, sx + 1, fill, flip) * ax * ay + 512) >> 10
    return level.astype(np.uint8)


def bilinear64(img, px, py, fill=0):
    """fp64 bilinear interpolation of img at the positions (px, py) (float64 arrays, pixels), the fill level outside: [.., 3]."""
    kx, ky = np.floor(px), np.floor(py)
    tx, ty = (px - kx)[..., None], (py - ky)[..., None]
    kx, ky = kx.astype(np.int64), ky.astype(np.int64)
    t = lambda yy, xx: taps(img, yy, xx, fill, 0).astype(np.float64)
    return (t(ky, kx) * (1 - tx) + t(ky, kx + 1) * tx) * (1 - ty) + (t(ky + 1, kx) * (1 - tx) + t(ky + 1, kx + 1) * tx) * ty


def forward_matrix(h, w, angle):
    """The matrix of a rotation by `angle` degrees about (w / 2, h / 2) on the grown canvas, and the canvas (height, width)."""
    a = angle * math.pi / 180
    al, be = math.cos(a), math.sin(a)
    cx, cy = w / 2, h / 2
    M = np.array([[al, be, (1 - al) * cx - be * cy], [-be, al, be * cx + (1 - al) * cy]], np.float64)
    ch, cw = abs(al) * h + abs(be) * w, abs(al) * w + abs(be) * h
    M[:, 2] += [cw / 2 - cx, ch / 2 - cy]
    return M, (int(ch), int(cw))


def inverse(M):
    """The inverse of a 2x3 map as 6 float64, through numpy's general inversion (not the code under test)."""
    return np.linalg.inv(np.vstack([M, [0, 0, 1]]))[:2].reshape(6)


def rotation(h, w, angle, shift=(0, 0)):
    """(inverse matrix, canvas size) of forward_matrix, the rotated image moved by `shift` = (dx, dy) pixels on the canvas."""
    M, size = forward_matrix(h, w, angle)
    M[:, 2] += shift
    return inverse(M), size


def make_group(rng, items, aligned, fill=0, extra_h=0):
    """items: (image [h, w, 3] uint8, inverse matrix, (dst_h, dst_w), flip, source row padding).  The sources are packed by collate_cases.pack (odd
    byte offsets, random bytes in every gap).  aligned: destination offsets and row strides are multiples of 4 (the 12-byte stores), with gaps and row
    padding; else odd offsets and any stride (the byte stores).  The last destination image ends the buffer."""
    src, src_offset, g8 = cc.pack(rng, [(img, None, flip, rowpad) for img, _, _, flip, rowpad in items])
    dst_offset, dst_geom, pos = [], [], 0
    for _, _, (dh, dw), _, _ in items:
        if aligned:
            pos = -(-pos // 4) * 4 + 4 * int(rng.randint(0, 3))
            stride = -(-3 * dw // 4) * 4 + 4 * int(rng.randint(0, 3))
        else:
            pos += (1 if pos % 2 == 0 else 0) + 2 * int(rng.randint(0, 3))
            stride = 3 * dw + int(rng.randint(0, 6))
        dst_offset.append(pos)
        dst_geom.append((stride, dh, dw, 0, 0, dh, dw, 0))
        pos += (dh - 1) * stride + 3 * dw
    dst_geom = np.array(dst_geom, np.int32).reshape(-1, 8)
    return dict(src=src, src_offset=src_offset, src_geom=np.ascontiguousarray(g8[:, [0, 1, 2, 7]]), inv=np.array([it[1] for it in items], np.float64).reshape(-1, 6),
                dst_offset=np.array(dst_offset, np.int64), dst_geom=dst_geom, nbytes=pos, fill=fill,
                max_h=int(dst_geom[:, 1].max()) + extra_h if len(items) else 8, max_w=int(dst_geom[:, 2].max()) if len(items) else 8)


ANGLES = (0, 5, -5, 30, 45, 90, -135, 180)
SIZES = ((7, 5), (21, 33), (40, 50), (70, 81), (30, 37), (12, 9), (70, 80), (33, 47))


def groups():
    """name -> group (make_group); every group is one launch."""
    rng = np.random.RandomState(23)
    im = lambda h, w: rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    g = {}
    # the smallest group: one 7x5 image, 45 degrees, odd offsets, byte stores
    g['small'] = make_group(rng, [(im(7, 5),) + rotation(7, 5, 45) + (0, 0)], aligned=False)
    # every angle onto its grown canvas, sizes 7x5 .. 70x81, flips alternating, some padded source rows; both destination layouts
    for name, aligned, fill in (('angles', True, 0), ('angles_bytes', False, 0x1E6DC3)):
        g[name] = make_group(rng, [(im(h, w),) + rotation(h, w, angle) + (k % 2, 3 * (k % 3)) for k, ((h, w), angle) in enumerate(zip(SIZES, ANGLES))], aligned, fill)
    # destination widths around the four-pixel item (a canvas of the caller's choice, not the grown one); source widths 1 .. 9 too
    for name, aligned in (('widths', True), ('widths_bytes', False)):
        g[name] = make_group(rng, [(im(9 + k, sw), rotation(9 + k, sw, angle)[0], (6 + k, dw), k % 2, 0)
                                   for k, (dw, sw, angle) in enumerate(zip((1, 3, 4, 5, 30, 64), (1, 3, 4, 5, 9, 8), (0, 30, -5, 45, 5, 30)))], aligned, 0x0000FF)
    # +-5 degrees with the image pushed partly off the canvas on each side: taps at sx = -1, sx = src_w - 1, sy = -1, sy = src_h - 1 next to the fill
    g['shift'] = make_group(rng, [(im(30, 37), rotation(30, 37, angle, shift)[0], rotation(30, 37, angle)[1], flip, 0)
                                  for angle, shift, flip in ((5, (-12, 0), 0), (-5, (12.5, 0), 1), (5, (0, -10), 1), (-5, (0, 10.25), 0),
                                                             (0, (-3, 0), 0), (0, (3, 0), 1), (0, (0, -3), 0), (0, (0, 3), 1))], True, 0x804020)
    g['b1'] = make_group(rng, [(im(23, 31),) + rotation(23, 31, 30) + (1, 0)], True)                      # B = 1, more than one row block
    g['b5'] = make_group(rng, [(im(h, w),) + rotation(h, w, angle) + (k % 2, 0) for k, (h, w, angle) in
                               enumerate(((37, 50, 5), (50, 37, -5), (33, 50, 45), (7, 5, 30), (28, 28, -135)))], True, 0, extra_h=37)      # ragged; max_h beyond every image
    g['b0'] = make_group(rng, [], True)
    return g


GROUP_NAMES = ['small', 'angles', 'angles_bytes', 'widths', 'widths_bytes', 'shift', 'b1', 'b5', 'b0']


def source(group, b):
    """The [src_h, src_w, 3] view of source image b."""
    sg = group['src_geom'][b]
    return cc.image_view(group['src'], int(group['src_offset'][b]), (sg[0], sg[1], sg[2]))


def restate(group):
    """The whole destination buffer (PAD sentinel bytes, nbytes, PAD sentinel bytes) as the contract says the launch leaves it."""
    buf = np.full(group['nbytes'] + 2 * PAD, SENTINEL, np.uint8)
    for b, dg in enumerate(group['dst_geom']):
        stride, dh, dw = (int(v) for v in dg[:3])
        out = warp_image(source(group, b), group['inv'][b], dh, dw, group['fill'], int(group['src_geom'][b, 3]))
        rows = np.lib.stride_tricks.as_strided(buf[PAD + int(group['dst_offset'][b]):], shape=(dh, 3 * dw), strides=(stride, 1))
        rows[:] = out.reshape(dh, 3 * dw)
    return buf


def host(group, buf=None, **change):
    """y2_warp_affine_images_host into a sentinel-filled buffer (or `buf`); `change` replaces tables of the group.  Returns (rc, buffer)."""
    import _hip
    g = dict(group, **change)
    if buf is None:
        buf = np.full(g['nbytes'] + 2 * PAD, SENTINEL, np.uint8)
    arrays = [np.ascontiguousarray(g[k]) for k in ('src', 'src_offset', 'src_geom', 'inv', 'dst_offset', 'dst_geom')]
    p = lambda a: a.ctypes.data if a.size else None
    rc = _hip.lib().y2_warp_affine_images_host(p(arrays[0]), p(arrays[1]), p(arrays[2]), p(arrays[3]), buf[PAD:].ctypes.data, p(arrays[4]), p(arrays[5]),
                                               len(g['dst_geom']), g['max_h'], g['max_w'], g['fill'])
    return rc, buf


# ---- the end-to-end batch: flip + rotate + RandomCrop + Collate

def config_of(g, angles='-30 30'):
    config = cc.config_of(g)
    config.read_dict({'augmentation': {'random_rotate': angles},
                      'transform': {'augmentation': 'transform.augmentation.RandomRotate transform.augmentation.RandomFlipHorizontally'}})
    return config


def make_batch(g, seed=1, rotated=True):
    """Five samples of tests/golden/collate.npz with seeded pixels: flip then rotate, rotate then flip, rotate alone, neither (the identity in a rotated
    batch), RandomRotate + RandomFlipHorizontally as config.ini orders them; then RandomCrop inside Collate.  rotated=False: the flips alone."""
    import transform.augmentation as ta
    import transform.resize.label
    import utils.data
    config = config_of(g)
    rng = np.random.RandomState(seed)
    random.seed(seed)
    np.random.seed(seed)
    rotate, flip = ta.RandomRotate(config), ta.RandomFlipHorizontally(config)
    samples = [cc.sample(g, k, rng) for k in (4, 9, 11, 5, 14)]
    if rotated:
        samples[0] = rotate(ta.flip_horizontally(samples[0]))
        samples[1] = ta.flip_horizontally(rotate(samples[1]))
        samples[2] = rotate(samples[2])
        samples[4] = flip(rotate(samples[4]))
    else:
        samples = [ta.flip_horizontally(s) if k % 2 else s for k, s in enumerate(samples)]
    collate = utils.data.Collate(transform.resize.label.RandomCrop(config), [(40, 56)], maintain=1)
    return samples, collate(samples)


def restate_batch(batch, lut, fill=0):
    """The fp32 tensor and the intermediate buffer of a rotated batch: collate_cases.restate applied to the restated warp output."""
    offset, geom = batch['offset'].numpy(), batch['geom'].numpy()
    group = dict(src=batch['raw'].numpy(), src_offset=batch['src_offset'].numpy(), src_geom=batch['src_geom'].numpy(), inv=batch['warp'].numpy(),
                 dst_offset=offset, dst_geom=geom, nbytes=int(batch['rot_bytes']), fill=fill)
    rot = restate(group)[PAD:PAD + group['nbytes']]
    H, W = batch['size']
    return cc.restate(rot, offset, geom, lut, H, W, 1), rot


def reference_lut(normalize=(0.5, 1.0)):
    import torch
    lut = torch.arange(256).float().div(255)          # ToTensor, then Normalize, with the reference's own operations
    lut = lut.sub(torch.tensor([normalize[0]])).div(torch.tensor([normalize[1]]))
    return lut.view(1, 256).repeat(3, 1).numpy()
