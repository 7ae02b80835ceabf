"""Shared by test_collate_cpu.py and test_gpu_collate.py: the numpy restatement of y2_collate_images' resampling contract (include/yolo2_hip.h), an
fp64 bilinear interpolation with the same geometry, and the case groups - one launch each - at the smallest shapes where each path can go wrong."""
import configparser
import random

import numpy as np

SENTINEL = np.float32(-12345.5)


def axis(s, d, edge):
    """Taps (clamped) and 11-bit coefficients of the d destination indices of an axis that reads a window of s pixels."""
    scale = np.float64(s) / np.float64(d)
    f = ((np.arange(d, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    k = np.floor(f)
    f = (f - k).astype(np.float32)
    k = k.astype(np.int64)
    if edge:
        lo, hi = k < 0, k >= s - 1
        k = np.where(lo, 0, np.where(hi, s - 1, k))
        f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
    c1 = np.rint(f * np.float32(2048)).astype(np.int64)
    c0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    return np.clip(k, 0, s - 1), np.clip(k + 1, 0, s - 1), c0, c1


def image_view(src, offset, g):
    """The [src_h, src_w, 3] view of one image of the packed buffer."""
    stride, sh, sw = int(g[0]), int(g[1]), int(g[2])
    return np.lib.stride_tricks.as_strided(src[offset:], shape=(sh, sw, 3), strides=(stride, 3, 1), writeable=False)


def window(src, offset, g):
    """The window of one image in the frame after the flip, int64 [win_h, win_w, 3]."""
    img = image_view(src, offset, g)
    if g[7]:
        img = img[:, ::-1]
    return img[g[3]:g[3] + g[5], g[4]:g[4] + g[6]].astype(np.int64)


def levels(src, offset, geom, H, W):
    """uint8 levels [B, H, W, 3] in SOURCE channel order: the recipe, restated."""
    out = np.zeros((len(geom), H, W, 3), np.uint8)
    for b, g in enumerate(geom):
        win = window(src, int(offset[b]), g)
        wh, ww = win.shape[:2]
        if wh == 2 * H and ww == 2 * W:
            lv = (win[0::2, 0::2] + win[0::2, 1::2] + win[1::2, 0::2] + win[1::2, 1::2] + 2) >> 2
        else:
            x0, x1, a0, a1 = axis(ww, W, True)
            y0, y1, b0, b1 = axis(wh, H, False)
            h = win[:, x0] * a0[None, :, None] + win[:, x1] * a1[None, :, None]          # [wh, W, 3]
            h0, h1 = h[y0] >> 4, h[y1] >> 4
            lv = (((b0[:, None, None] * h0) >> 16) + ((b1[:, None, None] * h1) >> 16) + 2) >> 2
        out[b] = np.clip(lv, 0, 255)
    return out


def restate(src, offset, geom, lut, H, W, flags):
    """fp32 [B, 3, H, W]: lut[c][level of source channel (2 - c if flags & 1 else c)]."""
    lv = levels(src, offset, geom, H, W)
    out = np.zeros((len(geom), 3, H, W), np.float32)
    for c in range(3):
        out[:, c] = lut[c][lv[..., 2 - c if flags & 1 else c]]
    return out


def bilinear64(src, offset, geom, H, W):
    """fp64 bilinear interpolation with the same half-pixel geometry and a replicated border, [B, H, W, 3] in source channel order."""
    out = np.zeros((len(geom), H, W, 3), np.float64)
    for b, g in enumerate(geom):
        win = window(src, int(offset[b]), g).astype(np.float64)
        wh, ww = win.shape[:2]
        fy = (np.arange(H) + 0.5) * (wh / H) - 0.5
        fx = (np.arange(W) + 0.5) * (ww / W) - 0.5
        ky, kx = np.floor(fy).astype(np.int64), np.floor(fx).astype(np.int64)
        ty, tx = (fy - ky)[:, None, None], (fx - kx)[None, :, None]
        y0, y1, x0, x1 = np.clip(ky, 0, wh - 1), np.clip(ky + 1, 0, wh - 1), np.clip(kx, 0, ww - 1), np.clip(kx + 1, 0, ww - 1)
        top = win[y0][:, x0] * (1 - tx) + win[y0][:, x1] * tx
        bot = win[y1][:, x0] * (1 - tx) + win[y1][:, x1] * tx
        out[b] = top * (1 - ty) + bot * ty
    return out


def pack(rng, images):
    """images: (array [h, w, 3] uint8, window (y0, x0, h, w) or None, flip, row padding bytes).  One byte buffer with random bytes in every gap
    (in front of the first image, between images, behind each row) and every image at an ODD byte offset; the last image ends the buffer."""
    chunks, offset, geom, pos = [], [], [], 0
    for img, win, flip, rowpad in images:
        h, w = img.shape[:2]
        gap = 1 + 2 * int(rng.randint(0, 3)) if pos % 2 == 0 else 2 * int(rng.randint(0, 3))
        chunks.append(rng.randint(0, 256, gap).astype(np.uint8))
        pos += gap
        stride = 3 * w + rowpad
        rows = rng.randint(0, 256, (h, stride)).astype(np.uint8)
        rows[:, :3 * w] = img.reshape(h, 3 * w)
        flat = rows.reshape(-1)[:(h - 1) * stride + 3 * w]          # no padding behind the last row: the image ends where its last pixel ends
        chunks.append(flat)
        offset.append(pos)
        geom.append((stride, h, w) + tuple(win if win is not None else (0, 0, h, w)) + (int(flip),))
        pos += flat.size
    src = np.concatenate(chunks) if chunks else np.zeros(0, np.uint8)
    return src, np.array(offset, np.int64), np.array(geom, np.int32).reshape(-1, 8)


def random_lut(seed=5):
    """A different random, non-monotonic table per channel: a plane or channel mix-up cannot cancel."""
    return np.random.RandomState(seed).uniform(-3, 3, (3, 256)).astype(np.float32)


def groups():
    """name -> (src, offset, geom, H, W); every group is one launch."""
    rng = np.random.RandomState(17)
    im = lambda h, w: rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    g = {}
    g['32x32'] = pack(rng, [
        (im(7, 5), None, 0, 0),                       # upscale on both axes
        (im(300, 301), None, 0, 0),                   # each output samples 2 of about 9 source pixels
        (im(40, 50), (0, 5, 20, 30), 0, 0),           # windows touching the top, bottom, left and right border
        (im(40, 50), (20, 5, 20, 30), 0, 0),
        (im(40, 50), (5, 0, 20, 30), 1, 0),
        (im(40, 50), (5, 20, 20, 30), 1, 0),
        (im(12, 9), (3, 7, 8, 1), 0, 0),              # win_w = 1 / win_h = 1: both taps are the same pixel
        (im(12, 9), (4, 2, 1, 6), 1, 0),
        (im(30, 37), (2, 9, 25, 20), 1, 0),           # flip, odd and even src_w, off-centre window
        (im(30, 36), (3, 1, 20, 22), 1, 0),
        (im(70, 80), (3, 9, 64, 64), 0, 0),           # exactly 2:1 on both axes: the box mean
        (im(70, 81), (5, 11, 64, 64), 1, 5),          # ... flipped, padded rows
        (im(70, 80), (3, 9, 64, 50), 0, 0),           # 2:1 on one axis only: bilinear
        (im(70, 80), (3, 9, 50, 64), 0, 0),
        (im(21, 33), None, 0, 7),                     # row_stride_bytes > 3 * src_w, random bytes in the padding
        (im(21, 33), (1, 2, 19, 30), 1, 2),
    ]) + (32, 32)
    g['32x64'] = pack(rng, [(im(97, 130), None, 0, 0), (im(10, 200), None, 0, 0), (im(200, 10), None, 1, 0)]) + (32, 64)      # down / up per axis
    g['w4'] = pack(rng, [(im(9, 9), None, 0, 0), (im(5, 3), None, 1, 0), (im(40, 8), (0, 0, 40, 8), 0, 0)]) + (20, 4)          # W = 4 (third: box)
    g['w30'] = pack(rng, [(im(9, 41), None, 1, 0), (im(50, 33), (1, 1, 40, 30), 0, 3), (im(40, 60), None, 0, 0)]) + (20, 30)   # scalar path (third: box)
    g['b1'] = pack(rng, [(im(23, 31), (2, 3, 20, 25), 1, 0)]) + (40, 36)                                                       # B = 1, more than one row block
    g['b5'] = pack(rng, [(im(37, 50), None, 0, 0), (im(50, 37), None, 1, 0), (im(33, 50), (0, 0, 33, 25), 1, 0), (im(50, 33), (10, 3, 40, 30), 0, 0),
                         (im(28, 28), None, 1, 0)]) + (16, 40)                                                                 # five sizes, mixed flips
    g['b0'] = pack(rng, []) + (32, 32)
    return g


# ---- shared helpers of the two test files

def host(src, offset, geom, lut, H, W, flags, out=None):
    """y2_collate_images_host; returns (rc, out) with out over-allocated by 64 floats on either side when not given."""
    B = len(geom)
    n = B * 3 * H * W
    if out is None:
        out = np.full(n + 128, SENTINEL, np.float32)
    src = np.ascontiguousarray(src)
    p = lambda a: a.ctypes.data if a.size else None
    import _hip
    rc = _hip.lib().y2_collate_images_host(p(src), p(offset), p(geom), lut.ctypes.data, B, H, W, flags, out[64:].ctypes.data)
    return rc, out


def config_of(g):
    config = configparser.ConfigParser()
    config.read_dict({'data': {'resize': 'rescale'},
                      'augmentation': {'random_flip_horizontally': repr(float(g['flip_prob'])), 'random_crop': repr(float(g['crop_scale']))},
                      'transform': {'augmentation': 'transform.augmentation.RandomFlipHorizontally', 'resize_train': 'transform.resize.label.RandomCrop',
                                    'resize_eval': 'transform.resize.label.Resize'}})
    return config


def sample(g, k, rng=None):
    n, (h, w) = int(g['count'][k]), g['size'][k]
    image = np.zeros((h, w, 3), np.uint8) if rng is None else rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    return dict(image=image, yx_min=g['in_min'][k, :n].copy(), yx_max=g['in_max'][k, :n].copy(), cls=np.arange(n, dtype=np.int64) % 3,
                difficult=np.zeros(n, np.uint8))


def make_batch(g, seed=1):
    import transform.augmentation
    import transform.resize.label
    import utils.data
    config = config_of(g)
    rng = np.random.RandomState(seed)
    flip, crop = transform.augmentation.RandomFlipHorizontally(config), transform.resize.label.RandomCrop(config)
    random.seed(seed)
    np.random.seed(seed)
    samples = [flip(sample(g, k, rng)) for k in (1, 4, 5, 9, 11)]
    collate = utils.data.Collate(crop, [(40, 56)], maintain=1)
    return samples, collate(samples)
