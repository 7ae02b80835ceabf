"""Shared by test_jitter_cpu.py and test_gpu_jitter.py: a numpy restatement of the whole contract of y2_collate_jitter_images (include/yolo2_hip.h),
written from the header and not from the C++ - the resize is collate_cases.levels, the division tables are the header's float64 formula, the blur
gathers reflected indices, the colour conversions are vectorised - and the case groups, one launch each into a sentinel-filled fp32 buffer, at the
smallest shapes where each mechanism can go wrong (the kernel's tile is 32 x 32 outputs, its halo up to 3 pixels on each side)."""
import numpy as np

import collate_cases as cc

SENTINEL = cc.SENTINEL
PAD = 64          # sentinel floats on either side of the output (256 bytes: the output keeps the buffer's 16-byte alignment unless `shift` moves it)
TILE_H = TILE_W = 32
MAX_BLUR = 7


# ---- the contract, restated

def reflect101(p, n):
    """borderInterpolate's BORDER_REFLECT_101 loop for one position."""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def blur(lv, kx, ky):
    """cv2.blur(lv, (kx, ky)) of a uint8 [H, W, 3] image, restated: integer window sums over reflected coordinates, one float64 product, rint."""
    H, W = lv.shape[:2]
    if kx == 1 and ky == 1:
        return lv.copy()
    ix = np.array([[reflect101(x - kx // 2 + i, W) for i in range(kx)] for x in range(W)])
    iy = np.array([[reflect101(y - ky // 2 + j, H) for j in range(ky)] for y in range(H)])
    s = lv.astype(np.int64)[:, ix].sum(2)[iy].sum(1)          # [H, W, 3]
    return np.clip(np.rint(s.astype(np.float64) * (1.0 / float(kx * ky))), 0, 255).astype(np.uint8)


def div_tables():
    """sdiv, hdiv int64 [256], by the header's float64 formula (numpy's rint rounds half to even)."""
    i = np.arange(1, 256, dtype=np.float64)
    sdiv, hdiv = np.zeros(256, np.int64), np.zeros(256, np.int64)
    sdiv[1:] = np.rint((255 << 12) / (1.0 * i)).astype(np.int64)
    hdiv[1:] = np.rint((180 << 12) / (6.0 * i)).astype(np.int64)
    return sdiv, hdiv


def bgr2hsv(bgr):
    """8-bit COLOR_BGR2HSV of a uint8 [..., 3] array (B, G, R), restated: uint8 [..., 3] (H, S, V)."""
    sdiv, hdiv = div_tables()
    b, g, r = (bgr[..., c].astype(np.int64) for c in range(3))
    v = np.maximum(np.maximum(b, g), r)
    diff = v - np.minimum(np.minimum(b, g), r)
    s = (diff * sdiv[v] + 2048) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * hdiv[diff] + 2048) >> 12
    h = np.where(h < 0, h + 180, h)
    return np.stack([np.clip(h, 0, 255), np.clip(s, 0, 255), np.clip(v, 0, 255)], -1).astype(np.uint8)


def hsv2rgb(hsv):
    """8-bit COLOR_HSV2RGB of a uint8 [..., 3] array (H, S, V), restated in float32 operations: uint8 [..., 3] (R, G, B)."""
    f = np.float32
    h, s, v = (hsv[..., c] for c in range(3))
    hf = h.astype(f)
    sf, vf = s.astype(f) * (f(1) / f(255)), v.astype(f) * (f(1) / f(255))
    hf = hf * (f(6) / f(180))
    while (hf >= f(6)).any():
        hf = np.where(hf >= f(6), hf - f(6), hf)
    sector = np.floor(hf)
    hf = hf - sector
    sector = sector.astype(np.int64)
    outside = (sector < 0) | (sector > 5)
    sector, hf = np.where(outside, 0, sector), np.where(outside, f(0), hf)
    one = f(1)
    tab = np.stack([vf, vf * (one - sf), vf * (one - sf * hf), vf * (one - sf * (one - hf))], -1)
    assert tab.dtype == np.float32
    order = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])[sector]          # [..., 3]: (b, g, r)
    bgr = np.take_along_axis(tab, order, -1)
    bgr = np.where((s == 0)[..., None], vf[..., None], bgr)
    level = np.clip(np.rint(bgr * f(255)), 0, 255).astype(np.uint8)
    return level[..., ::-1]


def colour(lv, hsv, tab, flags):
    """uint8 [..., 3]: the levels of the three output planes from blurred BGR levels."""
    if not hsv:
        return lv[..., ::-1] if flags & 1 else lv
    x = bgr2hsv(lv)
    return hsv2rgb(np.stack([tab[c][x[..., c]] for c in range(3)], -1))


def planes(group):
    """uint8 [B, H, W, 3]: the level of every output value, plane order last."""
    lv = cc.levels(group['src'], group['offset'], group['geom'], group['H'], group['W'])
    out = np.zeros_like(lv)
    for b, (kx, ky, hsv, _) in enumerate(group['jitter']):
        out[b] = colour(blur(lv[b], int(kx), int(ky)), hsv, None if group['hsv_tab'] is None else group['hsv_tab'][b], group['flags'])
    return out


def restate(group):
    """The whole output buffer (PAD sentinels, `shift` more, the tensor, sentinels) as the contract says the launch leaves it."""
    B, H, W = len(group['geom']), group['H'], group['W']
    buf = np.full(B * 3 * H * W + 2 * PAD, SENTINEL, np.float32)
    if B:
        p = planes(group)
        out = np.stack([np.take_along_axis(group['lut'][:, c], p[..., c].reshape(B, -1).astype(np.int64), 1) for c in range(3)], 1)      # [B, 3, H * W]
        at = PAD + group['shift']
        buf[at:at + out.size] = out.reshape(-1)
    return buf


# ---- the case groups

def random_tables(rng, B):
    """Random, non-monotonic uint8 H / S / V tables and fp32 output tables per image: a table, plane or image mix-up cannot cancel."""
    return rng.randint(0, 256, (B, 3, 256)).astype(np.uint8), rng.uniform(-3, 3, (B, 3, 256)).astype(np.float32)


def make_group(rng, images, H, W, jitter, flags=1, shift=0, hsv_tab='random', lut=None):
    """images: the tuples of collate_cases.pack; jitter: (kx, ky, hsv) per image."""
    src, offset, geom = cc.pack(rng, images)
    B = len(images)
    tabs, luts = random_tables(rng, B)
    return dict(src=src, offset=offset, geom=geom, H=H, W=W, flags=flags, shift=shift,
                jitter=np.array([tuple(j) + (0,) for j in jitter], np.int32).reshape(-1, 4),
                hsv_tab=tabs if isinstance(hsv_tab, str) else hsv_tab, lut=luts if lut is None else lut)


BLURS = ((7, 7), (4, 2), (1, 7), (7, 1))
# colour extremes as (B, G, R): grey, black, white, the primaries and secondaries (negative hue before the wrap), v == g and v == r ties, near-greys
COLOURS = np.array([(128, 128, 128), (0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 255, 255),
                    (10, 200, 200), (200, 200, 10), (200, 10, 200), (1, 0, 0), (0, 1, 0), (0, 0, 1), (255, 254, 255), (254, 255, 255), (7, 7, 8),
                    (255, 0, 1), (1, 0, 255), (0, 255, 1), (100, 50, 100), (50, 100, 100), (100, 100, 50)], np.uint8)


def groups():
    """name -> group (make_group); every group is one launch."""
    rng = np.random.RandomState(29)
    im = lambda h, w: rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    g = {}
    # outputs smaller than the blur: several reflections per tap, and the n == 1 rule; both colour paths
    for name, (H, W) in (('o1x1', (1, 1)), ('o1x5', (1, 5)), ('o2x3', (2, 3))):
        g[name] = make_group(rng, [(im(5, 7), None, 0, 0), (im(H, W), None, 1, 0), (im(9, 4), (1, 0, 6, 4), 0, 2)], H, W, [(7, 7, 1), (7, 7, 0), (6, 5, 1)])
    # one row and column more than a tile / one short of a tile: the halo crosses tile edges and the image border in the same tile; even sizes test
    # the anchor; 4-byte stores (W % 4 != 0)
    for name, (H, W) in (('tile_plus', (TILE_H + 1, TILE_W + 1)), ('tile_short', (TILE_H - 1, 2 * TILE_W - 1))):
        g[name] = make_group(rng, [(im(40 + 3 * k, 50 - 2 * k), None, k % 2, k) for k in range(4)], H, W, [b + (k % 2,) for k, b in enumerate(BLURS)])
    # W % 4 == 0: 16-byte stores, a last tile of 4 columns and 1 row; then the same launch into an output 4 bytes off: 4-byte stores
    images = [(im(30 + k, 41 + k), None, k % 2, 0) for k in range(4)]
    for name, shift in (('vec', 0), ('vec_shift', 1)):
        g[name] = make_group(np.random.RandomState(31), images, TILE_H + 1, TILE_W + 4, [b + ((k + 1) % 2,) for k, b in enumerate(BLURS)], shift=shift)
    # the images of collate_cases' 32x32 group (the 2:1 box mean, flips, windows on every image edge, padded rows, one-pixel windows) with mixed paths and
    # blur sizes in ONE launch, 1x1 included; BGR order kept on the plain path (flags 0)
    src = cc.groups()['32x32']
    mixed = [(int(rng.randint(1, 8)), int(rng.randint(1, 8)), k % 2) for k in range(len(src[2]))]
    mixed[0], mixed[1], mixed[10], mixed[11] = (1, 1, 0), (1, 1, 1), (5, 5, 1), (3, 4, 0)
    tabs, luts = random_tables(rng, len(mixed))
    g['mixed'] = dict(src=src[0], offset=src[1], geom=src[2], H=32, W=32, flags=0, shift=0, jitter=np.array([j + (0,) for j in mixed], np.int32), hsv_tab=tabs, lut=luts)
    # no image goes through HSV: hsv_tab may be absent; two tiles per row, 64 x 96 is the largest case
    g['plain'] = make_group(rng, [(im(100, 150), None, 0, 0), (im(128, 192), None, 1, 0), (im(70, 97), (3, 0, 64, 96), 0, 0)], 64, 96, [(5, 5, 0), (2, 3, 0), (1, 1, 0)], hsv_tab=None)
    # colour extremes through HSV at identity resize without blur; tables: identity, H moved beyond 179 (the hf >= 6 wrap), all 255, all 0, random
    tile = np.resize(COLOURS, (4, 12, 3))
    ident = np.arange(256, dtype=np.uint8)
    high = np.minimum(ident.astype(np.int64) + 76, 255).astype(np.uint8)
    tabs = np.stack([np.stack([ident] * 3), np.stack([high, ident, ident]), np.full((3, 256), 255, np.uint8), np.zeros((3, 256), np.uint8),
                     rng.randint(0, 256, (3, 256)).astype(np.uint8)])
    g['colours'] = make_group(rng, [(tile, None, 0, 0)] * 5, 4, 12, [(1, 1, 1)] * 5, hsv_tab=tabs)
    g['b0'] = make_group(rng, [], 32, 32, [])
    return g


GROUP_NAMES = ['o1x1', 'o1x5', 'o2x3', 'tile_plus', 'tile_short', 'vec', 'vec_shift', 'mixed', 'plain', 'colours', 'b0']


def host(group, **change):
    """y2_collate_jitter_images_host into a sentinel-filled buffer; `change` replaces tables or scalars of the group (B=...: the count handed over).
    Returns (rc, buffer)."""
    import _hip
    g = dict(group, **change)
    B = g.get('B', len(g['geom']))
    buf = np.full(len(g['geom']) * 3 * g['H'] * g['W'] + 2 * PAD, SENTINEL, np.float32)
    arrays = [None if g[k] is None else np.ascontiguousarray(g[k]) for k in ('src', 'offset', 'geom', 'jitter', 'hsv_tab', 'lut')]
    p = lambda a: a.ctypes.data if a is not None and a.size else None
    rc = _hip.lib().y2_collate_jitter_images_host(*[p(a) for a in arrays], B, g['H'], g['W'], g['flags'], buf[PAD + g['shift']:].ctypes.data)
    return rc, buf


# ---- the end-to-end batch

IMAGE_TRAIN = ('transform.image.RandomBlur transform.image.BGR2HSV transform.image.RandomHue transform.image.RandomSaturation transform.image.RandomBrightness '
               'transform.image.HSV2RGB transform.image.RandomGamma')
AUGMENTATION = {'random_blur': '5 5', 'random_hue': '0 25', 'random_saturation': '0.5 1.5', 'random_brightness': '0.5 1.5', 'random_gamma': '0.9 1.5'}


def config_of(golden):
    import rotate_cases as rc
    config = rc.config_of(golden)
    config.read_dict({'augmentation': AUGMENTATION, 'transform': {'image_train': IMAGE_TRAIN, 'normalize': '0.5 1'}})
    return config


def make_batch(golden, seed=1, rotated=True, sequence=IMAGE_TRAIN):
    """rotate_cases.make_batch with a transform_image: the same five samples, flips and rotations, then RandomCrop and the jitter draws inside Collate.
    sequence=None: Collate without transform_image."""
    import random

    import rotate_cases as rc
    import transform.augmentation as ta
    import transform.image
    import transform.resize.label
    import utils.data
    config = config_of(golden)
    rng = np.random.RandomState(seed)
    random.seed(seed)
    np.random.seed(seed)
    rotate, flip = ta.RandomRotate(config), ta.RandomFlipHorizontally(config)
    samples = [cc.sample(golden, k, rng) for k in (4, 9, 11, 5, 14)]
    if rotated:
        samples[0] = rotate(ta.flip_horizontally(samples[0]))
        samples[1] = ta.flip_horizontally(rotate(samples[1]))
        samples[2] = rotate(samples[2])
        samples[4] = flip(rotate(samples[4]))
    else:
        samples = [ta.flip_horizontally(s) if k % 2 else s for k, s in enumerate(samples)]
    kwargs = {} if sequence is None else dict(transform_image=transform.image.get_transform(config, sequence.split()))
    collate = utils.data.Collate(transform.resize.label.RandomCrop(config), [(40, 56)], maintain=1, **kwargs)
    return samples, collate(samples)


def restate_batch(batch, pixels):
    """The fp32 tensor of a jittered batch from the byte buffer its offset / geom index (`raw`, or the restated warp output of a rotated batch)."""
    H, W = batch['size']
    group = dict(src=pixels, offset=batch['offset'].numpy(), geom=batch['geom'].numpy(), H=H, W=W, flags=1 if batch['swap_rb'] else 0, shift=0,
                 jitter=batch['jitter'].numpy(), hsv_tab=batch['hsv_tab'].numpy() if 'hsv_tab' in batch else None, lut=batch['lut_b'].numpy())
    buf = restate(group)
    return buf[PAD:len(buf) - PAD].reshape(len(group['geom']), 3, H, W)
