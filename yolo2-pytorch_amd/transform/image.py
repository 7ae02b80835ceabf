"""`transform.image` — the image plugins of `[transform] image_train` / `image_test` under the reference's names and constructors
(transform/image.py): BGR2RGB, BGR2HSV, HSV2RGB, RandomBlur(config), RandomHue(config), RandomSaturation(config), RandomBrightness(config),
RandomGamma(config), and Normalize(config) of `[transform] tensor`.

The plugins touch no pixel.  The reference runs them on the resized image inside the worker; here each one draws the random numbers the reference
draws, in its order, and writes the outcome into a per-sample RECORD (`new_record()`), which utils.data.Collate turns into the tables of
y2_collate_jitter_images: the blur size, and per-level maps for everything else - hue, saturation and brightness as uint8[256] tables on H, S and V,
the gamma curve as a uint8[256] table on the RGB levels.  The maps are computed with the reference's own numpy arithmetic and dtypes on
`arange(256)`, so a table entry is what the reference computes for a pixel of that level:
  RandomHue          clip(h.astype(int) + a, 0, 179)
  RandomSaturation   clip(s * a, 0, 255).astype(uint8): a float64 product, truncated (RandomBrightness alike, on V)
  RandomGamma        skimage.exposure.adjust_gamma for uint8 images, restated: floor(255 * (arange(256) / 255.0) ** gamma) in float64, a negative
                     gamma raises ValueError.  Restated from memory; agreement with a real skimage is UNVERIFIED (later releases round instead of
                     truncating).  As stated, level 255 maps to 255 or, where the float64 power of 1.0 scaled comes out below 255, to 254.

`get_transform(config, sequence)` accepts the canonical shape
  [RandomBlur] (BGR2RGB | BGR2HSV {RandomHue, RandomSaturation, RandomBrightness: each at most once, any order} HSV2RGB) [RandomGamma]
and a lone BGR2RGB or nothing; anything else is a ValueError that names the sequence."""
import random

import numpy as np

MAX_BLUR = 7          # Y2_JITTER_MAX_BLUR (include/yolo2_hip.h)


def new_record():
    """The jitter of one sample before any plugin ran: no blur, identity tables, the draws made so far."""
    level = np.arange(256, dtype=np.uint8)
    return dict(blur=(1, 1), hsv=False, h=level.copy(), s=level.copy(), v=level.copy(), gamma=level.copy(), draws=[])


def _adjust(config, name, kind):
    return tuple(kind(v) for v in config.get('augmentation', name).split())


class BGR2RGB(object):
    def __call__(self, record):
        return record


class BGR2HSV(object):
    def __call__(self, record):
        record['hsv'] = True
        return record


class HSV2RGB(object):
    def __call__(self, record):
        return record


class RandomBlur(object):
    """`[augmentation] random_blur = a b`: cv2.blur with a (width, height) of random.randint(1, a), random.randint(1, b)."""

    def __init__(self, config):
        self.adjust = _adjust(config, 'random_blur', int)
        if len(self.adjust) != 2 or not all(1 <= a <= MAX_BLUR for a in self.adjust):
            raise ValueError('random_blur: two sizes in 1 .. %d (got %r)' % (MAX_BLUR, self.adjust))

    def __call__(self, record):
        adjust = tuple(random.randint(1, adjust) for adjust in self.adjust)
        record['draws'].append(adjust)
        record['blur'] = adjust
        return record


class RandomHue(object):
    def __init__(self, config):
        self.adjust = _adjust(config, 'random_hue', int)

    def __call__(self, record):
        adjust = random.randint(*self.adjust)
        record['draws'].append(adjust)
        h = record['h'].astype(int) + adjust
        record['h'] = np.clip(h, 0, 179).astype(np.uint8)
        return record


class RandomSaturation(object):
    def __init__(self, config):
        self.adjust = _adjust(config, 'random_saturation', float)

    def __call__(self, record):
        adjust = random.uniform(*self.adjust)
        record['draws'].append(adjust)
        s = record['s'] * adjust
        record['s'] = np.clip(s, 0, 255).astype(np.uint8)
        return record


class RandomBrightness(object):
    def __init__(self, config):
        self.adjust = _adjust(config, 'random_brightness', float)

    def __call__(self, record):
        adjust = random.uniform(*self.adjust)
        record['draws'].append(adjust)
        v = record['v'] * adjust
        record['v'] = np.clip(v, 0, 255).astype(np.uint8)
        return record


def gamma_table(gamma):
    """uint8 [256]: adjust_gamma of every uint8 level (gain 1), restated - see the module's docstring."""
    if gamma < 0:
        raise ValueError('Gamma should be a non-negative real number.')
    return np.floor(255 * (np.arange(256) / 255.0) ** gamma).astype(np.uint8)


class RandomGamma(object):
    def __init__(self, config):
        self.adjust = _adjust(config, 'random_gamma', float)

    def __call__(self, record):
        adjust = random.uniform(*self.adjust)
        record['draws'].append(adjust)
        record['gamma'] = gamma_table(adjust)[record['gamma']]
        return record


class Normalize(object):
    """`[transform] normalize = mean std`: one mean and one std for the three channels, applied to a [3, h, w] tensor as `sub(mean).div(std)`.
    utils.data folds it into the level table; `(mean, std)` is what Collate's `normalize` takes."""

    def __init__(self, config):
        self.mean, self.std = (float(v) for v in config.get('transform', 'normalize').split())

    def __call__(self, tensor):
        return tensor.sub(self.mean).div(self.std)


_HSV_MAPS = (RandomHue, RandomSaturation, RandomBrightness)


class Jitter(object):
    """What get_transform returns: called without arguments it runs the plugins on a fresh record - one call per sample, after the sample's resize
    transform, as the reference orders its draws - and returns the record.  `swap_rb`: the plain path swaps channels (the sequence has BGR2RGB);
    `active`: the sequence has a plugin the plain collate kernel cannot serve; `hsv`: it goes through HSV."""

    def __init__(self, plugins):
        self.plugins = plugins
        self.swap_rb = any(isinstance(p, BGR2RGB) for p in plugins)
        self.hsv = any(isinstance(p, BGR2HSV) for p in plugins)
        self.active = any(not isinstance(p, BGR2RGB) for p in plugins)

    def __call__(self, record=None):
        record = new_record() if record is None else record
        for plugin in self.plugins:
            record = plugin(record)
        return record


def _plugin(config, method):
    if not isinstance(method, str):
        return method
    module, _, name = method.rpartition('.')
    cls = globals().get(name) if module in ('transform.image', '') else None
    if not isinstance(cls, type) or cls in (Jitter, Normalize):
        return None          # no image plugin of this package
    return cls() if cls in (BGR2RGB, BGR2HSV, HSV2RGB) else cls(config)


def get_transform(config, sequence):
    """The Jitter of a `[transform] image_train` line: `sequence` holds dotted names ('transform.image.RandomBlur') or plugin objects."""
    sequence = list(sequence)
    plugins = [_plugin(config, method) for method in sequence]
    rest = list(plugins)
    if rest and isinstance(rest[0], RandomBlur):
        rest.pop(0)
    if rest and isinstance(rest[-1], RandomGamma):
        rest.pop()
    ok = None not in plugins and (not plugins or (len(rest) == 1 and isinstance(rest[0], BGR2RGB)))
    if not ok and None not in plugins and len(rest) >= 2 and isinstance(rest[0], BGR2HSV) and isinstance(rest[-1], HSV2RGB):
        maps = [type(p) for p in rest[1:-1]]
        ok = all(m in _HSV_MAPS for m in maps) and len(set(maps)) == len(maps)
    if not ok:
        raise ValueError('transform.image.get_transform: unsupported sequence %s - the device serves [RandomBlur] (BGR2RGB | BGR2HSV {RandomHue, '
                         'RandomSaturation, RandomBrightness} HSV2RGB) [RandomGamma]' % ' '.join(m if isinstance(m, str) else type(m).__name__ for m in sequence))
    return Jitter(plugins)
