"""`transform.resize.label` — Rescale, Resize(config), RandomCrop(config): the names and call signatures of the reference's resize plugins
(transform/resize/label.py), for the device collate step.

Each one leaves `data['image']` - the uint8 array as it was read - alone and records which part of it the sample shows, `data['window'] =
(y0, x0, h, w)` in the frame after the optional rotation (`data['rotate']`) and flip (`data['flip']`), for y2_collate_images to resample.  The labels get the arithmetic of the
reference in float32, operation for operation, and the random numbers are drawn as the reference draws them (tests/golden/collate.npz pins both).
A sample is resized ONCE: after it the labels are in output coordinates, so a second resize transform on the same sample raises."""
import numpy as np

from transform import frame_size


def _source_size(data, who):
    if 'window' in data:
        raise ValueError('%s: the sample already carries a window - one resize transform per sample' % who)
    return frame_size(data)


def _to_output(data, window, height, width):
    """Labels relative to `window` -> labels in the height x width output; records the window."""
    factor = np.array([height / window[2], width / window[3]], np.float32)
    data['yx_min'] *= factor
    data['yx_max'] *= factor
    data['window'] = tuple(int(v) for v in window)
    data['flip'] = bool(data.get('flip', False))
    return data


def rescale(data, height, width):
    """The whole image, stretched to height x width."""
    h, w = _source_size(data, 'rescale')
    return _to_output(data, (0, 0, h, w), height, width)


def _configured_resize(config):
    name = config.get('data', 'resize')
    if name != 'rescale':
        raise NotImplementedError('[data] resize = %s: only `rescale` has a device collate path (the padding resize stays host work)' % name)
    return rescale


def random_crop(config, data, height, width):
    """A random part of the image that still holds every box: on each side up to `[augmentation] random_crop` of the space between the image
    border and the hull of the boxes is cut away (np.random.rand(4): top, left, bottom, right; the cut is truncated to whole pixels, the labels
    move by the untruncated amount), then the part is stretched like `rescale`.  Without a box the hull does not exist: numpy's ValueError."""
    fraction = config.getfloat('augmentation', 'random_crop')
    if not 0 < fraction <= 1:
        raise ValueError('[augmentation] random_crop must be in (0, 1] (got %r)' % fraction)
    h, w = _source_size(data, 'random_crop')
    lo, hi = data['yx_min'], data['yx_max']
    extent = np.array([h, w], lo.dtype)
    room = np.concatenate([lo.min(0), extent - hi.max(0)])
    cut = fraction * np.random.rand(4).astype(lo.dtype) * room
    top, left = int(cut[0]), int(cut[1])
    bottom, right = (int(v) for v in extent - cut[2:])
    if not (0 <= top < bottom <= h and 0 <= left < right <= w):
        raise ValueError('random_crop: rows %d:%d, columns %d:%d leave the %dx%d image (boxes outside the image?)' % (top, bottom, left, right, h, w))
    data['yx_min'], data['yx_max'] = lo - cut[:2], hi - cut[:2]
    _configured_resize(config)          # (the reference resizes the crop with `[data] resize`)
    return _to_output(data, (top, left, bottom - top, right - left), height, width)


class Rescale(object):
    def __call__(self, data, height, width):
        return rescale(data, height, width)


class Resize(object):
    def __init__(self, config):
        self.fn = _configured_resize(config)

    def __call__(self, data, height, width):
        return self.fn(data, height, width)


class RandomCrop(object):
    def __init__(self, config):
        self.config = config

    def __call__(self, data, height, width):
        return random_crop(self.config, data, height, width)
