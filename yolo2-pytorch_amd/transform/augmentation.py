"""`transform.augmentation` — RandomRotate(config) and RandomFlipHorizontally(config): the names and call signatures of the reference's plugins
(transform/augmentation.py), for the device collate step.  Both do to the boxes what the reference does, in its operation order and dtypes, draw
the random numbers it draws (`random.uniform` once per rotated sample, `random.random()` once per sample for the flip) and leave the image alone:
`data['rotate']` (the forward matrix of the grown canvas and its size) tells y2_warp_affine_images how to resample the source, `data['flip']`
tells y2_collate_images to read the columns mirrored.

Order: a rotation comes before the resize transform and at most once per sample.  A flip recorded BEFORE the rotation moves into the rotation's
source addressing (`data['rotate']['flip']`); a flip after it is the collate kernel's, in the rotated frame."""
import math
import random

import numpy as np

from transform import frame_size


def rotation_matrix(center, angle, scale=1.0):
    """The documented cv2.getRotationMatrix2D: 2x3 float64, `center` = (x, y), `angle` in degrees, counter-clockwise for a top-left origin."""
    cx, cy = center
    a = angle * math.pi / 180
    alpha, beta = scale * math.cos(a), scale * math.sin(a)
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]], np.float64)


def rotate(data, angle):
    """Rotate the boxes by `angle` degrees about the image centre onto a canvas grown to hold the whole image; every box becomes the hull of its four
    rotated corners.  Records `data['rotate'] = dict(matrix, size, flip)`: the forward 2x3 float64 matrix, the canvas (height, width), and whether the
    source is read mirrored."""
    if 'window' in data:
        raise ValueError('rotate after a resize transform: the window is recorded in the rotated frame, rotate first')
    if 'rotate' in data:
        raise ValueError('rotate: the sample already carries a rotation - one rotation per sample')
    height, width = frame_size(data)
    cy, cx = height / 2, width / 2
    matrix = rotation_matrix((cx, cy), angle)
    r = np.abs(matrix[0, :2])
    canvas_h, canvas_w = np.inner(r, [height, width]), np.inner(r, [width, height])
    matrix[:, 2] += [canvas_w / 2 - cx, canvas_h / 2 - cy]
    size = (int(canvas_h), int(canvas_w))
    if min(size) < 1:
        raise ValueError('rotate: a %dx%d image rotated by %r degrees leaves a %dx%d canvas' % ((height, width, angle) + size))
    lo, hi = data['yx_min'], data['yx_max']
    # the corners (y_min, x_min), (y_max, x_max), (y_max, x_min), (y_min, x_max) of all boxes, as rows (x, y, 1) in the labels' dtype
    corners = np.concatenate([lo, hi, np.stack([hi[:, 0], lo[:, 1]], 1), np.stack([lo[:, 0], hi[:, 1]], 1)], 0)
    points = np.concatenate([corners[:, ::-1], np.ones((len(corners), 1), corners.dtype)], 1)
    moved = np.dot(matrix, points.T).T.astype(corners.dtype)[:, ::-1].reshape(4, -1, 2)          # float64 product, cast back, (y, x) again
    data['yx_min'], data['yx_max'] = moved.min(0), moved.max(0)
    data['rotate'] = dict(matrix=matrix, size=size, flip=bool(data.get('flip', False)))
    if 'flip' in data:
        data['flip'] = False
    return data


class RandomRotate(object):
    """Rotates by random.uniform(low, high) degrees, `[augmentation] random_rotate = low high`."""

    def __init__(self, config):
        self.range = tuple(float(v) for v in config.get('augmentation', 'random_rotate').split())

    def __call__(self, data):
        return rotate(data, random.uniform(*self.range))


def flip_horizontally(data):
    """Mirror the boxes about the vertical centre line.  The flip comes before the resize transform: its window is in the flipped frame."""
    if data['image'].ndim != 3:
        raise ValueError('flip_horizontally: the image must be [h, w, channels]')
    if 'window' in data:
        raise ValueError('flip_horizontally after a resize transform: the window is recorded in the flipped frame, flip first')
    width = frame_size(data)[1]
    x_min, x_max = width - data['yx_max'][:, 1], width - data['yx_min'][:, 1]
    data['yx_min'][:, 1] = x_min
    data['yx_max'][:, 1] = x_max
    data['flip'] = not data.get('flip', False)
    return data


class RandomFlipHorizontally(object):
    """Flips when random.random() exceeds `[augmentation] random_flip_horizontally`."""

    def __init__(self, config):
        self.threshold = config.getfloat('augmentation', 'random_flip_horizontally')

    def __call__(self, data):
        return flip_horizontally(data) if random.random() > self.threshold else data
