"""`transform.augmentation` — RandomFlipHorizontally(config): the name and call signature of the reference's plugin (transform/augmentation.py),
for the device collate step.  The boxes are mirrored in float32 as the reference mirrors them, `random.random()` is drawn once per sample, and the
image is left alone: `data['flip']` tells y2_collate_images to read the columns mirrored.

RandomRotate resamples the image itself (cv2.warpAffine) and stays host work: it is not part of this module."""
import random


def flip_horizontally(data):
    """Mirror the boxes about the vertical centre line.  The flip comes before the resize transform: its window is in the flipped frame."""
    if data['image'].ndim != 3:
        raise ValueError('flip_horizontally: the image must be [h, w, channels]')
    if 'window' in data:
        raise ValueError('flip_horizontally after a resize transform: the window is recorded in the flipped frame, flip first')
    width = data['image'].shape[1]
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
