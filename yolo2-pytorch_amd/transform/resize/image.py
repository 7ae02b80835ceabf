"""`transform.resize.image` — rescale, fixed, Rescale, Fixed, Resize(config): the names of the reference's test-time resize plugins
(transform/resize/image.py; `resize_test = transform.resize.image.Resize` in config.ini), for the device collate step.

Like transform.resize.label they RECORD instead of resampling: called as `(data, height, width)` on a sample dict whose `image` is the untouched uint8
array (or a utils.data.JpegImage), they leave the pixels alone and note what utils.data.collate_images / to_device have to do.
`rescale` records the whole image as `data['window']` (y2_collate_images stretches it), `fixed` records the aspect-preserving scale, the
interpolation mode and the forward matrix of the reference's cv2.warpAffine as `data['fixed']` (y2_fixed_images resamples through its inverse)."""


def rescale(data, height, width):
    """The whole image, stretched to height x width (cv2.resize(image, (width, height)))."""
    h, w = data['image'].shape[:2]
    data['window'] = (0, 0, int(h), int(w))
    data['flip'] = False
    return data


def fixed(data, height, width):
    """The image scaled by ONE factor into the top-left of a zero height x width canvas: the factor, the mode (0: INTER_AREA, which warpAffine runs as
    INTER_LINEAR, when shrinking; 1: INTER_CUBIC otherwise) and the 2x3 matrix, computed in Python floats as the reference computes them."""
    _height, _width = (int(v) for v in data['image'].shape[:2])
    if _height / _width > height / width:
        scale = height / _height
    else:
        scale = width / _width
    data['fixed'] = dict(scale=scale, mode=0 if scale < 1 else 1, matrix=[[scale, 0.0, 0.0], [0.0, scale, 0.0]])
    return data


class Rescale(object):
    def __call__(self, data, height, width):
        return rescale(data, height, width)


class Fixed(object):
    def __call__(self, data, height, width):
        return fixed(data, height, width)


class Resize(object):
    """`[data] resize`: rescale or fixed."""

    def __init__(self, config):
        name = config.get('data', 'resize')
        fns = dict(rescale=rescale, fixed=fixed)
        if name not in fns:
            raise NotImplementedError('[data] resize = %s: transform.resize.image knows `rescale` and `fixed`' % name)
        self.fn = fns[name]

    def __call__(self, data, height, width):
        return self.fn(data, height, width)
