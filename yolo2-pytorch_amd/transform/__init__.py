"""`transform` — the package of the transform plugins that config.ini names in `[transform]` (`transform.augmentation.RandomFlipHorizontally`,
`transform.resize.label.RandomCrop`, ...); `utils.parse_attr` resolves the dotted names.

Only the transforms whose pixel work the device does are here.  They do the reference's label arithmetic and RECORD the geometry
(`data['rotate']`, `data['window']`, `data['flip']`) instead of resampling `data['image']`; utils.data has the rest of the collate step."""


def frame_size(data):
    """(height, width) of the frame the sample's labels are in: the rotated canvas once `data['rotate']` is recorded, else the image's own size."""
    if 'rotate' in data:
        return data['rotate']['size']
    height, width = data['image'].shape[:2]
    return height, width
