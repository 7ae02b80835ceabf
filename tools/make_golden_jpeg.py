"""Writes tests/golden/jpeg/*.jpg and tests/golden/jpeg/expected.npz: tiny JPEG files at the edges of the device decoder (include/yolo2_hip.h:
y2_jpeg_decode_images) and what Pillow's libjpeg-turbo decodes from each, as BGR uint8 [h, w, 3] (the grey file: its `L` decode in all three channels).
Needs Pillow built on libjpeg-turbo; seeded.  The two files the probe must refuse (progressive; Exif orientation 6) are decoded too, the second also as
cv2.imread would return it (`<name>.oriented`: the orientation applied), for the host path of utils.data.read_image.

    python tools/make_golden_jpeg.py
"""
import io
import os

import numpy as np
from PIL import Image, ImageOps, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'jpeg')

# name: (h, w, kind of content, save options).  subsampling: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0
FIXTURES = [
    ('c444_16x16', 16, 16, 'scene', dict(quality=90, subsampling=0)),
    ('c420_8x8', 8, 8, 'scene', dict(quality=85, subsampling=2)),
    ('c420_17x13', 17, 13, 'scene', dict(quality=85, subsampling=2)),
    ('c422_33x47', 33, 47, 'scene', dict(quality=80, subsampling=1)),
    ('c420_rst_40x56', 40, 56, 'scene', dict(quality=85, subsampling=2, restart_marker_blocks=2)),
    ('c420_opt_35x21', 35, 21, 'scene', dict(quality=75, subsampling=2, optimize=True)),
    ('c420_q100_64x64', 64, 64, 'noise', dict(quality=100, subsampling=2)),
    ('grey_24x24', 24, 24, 'grey', dict(quality=85)),
    ('c420_3x4', 3, 4, 'noise', dict(quality=90, subsampling=2)),
    ('c420_2x3', 2, 3, 'noise', dict(quality=90, subsampling=2)),
    ('prog_48x40', 48, 40, 'scene', dict(quality=85, subsampling=2, progressive=True)),
    ('exif6_20x20', 20, 20, 'scene', dict(quality=85, subsampling=2, orientation=6)),
]
UNSUPPORTED = ('prog_48x40', 'exif6_20x20')


def content(rng, h, w, kind):
    """RGB (or grey) uint8: a coloured gradient with hard-edged patches and a little noise (chroma edges exercise the upsampling filters), or noise."""
    if kind == 'noise':
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([255 * x / max(w - 1, 1), 255 * y / max(h - 1, 1), 255 * (1 - (x + y) / max(h + w - 2, 1))], -1)
    for _ in range(4):
        y0, x0 = rng.randint(0, h), rng.randint(0, w)
        img[y0:y0 + rng.randint(1, h // 2 + 2), x0:x0 + rng.randint(1, w // 2 + 2)] = rng.randint(0, 256, 3)
    img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
    return img[..., 1] if kind == 'grey' else img


def bgr(image):
    return np.ascontiguousarray(np.asarray(image.convert('RGB'))[..., ::-1])


def main():
    assert features.check_feature('libjpeg_turbo'), 'the arbiter is libjpeg-turbo: this Pillow is built on another decoder'
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.RandomState(20)
    expected = {}
    for name, h, w, kind, options in FIXTURES:
        options = dict(options)
        orientation = options.pop('orientation', None)
        if orientation is not None:
            exif = Image.Exif()
            exif[0x0112] = orientation
            options['exif'] = exif.tobytes()
        buf = io.BytesIO()
        Image.fromarray(content(rng, h, w, kind)).save(buf, 'JPEG', **options)
        data = buf.getvalue()
        with open(os.path.join(OUT, name + '.jpg'), 'wb') as f:
            f.write(data)
        image = Image.open(io.BytesIO(data))
        expected[name] = bgr(image)
        assert expected[name].shape == (h, w, 3)
        if orientation is not None:
            expected[name + '.oriented'] = bgr(ImageOps.exif_transpose(image))
        markers = [m for m in (b'\xff\xc0', b'\xff\xc2', b'\xff\xdd') if m in data]
        print('%-18s %5d bytes  %s' % (name, len(data), ' '.join(m.hex() for m in markers)))
    np.savez_compressed(os.path.join(OUT, 'expected.npz'), **expected)
    total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print('%d files, %d bytes' % (len(os.listdir(OUT)), total))


if __name__ == '__main__':
    main()
