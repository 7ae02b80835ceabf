"""Shared by test_jpeg_cpu.py and test_gpu_jpeg.py: the committed JPEG fixtures (tests/golden/jpeg, written by tools/make_golden_jpeg.py with what Pillow's
libjpeg-turbo decodes from each), the ragged batch layout - odd source and destination offsets, padded row strides, canary bytes everywhere else - and the
host launch.  Nothing here needs Pillow."""
import os

import numpy as np

from conftest import GOLDEN

DIR = os.path.join(GOLDEN, 'jpeg')
CANARY = 0xA5
DESC_BYTES = 4096
# name: (h, w, components, luma h sampling, luma v sampling, restart interval)
SUPPORTED = {
    'c444_16x16': (16, 16, 3, 1, 1, 0),
    'c420_8x8': (8, 8, 3, 2, 2, 0),
    'c420_17x13': (17, 13, 3, 2, 2, 0),
    'c422_33x47': (33, 47, 3, 2, 1, 0),
    'c420_rst_40x56': (40, 56, 3, 2, 2, 2),
    'c420_opt_35x21': (35, 21, 3, 2, 2, 0),
    'c420_q100_64x64': (64, 64, 3, 2, 2, 0),
    'grey_24x24': (24, 24, 1, 1, 1, 0),
    'c420_3x4': (3, 4, 3, 2, 2, 0),
    'c420_2x3': (2, 3, 3, 2, 2, 0),
}
NAMES = list(SUPPORTED)
UNSUPPORTED = ['prog_48x40', 'exif6_20x20']
EINVAL, ENOSUP = -1, -3


def path(name):
    return os.path.join(DIR, name + '.jpg')


def file_bytes(name):
    return np.fromfile(path(name), np.uint8)


_EXPECTED = []


def expected():
    """name -> BGR uint8 [h, w, 3], Pillow's decode; loaded once, shared, never written to."""
    if not _EXPECTED:
        with np.load(os.path.join(DIR, 'expected.npz')) as z:
            _EXPECTED.append({k: z[k] for k in z.files})
        for a in _EXPECTED[0].values():
            a.setflags(write=False)
    return _EXPECTED[0]


def probe(data):
    """(return code, descriptor record) of y2_jpeg_probe_host on a file's bytes."""
    import _hip
    data = np.ascontiguousarray(data, np.uint8)
    desc = np.full(DESC_BYTES, CANARY, np.uint8)
    return _hip.lib().y2_jpeg_probe_host(data.ctypes.data if data.size else None, data.size, desc.ctypes.data), desc


def header(desc):
    """{height, width, components, hmax, vmax, restart interval, scan offset, scan bytes} of a record."""
    return [int(v) for v in desc[:32].view(np.int32)]


def pack(items):
    """items: (file bytes, descriptor) per image.  The tables of one y2_jpeg_decode_images launch: files at odd offsets with canary gaps between them,
    destination images at odd offsets with row strides of 3 w + {0, 1, 7, 16}, the destination filled with the canary."""
    import _hip
    B = len(items)
    src_offset, dst_offset, geom = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros((B, 8), np.int32)
    src, at, pos = [], 0, 0
    for b, (data, desc) in enumerate(items):
        gap = 2 * b + 1 + (at % 2)          # every file starts at an odd offset
        src.append(np.full(gap, CANARY, np.uint8))
        src_offset[b] = at + gap
        src.append(data)
        at += gap + data.size
        h, w = header(desc)[:2]
        stride = 3 * w + (0, 1, 7, 16)[b % 4]
        pos += 2 * b + 1
        pos += int(pos % 2 == 0)          # an odd offset behind a canary gap
        dst_offset[b] = pos
        geom[b] = (stride, h, w, 0, 0, h, w, 0)
        pos += h * stride
    desc = np.stack([d for _, d in items]) if B else np.zeros((0, DESC_BYTES), np.uint8)
    need = int(_hip.lib().y2_jpeg_workspace_bytes(desc.ctypes.data if B else None, B))
    assert need >= 0
    return dict(src=np.concatenate(src + [np.full(3, CANARY, np.uint8)]) if B else np.zeros(0, np.uint8), src_offset=src_offset, desc=desc,
                dst_bytes=pos + 5, dst_offset=dst_offset, geom=geom, ws_bytes=need, B=B)


def aligned(nbytes, fill=0):
    """A uint8 array of nbytes whose first byte is 16-byte aligned."""
    buf = np.full(nbytes + 16, fill, np.uint8)
    start = (-buf.ctypes.data) % 16
    return buf[start:start + nbytes]


def host(group, **change):
    """y2_jpeg_decode_images_host into a canary-filled destination: (return code, destination bytes, status)."""
    import _hip
    g = dict(group, **change)
    dst, ws, status = np.full(g['dst_bytes'], CANARY, np.uint8), aligned(max(g['ws_bytes'], 16)), np.full(g['B'], -7, np.int32)
    p = lambda a: a.ctypes.data if a.size else None
    rc = _hip.lib().y2_jpeg_decode_images_host(p(g['src']), g['src'].size, p(g['src_offset']), p(g['desc']), dst.ctypes.data, dst.size, p(g['dst_offset']),
                                               p(g['geom']), ws.ctypes.data, g['ws_bytes'], p(status), g['B'])
    return rc, dst, status


def image(group, dst, b):
    """Image b of a destination buffer, uint8 [h, w, 3]."""
    stride, h, w = (int(v) for v in group['geom'][b, :3])
    at = int(group['dst_offset'][b])
    rows = np.lib.stride_tricks.as_strided(dst[at:], (h, 3 * w), (stride, 1))
    return rows.reshape(h, w, 3).copy()


def outside(group, dst):
    """The bytes of a destination buffer that belong to no image's 3 w bytes per row (all of them must still be the canary)."""
    mask = np.ones(dst.size, bool)
    for b in range(group['B']):
        stride, h, w = (int(v) for v in group['geom'][b, :3])
        at = int(group['dst_offset'][b])
        for y in range(h):
            mask[at + y * stride:at + y * stride + 3 * w] = False
    return dst[mask]


def all_items():
    return [(file_bytes(name), probe(file_bytes(name))[1]) for name in NAMES]


def sample(name, image):
    """A data sample around one fixture: two boxes inside the image, `image` as given (a JpegImage or the golden array)."""
    h, w = SUPPORTED[name][:2]
    yx_min = np.array([[0.1 * h, 0.1 * w], [0.3 * h, 0.2 * w]], np.float32)
    yx_max = np.array([[0.8 * h, 0.9 * w], [0.9 * h, 0.7 * w]], np.float32)
    return dict(image=image, size=np.array([h, w]), yx_min=yx_min, yx_max=yx_max, cls=np.array([1, 2], np.int64), difficult=np.zeros(2, np.uint8))


PIPELINE_NAMES = ['c444_16x16', 'c420_17x13', 'c422_33x47', 'c420_rst_40x56', 'grey_24x24', 'c420_q100_64x64']


def make_batch(golden, kind, mode, seed=3):
    """One collated batch of PIPELINE_NAMES.  kind: 'jpeg' (every image a JpegImage), 'pixels' (the golden arrays), 'mixed' (alternating).
    mode: 'plain' (flips), 'rotated' (RandomRotate + flips), 'jittered' (the same with the colour jitter).  The same seed draws the same augmentations
    whatever the kind: the label transforms read the shape only."""
    import random

    import jitter_cases as jc
    import transform.augmentation as ta
    import transform.image
    import transform.resize.label
    import utils.data
    config = jc.config_of(golden)
    random.seed(seed)
    np.random.seed(seed)
    rotate, flip = ta.RandomRotate(config), ta.RandomFlipHorizontally(config)
    samples = []
    for k, name in enumerate(PIPELINE_NAMES):
        compressed = kind == 'jpeg' or (kind == 'mixed' and k % 2 == 0)
        data = sample(name, utils.data.probe_jpeg(file_bytes(name)) if compressed else expected()[name].copy())
        assert compressed == isinstance(data['image'], utils.data.JpegImage)
        samples.append(flip(rotate(data)) if mode != 'plain' and k != 3 else (ta.flip_horizontally(data) if k % 2 else data))
    kwargs = dict(transform_image=transform.image.get_transform(config, jc.IMAGE_TRAIN.split())) if mode == 'jittered' else {}
    collate = utils.data.Collate(transform.resize.label.RandomCrop(config), [(40, 56)], maintain=1, **kwargs)
    return collate(samples)
