"""`utils.data` — the collate step of the reference's data pipeline (utils/data.py:29-42, 93-141), split at the process boundary.

`Collate` runs in DataLoader worker processes, which must not touch the GPU: it chooses the batch's size (`next_size`: the reference's schedule), runs the
resize transform on the LABELS (transform.resize.label: the geometry is recorded, no pixel is touched), pads the labels (`padding_labels`) with
zero rows and packs the untouched uint8 images into one byte buffer with an offset and a geometry row per image.  It returns no `tensor`.
`to_device` runs in the main process: at most one copy per tensor, then ONE y2_collate_images launch (crop, flip, resize, channel swap, ToTensor +
Normalize as a table) writes `batch['tensor']`, the fp32 [B,3,H,W] input of the network.  On 'cpu' it runs y2_collate_images_host, the
bit-identical host function.

A batch in which a sample went through transform.augmentation.RandomRotate takes one launch more: `Collate` adds the tables of
y2_warp_affine_images (`src_offset`, `src_geom`, `warp`: the inverse matrices, `rot_bytes`, `rot_size`), `offset` / `geom` then describe the ROTATED
images inside an intermediate device buffer, and `to_device` launches the warp in front of the collate kernel.  A batch without a rotated sample
is untouched by all this: the same keys, the same bytes, one launch.

With `transform_image` (transform.image.get_transform: RandomBlur, the HSV chain, RandomGamma) `Collate` draws every sample's jitter after its resize
transform and adds `jitter`, `hsv_tab` (when the sequence goes through HSV) and `lut_b`, and `to_device` launches y2_collate_jitter_images IN PLACE
of y2_collate_images (behind the warp launch, when there is one).  Without it, or with a sequence that is only BGR2RGB, nothing changes.

What ships to the device is the source pixels as cv2.imread returned them - a quarter to a third of the bytes of the finished fp32 tensor.

`Dataset` (the reference's class, utils/data.py:53-90) reads a sample's file with `read_image`: a baseline JPEG that y2_jpeg_probe_host accepts stays
COMPRESSED - a `JpegImage` holding the file's bytes and its descriptor, with the `.shape`, `.ndim` and `.dtype` the label transforms read - and anything
else is decoded on the host as before.  `Collate` packs the pixels of host-decoded samples first, exactly as above, and gives every JpegImage sample
`offset` / `geom` rows that point at space reserved BEHIND them, which only exists on the device; the files' bytes travel as `jpeg`, `jpeg_offset`,
`jpeg_desc`.  `to_device` allocates the whole pixel buffer, copies the host part and the files (about a tenth of the pixel bytes), launches
y2_jpeg_decode_images in front of the launches above and adds `jpeg_status` without looking at it.  A batch without a JpegImage is untouched by all
this: the same keys, the same bytes, the same launches.

`collate_images` is the label-less counterpart of `Collate.__call__` for the test path (detect.Detector): pictures through a transform of
transform.resize.image, packed by the same code (`pack_images`).  With the `fixed` resize it adds `fixed_geom` / `fixed_inv`, and `to_device` launches
y2_fixed_images (the aspect-preserving warp, linear or cubic, fused with the channel swap and the level table) IN PLACE of y2_collate_images."""
import copy
import os
import pickle
import random

import numpy as np
import torch

import _hip
from transform import frame_size

LABELS = 'yx_min, yx_max, cls, difficult'.split(', ')


def padding_labels(data, dim, labels=LABELS):
    """The labels of one sample as arrays of `dim` boxes: the sample's own boxes first, zero rows behind them (the reference's helper of this name)."""
    for key in labels:
        label = data[key]
        padded = np.zeros((dim,) + label.shape[1:], label.dtype)
        padded[:len(label)] = label
        data[key] = padded
    return data


def load_pickles(paths):
    """The samples of the cache files (the reference's helper of this name)."""
    data = []
    for path in paths:
        with open(path, 'rb') as f:
            data += pickle.load(f)
    return data


class JpegImage(object):
    """A baseline JPEG file the device will decode (y2_jpeg_decode_images): `data`, the file's bytes (uint8 [n]), and `desc`, the record
    y2_jpeg_probe_host filled (uint8 [Y2_JPEG_DESC_BYTES]).  Stands where the decoded array would stand in `data['image']`: shape, ndim and dtype are
    all the label transforms read of it."""
    ndim = 3
    dtype = np.dtype(np.uint8)

    def __init__(self, data, desc):
        self.data, self.desc = data, desc

    @property
    def shape(self):
        height, width = self.desc[:8].view(np.int32)
        return (int(height), int(width), 3)

    def decode(self):
        """The pixels, BGR uint8 [h, w, 3], by the host function (bit-identical to the device); raises when the stream is damaged."""
        h, w, _ = self.shape
        lib = _hip.lib()
        ws = torch.empty(max(int(lib.y2_jpeg_workspace_bytes(self.desc.ctypes.data, 1)), 16), dtype=torch.uint8)
        out, status = np.empty((h, w, 3), np.uint8), np.zeros(1, np.int32)
        zero, geom = np.zeros(1, np.int64), np.array([[3 * w, h, w, 0, 0, h, w, 0]], np.int32)
        _hip.check(lib.y2_jpeg_decode_images_host(self.data.ctypes.data, self.data.size, zero.ctypes.data, self.desc.ctypes.data, out.ctypes.data, out.size,
                                                  zero.ctypes.data, geom.ctypes.data, ws.data_ptr(), ws.numel(), status.ctypes.data, 1), 'y2_jpeg_decode_images_host')
        if status[0]:
            raise ValueError('JpegImage.decode: damaged stream (status %d)' % status[0])
        return out


def probe_jpeg(data):
    """The JpegImage of a file's bytes (uint8 [n]) when the device decoder supports it, else None (not a JPEG, damaged headers, or a kind of JPEG
    include/yolo2_hip.h lists as not supported)."""
    data = np.ascontiguousarray(data, np.uint8).reshape(-1)
    desc = np.zeros(_hip.JPEG_DESC_BYTES, np.uint8)
    if data.size == 0 or _hip.lib().y2_jpeg_probe_host(data.ctypes.data, data.size, desc.ctypes.data) != 0:
        return None
    return JpegImage(data, desc)


def _orient(image, orientation):
    """An array turned as its Exif orientation says (what cv2.imread does on its own; Pillow does not)."""
    if orientation in (2, 4, 5, 7):
        image = image[:, ::-1]
    if orientation in (3, 4):
        image = image[::-1, ::-1]
    elif orientation in (6, 7):
        image = np.rot90(image, -1)
    elif orientation in (5, 8):
        image = np.rot90(image, 1)
    return np.ascontiguousarray(image)


def imread_host(path):
    """cv2.imread(path) - BGR uint8 [h, w, 3] - or, where cv2 does not import, the same from Pillow: RGB -> BGR, the Exif orientation applied."""
    try:
        import cv2
    except ImportError:
        from PIL import Image
        with Image.open(path) as image:
            orientation = image.getexif().get(0x0112, 1)
            return _orient(np.asarray(image.convert('RGB'))[..., ::-1], orientation)
    return cv2.imread(path)


def read_image(path, device_decode=True):
    """What `data['image']` becomes: a JpegImage when y2_jpeg_probe_host accepts the file (the device decodes it), else the decoded array.
    device_decode=False: always the array."""
    if device_decode:
        image = probe_jpeg(np.fromfile(path, np.uint8))
        if image is not None:
            return image
    return imread_host(path)


class Dataset(torch.utils.data.Dataset):
    """The reference's class of this name (utils/data.py:53-90): a deep copy of sample `index`, its image read (`read_image` in place of cv2.imread),
    `data['size']`, the transform on the labels, `cls` one-hot when `one_hot` (the number of classes) is given; the sample that raised is pickled
    into `dir` before the exception goes on.  device_decode: leave supported JPEG files compressed for the device."""

    def __init__(self, data, transform=lambda data: data, one_hot=None, shuffle=False, dir=None, device_decode=True):
        self.data = data
        if shuffle:
            random.shuffle(self.data)
        self.transform, self.one_hot, self.dir, self.device_decode = transform, one_hot, dir, device_decode

    def __len__(self):
        return len(self.data)

    def __getitem__(self, index):
        data = copy.deepcopy(self.data[index])
        try:
            image = read_image(data['path'], self.device_decode)
            data['image'] = image
            data['size'] = np.array(image.shape[:2])
            data = self.transform(data)
            if self.one_hot is not None:
                data['cls'] = np.eye(self.one_hot, dtype=np.float32)[np.asarray(data['cls'], np.int64)]          # (OneHotEncoder(one_hot, dtype=np.float32), dense)
        except Exception:
            if self.dir is not None:
                os.makedirs(self.dir, exist_ok=True)
                with open(os.path.join(self.dir, '%s.%s.pkl' % (type(self).__module__, type(self).__name__)), 'wb') as f:
                    pickle.dump(data, f)
            raise
        return data


def check_geometry(offset, geom, nbytes):
    """The tables of y2_collate_images against the byte buffer they index (host arrays): every image inside the buffer, every window inside its image."""
    offset, geom = np.asarray(offset, np.int64), np.asarray(geom, np.int64)
    if geom.ndim != 2 or geom.shape[1] != 8 or offset.shape != (geom.shape[0],):
        raise ValueError('collate: offset must be [B] and geom [B, 8] (got %s and %s)' % (offset.shape, geom.shape))
    stride, src_h, src_w, y0, x0, h, w, flip = geom.T
    bad = ((offset < 0) | (src_h < 1) | (src_w < 1) | (stride < 3 * src_w) | (h < 1) | (w < 1) | (y0 < 0) | (x0 < 0) | (y0 + h > src_h) | (x0 + w > src_w)
           | ((flip != 0) & (flip != 1)) | (offset + (src_h - 1) * stride + 3 * src_w > nbytes))
    if bad.any():
        b = int(np.argmax(bad))
        raise ValueError('collate: image %d: window or image outside its buffer (offset %d of %d bytes, geom %s)' % (b, offset[b], nbytes, geom[b].tolist()))


def invert_affine(matrix):
    """The inverse of a 2x3 affine map as 6 float64 (A0 .. A5: destination -> source), in the operation order of cv2.warpAffine's own inversion."""
    M0, M1, M2, M3, M4, M5 = (float(v) for v in np.asarray(matrix, np.float64).reshape(6))
    D = M0 * M4 - M1 * M3
    D = 1.0 / D if D != 0 else 0.0
    A0, A4, A1, A3 = M4 * D, M0 * D, -M1 * D, -M3 * D
    return np.array([A0, A1, -A0 * M2 - A1 * M5, A3, A4, -A3 * M2 - A4 * M5], np.float64)


def check_warp(src_offset, src_geom, warp, src_bytes, offset, geom, rot_bytes):
    """The tables of y2_warp_affine_images against the two byte buffers (host arrays): every source inside `src_bytes`, every destination inside
    `rot_bytes`, dimensions and matrix entries in the ranges of include/yolo2_hip.h."""
    src_offset, src_geom, offset, geom = (np.asarray(a, np.int64) for a in (src_offset, src_geom, offset, geom))
    warp = np.asarray(warp, np.float64)
    B = len(geom)
    if src_geom.shape != (B, 4) or src_offset.shape != (B,) or warp.shape != (B, 6) or geom.shape != (B, 8) or offset.shape != (B,):
        raise ValueError('warp: src_offset must be [B], src_geom [B, 4], warp [B, 6] beside offset [B] and geom [B, 8]')
    stride, src_h, src_w, flip = src_geom.T
    dstride, dst_h, dst_w = geom.T[:3]
    limit = _hip.WARP_MAX_DIM
    with np.errstate(invalid='ignore'):
        in_range = (np.abs(warp[:, [0, 1, 3, 4]]) <= 4).all(1) & (np.abs(warp[:, [2, 5]]) <= 2 ** 19).all(1)          # (a NaN is out of range)
    bad = ((src_offset < 0) | (src_h < 1) | (src_h > limit) | (src_w < 1) | (src_w > limit) | (stride < 3 * src_w) | ((flip != 0) & (flip != 1))
           | (src_offset + (src_h - 1) * stride + 3 * src_w > src_bytes)
           | (offset < 0) | (dst_h < 1) | (dst_h > limit) | (dst_w < 1) | (dst_w > limit) | (dstride < 3 * dst_w)
           | (offset + (dst_h - 1) * dstride + 3 * dst_w > rot_bytes) | ~in_range)
    if bad.any():
        b = int(np.argmax(bad))
        raise ValueError('warp: image %d: source or rotated image outside its buffer, or matrix out of range (src_offset %d of %d bytes, src_geom %s, '
                         'offset %d of %d bytes, geom %s, warp %s)' % (b, src_offset[b], src_bytes, src_geom[b].tolist(), offset[b], rot_bytes, geom[b, :3].tolist(), warp[b].tolist()))


def check_jitter(jitter, hsv_tab, lut_b, B):
    """The tables of y2_collate_jitter_images (host arrays; hsv_tab may be None): shapes, blur sizes in 1 .. Y2_JITTER_MAX_BLUR, hsv 0 or 1."""
    jitter = np.asarray(jitter)
    if jitter.shape != (B, 4) or jitter.dtype != np.int32 or tuple(lut_b.shape) != (B, 3, 256) or (hsv_tab is not None and tuple(hsv_tab.shape) != (B, 3, 256)):
        raise ValueError('jitter: jitter must be int32 [B, 4], hsv_tab uint8 [B, 3, 256] and lut_b fp32 [B, 3, 256]')
    kx, ky, hsv, zero = jitter.T.astype(np.int64)
    limit = _hip.JITTER_MAX_BLUR
    bad = (kx < 1) | (kx > limit) | (ky < 1) | (ky > limit) | ((hsv != 0) & (hsv != 1)) | (zero != 0) | ((hsv != 0) & (hsv_tab is None))
    if bad.any():
        b = int(np.argmax(bad))
        raise ValueError('jitter: image %d: blur size outside 1 .. %d, hsv not 0 / 1 or hsv without hsv_tab (jitter %s)' % (b, limit, jitter[b].tolist()))


def check_fixed(offset, fixed_geom, fixed_inv, nbytes):
    """The tables of y2_fixed_images against the byte buffer they index (host arrays): every image inside the buffer, dimensions, modes and matrix
    entries in the ranges of include/yolo2_hip.h."""
    offset, geom, inv = np.asarray(offset, np.int64), np.asarray(fixed_geom, np.int64), np.asarray(fixed_inv, np.float64)
    B = len(geom)
    if geom.ndim != 2 or geom.shape[1] != 4 or offset.shape != (B,) or inv.shape != (B, 6):
        raise ValueError('fixed: offset must be [B], fixed_geom [B, 4] and fixed_inv [B, 6] (got %s, %s and %s)' % (offset.shape, geom.shape, inv.shape))
    stride, src_h, src_w, mode = geom.T
    limit = _hip.WARP_MAX_DIM
    with np.errstate(invalid='ignore'):
        in_range = (np.abs(inv[:, [0, 1, 3, 4]]) <= 4).all(1) & (np.abs(inv[:, [2, 5]]) <= 2 ** 19).all(1)          # (a NaN is out of range)
    bad = ((offset < 0) | (src_h < 1) | (src_h > limit) | (src_w < 1) | (src_w > limit) | (stride < 3 * src_w) | ((mode != 0) & (mode != 1))
           | (offset + (src_h - 1) * stride + 3 * src_w > nbytes) | ~in_range)
    if bad.any():
        b = int(np.argmax(bad))
        raise ValueError('fixed: image %d: image outside its buffer, mode not 0 / 1 or matrix out of range (offset %d of %d bytes, fixed_geom %s, fixed_inv %s)'
                         % (b, offset[b], nbytes, geom[b].tolist(), inv[b].tolist()))


ROT_ROW_ALIGN, ROT_IMAGE_ALIGN = 16, 64     # the layout of the rotated images is Collate's: rows and images start where the warp kernel's 12-byte stores are aligned


def _window_row(data):
    """Columns 3-7 of a sample's geometry row: the recorded window and flip; a sample of transform.resize.image.fixed shows its whole image."""
    if 'window' not in data and 'fixed' in data:
        h, w = data['image'].shape[:2]
        return (0, 0, int(h), int(w), 0)
    return tuple(data['window']) + (int(bool(data['flip'])),)


def pack_images(samples):
    """The images of prepared samples as the tables of y2_collate_images: (raw uint8 [n], offset int64 [B], geom int32 [B, 8], the size of the pixel
    buffer in bytes, the JPEG tables as a dict).  Host-decoded pixels are packed back to back; JpegImage samples get rows that point at space reserved
    behind them, which only exists on the device."""
    offset = np.zeros(len(samples), np.int64)
    geom = np.zeros((len(samples), 8), np.int32)
    pos = 0
    compressed = [b for b, data in enumerate(samples) if isinstance(data['image'], JpegImage)]
    for b, data in enumerate(samples):
        if b not in compressed:
            h, w = data['image'].shape[:2]
            offset[b] = pos
            geom[b] = (3 * w, h, w) + _window_row(data)
            pos += 3 * h * w
    raw = np.empty(pos, np.uint8)
    for b, data in enumerate(samples):
        if b not in compressed:
            raw[offset[b]:offset[b] + data['image'].size] = data['image'].reshape(-1)
    extra = {}
    if compressed:
        # the decoded images live behind the host's pixels, on the device only: rows and images start where the decoder's 12-byte stores are aligned
        for b in compressed:
            h, w = samples[b]['image'].shape[:2]
            stride = -(-3 * w // ROT_ROW_ALIGN) * ROT_ROW_ALIGN
            pos = -(-pos // ROT_IMAGE_ALIGN) * ROT_IMAGE_ALIGN
            offset[b] = pos
            geom[b] = (stride, h, w) + _window_row(samples[b])
            pos += h * stride
        files = [samples[b]['image'] for b in compressed]
        jpeg_offset = np.cumsum([0] + [f.data.size for f in files]).astype(np.int64)
        desc = np.stack([f.desc for f in files])
        need = int(_hip.lib().y2_jpeg_workspace_bytes(desc.ctypes.data, len(files)))
        if need < 0:
            raise ValueError('collate: a JpegImage carries a descriptor that y2_jpeg_probe_host did not fill')
        extra.update(jpeg=torch.from_numpy(np.concatenate([f.data for f in files])), jpeg_offset=torch.from_numpy(jpeg_offset[:-1].copy()),
                     jpeg_desc=torch.from_numpy(desc), jpeg_index=torch.from_numpy(np.array(compressed, np.int64)),
                     jpeg_dst=torch.from_numpy(offset[compressed]), jpeg_geom=torch.from_numpy(geom[compressed]), jpeg_ws_bytes=need, raw_bytes=pos)
    return raw, offset, geom, pos, extra


class Collate(object):
    """The worker-process half of the collate step, with the constructor and the size schedule of the reference's class of this name.
    resize: transform.resize.label.Rescale / Resize / RandomCrop, called as resize(data, height, width): resizes the labels, records the geometry.
    sizes: the (height, width) pairs a batch's size is drawn from with random.choice; a drawn size serves `maintain` further batches.
    swap_rb: the images are BGR (cv2.imread) and the network reads RGB (transform.image.BGR2RGB).
    normalize: (mean, std) of transform.image.Normalize after ToTensor; None: ToTensor only.
    transform_image: the object of transform.image.get_transform; called once per sample after its resize transform (the reference's order of
    draws).  `swap_rb` then comes from its sequence.  None: no jitter.
    dir: where the sample that raised is pickled before the exception goes on."""

    def __init__(self, resize, sizes, maintain=1, swap_rb=True, normalize=(0.5, 1.0), dir=None, transform_image=None):
        if maintain <= 0:
            raise ValueError('Collate: maintain must be positive')
        self.resize, self.sizes, self.maintain, self.dir = resize, sizes, maintain, dir
        self.transform_image = transform_image
        self.swap_rb = bool(swap_rb) if transform_image is None else bool(transform_image.swap_rb)
        self.normalize = None if normalize is None else (float(normalize[0]), float(normalize[1]))
        self._repeats_left = 0

    def next_size(self):
        if self._repeats_left == 0:
            self.size = random.choice(self.sizes)
            self._repeats_left = self.maintain
        else:
            self._repeats_left -= 1
        return self.size

    def _prepare(self, data, height, width, dim):
        data = padding_labels(self.resize(data, height, width), dim)
        image = data['image']
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
            raise ValueError('collate: an image must be uint8 [h, w, 3] (got %s %s)' % (image.dtype, image.shape))
        if self.transform_image is not None and self.transform_image.active:
            data['jitter'] = self.transform_image()
        return data

    def _keep(self, data):
        if self.dir is not None:
            os.makedirs(self.dir, exist_ok=True)
            with open(os.path.join(self.dir, '%s.%s.pkl' % (type(self).__module__, type(self).__name__)), 'wb') as f:
                pickle.dump(data, f)

    def __call__(self, batch):
        height, width = self.next_size()
        dim = max(len(data['cls']) for data in batch)
        samples = []
        for data in batch:
            try:
                samples.append(self._prepare(data, height, width, dim))
            except Exception:
                self._keep(data)
                raise
        out = {key: torch.from_numpy(np.stack([data[key] for data in samples])) for key in LABELS}      # (what default_collate makes of numpy arrays)
        raw, offset, geom, pos, extra = pack_images(samples)
        if any('rotate' in data for data in samples):
            # every sample goes through the warp stage (an un-rotated one with the identity, an exact copy): what was packed above is its source, and
            # offset / geom move on to the rotated images inside the intermediate buffer
            src_offset, src_geom = offset, np.zeros((len(samples), 4), np.int32)
            offset, warp = np.zeros(len(samples), np.int64), np.zeros((len(samples), 6), np.float64)
            pos = 0
            for b, data in enumerate(samples):
                rotate = data.get('rotate')
                h, w = frame_size(data)
                stride = -(-3 * w // ROT_ROW_ALIGN) * ROT_ROW_ALIGN
                src_geom[b] = tuple(geom[b, :3]) + (int(rotate['flip']) if rotate else 0,)
                warp[b] = invert_affine(rotate['matrix']) if rotate else (1, 0, 0, 0, 1, 0)
                offset[b] = pos
                geom[b, :3] = (stride, h, w)
                pos += -(-h * stride // ROT_IMAGE_ALIGN) * ROT_IMAGE_ALIGN
            check_warp(src_offset, src_geom, warp, extra.get('raw_bytes', raw.size), offset, geom, pos)
            extra.update(src_offset=torch.from_numpy(src_offset), src_geom=torch.from_numpy(src_geom), warp=torch.from_numpy(warp), rot_bytes=pos,
                         rot_size=(int(geom[:, 1].max()), int(geom[:, 2].max())))
        if self.transform_image is not None and self.transform_image.active:
            records = [data['jitter'] for data in samples]
            jitter = np.array([tuple(r['blur']) + (int(r['hsv']), 0) for r in records], np.int32).reshape(-1, 4)
            level = level_table(self.normalize, 'cpu')
            extra['jitter'] = torch.from_numpy(jitter)
            if self.transform_image.hsv:
                extra['hsv_tab'] = torch.from_numpy(np.stack([np.stack([r['h'], r['s'], r['v']]) for r in records]).astype(np.uint8))
            extra['lut_b'] = torch.stack([level[:, torch.from_numpy(r['gamma'].astype(np.int64))] for r in records])      # lut_b[b, c, l] = level[c, gamma_b[l]]
            check_jitter(jitter, extra.get('hsv_tab'), extra['lut_b'], len(samples))
        check_geometry(offset, geom, pos)
        out.update(raw=torch.from_numpy(raw), offset=torch.from_numpy(offset), geom=torch.from_numpy(geom), size=(height, width),
                   swap_rb=self.swap_rb, normalize=self.normalize)
        out.update(extra)
        return out


def collate_images(samples, resize, height, width, swap_rb=True, normalize=(0.5, 1.0)):
    """The label-less counterpart of Collate.__call__ (the test path: detect.Detector): `samples` are dicts whose `image` is a uint8 [h, w, 3] array or a
    JpegImage, `resize` one of transform.resize.image (called as resize(data, height, width): it records, it does not resample).  Returns the batch
    dict of to_device - `raw` / `offset` / `geom` and the JPEG tables packed by the code of Collate, `size`, `swap_rb`, `normalize` - and, when the
    samples carry `fixed`, `fixed_geom` int32 [B, 4] {row_stride_bytes, src_h, src_w, mode} and `fixed_inv` float64 [B, 6], the inverse of each
    recorded matrix (invert_affine): to_device then launches y2_fixed_images in place of y2_collate_images.  A batch that mixes `fixed` and windowed
    samples raises."""
    prepared = []
    for data in samples:
        data = resize(data, height, width)
        image = data['image']
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
            raise ValueError('collate_images: an image must be uint8 [h, w, 3] (got %s %s)' % (image.dtype, image.shape))
        prepared.append(data)
    fixed = ['fixed' in data for data in prepared]
    if any(fixed) and (not all(fixed) or any('window' in data for data in prepared)):
        raise ValueError('collate_images: the batch mixes `fixed` and windowed samples (one resize per batch)')
    raw, offset, geom, pos, extra = pack_images(prepared)
    check_geometry(offset, geom, pos)
    out = dict(raw=torch.from_numpy(raw), offset=torch.from_numpy(offset), geom=torch.from_numpy(geom), size=(int(height), int(width)),
               swap_rb=bool(swap_rb), normalize=None if normalize is None else (float(normalize[0]), float(normalize[1])))
    out.update(extra)
    if any(fixed):
        fixed_geom = np.ascontiguousarray(geom[:, [0, 1, 2, 2]])
        fixed_geom[:, 3] = [int(data['fixed']['mode']) for data in prepared]
        fixed_inv = np.stack([invert_affine(data['fixed']['matrix']) for data in prepared]).reshape(-1, 6)
        check_fixed(offset, fixed_geom, fixed_inv, pos)
        out.update(fixed_geom=torch.from_numpy(fixed_geom), fixed_inv=torch.from_numpy(fixed_inv))
    return out


_LUT = {}


def level_table(normalize, device):
    """[3, 256] fp32: ToTensor (`.float().div(255)`) and Normalize (`sub(mean).div(std)`, one mean and std for the three channels:
    transform/image.py:101-105) of every uint8 level, computed with torch's own operations on the CPU - bit-identical to the reference's per-pixel
    arithmetic by construction.  Cached per (mean, std, device).  The FIRST call for a key on a GPU copies the table from pageable memory, which
    blocks the host and cannot be captured: call it (or to_device) once per (normalize, device) before a loop that must not synchronise."""
    normalize = None if normalize is None else (float(normalize[0]), float(normalize[1]))
    device = torch.device(device)
    key = (normalize, str(device))
    lut = _LUT.get(key)
    if lut is None:
        lut = torch.arange(256).float().div(255)
        if normalize is not None:
            mean, std = normalize
            lut = (lut - mean) / std
        lut = _LUT[key] = lut.view(1, 256).repeat(3, 1).contiguous().to(device)
    return lut


def to_device(batch, device=None, out=None, rot=None):
    """The main-process half of the collate step: a copy of `batch` (the dict of Collate) with every tensor on `device` - at most one copy each,
    non_blocking from pinned memory, no synchronisation once level_table() has met this (normalize, device) - and `tensor` [B,3,H,W] fp32 written by one y2_collate_images launch on the current
    stream (device 'cpu': y2_collate_images_host).  device=None: where `raw` is when that is a GPU, else the current GPU, else the CPU.
    `out`: the destination (e.g. the static input buffer of a captured graph) instead of a fresh tensor.  `batch['lut']` ([3,256] fp32), when
    present, replaces the ToTensor + Normalize table (any per-level map, e.g. a gamma curve).  The tables are checked here while they are host
    memory; tables that arrive on the device are the caller's.
    A batch with `warp` (a sample was rotated) takes TWO launches: y2_warp_affine_images writes every rotated uint8 image into an intermediate buffer
    of `batch['rot_bytes']` bytes - `rot`, a contiguous uint8 tensor of at least that size on `device` (a captured graph's static buffer), or a fresh
    torch.empty - and y2_collate_images reads that buffer instead of `raw`.  The result carries it as `rot`.  `batch['fill']` (0xC2C1C0, one byte per
    source channel; default 0, what the reference passes) is the level outside the source.  Without `warp`, `rot` is not touched.
    A batch with `jitter` (Collate had a transform_image) launches y2_collate_jitter_images instead of y2_collate_images: `jitter` int32 [B, 4],
    `hsv_tab` uint8 [B, 3, 256] (optional) and `lut_b` fp32 [B, 3, 256], the per-image table that takes the place of `lut`.
    A batch with `jpeg` (a sample's image is a JpegImage) takes y2_jpeg_decode_images (three kernels; 'cpu': y2_jpeg_decode_images_host) in front of all
    that: the pixel buffer of `batch['raw_bytes']` bytes is allocated on `device`, the host-decoded pixels of `raw` are copied to its front, the files
    (`jpeg`, `jpeg_offset`, `jpeg_desc`) follow, and the decoder writes the JpegImage samples where `jpeg_dst` / `jpeg_geom` (their `offset` / `geom`
    rows before any rotation) say.  The result carries the buffer as `raw` and `jpeg_status` (int32, one per `jpeg_index` entry, 0 = decoded: the
    status column of include/yolo2_hip.h) on `device`, un-synchronised: the caller decides when to look at it.
    A batch with `fixed_geom` (collate_images with transform.resize.image.fixed: the test-time aspect-preserving resize) launches y2_fixed_images IN
    PLACE of y2_collate_images ('cpu': y2_fixed_images_host), behind the JPEG decode when there is one: `fixed_geom` int32 [B, 4] and `fixed_inv`
    float64 [B, 6] are checked while they are host memory (ValueError, nothing is written).  Such a batch with `warp` or `jitter` raises: the test
    path has neither."""
    raw = batch['raw']
    if device is None:
        device = raw.device if raw.is_cuda else torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    H, W = (int(v) for v in batch['size'])
    warped = 'warp' in batch
    compressed = 'jpeg' in batch
    fixed = 'fixed_geom' in batch
    if fixed and (warped or 'jitter' in batch):
        raise ValueError('to_device: a batch with fixed_geom (the test-time `fixed` resize) cannot carry warp or jitter')
    source = int(batch['raw_bytes']) if compressed else raw.numel()      # the buffer of source pixels: `raw`, and behind it the images the device decodes
    pixels = int(batch['rot_bytes']) if warped else source               # the buffer that offset / geom index
    if not batch['geom'].is_cuda and not batch['offset'].is_cuda:
        check_geometry(batch['offset'].numpy(), batch['geom'].numpy(), pixels)
        if warped and not any(batch[k].is_cuda for k in ('src_offset', 'src_geom', 'warp')):
            check_warp(batch['src_offset'].numpy(), batch['src_geom'].numpy(), batch['warp'].numpy(), source, batch['offset'].numpy(), batch['geom'].numpy(), pixels)
    jittered = 'jitter' in batch
    if jittered and not any(batch[k].is_cuda for k in ('jitter', 'hsv_tab', 'lut_b') if k in batch):
        check_jitter(batch['jitter'].numpy(), batch.get('hsv_tab'), batch['lut_b'], batch['geom'].size(0))
    if fixed:
        if not any(batch[k].is_cuda for k in ('offset', 'fixed_geom', 'fixed_inv')):
            check_fixed(batch['offset'].numpy(), batch['fixed_geom'].numpy(), batch['fixed_inv'].numpy(), pixels)
    res = {k: (v.to(device, non_blocking=v.is_pinned()) if torch.is_tensor(v) and not (compressed and k == 'raw') else v) for k, v in batch.items()}
    jpeg_args = None
    if compressed:
        if raw.dtype != torch.uint8 or raw.dim() != 1 or raw.numel() > source:
            raise ValueError('to_device: raw must be uint8 [n] with n <= raw_bytes')
        res['raw'] = torch.empty(source, dtype=torch.uint8, device=device)
        if raw.numel():
            res['raw'][:raw.numel()].copy_(raw, non_blocking=raw.is_pinned())
        files, at, desc, dst_at, dst_geom = (res[k].contiguous() for k in ('jpeg', 'jpeg_offset', 'jpeg_desc', 'jpeg_dst', 'jpeg_geom'))
        n = desc.size(0)
        if (files.dtype != torch.uint8 or desc.dtype != torch.uint8 or desc.dim() != 2 or desc.size(1) != _hip.JPEG_DESC_BYTES or at.dtype != torch.int64
                or dst_at.dtype != torch.int64 or dst_geom.dtype != torch.int32 or at.numel() != n or dst_at.numel() != n or tuple(dst_geom.shape) != (n, 8)):
            raise ValueError('to_device: jpeg must be uint8, jpeg_desc uint8 [n, %d], jpeg_offset and jpeg_dst int64 [n], jpeg_geom int32 [n, 8]' % _hip.JPEG_DESC_BYTES)
        ws = torch.empty(max(int(batch['jpeg_ws_bytes']), 16), dtype=torch.uint8, device=device)
        res['jpeg_status'] = torch.empty(n, dtype=torch.int32, device=device)
        jpeg_args = (files.data_ptr(), files.numel(), at.data_ptr(), desc.data_ptr(), res['raw'].data_ptr(), source, dst_at.data_ptr(), dst_geom.data_ptr(),
                     ws.data_ptr(), ws.numel(), res['jpeg_status'].data_ptr(), n)
    raw, offset, geom = res['raw'], res['offset'], res['geom']
    B = geom.size(0)
    if raw.dtype != torch.uint8 or offset.dtype != torch.int64 or geom.dtype != torch.int32 or geom.dim() != 2 or geom.size(1) != 8 or offset.numel() != B:
        raise ValueError('to_device: raw must be uint8, offset int64 [B], geom int32 [B, 8]')
    if fixed:
        fixed_geom, fixed_inv = res['fixed_geom'].contiguous(), res['fixed_inv'].contiguous()
        if fixed_geom.dtype != torch.int32 or fixed_inv.dtype != torch.float64 or tuple(fixed_geom.shape) != (B, 4) or tuple(fixed_inv.shape) != (B, 6):
            raise ValueError('to_device: fixed_geom must be int32 [B, 4] and fixed_inv float64 [B, 6]')
        if not (0 < W <= _hip.WARP_MAX_DIM and 0 < H <= _hip.WARP_MAX_DIM):
            raise ValueError('to_device: size %dx%d (height and width are limited to %d)' % (H, W, _hip.WARP_MAX_DIM))
    elif not (0 < W <= _hip.COLLATE_MAX_W and H > 0):
        raise ValueError('to_device: size %dx%d (the width is limited to %d)' % (H, W, _hip.COLLATE_MAX_W))
    raw, offset, geom = raw.contiguous(), offset.contiguous(), geom.contiguous()
    lut = res.get('lut')
    if jittered:
        jitter, hsv_tab, lut = res['jitter'].contiguous(), res.get('hsv_tab'), res['lut_b'].contiguous()
        hsv_tab = None if hsv_tab is None else hsv_tab.contiguous()
        if (jitter.dtype != torch.int32 or tuple(jitter.shape) != (B, 4) or lut.dtype != torch.float32 or tuple(lut.shape) != (B, 3, 256)
                or (hsv_tab is not None and (hsv_tab.dtype != torch.uint8 or tuple(hsv_tab.shape) != (B, 3, 256)))):
            raise ValueError('to_device: jitter must be int32 [B, 4], hsv_tab uint8 [B, 3, 256], lut_b fp32 [B, 3, 256]')
    elif lut is None:
        lut = level_table(batch.get('normalize', (0.5, 1.0)), device)
    elif lut.dtype != torch.float32 or tuple(lut.shape) != (3, 256) or not lut.is_contiguous():
        raise ValueError('to_device: lut must be a contiguous fp32 [3, 256] tensor')
    if out is None:
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, 3, H, W) or not out.is_contiguous() or out.device != device:
        raise ValueError('to_device: out must be a contiguous fp32 [%d, 3, %d, %d] tensor on %s' % (B, H, W, device))
    warp_args = None
    if warped:
        src_offset, src_geom, inv = res['src_offset'].contiguous(), res['src_geom'].contiguous(), res['warp'].contiguous()
        if (src_offset.dtype != torch.int64 or src_geom.dtype != torch.int32 or inv.dtype != torch.float64 or tuple(src_geom.shape) != (B, 4)
                or tuple(inv.shape) != (B, 6) or src_offset.numel() != B):
            raise ValueError('to_device: src_offset must be int64 [B], src_geom int32 [B, 4], warp float64 [B, 6]')
        max_h, max_w = (int(v) for v in batch['rot_size'])
        if not (0 < max_h <= _hip.WARP_MAX_DIM and 0 < max_w <= _hip.WARP_MAX_DIM):
            raise ValueError('to_device: rot_size %dx%d (a rotated image is limited to %d rows and columns)' % (max_h, max_w, _hip.WARP_MAX_DIM))
        if rot is None:
            rot = torch.empty(pixels, dtype=torch.uint8, device=device)
        elif rot.dtype != torch.uint8 or rot.numel() < pixels or not rot.is_contiguous() or rot.device != device:
            raise ValueError('to_device: rot must be a contiguous uint8 tensor of at least %d bytes on %s' % (pixels, device))
        warp_args = (raw.data_ptr(), src_offset.data_ptr(), src_geom.data_ptr(), inv.data_ptr(), rot.data_ptr(), offset.data_ptr(), geom.data_ptr(),
                     B, max_h, max_w, int(batch.get('fill', 0)))
        raw = res['rot'] = rot
    tables = (jitter.data_ptr(), None if hsv_tab is None else hsv_tab.data_ptr(), lut.data_ptr()) if jittered else (lut.data_ptr(),)
    if fixed:
        tables = (fixed_geom.data_ptr(), fixed_inv.data_ptr(), lut.data_ptr())
    args = (raw.data_ptr(), offset.data_ptr()) + (() if fixed else (geom.data_ptr(),)) + tables + (B, H, W, 1 if batch.get('swap_rb', True) else 0, out.data_ptr())
    name = 'y2_fixed_images' if fixed else 'y2_collate_jitter_images' if jittered else 'y2_collate_images'
    if device.type == 'cuda':
        with torch.cuda.device(device):
            if compressed:
                _hip.check(_hip.lib().y2_jpeg_decode_images(*jpeg_args, _hip.stream()), 'y2_jpeg_decode_images')
            if warped:
                _hip.check(_hip.lib().y2_warp_affine_images(*warp_args, _hip.stream()), 'y2_warp_affine_images')
            _hip.check(getattr(_hip.lib(), name)(*args, _hip.stream()), name)
    else:
        if compressed:
            _hip.check(_hip.lib().y2_jpeg_decode_images_host(*jpeg_args), 'y2_jpeg_decode_images_host')
        if warped:
            _hip.check(_hip.lib().y2_warp_affine_images_host(*warp_args), 'y2_warp_affine_images_host')
        _hip.check(getattr(_hip.lib(), name + '_host')(*args), name + '_host')
    res['tensor'] = out
    return res
