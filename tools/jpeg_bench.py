#!/usr/bin/env python
"""Timing of JPEG decoding on one MI355X; prints ONE JSON line.

Workload: four batches of B = 64 VOC-like images (500x375 and 375x500, seeded smooth scenes with texture and noise) encoded as baseline 4:2:0 JPEG at
quality 90 with Pillow where it imports (`source: pillow`), else the largest committed fixture repeated (`source: fixture`; then the sizes are the
fixture's and the numbers say little).  Every batch is collated twice by utils.data.Collate (RandomCrop to 416x416) with the same seed: once with
JpegImage samples (`jpeg`), once with the decoded pixel arrays (`pixels`: the parent commit's path).  The device's decode is compared with the pixel
arrays once.  Medians over the timed batches of HIP-event times, everything measured `--runs` times in the process:
  (a) jpeg_to_device_ms    utils.data.to_device on the pinned `jpeg` batch: copy of the files and tables, y2_jpeg_decode_images, y2_collate_images
  (b) pixels_to_device_ms  the same on the pinned `pixels` batch: copy of the pixels, y2_collate_images
      (a) and (b) alternate batch by batch; the four batches rotate
  (c) decode_ms            y2_jpeg_decode_images alone, files and tables on the device
  (d) entropy_ms, idct_ms, colour_ms   its three kernels, from the library's per-kernel event hooks (y2_prof_*), in passes of their own
  (e) host_decode_ms_per_image / host_images_per_s   Pillow decoding the same files in this one process (host clock), where Pillow exists
and the bytes each path copies to the device.
    python tools/jpeg_bench.py [--batch 64] [--size 416] [--batches 24] [--warmup 4] [--runs 2]"""
import argparse
import configparser
import ctypes
import io
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'yolo2-pytorch_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

ROTATE = 4
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'jpeg', 'c420_q100_64x64.jpg')


def scene(rng, h, w):
    """RGB uint8 [h, w, 3]: gradients, rectangles, a sinusoidal texture and noise - compresses like a photograph, not like noise."""
    import numpy as np
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([255 * x / w, 255 * y / h, 255 * (1 - (x + y) / (h + w))], -1)
    for _ in range(12):
        y0, x0 = rng.randint(0, h), rng.randint(0, w)
        img[y0:y0 + rng.randint(8, h // 2), x0:x0 + rng.randint(8, w // 2)] = rng.randint(0, 256, 3)
    img += 24 * np.sin(x / rng.uniform(2, 9) + y / rng.uniform(2, 9))[..., None]
    return np.clip(img + rng.normal(0, 8, img.shape), 0, 255).astype(np.uint8)


def make_files(B, seed):
    """[(file bytes uint8 [n], decoded BGR array or None)] and the source's name."""
    import numpy as np
    try:
        from PIL import Image
    except ImportError:
        data = np.fromfile(FIXTURE, np.uint8)
        return [(data, None)] * B, 'fixture'
    rng = np.random.RandomState(seed)
    files = []
    for i in range(B):
        h, w = (375, 500) if i % 3 else (500, 375)
        buf = io.BytesIO()
        Image.fromarray(scene(rng, h, w)).save(buf, 'JPEG', quality=90, subsampling=2)
        files.append((np.frombuffer(buf.getvalue(), np.uint8).copy(), None))
    return files, 'pillow'


def collate_pair(files, S, seed):
    """The same batch collated from JpegImage samples and from the pixel arrays (decoded by the host function, which the tests hold to Pillow)."""
    import numpy as np

    import transform.augmentation
    import transform.resize.label
    import utils.data
    config = configparser.ConfigParser()
    config.read_dict({'data': {'resize': 'rescale'}, 'augmentation': {'random_flip_horizontally': '0.5', 'random_crop': '1'}})
    out = []
    images = [utils.data.probe_jpeg(data) for data, _ in files]
    assert all(image is not None for image in images)
    for kind in ('jpeg', 'pixels'):
        random.seed(seed)
        np.random.seed(seed)
        flip = transform.augmentation.RandomFlipHorizontally(config)
        collate = utils.data.Collate(transform.resize.label.RandomCrop(config), [(S, S)])
        samples = []
        for image in images:
            h, w, _ = image.shape
            samples.append(flip(dict(image=image if kind == 'jpeg' else image.decode(), yx_min=np.array([[0.2 * h, 0.2 * w]], np.float32),
                                     yx_max=np.array([[0.8 * h, 0.8 * w]], np.float32), cls=np.zeros(1, np.int64), difficult=np.zeros(1, np.uint8))))
        out.append(collate(samples))
    return out


def event_ms(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernel_ms(L, fn, passes):
    """name -> median ms per launch over `passes` calls of fn, by the library's per-kernel event hooks."""
    import torch
    torch.cuda.synchronize()
    L.y2_prof_enable(1)
    try:
        for _ in range(passes):
            fn()
        torch.cuda.synchronize()
    finally:
        L.y2_prof_enable(0)
    name, ms, fl, table = ctypes.create_string_buffer(96), ctypes.c_float(), ctypes.c_double(), {}
    for i in range(L.y2_prof_count()):
        if L.y2_prof_get(i, name, 96, ctypes.byref(ms), ctypes.byref(fl)) == 0:
            table.setdefault(name.value.decode(), []).append(ms.value)
    return {k: statistics.median(v) for k, v in table.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('--batches', type=int, default=24)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--runs', type=int, default=2)
    args = ap.parse_args()
    import torch

    import _hip
    import utils.data
    assert torch.cuda.is_available(), 'jpeg_bench.py measures on an MI355X'
    dev = torch.device('cuda', 0)
    B, S = args.batch, args.size
    labels = set(utils.data.LABELS)
    sets, source = [], None
    for r in range(ROTATE):
        files, source = make_files(B, 100 + r)
        sets.append((files, collate_pair(files, S, 100 + r)))
    pin = lambda b: {k: (v.pin_memory() if torch.is_tensor(v) and v.numel() else v) for k, v in b.items() if k not in labels}
    jpeg, pixels = [pin(p[0]) for _, p in sets], [pin(p[1]) for _, p in sets]
    outs = [torch.empty(B, 3, S, S, dtype=torch.float32, device=dev) for _ in range(ROTATE)]
    first = utils.data.to_device(jpeg[0], dev)
    assert first['jpeg_status'].tolist() == [0] * B, 'a stream did not decode'
    assert torch.equal(first['tensor'], utils.data.to_device(pixels[0], dev)['tensor']), 'the JPEG path and the pixel path differ'
    L, st = _hip.lib(), _hip.stream()
    on_dev, calls = [], []
    for b in jpeg:
        d = {k: b[k].to(dev) for k in ('jpeg', 'jpeg_offset', 'jpeg_desc', 'jpeg_dst', 'jpeg_geom')}
        d['dst'] = torch.empty(int(b['raw_bytes']), dtype=torch.uint8, device=dev)
        d['ws'] = torch.empty(int(b['jpeg_ws_bytes']), dtype=torch.uint8, device=dev)
        d['status'] = torch.empty(B, dtype=torch.int32, device=dev)
        on_dev.append(d)
        calls.append((d['jpeg'].data_ptr(), d['jpeg'].numel(), d['jpeg_offset'].data_ptr(), d['jpeg_desc'].data_ptr(), d['dst'].data_ptr(), d['dst'].numel(),
                      d['jpeg_dst'].data_ptr(), d['jpeg_geom'].data_ptr(), d['ws'].data_ptr(), d['ws'].numel(), d['status'].data_ptr(), B, st))
    copied = lambda b: sum(v.numel() * v.element_size() for v in b.values() if torch.is_tensor(v))
    res = dict(batch=B, size=S, batches=args.batches, source=source, device=torch.cuda.get_device_name(0),
               file_mbytes=round(statistics.mean(b['jpeg'].numel() for b in jpeg) / 1e6, 3), pixel_mbytes=round(statistics.mean(b['raw'].numel() for b in pixels) / 1e6, 3),
               jpeg_copied_mbytes=round(statistics.mean(copied(b) for b in jpeg) / 1e6, 3), pixels_copied_mbytes=round(statistics.mean(copied(b) for b in pixels) / 1e6, 3),
               scratch_mbytes=round(int(jpeg[0]['jpeg_ws_bytes']) / 1e6, 2))
    res['copied_ratio'] = round(res['pixels_copied_mbytes'] / res['jpeg_copied_mbytes'], 2)
    runs = []
    for _ in range(args.runs):
        a_ms, b_ms, c_ms = [], [], []
        for i in range(args.warmup + args.batches):
            j = i % ROTATE
            a = event_ms(lambda: utils.data.to_device(jpeg[j], dev, out=outs[j]))
            b = event_ms(lambda: utils.data.to_device(pixels[j], dev, out=outs[j]))
            c = event_ms(lambda: _hip.check(L.y2_jpeg_decode_images(*calls[j]), 'y2_jpeg_decode_images'))
            if i >= args.warmup:
                a_ms.append(a)
                b_ms.append(b)
                c_ms.append(c)
        k = kernel_ms(L, lambda: [_hip.check(L.y2_jpeg_decode_images(*c), 'y2_jpeg_decode_images') for c in calls], max(args.batches // ROTATE, 5))
        mm = lambda v: [round(min(v), 3), round(max(v), 3)]
        runs.append(dict(jpeg_to_device_ms=round(statistics.median(a_ms), 3), pixels_to_device_ms=round(statistics.median(b_ms), 3),
                         decode_ms=round(statistics.median(c_ms), 3), jpeg_to_device_ms_min_max=mm(a_ms), pixels_to_device_ms_min_max=mm(b_ms), decode_ms_min_max=mm(c_ms),
                         entropy_ms=round(k.get('jpeg_entropy_kernel', float('nan')), 3), idct_ms=round(k.get('jpeg_idct_kernel', float('nan')), 4),
                         colour_ms=round(k.get('jpeg_colour_kernel', float('nan')), 4)))
    res['runs'] = runs
    if source == 'pillow':
        from PIL import Image
        import numpy as np
        blobs = [bytes(data) for data, _ in sets[0][0]]
        for _ in range(2):
            t0 = time.perf_counter()
            for blob in blobs:
                np.asarray(Image.open(io.BytesIO(blob)).convert('RGB'))
            per = (time.perf_counter() - t0) / len(blobs)
        res.update(host_decode_ms_per_image=round(per * 1e3, 3), host_images_per_s=round(1 / per, 1))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
