"""Generate tests/golden/collate.npz from the REFERENCE's label transforms (only where the reference checkout exists).

    python tools/make_golden_collate.py

The reference's transform/resize/label.py, transform/augmentation.py and utils/data.py cannot be imported (cv2, inflection, sklearn): the files
are parsed with `ast` and only the function definitions rescale, resize (random_crop calls it), random_crop, flip_horizontally,
random_flip_horizontally and the method Collate.next_size are compiled, unmodified, into a namespace that holds np, random, inspect and a STUB
`cv2`.  The stub's `flip` returns its argument and notes that it was called; its `resize` returns a placeholder and records which part of the
image it was handed.  The "image" is an int32 array whose pixel (y, x) holds (y, x, 0), so the origin of the crop the reference cut can be read
from the view it passes on; no pixel of it is stored.

Per sample the random generators are seeded (`random.seed(seed)`, `np.random.seed(seed)`), then the reference's order of calls is followed:
random_flip_horizontally (the Dataset's augmentation), then random_crop or resize (Collate).  Stored, arrays only:
  size [K,2], target [K,2], seed [K], crop [K] (1: random_crop, 0: resize), count [K]      the inputs
  flip_prob, crop_scale                                                                     `[augmentation]` values used
  in_min / in_max [K,N,2] float32                                                           the labels handed in (zero rows beyond count)
  out_min / out_max [K,N,2] float32                                                         the labels the reference returns
  window [K,4] (y0, x0, h, w), flip [K]                                                     the part of the (flipped) image it resized
  sizes [S,2], maintain, size_seed, size_sequence [T,2]                                     Collate.next_size under random.seed(size_seed)
The archive is written with fixed time stamps: a second run reproduces it byte for byte."""
import ast
import configparser
import inspect
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import refload  # noqa: E402
from make_golden_eval import save_npz  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'collate.npz')
FLIP_PROB, CROP_SCALE, NMAX = 0.5, 1.0, 4
SIZES = [(320, 320), (352, 352), (384, 416), (416, 416), (608, 608)]
MAINTAIN, SIZE_SEED, SIZE_STEPS = 3, 11, 30


class StubCv2(object):
    def __init__(self):
        self.flipped, self.window = False, None

    def flip(self, image, code):
        assert code == 1
        self.flipped = not self.flipped
        return image

    def resize(self, image, dsize):
        self.window = (int(image[0, 0, 0]), int(image[0, 0, 1]), image.shape[0], image.shape[1])
        return np.zeros((1, 1, 3), np.uint8)


def cut(path, names, cls=None):
    tree = ast.parse(open(path).read(), path)
    body = tree.body
    if cls is not None:
        body = [n for n in body if isinstance(n, ast.ClassDef) and n.name == cls][0].body
    keep = [n for n in body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in keep) == sorted(names), path
    return ast.Module(body=keep, type_ignores=[]), path


def load_reference(cv2):
    ns = dict(np=np, random=random, inspect=inspect, cv2=cv2)
    for module, path in (cut(os.path.join(refload.REF, 'transform', 'resize', 'label.py'), ('rescale', 'resize', 'random_crop')),
                         cut(os.path.join(refload.REF, 'transform', 'augmentation.py'), ('flip_horizontally', 'random_flip_horizontally')),
                         cut(os.path.join(refload.REF, 'utils', 'data.py'), ('next_size',), cls='Collate')):
        exec(compile(module, path, 'exec'), ns)
    return types.SimpleNamespace(**{k: ns[k] for k in ('resize', 'random_crop', 'random_flip_horizontally', 'next_size')})


def coordinate_image(h, w):
    image = np.zeros((h, w, 3), np.int32)
    image[..., 0] = np.arange(h).reshape(h, 1)
    image[..., 1] = np.arange(w).reshape(1, w)
    return image


def samples():
    """(h, w), (height, width), seed, crop, labels: VOC-like and small odd sizes, 1-4 boxes, boxes touching the image border included."""
    rng = np.random.RandomState(3)
    out = []
    shapes = [(375, 500), (500, 375), (333, 500), (500, 334), (97, 130), (41, 23), (375, 500), (281, 500), (500, 500), (120, 77), (64, 64), (7, 5),
              (375, 500), (500, 375), (33, 47), (300, 301)]
    for k, (h, w) in enumerate(shapes):
        n = 1 + k % NMAX
        lo = rng.uniform(0, 0.6, (n, 2)) * (h, w)
        hi = lo + rng.uniform(0.1, 0.4, (n, 2)) * (h, w)
        if k % 5 == 0:
            lo[0], hi[0] = (0, 0), (h, w)              # a box that fills the image: no room to crop
        if k % 5 == 1:
            lo[0, 1], hi[0, 0] = 0, h                  # boxes on the left and bottom borders
        target = SIZES[k % len(SIZES)] if k % 3 else (32 * (1 + k % 4), 32 * (2 + k % 3))
        out.append(((h, w), target, 100 + k, 0 if k >= 12 else 1, lo.astype(np.float32), hi.astype(np.float32)))
    return out


def main():
    cv2 = StubCv2()
    ref = load_reference(cv2)
    config = configparser.ConfigParser()
    config.read_dict({'data': {'resize': 'rescale'}, 'augmentation': {'random_flip_horizontally': repr(FLIP_PROB), 'random_crop': repr(CROP_SCALE)}})
    sm = samples()
    K = len(sm)
    a = dict(size=np.zeros((K, 2), np.int32), target=np.zeros((K, 2), np.int32), seed=np.zeros(K, np.int64), crop=np.zeros(K, np.int32),
             count=np.zeros(K, np.int32), flip_prob=np.float64(FLIP_PROB), crop_scale=np.float64(CROP_SCALE),
             in_min=np.zeros((K, NMAX, 2), np.float32), in_max=np.zeros((K, NMAX, 2), np.float32),
             out_min=np.zeros((K, NMAX, 2), np.float32), out_max=np.zeros((K, NMAX, 2), np.float32),
             window=np.zeros((K, 4), np.int32), flip=np.zeros(K, np.uint8))
    for k, ((h, w), (height, width), seed, crop, lo, hi) in enumerate(sm):
        n = len(lo)
        a['size'][k], a['target'][k], a['seed'][k], a['crop'][k], a['count'][k] = (h, w), (height, width), seed, crop, n
        a['in_min'][k, :n], a['in_max'][k, :n] = lo, hi
        cv2.flipped, cv2.window = False, None
        random.seed(seed)
        np.random.seed(seed)
        image, yx_min, yx_max = ref.random_flip_horizontally(config, coordinate_image(h, w), lo.copy(), hi.copy())
        if crop:
            _, yx_min, yx_max = ref.random_crop(config, image, yx_min, yx_max, height, width)
        else:
            _, yx_min, yx_max = ref.resize(config, image, yx_min, yx_max, height, width)
        assert yx_min.dtype == np.float32 and yx_max.dtype == np.float32
        a['out_min'][k, :n], a['out_max'][k, :n] = yx_min, yx_max
        a['window'][k], a['flip'][k] = cv2.window, cv2.flipped
    assert 0 < a['flip'].sum() < K and (a['window'][a['crop'] == 1, 2:] < a['size'][a['crop'] == 1]).any()
    assert (a['window'][a['crop'] == 0] == np.concatenate([np.zeros((4, 2), np.int32), a['size'][a['crop'] == 0]], 1)).all()
    state = types.SimpleNamespace(sizes=SIZES, maintain=MAINTAIN, _maintain=MAINTAIN)
    random.seed(SIZE_SEED)
    a.update(sizes=np.array(SIZES, np.int32), maintain=np.int64(MAINTAIN), size_seed=np.int64(SIZE_SEED),
             size_sequence=np.array([ref.next_size(state) for _ in range(SIZE_STEPS)], np.int32))
    save_npz(OUT, a)
    print('wrote %s (%d bytes): %d samples, %d flipped, windows %s ...' % (OUT, os.path.getsize(OUT), K, a['flip'].sum(), a['window'][:3].tolist()))


if __name__ == '__main__':
    main()
