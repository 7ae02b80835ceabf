"""Generate tests/golden/jitter.npz from the REFERENCE's image plugins (only where the reference checkout exists).

    python tools/make_golden_jitter.py

The reference's transform/image.py cannot be imported (cv2, skimage, inflection, torchvision): the file is parsed with `ast` and only the classes
RandomBlur, RandomHue, RandomSaturation, RandomBrightness and RandomGamma are compiled, unmodified, into a namespace that holds
  random       the module, behind a proxy that records every randint / uniform result (the draws)
  np           numpy, with the removed alias `np.int` standing for `int`
  inflection   `underscore` (CamelCase -> snake_case), written here
  cv2          split / merge as numpy indexing and stacking; blur records the kernel size it was handed and returns the image
  skimage      exposure.adjust_gamma records the gamma it was handed and returns the image
So what runs of the reference is its `__init__` parsing, its random draws in its order and the hue / saturation / brightness clip arithmetic with its
dtypes.  No pixel of a blur, a colour conversion or a gamma curve is computed or stored.

Per case the generators are seeded, the five plugins run in config.ini's order (blur, hue, saturation, brightness, gamma) on a 16x16 "HSV image" whose
S and V planes hold every level once (H: every level 0 .. 179 and random ones), and `random.random()` is drawn once more: a transform that consumes
the generator differently cannot reproduce that value.  Stored, arrays only:
  seed [K]; random_blur [K,2] int, random_hue [K,2] int, random_saturation / random_brightness / random_gamma [K,2] float64      the `[augmentation]` values
  hsv_in [K,16,16,3] uint8                      the image handed to RandomHue
  blur [K,2] int                                the kernel size handed to cv2.blur, (width, height)
  hue [K] int, saturation / brightness / gamma [K] float64      the draws (gamma: also what adjust_gamma was handed)
  hsv_out [K,16,16,3] uint8                     the image RandomBrightness returned
  next_random [K] float64                       random.random() right after the chain
The archive is written with fixed time stamps: a second run reproduces it byte for byte."""
import ast
import configparser
import os
import random
import re
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import refload  # noqa: E402
from make_golden_eval import save_npz  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'jitter.npz')
NAMES = ('RandomBlur', 'RandomHue', 'RandomSaturation', 'RandomBrightness', 'RandomGamma')
CASES = [  # seed, random_blur, random_hue, random_saturation, random_brightness, random_gamma
    (300, (5, 5), (0, 25), (0.5, 1.5), (0.5, 1.5), (0.9, 1.5)),          # config.ini
    (301, (5, 5), (0, 25), (0.5, 1.5), (0.5, 1.5), (0.9, 1.5)),
    (302, (7, 3), (-25, 25), (0.0, 2.0), (1.0, 3.0), (0.5, 2.0)),
    (303, (1, 7), (-180, 0), (1.0, 1.0), (0.25, 0.75), (1.0, 1.0)),
    (304, (2, 2), (170, 200), (1.5, 4.0), (0.0, 0.1), (0.1, 0.2)),
    (305, (3, 6), (0, 0), (0.9, 1.1), (0.9, 1.1), (2.0, 4.0)),
    (306, (1, 1), (-3, 3), (0.3, 0.3), (1.7, 1.7), (0.0, 0.0)),
    (307, (7, 7), (10, 40), (0.99, 1.01), (1.2, 1.3), (0.7, 0.8)),
]


class Recorder(object):
    """`random` with every randint / uniform result appended to `draws`."""

    def __init__(self):
        self.draws = []

    def randint(self, a, b):
        self.draws.append(random.randint(a, b))
        return self.draws[-1]

    def uniform(self, a, b):
        self.draws.append(random.uniform(a, b))
        return self.draws[-1]


class Stubs(object):
    def __init__(self):
        self.blur_size = self.gamma = None

    def blur(self, image, ksize):
        self.blur_size = tuple(ksize)
        return image

    def adjust_gamma(self, image, gamma):
        self.gamma = gamma
        return image


def load_reference(rec, stubs):
    path = os.path.join(refload.REF, 'transform', 'image.py')
    tree = ast.parse(open(path).read(), path)
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in NAMES]
    assert sorted(n.name for n in keep) == sorted(NAMES), path
    numpy = types.SimpleNamespace(**{k: getattr(np, k) for k in ('clip',)}, int=int)
    cv2 = types.SimpleNamespace(split=lambda a: tuple(a[..., c] for c in range(a.shape[-1])), merge=lambda planes: np.stack(planes, -1), blur=stubs.blur)
    inflection = types.SimpleNamespace(underscore=lambda s: re.sub(r'([a-z\d])([A-Z])', r'\1_\2', re.sub(r'([A-Z]+)([A-Z][a-z])', r'\1_\2', s)).lower())
    skimage = types.SimpleNamespace(exposure=types.SimpleNamespace(adjust_gamma=stubs.adjust_gamma))
    ns = dict(np=numpy, random=rec, inflection=inflection, cv2=cv2, skimage=skimage)
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, 'exec'), ns)
    return [ns[n] for n in NAMES]


def main():
    rec, stubs = Recorder(), Stubs()
    classes = load_reference(rec, stubs)
    K = len(CASES)
    keys = ('random_blur', 'random_hue', 'random_saturation', 'random_brightness', 'random_gamma')
    a = dict(seed=np.zeros(K, np.int64), hsv_in=np.zeros((K, 16, 16, 3), np.uint8), hsv_out=np.zeros((K, 16, 16, 3), np.uint8), blur=np.zeros((K, 2), np.int64),
             hue=np.zeros(K, np.int64), saturation=np.zeros(K, np.float64), brightness=np.zeros(K, np.float64), gamma=np.zeros(K, np.float64),
             next_random=np.zeros(K, np.float64))
    for k, key in enumerate(keys):
        a[key] = np.zeros((K, 2), np.int64 if k < 2 else np.float64)
    for k, case in enumerate(CASES):
        seed = case[0]
        rng = np.random.RandomState(seed)
        hsv = np.stack([np.concatenate([rng.permutation(180), rng.randint(0, 180, 76)]), rng.permutation(256), rng.permutation(256)], -1).astype(np.uint8).reshape(16, 16, 3)
        config = configparser.ConfigParser()
        config.read_dict({'augmentation': {key: ' '.join(repr(v) for v in value) for key, value in zip(keys, case[1:])}})
        plugins = [cls(config) for cls in classes]
        a['seed'][k], a['hsv_in'][k] = seed, hsv
        for key, value in zip(keys, case[1:]):
            a[key][k] = value
        rec.draws, stubs.blur_size, stubs.gamma = [], None, None
        random.seed(seed)
        out = hsv.copy()
        for plugin in plugins:
            out = plugin(out)
        a['next_random'][k] = random.random()
        assert out.dtype == np.uint8 and out.shape == hsv.shape and len(rec.draws) == 6 and stubs.blur_size == tuple(rec.draws[:2]) and stubs.gamma == rec.draws[5]
        a['blur'][k], a['hue'][k], a['saturation'][k], a['brightness'][k], a['gamma'][k] = stubs.blur_size, rec.draws[2], rec.draws[3], rec.draws[4], rec.draws[5]
        a['hsv_out'][k] = out
    save_npz(OUT, a)
    print('wrote %s (%d bytes): %d cases, blur sizes %s ...' % (OUT, os.path.getsize(OUT), K, a['blur'][:4].tolist()))


if __name__ == '__main__':
    main()
