"""Generate tests/golden/rotate.npz from the REFERENCE's rotation (only where the reference checkout exists).

    python tools/make_golden_rotate.py

The reference's transform/augmentation.py cannot be imported (cv2, inflection): the file is parsed with `ast` and only the class Rotator and the
function random_rotate are compiled, unmodified, into a namespace that holds np, random, inspect and a STUB `cv2` with three parts:
  getRotationMatrix2D  the documented formula (alpha = scale cos a, beta = scale sin a; [[alpha, beta, (1 - alpha) cx - beta cy],
                       [-beta, alpha, beta cx + (1 - alpha) cy]], float64), written here
  warpAffine           records the matrix, dsize, flags, border mode and border value it was handed and returns a placeholder of dsize
  INTER_LINEAR, BORDER_CONSTANT
No pixel is stored: the "image" is an empty uint8 array of the sample's size.

Per sample the random generators are seeded (`random.seed(seed)`, `np.random.seed(seed)`), random_rotate runs, and `random.random()` is drawn
once more: a transform that consumes the generators differently cannot reproduce that value.  Stored, arrays only:
  size [K,2], seed [K], count [K], angle_range [K,2]                the inputs (`[augmentation] random_rotate` per sample)
  in_min / in_max [K,N,2] float32                                   the labels handed in (zero rows beyond count)
  out_min / out_max [K,N,2] float32                                 the labels the reference returns
  matrix [K,2,3] float64, rotated [K,2] (height, width)             what it handed to warpAffine (dsize swapped to height, width)
  fill [K] float64                                                  the border value it passed
  next_random [K] float64                                           random.random() right after the call
The archive is written with fixed time stamps: a second run reproduces it byte for byte."""
import ast
import configparser
import inspect
import math
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import refload  # noqa: E402
from make_golden_eval import save_npz  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'rotate.npz')
NMAX = 4
RANGES = [(-5, 5), (-45, 45), (0, 0), (170, 190)]


class StubCv2(object):
    INTER_LINEAR, BORDER_CONSTANT = 1, 0

    def __init__(self):
        self.call = None

    @staticmethod
    def getRotationMatrix2D(center, angle, scale):
        a = angle * math.pi / 180
        alpha, beta = scale * math.cos(a), scale * math.sin(a)
        return np.array([[alpha, beta, (1 - alpha) * center[0] - beta * center[1]], [-beta, alpha, beta * center[0] + (1 - alpha) * center[1]]], np.float64)

    def warpAffine(self, image, matrix, dsize, flags=None, borderMode=None, borderValue=None):
        assert self.call is None, 'one warpAffine per sample'
        self.call = dict(matrix=np.array(matrix, np.float64), dsize=tuple(dsize), flags=flags, border=borderMode, fill=borderValue)
        return np.zeros((dsize[1], dsize[0], 3), np.uint8)


def load_reference(cv2):
    path = os.path.join(refload.REF, 'transform', 'augmentation.py')
    tree = ast.parse(open(path).read(), path)
    keep = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in ('Rotator', 'random_rotate')]
    assert sorted(n.name for n in keep) == ['Rotator', 'random_rotate'], path
    ns = dict(np=np, random=random, inspect=inspect, cv2=cv2)
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, 'exec'), ns)
    return ns['random_rotate']


def samples():
    """(h, w), seed, angle range, labels: VOC-like and small odd sizes down to 7x5, 1-4 boxes, boxes on the image border included."""
    rng = np.random.RandomState(7)
    shapes = [(375, 500), (500, 375), (333, 500), (500, 334), (97, 130), (41, 23), (375, 500), (281, 500), (500, 500), (120, 77), (64, 64), (7, 5),
              (375, 500), (500, 375), (33, 47), (300, 301)]
    out = []
    for k, (h, w) in enumerate(shapes):
        n = 1 + k % NMAX
        lo = rng.uniform(0, 0.6, (n, 2)) * (h, w)
        hi = lo + rng.uniform(0.1, 0.4, (n, 2)) * (h, w)
        if k % 5 == 0:
            lo[0], hi[0] = (0, 0), (h, w)              # a box that fills the image
        if k % 5 == 1:
            lo[0, 1], hi[0, 0] = 0, h                  # boxes on the left and bottom borders
        out.append(((h, w), 200 + k, RANGES[k % len(RANGES)], lo.astype(np.float32), hi.astype(np.float32)))
    return out


def main():
    cv2 = StubCv2()
    random_rotate = load_reference(cv2)
    sm = samples()
    K = len(sm)
    a = dict(size=np.zeros((K, 2), np.int32), seed=np.zeros(K, np.int64), count=np.zeros(K, np.int32), angle_range=np.zeros((K, 2), np.float64),
             in_min=np.zeros((K, NMAX, 2), np.float32), in_max=np.zeros((K, NMAX, 2), np.float32),
             out_min=np.zeros((K, NMAX, 2), np.float32), out_max=np.zeros((K, NMAX, 2), np.float32),
             matrix=np.zeros((K, 2, 3), np.float64), rotated=np.zeros((K, 2), np.int32), fill=np.zeros(K, np.float64), next_random=np.zeros(K, np.float64))
    for k, ((h, w), seed, (low, high), lo, hi) in enumerate(sm):
        n = len(lo)
        a['size'][k], a['seed'][k], a['count'][k], a['angle_range'][k] = (h, w), seed, n, (low, high)
        a['in_min'][k, :n], a['in_max'][k, :n] = lo, hi
        config = configparser.ConfigParser()
        config.read_dict({'augmentation': {'random_rotate': '%r %r' % (low, high)}})
        cv2.call = None
        random.seed(seed)
        np.random.seed(seed)
        image, yx_min, yx_max = random_rotate(config, np.zeros((h, w, 3), np.uint8), lo.copy(), hi.copy())
        a['next_random'][k] = random.random()
        call = cv2.call
        assert call['flags'] == cv2.INTER_LINEAR and call['border'] == cv2.BORDER_CONSTANT and np.isscalar(call['fill'])
        assert image.shape[:2] == call['dsize'][::-1] and yx_min.dtype == np.float32 and yx_max.dtype == np.float32 and yx_min.shape == (n, 2)
        a['out_min'][k, :n], a['out_max'][k, :n] = yx_min, yx_max
        a['matrix'][k], a['rotated'][k], a['fill'][k] = call['matrix'], call['dsize'][::-1], call['fill']
    assert not a['fill'].any() and (a['rotated'][a['angle_range'][:, 1] == 0] == a['size'][a['angle_range'][:, 1] == 0]).all()
    save_npz(OUT, a)
    print('wrote %s (%d bytes): %d samples, rotated sizes %s ...' % (OUT, os.path.getsize(OUT), K, a['rotated'][:4].tolist()))


if __name__ == '__main__':
    main()
