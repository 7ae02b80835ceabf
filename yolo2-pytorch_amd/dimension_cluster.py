"""`dimension_cluster` — choosing a dataset's anchors: k-means on the distance 1 - IoU over the box sizes of the cache files, under the reference's
names (dimension_cluster.py: `distance`, `get_data`, `main`, `make_args`).

The reference hands `distance` to nltk.cluster.kmeans.KMeansClusterer, which runs every Lloyd iteration as Python calls and repeats "until Ctrl-C".
Here a trial is one workgroup of one y2_anchor_kmeans launch (include/yolo2_hip.h states the algorithm - nltk's, restated from memory and
UNVERIFIED against a real nltk run - and the fixed summation order), `cluster` runs `repeats` trials in chunks and selects among them on the host.
GPU data takes the device entry point, CPU data the bit-identical y2_anchor_kmeans_host.

Three deviations from the reference:
1. nltk reuses trial 0's converged means as the start of trial 1 (its test is `trial > 1`).  Here every trial draws its own sample.
2. The reference's random generator is unseeded.  Here `seed` seeds it (`None`: from the system, as there).
3. The reference divides (height, width) box sizes by Pillow's (width, height) image size.  Here each axis is divided by its own extent."""
import argparse
import configparser
import logging
import logging.config
import os
import random

import numpy as np
import torch

import _hip
import utils
import utils.data
import utils.iou.numpy

CHUNK = 4096          # trials per launch at most; a KeyboardInterrupt is honoured between chunks


def distance(a, b):
    return 1 - utils.iou.numpy.iou(-a, a, -b, b)


def get_data(paths):
    """The box sizes of the cache files as fractions of their images: float64 [N, 2], (height, width) per box."""
    sizes = []
    for data in utils.data.load_pickles(paths):
        width, height = utils.image_size(data['path'])
        sizes.append((np.asarray(data['yx_max']) - np.asarray(data['yx_min'])).reshape(-1, 2) / np.array([height, width]))
    return np.concatenate(sizes).astype(np.float64) if sizes else np.zeros((0, 2), np.float64)


def run_trials(size, init, max_iter=1000, conv_test=1e-6):
    """One y2_anchor_kmeans launch (or host call): size, a contiguous float64 tensor [N, 2] on the GPU or the CPU; init, int array [R, K] of box
    indices.  Returns numpy arrays: means [R, K, 2], iters [R], status [R], cost [R], counts [R, K]."""
    init = np.ascontiguousarray(init, np.int32)
    (R, K), N = init.shape, size.size(0)
    assert size.dtype == torch.float64 and size.is_contiguous() and size.dim() == 2 and size.size(1) == 2
    if init.min() < 0 or init.max() >= N:
        raise ValueError('dimension_cluster: an initial index lies outside [0, %d)' % N)
    dev = size.device
    out = dict(means=torch.empty(R, K, 2, dtype=torch.float64, device=dev), iters=torch.empty(R, dtype=torch.int32, device=dev),
               status=torch.empty(R, dtype=torch.int32, device=dev), cost=torch.empty(R, dtype=torch.float64, device=dev),
               counts=torch.empty(R, K, dtype=torch.int32, device=dev))
    ptrs = [out[k].data_ptr() for k in ('means', 'iters', 'status', 'cost', 'counts')]
    if size.is_cuda:
        with torch.cuda.device(dev):
            start = torch.from_numpy(init).to(dev)
            _hip.check(_hip.lib().y2_anchor_kmeans(size.data_ptr(), N, K, start.data_ptr(), R, max_iter, conv_test, *ptrs, _hip.stream()), 'y2_anchor_kmeans')
            return {k: v.cpu().numpy() for k, v in out.items()}          # (the copy waits for the launch: `start` outlives it)
    _hip.check(_hip.lib().y2_anchor_kmeans_host(size.data_ptr(), N, K, init.ctypes.data, R, max_iter, conv_test, *ptrs), 'y2_anchor_kmeans_host')
    return {k: v.numpy() for k, v in out.items()}


def assign(data, means, device=None):
    """Every box's nearest mean and its IoU with it (y2_anchor_assign): (index int32 [N], iou float64 [N]) as numpy arrays."""
    size = _tensor(data, device)
    m = torch.from_numpy(np.array(means, np.float64)).reshape(-1, 2).to(size.device)
    N, K = size.size(0), m.size(0)
    index, iou = torch.empty(N, dtype=torch.int32, device=size.device), torch.empty(N, dtype=torch.float64, device=size.device)
    if size.is_cuda:
        with torch.cuda.device(size.device):
            _hip.check(_hip.lib().y2_anchor_assign(size.data_ptr(), N, m.data_ptr(), K, index.data_ptr(), iou.data_ptr(), _hip.stream()), 'y2_anchor_assign')
    else:
        _hip.check(_hip.lib().y2_anchor_assign_host(size.data_ptr(), N, m.data_ptr(), K, index.data_ptr(), iou.data_ptr()), 'y2_anchor_assign_host')
    return index.cpu().numpy(), iou.cpu().numpy()


def _tensor(data, device):
    size = data if torch.is_tensor(data) else torch.from_numpy(np.array(data, np.float64))          # (a copy: the caller's array may be read-only)
    if device is not None:
        size = size.to(device)
    size = size.to(torch.float64).contiguous()
    if size.dim() != 2 or size.size(1) != 2 or size.size(0) < 1:
        raise ValueError('dimension_cluster: data must be [N, 2] (height, width) with N >= 1')
    if not bool((torch.isfinite(size) & (size > 0)).all()):
        raise ValueError('dimension_cluster: box sizes must be finite and positive')
    return size


def sort_means(means):
    """The permutation nltk's `means.sort(key=sum)` applies to one trial's means [K, 2] (stable)."""
    return np.argsort(means[:, 0] + means[:, 1], kind='stable')


def consensus(meanss):
    """nltk's choice among trials: of the sets of means [T, K, 2] (each sorted by sum) the first whose summed distance to all other sets is minimal."""
    T = len(meanss)
    total = np.zeros(T)
    rows = max(1, (1 << 19) // (T * meanss.shape[1]))          # blocks of rows: T x T x K distances never exist at once
    for i0 in range(0, T, rows):
        d = distance(meanss[i0:i0 + rows, None], meanss[None])          # [rows, T, K]; a set's distance to itself is exactly 0
        total[i0:i0 + rows] = d.sum(-1).sum(-1)
    return int(np.argmin(total))


def cluster(data, num, repeats=256, seed=None, device=None, max_iter=1000, conv_test=1e-6, select='consensus'):
    """k-means with `num` means on `data` [N, 2] (numpy array or tensor; a CUDA tensor, or `device`, runs on the GPU), `repeats` trials.
    Trial r starts from random.Random(seed).sample(range(N), num), drawn in trial order - the draw nltk makes from the vectors.  Trials that fail
    (status != 0: an empty cluster, max_iter reached) are left out of the selection; select='consensus' is nltk's rule (`consensus`), 'cost' takes
    the lowest cost.  With more than one trial the means are sorted by sum, as nltk leaves them.
    Returns a dict: means [num, 2], iou (the mean IoU of every box with its nearest mean, the paper's figure of merit), counts [num], trial (the
    chosen trial), and per trial trial_means [R, num, 2] (as the library returned them, unsorted), iters, status, cost; interrupted: a
    KeyboardInterrupt arrived between chunks and R is smaller than `repeats`."""
    if select not in ('consensus', 'cost'):
        raise ValueError("dimension_cluster: select must be 'consensus' or 'cost'")
    size = _tensor(data, device)
    N = size.size(0)
    if not 1 <= num <= _hip.KMEANS_MAX_K:
        raise ValueError('dimension_cluster: num must be in 1 .. %d' % _hip.KMEANS_MAX_K)
    if num > N:
        raise ValueError('dimension_cluster: %d means from %d boxes' % (num, N))
    if repeats < 1:
        raise ValueError('dimension_cluster: repeats must be positive')
    rng = random.Random(seed)
    parts, done, interrupted = [], 0, False
    try:
        while done < repeats:
            n = min(CHUNK, repeats - done)
            init = np.array([rng.sample(range(N), num) for _ in range(n)], np.int32).reshape(n, num)
            parts.append(run_trials(size, init, max_iter, conv_test))
            done += n
    except KeyboardInterrupt:
        if not parts:
            raise
        interrupted = True
    res = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    good = np.flatnonzero(res['status'] == 0)
    if good.size == 0:
        raise RuntimeError('dimension_cluster: none of the %d trials converged (status %s)' % (len(res['status']), sorted(set(res['status'].tolist()))))
    means, counts = res['means'][good], res['counts'][good]
    if len(res['status']) > 1:
        order = np.stack([sort_means(m) for m in means])
        means, counts = np.take_along_axis(means, order[..., None], 1), np.take_along_axis(counts, order, 1)
    pick = consensus(means) if select == 'consensus' else int(np.argmin(res['cost'][good]))
    return dict(means=means[pick], iou=1 - res['cost'][good[pick]] / N, counts=counts[pick], trial=int(good[pick]), trial_means=res['means'],
                iters=res['iters'], status=res['status'], cost=res['cost'], interrupted=interrupted)


def write_anchors(path, means, rows, cols):
    """The `width<TAB>height` table in cell units that utils.get_anchors reads back."""
    with open(path, 'w') as f:
        f.write('width\theight\n')
        for height, width in means:
            f.write('%s\t%s\n' % (repr(float(width * cols)), repr(float(height * rows))))


def main(argv=None):
    args = make_args(argv)
    config = configparser.ConfigParser()
    utils.load_config(config, args.config)
    path = os.path.expanduser(os.path.expandvars(args.logging))
    try:
        import yaml
        with open(path, 'r') as f:
            logging.config.dictConfig(yaml.safe_load(f))
    except (ImportError, OSError):
        logging.basicConfig(level=logging.INFO)
    cache_dir = utils.get_cache_dir(config)
    paths = [os.path.join(cache_dir, phase + '.pkl') for phase in args.phase]
    data = get_data(paths)
    logging.info('num_examples=%d' % len(data))
    res = cluster(data, args.num, args.repeats, seed=args.seed, device=args.device, select=args.select)
    if res['interrupted']:
        logging.warning('interrupted')
    logging.info('trials=%d, failed=%d, mean IoU=%f, counts=%s' % (len(res['status']), int((res['status'] != 0).sum()), res['iou'], res['counts'].tolist()))
    for m in res['means']:
        print('\t'.join(map(str, m)))
    if args.output is not None:
        if args.cells is None:
            raise SystemExit('--output needs --cells ROWS COLS')
        write_anchors(os.path.expanduser(os.path.expandvars(args.output)), res['means'], *args.cells)
    return res


def make_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('num', type=int)
    parser.add_argument('-r', '--repeats', type=int, default=256)
    parser.add_argument('-c', '--config', nargs='+', default=['config.ini'], help='config file')
    parser.add_argument('-p', '--phase', nargs='+', default=['train', 'val', 'test'])
    parser.add_argument('--logging', default='logging.yml', help='logging config')
    parser.add_argument('--seed', type=int, help='seed of the initial samples')
    parser.add_argument('--select', choices=['consensus', 'cost'], default='consensus', help='which trial to report')
    parser.add_argument('--device', help="where the trials run ('cuda', 'cpu'); default: the GPU when there is one")
    parser.add_argument('--cells', nargs=2, type=int, metavar=('ROWS', 'COLS'), help='cells of the output grid, to convert the means into anchors')
    parser.add_argument('--output', help='anchor table (width<TAB>height in cell units) to write')
    args = parser.parse_args(argv)
    if args.device is None:
        args.device = 'cuda' if torch.cuda.is_available() else 'cpu'
    return args


if __name__ == '__main__':
    main()
