"""Parts shared by the two training graphs: model/train_graph.py (Darknet) and model/train_oplist.py (the op-list graph of Tiny, the ResNets,
MobileNet and the DenseNets).  Depends on neither graph: the gradient sink, the BatchNorm-statistics arena, the BatchNorm-parameter step, the
general-convolution launcher and the GEMM-operand buffer cache with its one y2_prep_weights launch."""
import ctypes

import torch

import _hip
from model._infer_parts import BN_EPS, LEAKY, fold_bn  # noqa: F401 (LEAKY: re-exported to the two graphs)

BN_MOMENTUM = 0.01          # Darknet and Tiny (model/yolo2.py)
PLUGIN_MOMENTUM = 0.1       # the ResNet, MobileNet and DenseNet plugins (nn.BatchNorm2d's default)


def _counter(bn):
    """nn.BatchNorm2d.num_batches_tracked as y2_bn_finalize increments it in place: an int64 scalar on the module's device."""
    t = bn.num_batches_tracked
    if t is None:
        return None
    if t.dtype != torch.int64 or not t.is_cuda:
        raise RuntimeError('BatchNorm2d.num_batches_tracked must be an int64 GPU tensor (got %s on %s)' % (t.dtype, t.device))
    return t


def _new(dev, *shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device=dev)


class GradSink(object):
    """Where a backward pass hands its parameter gradients: `grads` {id(param): tensor} and, when the network carries them, the hooks of the
    data-parallel wrapper (train.DataParallelRCCL) or of a StepPlan - grad_ready_hook(param, g) is told about every finished gradient,
    grad_buffer_hook(param) names where the averaged gradient will live (its flat-bucket slice)."""

    def __init__(self, net, dev):
        self.dev, self.grads = dev, {}
        self._ready_hook = getattr(net, 'grad_ready_hook', None)
        self._buffer_hook = getattr(net, 'grad_buffer_hook', None)

    def ready(self, param, g):
        self.grads[id(param)] = g
        if self._ready_hook is not None:
            self._ready_hook(param, g)

    def dest(self, param):
        """Tensor a finished gradient of `param` is written to: the data-parallel bucket slice when the wrapper offers one (the
        all-reduce then runs in place, no copy into the bucket), else fresh memory."""
        t = self._buffer_hook(param) if self._buffer_hook is not None else None
        return t if t is not None else _new(self.dev, *param.shape)

    def hand_affine(self, sums_arena, entries, st):
        """Affine-parameter gradients = the fp64 sums of BatchNorm-backward pass 1.  entries: (parameter, offset into sums_arena, length).
        Converted to fp32 by ONE y2_multi call (the library splits a table longer than it launches at once), straight into the bucket
        slices where the wrapper offers them, else into one fp32 image of the whole arena; then handed over."""
        items, handed, whole = [], [], None
        for prm, off, ln in entries:
            t = self._buffer_hook(prm) if self._buffer_hook is not None else None
            if t is None:
                if whole is None:
                    whole = _new(self.dev, sums_arena.numel())
                    items.append((_hip.MULTI_F64_TO_F32, whole, sums_arena))
                t = whole[off:off + ln]
            else:
                items.append((_hip.MULTI_F64_TO_F32, t, sums_arena[off:off + ln]))
            handed.append((prm, t))
        _hip.multi(items, st)
        for prm, t in handed:
            self.ready(prm, t)


class StatsArena(object):
    """One zero-filled fp64 arena for the replicated BatchNorm-statistics accumulators of every layer of a forward pass (one fill launch
    instead of one per layer); nothing is allocated for a frozen pass.  Owns the deterministic-mode rule: the producing kernel's epilogue
    gets no pointer (its atomics have no fixed order) and y2_colstats_det reduces the finished output instead."""

    def __init__(self, dev, channels, frozen):
        self.det = _hip.ensure_deterministic(dev)
        self.buf, self.used = None, 0
        if not frozen:
            self.buf = torch.empty(_hip.STATS_REPL * 2 * channels, dtype=torch.float64, device=dev)
            if self.buf.numel():
                _hip.multi([(_hip.MULTI_ZERO, self.buf, None)])

    def take(self, C):
        t = self.buf[self.used:self.used + _hip.STATS_REPL * 2 * C]
        self.used += _hip.STATS_REPL * 2 * C
        return t

    def epilogue(self, stats):
        """What the producing kernel is given as its statistics pointer."""
        return None if self.det else stats

    def settle(self, stats, z, M, C, ld):
        """After the producing kernel: z is [M rows][C channels], row stride ld."""
        if self.det and stats is not None:
            _hip.colstats_det(z, M, C, ld, stats)


def bn_params(L, st, dev, bn, stats, count, C, frozen, momentum, tensors=None):
    """scale, shift, mean, invstd of one BatchNorm over C channels.  frozen: the folded affine of the inference path (y2_bn_fold), mean /
    invstd from the running statistics, nothing updated.  Else y2_bn_finalize from the batch statistics of `count` elements per channel
    (running statistics and step counter updated through raw pointers).
    stats: the layer's accumulator, or a list of (channel offset, n, accumulator) slabs covering 0 .. C in order, each finalised on its own
    (slabs behind C are ignored; the step counter advances with the first).
    tensors: (gamma, beta, running_mean, running_var) to use instead of the module's own (Darknet: its effective, possibly zero-padded
    parameters).  Without it the module's tensors the kernel wrote are reported with _hip.wrote here; with it, reporting what was written -
    and copying stand-ins back - is the caller's."""
    gamma, beta, rm, rv = tensors if tensors is not None else (bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var)
    gamma, beta = _hip.f32c(gamma), _hip.f32c(beta)
    if frozen:
        scale, shift = fold_bn(L, st, dev, bn, (gamma, beta, rm, rv), C)
        return scale, shift, _hip.f32c(rm), torch.rsqrt(_hip.f32c(rv) + BN_EPS)
    scale, shift = _new(dev, C), _new(dev, C)
    mean, invstd = _new(dev, C), _new(dev, C)
    counter = _counter(bn)
    covered = 0
    for off, n, s in (stats if isinstance(stats, list) else [(0, C, stats)]):
        if off >= C:
            break
        assert off == covered and off + n <= C
        part = (gamma, beta, rm, rv, scale, shift, mean, invstd)
        if n != C:
            part = tuple(t[off:off + n] for t in part)
        g, b, m, v, sc, sh, mu, inv = part
        _hip.check(L.y2_bn_finalize(_hip.ptr(s), float(count), _hip.ptr(g), _hip.ptr(b), _hip.ptr(m), _hip.ptr(v), momentum, BN_EPS,
                                    _hip.ptr(sc), _hip.ptr(sh), _hip.ptr(mu), _hip.ptr(inv), n, _hip.ptr(counter) if off == 0 else None, st), 'y2_bn_finalize')
        covered = off + n
    assert covered == C
    if tensors is None:
        _hip.wrote([t for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked) if t is not None])
    return scale, shift, mean, invstd


def gen_conv(L, st, x, wp, y, B, H, W, cin, ldx, cout, k, stride, pad, ldy=None, coff=0, stats=None, transposed=False, out_hw=None):
    """One y2_conv_fwd of the general kernel family: any stride / padding, raw output (no affine, no activation) written at channel offset
    coff of rows ldy wide (default: a tensor of its own), BatchNorm statistics in the epilogue when `stats` is given.  transposed: the data
    gradient of a strided convolution, out_hw = the size of its result.  3x3 / stride 1 / pad 1 problems are offered the Winograd form."""
    p = _hip.ConvParams()
    p.x, p.w, p.y = x.data_ptr(), wp.data_ptr(), y.data_ptr()
    p.stats = stats.data_ptr() if stats is not None else None
    p.B, p.H, p.W, p.Cin, p.ldx, p.Cout, p.ksize = B, H, W, cin, ldx, cout, k
    p.ldy, p.coff, p.slope, p.tile = (cout if ldy is None else ldy), coff, 1.0, 0
    p.stride, p.pad_plus1 = stride, pad + 1
    if transposed:
        p.transposed, p.out_h, p.out_w = 1, out_hw[0], out_hw[1]
    u = _hip.wino_weight(wp, cout, cin) if (not transposed and stride == 1 and pad == 1 and _hip.wino_eligible(cout, cin, k)) else None
    _hip.autotune_conv(p, x.device, wino_w=u)
    _hip.conv_workspace(p, x.device)
    _hip.check(L.y2_conv_fwd(ctypes.byref(p), st), 'y2_conv_fwd')


def cached_buf(bufs, tag, n, dev):
    """The fp32 buffer `tag` of a buffer dict (per model, or owned by a StepPlan): kept from step to step, reallocated when its size changes."""
    t = bufs.get(tag)
    if t is None or t.numel() != n or t.device != dev:
        t = bufs[tag] = torch.empty(n, dtype=torch.float32, device=dev)
    return t


def prep_weights(items):
    """ONE y2_prep_weights launch.  items: (state_dict-layout weight, destination, Cout, Cin, ksize, _hip.PREP_* mode)."""
    if not items:
        return
    table = (_hip.PrepItem * len(items))()
    for e, (src, dst, cout, cin, k, mode) in zip(table, items):
        e.src, e.dst, e.Cout, e.Cin, e.ksize, e.mode = src.data_ptr(), dst.data_ptr(), cout, cin, k, mode
    _hip.check(_hip.lib().y2_prep_weights(table, len(items), _hip.stream()), 'y2_prep_weights')
