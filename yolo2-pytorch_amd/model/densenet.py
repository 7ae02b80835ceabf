"""`model.densenet` — the DenseNet backbone plugins of the reference (model/densenet.py:29-117), MI355X-native.

Drop-in for `[model] dnn = model.densenet.densenet121` (169 / 201 / 161): same constructor
`DenseNet(config_channels, anchors, num_cls, growth_rate=32, block_config=(6, 12, 24, 16), num_init_features=64, bn_size=4, drop_rate=0)`,
the module tree torchvision gives the reference and therefore the same `state_dict()` keys / shapes (`features.conv0`, `features.norm0`,
`features.denseblock<i>.denselayer<j>.{norm1,conv1,norm2,conv2}`, `features.transition<i>.{norm,conv}`, `features.norm5`,
`features.conv` with bias), same `forward(x[B,3,H,W]) -> [B, A*(5+C), H/32, W/32]`.  No torchvision import.  Like the reference, widths come from
the constructor arguments, not from ConfigChannels.

Execution (inference): the NCHW input is converted once to zero-padded 4-channel NHWC; the 7x7/2 stem is one y2_conv_fwd launch (norm0 folded,
ReLU) and its MaxPool2d(3, 2, 1) writes straight into the first block buffer.  A dense block is ONE buffer [B, h, w, C_end]: the concatenation is
free (every layer's 3x3 convolution writes its growth_rate channels at its channel offset, every consumer reads the first C_in channels with
the buffer's pixel stride).  Per dense layer two launches: y2_preact_conv1x1_fwd (csrc/dense.hip: norm1 folded into the per-input-channel
pre-affine + ReLU in the operand loader, norm2 + ReLU in the epilogue), then the 3x3 y2_conv_fwd (raw) at channel offset C_in.  Per transition
one y2_preact_conv1x1_fwd launch with pool = 1 (the 2x2 average is taken on the pre-activated input: a 1x1 convolution and an average pool
commute) into the next block buffer.  The head is y2_preact_conv1x1_fwd with norm5 as the pre-affine (no ReLU, model/densenet.py:53-54) and the
bias in the epilogue.  Y2_DENSE_FUSED=0 runs every pre-activated 1x1 as the two-kernel form instead (y2_preact_fwd + 1x1 y2_conv_fwd): the A/B leg
of tools/densenet_bench.py.  The plan per input shape is built from the shared parts of model/_infer_parts.py (version-keyed prep, y2_conv_params
filler, zero-filled plan buffers, scratch, forward() dispatch); a new parameter version plans again.  nn.Conv2d / nn.BatchNorm2d are parameter
containers only.

Training runs through model/train_oplist.py (OpListTrainFn, _build_densenet: 'pre' / 'grow' ops): the batch statistics of a slab of the
concatenation are taken once, by its producer, and every consumer's BatchNorm finalises from them; the backward walks a block's layers in reverse
and accumulates into ONE gradient buffer per block through y2_preact_bwd.  It needs every width to be a multiple of 4.
"""
import collections
import ctypes
import os

import torch
import torch.nn as nn

import model
import _hip
from model import _infer_parts as parts
from model._infer_parts import pad4 as _pad4

# How a pre-activated 1x1 convolution runs: True = y2_preact_conv1x1_fwd, False = the two-kernel form (y2_preact_fwd + 1x1 y2_conv_fwd), None = per layer
# shape whichever measures faster on this device (timed once when the shape is first planned, kept in the tune table like the algorithm choices of
# _hip.autotune_conv; the fused kernel where nothing can be measured: Y2_AUTOTUNE=0, deterministic mode, during a graph capture).
FUSED = {'1': True, '0': False}.get(os.environ.get('Y2_DENSE_FUSED', ''))


class _Seq(nn.Sequential):
    def forward(self, x):
        raise RuntimeError('model.densenet layers are parameter containers; the network runs through DenseNet.forward (HIP)')


class _DenseLayer(_Seq):
    def __init__(self, num_input_features, growth_rate, bn_size):
        _Seq.__init__(self, collections.OrderedDict([
            ('norm1', nn.BatchNorm2d(num_input_features)),
            ('relu1', nn.ReLU(inplace=True)),
            ('conv1', nn.Conv2d(num_input_features, bn_size * growth_rate, kernel_size=1, stride=1, bias=False)),
            ('norm2', nn.BatchNorm2d(bn_size * growth_rate)),
            ('relu2', nn.ReLU(inplace=True)),
            ('conv2', nn.Conv2d(bn_size * growth_rate, growth_rate, kernel_size=3, stride=1, padding=1, bias=False)),
        ]))


class _DenseBlock(_Seq):
    def __init__(self, num_layers, num_input_features, bn_size, growth_rate):
        _Seq.__init__(self, collections.OrderedDict(
            ('denselayer%d' % (i + 1), _DenseLayer(num_input_features + i * growth_rate, growth_rate, bn_size)) for i in range(num_layers)))


class _Transition(_Seq):
    def __init__(self, num_input_features, num_output_features):
        _Seq.__init__(self, collections.OrderedDict([
            ('norm', nn.BatchNorm2d(num_input_features)),
            ('relu', nn.ReLU(inplace=True)),
            ('conv', nn.Conv2d(num_input_features, num_output_features, kernel_size=1, stride=1, bias=False)),
            ('pool', nn.AvgPool2d(kernel_size=2, stride=2)),
        ]))


class DenseNet(parts.InferMixin, nn.Module):
    """model/densenet.py:29-65."""

    def __init__(self, config_channels, anchors, num_cls, growth_rate=32, block_config=(6, 12, 24, 16), num_init_features=64, bn_size=4, drop_rate=0):
        nn.Module.__init__(self)
        if drop_rate != 0:
            raise NotImplementedError('model.densenet: drop_rate != 0 (dropout inside the dense layers) is not implemented')
        self.features = _Seq(collections.OrderedDict([
            ('conv0', nn.Conv2d(3, num_init_features, kernel_size=7, stride=2, padding=3, bias=False)),
            ('norm0', nn.BatchNorm2d(num_init_features)),
            ('relu0', nn.ReLU(inplace=True)),
            ('pool0', nn.MaxPool2d(kernel_size=3, stride=2, padding=1)),
        ]))
        num_features = num_init_features
        for i, num_layers in enumerate(block_config):
            self.features.add_module('denseblock%d' % (i + 1), _DenseBlock(num_layers, num_features, bn_size, growth_rate))
            num_features = num_features + num_layers * growth_rate
            if i != len(block_config) - 1:
                self.features.add_module('transition%d' % (i + 1), _Transition(num_features, num_features // 2))
                num_features = num_features // 2
        self.features.add_module('norm5', nn.BatchNorm2d(num_features))
        self.features.add_module('conv', nn.Conv2d(num_features, model.output_channels(len(anchors), num_cls), 1))
        for m in self.modules():       # model/densenet.py:57-62
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
        self.block_config = tuple(block_config)
        self._init_runtime()

    # ---- structure
    def blocks(self):
        """[(block, transition or None)] in forward order."""
        n = len(self.block_config)
        return [(getattr(self.features, 'denseblock%d' % (i + 1)), getattr(self.features, 'transition%d' % (i + 1)) if i != n - 1 else None) for i in range(n)]

    # ------------------------------------------------------------------ preparation: packed weights + folded BN
    def _prepare(self, dev):
        """prep[bn] = (scale, shift); prep[conv] = (weight as its kernel reads it, Cin as stored, Cout, k); prep['bias'] = the head's."""
        ver = (dev, self._versions())
        prep = self._cached_prep(ver)
        if prep is not None:
            return prep
        L = _hip.lib()
        st = _hip.stream()
        prep = {}

        def fold_bn(bn):
            prep[bn] = parts.fold_bn(L, st, dev, bn)

        def pack(conv):
            prep[conv] = parts.pack_weight(L, st, dev, conv.weight)      # (zero-padded input channels: the 3-channel image, widths that are not multiples of 4)

        def plain(conv):
            w = _hip.f32c(conv.weight.detach())           # [N][K][1][1]: read as it is by y2_preact_conv1x1_fwd (and, k = 1, by y2_conv_fwd)
            _hip.require_gpu(w)
            prep[conv] = (w, w.shape[1], w.shape[0], 1)
        f = self.features
        pack(f.conv0)
        fold_bn(f.norm0)
        for block, trans in self.blocks():
            for layer in block:
                fold_bn(layer.norm1)
                plain(layer.conv1)
                fold_bn(layer.norm2)
                pack(layer.conv2)
            if trans is not None:
                fold_bn(trans.norm)
                plain(trans.conv)
        fold_bn(f.norm5)
        plain(f.conv)
        prep['bias'] = parts.affine(L, st, dev, f.conv, None)[1]
        self._cache = (ver, prep)
        return prep

    def _plan(self, prep, dev, B, cin0, H, W):
        key = self._plan_key(dev, B, cin0, H, W, FUSED)
        plan = self._plans.get(key)
        if plan is not None and plan['prep'] is prep:
            return plan
        # (a new parameter version re-plans: the buffers of the old plan are dropped with it; the algorithm choices come from the table)
        build = parts.PlanBuilder(dev, torch.zeros)      # zero: the channel padding of an activation stays zero
        new, keep = build.new, build.keep
        steps, convs = [], []
        wino = {}

        def conv_step(conv, scale, shift, x, h, w, ldx, y, ldy, coff, stride, pad, slope):
            wp, cin, cout, k = prep[conv]
            p, f = parts.conv_params(x, wp, scale, shift, B, h, w, cin, ldx, cout, k, slope, y=y, ldy=ldy, coff=coff, stride=stride, pad=pad,
                                     real_cin=conv.weight.shape[1])
            build.flops += f
            u = None
            if _hip.wino_eligible(cout, cin, k, stride) and pad == 1:
                u = wino[id(p)] = _hip.wino_weight(wp, cout, cin)
            _hip.autotune_conv(p, dev, wino_w=u)
            convs.append(p)
            steps.append(('conv', p))

        def two_kernel(conv, pre, pre_slope, scale, shift, slope, x, h, w, K, ldx, y, ldy, coff, pool):
            wt, _, N, _ = prep[conv]
            ho, wo = (h // 2, w // 2) if pool else (h, w)
            act = torch.empty(B, ho, wo, K, dtype=torch.float32, device=dev)
            p, _ = parts.conv_params(act, wt, scale, shift, B, ho, wo, K, K, N, 1, slope, y=y, ldy=ldy, coff=coff, stride=1, pad=0)
            _hip.autotune_conv(p, dev)
            _hip.conv_workspace(p, dev)
            return act, p, [('act', x, pre[0], pre[1], pre_slope, act, h, w, K, ldx, pool), ('conv', p)]

        def preact_step(conv, pre, pre_slope, scale, shift, slope, x, h, w, K, ldx, y, ldy, coff, pool):
            wt, cin, N, _ = prep[conv]
            assert cin == K
            ho, wo = (h // 2, w // 2) if pool else (h, w)
            build.flops += 2.0 * K * N * B * ho * wo
            fused_step = ('pre', x, wt, pre[0], pre[1], pre_slope, scale, shift, slope, y, h, w, K, ldx, N, ldy, coff, pool)
            args = (conv, pre, pre_slope, scale, shift, slope, x, h, w, K, ldx, y, ldy, coff, pool)
            fused = FUSED
            if K % 4:          # (y2_conv_fwd reads 4-aligned channel counts)
                if fused is False:
                    raise RuntimeError('model.densenet: the two-kernel form (Y2_DENSE_FUSED=0) needs channel counts that are multiples of 4 (got %d)' % K)
                fused = True
            pair = None
            if fused is None:
                tkey = ('preact', B, h, w, K, ldx, N, pool, str(dev))
                hit = _hip.tune_lookup(tkey, dev)
                if hit is not None:
                    fused = bool(hit)
                elif not _hip.AUTOTUNE or _hip.DETERMINISTIC or torch.cuda.is_current_stream_capturing():
                    fused = True
                else:
                    pair = two_kernel(*args)
                    t_fused, t_pair = self._time(dev, B, [fused_step]), self._time(dev, B, pair[2])
                    fused = t_fused <= t_pair
                    _hip.tune_store(tkey, int(fused))
            if fused:
                steps.append(fused_step)
                return
            act, p, pair = pair if pair is not None else two_kernel(*args)
            build.nbytes += act.numel() * 4
            keep.append(act)
            convs.append(p)
            steps.extend(pair)

        f = self.features
        cpad = _pad4(cin0)
        x4 = new(B, H, W, cpad)
        c0 = f.conv0.weight.shape[0]
        h1, w1 = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
        stem = new(B, h1, w1, _pad4(c0))
        conv_step(f.conv0, prep[f.norm0][0], prep[f.norm0][1], x4, H, W, cpad, stem, _pad4(c0), 0, 2, 3, 0.0)
        h, w = (h1 + 2 - 3) // 2 + 1, (w1 + 2 - 3) // 2 + 1
        c, buf = c0, None
        for bi, (block, trans) in enumerate(self.blocks()):
            c_end = c + sum(layer.conv2.weight.shape[0] for layer in block)
            nxt = new(B, h, w, c_end)
            if bi == 0:
                steps.append(('maxpool', stem, nxt, h1, w1, c0, _pad4(c0), c_end))
            else:
                tr = self.blocks()[bi - 1][1]
                preact_step(tr.conv, prep[tr.norm], 0.0, None, None, 1.0, buf, 2 * h, 2 * w, c_prev_end, c_prev_end, nxt, c_end, 0, 1)
            buf = nxt
            for layer in block:
                n1 = layer.conv1.weight.shape[0]
                tmp = new(B, h, w, _pad4(n1))
                preact_step(layer.conv1, prep[layer.norm1], 0.0, prep[layer.norm2][0], prep[layer.norm2][1], 0.0, buf, h, w, c, c_end, tmp, _pad4(n1), 0, 0)
                conv_step(layer.conv2, None, None, tmp, h, w, _pad4(n1), buf, c_end, c, 1, 1, 1.0)
                c += layer.conv2.weight.shape[0]
            assert c == c_end
            c_prev_end = c_end
            if trans is not None:
                c = trans.conv.weight.shape[0]
                h, w = h // 2, w // 2
        head = f.conv
        head_shape = (B, h, w, head.weight.shape[0])
        head_y = new(*head_shape)          # (what the timing runs of the head write; forward_nhwc binds a fresh output per call)
        preact_step(head, prep[f.norm5], 1.0, None, prep['bias'], 1.0, buf, h, w, c, c, head_y, head.weight.shape[0], 0, 0)
        ws = build.share_workspace(convs)
        plan = dict(key=key, x4=x4, cpad=cpad, steps=steps, head_shape=head_shape, flops=build.flops, prep=prep, keep=(keep, ws, wino))
        self._plans.put(key, plan, build.nbytes)
        return plan

    @staticmethod
    def _run(steps, B, st, out=None):
        """Enqueue a step list; `out` (when given) receives what the LAST step writes."""
        L = _hip.lib()
        last = len(steps) - 1 if out is not None else -1
        for i, step in enumerate(steps):
            kind = step[0]
            if kind == 'conv':
                if i == last:
                    step[1].y = out.data_ptr()
                _hip.check(L.y2_conv_fwd(ctypes.byref(step[1]), st), 'y2_conv_fwd')
            elif kind == 'pre':
                _, xin, wt, ps, pb, pslope, scale, shift, slope, y, h, w, K, ldx, N, ldy, coff, pool = step
                _hip.check(L.y2_preact_conv1x1_fwd(_hip.ptr(xin), _hip.ptr(wt), _hip.ptr(ps), _hip.ptr(pb), pslope, _hip.ptr(scale), _hip.ptr(shift), slope,
                                                   _hip.ptr(out if i == last else y), None, B, h, w, K, ldx, N, ldy, coff, pool, st), 'y2_preact_conv1x1_fwd')
            elif kind == 'act':
                _, xin, ps, pb, pslope, act, h, w, K, ldx, pool = step
                _hip.check(L.y2_preact_fwd(_hip.ptr(xin), _hip.ptr(ps), _hip.ptr(pb), pslope, _hip.ptr(act), B, h, w, K, ldx, K, pool, st), 'y2_preact_fwd')
            else:
                _, src, dst, h1, w1, c0, lds, ldd = step
                _hip.check(L.y2_maxpool_fwd(_hip.ptr(src), _hip.ptr(dst), B, h1, w1, c0, lds, ldd, 3, 2, 1, 1, st), 'y2_maxpool_fwd')

    @classmethod
    def _time(cls, dev, B, steps, rounds=7, reps=3):
        """Median over `rounds` event pairs of `reps` warm executions of a step list, in ms per execution."""
        st = _hip.stream()
        cls._run(steps, B, st)
        times = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                cls._run(steps, B, st)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) / reps)
        return sorted(times)[len(times) // 2]

    def forward_nhwc(self, x):
        x, B, cin0, H, W, dev = parts.enter(x)
        L = _hip.lib()
        prep = self._prepare(dev)
        plan = self._plan(prep, dev, B, cin0, H, W)
        st = _hip.stream()
        out = torch.empty(plan['head_shape'], dtype=torch.float32, device=dev)
        e0 = parts.profile_begin(self)
        _hip.check(L.y2_nchw_to_nhwc(_hip.ptr(x), _hip.ptr(plan['x4']), B, cin0, H, W, plan['cpad'], st), 'y2_nchw_to_nhwc')
        self._run(plan['steps'], B, st, out)
        parts.profile_end(self, e0, plan['flops'])
        return out

    def forward(self, x):
        _hip.require_gpu(x)
        return parts.InferMixin.forward(self, x)

    def backward_param_order(self):
        """Convolution weights in the order the training backward finishes their gradients (the reverse of the forward's op list)."""
        f = self.features
        fwd = [f.conv0]
        for block, trans in self.blocks():
            for layer in block:
                fwd += [layer.conv1, layer.conv2]
            if trans is not None:
                fwd.append(trans.conv)
        fwd.append(f.conv)
        return [c.weight for c in reversed(fwd)]


def _make(**arch):
    def ctor(config_channels, anchors, num_cls, **kwargs):
        net = DenseNet(config_channels, anchors, num_cls, **dict(arch, **kwargs))
        parts.refuse_pretrained(config_channels, 'model.densenet')      # model/densenet.py:70-77
        return net
    return ctor


densenet121 = _make(num_init_features=64, growth_rate=32, block_config=(6, 12, 24, 16))
densenet169 = _make(num_init_features=64, growth_rate=32, block_config=(6, 12, 32, 32))
densenet201 = _make(num_init_features=64, growth_rate=32, block_config=(6, 12, 48, 32))
densenet161 = _make(num_init_features=96, growth_rate=48, block_config=(6, 12, 36, 24))
