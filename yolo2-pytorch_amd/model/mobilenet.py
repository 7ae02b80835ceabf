"""`model.mobilenet` — the MobileNet backbone plugin of the reference (model/mobilenet.py:54-85), MI355X-native.

Drop-in for `[model] dnn = model.mobilenet.MobileNet`: same constructor `MobileNet(config_channels, anchors, num_cls)`, same module
tree and therefore the same `state_dict()` keys / shapes (`layers.0.conv.weight`, `layers.0.bn.*`, `layers.N.dw.conv.weight` [C,1,3,3],
`layers.N.dw.bn.*`, `layers.N.pw.conv.weight`, `layers.N.pw.bn.*`, `layers.14.{weight,bias}`), same
`forward(x[B,3,H,W]) -> [B, A*(5+C), H/32, W/32]`.  Widths come from ConfigChannels; only the stem and the pointwise convolutions
are named (a depthwise layer's width is its input width), as in the reference.

Execution (inference): the NCHW input is converted once to zero-padded 4-channel NHWC (y2_nchw_to_nhwc); the 3x3/s2 stem and every
1x1 pointwise convolution are y2_conv_fwd launches with BatchNorm folded into the epilogue and ReLU as LeakyReLU(slope 0); every
depthwise 3x3 is one y2_dwconv_fwd launch (csrc/dwconv.hip) with its folded BatchNorm and ReLU in the epilogue; the head is a 1x1
y2_conv_fwd with its bias.  Activations carry a pixel stride rounded up to 4 channels (zero padding), so pruned odd widths run in
inference (the depthwise kernel then takes its scalar path).  The plan per input shape is built from the shared parts of model/_infer_parts.py
(version-keyed prep, y2_conv_params filler, zero-filled plan buffers, scratch, pointer rebinding, forward() dispatch).  nn.Conv2d /
nn.BatchNorm2d are parameter containers only.  Training
runs through model/train_oplist.py (OpListTrainFn, _build_mobilenet: batch-statistics BN, depthwise data / weight gradients by
y2_dwconv_dgrad / y2_dwconv_wgrad); it needs every width to be a multiple of 4.
"""
import collections
import ctypes

import torch
import torch.nn as nn

import model
import _hip
from model import _infer_parts as parts
from model._infer_parts import pad4 as _pad4
STRIDES = (1, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 2, 1)                      # layers.1 .. layers.13 (model/mobilenet.py:58-70)
WIDTHS = (64, 128, 128, 256, 256, 512, 512, 512, 512, 512, 512, 1024, 1024)


class _Seq(nn.Sequential):
    def forward(self, x):
        raise RuntimeError('model.mobilenet layers are parameter containers; the network runs through MobileNet.forward (HIP)')


def conv_bn(in_channels, out_channels, stride):
    return _Seq(collections.OrderedDict([
        ('conv', nn.Conv2d(in_channels, out_channels, 3, stride, 1, bias=False)),
        ('bn', nn.BatchNorm2d(out_channels)),
        ('act', nn.ReLU(inplace=True)),
    ]))


def conv_dw(in_channels, stride):
    return _Seq(collections.OrderedDict([
        ('conv', nn.Conv2d(in_channels, in_channels, 3, stride, 1, groups=in_channels, bias=False)),
        ('bn', nn.BatchNorm2d(in_channels)),
        ('act', nn.ReLU(inplace=True)),
    ]))


def conv_pw(in_channels, out_channels):
    return _Seq(collections.OrderedDict([
        ('conv', nn.Conv2d(in_channels, out_channels, 1, 1, 0, bias=False)),
        ('bn', nn.BatchNorm2d(out_channels)),
        ('act', nn.ReLU(inplace=True)),
    ]))


def conv_unit(in_channels, out_channels, stride):
    return _Seq(collections.OrderedDict([
        ('dw', conv_dw(in_channels, stride)),
        ('pw', conv_pw(in_channels, out_channels)),
    ]))


class MobileNet(parts.InferMixin, nn.Module):
    """model/mobilenet.py:54-85."""

    def __init__(self, config_channels, anchors, num_cls):
        nn.Module.__init__(self)
        layers = [conv_bn(config_channels.channels, config_channels(32, 'layers.0.conv.weight'), 2)]
        for width, stride in zip(WIDTHS, STRIDES):
            layers.append(conv_unit(config_channels.channels, config_channels(width, 'layers.%d.pw.conv.weight' % len(layers)), stride))
        layers.append(nn.Conv2d(config_channels.channels, model.output_channels(len(anchors), num_cls), 1))
        self.layers = _Seq(*layers)
        for m in self.modules():       # model/mobilenet.py:79-84
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
        self._init_runtime()

    # ---- structure
    def stem(self):
        return self.layers[0]

    def units(self):
        """[(name, unit, stride)] of layers.1 .. layers.13."""
        return [('layers.%d' % i, self.layers[i], s) for i, s in zip(range(1, 1 + len(STRIDES)), STRIDES)]

    def head(self):
        return self.layers[len(STRIDES) + 1]

    def backward_param_order(self):
        """Convolution weights in the order the training backward finishes their gradients (the reverse of the forward's op list,
        model.train_oplist._build_mobilenet: stem, per unit depthwise then pointwise, head)."""
        fwd = [self.stem().conv]
        for _, unit, _ in self.units():
            fwd += [unit.dw.conv, unit.pw.conv]
        fwd.append(self.head())
        return [c.weight for c in reversed(fwd)]

    # ------------------------------------------------------------------ preparation: packed weights + folded BN
    def _prepare(self, dev):
        """prep[conv] = (wp, scale, shift, Cin as packed, Cout, k); of a depthwise convolution (w, scale, shift)."""
        ver = (dev, self._versions())
        prep = self._cached_prep(ver)
        if prep is not None:
            return prep
        L = _hip.lib()
        st = _hip.stream()
        prep = {}

        def fold(conv, bn):
            wp, cin, cout, k = parts.pack_weight(L, st, dev, conv.weight)      # (zero-padded input channels: the 3-channel image, pruned widths)
            prep[conv] = (wp,) + parts.affine(L, st, dev, conv, bn) + (cin, cout, k)

        def fold_dw(conv, bn):
            w = _hip.f32c(conv.weight.detach())           # [C][1][3][3]: read as it is by y2_dwconv_fwd
            _hip.require_gpu(w)
            prep[conv] = (w,) + parts.affine(L, st, dev, conv, bn)
        fold(self.stem().conv, self.stem().bn)
        for _, unit, _ in self.units():
            fold_dw(unit.dw.conv, unit.dw.bn)
            fold(unit.pw.conv, unit.pw.bn)
        fold(self.head(), None)
        self._cache = (ver, prep)
        return prep

    def _plan(self, prep, dev, B, cin0, H, W):
        key = self._plan_key(dev, B, cin0, H, W)
        plan = self._plans.get(key)
        if plan is not None:
            if plan['prep'] is not prep:
                for step in plan['steps']:
                    if step[0] == 'conv':
                        parts.PlanBuilder.rebind(step[1], *prep[step[2]][:3])
                    else:
                        step[2] = prep[step[1]]
                plan['prep'] = prep
            return plan
        build = parts.PlanBuilder(dev, torch.zeros)      # zero: the channel padding of every activation stays zero
        new = build.new
        steps = []

        def conv_step(conv, x, h, w, ldx, y, ldy, stride, pad, slope):
            wp, scale, shift, cin, cout, k = prep[conv]
            p, f = parts.conv_params(x, wp, scale, shift, B, h, w, cin, ldx, cout, k, slope, y=y, ldy=ldy, stride=stride, pad=pad,
                                     real_cin=conv.weight.shape[1])
            build.flops += f
            steps.append(['conv', p, conv])

        cpad = _pad4(cin0)
        x4 = new(B, H, W, cpad)
        c = self.stem().conv.weight.shape[0]
        ld = _pad4(c)
        h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        cur = new(B, h, w, ld)
        conv_step(self.stem().conv, x4, H, W, cpad, cur, ld, 2, 1, 0.0)
        for _, unit, s in self.units():
            ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
            d = new(B, ho, wo, ld)
            steps.append(['dw', unit.dw.conv, prep[unit.dw.conv], cur, d, B, h, w, c, ld, ld, s])
            build.flops += 2.0 * 9 * B * ho * wo * c
            co = unit.pw.conv.weight.shape[0]
            ldo = _pad4(co)
            y = new(B, ho, wo, ldo)
            conv_step(unit.pw.conv, d, ho, wo, ld, y, ldo, 1, 0, 0.0)
            cur, h, w, c, ld = y, ho, wo, co, ldo
        head = self.head()
        head_shape = (B, h, w, head.weight.shape[0])
        conv_step(head, cur, h, w, ld, cur, head.weight.shape[0], 1, 0, 1.0)      # y is bound per call (forward_nhwc)
        head_p = steps[-1][1]
        convs = [st[1] for st in steps if st[0] == 'conv']
        for p in convs:
            if p is not head_p:
                _hip.autotune_conv(p, dev)
        ws = build.share_workspace(convs)
        plan = dict(key=key, x4=x4, cpad=cpad, steps=steps, head=head_p, head_shape=head_shape, flops=build.flops, prep=prep, keep=(build.keep, ws))
        self._plans.put(key, plan, build.nbytes)
        return plan

    def forward_nhwc(self, x):
        x, B, cin0, H, W, dev = parts.enter(x)
        L = _hip.lib()
        prep = self._prepare(dev)
        plan = self._plan(prep, dev, B, cin0, H, W)
        st = _hip.stream()
        out = torch.empty(plan['head_shape'], dtype=torch.float32, device=dev)
        plan['head'].y = out.data_ptr()
        e0 = parts.profile_begin(self)
        _hip.check(L.y2_nchw_to_nhwc(_hip.ptr(x), _hip.ptr(plan['x4']), B, cin0, H, W, plan['cpad'], st), 'y2_nchw_to_nhwc')
        for step in plan['steps']:
            if step[0] == 'conv':
                _hip.check(L.y2_conv_fwd(ctypes.byref(step[1]), st), 'y2_conv_fwd')
            else:
                _, _, (wt, scale, shift), xin, y, b, h, w, c, ldx, ldy, s = step
                _hip.check(L.y2_dwconv_fwd(_hip.ptr(xin), _hip.ptr(wt), _hip.ptr(scale), _hip.ptr(shift), 0.0, _hip.ptr(y), None,
                                           b, h, w, c, ldx, ldy, s, st), 'y2_dwconv_fwd')
        parts.profile_end(self, e0, plan['flops'])
        return out
