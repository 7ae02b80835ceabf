"""`model.resnet` — the ResNet backbone plugins (resnet18 ... resnet152) of the reference, MI355X-native.

Drop-in for model/resnet.py:29-224: same constructors `resnetNN(config_channels, anchors, num_cls)`, same
`state_dict()` keys/shapes (`conv1.weight`, `bn1.*`, `layerL.B.conv{1,2,3}.weight`, `layerL.B.bn{1,2,3}.*`,
`layerL.B.downsample.{0,1}.*`, `conv.{weight,bias}`), same `forward(x[B,3,H,W]) -> [B, A*(5+C), H/32, W/32]`;
`[model] dnn = model.resnet.resnet50` in an unmodified ini selects it (BASELINE config 5 exercises the plugin swap).

Execution (inference): the NCHW input is converted once to zero-padded 4-channel NHWC (y2_nchw_to_nhwc); every
convolution — 7x7/s2 stem, 3x3/s2, 1x1/s2 down-sample, 1x1, 3x3 — is one y2_conv_fwd launch of the general fp32-MFMA
LDS-DMA kernel with BatchNorm folded into the epilogue, ReLU as LeakyReLU(slope 0), and the residual addition of
BasicBlock / Bottleneck (model/resnet.py:59,101) fused into the epilogue of the block's last convolution; the stem
max-pool is y2_maxpool_fwd.  The whole chain is one y2_conv_fwd_batch call per stage list, built once per input shape from the shared parts of
model/_infer_parts.py (version-keyed prep, y2_conv_params filler, plan buffers and scratch, pointer rebinding, forward() dispatch).
nn.Conv2d / nn.BatchNorm2d objects are parameter containers only.  Training runs through model/train_oplist.py
(OpListTrainFn, _build_resnet: batch-statistics BN, strided data gradients as transposed convolutions, general weight gradient).
"""
import ctypes

import torch
import torch.nn as nn

import model
import _hip
from model import _infer_parts as parts


class _Block(nn.Module):
    """A residual block as data: SPEC lists its convolutions as (kernel, width multiplier, carries the block stride, padding).
    Attribute names conv<i>/bn<i>/downsample are the reference's state_dict keys (= torchvision's)."""
    SPEC = ()

    def __init__(self, config_channels, prefix, channels, stride=1):
        nn.Module.__init__(self)
        self.stride = stride
        c_in = config_channels.channels
        self._convs = []
        for i, (k, mult, strided, pad) in enumerate(self.SPEC, 1):
            cin = config_channels.channels
            cout = config_channels(channels * mult, '%s.conv%d.weight' % (prefix, i))
            s_i = stride if strided else 1
            conv, bn = nn.Conv2d(cin, cout, k, s_i, pad, bias=False), nn.BatchNorm2d(cout)
            setattr(self, 'conv%d' % i, conv)
            setattr(self, 'bn%d' % i, bn)
            self._convs.append((conv, bn, s_i, pad))
        c_out = config_channels.channels
        self.downsample = None
        if stride > 1 or c_in != c_out:      # projection shortcut (model/resnet.py:44-50, 86-92)
            self.downsample = nn.Sequential(nn.Conv2d(c_in, c_out, 1, stride, bias=False), nn.BatchNorm2d(c_out))

    def convs(self):
        return list(self._convs)

    def forward(self, x):
        raise RuntimeError('model.resnet blocks are parameter containers; the network runs through ResNet.forward (HIP)')


class BasicBlock(_Block):
    """model/resnet.py:29-62: 3x3 (strided) -> 3x3."""
    SPEC = ((3, 1, True, 1), (3, 1, False, 1))


class Bottleneck(_Block):
    """model/resnet.py:65-104: 1x1 -> 3x3 (strided) -> 1x1 (4x wide)."""
    SPEC = ((1, 1, False, 0), (3, 1, True, 1), (1, 4, False, 0))


class ResNet(parts.InferMixin, nn.Module):
    """model/resnet.py:107-159."""
    STAGES = ((64, 1), (128, 2), (256, 2), (512, 2))       # (width, stride of the first block) of layer1..layer4

    def __init__(self, config_channels, anchors, num_cls, block, layers):
        nn.Module.__init__(self)
        c_in = config_channels.channels
        self.conv1 = nn.Conv2d(c_in, config_channels(64, 'conv1.weight'), kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(config_channels.channels)
        for li, ((width, stride), count) in enumerate(zip(self.STAGES, layers), 1):
            name = 'layer%d' % li
            blocks = [block(config_channels, '%s.%d' % (name, bi), width, stride if bi == 0 else 1) for bi in range(count)]
            setattr(self, name, nn.Sequential(*blocks))
        self.conv = nn.Conv2d(config_channels.channels, model.output_channels(len(anchors), num_cls), 1)
        for m in self.modules():       # model/resnet.py:120-126
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
        self._init_runtime()

    def backward_param_order(self):
        """Convolution weights in the order the training backward finishes their gradients (the reverse of the forward's op list,
        model.train_oplist._build_resnet: stem, per block the projection shortcut then its convolutions, head)."""
        fwd = [self.conv1]
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                if blk.downsample is not None:
                    fwd.append(blk.downsample[0])
                fwd += [conv for conv, _, _, _ in blk.convs()]
        fwd.append(self.conv)
        return [c.weight for c in reversed(fwd)]

    def scope(self, name):
        """Pruning helper (model/resnet.py:142-156): the block-level scope of a parameter name - 'layer1.0.conv2.weight' ->
        'layer1.0.2', 'layer2.0.downsample.0.weight' -> 'layer2.0', 'conv.weight' -> 'conv'."""
        import re
        comp = name.split('.')[:-1]
        m = re.search(r'[(conv)|(bn)](\d+)', comp[-1])
        if m is not None:
            comp[-1] = m.group(1)
        elif len(comp) > 1:
            if comp[-2] != 'downsample':
                raise ValueError('unexpected parameter name %s' % name)
            comp = comp[:-1]
        elif comp[-1] != 'conv':
            raise ValueError('unexpected parameter name %s' % name)
        return '.'.join(comp)

    # ------------------------------------------------------------------ preparation: packed weights + folded BN
    def _prepare(self, dev):
        """prep[conv] = (wp, scale, shift, Cin as packed, Cout, k); prep['wino'][id(wp)] = Winograd copy of the stride-1 3x3 filters."""
        ver = (dev, self._versions())
        prep = self._cached_prep(ver)
        if prep is not None:
            return prep
        L = _hip.lib()
        st = _hip.stream()
        prep, wino = {}, {}

        def fold(conv, bn):
            wp, cin, cout, k = parts.pack_weight(L, st, dev, conv.weight)      # (the stem's 3 input channels are zero-padded to the 4-channel NHWC image)
            prep[conv] = (wp,) + parts.affine(L, st, dev, conv, bn) + (cin, cout, k)
            if _hip.wino_eligible(cout, cin, k, conv.stride[0]) and conv.padding[0] == 1:
                wino[id(wp)] = _hip.wino_weight(wp, cout, cin)     # (conv2 of every block)
        fold(self.conv1, self.bn1)
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                for conv, bn, _, _ in blk.convs():
                    fold(conv, bn)
                if blk.downsample is not None:
                    fold(blk.downsample[0], blk.downsample[1])
        fold(self.conv, None)
        prep['wino'] = wino
        self._cache = (ver, prep)
        return prep

    def _plan(self, prep, dev, B, cin0, H, W):
        key = self._plan_key(dev, B, cin0, H, W)
        plan = self._plans.get(key)
        if plan is not None:
            if plan['prep'] is not prep:
                for p, conv in zip([plan['stem']] + list(plan['arr']), plan['convs']):
                    wp, scale, shift = prep[conv][:3]
                    parts.PlanBuilder.rebind(p, prep['wino'].get(id(wp)) if p.algo in _hip.ALGOS_READ_U else wp, scale, shift)
                plan['prep'] = prep
            return plan
        build = parts.PlanBuilder(dev)
        new = build.new
        ulist, conv_order = {}, []

        def conv_params(conv, x, h, w, ldx, y, stride, pad, slope, residual=None):
            wp, scale, shift, cin, cout, k = prep[conv]
            p, f = parts.conv_params(x, wp, scale, shift, B, h, w, cin, ldx, cout, k, slope, y=y, ldy=cout, residual=residual, ldr=cout,
                                     stride=stride, pad=pad, real_cin=conv.weight.shape[1])
            build.flops += f
            ulist[id(p)] = prep['wino'].get(id(wp))
            conv_order.append(conv)
            return p

        cpad = parts.pad4(cin0)
        x4 = new(B, H, W, cpad)
        c1 = self.conv1.weight.shape[0]
        h1, w1 = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
        stem = new(B, h1, w1, c1)
        p_stem = conv_params(self.conv1, x4, H, W, cpad, stem, 2, 3, 0.0)
        h, w = (h1 + 2 - 3) // 2 + 1, (w1 + 2 - 3) // 2 + 1
        pooled = new(B, h, w, c1)
        plist = []
        cur, ld = pooled, c1
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                s = blk.stride
                ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
                cout_blk = blk.convs()[-1][0].weight.shape[0]
                residual = cur
                if blk.downsample is not None:
                    residual = new(B, ho, wo, cout_blk)
                    plist.append(conv_params(blk.downsample[0], cur, h, w, ld, residual, s, 0, 1.0))   # BN folded, no activation
                t, th, tw, tld = cur, h, w, ld
                convs = blk.convs()
                for i, (conv, bn, cs, cp) in enumerate(convs):
                    co = conv.weight.shape[0]
                    oh, ow = (th + 2 * cp - conv.kernel_size[0]) // cs + 1, (tw + 2 * cp - conv.kernel_size[0]) // cs + 1
                    out = new(B, oh, ow, co)
                    last = i == len(convs) - 1
                    plist.append(conv_params(conv, t, th, tw, tld, out, cs, cp, 0.0, residual=residual if last else None))   # ReLU = slope 0
                    t, th, tw, tld = out, oh, ow, co
                cur, h, w, ld = t, th, tw, tld
        head_index = len(plist)
        plist.append(conv_params(self.conv, cur, h, w, ld, cur, 1, 0, 1.0))
        head_shape = (B, h, w, self.conv.weight.shape[0])
        tuned = [p_stem] + plist[:head_index]      # (the head runs the default kernel)
        for p in tuned:
            _hip.autotune_conv(p, dev, wino_w=ulist.get(id(p)))
        ws = build.share_workspace(tuned, unsized=plist[head_index:])
        arr = (_hip.ConvParams * len(plist))(*plist)
        plan = dict(key=key, x4=x4, cpad=cpad, stem=p_stem, stem_out=stem, stem_hw=(h1, w1, c1), pooled=pooled, arr=arr, n=len(plist), head_index=head_index,
                    head_shape=head_shape, flops=build.flops, convs=conv_order, prep=prep, keep=(build.keep, ws))
        self._plans.put(key, plan, build.nbytes)
        return plan

    def forward_nhwc(self, x):
        x, B, cin0, H, W, dev = parts.enter(x)
        L = _hip.lib()
        prep = self._prepare(dev)
        plan = self._plan(prep, dev, B, cin0, H, W)
        st = _hip.stream()
        out = torch.empty(plan['head_shape'], dtype=torch.float32, device=dev)
        plan['arr'][plan['head_index']].y = out.data_ptr()
        e0 = parts.profile_begin(self)
        _hip.check(L.y2_nchw_to_nhwc(_hip.ptr(x), _hip.ptr(plan['x4']), B, cin0, H, W, plan['cpad'], st), 'y2_nchw_to_nhwc')
        _hip.check(L.y2_conv_fwd(ctypes.byref(plan['stem']), st), 'y2_conv_fwd')
        h1, w1, c1 = plan['stem_hw']
        _hip.check(L.y2_maxpool_fwd(_hip.ptr(plan['stem_out']), _hip.ptr(plan['pooled']), B, h1, w1, c1, c1, c1, 3, 2, 1, 1, st), 'y2_maxpool_fwd')
        _hip.check(L.y2_conv_fwd_batch(plan['arr'], plan['n'], st), 'y2_conv_fwd_batch')
        parts.profile_end(self, e0, plan['flops'])
        return out


def _make(block, layers):
    def ctor(config_channels, anchors, num_cls, **kwargs):
        net = ResNet(config_channels, anchors, num_cls, block, layers, **kwargs)
        parts.refuse_pretrained(config_channels, 'model.resnet')      # model/resnet.py:164-171
        return net
    return ctor


resnet18 = _make(BasicBlock, [2, 2, 2, 2])
resnet34 = _make(BasicBlock, [3, 4, 6, 3])
resnet50 = _make(Bottleneck, [3, 4, 6, 3])
resnet101 = _make(Bottleneck, [3, 4, 23, 3])
resnet152 = _make(Bottleneck, [3, 8, 36, 3])
