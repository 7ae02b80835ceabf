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
inference (the depthwise kernel then takes its scalar path).  nn.Conv2d / nn.BatchNorm2d are parameter containers only.  Training
runs through model/train_oplist.py (OpListTrainFn, _build_mobilenet: batch-statistics BN, depthwise data / weight gradients by
y2_dwconv_dgrad / y2_dwconv_wgrad); it needs every width to be a multiple of 4.
"""
import collections
import ctypes

import torch
import torch.nn as nn

import model
import _hip

BN_EPS = 1e-5
STRIDES = (1, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 2, 1)                      # layers.1 .. layers.13 (model/mobilenet.py:58-70)
WIDTHS = (64, 128, 128, 256, 256, 512, 512, 512, 512, 512, 512, 1024, 1024)


def _pad4(c):
    return (c + 3) // 4 * 4


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


class MobileNet(nn.Module):
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
        self._cache = None
        self._plans = _hip.PlanCache()
        self.profile = None
        self.grad_ready_hook = None   # train.DataParallelRCCL: called as hook(param, grad) from inside backward

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

    @property
    def _plan_cache(self):
        """(tools / bench) the most recently used plan as (key, plan), None before the first forward."""
        plan = self._plans.latest()
        return None if plan is None else (plan['key'], plan)

    @_plan_cache.setter
    def _plan_cache(self, value):
        assert value is None
        self._plans.clear()

    # ------------------------------------------------------------------ preparation: packed weights + folded BN
    def _versions(self):
        return tuple((p.data_ptr(), p._version) for p in list(self.parameters()) + list(self.buffers()))

    def _prepare(self, dev):
        ver = (dev, self._versions())
        if self._cache is not None and self._cache[0] == ver:
            return self._cache[1]
        L = _hip.lib()
        st = _hip.stream()
        prep = {}

        def affine(conv, bn):
            cout = conv.weight.shape[0]
            if bn is None:
                return None, (_hip.f32c(conv.bias.detach()) if conv.bias is not None else None)
            scale, shift = torch.empty(cout, device=dev), torch.empty(cout, device=dev)
            _hip.check(L.y2_bn_fold(_hip.ptr(_hip.f32c(bn.weight.detach())), _hip.ptr(_hip.f32c(bn.bias.detach())), _hip.ptr(_hip.f32c(bn.running_mean)),
                                    _hip.ptr(_hip.f32c(bn.running_var)), BN_EPS, _hip.ptr(scale), _hip.ptr(shift), cout, st), 'y2_bn_fold')
            return scale, shift

        def fold(conv, bn):
            w = _hip.f32c(conv.weight.detach())
            _hip.require_gpu(w)
            cout, cin, k, _ = w.shape
            if cin % 4:                                   # zero-padded input channels (the 3-channel image, pruned widths)
                wpad = torch.zeros(cout, _pad4(cin), k, k, dtype=torch.float32, device=dev)
                wpad[:, :cin] = w
                w, cin = wpad, wpad.shape[1]
            wp = torch.empty(w.numel(), dtype=torch.float32, device=dev)
            _hip.check(L.y2_pack_weight(_hip.ptr(w), _hip.ptr(wp), cout, cin, k, 0, st), 'y2_pack_weight')
            scale, shift = affine(conv, bn)
            prep[conv] = (wp, scale, shift, cin, cout, k)

        def fold_dw(conv, bn):
            w = _hip.f32c(conv.weight.detach())           # [C][1][3][3]: read as it is by y2_dwconv_fwd
            _hip.require_gpu(w)
            scale, shift = affine(conv, bn)
            prep[conv] = (w, scale, shift)
        fold(self.stem().conv, self.stem().bn)
        for _, unit, _ in self.units():
            fold_dw(unit.dw.conv, unit.dw.bn)
            fold(unit.pw.conv, unit.pw.bn)
        fold(self.head(), None)
        self._cache = (ver, prep)
        return prep

    def _plan(self, prep, dev, B, cin0, H, W):
        widths = tuple(tuple(m.weight.shape) for m in self.modules() if isinstance(m, nn.Conv2d))      # (pruned / replaced layers re-plan)
        key = (str(dev), B, cin0, H, W, _hip.tune_epoch(), _hip.WINOGRAD, _hip.FORCE_ALGO, widths)
        plan = self._plans.get(key)
        if plan is not None:
            if plan['prep'] is not prep:      # same shape, new parameter version: only the weight / affine pointers move
                for step in plan['steps']:
                    if step[0] == 'conv':
                        p, conv = step[1], step[2]
                        wp, scale, shift = prep[conv][:3]
                        p.w = wp.data_ptr()
                        p.scale = scale.data_ptr() if scale is not None else None
                        p.shift = shift.data_ptr() if shift is not None else None
                    else:
                        step[2] = prep[step[1]]
                plan['prep'] = prep
            return plan
        nbytes = [0]

        def new(*s):
            t = torch.zeros(*s, dtype=torch.float32, device=dev)       # zero: the channel padding of every activation stays zero
            nbytes[0] += t.numel() * 4
            return t
        keep, steps, flops = [], [], [0.0]

        def conv_step(conv, x, h, w, ldx, y, ldy, stride, pad, slope):
            wp, scale, shift, cin, cout, k = prep[conv]
            p = _hip.ConvParams()
            p.x, p.w = x.data_ptr(), wp.data_ptr()
            p.scale = scale.data_ptr() if scale is not None else None
            p.shift = shift.data_ptr() if shift is not None else None
            p.y, p.ldy = y.data_ptr(), ldy
            p.B, p.H, p.W, p.Cin, p.ldx, p.Cout, p.ksize = B, h, w, cin, ldx, cout, k
            p.stride, p.pad_plus1, p.slope, p.tile = stride, pad + 1, slope, 0
            ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
            flops[0] += 2.0 * conv.weight.shape[1] * cout * k * k * B * ho * wo
            steps.append(['conv', p, conv])
            return ho, wo

        cpad = _pad4(cin0)
        x4 = new(B, H, W, cpad)
        keep.append(x4)
        c = self.stem().conv.weight.shape[0]
        ld = _pad4(c)
        h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        cur = new(B, h, w, ld)
        keep.append(cur)
        conv_step(self.stem().conv, x4, H, W, cpad, cur, ld, 2, 1, 0.0)
        for _, unit, s in self.units():
            ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
            d = new(B, ho, wo, ld)
            keep.append(d)
            steps.append(['dw', unit.dw.conv, prep[unit.dw.conv], cur, d, B, h, w, c, ld, ld, s])
            flops[0] += 2.0 * 9 * B * ho * wo * c
            co = unit.pw.conv.weight.shape[0]
            ldo = _pad4(co)
            y = new(B, ho, wo, ldo)
            keep.append(y)
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
        need = max([_hip.lib().y2_conv_fwd_workspace_bytes(ctypes.byref(p)) for p in convs] + [0])
        ws = _hip.workspace(dev, need) if need > 0 else None
        for p in convs:
            p.workspace, p.workspace_bytes = (ws.data_ptr(), ws.numel() * 4) if ws is not None else (None, 0)
        plan = dict(key=key, x4=x4, cpad=cpad, steps=steps, head=head_p, head_shape=head_shape, flops=flops[0], prep=prep, keep=(keep, ws))
        self._plans.put(key, plan, nbytes[0])
        return plan

    def forward_nhwc(self, x):
        _hip.require_gpu(x)
        L = _hip.lib()
        x = _hip.f32c(x)
        B, cin0, H, W = x.shape
        if H % 32 or W % 32:
            raise ValueError('input size must be a multiple of 32 (got %dx%d)' % (H, W))
        dev = x.device
        prep = self._prepare(dev)
        plan = self._plan(prep, dev, B, cin0, H, W)
        st = _hip.stream()
        out = torch.empty(plan['head_shape'], dtype=torch.float32, device=dev)
        plan['head'].y = out.data_ptr()
        prof = self.profile
        if prof is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        _hip.check(L.y2_nchw_to_nhwc(_hip.ptr(x), _hip.ptr(plan['x4']), B, cin0, H, W, plan['cpad'], st), 'y2_nchw_to_nhwc')
        for step in plan['steps']:
            if step[0] == 'conv':
                _hip.check(L.y2_conv_fwd(ctypes.byref(step[1]), st), 'y2_conv_fwd')
            else:
                _, _, (wt, scale, shift), xin, y, b, h, w, c, ldx, ldy, s = step
                _hip.check(L.y2_dwconv_fwd(_hip.ptr(xin), _hip.ptr(wt), _hip.ptr(scale), _hip.ptr(shift), 0.0, _hip.ptr(y), None,
                                           b, h, w, c, ldx, ldy, s, st), 'y2_dwconv_fwd')
        if prof is not None:
            e1.record()
            prof.append(('conv_fwd', plan['flops'], e0, e1))
        return out

    def forward(self, x):
        if self.training:        # BN semantics follow self.training alone (see model.yolo2.Darknet.forward)
            from model import train_oplist
            return train_oplist.forward(self, x)
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            from model import train_oplist
            return train_oplist.forward(self, x, frozen=True)     # differentiable eval mode: frozen BatchNorm statistics
        with torch.no_grad():
            out = self.forward_nhwc(x)
        return out.permute(0, 3, 1, 2)
