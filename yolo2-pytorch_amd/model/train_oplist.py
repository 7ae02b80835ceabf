"""The op-list training graph: model.yolo2.Tiny, model.resnet.ResNet, model.mobilenet.MobileNet and model.densenet.DenseNet.

forward(net, x) records the network as a list of operations while it launches them - a builder function per architecture drives a
_Recorder, whose conv_bn / dwconv_bn / maxpool methods launch one operation each and note what its backward needs - and
OpListTrainFn.backward walks that list in reverse with gradient fan-in per tensor.  A new backbone is a builder over the recorder
(and an entry in _builder); the parts shared with the Darknet graph of model/train_graph.py live in model/_train_parts.py.  For inference
the same backbone writes a class on model/_infer_parts.InferMixin with its own _prepare (pack_weight / fold_bn per layer), _plan (a walk that
fills conv_params into a PlanBuilder) and forward_nhwc (enter, the launches)."""
import torch

import _hip
from model._train_parts import BN_MOMENTUM, LEAKY, PLUGIN_MOMENTUM, GradSink, StatsArena, _new, bn_params, cached_buf, gen_conv, prep_weights


class _ROp(object):
    """One recorded operation of the training forward (conv+BN+ReLU[+residual], a max-pool, or a depthwise conv+BN+ReLU)."""
    __slots__ = ('kind', 'conv', 'bn', 'x', 'ldx', 'h', 'w', 'ho', 'wo', 'stride', 'pad', 'k', 'cin', 'cout', 'z', 'scale', 'shift', 'mean', 'invstd',
                 'residual', 'y', 'slope', 'first', 'pool', 'filt')       # pool = (ksize, stride, pad, pad_end) of a 'pool' op; filt = the filter of a 'dw' op


def forward(net, x, frozen=False):
    """Training-mode forward of a plugin; returns the NCHW view like the inference path.
    frozen: eval()-mode BatchNorm (running statistics, nothing updated) with autograd recording."""
    params = [p for p in net.parameters()]
    out = OpListTrainFn.apply(net, x, frozen, *params)
    return out.permute(0, 3, 1, 2)


def _operands(net, dev, scope=None):
    """{nn.Conv2d: dict(wp, wd)}: the forward / data-gradient GEMM operands of every convolution of a plugin whose channel
    counts need no padding, derived by ONE y2_prep_weights launch per parameter version (the per-layer path costs two y2_pack_weight
    launches per convolution and step: 107 for ResNet-50).  scope: see train_graph._train_operands."""
    import torch.nn as nn
    convs = [m for m in net.modules() if isinstance(m, nn.Conv2d)]
    key = (dev, tuple((c.weight.data_ptr(), c.weight._version) for c in convs))
    if scope is not None:
        bufs = scope
    else:
        cache = net.__dict__.get('_train_cache')
        if cache is not None and cache[0] == key:
            return cache[1]
        held = net.__dict__.get('_train_bufs')
        if held is None or held[0] != dev:
            held = net.__dict__['_train_bufs'] = (dev, {})
        bufs = held[1]
    items, ops = [], {}
    for i, c in enumerate(convs):
        w = c.weight.detach()
        cout, cin, k, _ = w.shape
        if cout % 4 or cin % 4 or not w.is_contiguous() or w.dtype != torch.float32 or not w.is_cuda:
            continue          # the 3-channel stem and the 425-wide head run zero-padded: per-layer path
        d = {}
        for tag, mode in (('wp', _hip.PREP_FPROP), ('wd', _hip.PREP_DGRAD)):
            d[tag] = cached_buf(bufs, ('rn', i, tag), w.numel(), dev)
            items.append((w, d[tag], cout, cin, k, mode))
        ops[c] = d
    prep_weights(items)
    if scope is None:
        net.__dict__['_train_cache'] = (key, ops)
    return ops


class _Recorder(object):
    """One forward pass being recorded: what every builder needs (L, st, dev, B, frozen, the statistics arena, the prepared operands, the
    4-channel NHWC image x4) and `ops`, the list its methods append to.  Each method launches one operation and returns its output."""

    def __init__(self, net, x, frozen, scope):
        import torch.nn as nn
        self.L, self.st, self.dev, self.frozen = _hip.lib(), _hip.stream(), x.device, frozen
        self.B, self.cin0, self.H, self.W = x.shape
        self.ops, self.dense = [], None
        self.prepared = _operands(net, self.dev, scope)
        self.stats = StatsArena(self.dev, sum(m.num_features for m in net.modules() if isinstance(m, nn.BatchNorm2d)), frozen)
        self.cpad = (self.cin0 + 3) // 4 * 4
        self.x4 = _new(self.dev, self.B, self.H, self.W, self.cpad)
        _hip.check(self.L.y2_nchw_to_nhwc(_hip.ptr(x), _hip.ptr(self.x4), self.B, self.cin0, self.H, self.W, self.cpad, self.st), 'y2_nchw_to_nhwc')

    def conv_bn(self, conv, bn, xin, ldx, h, w, stride, pad, slope, residual=None, first=False, momentum=PLUGIN_MOMENTUM):
        """conv (general kernel, BN statistics in the epilogue) -> BN -> [+ residual] -> activation.  Returns (y, ho, wo, cout)."""
        L, st, dev, B = self.L, self.st, self.dev, self.B
        op = _ROp()
        weight = _hip.f32c(conv.weight.detach())
        cout, cin_true, k, _ = weight.shape
        if ldx % 4 or (cin_true % 4 and not first):
            raise RuntimeError('training needs conv input channel counts that are multiples of 4 (got %d)' % cin_true)
        if cin_true != ldx:           # stem: zero-padded input channels
            wpad = torch.zeros(cout, ldx, k, k, dtype=torch.float32, device=dev)
            wpad[:, :cin_true] = weight
            weight = wpad
        if conv in self.prepared and cin_true == ldx:
            wp = self.prepared[conv]['wp']
        else:
            wp = _new(dev, weight.numel())
            _hip.check(L.y2_pack_weight(_hip.ptr(weight), _hip.ptr(wp), cout, ldx, k, 0, st), 'y2_pack_weight')
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        z = _new(dev, B, ho, wo, cout)
        stats = self.stats.take(cout) if (bn is not None and not self.frozen) else None
        gen_conv(L, st, xin, wp, z, B, h, w, ldx, ldx, cout, k, stride, pad, stats=self.stats.epilogue(stats))
        self.stats.settle(stats, z, B * ho * wo, cout, cout)
        op.kind, op.conv, op.bn, op.x, op.ldx, op.h, op.w, op.ho, op.wo = 'conv', conv, bn, xin, ldx, h, w, ho, wo
        op.stride, op.pad, op.k, op.cin, op.cout, op.z, op.residual, op.slope, op.first = stride, pad, k, cin_true, cout, z, residual, slope, first
        return self._bn_act(op, stats, momentum)

    def _bn_act(self, op, stats, momentum):
        L, st, dev, B = self.L, self.st, self.dev, self.B
        bn, cout, ho, wo, residual = op.bn, op.cout, op.ho, op.wo, op.residual
        if bn is not None:
            op.scale, op.shift, op.mean, op.invstd = bn_params(L, st, dev, bn, stats, B * ho * wo, cout, self.frozen, momentum)
        else:
            op.scale = op.mean = op.invstd = None
            op.shift = _hip.f32c(op.conv.bias.detach()) if op.conv.bias is not None else None
        y = _new(dev, B, ho, wo, cout)
        _hip.check(L.y2_bn_act_fwd_ex(_hip.ptr(op.z), _hip.ptr(op.scale), _hip.ptr(op.shift), op.slope, _hip.ptr(residual), cout if residual is not None else 0,
                                      _hip.ptr(y), None, B, ho, wo, cout, cout, cout, 0, 0, 0, 0, st), 'y2_bn_act_fwd_ex')
        op.y = y
        self.ops.append(op)
        return y, ho, wo, cout

    def dwconv_bn(self, conv, bn, xin, C, h, w, stride):
        """depthwise 3x3 / pad 1 (model/mobilenet.py conv_dw): raw output with the BN statistics, then the shared BN + ReLU step.  Returns (y, ho, wo)."""
        L, st, dev, B = self.L, self.st, self.dev, self.B
        op = _ROp()
        weight = _hip.f32c(conv.weight.detach())
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        z = _new(dev, B, ho, wo, C)
        stats = self.stats.take(C) if not self.frozen else None
        _hip.check(L.y2_dwconv_fwd(_hip.ptr(xin), _hip.ptr(weight), None, None, 1.0, _hip.ptr(z), _hip.ptr(self.stats.epilogue(stats)),
                                   B, h, w, C, C, C, stride, st), 'y2_dwconv_fwd')
        self.stats.settle(stats, z, B * ho * wo, C, C)
        op.kind, op.conv, op.bn, op.x, op.ldx, op.h, op.w, op.ho, op.wo = 'dw', conv, bn, xin, C, h, w, ho, wo
        op.stride, op.pad, op.k, op.cin, op.cout, op.z, op.residual, op.slope, op.first = stride, 1, 3, C, C, z, None, 0.0, False
        op.filt = weight           # the data gradient reads the filter the forward read
        return self._bn_act(op, stats, PLUGIN_MOMENTUM)[:3]

    def maxpool(self, cur, h, w, ld, ksize, stride, pad, pad_end):
        L, dev, B = self.L, self.dev, self.B
        pool = _ROp()
        pool.kind, pool.x, pool.h, pool.w, pool.cout, pool.pool = 'pool', cur, h, w, ld, (ksize, stride, pad, pad_end)
        ph, pw = (h + pad + pad_end - ksize) // stride + 1, (w + pad + pad_end - ksize) // stride + 1
        pooled = _new(dev, B, ph, pw, ld)
        _hip.check(L.y2_maxpool_fwd(_hip.ptr(cur), _hip.ptr(pooled), B, h, w, ld, ld, ld, ksize, stride, pad, pad_end, self.st), 'y2_maxpool_fwd')
        pool.y, pool.ho, pool.wo = pooled, ph, pw
        self.ops.append(pool)
        return pooled, ph, pw


# ---- one builder per architecture: launches and records the network's operations through a _Recorder, returns the head image (NHWC)
def _build_tiny(rec, net):
    """model/yolo2.py:140-173: nn.Sequential of Conv2d blocks (BN momentum 0.01, LeakyReLU 0.1), MaxPool2d(2) and the
    ConstantPad2d((0,1,0,1)) + MaxPool2d(2, stride=1) pair; the 3-channel input runs zero-padded to 4 NHWC channels."""
    from model import yolo2 as _yolo2
    cur, h, w, ld = rec.x4, rec.H, rec.W, rec.cpad
    mods = list(net.layers)
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, _yolo2.Conv2d):
            cur, h, w, ld = rec.conv_bn(m.conv, m.bn, cur, ld, h, w, 1, (m.kernel_size - 1) // 2, LEAKY if m.has_act else 1.0, first=(i == 0), momentum=BN_MOMENTUM)
        elif isinstance(m, _yolo2._PadPool):
            cur, h, w = rec.maxpool(cur, h, w, ld, 2, 1, 0, 1)
            i += 1          # the pad + pool pair
        else:
            cur, h, w = rec.maxpool(cur, h, w, ld, 2, 2, 0, 0)
        i += 1
    return cur


def _build_mobilenet(rec, net):
    """model/mobilenet.py:54-85: 3x3/s2 stem, 13 units of {depthwise 3x3 + BN + ReLU, pointwise 1x1 + BN + ReLU}, 1x1 head with bias."""
    for name, conv in [('layers.0.conv', net.stem().conv)] + [('%s.pw.conv' % n, u.pw.conv) for n, u, _ in net.units()]:
        if conv.weight.shape[0] % 4:
            raise RuntimeError('model.mobilenet: training needs widths that are multiples of 4 (%s.weight has %d output channels)' % (name, conv.weight.shape[0]))
    stem = net.stem()
    cur, h, w, ld = rec.conv_bn(stem.conv, stem.bn, rec.x4, rec.cpad, rec.H, rec.W, 2, 1, 0.0, first=True)
    for _, unit, s in net.units():
        cur, h, w = rec.dwconv_bn(unit.dw.conv, unit.dw.bn, cur, ld, h, w, s)
        cur, h, w, ld = rec.conv_bn(unit.pw.conv, unit.pw.bn, cur, ld, h, w, 1, 0, 0.0)
    return rec.conv_bn(net.head(), None, cur, ld, h, w, 1, 0, 1.0)[0]


def _build_resnet(rec, net):
    """model/resnet.py:29-158: 7x7/s2 stem + max-pool, per block the projection shortcut then its convolutions (the last one adds the
    residual before its ReLU), 1x1 head with bias."""
    cur, h, w, ld = rec.conv_bn(net.conv1, net.bn1, rec.x4, rec.cpad, rec.H, rec.W, 2, 3, 0.0, first=True)
    cur, h, w = rec.maxpool(cur, h, w, ld, 3, 2, 1, 1)
    for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
        for blk in layer:
            residual = cur
            if blk.downsample is not None:
                residual, _, _, _ = rec.conv_bn(blk.downsample[0], blk.downsample[1], cur, ld, h, w, blk.stride, 0, 1.0)
            t, th, tw, tld = cur, h, w, ld
            convs = blk.convs()
            for i, (conv, bn, cs, cp) in enumerate(convs):
                last = i == len(convs) - 1
                t, th, tw, tld = rec.conv_bn(conv, bn, t, tld, th, tw, cs, cp, 0.0, residual=residual if last else None)
            cur, h, w, ld = t, th, tw, tld
    return rec.conv_bn(net.conv, None, cur, ld, h, w, 1, 0, 1.0)[0]


class _DOp(object):
    """One recorded DenseNet operation.  kind 'pre': BatchNorm -> ReLU -> 1x1 convolution [-> AvgPool 2x2] on the first K channels of a block buffer
    (norm1 + conv1 of a dense layer with its norm2 + ReLU behind it; a transition; norm5 + the head); kind 'grow': the raw 3x3 convolution that
    appends growth_rate channels to the block buffer."""
    __slots__ = ('kind', 'bn', 'conv', 'buf', 'gbuf', 'K', 'ld', 'h', 'w', 'pool', 'pre_slope', 'scale', 'shift', 'mean', 'invstd', 'N', 'z', 'bn2', 'scale2',
                 'shift2', 'mean2', 'invstd2', 'a2', 'out', 'out_ld', 'out_off', 'role')


def _build_densenet(rec, net):
    """model/densenet.py:29-65.  A dense block is one buffer [B, h, w, C_end]; the batch statistics of a slab of it (the stem's pooled output, a
    transition's output, the growth_rate channels of a layer) are taken ONCE, by its producer, and every consumer's BatchNorm finalises from them
    with its own gamma / beta and updates its own running statistics (the reference recomputes the identical statistics per consumer).
    The stem goes through the recorder's ops; the blocks are 'pre' / 'grow' ops of their own, left in rec.dense for _densenet_bwd."""
    import torch.nn as nn
    L, st, dev, B, frozen, arena = rec.L, rec.st, rec.dev, rec.B, rec.frozen, rec.stats
    f = net.features
    for name, m in net.named_modules():
        if isinstance(m, nn.Conv2d) and m is not f.conv and (m.weight.shape[0] % 4 or (m.weight.shape[1] % 4 and m is not f.conv0)):
            raise RuntimeError('model.densenet: training needs widths that are multiples of 4 (%s.weight is %s)' % (name, tuple(m.weight.shape)))
    dops = []

    def finalize(bn, slabs, C, count):
        return bn_params(L, st, dev, bn, slabs, count, C, frozen, PLUGIN_MOMENTUM)

    def pre(role, bn, conv, buf, slabs, K, ld, h, w, pool, pre_slope, out, out_ld, out_off, shift=None, want_stats=False):
        op = _DOp()
        op.kind, op.role, op.bn, op.conv, op.buf, op.K, op.ld, op.h, op.w, op.pool, op.pre_slope = 'pre', role, bn, conv, buf, K, ld, h, w, pool, pre_slope
        op.scale, op.shift, op.mean, op.invstd = finalize(bn, slabs, K, B * h * w)
        op.N = N = conv.weight.shape[0]
        op.out, op.out_ld, op.out_off, op.bn2 = out, out_ld, out_off, None
        stats = arena.take(N) if (want_stats and not frozen) else None
        _hip.check(L.y2_preact_conv1x1_fwd(_hip.ptr(buf), _hip.ptr(_hip.f32c(conv.weight.detach())), _hip.ptr(op.scale), _hip.ptr(op.shift), pre_slope, None,
                                           _hip.ptr(shift), 1.0, _hip.ptr(out), _hip.ptr(arena.epilogue(stats)), B, h, w, K, ld, N, out_ld, out_off, pool, st),
                   'y2_preact_conv1x1_fwd')
        ho, wo = (h // 2, w // 2) if pool else (h, w)
        arena.settle(stats, out.view(-1)[out_off:], B * ho * wo, N, out_ld)
        dops.append(op)
        return op, stats

    # ---- stem: conv0 + norm0 + ReLU + MaxPool2d(3, 2, 1) (the ResNet stem ops), copied into block buffer 1
    c0 = f.conv0.weight.shape[0]
    cur, h, w, _ = rec.conv_bn(f.conv0, f.norm0, rec.x4, rec.cpad, rec.H, rec.W, 2, 3, 0.0, first=True)
    pooled, h, w = rec.maxpool(cur, h, w, c0, 3, 2, 1, 1)
    c, buf, prev = c0, None, None
    blocks = net.blocks()
    for bi, (block, trans) in enumerate(blocks):
        c_end = c + sum(layer.conv2.weight.shape[0] for layer in block)
        nxt = _new(dev, B, h, w, c_end)
        if bi == 0:
            _hip.check(L.y2_bn_act_fwd(_hip.ptr(pooled), None, None, 1.0, _hip.ptr(nxt), None, B, h, w, c0, c0, c_end, 0, 0, 0, 0, st), 'y2_bn_act_fwd')
            pstats = None if frozen else arena.take(c0)          # the pooled slab has no producing convolution: its statistics are reduced here, in every mode
            if pstats is not None:
                _hip.colstats_det(pooled, B * h * w, c0, c0, pstats)
            slabs = [(0, c0, pstats)]
        else:
            pbuf, pslabs, pc, ph, pw, ptr_ = prev
            op, stats = pre('trans', ptr_.norm, ptr_.conv, pbuf, pslabs, pc, pc, ph, pw, 1, 0.0, nxt, c_end, 0, want_stats=True)
            slabs = [(0, c, stats)]
        buf = nxt
        for layer in block:
            n1, g = layer.conv1.weight.shape[0], layer.conv2.weight.shape[0]
            z1 = _new(dev, B, h, w, n1)
            op, stats1 = pre('layer', layer.norm1, layer.conv1, buf, slabs, c, c_end, h, w, 0, 0.0, z1, n1, 0, want_stats=True)
            op.z, op.bn2 = z1, layer.norm2
            op.scale2, op.shift2, op.mean2, op.invstd2 = finalize(layer.norm2, [(0, n1, stats1)], n1, B * h * w)
            a2 = _new(dev, B, h, w, n1)
            _hip.check(L.y2_bn_act_fwd_ex(_hip.ptr(z1), _hip.ptr(op.scale2), _hip.ptr(op.shift2), 0.0, None, 0, _hip.ptr(a2), None, B, h, w, n1, n1, n1, 0, 0, 0, 0, st),
                       'y2_bn_act_fwd_ex')
            op.a2 = a2
            # the raw 3x3 / pad 1 convolution of the layer writes its g channels at channel offset c of the block buffer
            gstats = arena.take(g) if not frozen else None
            gen_conv(L, st, a2, rec.prepared[layer.conv2]['wp'], buf, B, h, w, n1, n1, g, 3, 1, 1, ldy=c_end, coff=c, stats=arena.epilogue(gstats))
            arena.settle(gstats, buf.view(-1)[c:], B * h * w, g, c_end)
            grow = _DOp()
            grow.kind, grow.conv, grow.buf, grow.K, grow.ld, grow.h, grow.w, grow.N, grow.a2, grow.out_off = 'grow', layer.conv2, buf, n1, c_end, h, w, g, a2, c
            dops.append(grow)
            slabs.append((c, g, gstats))
            c += g
        if trans is not None:
            prev = (buf, slabs, c_end, h, w, trans)
            c = trans.conv.weight.shape[0]
            h, w = h // 2, w // 2
    nout = f.conv.weight.shape[0]
    out = _new(dev, B, h, w, nout)
    op, _ = pre('head', f.norm5, f.conv, buf, slabs, c, c, h, w, 0, 1.0, out, nout, 0, shift=_hip.f32c(f.conv.bias.detach()))
    op.z = out
    rec.dense = dict(ops=dops, pooled=pooled, c0=c0)
    return out


def _builder(net):
    """The builder function of a network's class."""
    from model import densenet, mobilenet, resnet, yolo2
    for cls, build in ((yolo2.Tiny, _build_tiny), (mobilenet.MobileNet, _build_mobilenet), (densenet.DenseNet, _build_densenet), (resnet.ResNet, _build_resnet)):
        if isinstance(net, cls):
            return build
    raise TypeError('model.train_oplist: no training-graph builder for %s.%s (Tiny, MobileNet, DenseNet and ResNet have one; Darknet trains through model.train_graph)'
                    % (type(net).__module__, type(net).__name__))


def _densenet_bwd(ctx, dout, sink):
    """Reverse walk of the 'pre' / 'grow' ops.  Every block has ONE gradient buffer [B, h, w, C_end]: the block's consumer (transition / head) writes
    all of it through y2_preact_bwd, every layer then reads the finished gradient of its own slab and ADDS its input gradient into the first K
    channels.  Returns the gradient of the stem's pooled output (the ResNet stem ops finish the walk)."""
    L, st = _hip.lib(), _hip.stream()
    dense, B, net = ctx.dense, ctx.B, ctx.net
    dev = dout.device
    prepared = ctx.prepared
    dops = dense['ops']
    pres = [op for op in dops if op.kind == 'pre']
    total = sum(2 * op.K + (2 * op.N if op.bn2 is not None else 0) for op in pres)
    nout = pres[-1].N
    sums_arena = torch.empty(total + 2 * nout, dtype=torch.float64, device=dev)
    head = pres[-1]
    head_cop = (nout + 3) // 4 * 4
    head_dz = _new(dev, B, head.h, head.w, head_cop)
    head_dwp, head_w = _new(dev, head_cop * head.K), _new(dev, head_cop, head.K, 1, 1)
    zero = [sums_arena, head_dz, head_dwp, head_w]
    wbuf = {}
    for op in pres:          # the 1x1 weight gradients: [N][1][K] IS the state_dict layout; the direct kernel adds split partial sums into a zeroed buffer
        if op.role != 'head':
            wbuf[id(op)] = sink.dest(op.conv.weight)
            zero.append(wbuf[id(op)].view(-1))
    # 64 targets per call although y2_multi splits a longer table itself (at 96): with the 65 targets of DenseNet-121 one call would be one launch
    # where this walk has always issued two, and a restructuring of this file is checked by the step's launch list staying the same
    for i in range(0, len(zero), 64):
        _hip.multi([(_hip.MULTI_ZERO, t, None) for t in zero[i:i + 64]], st)
    has_bn = 2 if ctx.frozen else 1
    affine, off = [], 0
    gbufs = {}

    def gbuf_of(op):
        t = gbufs.get(id(op.buf))
        if t is None:
            t = gbufs[id(op.buf)] = _new(dev, *op.buf.shape)
        return t

    def dgrad(conv, dz, h, w, cop, ldz, cin, k, wd=None):
        if wd is None:
            wd = prepared[conv]['wd']
        dx = _new(dev, B, h, w, cin)
        gen_conv(L, st, dz, wd, dx, B, h, w, cop, ldz, cin, k, 1, k - 1 - (k - 1) // 2)
        return dx

    def bn_sums(bn, C):
        nonlocal off
        t = sums_arena[off:off + 2 * C]
        affine.append((bn.bias, off, C))
        affine.append((bn.weight, off + C, C))
        off += 2 * C
        return t

    for op in reversed(dops):
        h, w = op.h, op.w
        if op.kind == 'grow':
            # 3x3: weight gradient from (a2, gradient of the slab), data gradient -> gradient of a2 (kept on the op for the 'pre' op in front of it)
            gb = gbuf_of(op)
            dslab = gb.view(-1)[op.out_off:]
            n1, g = op.K, op.N
            dwp = _hip.conv_wgrad(op.a2, dslab, B, h, w, n1, n1, g, op.ld, 3)
            dw = sink.dest(op.conv.weight)
            _hip.check(L.y2_unpack_weight_grad(_hip.ptr(dwp), _hip.ptr(dw), g, n1, 3, st), 'y2_unpack_weight_grad')
            sink.ready(op.conv.weight, dw)
            op.z = dgrad(op.conv, dslab, h, w, g, op.ld, n1, 3)
            grow = op
            continue
        ho, wo = (h // 2, w // 2) if op.pool else (h, w)
        K, N = op.K, op.N
        if op.role == 'head':
            # bias + no activation (has_bn = 0: dz = dout, sums = d bias), written zero-padded to a multiple of 4 channels for the GEMM kernels
            cop, dz, dwp, wsrc = head_cop, head_dz, head_dwp, head_w
            bsum = sums_arena[total:total + 2 * N]
            _hip.check(L.y2_bn_act_bwd_ex(_hip.ptr(op.z), None, _hip.ptr(_hip.f32c(op.conv.bias.detach())), None, None, None, 1.0, _hip.ptr(_hip.f32c(dout)), N, 0, 0,
                                          None, 0, 0, None, 0, None, 0, None, 0, _hip.ptr(bsum), _hip.ptr(dz), cop, B, ho, wo, N, N, 0, st), 'y2_bn_act_bwd_ex')
            affine.append((op.conv.bias, total, N))
            ldz = cop
            wsrc[:N] = _hip.f32c(op.conv.weight.detach())
            wd = _new(dev, wsrc.numel())
            _hip.check(L.y2_pack_weight(_hip.ptr(wsrc), _hip.ptr(wd), cop, K, 1, 1, st), 'y2_pack_weight')
        elif op.role == 'trans':
            cop, wd = N, None
            nb = [o for o in dops if o.kind == 'pre' and o.buf is op.out][0]
            dz = gbuf_of(nb)          # the first N channels of the next block's gradient buffer
            ldz = op.out_ld
            dwp = wbuf[id(op)].view(-1)
        else:
            # norm2 + ReLU between the 1x1 and the 3x3: gradient of a2 (from the 'grow' op) -> gradient of the raw 1x1 output
            cop, wd, ldz = N, None, N
            dz = _new(dev, B, h, w, N)
            _hip.check(L.y2_bn_act_bwd_ex(_hip.ptr(op.z), _hip.ptr(op.scale2), _hip.ptr(op.shift2), _hip.ptr(op.mean2), _hip.ptr(op.invstd2),
                                          _hip.ptr(op.bn2.weight.detach()), 0.0, _hip.ptr(grow.z), N, 0, 0, None, 0, 0, None, 0, None, 0, None, 0,
                                          _hip.ptr(bn_sums(op.bn2, N)), _hip.ptr(dz), N, B, h, w, N, N, has_bn, st), 'y2_bn_act_bwd_ex')
            grow.z = None
            dwp = wbuf[id(op)].view(-1)
        # 1x1 weight gradient from the recomputed pre-activated operand
        act = _new(dev, B, ho, wo, K)
        _hip.check(L.y2_preact_fwd(_hip.ptr(op.buf), _hip.ptr(op.scale), _hip.ptr(op.shift), op.pre_slope, _hip.ptr(act), B, h, w, K, op.ld, K, op.pool, st), 'y2_preact_fwd')
        _hip.check(L.y2_conv_wgrad_ex(_hip.ptr(act), _hip.ptr(dz), _hip.ptr(dwp), B, ho, wo, K, K, cop, ldz, 1, 1, 0, st), 'y2_conv_wgrad_ex')
        if op.role == 'head':
            sink.ready(op.conv.weight, dwp.view(cop, K, 1, 1)[:N].contiguous())
        else:
            sink.ready(op.conv.weight, wbuf[id(op)])
        dA = dgrad(op.conv, dz, ho, wo, cop, ldz, K, 1, wd=wd)
        _hip.check(L.y2_preact_bwd(_hip.ptr(op.buf), _hip.ptr(op.scale), _hip.ptr(op.shift), op.pre_slope, _hip.ptr(op.mean), _hip.ptr(op.invstd),
                                   _hip.ptr(op.bn.weight.detach()), _hip.ptr(dA), K, _hip.ptr(bn_sums(op.bn, K)), _hip.ptr(gbuf_of(op)), op.ld,
                                   1 if op.role == 'layer' else 0, B, h, w, K, op.ld, op.pool, has_bn, st), 'y2_preact_bwd')
        op.z = op.a2 = None
    sink.hand_affine(sums_arena, affine, st)
    # ---- gradient of the stem's pooled output: the first c0 channels of block 1's gradient buffer
    first = dops[0]
    c0 = dense['c0']
    dpool = _new(dev, *dense['pooled'].shape)
    gb = gbufs[id(first.buf)]
    _hip.check(L.y2_bn_act_fwd(_hip.ptr(gb), None, None, 1.0, _hip.ptr(dpool), None, B, first.h, first.w, c0, first.ld, c0, 0, 0, 0, 0, st), 'y2_bn_act_fwd')
    ctx.dense = None
    return dpool


class OpListTrainFn(torch.autograd.Function):
    """Training graph of the plugins as a recorded op list.  'conv' op (model/resnet.py:29-158): {raw general conv with BN statistics in the
    epilogue -> y2_bn_finalize -> y2_bn_act_fwd_ex (affine [+ residual] + activation)}; backward in reverse with
    gradient fan-in per tensor: y2_bn_act_bwd_ex (activation mask from the recomputed pre-activation, BN backward, gradient of
    the residual input) -> y2_conv_wgrad_ex -> data gradient (stride 1: forward kernel on rotated weights; stride 2:
    transposed mode of the general kernel).  'pool' op: y2_maxpool_fwd / y2_maxpool_bwd.  'dw' op (MobileNet's depthwise convolutions): y2_dwconv_fwd
    (raw, BN statistics) -> y2_bn_finalize -> y2_bn_act_fwd_ex; backward y2_bn_act_bwd_ex -> y2_dwconv_wgrad -> y2_dwconv_dgrad.
    DenseNet's blocks are 'pre' / 'grow' ops (_build_densenet, _densenet_bwd) between the stem's ops and the image."""

    @staticmethod
    def forward(ctx, net, x, frozen, *params):
        _hip.require_gpu(x)
        build = _builder(net)
        ctx.need_dx = x.requires_grad
        x = _hip.f32c(x.detach())
        if x.shape[2] % 32 or x.shape[3] % 32:
            raise ValueError('input size must be a multiple of 32 (got %dx%d)' % (x.shape[2], x.shape[3]))
        scope = getattr(ctx, 'scope', None)
        rec = _Recorder(net, x, frozen, scope)
        out = build(rec, net)
        ctx.frozen, ctx.prepared = frozen, rec.prepared
        ctx.prepared_key = net.__dict__['_train_cache'][0] if scope is None else None
        ctx.x4, ctx.cin0, ctx.dense = rec.x4, rec.cin0, rec.dense
        ctx.net, ctx.ops, ctx.B = net, rec.ops, rec.B
        ctx.param_ids = [id(p) for p in params]
        return out

    @staticmethod
    def backward(ctx, dout):
        L = _hip.lib()
        st = _hip.stream()
        net, ops, B = ctx.net, ctx.ops, ctx.B
        dev = dout.device
        prepared = getattr(ctx, 'prepared', None) or {}
        if prepared and getattr(ctx, 'prepared_key', None) is not None and net.__dict__.get('_train_cache', (None,))[0] != ctx.prepared_key:
            raise RuntimeError('model.train_oplist: a convolution weight was modified between this forward and its backward; the per-model GEMM operand '
                               'buffers this graph was recorded against hold other weights now')
        sink = GradSink(net, dev)
        ready, dest = sink.ready, sink.dest
        if getattr(ctx, 'dense', None) is not None:
            dout = _densenet_bwd(ctx, dout, sink)          # leaves the stem ops (conv0 + norm0 + ReLU, max-pool) to the walk below
        convs = [op for op in ops if op.kind in ('conv', 'dw')]
        # everything that must start from zero, filled by ONE launch: the fp64 sums of every BatchNorm backward, the accumulation targets of the
        # direct (split, atomically added) weight gradients, the zero-padded gradient of the 425-wide head
        sums_arena = torch.empty(2 * sum(op.cout for op in convs), dtype=torch.float64, device=dev)
        zero = [sums_arena]
        plan = {}
        off = 0
        for op in convs:
            cout, cin, k = op.cout, op.ldx, op.k
            cop = (cout + 3) // 4 * 4
            e = plan[id(op)] = dict(sums=sums_arena[off:off + 2 * cout], off=off)
            off += 2 * cout
            e['dz'] = None
            if op.kind == 'dw':
                e['wino'] = False
                continue
            if cop != cout:
                e['dz'] = _new(dev, B, op.ho, op.wo, cop)
                zero.append(e['dz'])
            wino = k == 3 and op.stride == 1 and op.pad == 1
            e['wino'] = wino
            if not wino:
                # [cop][k*k][cin]: for a 1x1 convolution that IS the state_dict layout - the kernel writes the gradient tensor itself
                direct_out = k == 1 and cop == cout and cin == op.cin
                e['dwp'] = dest(op.conv.weight).view(-1) if direct_out else _new(dev, cop * k * k * cin)
                e['final'] = direct_out
                zero.append(e['dwp'])
        _hip.multi([(_hip.MULTI_ZERO, t, None) for t in zero], st)
        affine = []
        G = {id(ops[-1].y): [_hip.f32c(dout)]}      # gradient sources per activation tensor
        for op in reversed(ops):
            srcs = G.pop(id(op.y), [])
            assert 1 <= len(srcs) <= 2, len(srcs)
            if op.kind == 'pool':
                dx = _new(dev, B, op.h, op.w, op.cout)
                pk, ps, pp, pe = op.pool
                _hip.check(L.y2_maxpool_bwd(_hip.ptr(op.x), _hip.ptr(srcs[0]), _hip.ptr(srcs[1]) if len(srcs) > 1 else None, _hip.ptr(dx),
                                            B, op.h, op.w, op.cout, op.cout, op.cout, op.cout, pk, ps, pp, pe, st), 'y2_maxpool_bwd')
                G.setdefault(id(op.x), []).append(dx)
                continue
            cout, cin, k, ho, wo = op.cout, op.ldx, op.k, op.ho, op.wo
            cop = (cout + 3) // 4 * 4
            e = plan[id(op)]
            sums, dz = e['sums'], (e['dz'] if e['dz'] is not None else _new(dev, B, ho, wo, cop))
            dres = _new(dev, B, ho, wo, cout) if op.residual is not None else None
            has_bn = op.bn is not None
            _hip.check(L.y2_bn_act_bwd_ex(_hip.ptr(op.z), _hip.ptr(op.scale), _hip.ptr(op.shift), _hip.ptr(op.mean), _hip.ptr(op.invstd),
                                          _hip.ptr(op.bn.weight.detach()) if has_bn else None, op.slope,
                                          _hip.ptr(srcs[0]), cout, 0, 0, None, 0, 0,
                                          _hip.ptr(srcs[1]) if len(srcs) > 1 else None, cout,
                                          _hip.ptr(op.residual), cout if op.residual is not None else 0, _hip.ptr(dres), cout,
                                          _hip.ptr(sums), _hip.ptr(dz), cop, B, ho, wo, cout, cout, (2 if ctx.frozen else 1) if has_bn else 0, st), 'y2_bn_act_bwd_ex')
            if op.residual is not None:
                G.setdefault(id(op.residual), []).append(dres)
            # parameter gradients of the affine part = the fp64 sums of pass 1: converted for ALL layers by one launch after the loop
            if has_bn:
                affine.append((op.bn.bias, e['off'], cout))
                affine.append((op.bn.weight, e['off'] + cout, cout))
            elif op.conv.bias is not None:
                affine.append((op.conv.bias, e['off'], cout))
            if op.kind == 'dw':
                # ---- depthwise: weight gradient straight into the state_dict layout (two fixed-order stages), data gradient in gather form
                C = op.cout
                dw = dest(op.conv.weight)
                nws = L.y2_dwconv_wgrad_workspace_bytes(B, op.h, op.w, C, op.stride)
                ws = _new(dev, max(nws // 4, 4))
                _hip.check(L.y2_dwconv_wgrad(_hip.ptr(op.x), _hip.ptr(dz), _hip.ptr(dw), _hip.ptr(ws), ws.numel() * 4, B, op.h, op.w, C, C, C, op.stride, st),
                           'y2_dwconv_wgrad')
                ready(op.conv.weight, dw)
                op.z = None
                dx = _new(dev, B, op.h, op.w, C)
                _hip.check(L.y2_dwconv_dgrad(_hip.ptr(dz), _hip.ptr(op.filt), _hip.ptr(dx), B, op.h, op.w, C, C, C, op.stride, st), 'y2_dwconv_dgrad')
                G.setdefault(id(op.x), []).append(dx)
                continue
            # ---- weight gradient
            if e['wino']:
                dwp = _hip.conv_wgrad(op.x, dz, B, op.h, op.w, cin, cin, cop, cop, k)     # direct or Winograd, by measurement
            else:
                dwp = e['dwp']
                _hip.check(L.y2_conv_wgrad_ex(_hip.ptr(op.x), _hip.ptr(dz), _hip.ptr(dwp), B, op.h, op.w, cin, cin, cop, cop, k, op.stride, op.pad, st), 'y2_conv_wgrad_ex')
            if not e['wino'] and e['final']:
                ready(op.conv.weight, dwp.view(cout, cin, 1, 1))
            else:
                dw = dest(op.conv.weight) if (cop == cout and cin == op.cin) else _new(dev, cop, cin, k, k)
                _hip.check(L.y2_unpack_weight_grad(_hip.ptr(dwp), _hip.ptr(dw), cop, cin, k, st), 'y2_unpack_weight_grad')
                ready(op.conv.weight, dw if (cop == cout and cin == op.cin) else dw[:cout, :op.cin].contiguous())
            op.z = None
            if op.first and not ctx.need_dx:
                continue
            # ---- data gradient (of the first layer only when the image's gradient is wanted: its result is the 4-channel NHWC image gradient)
            ready_ops = prepared.get(op.conv)
            if ready_ops is not None and cop == cout and op.cin == cin:
                wd = ready_ops['wd']          # rotated / in-out-swapped operand prepared with the forward's (same parameter version)
            else:
                wsrc = _hip.f32c(op.conv.weight.detach())
                if cop != cout or wsrc.shape[1] != cin:          # zero rows for padded output channels, zero columns for the stem's padded input channels
                    wpad = torch.zeros(cop, cin, k, k, dtype=torch.float32, device=dev)
                    wpad[:cout, :wsrc.shape[1]] = wsrc
                    wsrc = wpad
                wd = _new(dev, wsrc.numel())
                _hip.check(L.y2_pack_weight(_hip.ptr(wsrc), _hip.ptr(wd), cop, cin, k, 1, st), 'y2_pack_weight')
            dx = _new(dev, B, op.h, op.w, cin)
            if op.stride == 1:
                gen_conv(L, st, dz, wd, dx, B, ho, wo, cop, cop, cin, k, 1, k - 1 - op.pad)
            else:
                gen_conv(L, st, dz, wd, dx, B, ho, wo, cop, cop, cin, k, op.stride, op.pad, transposed=True, out_hw=(op.h, op.w))
            G.setdefault(id(op.x), []).append(dx)
        sink.hand_affine(sums_arena, affine, st)
        dx_img = None
        if ctx.need_dx:
            gx = G.pop(id(ctx.x4), None)
            if gx:
                dx_img = gx[0][..., :ctx.cin0].permute(0, 3, 1, 2).contiguous()
        out = [None, dx_img, None]
        for pid in ctx.param_ids:
            out.append(sink.grads.get(pid))
        ctx.ops = None
        ctx.prepared = None
        return tuple(out)

