"""Parts shared by the inference side of the backbone classes (model/yolo2.py Darknet and Tiny, model/resnet.py, model/mobilenet.py,
model/densenet.py): the twin of model/_train_parts.py.  A class keeps the walk over its own architecture - which layer feeds which buffer,
the layout of its `prep`, its step list; what a walk is made of lives here: the runtime attributes and forward() dispatch (InferMixin), the
entry checks of forward_nhwc (enter), BatchNorm folding and weight packing (fold_bn, pack_weight, affine), the y2_conv_params filler
(conv_params) and what a plan owns while it is built (PlanBuilder: buffers, byte and flop counts, the shared scratch)."""
import ctypes

import torch
from torch.nn import Conv2d

import _hip

BN_EPS = 1e-5
LEAKY = 0.1


def pad4(c):
    return (c + 3) // 4 * 4


class InferMixin(object):
    """What every backbone class carries besides its architecture.  A class provides forward_nhwc(x) and, where its training graph is not the
    op-list one, _train_forward."""

    def _init_runtime(self):
        self._cache = None  # (version key, prep): packed weights / folded BN for eval, keyed on parameter versions
        self._plans = _hip.PlanCache()  # execution plans (intermediate buffers + y2_conv_params) per input shape, LRU
        self.grad_ready_hook = None  # set by train.DataParallelRCCL: called as hook(param, grad) inside backward, layer by layer
        self.profile = None  # tools: list receiving (kernel, flops, start_event, end_event) per forward_nhwc

    def _versions(self):
        """Cache key of everything derived from the parameters and buffers: (address, torch version counter) per tensor.  The
        raw-pointer writers (utils.optim, y2_bn_finalize) advance the counters of what they wrote through _hip.wrote, so the key is
        per tensor and per model: training another model does not touch it."""
        return tuple((p.data_ptr(), p._version) for p in list(self.parameters()) + list(self.buffers()))

    def _cached_prep(self, ver):
        """The prep stored under version key `ver` (self._cache = (ver, prep)), None when the parameters moved on."""
        return self._cache[1] if self._cache is not None and self._cache[0] == ver else None

    @property
    def _plan_cache(self):
        """(tools / bench) the most recently used plan as (key, plan), None before the first forward."""
        plan = self._plans.latest()
        return None if plan is None else (plan['key'], plan)

    @_plan_cache.setter
    def _plan_cache(self, value):
        assert value is None
        self._plans.clear()

    def _plan_key(self, dev, B, cin0, H, W, *extra):
        """Key of an execution plan.  The widths are part of it: a plan's buffers, leading dimensions and algorithm choices are sized for the
        conv weights it was built for (channel surgery, a replaced head re-plan) - what a new parameter VERSION of the same shapes does to a
        plan is the class's choice (PlanBuilder.rebind, or a new plan)."""
        widths = tuple(tuple(m.weight.shape) for m in self.modules() if isinstance(m, Conv2d))
        return (str(dev), B, cin0, H, W, _hip.tune_epoch(), _hip.WINOGRAD, _hip.FORCE_ALGO, *extra, widths)

    def _train_forward(self, x, frozen):
        from model import train_oplist  # training graph (autograd.Function over the HIP kernels)
        return train_oplist.forward(self, x, frozen=frozen)

    def forward(self, x):
        # BN semantics follow self.training alone, like nn.BatchNorm2d (model/yolo2.py:58): train() mode normalises with batch
        # statistics and updates the running ones whether or not autograd is recording (under no_grad the graph is simply
        # not taped); eval() mode runs the folded-BN inference chain - and stays differentiable like any nn.Module when autograd is
        # recording (frozen-BatchNorm fine-tuning; the reference back-propagates through `dnn` in eval mode,
        # receptive_field_analyzer.py:67,87): the backward then re-runs the layers with frozen statistics.
        if self.training:
            return self._train_forward(x, False)
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return self._train_forward(x, True)
        with torch.no_grad():
            out = self.forward_nhwc(x)
        # NCHW view of the NHWC head image: same values/shape as the reference's output; model.Inference's
        # permute(0,2,3,1).contiguous() (model/__init__.py:122) is then free.
        return out.permute(0, 3, 1, 2)


def enter(x):
    """The checks at the top of every forward_nhwc: x [B,Cin,H,W] NCHW on the GPU -> (contiguous fp32 x, B, Cin, H, W, device)."""
    _hip.require_gpu(x)
    x = _hip.f32c(x)
    B, cin0, H, W = x.shape
    if H % 32 or W % 32:
        raise ValueError('input size must be a multiple of 32 (got %dx%d)' % (H, W))
    return x, B, cin0, H, W, x.device


def profile_begin(net):
    """Start event of one forward_nhwc when a tool listens on net.profile, else None."""
    if net.profile is None:
        return None
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record()
    return e0


def profile_end(net, e0, flops):
    if e0 is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        net.profile.append(('conv_fwd', flops, e0, e1))


def fold_bn(L, st, dev, bn, tensors=None, C=None):
    """(scale, shift) of an inference BatchNorm (y2_bn_fold).  tensors: (gamma, beta, running_mean, running_var) to fold instead of the
    module's own, over C channels."""
    gamma, beta, rm, rv = tensors if tensors is not None else (bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var)
    C = gamma.shape[0] if C is None else C
    scale, shift = torch.empty(C, dtype=torch.float32, device=dev), torch.empty(C, dtype=torch.float32, device=dev)
    _hip.check(L.y2_bn_fold(_hip.ptr(_hip.f32c(gamma)), _hip.ptr(_hip.f32c(beta)), _hip.ptr(_hip.f32c(rm)), _hip.ptr(_hip.f32c(rv)),
                            BN_EPS, _hip.ptr(scale), _hip.ptr(shift), C, st), 'y2_bn_fold')
    return scale, shift


def affine(L, st, dev, conv, bn):
    """Epilogue (scale, shift) of a convolution: its BatchNorm folded, or (None, bias-or-None)."""
    if bn is not None:
        return fold_bn(L, st, dev, bn)
    return None, (_hip.f32c(conv.bias.detach()) if conv.bias is not None else None)


def pack_weight(L, st, dev, weight, pad=True):
    """[Cout,Cin,k,k] (state_dict layout) -> (wp [Cout][tap][Cin] as y2_conv_fwd reads it, Cin as packed, Cout, k).  pad: Cin is zero-padded
    to a multiple of 4 (the 3-channel image, pruned widths: activations carry a pixel stride rounded up to 4 channels)."""
    _hip.require_gpu(weight)
    w = _hip.f32c(weight.detach())
    cout, cin, k, _ = w.shape
    if pad and cin % 4:
        wpad = torch.zeros(cout, pad4(cin), k, k, dtype=torch.float32, device=dev)
        wpad[:, :cin] = w
        w, cin = wpad, wpad.shape[1]
    wp = torch.empty(w.numel(), dtype=torch.float32, device=dev)
    _hip.check(L.y2_pack_weight(_hip.ptr(w), _hip.ptr(wp), cout, cin, k, 0, st), 'y2_pack_weight')
    return wp, cin, cout, k


def conv_params(x, w, scale, shift, B, H, W, cin, ldx, cout, k, slope, y=None, ldy=0, coff=0, y_pool=None, ldp=0, poff=0, out_mode=0,
                residual=None, ldr=0, stride=None, pad=None, real_cin=None):
    """One filled y2_conv_params and the layer's multiply-add count (over real_cin input channels where cin is a zero-padded count).
    stride / pad: left UNSET (0, 0: the stride-1 "same" convolution) unless given - both fields are part of _hip.autotune_conv's key, so
    Darknet, whose measured table was keyed without them, must not write 1 / pad + 1 for the same convolution."""
    p = _hip.ConvParams()
    p.x, p.w = x.data_ptr(), w.data_ptr()
    p.scale = scale.data_ptr() if scale is not None else None
    p.shift = shift.data_ptr() if shift is not None else None
    p.y = y.data_ptr() if y is not None else None
    p.y_pool = y_pool.data_ptr() if y_pool is not None else None
    p.B, p.H, p.W, p.Cin, p.ldx, p.Cout, p.ksize = B, H, W, cin, ldx, cout, k
    p.ldy, p.coff, p.ldp, p.poff, p.out_mode = ldy, coff, ldp, poff, out_mode
    p.slope, p.tile = slope, 0
    ho, wo = H, W
    if stride is not None:
        p.stride, p.pad_plus1 = stride, pad + 1
        ho, wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if residual is not None:
        p.residual, p.ldr = residual.data_ptr(), ldr
    return p, 2.0 * (cin if real_cin is None else real_cin) * cout * k * k * B * ho * wo


class PlanBuilder(object):
    """What a plan owns while a class's _plan walks its architecture: the intermediate buffers (`keep`), their bytes, the flop sum."""

    def __init__(self, dev, alloc=torch.empty):
        # alloc: torch.empty, or torch.zeros where the channel padding of an activation must stay zero (MobileNet, DenseNet)
        self.dev, self.alloc = dev, alloc
        self.nbytes, self.flops, self.keep = 0, 0.0, []

    def new(self, *shape):
        t = self.alloc(*shape, dtype=torch.float32, device=self.dev)
        self.nbytes += t.numel() * 4
        self.keep.append(t)
        return t

    def share_workspace(self, sized, private=False, unsized=()):
        """One scratch for every y2_conv_params of the plan, as large as the largest need among `sized`; `unsized` receive it too.
        Consecutive convolutions on one stream may share the per-device scratch (_hip.workspace); private: the plan's own, counted in
        its bytes (plans whose launches overlap on another stream)."""
        L = _hip.lib()
        need = max([L.y2_conv_fwd_workspace_bytes(ctypes.byref(p)) for p in sized] + [0])
        ws = None
        if need > 0:
            ws = self.new(int(need) // 4 + 4) if private else _hip.workspace(self.dev, need)
        for p in list(sized) + list(unsized):
            p.workspace, p.workspace_bytes = (ws.data_ptr(), ws.numel() * 4) if ws is not None else (None, 0)
        return ws

    @staticmethod
    def rebind(p, w, scale, shift):
        """Same shape, new parameter version: the buffers, algorithms and tiles of a plan stay, only the operand pointers of the packed /
        folded / transformed weights move."""
        p.w = w.data_ptr()
        p.scale = scale.data_ptr() if scale is not None else None
        p.shift = shift.data_ptr() if shift is not None else None


def refuse_pretrained(config_channels, module_name):
    """The reference's plugin constructors load torchvision model-zoo weights by URL under [model] pretrained=1."""
    try:
        pretrained = config_channels.config.getboolean('model', 'pretrained')
    except Exception:
        pretrained = False
    if pretrained:
        raise RuntimeError('%s: [model] pretrained=1 cannot be honoured (no torchvision model zoo / network here); set pretrained=0 and load a '
                           'checkpoint with load_state_dict (same keys as torchvision.%s)' % (module_name, module_name.replace('model.', 'models.')))
