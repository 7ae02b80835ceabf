"""GPU parity tests of train.hip's streaming kernels, one dispatch path at a time: BatchNorm finalise, BN + LeakyReLU (+ MaxPool / reorg /
residual) forward and backward, the general max-pool forward / backward, y2_colsum, y2_f64_to_f32 and y2_decode_bwd.

Ground rules of every test here: inputs are drawn in fp32 from a seeded generator and upcast to fp64 for the reference, so kernel and
reference see bit-identical inputs; the reference is torch-CPU fp64 autograd of the composed operators (never the kernel's formula restated);
every output buffer that has room around its channel window carries the -7.0 sentinel there, and so does every buffer a call must not touch."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import darknet as odark
from oracle import head as ohead

pytestmark = pytest.mark.gpu
TOL = 2e-5                      # forward activations (the project's bound, tests/test_gpu_train.py)
TOL_DZ = 5e-5                   # dz / dres (the bound test_bn_act_forward_backward uses)
EPS32 = float(torch.finfo(torch.float32).eps)
BN_EPS = 1e-5
SENT = -7.0
NUM_CU = 256                    # Y2_NUM_CU (csrc/common.h)
EINVAL = -1


def dev():
    return torch.device('cuda:0')


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2)


def rel(got, ref):
    ref = ref.double()
    rms = ref.pow(2).mean().sqrt().item()
    return (got.double().cpu() - ref).abs().max().item() / max(rms, 1e-30)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn32(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def window(t, ld, off=0):
    """Device buffer [..., ld] full of the sentinel with the channels-last tensor t in channels off .. off + C."""
    C = t.shape[-1]
    assert ld >= off + C
    buf = torch.full(tuple(t.shape[:-1]) + (ld,), SENT, dtype=t.dtype)
    buf[..., off:off + C] = t
    return buf.to(dev())


def blank(prefix, ld, dtype=torch.float32):
    return torch.full(tuple(prefix) + (ld,), SENT, dtype=dtype, device=dev())


def guards_intact(buf, off, C):
    return bool((buf[..., :off] == SENT).all()) and bool((buf[..., off + C:] == SENT).all())


def untouched(buf):
    return bool((buf == SENT).all())


def act_grid(total, Cg):
    """csrc/train.hip: act_grid - workgroups of 256 threads, 8 items per thread, capped at 8 per CU, total thread count a multiple of Cg."""
    unit = Cg // math.gcd(256, Cg)
    want = min(max((total + 256 * 8 - 1) // (256 * 8), 1), NUM_CU * 8)
    return (want + unit - 1) // unit * unit


def bwd_launch(B, H, W, C, pooled, vec, dz_kind):
    """What bn_act_bwd_impl launches in the default (atomic) mode: (grid, path, items per thread).  path: 'atomics' (grid <= 16),
    'atomics>16' (a larger grid that still may not park its partial sums in dz: dz NULL, strided or aliasing an input) or 'block1' / 'block4' /
    'block16' (per-workgroup partial rows parked in the dense dz, added by bn_bwd_block_reduce_kernel with 1 / 4 / 16 row slices)."""
    Cg = C // 4 if vec else C
    npix = B * (H // 2) * (W // 2) if pooled else B * H * W
    grid = act_grid(npix * Cg, Cg)
    assert (grid * 256) % Cg == 0
    pstep = grid * 256 // Cg
    items = (4 if pooled else 1) * ((npix + pstep - 1) // pstep)
    if grid <= 16:
        path = 'atomics'
    elif dz_kind != 'dense' or grid * 2 * C > B * H * W * C:
        path = 'atomics>16'
    else:
        path = 'block16' if grid >= 512 else ('block4' if grid >= 64 else 'block1')
    return grid, path, items


# ================================================================================================ 1. BN + activation forward
FWD_DEFAULT = dict(C=32, pool='none', ldz=0, coff=0, ldy=0, poff=0, ldp=0, out_mode=0, res='none', slope=0.1, affine=True, H=6, W=10)
FWD_CASES = {
    'c32-full': dict(),
    'c32-pool-only-window': dict(pool='pool', poff=4, ldp=8),
    'c32-pool+full-windows': dict(pool='both', ldz=4, coff=4, ldy=12, poff=8, ldp=8),
    'c24-full-ldz': dict(C=24, ldz=8),
    'c24-pool+full': dict(C=24, pool='both', coff=4, ldy=4),
    'c24-pool-only': dict(C=24, pool='pool'),
    'c6-full-window': dict(C=6, ldz=1, coff=3, ldy=5),
    'c6-pool+full-window': dict(C=6, pool='both', poff=1, ldp=3),
    'c6-pool-only': dict(C=6, pool='pool', ldz=2),
    'c32-reorg-affine': dict(out_mode=1, coff=4, ldy=12),
    'c6-reorg-affine': dict(C=6, out_mode=1, coff=1, ldy=2),
    'c32-residual': dict(res='window'),
    'c32-residual-off-by-one-float': dict(res='unaligned'),
    'c6-residual': dict(C=6, res='window'),
    'c24-residual-pool+full': dict(C=24, res='window', pool='both', ldp=4),
    'c32-identity': dict(affine=False),
    'c32-slope0-pool+full': dict(slope=0.0, pool='both'),
    'c6-slope0': dict(C=6, slope=0.0),
    'c32-slope1': dict(slope=1.0, res='window'),
    'c6-slope1-pool+full': dict(C=6, slope=1.0, pool='both'),
}


def _fwd_reference(cfg, g):
    B, H, W, C = 2, cfg['H'], cfg['W'], cfg['C']
    z = randn32(g, B, C, H, W)
    sign = torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)                       # a third of the channels scale negatively
    gamma = ((torch.rand(C, generator=g, dtype=torch.float32) + 0.5) * sign).double()
    beta = (randn32(g, C) * 0.3).double()
    rm = (randn32(g, C) * 0.3).double()
    rv = (torch.rand(C, generator=g, dtype=torch.float32) + 0.5).double()
    res = randn32(g, B, C, H, W) if cfg['res'] != 'none' else None
    u = F.batch_norm(z.double(), rm, rv, gamma, beta, False, 0.0, BN_EPS) if cfg['affine'] else z.double()
    if res is not None:
        u = u + res.double()
    y = F.leaky_relu(u, cfg['slope'])
    istd = 1.0 / torch.sqrt(rv + BN_EPS)
    scale, shift = (gamma * istd).float(), (beta - rm * gamma * istd).float()
    return z, res, scale, shift, y


def _fwd_call(L, cfg, zd, scale, shift, resd, ldr, y, yp, B, H, W, C, ldz, ldy, ldp):
    import _hip
    sc, sh = (_hip.ptr(scale), _hip.ptr(shift)) if cfg['affine'] else (None, None)
    if resd is None:
        return L.y2_bn_act_fwd(_hip.ptr(zd), sc, sh, cfg['slope'], _hip.ptr(y), _hip.ptr(yp), B, H, W, C, ldz, ldy, cfg['coff'], ldp, cfg['poff'], cfg['out_mode'], _hip.stream())
    return L.y2_bn_act_fwd_ex(_hip.ptr(zd), sc, sh, cfg['slope'], _hip.ptr(resd), ldr, _hip.ptr(y), _hip.ptr(yp), B, H, W, C, ldz, ldy, cfg['coff'], ldp, cfg['poff'],
                              cfg['out_mode'], _hip.stream())


@pytest.mark.parametrize('name', list(FWD_CASES))
def test_bn_act_forward_paths(name):
    """y2_bn_act_fwd / y2_bn_act_fwd_ex against fp64 F.batch_norm (eval form of the folded scale / shift) + residual + F.leaky_relu (+ F.max_pool2d /
    reorg): vector (C = 32, 24: Cg = 6, a grid that is a multiple of 3) and scalar (C = 6) channel counts, strided input, channel windows in y and
    y_pool, reorg output with negative scales, residual with a wider pixel stride, and a residual pointer one float off 16-byte alignment (the
    scalar path, silently)."""
    import _hip
    L = _hip.lib()
    d = dev()
    cfg = dict(FWD_DEFAULT, **FWD_CASES[name])
    B, H, W, C = 2, cfg['H'], cfg['W'], cfg['C']
    z, res, scale, shift, yref = _fwd_reference(cfg, gen(sum(map(ord, name))))
    reorg = cfg['out_mode'] == 1
    Cy = 4 * C if reorg else C
    ldz, ldy, ldp = C + cfg['ldz'], cfg['coff'] + Cy + cfg['ldy'], cfg['poff'] + C + cfg['ldp']
    zd = window(nhwc(z), ldz)
    resd, ldr = None, 0
    if cfg['res'] == 'window':
        ldr = C + 4
        resd = window(nhwc(res), ldr)
    elif cfg['res'] == 'unaligned':
        ldr = C + 4
        flat = torch.full((B * H * W * ldr + 1,), SENT, device=d)
        resd = flat[1:].view(B, H, W, ldr)
        resd[..., :C] = nhwc(res).to(d)
        assert resd.data_ptr() % 16 == 4
    want_y, want_p = cfg['pool'] != 'pool', cfg['pool'] != 'none'
    y = blank((B, H // 2, W // 2) if reorg else (B, H, W), ldy) if want_y else None
    yp = blank((B, H // 2, W // 2), ldp) if want_p else None
    _hip.check(_fwd_call(L, cfg, zd, scale.to(d), shift.to(d), resd, ldr, y, yp, B, H, W, C, ldz, ldy, ldp), 'fwd')
    if want_y:
        ref = odark.reorg(yref) if reorg else yref
        assert rel(nchw(y[..., cfg['coff']:cfg['coff'] + Cy]), ref) <= TOL
        assert guards_intact(y, cfg['coff'], Cy), 'y written outside its channel window'
    if want_p:
        assert rel(nchw(yp[..., cfg['poff']:cfg['poff'] + C]), F.max_pool2d(yref, 2)) <= TOL
        assert guards_intact(yp, cfg['poff'], C), 'y_pool written outside its channel window'
    assert guards_intact(zd, 0, C) and (resd is None or guards_intact(resd, 0, C))
    if cfg['C'] == 24:
        assert act_grid(B * (H // 2 if cfg['pool'] != 'none' else H) * (W // 2 if cfg['pool'] != 'none' else W) * 6, 6) % 3 == 0


@pytest.mark.parametrize('H,W,pool,out_mode', [(7, 10, True, 0), (6, 9, True, 0), (7, 10, False, 1), (6, 9, False, 1)])
def test_bn_act_forward_rejects_odd_sizes(H, W, pool, out_mode):
    """An odd H or W with a pool output or the reorg output mode: Y2_EINVAL, and nothing is written."""
    import _hip
    L = _hip.lib()
    B, C = 2, 8
    zd = randn32(gen(3), B, H, W, C).to(dev())
    y = blank((B, H, W), 4 * C + 4)
    yp = blank((B, H, W), C + 4) if pool else None
    assert L.y2_bn_act_fwd(_hip.ptr(zd), None, None, 0.1, _hip.ptr(y), _hip.ptr(yp), B, H, W, C, C, 4 * C + 4, 0, C + 4, 0, out_mode, _hip.stream()) == EINVAL
    assert L.y2_bn_act_fwd_ex(_hip.ptr(zd), None, None, 0.1, _hip.ptr(zd), C, _hip.ptr(y), _hip.ptr(yp), B, H, W, C, C, 4 * C + 4, 0, C + 4, 0, out_mode, _hip.stream()) == EINVAL
    torch.cuda.synchronize()
    assert untouched(y) and (yp is None or untouched(yp))


# ================================================================================================ 2. BN + activation backward
# name: (has_bn, gradient sources, residual + dres, dz kind, strides / offsets added to the dense ones)
BWD_DEFAULT = dict(res=False, dz='dense', ldz=0, ldf=0, foff=0, ldp=0, poff=0, ld2=0, ldr=0, lddr=0)
BWD_CFGS = {
    'bn1-full': dict(has_bn=1, src='full'),
    'bn1-pool': dict(has_bn=1, src='pool'),
    'bn1-pool+full': dict(has_bn=1, src='both', ldz=4, poff=4, ldp=4),
    'bn1-full+full2': dict(has_bn=1, src='full2', foff=4, ldf=4, ld2=4),
    'bn1-reorg-window': dict(has_bn=1, src='reorg', foff=8, ldf=12),
    'bn2-full': dict(has_bn=2, src='full'),
    'bn2-pool+full': dict(has_bn=2, src='both'),
    'bn0-full': dict(has_bn=0, src='full'),
    'bn0-pool': dict(has_bn=0, src='pool'),
    'bn1-full-residual': dict(has_bn=1, src='full', res=True, ldr=4, lddr=8),
    'bn1-pool+full-residual': dict(has_bn=1, src='both', res=True, ldr=4, lddr=8),
    'bn2-full+full2-residual': dict(has_bn=2, src='full2', res=True, ldr=8, lddr=4),
    'bn1-full-strided-dz': dict(has_bn=1, src='full', dz='strided'),
    'bn1-full-in-place': dict(has_bn=1, src='full', dz='inplace'),
    'bn1-full-sums-only': dict(has_bn=1, src='full', dz='null'),
    'bn1-pool-sums-only': dict(has_bn=1, src='pool', dz='null', poff=4, ldp=4),
}
POOLED = ('pool', 'both')

# geometry: (B, H, W, C), vector path?, launch path with a dense dz [full-resolution grid, pooled grid], K = items per thread + 256 LDS atomics
# [full-resolution, pooled].  The paths and K are asserted against act_grid's arithmetic, so a change of act_grid cannot move a case off its path
# unnoticed.
GEOMS = {
    'atomics': ((3, 8, 12, 32), True, ('atomics', 'atomics'), (261, 268)),
    'block1': ((2, 26, 26, 128), True, ('block1', 'atomics'), (264, 288)),
    'block4': ((4, 32, 32, 128), True, ('block4', 'atomics'), (264, 288)),
    'block16': ((8, 64, 64, 128), True, ('block16', 'block4'), (264, 288)),
    'capped': ((20, 64, 64, 256), True, ('block16', None), (266, None)),
    'scalar': ((4, 40, 40, 6), False, ('block1', 'atomics'), (264, 284)),
    'cg6': ((4, 40, 40, 24), True, ('block1', 'atomics'), (264, 284)),
}
SMALL = 1 << 20                 # references of at most this many elements are kept for the other tests that use them


def _bwd_reference_uncached(geom, cfgname):
    B, H, W, C = GEOMS[geom][0]
    cfg = dict(BWD_DEFAULT, **BWD_CFGS[cfgname])
    has_bn, src, slope = cfg['has_bn'], cfg['src'], 0.1
    pooled = src in POOLED
    g = gen(1000 * list(GEOMS).index(geom) + list(BWD_CFGS).index(cfgname))
    z = randn32(g, B, C, H, W)
    res = randn32(g, B, C, H, W) if cfg['res'] else None
    if pooled:          # exact ties inside the 2x2 windows: the first maximum in scan order takes the pooled gradient
        z = (z * 2).round() / 2
        if res is not None:         # one residual value per window and channel: ties stay exact, two candidates never differ by rounding only
            res = res[:, :, ::2, ::2].repeat_interleave(2, 2).repeat_interleave(2, 3).contiguous()
    if has_bn:
        sign = torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)                    # negative-scale channels: the arg-max follows the smallest z
        gamma = ((torch.rand(C, generator=g, dtype=torch.float32) + 0.5) * sign).double()
        beta = (randn32(g, C) * 0.3).double()
    else:
        gamma, beta = torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    rm = (randn32(g, C) * 0.3).double()                                            # has_bn = 2: running statistics, not the batch's (0, 1)
    rv = (torch.rand(C, generator=g, dtype=torch.float32) + 0.5).double()

    def bn(zz, ga, be):
        if has_bn == 1:
            return F.batch_norm(zz, None, None, ga, be, True, 0.0, BN_EPS)
        if has_bn == 2:
            return F.batch_norm(zz, rm, rv, ga, be, False, 0.0, BN_EPS)
        return zz * ga.view(1, -1, 1, 1) + be.view(1, -1, 1, 1)

    def pre_of(zz):
        u = bn(zz.double(), gamma, beta)
        return u + res.double() if res is not None else u

    # LeakyReLU's derivative jumps at 0: an fp32 pre-activation within rounding of 0 may take the other side than the fp64 one.  Inputs whose
    # pre-activation is that close to 0 are moved by one 0.5 step (which keeps the tie grid), so the comparison is well-conditioned.
    with torch.no_grad():
        for _ in range(8):          # (a moved input shifts the batch mean a little: repeat until nothing is close)
            pre = pre_of(z)
            if pre.abs().min().item() >= 1e-3:
                break
            z = torch.where(pre.abs() < 1e-3, z + 0.5, z)
        assert pre.abs().min().item() > 1e-4, 'test input: a pre-activation sits on the LeakyReLU kink'
        if pooled:      # ... and so are windows whose two largest activations differ by rounding only
            v = F.leaky_relu(pre, slope)
            v = v.view(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
            gap = v.max(-1, keepdim=True).values - v
            assert gap[gap > 0].min().item() > 1e-4, 'test input: a near-tie inside a pooling window'
    dy = randn32(g, B, C, H, W) if src in ('full', 'both', 'full2') else None
    dy2 = randn32(g, B, C, H, W) if src == 'full2' else None
    dcat = randn32(g, B, 4 * C, H // 2, W // 2) if src == 'reorg' else None
    dyp = randn32(g, B, C, H // 2, W // 2) if pooled else None

    z64 = z.double().requires_grad_(True)
    ga, be = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    r64 = res.double().requires_grad_(True) if res is not None else None
    u = bn(z64, ga, be)
    u.retain_grad()
    y = F.leaky_relu(u + r64 if r64 is not None else u, slope)
    loss = 0.0
    if dy is not None:
        loss = loss + (y * dy.double()).sum()
    if dy2 is not None:
        loss = loss + (y * dy2.double()).sum()
    if dcat is not None:
        loss = loss + (odark.reorg(y) * dcat.double()).sum()
    if dyp is not None:
        loss = loss + (F.max_pool2d(y, 2) * dyp.double()).sum()
    loss.backward()
    with torch.no_grad():
        if has_bn == 1:
            _, mean, invstd = torch.native_batch_norm(z.double(), gamma, beta, None, None, True, 0.0, BN_EPS)
        elif has_bn == 2:
            mean, invstd = rm, 1.0 / torch.sqrt(rv + BN_EPS)
        else:
            mean, invstd = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
        zhat = (z.double() - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)
        gu = u.grad
        abs1, abs2 = gu.abs().sum((0, 2, 3)), (gu * zhat).abs().sum((0, 2, 3))     # only the SIZE of the summation bound comes from these
    ref = dict(z=z, res=res, dy=dy, dy2=dy2, dcat=dcat, dyp=dyp, gamma=gamma.float(), mean=mean.float(), invstd=invstd.float(),
               scale=(gamma * invstd).float(), shift=(beta - mean * gamma * invstd).float(), slope=slope,
               dz=z64.grad, dbeta=be.grad, dgamma=ga.grad, dres=r64.grad if r64 is not None else None, abs1=abs1, abs2=abs2)
    return ref


@functools.lru_cache(maxsize=None)
def _bwd_reference_small(geom, cfgname):
    return _bwd_reference_uncached(geom, cfgname)


def bwd_reference(geom, cfgname):
    """The fp64 autograd reference of one (geometry, configuration): computed once, shared (and left unchanged) by the tests that use it."""
    B, H, W, C = GEOMS[geom][0]
    return _bwd_reference_small(geom, cfgname) if B * H * W * C <= SMALL else _bwd_reference_uncached(geom, cfgname)


def run_bwd(geom, cfgname, ref):
    """One y2_bn_act_bwd(_ex) call on fresh buffers -> (sums [2C] fp64 on the CPU, dz window or None, dres window or None, K); asserts the launch path,
    the return code and every guard cell."""
    import _hip
    L = _hip.lib()
    d = dev()
    (B, H, W, C), vec, paths, Ks = GEOMS[geom]
    cfg = dict(BWD_DEFAULT, **BWD_CFGS[cfgname])
    has_bn, src, dzk = cfg['has_bn'], cfg['src'], cfg['dz']
    pooled = src in POOLED
    ldz, ldp, ld2, ldr, lddr = C + cfg['ldz'], cfg['poff'] + C + cfg['ldp'], C + cfg['ld2'], C + cfg['ldr'], C + cfg['lddr']
    Cf = 4 * C if src == 'reorg' else C
    ldf = cfg['foff'] + Cf + cfg['ldf']
    ldd = C + 4 if dzk == 'strided' else C
    # ---- the branch of bn_act_bwd_impl this case is meant to take
    is_vec = C % 4 == 0 and all(v % 4 == 0 for v in (ldz, ldp, ld2, ldr, lddr, ldf, ldd, cfg['foff'], cfg['poff']))
    assert is_vec == vec
    grid, path, items = bwd_launch(B, H, W, C, pooled, vec, 'dense')
    assert path == paths[pooled], (grid, path)
    K = items + 256
    assert K == Ks[pooled], K
    if dzk != 'dense':
        path = bwd_launch(B, H, W, C, pooled, vec, dzk)[1]
        assert path == ('atomics>16' if grid > 16 else 'atomics')
    if geom == 'capped':
        assert (B * H * W * (C // 4) + 2047) // 2048 > NUM_CU * 8 and grid == NUM_CU * 8 and items > 8
    # ---- buffers
    zd = window(nhwc(ref['z']), ldz)
    full = ref['dcat'] if src == 'reorg' else ref['dy']
    dyf = window(nhwc(full), ldf, cfg['foff']) if full is not None else None
    dypd = window(nhwc(ref['dyp']), ldp, cfg['poff']) if pooled else None
    dy2d = window(nhwc(ref['dy2']), ld2) if ref['dy2'] is not None else None
    resd = window(nhwc(ref['res']), ldr) if cfg['res'] else None
    dres = blank((B, H, W), lddr) if (cfg['res'] and dzk != 'null') else None
    if dzk == 'inplace':
        assert ldf == C and cfg['foff'] == 0
        dz = dyf
    elif dzk == 'null':
        dz = None
    else:
        dz = blank((B, H, W), ldd)
    sums = torch.full((2 * C + 4,), SENT, dtype=torch.float64, device=d)
    sums[:2 * C] = 0.0
    held = {k: ref[k].to(d) for k in ('mean', 'invstd', 'gamma', 'scale', 'shift')}          # alive until the synchronize below
    bnp = [_hip.ptr(held[k]) if has_bn else None for k in ('mean', 'invstd', 'gamma')]
    sc, sh = (_hip.ptr(held['scale']), _hip.ptr(held['shift'])) if has_bn else (None, None)
    inputs = [t for t in (zd, dypd, dy2d, resd) + ((dyf,) if dzk != 'inplace' else ()) if t is not None]
    before = [t.clone() for t in inputs]
    fmode = 1 if src == 'reorg' else 0
    if dy2d is None and resd is None:
        rc = L.y2_bn_act_bwd(_hip.ptr(zd), sc, sh, *bnp, ref['slope'], _hip.ptr(dyf), ldf, cfg['foff'], fmode, _hip.ptr(dypd), ldp, cfg['poff'],
                             _hip.ptr(sums), _hip.ptr(dz), ldd, B, H, W, C, ldz, has_bn, _hip.stream())
    else:
        rc = L.y2_bn_act_bwd_ex(_hip.ptr(zd), sc, sh, *bnp, ref['slope'], _hip.ptr(dyf), ldf, cfg['foff'], fmode, _hip.ptr(dypd), ldp, cfg['poff'],
                                _hip.ptr(dy2d), ld2, _hip.ptr(resd), ldr, _hip.ptr(dres), lddr,
                                _hip.ptr(sums), _hip.ptr(dz), ldd, B, H, W, C, ldz, has_bn, _hip.stream())
    _hip.check(rc, 'bn_act_bwd')
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(inputs, before)), 'an input buffer was written'
    assert bool((sums[2 * C:] == SENT).all()), 'sums written past 2C'
    if dz is not None:
        assert guards_intact(dz, 0, C), 'dz written outside its channels'
    if dres is not None:
        assert guards_intact(dres, 0, C), 'dres written outside its channels'
    return sums[:2 * C].cpu(), (dz[..., :C].clone() if dz is not None else None), (dres[..., :C].clone() if dres is not None else None), K


def check_bwd(ref, sums, dz, dres, K, C):
    e1, e2 = (sums[:C] - ref['dbeta']).abs(), (sums[C:] - ref['dgamma']).abs()
    b1, b2 = K * EPS32 * ref['abs1'], K * EPS32 * ref['abs2']
    print('sums: worst |err| / bound = %.3g (sum g), %.3g (sum g*zhat), K = %d' % ((e1 / b1).max().item(), (e2 / b2).max().item(), K))
    if dz is not None:
        print('dz: %.3g x rms' % rel(nchw(dz), ref['dz']))
    if dres is not None:
        print('dres: %.3g x rms' % rel(nchw(dres), ref['dres']))
    assert bool((e1 <= b1).all()), 'sum g (d beta) outside K * eps32 * sum |g|: worst %.3g x the bound' % (e1 / b1).max().item()
    assert bool((e2 <= b2).all()), 'sum g*zhat (d gamma) outside K * eps32 * sum |g*zhat|: worst %.3g x the bound' % (e2 / b2).max().item()
    if dz is not None:
        assert rel(nchw(dz), ref['dz']) <= TOL_DZ
    if dres is not None:
        assert rel(nchw(dres), ref['dres']) <= TOL_DZ


@pytest.mark.parametrize('geom', ['atomics', 'block1'])
@pytest.mark.parametrize('cfgname', list(BWD_CFGS))
def test_bn_act_backward_configurations(cfgname, geom):
    """Every configuration of y2_bn_act_bwd / y2_bn_act_bwd_ex (has_bn 1 / 2 / 0; gradient from dy_full, dy_pool, both, dy_full + dy_full2, or the
    reorg gather with a channel window; residual mask with dres; strided, in-place and absent dz) against fp64 autograd of F.batch_norm + residual +
    F.leaky_relu (+ F.max_pool2d / reorg), on a 2-workgroup launch and on the smallest one that parks per-workgroup partial sums in dz.
    dz, dres: rel() <= 5e-5.  sums: |got - ref| <= K * eps32 * sum |summand|, K = items per thread + 256 (GEOMS)."""
    C = GEOMS[geom][0][3]
    ref = bwd_reference(geom, cfgname)
    sums, dz, dres, K = run_bwd(geom, cfgname, ref)
    check_bwd(ref, sums, dz, dres, K, C)


@pytest.mark.parametrize('geom,cfgname', [(gm, c) for gm in ('block4', 'block16', 'scalar', 'cg6') for c in ('bn1-full', 'bn1-pool+full')] + [('capped', 'bn1-full')])
def test_bn_act_backward_geometries(geom, cfgname):
    """The launch geometries of bn_act_bwd_impl beyond the first two: 4 and 16 row slices of bn_bwd_block_reduce_kernel, the capped grid whose
    threads walk more than 8 pixels, the scalar path on more than 16 workgroups and a channel-group count that is no power of two.
    dz meets rel() <= 5e-5 at every one of them (measured on an MI355X: 1.1e-6 / 1.3e-6 / 1.3e-6 at the 4-slice, 16-slice and capped
    geometries, 1.5e-6 at worst with the pooled gradient), so no fp32-floor allowance is used; the sums stay below 4e-4 of their bound."""
    C = GEOMS[geom][0][3]
    ref = bwd_reference(geom, cfgname)
    sums, dz, dres, K = run_bwd(geom, cfgname, ref)
    check_bwd(ref, sums, dz, dres, K, C)


@pytest.mark.parametrize('geom', ['block1', 'scalar'])
def test_bn_act_backward_deterministic_mode(geom):
    """Deterministic mode (per-thread partial rows added in a fixed tree): the same tolerances, and bit-identical sums and dz on a second call."""
    import _hip
    C = GEOMS[geom][0][3]
    ref = bwd_reference(geom, 'bn1-full')
    _hip.set_deterministic(True)
    try:
        a = run_bwd(geom, 'bn1-full', ref)
        b = run_bwd(geom, 'bn1-full', ref)
    finally:
        _hip.set_deterministic(False)
    check_bwd(ref, a[0], a[1], a[2], a[3], C)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ================================================================================================ 3. BN finalise
def _finalize_case(C, N, seed):
    g = gen(seed)
    x = randn32(g, N, C).double() * (torch.rand(C, generator=g, dtype=torch.float32).double() + 0.5) + randn32(g, C).double() * 0.5
    gamma = (torch.rand(C, generator=g, dtype=torch.float32) + 0.5) * torch.where(torch.arange(C) % 4 == 2, -1.0, 1.0)
    beta = randn32(g, C) * 0.3
    rm, rv = randn32(g, C) * 0.2, torch.rand(C, generator=g, dtype=torch.float32) + 0.5
    true = torch.cat([x.sum(0), (x * x).sum(0)])                                   # [2C]
    # the sums spread over ALL replicated copies: random weights of both signs that add up to 1 (parts that cancel)
    w = torch.randn(32, 2 * C, generator=g, dtype=torch.float64)
    w = w - w.mean(0, keepdim=True) + 1.0 / 32
    return x, gamma, beta, rm, rv, (w * true).reshape(-1)


@pytest.mark.parametrize('C', [6, 300])
def test_bn_finalize_all_copies_and_running_statistics(C):
    """y2_bn_finalize against fp64 batch norm in training mode on a tensor with exactly the given sums: the sums are spread over all 32 replicated
    copies, momentum is 0.1 and the incoming running statistics are not the defaults.  C = 300 takes two workgroups."""
    import _hip
    L = _hip.lib()
    d = dev()
    N, mom = 50, 0.1
    assert _hip.STATS_REPL == 32
    x, gamma, beta, rm, rv, stats = _finalize_case(C, N, 11 + C)
    rm64, rv64 = rm.double(), rv.double()
    out, mean, invstd = torch.native_batch_norm(x, gamma.double(), beta.double(), rm64, rv64, True, mom, BN_EPS)      # updates rm64 / rv64 (unbiased variance)
    outs = [blank((), C + 8) for _ in range(4)]                  # scale, shift, mean, invstd at floats 4 .. 4 + C
    p = [ctypes.c_void_p(o.data_ptr() + 16) for o in outs]
    rmd, rvd = window(rm, C + 4), window(rv, C + 4)
    steps = torch.tensor([41, 77], dtype=torch.int64, device=d)
    statd, gd, bd = stats.to(d), gamma.to(d), beta.to(d)
    _hip.check(L.y2_bn_finalize(_hip.ptr(statd), float(N), _hip.ptr(gd), _hip.ptr(bd), _hip.ptr(rmd), _hip.ptr(rvd), mom, BN_EPS, *p, C, _hip.ptr(steps), _hip.stream()), 'fin')
    scale, shift, mean_k, invstd_k = (o[4:4 + C].cpu().double() for o in outs)
    assert all(guards_intact(o, 4, C) for o in outs) and guards_intact(rmd, 0, C) and guards_intact(rvd, 0, C)
    assert steps.tolist() == [42, 77]
    np.testing.assert_allclose(mean_k.numpy(), mean.numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(invstd_k.numpy(), invstd.numpy(), rtol=1e-5)
    np.testing.assert_allclose(scale.numpy(), (gamma.double() * invstd).numpy(), rtol=1e-5)
    np.testing.assert_allclose(shift.numpy(), (beta.double() - mean * gamma.double() * invstd).numpy(), rtol=1e-5, atol=1e-6)
    assert rel(x * scale + shift, out) <= TOL                    # the folded pair reproduces the normalised tensor
    np.testing.assert_allclose(rmd[:C].cpu().numpy(), rm64.numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(rvd[:C].cpu().numpy(), rv64.numpy(), rtol=1e-5)
    assert torch.equal(statd.cpu(), stats) and torch.equal(gd.cpu(), gamma) and torch.equal(bd.cpu(), beta)
    # ---- no running statistics, no counter: the four outputs and nothing else
    outs2 = [blank((), C + 8) for _ in range(4)]
    p2 = [ctypes.c_void_p(o.data_ptr() + 16) for o in outs2]
    _hip.check(L.y2_bn_finalize(_hip.ptr(statd), float(N), _hip.ptr(gd), _hip.ptr(bd), None, None, mom, BN_EPS, *p2, C, None, _hip.stream()), 'fin')
    assert all(torch.equal(a, b) for a, b in zip(outs, outs2))
    assert steps.tolist() == [42, 77] and torch.equal(statd.cpu(), stats) and torch.equal(gd.cpu(), gamma) and torch.equal(bd.cpu(), beta)
    np.testing.assert_allclose(rmd[:C].cpu().numpy(), rm64.numpy(), rtol=1e-5, atol=1e-7)


def test_bn_finalize_single_sample_count():
    """count = 1 (one pixel per channel): the variance is 0 and stays unscaled (no n / (n - 1) = 1 / 0), nothing becomes NaN.  torch refuses to train
    batch norm on one value per channel, so the expectation is the eval form with mean = x, var = 0."""
    import _hip
    L = _hip.lib()
    d = dev()
    C, mom = 6, 0.1
    x, gamma, beta, rm, rv, stats = _finalize_case(C, 1, 5)
    outs = [torch.empty(C, device=d) for _ in range(4)]
    rmd, rvd = rm.to(d), rv.to(d)
    statd, gd, bd = stats.to(d), gamma.to(d), beta.to(d)
    _hip.check(L.y2_bn_finalize(_hip.ptr(statd), 1.0, _hip.ptr(gd), _hip.ptr(bd), _hip.ptr(rmd), _hip.ptr(rvd), mom, BN_EPS, *[_hip.ptr(o) for o in outs], C, None, _hip.stream()), 'fin')
    scale, shift, mean, invstd = (o.cpu().double() for o in outs)
    assert all(bool(torch.isfinite(t).all()) for t in (scale, shift, mean, invstd, rmd.cpu(), rvd.cpu()))
    probe = torch.stack([x[0], x[0] + 1.0])
    ref = F.batch_norm(probe, x[0].clone(), torch.zeros(C, dtype=torch.float64), gamma.double(), beta.double(), False, 0.0, BN_EPS)
    assert rel(probe * scale + shift, ref) <= TOL
    np.testing.assert_allclose(mean.numpy(), x[0].numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(rmd.cpu().numpy(), ((1 - mom) * rm.double() + mom * x[0]).numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(rvd.cpu().numpy(), ((1 - mom) * rv.double()).numpy(), rtol=1e-5, atol=1e-7)


# ================================================================================================ 4. max-pool forward / backward
@pytest.mark.parametrize('ties', [False, True])
@pytest.mark.parametrize('with_dy2', [False, True])
@pytest.mark.parametrize('C', [6, 8, 32])
@pytest.mark.parametrize('k,s,pad,pad_end', [(3, 2, 1, 1), (2, 1, 0, 1), (2, 2, 0, 0), (3, 1, 1, 1)])
def test_maxpool_forward_backward_general(k, s, pad, pad_end, C, with_dy2, ties):
    """y2_maxpool_fwd / y2_maxpool_bwd (scalar, 4-channel and - for (3, 2, 1) with C = 32 - LDS-tiled backward) against F.pad(-inf) + F.max_pool2d in
    fp64, odd H and W spanning two tiles of the tiled kernel each way, every pixel stride wider than C, with and without the second gradient,
    on continuous and on tie-heavy inputs.  Forward bit-equal; backward within rtol = atol = 1e-6."""
    import _hip
    L = _hip.lib()
    B, H, W = 2, 11, 37
    g = gen(100 * k + 10 * s + pad + C)
    x = randn32(g, B, C, H, W)
    if ties:
        x = (x * 2).round() / 2
    x64 = x.double().requires_grad_(True)
    y = F.max_pool2d(F.pad(x64, (pad, pad_end, pad, pad_end), value=float('-inf')), k, s, 0)
    Ho, Wo = y.shape[-2:]
    assert (Ho, Wo) == ((H + pad + pad_end - k) // s + 1, (W + pad + pad_end - k) // s + 1)
    dy = randn32(g, B, C, Ho, Wo)
    dy2 = randn32(g, B, C, Ho, Wo) if with_dy2 else None
    y.backward(dy.double() + dy2.double() if with_dy2 else dy.double())
    ldx, ldy, lddx = (C + 4, C + 8, C + 12) if C % 4 == 0 else (C + 1, C + 3, C + 2)
    xd = window(nhwc(x), ldx)
    yo = blank((B, Ho, Wo), ldy)
    _hip.check(L.y2_maxpool_fwd(_hip.ptr(xd), _hip.ptr(yo), B, H, W, C, ldx, ldy, k, s, pad, pad_end, _hip.stream()), 'pool')
    assert torch.equal(nchw(yo[..., :C]).cpu(), y.detach().float())
    assert guards_intact(yo, 0, C)
    dx = blank((B, H, W), lddx)
    a = window(nhwc(dy), ldy)
    b = window(nhwc(dy2), ldy) if with_dy2 else None
    _hip.check(L.y2_maxpool_bwd(_hip.ptr(xd), _hip.ptr(a), _hip.ptr(b), _hip.ptr(dx), B, H, W, C, ldx, ldy, lddx, k, s, pad, pad_end, _hip.stream()), 'pool_bwd')
    np.testing.assert_allclose(nchw(dx[..., :C]).cpu().numpy(), x64.grad.float().numpy(), rtol=1e-6, atol=1e-6)
    assert guards_intact(dx, 0, C) and guards_intact(xd, 0, C) and guards_intact(a, 0, C)


# ================================================================================================ 5. colsum, f64 -> f32, decode backward
@pytest.mark.parametrize('M', [1, 13 * 13 * 2, 19 * 19 * 8])
@pytest.mark.parametrize('C', [1, 4, 125, 425])
def test_colsum_accumulates_column_sums(C, M):
    """y2_colsum (out += column sums of a strided [M, C] matrix) at the VOC / COCO head widths; the summation bound of the BN-backward sums with
    K = items per thread + 256 LDS atomics."""
    import _hip
    L = _hip.lib()
    ld = C + 3
    x = randn32(gen(C + M), M, C)
    xd = window(x, ld)
    out = torch.full((C + 4,), SENT, dtype=torch.float64, device=dev())
    out[:C] = 3.0
    _hip.check(L.y2_colsum(_hip.ptr(xd), M, C, ld, _hip.ptr(out), _hip.stream()), 'colsum')
    unit = C // math.gcd(256, C)
    want = min(max((M * C + 256 * 16 - 1) // (256 * 16), 1), NUM_CU * 4)
    grid = (want + unit - 1) // unit * unit
    K = (M * C + grid * 256 - 1) // (grid * 256) + 256
    err = (out[:C].cpu() - (3.0 + x.double().sum(0))).abs()
    bound = K * EPS32 * x.double().abs().sum(0)
    assert bool((err <= bound).all()), (err / bound).max().item()
    assert bool((out[C:] == SENT).all()) and guards_intact(xd, 0, C)


@pytest.mark.parametrize('n', [1, 257])
def test_f64_to_f32_scales_and_rounds(n):
    import _hip
    L = _hip.lib()
    mul = 1.0 / 77.0
    src = torch.randn(n, generator=gen(n), dtype=torch.float64) * 1e3
    dst = torch.full((n + 8,), SENT, device=dev())
    sd = src.to(dev())
    _hip.check(L.y2_f64_to_f32(_hip.ptr(sd), ctypes.c_void_p(dst.data_ptr() + 16), n, mul, _hip.stream()), 'f64_to_f32')
    assert torch.equal(dst[4:4 + n].cpu(), (src * mul).float())
    assert guards_intact(dst, 4, n) and torch.equal(sd.cpu(), src)


@pytest.mark.parametrize('null', [None, 'iou', 'center_offset', 'size_norm', 'logits'])
@pytest.mark.parametrize('C', [0, 3, 20])
def test_decode_backward_matches_autograd(C, null):
    """y2_decode_bwd against fp64 autograd through oracle/head.py's decode; each incoming gradient is NULL in one run, and its block of d_feature
    is then exactly zero.  The kernel takes the fp32 sigmoid s as an input, so 1 - s carries a relative error eps * e^x: features are kept within
    +-3 (e^3 * 6e-8 = 1.2e-6), inside rtol = 1e-5."""
    import _hip
    L = _hip.lib()
    d = dev()
    B, S, A = 2, 5, 3
    E = 5 + C
    g = gen(7 * C + 1)
    feature = randn32(g, B, A * E, S, S).clamp(-3.0, 3.0)
    anchors = (torch.rand(A, 2, generator=g, dtype=torch.float32) * 3 + 0.5).double()
    f64 = feature.double().requires_grad_(True)
    pred = ohead.decode(f64, anchors)
    names = ['iou', 'center_offset', 'size_norm'] + (['logits'] if C > 0 else [])
    grads = {k: (randn32(g, *pred[k].shape) if k != null else None) for k in names}
    grads.setdefault('logits', None)
    sum((pred[k] * grads[k].double()).sum() for k in names if grads[k] is not None).backward()
    boxes = B * S * S * A
    iou, co = pred['iou'].detach().float().contiguous().to(d), pred['center_offset'].detach().float().contiguous().to(d)
    gd = {k: (v.contiguous().to(d) if v is not None else None) for k, v in grads.items()}
    dfeat = torch.full((boxes * E + 8,), SENT, device=d)
    _hip.check(L.y2_decode_bwd(_hip.ptr(iou), _hip.ptr(co), _hip.ptr(gd['iou']), _hip.ptr(gd['center_offset']), _hip.ptr(gd['size_norm']), _hip.ptr(gd['logits']),
                               _hip.ptr(dfeat), boxes, C, _hip.stream()), 'decode_bwd')
    got = dfeat[:boxes * E].view(boxes, E).cpu()
    ref = f64.grad.permute(0, 2, 3, 1).reshape(boxes, E)
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-5, atol=1e-7)
    assert bool((dfeat[boxes * E:] == SENT).all())
    blocks = {'iou': slice(0, 1), 'center_offset': slice(1, 3), 'size_norm': slice(3, 5), 'logits': slice(5, E)}
    if null is not None:
        assert bool((got[:, blocks[null]] == 0).all())
        assert bool((ref[:, blocks[null]] == 0).all())
