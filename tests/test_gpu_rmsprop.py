"""GPU tests of y2_opt_rmsprop / utils.optim.RMSprop against torch.optim.RMSprop on the same device: the five hyper-parameter forms on the
tensor set of test_fused_optimizer_matches_torch_optim, the sizes at which the chunking and the 16-B / scalar paths change, writes confined to
each tensor (sentinel padding), the refusals of the C entry point, and a captured launch."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 2e-7          # test_fused_optimizer_matches_torch_optim's
KINDS = dict(plain=dict(), wd=dict(weight_decay=1e-2), momentum=dict(momentum=0.9), centered=dict(centered=True),
             centered_momentum_wd=dict(centered=True, momentum=0.9, weight_decay=1e-2))
STATES = ('square_avg', 'momentum_buffer', 'grad_avg')


def dev():
    return torch.device('cuda:0')


def worst(got, want):
    """max of |got - want| / (ATOL + RTOL * |want|): <= 1 is what assert_allclose(rtol=RTOL, atol=ATOL) accepts."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float(((got - want).abs() / (ATOL + RTOL * want.abs())).max())


@pytest.mark.parametrize('kind', list(KINDS))
def test_fused_rmsprop_matches_torch_optim(kind):
    """utils.optim.RMSprop (one launch per 48 tensors) against torch.optim.RMSprop on 60 tensors of assorted (odd, unaligned, large) sizes plus a
    view offset by one float, 4 steps, one parameter skipping step 2: parameters and every state tensor at rtol=2e-5, atol=2e-7.
    Measured on an MI355X with torch 2.10, worst error in units of that tolerance: 0.0 for parameters and states in all five forms (bit-identical).
    A kernel that rounds every product separately gave plain 0.22, wd 2.9 (param), momentum 17.7 (momentum_buffer), centered 0.22,
    centered_momentum_wd 10.6 (param) / 15.8 (momentum_buffer): the kernel fuses the multiply-adds torch's own kernels fuse (csrc/optim.hip)."""
    import utils
    d = dev()
    g = torch.Generator().manual_seed(3)
    shapes = [(125,), (1,), (3, 3, 3, 3), (1024, 1025), (7,), (64, 32, 3, 3), (33,), (4096,), (4097,), (2, 5)] * 6
    init = [torch.randn(*s, generator=g) for s in shapes]
    ours = [torch.nn.Parameter(t.clone().to(d)) for t in init]
    ref = [torch.nn.Parameter(t.clone().to(d)) for t in init]
    base_o = torch.randn(1001, generator=g).to(d)
    base_r = base_o.clone()
    ours.append(torch.nn.Parameter(base_o[1:]))          # storage offset by one float: 16-B alignment lost -> scalar path
    ref.append(torch.nn.Parameter(base_r[1:]))
    kw = KINDS[kind]
    a, b = utils.optim.RMSprop(ours, 1e-2, alpha=0.99, eps=1e-8, **kw), torch.optim.RMSprop(ref, 1e-2, alpha=0.99, eps=1e-8, **kw)
    for step in range(4):
        for po, pr in zip(ours, ref):
            gr = torch.randn(po.shape, generator=g).to(d)
            po.grad, pr.grad = gr.clone(), gr.clone()
        if step == 2:       # a parameter that skips a step keeps its state
            ours[3].grad = None
            ref[3].grad = None
        a.step()
        b.step()
    figures = dict(param=max(worst(po, pr) for po, pr in zip(ours, ref)))
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sa['state'].keys()) == set(sb['state'].keys())
    for k in sa['state']:
        assert set(sa['state'][k].keys()) == set(sb['state'][k].keys()), k
        assert float(sa['state'][k]['step']) == float(sb['state'][k]['step']), k
        for name in STATES:
            if name in sb['state'][k]:
                figures[name] = max(figures.get(name, 0.0), worst(sa['state'][k][name], sb['state'][k][name]))
    print('rmsprop %s: worst error in units of the tolerance: %s' % (kind, figures))
    expected = {'param', 'square_avg'} | ({'momentum_buffer'} if kw.get('momentum') else set()) | ({'grad_avg'} if kw.get('centered') else set())
    assert set(figures) == expected
    for po, pr in zip(ours, ref):
        np.testing.assert_allclose(po.detach().cpu().numpy(), pr.detach().cpu().numpy(), rtol=RTOL, atol=ATOL)
    for k in sa['state']:
        for name in STATES:
            if name in sb['state'][k]:
                np.testing.assert_allclose(sa['state'][k][name].cpu().numpy(), sb['state'][k][name].cpu().numpy(), rtol=RTOL, atol=ATOL, err_msg='%s[%s]' % (name, k))


PAD = 4                 # floats of sentinel in front of and behind every buffer (16 bytes: an aligned interior stays aligned)
SENTINEL = 12345.0
# (numel, offset of the parameter / gradient / momentum / grad_avg views beyond PAD, offset of square_avg beyond PAD)
EDGES = [(1, 0, 0), (3, 0, 0), (4, 0, 0), (5, 0, 0), (1023, 0, 0), (1024, 0, 0), (1025, 0, 0), (4095, 0, 0), (4096, 0, 0), (4097, 0, 0), (8193, 0, 0),
         (1000, 1, 1),          # a view at storage offset 1: every pointer unaligned
         (1000, 0, 1)]          # an aligned parameter whose square_avg alone is a view at offset 1: the tensor must take the scalar path


def padded(values, offset):
    """(whole buffer, view of len(values) elements at PAD + offset) on the device, sentinels everywhere else."""
    whole = torch.full((PAD + offset + values.numel() + PAD,), SENTINEL)
    whole[PAD + offset:PAD + offset + values.numel()] = values
    whole = whole.to(dev())
    return whole, whole[PAD + offset:PAD + offset + values.numel()]


def test_rmsprop_edge_sizes_in_one_49_tensor_call_write_nothing_outside():
    """49 tensors (the table splits 48 + 1) of the sizes where the kernel changes path - numel 1, 3, 4, 5 (vector tail), 1023, 1024, 1025 (one
    pass of 256 lanes x 4), 4095, 4096, 4097 (one chunk), 8193, and the two unaligned forms - centred with momentum and weight decay so that all
    five buffers of a tensor are read and written.  Two steps against torch.optim.RMSprop; the sentinels around every buffer are untouched."""
    import utils
    g = torch.Generator().manual_seed(11)
    kw = dict(alpha=0.99, eps=1e-8, centered=True, momentum=0.9, weight_decay=1e-2)
    cases = [EDGES[i % len(EDGES)] for i in range(49)]
    assert cases[48] == EDGES[48 % len(EDGES)] and len(cases) == 49
    buffers, ours, ref = [], [], []
    for n, off, off_sq in cases:
        value = torch.randn(n, generator=g)
        whole, view = padded(value, off)
        p = torch.nn.Parameter(view)
        assert (p.data_ptr() % 16 == 0) == (off == 0)
        states = {}
        for name, o in (('square_avg', off_sq), ('momentum_buffer', off), ('grad_avg', off)):
            w, v = padded(torch.zeros(n), o)
            buffers.append((name, n, o, w))
            states[name] = v
        buffers.append(('param', n, off, whole))
        ours.append((p, states))
        ref.append(torch.nn.Parameter(value.clone().to(dev())))
    a = utils.optim.RMSprop([p for p, _ in ours], 1e-2, **kw)
    for p, states in ours:          # the optimizer's own state layout, on the padded buffers
        a.state[p] = dict(step=torch.tensor(0.0), **states)
    b = torch.optim.RMSprop(ref, 1e-2, **kw)
    for step in range(2):
        for (p, _), pr, (n, off, _) in zip(ours, ref, cases):
            gr = torch.randn(n, generator=g)
            whole, view = padded(gr, off)
            buffers.append(('grad', n, off, whole))
            p.grad, pr.grad = view, gr.to(dev())
        a.step()
        b.step()
    torch.cuda.synchronize()
    for (p, states), pr, case in zip(ours, ref, cases):
        np.testing.assert_allclose(p.detach().cpu().numpy(), pr.detach().cpu().numpy(), rtol=RTOL, atol=ATOL, err_msg=str(case))
        for name in STATES:
            np.testing.assert_allclose(states[name].cpu().numpy(), b.state[pr][name].cpu().numpy(), rtol=RTOL, atol=ATOL, err_msg='%s %s' % (name, case))
        assert float(a.state[p]['step']) == 2.0
    for name, n, o, whole in buffers:
        h = whole.cpu()
        assert bool((h[:PAD + o] == SENTINEL).all()) and bool((h[PAD + o + n:] == SENTINEL).all()), (name, n, o)


def _table(rows):
    import _hip
    table = (_hip.OptTensor * len(rows))()
    for e, (p, g, s1, s2, n) in zip(table, rows):
        e.param, e.grad, e.state1, e.state2, e.numel = p, g, s1, s2, n
    return table


def test_rmsprop_refusals_return_einval_and_write_nothing():
    import _hip
    L = _hip.lib()
    EINVAL = -1
    assert _hip.ERRORS[EINVAL].startswith('Y2_EINVAL')
    d = dev()
    n = 100
    p, g, sq, buf, ga = (torch.full((n,), float(i + 1), device=d) for i in range(5))
    before = [t.clone() for t in (p, g, sq, buf, ga)]
    row = (p.data_ptr(), g.data_ptr(), sq.data_ptr(), buf.data_ptr(), n)
    third = (ctypes.c_void_p * 49)(*([ga.data_ptr()] * 49))
    hyper = (1e-2, 0.99, 1e-8, 0.0)
    st = _hip.stream()
    call = lambda table, count, grad_avg, momentum, centered: L.y2_opt_rmsprop(table, count, grad_avg, *hyper, momentum, centered, st)
    assert call(_table([row]), 0, third, 0.9, 1) == EINVAL
    assert call(_table([row] * 49), 49, third, 0.9, 1) == EINVAL
    assert call(None, 1, third, 0.9, 1) == EINVAL
    assert call(_table([(row[0], row[1], row[2], None, n)]), 1, None, 0.9, 0) == EINVAL            # momentum without state2
    assert call(_table([row]), 1, None, 0.0, 1) == EINVAL                                            # centred without grad_avg
    assert call(_table([row]), 1, (ctypes.c_void_p * 1)(None), 0.0, 1) == EINVAL                     # ... or with a NULL entry
    assert call(_table([(row[0], None, row[2], row[3], n)]), 1, third, 0.9, 1) == EINVAL             # a NULL grad
    assert call(_table([(None, row[1], row[2], row[3], n)]), 1, third, 0.9, 1) == EINVAL             # a NULL param
    assert call(_table([(row[0], row[1], None, row[3], n)]), 1, third, 0.9, 1) == EINVAL             # no square_avg
    assert call(_table([row[:4] + (0,)]), 1, third, 0.9, 1) == EINVAL                                # numel <= 0
    assert call(_table([row, (row[0], None, row[2], row[3], n)]), 2, third, 0.9, 1) == EINVAL        # the second row is bad: the first is not launched either
    torch.cuda.synchronize()
    for t, was in zip((p, g, sq, buf, ga), before):
        assert torch.equal(t, was)
    # state2 and grad_avg that are not required are not read: plain RMSprop with both absent runs
    assert call(_table([(row[0], row[1], row[2], None, n)]), 1, None, 0.0, 0) == 0
    torch.cuda.synchronize()
    assert not torch.equal(p, before[0]) and torch.equal(buf, before[3]) and torch.equal(ga, before[4])


def test_rmsprop_launch_replays_from_a_captured_graph():
    """One y2_opt_rmsprop launch captured in a graph and replayed twice leaves parameters and states bit-equal to two eager launches."""
    import _hip
    L = _hip.lib()
    d = dev()
    sizes = (4097, 33, 1024)
    hyper = (1e-2, 0.99, 1e-8, 1e-2, 0.9, 1)

    def make():
        gen = torch.Generator().manual_seed(6)
        return [[torch.randn(n, generator=gen).to(d), torch.randn(n, generator=gen).to(d)] + [torch.zeros(n, device=d) for _ in range(3)] for n in sizes]

    def launch(rows):
        table = _table([(p.data_ptr(), gr.data_ptr(), sq.data_ptr(), buf.data_ptr(), p.numel()) for p, gr, sq, buf, ga in rows])
        third = (ctypes.c_void_p * len(rows))(*[ga.data_ptr() for _, _, _, _, ga in rows])
        _hip.check(L.y2_opt_rmsprop(table, len(rows), third, *hyper, _hip.stream()), 'y2_opt_rmsprop')
    eager, static = make(), make()
    launch(eager)
    launch(eager)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(static)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for re, rs in zip(eager, static):
        for te, ts in zip(re, rs):
            assert torch.equal(te, ts)
    assert not torch.equal(eager[0][0], make()[0][0])
