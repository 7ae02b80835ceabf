"""Host logic of the binding that needs no GPU: the per-shape plan LRU (multi-scale training, utils/data.py:135-141), the measured-choice
table's export / import (what data-parallel ranks exchange, train.py:427-433) and the static algorithm preferences (Y2_AUTOTUNE=0)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'yolo2-pytorch_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def test_plan_cache_is_an_lru_bounded_by_entries_and_bytes():
    import _hip
    c = _hip.PlanCache(entries=3, gbytes=1.0)
    for i in range(3):
        c.put(('shape', i), {'id': i}, 100 << 20)
    assert c.get(('shape', 0))['id'] == 0                      # touch 0: 1 is now the oldest
    c.put(('shape', 3), {'id': 3}, 100 << 20)
    assert c.get(('shape', 1)) is None and c.get(('shape', 0)) is not None and c.get(('shape', 3)) is not None
    c.put(('shape', 4), {'id': 4}, 900 << 20)                  # the byte bound evicts until the newest fits with what is left
    assert c.get(('shape', 4)) is not None and sum(p['nbytes'] for p in c.d.values()) <= (1 << 30)
    c.put(('huge',), {'id': 9}, 5 << 30)                       # a plan larger than the bound still stays (the cache never drops its only entry)
    assert c.latest()['id'] == 9 and len(c.d) == 1
    assert c.hits == 4 and c.misses == 1


def test_tune_table_round_trip_keeps_choices_and_device_placeholders(monkeypatch):
    import _hip
    monkeypatch.setattr(_hip, '_TUNE', {})
    monkeypatch.setattr(_hip, 'TUNE_CACHE', None)
    key_conv = (64, 13, 13, 512, 512, 1024, 3, True, False, False, 0, 0, 0, False, 0, 0, 0, 'cuda:0', True, True)
    key_wgrad = ('wgrad', 64, 13, 13, 512, 512, 1024, 1024, True, 'cuda:0')
    _hip._TUNE[key_conv] = [2, 3]
    _hip._TUNE[key_wgrad] = 2
    blob = _hip.export_tune()
    monkeypatch.setattr(_hip, '_TUNE', {})
    epoch = _hip.tune_epoch()
    _hip.import_tune(blob, 'cuda:3')                           # another rank's device name
    assert len(_hip._TUNE) == 2 and _hip.tune_epoch() != epoch     # plans built on the old choices are invalidated
    got = {k: v for k, v in _hip._TUNE.items()}
    assert any(k[0] == 'wgrad' and k[-1] == 'cuda:3' and v == 2 for k, v in got.items())
    assert any(k[0] == 64 and 'cuda:3' in k and list(v) == [2, 3] for k, v in got.items())


def test_tune_table_merge_keeps_local_entries_and_moves_the_epoch_only_on_change(monkeypatch):
    import _hip
    monkeypatch.setattr(_hip, '_TUNE', {('a', 'cuda:1'): [1, 5], ('mine', 'cuda:1'): 2})
    epoch = _hip.tune_epoch()
    _hip.import_tune([(('a', '@dev'), (1, 5))], 'cuda:1', merge=True)          # nothing new: plans stay valid
    assert _hip.tune_epoch() == epoch and len(_hip._TUNE) == 2
    _hip.import_tune([(('a', '@dev'), [2, 0]), (('b', '@dev'), 1)], 'cuda:1', merge=True)
    assert _hip.tune_epoch() == epoch + 1
    assert _hip._TUNE == {('a', 'cuda:1'): [2, 0], ('mine', 'cuda:1'): 2, ('b', 'cuda:1'): 1}


@pytest.mark.parametrize('cin,hw,want', [(32, 208, 0), (64, 104, 0), (128, 52, 1), (256, 26, 1), (512, 13, 2), (1024, 19, 2), (1280, 13, 2)])
def test_static_weight_gradient_preferences(monkeypatch, cin, hw, want):
    """Y2_AUTOTUNE=0: the choices the measurements converge to - direct kernel below 128 input channels, the 2x2-tile Winograd reduction above,
    its 4x4-tile form on the 13x13 / 19x19 layers; the deterministic mode never takes the 4x4 form (the library refuses it there)."""
    import _hip
    monkeypatch.setattr(_hip, 'AUTOTUNE', False)
    monkeypatch.setattr(_hip, 'DETERMINISTIC', False)
    monkeypatch.setattr(_hip, 'WINOGRAD', True)
    monkeypatch.setattr(_hip, 'WGRAD_F34', True)
    assert _hip.wgrad_choice(64, hw, hw, cin, cin, 2 * cin, 2 * cin, 3, True, 'cuda:0') == want
    assert _hip.wgrad_choice(64, hw, hw, cin, cin, 2 * cin, 2 * cin, 1, True, 'cuda:0') == 0          # 1x1 layers: the direct kernel
    monkeypatch.setattr(_hip, 'DETERMINISTIC', True)
    assert _hip.wgrad_choice(64, hw, hw, cin, cin, 2 * cin, 2 * cin, 3, True, 'cuda:0') == (1 if cin >= 128 else 0)


def test_default_tune_table_is_adopted_only_for_the_kernels_it_was_measured_on(monkeypatch, tmp_path):
    """The committed table (yolo2-pytorch_amd/tune/default_gfx950.json) carries the hash of the kernel sources: entries are adopted for the
    device they are asked for, never over a choice this process already holds, and not at all when the sources have changed."""
    import json

    import _hip
    monkeypatch.setattr(_hip, '_TUNE', {('mine', 'cuda:2'): [1, 5]})
    monkeypatch.setattr(_hip, '_DEFAULTS_SEEN', {})
    monkeypatch.setattr(_hip, 'TUNE_DEFAULTS', True)
    h = _hip.kernel_hash()
    assert h is not None and len(h) == 16 and h == _hip.kernel_hash()
    good = tmp_path / 'good.json'
    json.dump({'kernels': h, 'entries': [[['mine', '@dev'], [0, 0]], [['wgrad', 64, 13, 13, 512, 512, 1024, 1024, True, '@dev'], 2], [[32, 13, 13, True, '@dev', False], [1, 5]]]}, open(good, 'w'))
    assert _hip.load_tune_defaults('cuda:2', str(good)) == 2
    assert _hip._TUNE[('mine', 'cuda:2')] == [1, 5]                       # what the process held stays
    assert _hip._TUNE[('wgrad', 64, 13, 13, 512, 512, 1024, 1024, True, 'cuda:2')] == 2 and _hip._TUNE[(32, 13, 13, True, 'cuda:2', False)] == [1, 5]
    stale = tmp_path / 'stale.json'
    json.dump({'kernels': '0' * 16, 'entries': [[['other', '@dev'], [2, 0]]]}, open(stale, 'w'))
    assert _hip.load_tune_defaults('cuda:2', str(stale)) == 0 and ('other', 'cuda:2') not in _hip._TUNE
    # the committed file, when there is one, parses and names a hash
    if os.path.exists(_hip.DEFAULTS_PATH):
        d = json.load(open(_hip.DEFAULTS_PATH))
        assert len(d['kernels']) == 16 and all(len(e) == 2 for e in d['entries'])


def test_step_runner_keeps_one_plan_per_shape_and_degrades_per_shape(monkeypatch):
    """train.StepRunner's bookkeeping without a GPU (the plans are stand-ins): a batch with fewer boxes runs in the plan captured for more, a batch with
    more supersedes it, warm-up is counted per input shape, a capture that runs out of memory drops the OTHER captured steps and leaves that shape on
    eager launches, any other capture failure stops capturing - and no failure ever stops the step from running."""
    import torch

    import train
    from model import train_graph

    made = []

    class FakePlan(object):
        WARM = 3

        def __init__(self, inference, anchors, hparam, threshold, dp=None, pool=None, shared=None, arena=None, scope=None):
            self.ops, self.capture_error, self.calls, self.static, self.params, self.last_grads = None, None, 0, None, [], {}
            self.used_last = None
            self.fail = None
            made.append(self)

        def _alloc(self, data, npad):
            self.static = {'npad': npad}

        def valid(self):
            return True

        def run(self, data, capture=True):
            self.calls += 1
            if self.ops is None and capture and self.calls > self.WARM and self.capture_error is None:
                if self.fail is not None:
                    self.capture_error = self.fail
                else:
                    self.ops = [('graph', None)]
            return {'ran': self.calls}
    monkeypatch.setattr(train_graph, 'StepPlan', FakePlan)
    monkeypatch.setattr(torch.cuda, 'graph_pool_handle', lambda: object())
    monkeypatch.setattr(torch.cuda, 'empty_cache', lambda: None)
    monkeypatch.setattr(train.StepRunner, 'eligible', lambda self, data: True)
    r = train.StepRunner(object(), None, object(), {'foreground': 5.0}, 0.6)

    def batch(S, n):
        return {'tensor': torch.zeros(2, 3, S, S), 'yx_min': torch.zeros(2, n, 2), 'yx_max': torch.zeros(2, n, 2), 'cls': torch.zeros(2, n, dtype=torch.int64)}
    for _ in range(5):
        assert r.step(batch(96, 6))['ran']
    assert len(r.plans) == 1 and r.captures == 1 and made[-1].static['npad'] == 16
    assert r.step(batch(96, 3)) and len(r.plans) == 1 and len(made) == 1                 # fewer boxes: the same plan
    assert r.step(batch(96, 40)) and len(r.plans) == 1 and len(made) == 2               # more boxes: a 64-row plan supersedes it ...
    assert made[-1].static['npad'] == 64 and r.captures == 2                             # ... captured at its first call (the shape is warm)
    assert r.step(batch(96, 6)) and len(made) == 2                                       # and serves the small batches from now on
    for _ in range(4):
        r.step(batch(128, 6))
    assert len(r.plans) == 2 and r.captures == 3
    # out of memory while capturing a third shape: the step runs, the other captured steps are dropped, the shape stays eager
    for i in range(3):
        r.step(batch(160, 6))
    made[-1].fail = torch.cuda.OutOfMemoryError('HIP out of memory')
    assert r.step(batch(160, 6))['ran'] == 4
    assert len(r.plans) == 1 and not r.broken and len(r.eager_only) == 1
    assert r.step(batch(160, 6))['ran'] == 5 and made[-1].ops is None                   # no second attempt for that shape
    for _ in range(4):
        r.step(batch(96, 6))                                                             # the others capture again, in a fresh pool
    assert r.captures == 4
    # any other failure: no more captures for this model, steps keep running
    for i in range(3):
        r.step(batch(192, 6))
    made[-1].fail = RuntimeError('boom')
    assert r.step(batch(192, 6))['ran'] == 4 and r.broken
    for _ in range(5):
        assert r.step(batch(224, 6))
    assert made[-1].ops is None and r.captures == 4


def test_oplist_builder_selection_names_an_unknown_class():
    """model.train_oplist picks the builder function by the network's class, in one place; a module of any other class is refused by name
    before anything is launched."""
    import torch.nn as nn

    import model.resnet
    import model.yolo2
    from model import train_oplist
    assert train_oplist._builder(object.__new__(model.yolo2.Tiny)) is train_oplist._build_tiny          # (a subclass of Darknet: not Darknet's graph)
    assert train_oplist._builder(object.__new__(model.resnet.ResNet)) is train_oplist._build_resnet
    with pytest.raises(TypeError, match=r'no training-graph builder for torch\.nn\.modules\.linear\.Linear'):
        train_oplist._builder(nn.Linear(1, 1))


# ---- the backward's decisions: taken once per pass (model.train_graph._decide_bwd), applied - not looked up again - by _hip.conv_wgrad / autotune_conv
def _darknet19_geometry(tg, _hip, B=64, S=416):
    """[_Geo] of the full-width Darknet-19 at SxS, from the oracle's layer table (prepared operands everywhere but the first layer and the head)."""
    from oracle import darknet as odark
    rows, h, c = [], S, 3                        # (name, H, cin, cout, k, pool)
    for j, item in enumerate(odark.LAYERS1):
        if item == 'M':
            continue
        name, k, cout = item
        pool = odark.LAYERS1[j + 1:j + 2] == ['M'] or name == odark.LAYERS1[-1][0]          # (layers2's leading pool belongs to layers1[-1])
        rows.append((name, h, c, cout, k, pool))
        h, c = (h // 2 if pool else h), cout
    n1, c_pt = len(rows), odark.PASSTHROUGH[2]
    rows.append(('passthrough', 2 * h, c, c_pt, 1, False))
    for name, k, cout in odark.LAYERS2[1:] + [(odark.LAYERS3[0][0], odark.LAYERS3[0][1], odark.LAYERS3[0][2]), ('layers3.1', 1, 125)]:
        cin = 4 * c_pt + c if name == 'layers3.0' else c
        rows.append((name, h, cin, cout, k, False))
        c = cout
    names = [r[0] for r in rows]
    routes, full, pooled = tg._routes(names, [r[5] for r in rows], n1, c_pt)
    geo = [tg._Geo(H, H, cin, cout, k, cin, i == 0, False, False, None if (i == 0 or cout % 4) else bool(_hip.wino_eligible(cin, cout, k)), full[i], pooled[i])
           for i, (name, H, cin, cout, k, pool) in enumerate(rows)]
    return names, geo


def _wgrad_key(g, B=64):
    return ('wgrad', B, g.H, g.W, g.cin, g.ldx, g.cout, g.cout, False, 'cuda:0')


def _dgrad_key(g, B=64):          # the data gradient of a block is a convolution with the roles of Cin and Cout exchanged, offered the 4x4-tile form
    return (B, g.H, g.W, g.cout, g.cout, g.cin, 3, True, False, False, 0, 0, 0, False, 0, 0, 0, 'cuda:0', True, True, 'f43')


@pytest.fixture
def tune_defaults(monkeypatch):
    """An empty algorithm table, nothing pinned, every A/B switch at its default."""
    import _hip
    from model import train_graph as tg
    for name, value in (('_TUNE', {}), ('_DEFAULTS_SEEN', {'cuda:0': 0}), ('TUNE_CACHE', None), ('AUTOTUNE', True), ('DETERMINISTIC', False), ('WINOGRAD', True), ('IMPLICIT', True),
                        ('PERSIST', True), ('SPLIT', ''), ('FORCE_ALGO', None), ('FORCE_GRAD', None), ('FORCE_WGRAD', None)):
        monkeypatch.setattr(_hip, name, value)
    for name, value in (('FUSE_CONV0', True), ('FUSE_WINO6', True), ('GRAD_F43', True), ('DEBUG_TAP', None)):
        monkeypatch.setattr(tg, name, value)
    return _hip, tg


def test_backward_decisions_are_taken_once_from_the_table(tune_defaults, monkeypatch):
    _hip, tg = tune_defaults
    names, geo = _darknet19_geometry(tg, _hip)
    assert len(geo) == 23 and names[-2:] == ['layers3.0', 'layers3.1'] and geo[-2].cin == 1280 and geo[13].H == 26 and geo[14].H == 13
    deep = [i for i, g in enumerate(geo) if (g.H, g.cin, g.cout, g.k) == (13, 512, 1024, 3)]
    assert [names[i] for i in deep] == ['layers2.1', 'layers2.3', 'layers2.5']
    for i in deep:
        _hip._TUNE[_wgrad_key(geo[i])] = 2
        _hip._TUNE[_dgrad_key(geo[i])] = [6, 5]
    plans = tg._decide_bwd(geo, 64, 'cuda:0')
    assert [i for i, p in enumerate(plans) if p.fused6] == deep and all(plans[i].fused6 == (6, 5) and plans[i].wgrad == 2 and not plans[i].zero for i in deep)
    assert plans[0] == tg._Plan(0, True, True, True, None, None)                                  # the first layer: its own kernel, dz formed inside it
    assert not tg._decide_bwd(geo, 64, 'cuda:0', need_dx=True)[0].fuse0
    for i, (g, p) in enumerate(zip(geo, plans)):
        if i and g.k == 3 and i not in deep:                                                # no entry: unknown - and NOT in the zero fill as if it were choice 0
            assert p.wgrad is None and not p.zero and not p.final and p.fused6 is None, names[i]
        if g.k == 1:                                                                        # the direct kernel: accumulates; [cout][1][cin] is the gradient's layout
            assert p.wgrad == 0 and p.zero and p.final == (g.cout % 4 == 0) and p.fused6 is None, names[i]
    # the records are values, not views of the table
    kept = list(plans)
    _hip._TUNE.clear()
    monkeypatch.setattr(_hip, 'FORCE_WGRAD', 'direct')
    assert plans == kept and plans[deep[0]].wgrad == 2 and plans[deep[0]].fused6 == (6, 5)
    # pinned to the direct kernel (a table that says otherwise does not count): every 3x3 target is zero filled, nothing is fused
    for i in deep:
        _hip._TUNE[_wgrad_key(geo[i])] = 2
        _hip._TUNE[_dgrad_key(geo[i])] = [6, 5]
    direct = tg._decide_bwd(geo, 64, 'cuda:0')
    assert all(p.zero and p.wgrad == 0 for g, p in zip(geo, direct) if g.k == 3) and not any(p.fused6 for p in direct)
    # a table that offers both 4x4-tile forms EVERYWHERE: the pooled blocks, the reorg source and the head still never take the fused form
    monkeypatch.setattr(_hip, 'FORCE_WGRAD', None)
    for g in geo[1:]:
        _hip._TUNE[_wgrad_key(g)] = 2
        _hip._TUNE[_dgrad_key(g)] = [6, 5]
    wide = tg._decide_bwd(geo, 64, 'cuda:0')
    fused = [names[i] for i, p in enumerate(wide) if p.fused6]
    assert fused == ['layers1.8', 'layers1.12', 'layers1.14'] + ['layers2.%d' % j for j in (1, 3, 5, 6, 7)] + ['layers3.0']
    assert not any(p.fused6 for g, p in zip(geo, wide) if g.pooled or g.full != 0 or g.k == 1) and any(g.pooled and p.wgrad == 2 for g, p in zip(geo, wide))
    for flag, holder in (('FUSE_WINO6', tg), ('DETERMINISTIC', _hip), ('SPLIT', _hip)):     # the A/B switch, the deterministic and the split modes: never
        monkeypatch.setattr(holder, flag, not getattr(holder, flag))
        assert not any(p.fused6 for p in tg._decide_bwd(geo, 64, 'cuda:0')), flag
        monkeypatch.setattr(holder, flag, not getattr(holder, flag))


class _Recorder(object):
    """Stands in for _hip.lib(): records the entry points asked for; they run when `real` is given, else return `rc`."""

    def __init__(self, real=None, rc=0):
        self.real, self.rc, self.names = real, rc, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self.real, name) if self.real is not None else (lambda *a: self.rc)


@pytest.mark.parametrize('B,hw,cin,want', [(2, 13, 1024, (6, 5)), (32768, 52, 1024, (0, 0))])          # accepted; refused on size (tiles x Cin >= 2^32)
def test_peek_equals_launch_under_the_pinned_gradient_algorithm(tune_defaults, monkeypatch, B, hw, cin, want):
    import torch
    _hip, tg = tune_defaults
    monkeypatch.setattr(_hip, 'FORCE_GRAD', 'f43')
    rec = _Recorder(_hip.lib())
    monkeypatch.setattr(_hip, 'lib', lambda: rec)
    monkeypatch.setattr(_hip, 'workspace', lambda *a: pytest.fail('scratch allocated'))
    operand = torch.zeros(4)

    def never():
        pytest.fail('the 4x4-tile operand was built for a question')
    p = tg._problem(B, hw, hw, cin, cin, 512, 3, 512)
    assert _hip.autotune_conv(p, 'cuda:0', f43=never, wino_eligible=True, peek=True) == want and (p.algo, p.tile, p.w) == (0, 0, None)
    p.w = None          # a pruned step: no packed weight at hand - a missing operand is not a refusal
    assert _hip.autotune_conv(p, 'cuda:0', f43=lambda: operand, wino_eligible=True) == want and (p.algo, p.tile) == want
    assert p.w == (operand.data_ptr() if want[0] == 6 else None)
    assert set(rec.names) == {'y2_conv_fwd_workspace_bytes'} and len(rec.names) == 2
    # a decision handed in is applied without a question
    assert _hip.autotune_conv(p, 'cuda:0', f43=lambda: operand, wino_eligible=True, choice=(6, 3)) == (6, 3) and (p.algo, p.tile) == (6, 3) and len(rec.names) == 2
    with pytest.raises(_hip.OperandMissing):
        _hip.autotune_conv(p, 'cuda:0', wino_eligible=True, choice=(1, 5))


def test_conv_wgrad_runs_the_choice_it_is_given(tune_defaults, monkeypatch):
    import torch
    _hip, tg = tune_defaults
    rec = _Recorder(rc=4096)          # (a workspace size; the launches' return codes go through the patched check)
    monkeypatch.setattr(_hip, 'lib', lambda: rec)
    monkeypatch.setattr(_hip, 'check', lambda rc, what: None)
    monkeypatch.setattr(_hip, 'stream', lambda: None)
    B, H, C = 2, 8, 64
    x, dz, out, native = torch.zeros(B, H, H, C), torch.zeros(B, H, H, C), torch.zeros(C * 9 * C), torch.zeros(C, C, 3, 3)
    key = ('wgrad', B, H, H, C, C, C, C, False, 'cpu')
    launch = {0: 'y2_conv_wgrad', 1: 'y2_wino_wgrad', 2: 'y2_wino_wgrad_ex'}

    def run(**kw):
        del rec.names[:]
        got = _hip.conv_wgrad(x, dz, B, H, H, C, C, C, C, 3, out=out, **kw)
        return got, [n for n in rec.names if 'workspace' not in n]
    for choice in (0, 1, 2):
        for table in ({}, {key: (choice + 1) % 3}, {key: (choice + 2) % 3}):          # empty (a lookup would MEASURE), and holding each other answer
            monkeypatch.setattr(_hip, '_TUNE', dict(table))
            assert run(choice=choice, zeroed=True) == (out, [launch[choice]])
            assert run(choice=choice) == (out, (['y2_multi'] if choice == 0 else []) + [launch[choice]])          # the fill: the library's, on the launch stream
            got, names = run(choice=choice, zeroed=True, native=native)
            assert names == ['y2_wino_wgrad_ex' if choice else 'y2_conv_wgrad'] and got is (native if choice else out)
        monkeypatch.setattr(_hip, '_TUNE', {key: choice})
        assert run() == run(choice=choice)                                              # not given: looked up, as before
    monkeypatch.setattr(_hip, 'wgrad_choice', lambda *a: pytest.fail('the table was read'))
    assert run(choice=2, dz_pre=True, native=native) == (native, ['y2_wino_wgrad_ex'])
    with pytest.raises(AssertionError):
        run(choice=0, dz_pre=True)                                                      # a transformed gradient serves the 4x4-tile form only


def _fields(p):
    return {name: getattr(p, name) for name, _ in type(p)._fields_}


def test_conv_params_filler_writes_each_family_form_and_nothing_else():
    """model._infer_parts.conv_params on CPU tensors (addresses only; nothing is launched): Darknet's pooled form leaves stride / pad_plus1 unset -
    they are part of _hip.autotune_conv's key and so of every entry of the committed table -, a ResNet stride-2 residual form and DenseNet's
    channel-offset form set them; every other field is what was asked for or zero."""
    import json
    import torch
    import _hip
    from model._infer_parts import conv_params
    x, w, scale, shift, y, yp, r = [torch.zeros(8) for _ in range(7)]
    zero = dict.fromkeys([name for name, _ in _hip.ConvParams._fields_], 0)
    zero.update(dict.fromkeys(['x', 'w', 'scale', 'shift', 'y', 'y_pool', 'stats', 'workspace', 'residual'], None))

    # Darknet, last layer of layers1: full-resolution output for the passthrough and the pooled one for layers2
    p, f = conv_params(x, w, scale, shift, 2, 8, 12, 16, 16, 32, 3, 0.1, y=y, y_pool=yp, ldy=32, ldp=32)
    assert p.stride == 0 and p.pad_plus1 == 0
    assert _fields(p) == dict(zero, x=x.data_ptr(), w=w.data_ptr(), scale=scale.data_ptr(), shift=shift.data_ptr(), y=y.data_ptr(), y_pool=yp.data_ptr(),
                              B=2, H=8, W=12, Cin=16, ldx=16, Cout=32, ksize=3, ldy=32, ldp=32, slope=_hip.c_float(0.1).value)
    assert f == 2.0 * 16 * 32 * 9 * 2 * 8 * 12
    # the passthrough's reorg'ed output at a channel offset of the concat buffer, no BatchNorm: bias only
    p, _ = conv_params(x, w, None, shift, 2, 8, 12, 16, 16, 4, 1, 1.0, y=y, ldy=48, coff=16, poff=3, out_mode=1)
    assert _fields(p) == dict(zero, x=x.data_ptr(), w=w.data_ptr(), shift=shift.data_ptr(), y=y.data_ptr(),
                              B=2, H=8, W=12, Cin=16, ldx=16, Cout=4, ksize=1, ldy=48, coff=16, poff=3, out_mode=1, slope=1.0)

    # ResNet: the 3x3 stride-2 convolution that ends a block, residual added in the epilogue; the stem's 3 input channels are packed as 4
    pad = 1
    p, f = conv_params(x, w, scale, shift, 2, 9, 13, 4, 4, 8, 3, 0.0, y=y, ldy=8, residual=r, ldr=8, stride=2, pad=pad, real_cin=3)
    assert p.stride == 2 and p.pad_plus1 == pad + 1 and p.residual == r.data_ptr() and p.ldr == 8
    assert _fields(p) == dict(zero, x=x.data_ptr(), w=w.data_ptr(), scale=scale.data_ptr(), shift=shift.data_ptr(), y=y.data_ptr(), residual=r.data_ptr(),
                              B=2, H=9, W=13, Cin=4, ldx=4, Cout=8, ksize=3, ldy=8, ldr=8, stride=2, pad_plus1=2)
    assert f == 2.0 * 3 * 8 * 9 * 2 * 5 * 7          # over the real input channels and the 5x7 output
    # without a residual ldr stays unset
    assert conv_params(x, w, scale, shift, 2, 9, 13, 4, 4, 8, 3, 0.0, y=y, ldy=8, ldr=8, stride=2, pad=pad)[0].ldr == 0

    # DenseNet: a layer's raw 3x3 writes its growth_rate channels at its offset of the block buffer
    p, f = conv_params(x, w, None, None, 2, 8, 8, 12, 12, 6, 3, 1.0, y=y, ldy=40, coff=22, stride=1, pad=1)
    assert p.coff == 22 and p.ldy == 40
    assert _fields(p) == dict(zero, x=x.data_ptr(), w=w.data_ptr(), y=y.data_ptr(),
                              B=2, H=8, W=8, Cin=12, ldx=12, Cout=6, ksize=3, ldy=40, coff=22, slope=1.0, stride=1, pad_plus1=2)
    assert f == 2.0 * 12 * 6 * 9 * 2 * 8 * 8

    # the committed table was measured on these kernel sources: a Python-side change must not make it stale
    assert _hip.kernel_hash() == json.load(open(_hip.DEFAULTS_PATH))['kernels']
