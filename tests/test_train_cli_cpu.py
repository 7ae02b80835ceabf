"""CPU-side checks of the train.py / eval.py workflows: utils.train's Timer / Saver / load_sizes, utils.RegexList, the two command lines, finetune,
the scheduler's epochs, check_nan, the evaluation database, the training loader with worker processes, Eval with a stub detector, and the
constructor / state layout of utils.optim.RMSprop.  No GPU: the loader and Eval use the library's host functions, like tests/test_eval_cpu.py."""
import configparser
import importlib
import json
import logging
import os

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the application on sys.path)

import _hip
import train_cli_cases as cases


@pytest.fixture(scope='module', autouse=True)
def built():
    if not os.path.exists(_hip.LIB_PATH):
        _hip.build()


@pytest.fixture(scope='module')
def workspace(tmp_path_factory):
    root = tmp_path_factory.mktemp('train_cli')
    return root, cases.make_cache(str(root))


# ------------------------------------------------------------------------------------------------ utils.train, utils
@pytest.mark.parametrize('first', [True, False])
def test_timer(monkeypatch, first):
    import utils.train
    now = [1000.0]
    monkeypatch.setattr(utils.train.time, 'time', lambda: now[0])
    timer = utils.train.Timer(10, first)
    assert timer() is first           # first=True: an event at the first call
    now[0] += 10
    assert timer() is False           # exactly `max` seconds: not yet
    now[0] += 0.5
    assert timer() is True
    assert timer() is False           # ... and the clock starts again
    now[0] += 10.5
    assert timer() is True


def test_saver_keeps_the_newest_and_load_model_reads_them_back(tmp_path):
    import utils.train
    notes = []
    saver = utils.train.Saver(str(tmp_path / 'm'), 2, logger=notes.append)
    for step, epoch in ((1, 0), (5, None), (10, 3)):          # step 5 without an epoch file
        base = saver({'w': torch.full((2,), float(step))}, step, epoch)
        assert base == str(tmp_path / 'm' / str(step))
    assert sorted(os.listdir(str(tmp_path / 'm'))) == ['10.epoch', '10.pth', '5.pth']
    path, step, epoch = utils.train.load_model(str(tmp_path / 'm'))
    assert (os.path.basename(path), step, epoch) == ('10.pth', 10, 3)
    assert torch.equal(torch.load(path)['w'], torch.full((2,), 10.0))
    assert utils.train.load_model(str(tmp_path / 'm'), 5)[1:] == (5, None)
    saver({'w': torch.zeros(1)}, 11, 4)                        # 5 goes, its missing .epoch is reported and tolerated
    assert sorted(os.listdir(str(tmp_path / 'm'))) == ['10.epoch', '10.pth', '11.epoch', '11.pth']
    assert any('5.epoch not found' in n for n in notes)
    with open(str(tmp_path / 'm' / '11.epoch')) as f:
        assert f.read() == '4'
    # keep = 2 over 1, 5, 10 with all their epoch files
    saver = utils.train.Saver(str(tmp_path / 'n'), 2, logger=None)
    for step in (1, 5, 10):
        saver({}, step, step)
    assert sorted(os.listdir(str(tmp_path / 'n'))) == ['10.epoch', '10.pth', '5.epoch', '5.pth']


def test_load_sizes_on_the_reference_line():
    import utils.train
    config = configparser.ConfigParser()
    config.read_dict({'data': {'sizes': cases.SIZES_LINE}})
    assert utils.train.load_sizes(config) == [(s, s) for s in range(320, 609, 32)]
    config.set('data', 'sizes', '96,128')
    assert utils.train.load_sizes(config) == [(96, 128)]


def test_regex_list():
    import utils
    ignore = utils.RegexList([r'conv\.', r'layers2\.\d+\.bn'])
    assert ignore('conv.weight') and ignore('layers2.3.bn.weight')
    assert not ignore('layers1.0.conv.weight')            # match, not search: anchored at the start of the key
    assert not ignore('layers2.x.bn') and not utils.RegexList([])('anything')
    assert len(ignore) == 2


def test_make_args_of_both_command_lines():
    import train
    ev = importlib.import_module('eval')
    a = train.make_args([])
    assert (a.config, a.modify, a.batch_size, a.finetune, a.ignore, a.learning_rate, a.delete, a.quiet, a.run, a.logging) == (['config.ini'], [], 16, None, [], 1e-3, False, False, None, None)
    assert a.epoch == np.iinfo(np.int64).max
    a = train.make_args(['-c', 'a.ini', 'b.ini', '-m', 'train/phase=train', 'save/keep=1', '-b', '4', '-f', 'dir', '-i', r'conv\.', 'x', '-lr', '0.01', '-e', '2', '-d', '-q',
                         '-r', 'run0', '--logging', 'logging.yml'])
    assert (a.config, a.modify, a.batch_size, a.finetune, a.ignore, a.learning_rate, a.epoch, a.delete, a.quiet, a.run, a.logging) == (
        ['a.ini', 'b.ini'], ['train/phase=train', 'save/keep=1'], 4, 'dir', [r'conv\.', 'x'], 0.01, 2, True, True, 'run0', 'logging.yml')
    a = train.make_args(['--finetune', 'f', '--ignore', 'y', '--epoch', '3', '--run', 'r', '--delete', '--quiet', '--learning_rate', '1', '--batch_size', '2'])
    assert (a.finetune, a.ignore, a.epoch, a.run, a.delete, a.quiet, a.learning_rate, a.batch_size) == ('f', ['y'], 3, 'r', True, True, 1.0, 2)
    e = ev.make_args([])
    assert (e.config, e.modify, e.batch_size, e.logging) == (['config.ini'], [], 16, None)
    e = ev.make_args(['-c', 'a.ini', '-m', 'eval/metric07=0', '-b', '64', '--logging', 'logging.yml'])
    assert (e.config, e.modify, e.batch_size, e.logging) == (['a.ini'], ['eval/metric07=0'], 64, 'logging.yml')


# ------------------------------------------------------------------------------------------------ pieces of Train
def tiny(seed):
    import model
    import model.yolo2
    config = configparser.ConfigParser()
    config.read_dict({'batch_norm': {'enable': '1'}, 'model': {'pretrained': '0'}})
    torch.manual_seed(seed)
    anchors = torch.tensor(cases.ANCHORS)[:, [1, 0]].contiguous()
    return model.yolo2.Tiny(model.ConfigChannels(config), anchors, 20)


def test_finetune_copies_what_is_not_ignored_and_warns_about_missing_keys(tmp_path, caplog):
    import train
    import utils.train
    source, target = tiny(1), tiny(2)
    state = source.state_dict()
    names = list(state)
    head = [k for k in names if k.startswith('layers.15.')]          # Tiny's head (Darknet's is `conv.`)
    assert head and len(head) < len(names)
    absent = next(k for k in names if not k.startswith('layers.15.'))
    del state[absent]
    utils.train.Saver(str(tmp_path / 'src'), 1, logger=None)(state, 7, 0)
    before = {k: v.clone() for k, v in target.state_dict().items()}
    with caplog.at_level(logging.WARNING):
        path = train.finetune(target, str(tmp_path / 'src'), [r'layers\.15\.'])           # a directory: its newest checkpoint
    assert path == str(tmp_path / 'src' / '7.pth')
    after = target.state_dict()
    want = source.state_dict()
    for k in names:
        if k in head or k == absent:
            assert torch.equal(after[k], before[k]), k                            # ignored, or absent from the file: stays
        else:
            assert torch.equal(after[k], want[k]), k
    differs = [k for k in names if k not in head and k != absent and not torch.equal(before[k], want[k])]
    assert differs                                                                # (the two seeds do differ: the copy is visible)
    assert [r for r in caplog.records if absent in r.getMessage() and 'not in finetune file' in r.getMessage()]
    assert not [r for r in caplog.records if any(k in r.getMessage() for k in head)]
    train.finetune(target, path)                                                  # a file, nothing ignored
    assert all(torch.equal(target.state_dict()[k], want[k]) for k in head)


def test_scheduler_gives_the_rate_of_each_epoch_also_on_a_resumed_run():
    import train
    config = configparser.ConfigParser()
    config.read_dict({'train': {'scheduler': 'lambda optimizer: torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=[1, 2], gamma=0.1)'}})
    lr = 0.5

    def fresh():
        optimizer = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr)
        return optimizer, train.make_scheduler(config, optimizer)
    optimizer, scheduler = fresh()
    seen = []
    for epoch in range(3):
        rates = train.set_epoch(scheduler, epoch)
        assert rates == [optimizer.param_groups[0]['lr']]
        seen.append(rates[0])
        optimizer.step()
    np.testing.assert_allclose(seen, [lr, 0.1 * lr, 0.01 * lr], rtol=1e-12)
    optimizer, scheduler = fresh()                    # resumed: the first epoch it runs is 2
    np.testing.assert_allclose(train.set_epoch(scheduler, 2), [0.01 * lr], rtol=1e-12)
    np.testing.assert_allclose(train.set_epoch(scheduler, 2), [0.01 * lr], rtol=1e-12)          # asking again changes nothing
    config.remove_option('train', 'scheduler')
    assert train.make_scheduler(config, optimizer) is None


def test_check_nan_dumps_and_raises_only_for_a_nan_total(tmp_path):
    import train
    dnn = torch.nn.Linear(2, 2)
    data = dict(tensor=torch.ones(1, 3, 4, 4), size=(4, 4))
    loss = dict(foreground=torch.tensor(1.0), cls=torch.tensor(float('nan')))
    train.check_nan(str(tmp_path), dnn, 3, torch.tensor(2.5), loss, data)
    assert os.listdir(str(tmp_path)) == []
    with pytest.raises(OverflowError, match='NaN loss'):
        train.check_nan(str(tmp_path), dnn, 3, torch.tensor(float('nan')), loss, data)
    assert sorted(os.listdir(str(tmp_path / '3'))) == ['data.pth', 'model.pth']
    assert set(torch.load(str(tmp_path / '3' / 'model.pth'))) == {'weight', 'bias'}
    assert torch.equal(torch.load(str(tmp_path / '3' / 'data.pth'))['tensor'], data['tensor'])


def test_world_size_above_one_is_refused(monkeypatch, workspace):
    import train
    root, _ = workspace
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(NotImplementedError, match='WORLD_SIZE'):
        train.Train(train.make_args(['-b', '2']), cases.load_config(cases.make_config(str(root))))


def test_eval_db_rows_reload_in_the_reference_layout(tmp_path):
    ev = importlib.import_module('eval')
    path = str(tmp_path / 'sub' / 'eval.json')
    assert ev.save_db(path, dict(step=6, mean_ap=0.25, cls_ap={'cat': 0.25})) == '1'
    assert ev.save_db(path, dict(step=9, mean_ap=0.5, cls_ap={'cat': 0.5})) == '2'
    with open(path) as f:
        table = json.load(f)['_default']
    assert sorted(table) == ['1', '2'] and table['1']['step'] == 6 and table['2']['cls_ap'] == {'cat': 0.5}


# ------------------------------------------------------------------------------------------------ the loader and Eval on a cache directory
def test_training_loader_with_worker_processes(workspace):
    """`[data] workers = 2`: two epochs over the 10-picture cache in batches of 4 yield what utils.data.to_device takes, at sizes drawn from
    `[data] sizes`, with every sample of the cache in every epoch."""
    import train
    import utils
    import utils.data
    root, samples = workspace
    config = cases.load_config(cases.make_config(str(root), **{'data/workers': 2}))
    loader = train.make_loader(config, utils.get_cache_dir(config), str(root / 'model_dir'), 20, 4)
    assert loader.num_workers == 2 and len(loader) == 3
    sizes = set()
    for epoch in range(2):
        counts = []
        for batch in loader:
            for key in ('raw', 'offset', 'geom', 'size', 'swap_rb', 'normalize', 'yx_min', 'yx_max', 'cls', 'difficult'):
                assert key in batch, key
            B = batch['geom'].size(0)
            counts.append(B)
            assert tuple(batch['size']) in [(96, 96), (128, 128)]
            sizes.add(tuple(batch['size']))
            G = batch['cls'].size(1)
            assert batch['cls'].dtype == torch.int64 and tuple(batch['yx_min'].shape) == (B, G, 2) and batch['yx_min'].dtype == torch.float32
            assert batch['swap_rb'] is True and batch['normalize'] == (0.5, 1.0)
            out = utils.data.to_device(batch, 'cpu')
            assert tuple(out['tensor'].shape) == (B, 3) + tuple(batch['size']) and bool(torch.isfinite(out['tensor']).all())
            assert float(out['tensor'].min()) >= -0.5 and float(out['tensor'].max()) <= 0.5
            assert bool((batch['yx_max'] <= max(batch['size']) + 1e-3).all()) and bool((batch['yx_min'] >= -1e-3).all())
        assert sorted(counts) == [2, 4, 4]
    assert sizes <= {(96, 96), (128, 128)} and sizes


class GroundTruthDetector(object):
    """Eval's test hook: every image's valid, non-difficult ground-truth boxes come back as detections with score 1 (boxes as fractions of the
    image: no `grid`); `extra` adds one box of class `extra` with score 0.5 to every image."""

    def __init__(self, size, extra=None):
        self.size, self.extra, self.batches = size, extra, 0

    def __call__(self, data):
        self.batches += 1
        assert 'tensor' in data and tuple(data['tensor'].shape[-2:]) == self.size
        scale = torch.tensor([float(self.size[0]), float(self.size[1])]).view(1, 1, 2)
        lo, hi = data['yx_min'].float() / scale, data['yx_max'].float() / scale
        B, G = data['cls'].shape
        M = G + 1
        out = dict(yx_min=torch.zeros(B, M, 2), yx_max=torch.zeros(B, M, 2), cls=torch.zeros(B, M, dtype=torch.int64), score=torch.zeros(B, M),
                   count=torch.zeros(B, dtype=torch.int32))
        for b in range(B):
            valid = (lo[b] < hi[b]).all(-1) & (data['difficult'][b] < 1)
            n = int(valid.sum())
            out['yx_min'][b, :n], out['yx_max'][b, :n], out['cls'][b, :n], out['score'][b, :n] = lo[b][valid], hi[b][valid], data['cls'][b][valid], 1.0
            if self.extra is not None:
                out['yx_min'][b, n], out['yx_max'][b, n], out['cls'][b, n], out['score'][b, n] = lo[b][valid][0], hi[b][valid][0], self.extra, 0.5
                n += 1
            out['count'][b] = n
        return out


@pytest.mark.parametrize('metric07', [0, 1])
def test_eval_with_a_ground_truth_detector_scores_one(workspace, metric07):
    ev = importlib.import_module('eval')
    import utils
    import utils.train
    root, samples = workspace
    path = cases.make_config(str(root), **{'eval/metric07': metric07, 'eval/db': 'eval_stub%d.json' % metric07})
    config = cases.load_config(path)
    utils.train.Saver(utils.get_model_dir(config), 5, logger=None)({}, 6, 1)          # Eval reads step and epoch of the newest checkpoint
    present = sorted({int(c) for s in samples for c, d in zip(s['cls'], s['difficult']) if not d})
    absent = next(c for c in range(20) if c not in {int(c) for s in samples for c in s['cls']})
    detector = GroundTruthDetector((128, 128))
    cls_ap = ev.main(['-c', path, '-b', '4'], detector=detector)
    assert detector.batches == 3
    assert sorted(cls_ap) == present
    # perfect precision at every recall: exactly 1.0 as the area under the envelope, and exactly what the 11-point metric makes of it - the
    # reference's `ap + p / 11.` eleven times, which is 1.0000000000000002 in float64
    perfect = ev.voc_ap([1.0], [1.0], bool(metric07))
    assert perfect == (1.0 if not metric07 else sum([1 / 11.] * 11)) and abs(perfect - 1.0) < 3e-16
    assert all(ap == perfect for ap in cls_ap.values()), cls_ap
    # a wrong-class box with a lower score in every image: the classes with ground truth keep AP 1.0; the class of the box that has none is not added
    for extra in (absent, present[0]):
        again = ev.Eval(ev.make_args(['-c', path, '-b', '4']), config, detector=GroundTruthDetector((128, 128), extra=extra))()
        assert sorted(again) == present
        assert all(again[c] == perfect for c in present), again
    with open(utils.get_eval_db(config)) as f:
        table = json.load(f)['_default']
    assert sorted(table) == ['1', '2', '3']
    row = table['1']
    assert row['step'] == 6 and row['epoch'] == 1 and row['dnn'] == 'model.yolo2.Tiny' and row['size'] == '128 128' and row['mean_ap'] == perfect
    assert row['cls_ap'] == {cases.CATEGORY[c]: perfect for c in present} and isinstance(row['timestamp'], float)


# ------------------------------------------------------------------------------------------------ utils.optim.RMSprop without a GPU
def test_rmsprop_ini_lambda_evaluates():
    import train
    config = configparser.ConfigParser()
    config.read_dict({'train': {'optimizer': 'lambda params, lr: utils.optim.RMSprop(params, lr, alpha=0.99, eps=1e-8)'}})
    frozen = torch.nn.Parameter(torch.zeros(2), requires_grad=False)
    live = torch.nn.Parameter(torch.zeros(3))
    optimizer = train.make_optimizer(config, [frozen, live], 0.25)
    import utils
    assert isinstance(optimizer, utils.optim.RMSprop) and isinstance(optimizer, torch.optim.Optimizer)
    group, = optimizer.param_groups
    assert group['lr'] == 0.25 and group['alpha'] == 0.99 and group['eps'] == 1e-8 and group['momentum'] == 0 and group['centered'] is False
    assert len(group['params']) == 1 and group['params'][0] is live


@pytest.mark.parametrize('kw', [dict(), dict(momentum=0.9), dict(centered=True), dict(momentum=0.9, centered=True)])
def test_rmsprop_state_dict_has_torchs_layout(kw, monkeypatch):
    """The key sets of state_dict() equal torch.optim.RMSprop's.  The launch itself needs a GPU: here the library call is replaced by a recorder,
    which also shows what step() hands to y2_opt_rmsprop."""
    import utils
    calls = []

    class Recorder(object):
        def y2_opt_rmsprop(self, table, count, grad_avg, lr, alpha, eps, weight_decay, momentum, centered, stream):
            calls.append((count, grad_avg is not None, [bool(table[i].state2) for i in range(count)], momentum, centered))
            return 0
    monkeypatch.setattr(utils.optim._hip, 'lib', lambda: Recorder())
    monkeypatch.setattr(utils.optim._hip, 'stream', lambda: None)
    monkeypatch.setattr(utils.optim, '_check_tensor', lambda t, what: None)
    ours = [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2, 2)), torch.nn.Parameter(torch.ones(1))]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ours]
    a, b = utils.optim.RMSprop(ours, 1e-2, **kw), torch.optim.RMSprop(ref, 1e-2, **kw)
    for po, pr in list(zip(ours, ref))[:2]:          # the third parameter has no gradient: no state
        po.grad, pr.grad = torch.ones_like(po), torch.ones_like(pr)
    versions = [p._version for p in ours]
    a.step()
    b.step()
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sa['state']) == set(sb['state']) == {0, 1}
    for k in sa['state']:
        assert set(sa['state'][k]) == set(sb['state'][k])
        assert float(sa['state'][k]['step']) == float(sb['state'][k]['step']) == 1.0
    assert set(sa['param_groups'][0]) == set(sb['param_groups'][0])
    assert calls == [(2, bool(kw.get('centered')), [bool(kw.get('momentum'))] * 2, kw.get('momentum', 0), int(bool(kw.get('centered'))))]
    assert [p._version > v for p, v in zip(ours, versions)] == [True, True, False]          # _hip.wrote on the parameters that were stepped
    b.load_state_dict(sa)                              # and the two classes read each other's checkpoints
    a.load_state_dict(sb)


@pytest.mark.parametrize('kw', [dict(lr=-1.0), dict(eps=-1e-8), dict(momentum=-0.1), dict(weight_decay=-1.0), dict(alpha=-0.5)])
def test_rmsprop_refuses_what_torch_refuses(kw):
    import utils
    p = [torch.nn.Parameter(torch.zeros(2))]
    with pytest.raises(ValueError):
        torch.optim.RMSprop(p, **kw)
    with pytest.raises(ValueError):
        utils.optim.RMSprop(p, **kw)


def test_rmsprop_refuses_cpu_and_non_fp32_parameters():
    import utils
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match='GPU'):
        utils.optim.RMSprop([p]).step()
    assert float(p.detach().sum()) == 0.0
    h = torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))
    h.grad = torch.ones(4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='fp32'):
        utils.optim.RMSprop([h]).step()
