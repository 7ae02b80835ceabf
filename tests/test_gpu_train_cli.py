"""GPU tests of the train.py and eval.py command lines on a cache directory the test draws itself (tests/train_cli_cases.py): model.yolo2.Tiny,
inputs of 96x96 and 128x128, no autotuning, no loader workers (tests/test_train_cli_cpu.py runs the loader with workers)."""
import importlib
import json
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the application on sys.path)

import train_cli_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def no_autotune():
    import _hip
    was = _hip.AUTOTUNE
    _hip.AUTOTUNE = False          # Y2_AUTOTUNE=0: the static algorithm preferences, nothing is timed
    yield
    _hip.AUTOTUNE = was


def scalars(model_dir, run):
    with open(os.path.join(model_dir, run, 'scalars.jsonl')) as f:
        return [json.loads(line) for line in f]


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """`train.py -b 4 -e 2 -q` on the 10-picture cache (3 batches x 2 epochs), then once more with `-e 3` and `[save] keep = 1`."""
    import train
    import utils
    root = str(tmp_path_factory.mktemp('train_cli_gpu'))
    cases.make_cache(root)
    path = cases.make_config(root)
    model_dir = utils.get_model_dir(cases.load_config(path))
    out = dict(root=root, path=path, model_dir=model_dir)
    out['step_a'] = train.main(['-c', path, '-b', '4', '-e', '2', '-q', '-r', 'run0'])
    out['files_a'] = sorted(os.listdir(model_dir))
    with open(os.path.join(model_dir, '6.epoch')) as f:
        out['epoch_a'] = f.read()
    out['state_a'] = torch.load(os.path.join(model_dir, '6.pth'), map_location='cpu')
    out['rows_a'] = scalars(model_dir, 'run0')
    out['step_b'] = train.main(['-c', path, '-m', 'save/keep=1', '-b', '4', '-e', '3', '-q', '-r', 'run1'])
    out['files_b'] = sorted(os.listdir(model_dir))
    out['rows_b'] = scalars(model_dir, 'run1')
    return out


def test_two_epochs_write_the_checkpoint_the_ini_and_the_scalars(trained):
    import filelock
    import model
    import utils
    assert trained['step_a'] == 6
    assert '6.pth' in trained['files_a'] and '6.epoch' in trained['files_a'] and trained['epoch_a'] == '1'
    config = cases.load_config(trained['path'])
    anchors = torch.from_numpy(utils.get_anchors(config)).contiguous()
    dnn = utils.parse_attr(config.get('model', 'dnn'))(model.ConfigChannels(config), anchors, 20)
    assert list(trained['state_a']) == list(dnn.state_dict())
    assert all(not v.is_cuda for v in trained['state_a'].values())
    assert all(bool(torch.isfinite(v.float()).all()) for v in trained['state_a'].values())
    written = cases.load_config(trained['model_dir'] + '.ini')
    assert written.get('model', 'dnn') == 'model.yolo2.Tiny' and written.get('data', 'sizes') == '96,96 128,128'
    lock = filelock.FileLock(os.path.join(trained['model_dir'], 'lock'), timeout=0)
    lock.acquire()
    lock.release()
    rows = trained['rows_a']
    assert [r['step'] for r in rows] == [1, 2, 3, 4, 5, 6] and [r['epoch'] for r in rows] == [0, 0, 0, 1, 1, 1]          # `[summary] scalar = 0`: a row per step
    for r in rows:
        assert set(r['loss']) == set(r['loss_hparam']) == {'foreground', 'background', 'center', 'size', 'cls'}
        assert all(np.isfinite(v) for v in r['loss'].values()) and np.isfinite(r['loss_total'])
        np.testing.assert_allclose(r['loss_hparam']['foreground'], 5 * r['loss']['foreground'], rtol=1e-6)
        np.testing.assert_allclose(sum(r['loss_hparam'].values()), r['loss_total'], rtol=1e-5)


def test_a_second_call_resumes_and_keeps_only_the_newest(trained):
    assert trained['step_b'] == 9
    assert [r['step'] for r in trained['rows_b']] == [7, 8, 9] and [r['epoch'] for r in trained['rows_b']] == [2, 2, 2]
    kept = [n for n in trained['files_b'] if n.endswith('.pth') or n.endswith('.epoch')]
    assert kept == ['9.epoch', '9.pth']
    with open(os.path.join(trained['model_dir'], '9.epoch')) as f:
        assert f.read() == '2'


def chain_by_hand(path, batch_size):
    """The evaluation the test assembles itself: the `[eval] phase` samples in file order, unshuffled, through to_device -> network ->
    detect_batch / expand_batch -> Accumulator."""
    import detect
    import model
    import utils
    import utils.data
    import utils.train
    ev = importlib.import_module('eval')
    config = cases.load_config(path)
    category = utils.get_category(config, utils.get_cache_dir(config))
    anchors = torch.from_numpy(utils.get_anchors(config)).contiguous()
    ckpt, _, _ = utils.train.load_model(utils.get_model_dir(config), logger=None)
    state_dict = torch.load(ckpt, map_location='cpu')
    dnn = utils.parse_attr(config.get('model', 'dnn'))(model.ConfigChannels(config, state_dict), anchors, len(category))
    dnn.load_state_dict(state_dict)
    dnn = dnn.eval().cuda()
    size = tuple(int(v) for v in config.get('image', 'size').split())
    samples = utils.data.load_pickles([os.path.join(utils.get_cache_dir(config), 'test.pkl')])
    dataset = utils.data.Dataset(samples)
    swap_rb, normalize = detect.image_options(config)
    collate = utils.data.Collate(detect.parse_resize(config, config.get('transform', 'resize_eval')), [size], swap_rb=swap_rb, normalize=normalize)
    acc = ev.Accumulator(config, num_cls=len(category))
    fix = config.getboolean('detect', 'fix')
    kw = dict(fix=fix, threshold=config.getfloat('detect', 'threshold'), threshold_cls=config.getfloat('detect', 'threshold_cls'), overlap=config.getfloat('detect', 'overlap'))
    for first in range(0, len(dataset), batch_size):
        data = utils.data.to_device(collate([dataset[i] for i in range(first, min(first + batch_size, len(dataset)))]))
        with torch.no_grad():
            feature = dnn.forward_nhwc(data['tensor'])
            dets = detect.expand_batch(detect.detect_batch(feature, anchors.cuda(), **kw), fix, kw['threshold_cls'])
        acc.update(data, dets, image_size=size, grid=tuple(feature.shape[1:3]))
    return acc.result()


@pytest.mark.parametrize('modify', [[], ['detect/fix=1', 'detect/threshold=0.05', 'eval/metric07=0']])
def test_eval_command_equals_the_chain_assembled_by_hand(trained, modify, tmp_path):
    import utils
    ev = importlib.import_module('eval')
    path = trained['path']
    if modify:
        config = cases.load_config(path)
        for cmd in modify:
            utils.modify_config(config, cmd)
        path = str(tmp_path / 'config.ini')
        with open(path, 'w') as f:
            config.write(f)
    db = utils.get_eval_db(cases.load_config(path))
    rows = 0
    if os.path.exists(db):
        with open(db) as f:
            rows = len(json.load(f)['_default'])
    got = ev.main(['-c', trained['path'], '-b', '4'] + (['-m'] + modify if modify else []))
    want = chain_by_hand(path, 4)
    print('eval.main: %s' % got)
    assert isinstance(got, dict) and got == want
    assert all(0.0 <= ap <= 1.0 + 1e-12 for ap in got.values())
    with open(db) as f:
        table = json.load(f)['_default']
    assert len(table) == rows + 1
    row = table[str(rows + 1)]
    assert row['step'] == 9 and row['epoch'] == 2 and row['dnn'] == 'model.yolo2.Tiny'
    assert row['cls_ap'] == {cases.CATEGORY[c]: ap for c, ap in got.items()}


def test_finetune_takes_the_backbone_and_leaves_the_head(trained, tmp_path):
    """`--finetune <model directory> -i <the head>`.  The issue's pattern, `conv\\.`, names Darknet's head; Tiny's head is `layers.15.` (RegexList
    matches at the start of a key), so that is the pattern here."""
    import train
    root = str(tmp_path)
    os.symlink(os.path.join(trained['root'], 'cache'), os.path.join(root, 'cache'))
    path = cases.make_config(root, **{'cache/category': os.path.join(trained['root'], 'cache', 'category')})
    torch.manual_seed(1234)
    t = train.Train(train.make_args(['-c', path, '-b', '4', '-e', '1', '-q', '-f', trained['model_dir'], '-i', r'layers\.15\.']), cases.load_config(path))
    file = torch.load(os.path.join(trained['model_dir'], '9.pth'), map_location='cpu')
    state = {k: v.cpu() for k, v in t.dnn.state_dict().items()}
    head = [k for k in state if k.startswith('layers.15.')]
    assert head and t.step == 0
    for k in state:
        if k in head:
            assert not torch.equal(state[k], file[k]), k
        else:
            assert torch.equal(state[k], file[k]), k
    assert next(t.inference.parameters()).is_cuda and t.inference.training


@pytest.fixture(scope='module')
def four(tmp_path_factory):
    """A cache of exactly 4 pictures: one batch per epoch."""
    root = str(tmp_path_factory.mktemp('train_cli_four'))
    cases.make_cache(root, count=4, seed=3)
    return root


OPTIMIZERS = dict(adam='lambda params, lr: utils.optim.Adam(params, lr, betas=(0.9, 0.999), eps=1e-8)',
                  rmsprop='lambda params, lr: utils.optim.RMSprop(params, lr, alpha=0.99, eps=1e-8)')


@pytest.mark.parametrize('name', list(OPTIMIZERS))
def test_twelve_steps_on_four_pictures_lower_the_loss(four, name):
    """One size, no augmentation, the whole picture (`resize_train = transform.resize.label.Resize`), the optimizer at 1e-3: the same batch twelve
    times; the total of the last step is below the first (the assertion of test_multi_scale_training_steps_with_fused_adam_and_clip)."""
    import train
    import utils
    path = cases.make_config(four, **{'model/name': 'model_' + name, 'data/sizes': '96,96', 'transform/augmentation': '',
                                      'transform/resize_train': 'transform.resize.label.Resize', 'train/optimizer': OPTIMIZERS[name]})
    assert train.main(['-c', path, '-b', '4', '-e', '12', '-q', '-lr', '1e-3', '-r', 'run']) == 12
    rows = scalars(utils.get_model_dir(cases.load_config(path)), 'run')
    totals = [r['loss_total'] for r in rows]
    print('%s: loss_total per step: %s' % (name, ' '.join('%.4f' % v for v in totals)))
    assert len(totals) == 12 and all(np.isfinite(totals))
    assert totals[-1] < totals[0], totals


def test_evaluation_during_training_keeps_the_best_model(four):
    """`[eval] secs = 0`, `first = 1`: the trainer saves and evaluates after every step; the best model and its APs land beside the model directory."""
    import train
    import utils
    path = cases.make_config(four, **{'model/name': 'model_eval', 'data/sizes': '96,96', 'eval/secs': '0', 'eval/first': '1', 'eval/db': 'eval_during.json'})
    config = cases.load_config(path)
    model_dir = utils.get_model_dir(config)
    assert train.main(['-c', path, '-b', '4', '-e', '2', '-q', '-r', 'run']) == 2
    assert os.path.exists(model_dir + '.pth') and os.path.exists(model_dir + '.pkl')
    with open(model_dir + '.pkl', 'rb') as f:
        best = pickle.load(f)
    assert isinstance(best, dict) and all(isinstance(c, int) for c in best)
    with open(utils.get_eval_db(config)) as f:
        table = json.load(f)['_default']
    assert sorted(table) == ['1', '2'] and [table[k]['step'] for k in ('1', '2')] == [1, 2]
    assert set(torch.load(model_dir + '.pth', map_location='cpu')) == set(torch.load(os.path.join(model_dir, '2.pth'), map_location='cpu'))
