"""CPU-side checks of the DenseNet plugin boundary (model.densenet, reference model/densenet.py:29-117): plugin resolution, the
state_dict layout of the reference for densenet121 and for the narrow constructor arguments of the fixture (tests/golden/densenet.npz,
tools/make_golden_densenet.py), the refusals, no CPU fallback, the new library symbols."""
import collections
import configparser
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import synth

import _hip
import model
import model.densenet
import utils

NARROW = dict(growth_rate=16, block_config=(2, 4, 4, 2), num_init_features=32, bn_size=2)


def unpack(z, group):
    """name -> array of one concatenated group of the fixture: 'sd' (with zero num_batches_tracked), 'grad' or 'run'."""
    keys = [str(k) for k in z['keys']]
    shapes = {k: tuple(int(d) for d in s if d) for k, s in zip(keys, z['shapes'])}
    names = keys if group == 'sd' else [str(k) for k in z[group + '_keys']]
    data, out, o = z[group + '_flat'], collections.OrderedDict(), 0
    for k in names:
        if k.endswith('num_batches_tracked'):
            out[k] = np.zeros((), np.int64)
            continue
        n = int(np.prod(shapes[k]))
        out[k] = data[o:o + n].reshape(shapes[k])
        o += n
    assert o == data.size
    return out


def config(pretrained=None):
    cfg = configparser.ConfigParser()
    cfg.read_dict({'model': {'dnn': 'model.densenet.densenet121'}})
    if pretrained is not None:
        cfg.set('model', 'pretrained', pretrained)
    return cfg


def anchors():
    return torch.from_numpy(synth.ANCHORS_VOC)


def test_plugin_resolution_by_dotted_path():
    assert utils.parse_attr(config().get('model', 'dnn')) is model.densenet.densenet121
    for name in ('DenseNet', 'densenet169', 'densenet201', 'densenet161'):
        assert callable(getattr(model.densenet, name))


def test_densenet121_state_dict_matches_reference_layout(golden):
    g = golden('densenet')
    dnn = model.densenet.densenet121(model.ConfigChannels(config()), anchors(), 20)
    sd = dnn.state_dict()
    assert len(sd) == 727
    assert sum(v.numel() for v in sd.values()) == 7165750
    assert list(sd.keys()) == [str(k) for k in g['full_keys']]
    for (k, v), shape in zip(sd.items(), g['full_shapes']):
        assert list(v.shape) == [int(s) for s in shape[:v.dim()]], k
    assert sd['features.conv0.weight'].shape == (64, 3, 7, 7)
    assert sd['features.denseblock3.denselayer24.conv1.weight'].shape == (128, 992, 1, 1)
    assert sd['features.denseblock3.denselayer24.conv2.weight'].shape == (32, 128, 3, 3)
    assert sd['features.transition3.conv.weight'].shape == (512, 1024, 1, 1)
    assert sd['features.conv.weight'].shape == (125, 1024, 1, 1) and sd['features.conv.bias'].shape == (125,)
    assert all(not p.is_cuda for p in dnn.parameters())
    # reference initialisation: kaiming-normal convolutions, gamma = 1, beta = 0
    assert torch.equal(sd['features.norm5.weight'], torch.ones(1024)) and torch.equal(sd['features.transition1.norm.bias'], torch.zeros(256))


@pytest.mark.parametrize('name, features, entries', [('densenet169', 1664, 1015), ('densenet201', 1920, 1207), ('densenet161', 2208, 967)])
def test_other_depths_follow_the_reference_arguments(name, features, entries):
    dnn = getattr(model.densenet, name)(model.ConfigChannels(config()), anchors(), 20)
    sd = dnn.state_dict()
    assert sd['features.norm5.weight'].shape == (features,) and len(sd) == entries


def test_narrow_arguments_reproduce_the_fixture_and_load_strictly(golden):
    g = golden('densenet')
    dnn = model.densenet.DenseNet(model.ConfigChannels(config()), anchors(), 20, **NARROW)
    sd = dnn.state_dict()
    assert len(sd) == 175 and sum(v.numel() for v in sd.values()) == 113106
    assert list(sd.keys()) == [str(k) for k in g['keys']]
    for (k, v), shape in zip(sd.items(), g['shapes']):
        assert list(v.shape) == [int(s) for s in shape[:v.dim()]], k
    res = dnn.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in unpack(g, 'sd').items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert [len(b) for b, _ in dnn.blocks()] == [2, 4, 4, 2] and [t is not None for _, t in dnn.blocks()] == [True, True, True, False]


def test_refusals():
    with pytest.raises(NotImplementedError, match='drop_rate'):
        model.densenet.DenseNet(model.ConfigChannels(config()), anchors(), 20, drop_rate=0.2)
    with pytest.raises(RuntimeError, match='load_state_dict'):
        model.densenet.densenet121(model.ConfigChannels(config('1')), anchors(), 20)


def test_no_cpu_fallback_and_no_torch_operators_in_the_product_path():
    dnn = model.densenet.DenseNet(model.ConfigChannels(config()), anchors(), 20, **NARROW).eval()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dnn(torch.zeros(1, 3, 64, 64))
    text = open(model.densenet.__file__).read()
    for word in ('F.conv2d', 'F.batch_norm', 'avg_pool2d', 'load_url', 'import torchvision'):
        assert word not in text, word


def test_preactivation_entry_points_are_declared_exported_and_bound():
    if not os.path.exists(_hip.LIB_PATH):
        _hip.build()
    text = open(os.path.join(ROOT, 'include', 'yolo2_hip.h')).read()
    L = _hip.lib()
    for name in ('y2_preact_conv1x1_fwd', 'y2_preact_fwd', 'y2_preact_bwd'):
        assert name + '(' in text and name in _hip.SIGNATURES and hasattr(ctypes.CDLL(_hip.LIB_PATH), name), name
    assert L.y2_abi_version() == 2
    # argument checks happen before anything touches a device
    assert L.y2_preact_conv1x1_fwd(None, None, None, None, 0.0, None, None, 0.0, None, None, 1, 8, 8, 64, 64, 128, 128, 0, 0, None) == -1
    assert L.y2_preact_fwd(None, None, None, 0.0, None, 1, 8, 8, 64, 64, 64, 0, None) == -1
    assert L.y2_preact_bwd(None, None, None, 0.0, None, None, None, None, 64, None, None, 64, 0, 1, 8, 8, 64, 64, 0, 1, None) == -1
    # (bad shapes with non-null pointers: an odd map cannot be pooled, a pixel stride below the channel count, an output slice past ldy)
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.y2_preact_conv1x1_fwd(p, p, None, None, 0.0, None, None, 0.0, p, None, 1, 7, 8, 64, 64, 128, 128, 0, 1, None) == -1
    assert L.y2_preact_conv1x1_fwd(p, p, None, None, 0.0, None, None, 0.0, p, None, 1, 8, 8, 64, 60, 128, 128, 0, 0, None) == -1
    assert L.y2_preact_conv1x1_fwd(p, p, None, None, 0.0, None, None, 0.0, p, None, 1, 8, 8, 64, 64, 128, 128, 4, 0, None) == -1


def test_fixture_is_consistent(golden):
    g = golden('densenet')
    x96 = synth.images(2, 96, seed=1)
    assert np.array_equal(x96.reshape(-1)[:64].numpy(), g['x96_head'])
    assert g['train_out_fp64'].shape == (2, 125, 3, 3) and g['eval_x64x96_fp64'].shape == (1, 125, 2, 3)
    grads, run = unpack(g, 'grad'), unpack(g, 'run')
    assert len(grads) == 88 and len(run) == 58 and g['gfloor'].shape == (88,) and g['rfloor'].shape == (58,)
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'densenet.npz')) < (1 << 20)
