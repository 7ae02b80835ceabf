"""CPU-side checks of the MobileNet plugin boundary (model.mobilenet, reference model/mobilenet.py:54-85): plugin resolution,
state_dict layout of the reference at default and at ConfigChannels-driven widths, no CPU fallback, the new library symbols."""
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
import model.mobilenet
import utils


def config():
    cfg = configparser.ConfigParser()
    cfg.read_dict({'model': {'dnn': 'model.mobilenet.MobileNet'}})
    return cfg


def narrow_state_dict(golden):
    g = golden('mobilenet')
    return {k: torch.from_numpy(g['sd/' + k]) for k in g['keys']}


def test_plugin_resolution_by_dotted_path():
    assert utils.parse_attr(config().get('model', 'dnn')) is model.mobilenet.MobileNet


def test_default_width_state_dict_matches_reference_layout(golden):
    g = golden('mobilenet')
    anchors = torch.from_numpy(synth.ANCHORS_VOC)
    dnn = model.mobilenet.MobileNet(model.ConfigChannels(config()), anchors, 20)
    sd = dnn.state_dict()
    assert len(sd) == 164
    assert sum(v.numel() for v in sd.values()) == 3357016
    assert list(sd.keys()) == list(g['full_keys'])
    for (k, v), shape in zip(sd.items(), g['full_shapes']):
        assert list(v.shape) == [int(s) for s in shape[:v.dim()]], k
    assert sd['layers.1.dw.conv.weight'].shape == (32, 1, 3, 3)
    assert sd['layers.14.weight'].shape == (125, 1024, 1, 1) and sd['layers.14.bias'].shape == (125,)
    assert all(not p.is_cuda for p in dnn.parameters())
    # reference initialisation: kaiming-normal convolutions, gamma = 1, beta = 0
    assert torch.equal(sd['layers.3.dw.bn.weight'], torch.ones(128)) and torch.equal(sd['layers.3.pw.bn.bias'], torch.zeros(128))


def test_narrow_widths_follow_config_channels(golden):
    g = golden('mobilenet')
    sd = narrow_state_dict(golden)
    dnn = model.mobilenet.MobileNet(model.ConfigChannels(config(), sd), torch.from_numpy(synth.ANCHORS_VOC), 20)
    res = dnn.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys
    assert all(k.endswith('num_batches_tracked') for k in res.missing_keys)
    assert list(dnn.state_dict().keys()) == list(g['keys'])
    assert dnn.layers[0].conv.weight.shape == (4, 3, 3, 3)
    assert dnn.layers[1].dw.conv.weight.shape == (4, 1, 3, 3)           # a depthwise layer's width is its input width
    assert dnn.layers[13].pw.conv.weight.shape == (128, 128, 1, 1)
    assert dnn.layers[14].weight.shape == (125, 128, 1, 1)
    assert [s for _, _, s in dnn.units()] == [1, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 2, 1]


def test_no_cpu_fallback():
    dnn = model.mobilenet.MobileNet(model.ConfigChannels(config()), torch.from_numpy(synth.ANCHORS_VOC), 20).eval()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dnn(torch.zeros(1, 3, 64, 64))
    dnn.train()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dnn(torch.zeros(1, 3, 64, 64))


def test_backward_param_order_covers_every_convolution():
    dnn = model.mobilenet.MobileNet(model.ConfigChannels(config()), torch.from_numpy(synth.ANCHORS_VOC), 20)
    order = dnn.backward_param_order()
    convs = [m.weight for m in dnn.modules() if isinstance(m, torch.nn.Conv2d)]
    assert len(order) == len(convs) == 28 and {id(p) for p in order} == {id(p) for p in convs}
    assert order[0] is dnn.layers[14].weight and order[-1] is dnn.layers[0].conv.weight
    assert order[1] is dnn.layers[13].pw.conv.weight and order[2] is dnn.layers[13].dw.conv.weight


def test_depthwise_entry_points_are_exported_and_bound():
    if not os.path.exists(_hip.LIB_PATH):
        _hip.build()
    text = open(os.path.join(ROOT, 'include', 'yolo2_hip.h')).read()
    L = _hip.lib()
    for name in ('y2_dwconv_fwd', 'y2_dwconv_dgrad', 'y2_dwconv_wgrad', 'y2_dwconv_wgrad_workspace_bytes'):
        assert name + '(' in text and name in _hip.SIGNATURES and hasattr(ctypes.CDLL(_hip.LIB_PATH), name), name
    assert L.y2_abi_version() == 2
    # argument checks happen before anything touches a device
    assert L.y2_dwconv_fwd(None, None, None, None, 0.0, None, None, 1, 8, 8, 4, 4, 4, 1, None) == -1
    assert L.y2_dwconv_dgrad(None, None, None, 1, 8, 8, 4, 4, 4, 1, None) == -1
    assert L.y2_dwconv_wgrad(None, None, None, None, 0, 1, 8, 8, 4, 4, 4, 1, None) == -1
    # the workspace query: per-workgroup partial sums of C * 9 floats, more workgroups for a larger problem, 0 for a bad shape
    small = L.y2_dwconv_wgrad_workspace_bytes(1, 13, 13, 1024, 1)
    large = L.y2_dwconv_wgrad_workspace_bytes(64, 208, 208, 32, 1)
    assert small > 0 and small % (1024 * 9 * 4) == 0
    assert large % (32 * 9 * 4) == 0 and large // (32 * 9 * 4) > small // (1024 * 9 * 4)
    assert L.y2_dwconv_wgrad_workspace_bytes(1, 13, 13, 1024, 3) == 0
    assert L.y2_dwconv_wgrad_workspace_bytes(0, 13, 13, 8, 1) == 0


def test_fixture_is_consistent(golden):
    g = golden('mobilenet')
    x96 = synth.images(2, 96, seed=1)
    assert np.array_equal(x96.reshape(-1)[:64].numpy(), g['x96_head'])
    assert g['train_out_fp64'].shape == (2, 125, 3, 3) and g['eval_x64x96_fp64'].shape == (1, 125, 2, 3)
