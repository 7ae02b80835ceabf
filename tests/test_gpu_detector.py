"""detect.Detector on the MI355X: generated pictures of different sizes and aspect ratios through model.yolo2.Tiny at 64 x 64 with seeded weights, under
`resize = rescale` and `resize = fixed`, against the hand-assembled chain collate_images -> to_device -> forward_nhwc -> detect_batch ->
postprocess_batch -> to_source; a second call with other pictures goes through the cached graph."""
import configparser

import numpy as np
import pytest
import torch

import detect
import fixed_cases as fx
import model
import model.yolo2
import utils.data
from oracle import darknet as odark
from oracle import synth

pytestmark = pytest.mark.gpu

SIZES = ((48, 80), (90, 40), (64, 64))          # wide and tall (letterboxed by `fixed`, both shrunk: mode 0) and exactly the input size (mode 1, a copy)
OTHER = ((30, 31), (100, 70), (50, 120))          # one enlarged (mode 1), two shrunk


def dev():
    return torch.device('cuda', 0)


def make_config(resize, fix):
    config = configparser.ConfigParser()
    config.read_dict({'batch_norm': {'enable': '1'}, 'model': {'pretrained': '0'}, 'image': {'size': '64 64'}, 'data': {'resize': resize},
                      'transform': {'resize_test': 'transform.resize.image.Resize', 'image_test': 'transform.image.BGR2RGB',
                                    'tensor': 'torchvision.transforms.ToTensor transform.image.Normalize', 'normalize': '0.5 1'},
                      'detect': {'fix': str(fix), 'threshold': '0.05', 'threshold_cls': '0.005', 'overlap': '0.45'}})
    return config


@pytest.fixture(scope='module')
def network():
    config = make_config('rescale', 0)
    anchors = torch.from_numpy(synth.ANCHORS_VOC)
    sd = odark.init_tiny_state_dict(5, 20, seed=0, div=8, head_scale=0.25)
    dnn = model.yolo2.Tiny(model.ConfigChannels(config, sd), anchors, 20)
    dnn.load_state_dict(sd, strict=False)
    return dnn.to(dev()).eval(), anchors


def by_hand(detector, dnn, anchors, images):
    samples, batch = detector.collate(images)
    x = utils.data.to_device(batch, dev())['tensor']
    with torch.no_grad():
        feature = dnn.forward_nhwc(x)
        rows, cols = feature.shape[1:3]
        d = detect.detect_batch(feature, anchors.to(dev()), **detector.kwargs)
    results = detect.postprocess_batch(d, detector.fix, detector.kwargs['threshold_cls'], to_host=True)
    out = []
    for record, r in zip(samples, results):
        out.append(None if r is None else (detect.to_source(r[1].numpy(), record, rows, cols, 64, 64), detect.to_source(r[2].numpy(), record, rows, cols, 64, 64),
                                           r[3].numpy(), r[4].numpy()))
    return out, batch


@pytest.mark.parametrize('resize,fix', [('rescale', 0), ('fixed', 0), ('fixed', 1)])
def test_detector_equals_the_hand_assembled_chain(network, resize, fix):
    dnn, anchors = network
    detector = detect.Detector(make_config(resize, fix), dnn, anchors, dev())
    rng = np.random.RandomState(31)
    for call, sizes in enumerate((SIZES, OTHER)):          # the second call replays the graph captured by the first
        images = [fx.picture(rng, h, w) for h, w in sizes]
        got = detector(images)
        want, batch = by_hand(detector, dnn, anchors, images)
        assert ('fixed_geom' in batch) == (resize == 'fixed')
        assert len(got) == len(want) == 3 and len(detector._graphs) == 1
        for (h, w), g, t in zip(sizes, got, want):
            assert g is not None and t is not None and len(g[0]) > 0          # thresholds low enough that every picture yields detections
            for a, b in zip(g, t):
                np.testing.assert_array_equal(a, b)
            assert g[0].dtype == np.float32 and g[0].shape == g[1].shape == (len(g[2]), 2) and len(g[3]) == len(g[2])
    # the two resizes place the same cell differently on a letterboxed picture: source pixels, not canvas pixels
    record = detector.collate([np.zeros((90, 40, 3), np.uint8)])[0][0]
    corner = detect.to_source(np.array([[2.0, 2.0]], np.float32), record, 2, 2, 64, 64)
    np.testing.assert_allclose(corner, [[90, 40]] if resize == 'rescale' else [[90, 90]], rtol=1e-6)
