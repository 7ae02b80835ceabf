"""y2_collate_images on the MI355X against y2_collate_images_host (bit for bit, on the case groups of collate_cases.py, one launch per group),
utils.data.to_device on the device, and the tensor it writes as the input of a Darknet forward."""
import configparser

import numpy as np
import pytest
import torch

import _hip
import collate_cases as cc
import utils.data
from oracle import darknet as odark
from oracle import synth
from oracle.make_golden import NARROW
from collate_cases import config_of, host, make_batch, sample

pytestmark = pytest.mark.gpu

PAD = 64          # floats of sentinel on either side of the output (256 bytes: the output itself stays 16-byte aligned)


def dev():
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def groups():
    return cc.groups()


@pytest.fixture(scope='module')
def lut():
    return cc.random_lut()


def device(src, offset, geom, lut, H, W, flags, shift=0):
    """One y2_collate_images launch into an over-allocated, sentinel-filled buffer; returns the whole buffer on the host."""
    B = len(geom)
    n = B * 3 * H * W
    buf = torch.full((n + 2 * PAD,), float(cc.SENTINEL), dtype=torch.float32, device=dev())
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev()) for a in (src, offset, geom.reshape(-1), lut)]
    p = lambda x: x.data_ptr() if x.numel() else None
    rc = _hip.lib().y2_collate_images(p(t[0]), p(t[1]), p(t[2]), p(t[3]), B, H, W, flags, buf.data_ptr() + 4 * (PAD + shift), _hip.stream())
    assert rc == 0
    return buf.cpu().numpy()


@pytest.mark.parametrize('name', ['32x32', '32x64', 'w4', 'w30', 'b1', 'b5', 'b0'])
@pytest.mark.parametrize('flags', [0, 1])
def test_device_equals_host(groups, lut, name, flags):
    src, offset, geom, H, W = groups[name]
    n = len(geom) * 3 * H * W
    _, want = host(src, offset, geom, lut, H, W, flags)
    got = device(src, offset, geom, lut, H, W, flags)
    np.testing.assert_array_equal(got[PAD:PAD + n].view(np.uint32), want[64:64 + n].view(np.uint32))
    assert (got[:PAD] == cc.SENTINEL).all() and (got[PAD + n:] == cc.SENTINEL).all()          # nothing outside [B][3][H][W] changed


def test_unaligned_output_takes_the_scalar_stores(groups, lut):
    """W % 4 == 0 but the output starts 4 bytes past a 16-byte boundary: the same values through 4-byte stores."""
    src, offset, geom, H, W = groups['b5']
    n = len(geom) * 3 * H * W
    _, want = host(src, offset, geom, lut, H, W, 1)
    got = device(src, offset, geom, lut, H, W, 1, shift=1)
    np.testing.assert_array_equal(got[PAD + 1:PAD + 1 + n].view(np.uint32), want[64:64 + n].view(np.uint32))
    assert (got[:PAD + 1] == cc.SENTINEL).all() and (got[PAD + 1 + n:] == cc.SENTINEL).all()


def test_to_device_equals_the_cpu_path(golden):
    _, batch = make_batch(golden('collate'))
    want = utils.data.to_device(batch, 'cpu')
    H, W = batch['size']
    res = utils.data.to_device(batch, dev())
    assert res['tensor'].device == dev() and all(v.device == dev() for v in res.values() if torch.is_tensor(v))
    assert torch.equal(res['tensor'].cpu(), want['tensor'])
    for key in ('yx_min', 'yx_max', 'cls', 'difficult'):
        assert res[key].dtype == batch[key].dtype and torch.equal(res[key].cpu(), batch[key])
    # a batch that already is on the device (no host tables to check), on a non-default stream, into a supplied buffer
    on_dev = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in batch.items()}
    buf = torch.full((5, 3, H, W), float(cc.SENTINEL), device=dev())
    s = torch.cuda.Stream(device=dev())
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        res2 = utils.data.to_device(on_dev, out=buf)
        res3 = utils.data.to_device(batch)          # host batch: copies and launch on the side stream
    s.synchronize()
    assert res2['tensor'] is buf and res2['raw'] is on_dev['raw']
    assert torch.equal(buf.cpu(), want['tensor']) and torch.equal(res3['tensor'].cpu(), want['tensor'])
    # pinned source: the non-blocking copies are ordered in front of the launch
    pinned = {k: (v.pin_memory() if torch.is_tensor(v) else v) for k, v in batch.items()}
    assert torch.equal(utils.data.to_device(pinned, dev())['tensor'].cpu(), want['tensor'])


def test_darknet_forward_reads_the_collated_tensor(golden):
    """The layout is what the first layer reads: the forward on the device-collated tensor equals the forward on the host function's tensor, and
    both are the fp64 oracle's forward of that tensor (2e-5 x rms, the forward tolerance of the smoke run)."""
    import model
    import model.yolo2
    import transform.resize.label
    g = golden('collate')
    rng = np.random.RandomState(4)
    samples = [sample(g, k, rng) for k in (0, 2, 13)]
    batch = utils.data.Collate(transform.resize.label.Resize(config_of(g)), [(64, 96)])(samples)
    x_host = utils.data.to_device(batch, 'cpu')['tensor']
    x_dev = utils.data.to_device(batch, dev())['tensor']
    cfg = configparser.ConfigParser()
    cfg.read_dict({'batch_norm': {'enable': '1'}})
    anchors = torch.from_numpy(synth.ANCHORS_VOC)
    sd = odark.init_state_dict(5, 20, seed=0, channels=NARROW, head_scale=1 / 8.0)
    dnn = model.yolo2.Darknet(model.ConfigChannels(cfg, sd), anchors, 20)
    dnn.load_state_dict(sd, strict=False)
    inf = model.Inference(cfg, dnn, anchors).to(dev()).eval()
    with torch.no_grad():
        a = model._inference(inf, x_dev)['feature'].cpu()
        b = model._inference(inf, x_host.to(dev()))['feature'].cpu()
        ref = odark.forward(x_host.double(), {k: v.double() for k, v in sd.items()})
    assert torch.equal(a, b)
    err = (a.double() - ref).abs().max().item() / ref.pow(2).mean().sqrt().item()
    print('forward error %.2e x rms' % err)
    assert err <= 2e-5
