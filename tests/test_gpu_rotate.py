"""y2_warp_affine_images on the MI355X against y2_warp_affine_images_host (bit for bit, on the case groups of rotate_cases.py, one launch per group,
sentinels around and between the rows intact), and utils.data.to_device with rotated samples on the device against its CPU path."""
import numpy as np
import pytest
import torch

import _hip
import collate_cases as cc
import rotate_cases as rc
import utils.data

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def groups():
    return rc.groups()


def device(g):
    """One y2_warp_affine_images launch into a sentinel-filled buffer (PAD bytes on either side); returns the whole buffer on the host."""
    buf = torch.full((g['nbytes'] + 2 * rc.PAD,), int(rc.SENTINEL), dtype=torch.uint8, device=dev())
    t = [torch.from_numpy(np.ascontiguousarray(g[k]).reshape(-1)).to(dev()) for k in ('src', 'src_offset', 'src_geom', 'inv', 'dst_offset', 'dst_geom')]
    p = lambda x: x.data_ptr() if x.numel() else None
    code = _hip.lib().y2_warp_affine_images(p(t[0]), p(t[1]), p(t[2]), p(t[3]), buf.data_ptr() + rc.PAD, p(t[4]), p(t[5]),
                                            len(g['dst_geom']), g['max_h'], g['max_w'], g['fill'], _hip.stream())
    assert code == 0
    return buf.cpu().numpy()


@pytest.mark.parametrize('name', rc.GROUP_NAMES)
def test_device_equals_host(groups, name):
    code, want = rc.host(groups[name])
    assert code == 0
    np.testing.assert_array_equal(device(groups[name]), want)          # the images, and every sentinel byte around them and behind their rows


def test_to_device_equals_the_cpu_path(golden):
    _, batch = rc.make_batch(golden('collate'), seed=2)
    batch['fill'] = 0x3C78B4
    H, W = batch['size']
    rot_cpu = torch.full((batch['rot_bytes'] + 100,), int(rc.SENTINEL), dtype=torch.uint8)
    want = utils.data.to_device(batch, 'cpu', rot=rot_cpu)
    launches = _hip.LAUNCHES[0]
    res = utils.data.to_device(batch, dev())
    assert _hip.LAUNCHES[0] - launches == 2
    assert res['tensor'].device == dev() and all(v.device == dev() for v in res.values() if torch.is_tensor(v))
    assert torch.equal(res['tensor'].cpu(), want['tensor'])
    # a batch that already is on the device (no host tables to check), on a non-default stream, into the caller's buffers
    on_dev = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in batch.items()}
    buf = torch.full((5, 3, H, W), float(cc.SENTINEL), device=dev())
    rot = torch.full((batch['rot_bytes'] + 100,), int(rc.SENTINEL), dtype=torch.uint8, device=dev())
    s = torch.cuda.Stream(device=dev())
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        res2 = utils.data.to_device(on_dev, out=buf, rot=rot)
    s.synchronize()
    assert res2['tensor'] is buf and res2['rot'] is rot and res2['raw'] is on_dev['raw']
    assert torch.equal(buf.cpu(), want['tensor']) and torch.equal(rot.cpu(), rot_cpu)          # the intermediate too, the bytes it leaves alone included
    # pinned source: the non-blocking copies are ordered in front of the two launches
    pinned = {k: (v.pin_memory() if torch.is_tensor(v) else v) for k, v in batch.items()}
    assert torch.equal(utils.data.to_device(pinned, dev())['tensor'].cpu(), want['tensor'])


def test_unrotated_batch_makes_no_warp_launch(golden):
    _, batch = rc.make_batch(golden('collate'), rotated=False)
    want = utils.data.to_device(batch, 'cpu')['tensor']
    rot = torch.full((256,), int(rc.SENTINEL), dtype=torch.uint8, device=dev())
    launches = _hip.LAUNCHES[0]
    res = utils.data.to_device(batch, dev(), rot=rot)
    assert _hip.LAUNCHES[0] - launches == 1 and 'rot' not in res
    assert torch.equal(res['tensor'].cpu(), want) and (rot.cpu() == int(rc.SENTINEL)).all()
