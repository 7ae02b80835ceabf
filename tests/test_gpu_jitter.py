"""y2_collate_jitter_images on the MI355X against y2_collate_jitter_images_host (bit for bit, on the case groups of jitter_cases.py, one launch per
group, the whole sentinel-padded buffer compared), and utils.data.to_device with a jittered batch on the device against its CPU path."""
import numpy as np
import pytest
import torch

import _hip
import collate_cases as cc
import jitter_cases as jc
import rotate_cases as rc
import utils.data

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def groups():
    return jc.groups()


def device(g):
    """One y2_collate_jitter_images launch into a sentinel-filled buffer; returns the whole buffer on the host."""
    B = len(g['geom'])
    buf = torch.full((B * 3 * g['H'] * g['W'] + 2 * jc.PAD,), float(jc.SENTINEL), dtype=torch.float32, device=dev())
    t = [None if g[k] is None else torch.from_numpy(np.ascontiguousarray(g[k]).reshape(-1)).to(dev()) for k in ('src', 'offset', 'geom', 'jitter', 'hsv_tab', 'lut')]
    p = lambda x: x.data_ptr() if x is not None and x.numel() else None
    code = _hip.lib().y2_collate_jitter_images(*[p(x) for x in t], B, g['H'], g['W'], g['flags'], buf.data_ptr() + 4 * (jc.PAD + g['shift']), _hip.stream())
    assert code == 0
    return buf.cpu().numpy()


@pytest.mark.parametrize('name', jc.GROUP_NAMES)
def test_device_equals_host(groups, name):
    code, want = jc.host(groups[name])
    assert code == 0
    np.testing.assert_array_equal(device(groups[name]), want)          # the tensor, and every sentinel around it


@pytest.mark.parametrize('rotated', [False, True])
def test_to_device_equals_the_cpu_path(golden, rotated):
    _, batch = jc.make_batch(golden('collate'), seed=2, rotated=rotated)
    assert ('warp' in batch) == rotated and 'jitter' in batch
    H, W = batch['size']
    rot_cpu = torch.full((batch.get('rot_bytes', 0) + 100,), int(rc.SENTINEL), dtype=torch.uint8)
    want = utils.data.to_device(batch, 'cpu', rot=rot_cpu)
    launches = _hip.LAUNCHES[0]
    res = utils.data.to_device(batch, dev())
    assert _hip.LAUNCHES[0] - launches == (2 if rotated else 1)
    assert res['tensor'].device == dev() and all(v.device == dev() for v in res.values() if torch.is_tensor(v))
    assert torch.equal(res['tensor'].cpu(), want['tensor'])
    # a batch that already is on the device (no host tables to check), on a non-default stream, into the caller's buffers
    on_dev = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in batch.items()}
    buf = torch.full((5, 3, H, W), float(cc.SENTINEL), device=dev())
    rot = torch.full((batch.get('rot_bytes', 0) + 100,), int(rc.SENTINEL), dtype=torch.uint8, device=dev())
    s = torch.cuda.Stream(device=dev())
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        res2 = utils.data.to_device(on_dev, out=buf, rot=rot)
    s.synchronize()
    assert res2['tensor'] is buf and res2['raw'] is on_dev['raw'] and (res2.get('rot') is rot) == rotated
    assert torch.equal(buf.cpu(), want['tensor'])
    assert torch.equal(rot.cpu(), rot_cpu)          # the intermediate too, the bytes it leaves alone included; untouched without rotation
    # pinned source: the non-blocking copies are ordered in front of the launches
    pinned = {k: (v.pin_memory() if torch.is_tensor(v) else v) for k, v in batch.items()}
    assert torch.equal(utils.data.to_device(pinned, dev())['tensor'].cpu(), want['tensor'])


def test_unjittered_batch_makes_no_jitter_launch(golden, monkeypatch):
    _, batch = jc.make_batch(golden('collate'), rotated=False, sequence='transform.image.BGR2RGB')
    _, today = rc.make_batch(golden('collate'), rotated=False)
    assert 'jitter' not in batch
    calls = []
    lib = _hip.lib()
    real = lib.y2_collate_jitter_images
    monkeypatch.setattr(lib, 'y2_collate_jitter_images', lambda *a: calls.append(a) or real(*a))
    launches = _hip.LAUNCHES[0]
    res = utils.data.to_device(batch, dev())
    assert _hip.LAUNCHES[0] - launches == 1 and not calls
    assert torch.equal(res['tensor'].cpu(), utils.data.to_device(today, 'cpu')['tensor'])
