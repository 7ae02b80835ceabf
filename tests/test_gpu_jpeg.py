"""y2_jpeg_decode_images on the MI355X against Pillow's decode of the committed fixtures (tests/golden/jpeg/expected.npz) and against
y2_jpeg_decode_images_host - bit for bit, the whole canary-filled destination compared - and utils.data.to_device with JpegImage samples on the device
against the same samples fed as pixel arrays.  Well-formed streams only: the damaged ones are the host function's (test_jpeg_cpu.py), which runs the
same csrc/jpeg.h."""
import numpy as np
import pytest
import torch

import _hip
import jpeg_cases as jp
import utils.data

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def items():
    return jp.all_items()


def device(g):
    """One y2_jpeg_decode_images launch into a canary-filled destination; returns (destination bytes, status) on the host."""
    dst = torch.full((g['dst_bytes'],), jp.CANARY, dtype=torch.uint8, device=dev())
    status = torch.full((max(g['B'], 1),), -7, dtype=torch.int32, device=dev())
    ws = torch.empty(max(g['ws_bytes'], 16), dtype=torch.uint8, device=dev())
    t = {k: torch.from_numpy(np.ascontiguousarray(g[k])).to(dev()) for k in ('src', 'src_offset', 'desc', 'dst_offset', 'geom')}
    p = lambda x: x.data_ptr() if x.numel() else None
    code = _hip.lib().y2_jpeg_decode_images(p(t['src']), t['src'].numel(), p(t['src_offset']), p(t['desc']), dst.data_ptr(), dst.numel(), p(t['dst_offset']),
                                            p(t['geom']), ws.data_ptr(), g['ws_bytes'], status.data_ptr(), g['B'], _hip.stream())
    assert code == 0
    return dst.cpu().numpy(), status.cpu().numpy()[:g['B']]


def check(group, names):
    dst, status = device(group)
    code, want, want_status = jp.host(group)
    assert code == 0
    assert status.tolist() == [0] * len(names) == want_status.tolist()
    for b, name in enumerate(names):
        np.testing.assert_array_equal(jp.image(group, dst, b), jp.expected()[name], err_msg=name)
    np.testing.assert_array_equal(dst, want)          # the images, and every canary around and between them


@pytest.mark.parametrize('name', jp.NAMES)
def test_fixture_alone(items, name):
    check(jp.pack([items[jp.NAMES.index(name)]]), [name])


def test_ragged_batch_in_one_launch(items):
    check(jp.pack(items), jp.NAMES)


def test_b0_launches_nothing():
    group = dict(jp.pack([]), dst_bytes=64)
    dst, status = device(group)
    assert (dst == jp.CANARY).all() and status.size == 0


@pytest.mark.parametrize('mode', ['plain', 'rotated', 'jittered'])
def test_to_device_equals_the_pixel_arrays(golden, mode):
    g = golden('collate')
    want = utils.data.to_device(jp.make_batch(g, 'pixels', mode), 'cpu')['tensor']
    for kind in ('jpeg', 'mixed'):
        batch = jp.make_batch(g, kind, mode)
        launches = _hip.LAUNCHES[0]
        res = utils.data.to_device(batch, dev())
        assert _hip.LAUNCHES[0] - launches == 1 + (mode != 'plain') + 1
        assert res['tensor'].device == dev() and all(v.device == dev() for v in res.values() if torch.is_tensor(v))
        assert res['jpeg_status'].tolist() == [0] * batch['jpeg_desc'].size(0)
        assert torch.equal(res['tensor'].cpu(), want), kind
        # pinned source, a non-default stream: the copies are ordered in front of the launches
        pinned = {k: (v.pin_memory() if torch.is_tensor(v) and v.numel() else v) for k, v in batch.items()}
        s = torch.cuda.Stream(device=dev())
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            res2 = utils.data.to_device(pinned, dev())
        s.synchronize()
        assert torch.equal(res2['tensor'].cpu(), want), kind
