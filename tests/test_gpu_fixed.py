"""y2_fixed_images on the MI355X against y2_fixed_images_host (bit for bit, on the case groups of fixed_cases.py, one launch per group, the sentinels
around `out` intact), and utils.data.to_device with a `fixed` batch on the device against its CPU path."""
import numpy as np
import pytest
import torch

import _hip
import fixed_cases as fx
import jpeg_cases as jp
import transform.resize.image
import utils.data

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def groups():
    return fx.groups()


def device(g):
    """One y2_fixed_images launch into a sentinel-filled buffer (PAD floats on either side); returns the whole buffer on the host."""
    buf = torch.full((fx.numel(g) + 2 * fx.PAD,), float(fx.SENTINEL), dtype=torch.float32, device=dev())
    assert buf.data_ptr() % 16 == 0
    t = [torch.from_numpy(np.ascontiguousarray(g[k]).reshape(-1)).to(dev()) for k in ('src', 'offset', 'geom', 'inv', 'lut')]
    p = lambda x: x.data_ptr() if x.numel() else None
    code = _hip.lib().y2_fixed_images(p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), len(g['geom']), g['H'], g['W'], g['flags'],
                                      buf.data_ptr() + 4 * (fx.PAD + g['misalign']), _hip.stream())
    assert code == 0
    return buf.cpu().numpy()


@pytest.mark.parametrize('name', fx.GROUP_NAMES)
def test_device_equals_host(groups, name):
    code, want = fx.host(groups[name])
    assert code == 0
    np.testing.assert_array_equal(device(groups[name]), want)          # every value, and every sentinel in front of and behind them


def make_batch(kind):
    """A `fixed` batch at 40 x 56 that mixes the two modes: generated pictures, or - `jpeg` - the committed JPEG fixtures left compressed beside one of them."""
    rng = np.random.RandomState(12)
    images = [fx.picture(rng, h, w) for h, w in ((37, 50), (50, 37), (20, 13), (40, 56), (90, 80))]
    if kind == 'jpeg':
        files = [utils.data.read_image(jp.path(name)) for name in ('c420_rst_40x56', 'c422_33x47', 'c420_q100_64x64', 'c420_3x4')]
        assert all(isinstance(f, utils.data.JpegImage) for f in files)
        images = files[:2] + images[:1] + files[2:]
    batch = utils.data.collate_images([dict(image=image) for image in images], transform.resize.image.Fixed(), 40, 56)
    assert sorted(set(batch['fixed_geom'][:, 3].tolist())) == [0, 1]
    return images, batch


@pytest.mark.parametrize('kind', ['pixels', 'jpeg'])
def test_to_device_equals_the_cpu_path(kind):
    images, batch = make_batch(kind)
    B, expect = len(images), 2 if kind == 'jpeg' else 1
    want = utils.data.to_device(batch, 'cpu')['tensor']
    if kind == 'jpeg':          # ... which is what the same pictures give as pixel arrays
        pixels = [image.decode() if isinstance(image, utils.data.JpegImage) else image for image in images]
        plain = utils.data.collate_images([dict(image=image) for image in pixels], transform.resize.image.Fixed(), 40, 56)
        assert torch.equal(utils.data.to_device(plain, 'cpu')['tensor'], want)
    # pageable memory
    launches = _hip.LAUNCHES[0]
    res = utils.data.to_device(batch, dev())
    assert _hip.LAUNCHES[0] - launches == expect
    assert res['tensor'].device == dev() and all(v.device == dev() for v in res.values() if torch.is_tensor(v))
    assert torch.equal(res['tensor'].cpu(), want)
    # pinned memory: the non-blocking copies are ordered in front of the launch
    pinned = {k: (v.pin_memory() if torch.is_tensor(v) and v.numel() else v) for k, v in batch.items()}
    launches = _hip.LAUNCHES[0]
    res = utils.data.to_device(pinned, dev())
    assert _hip.LAUNCHES[0] - launches == expect and torch.equal(res['tensor'].cpu(), want)
    # a batch that already is on the device (no host tables to check), on a side stream, into the caller's buffer
    on_dev = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in batch.items()}
    buf = torch.full((B, 3, 40, 56), float(fx.SENTINEL), device=dev())
    s = torch.cuda.Stream(device=dev())
    s.wait_stream(torch.cuda.current_stream())
    launches = _hip.LAUNCHES[0]
    with torch.cuda.stream(s):
        res = utils.data.to_device(on_dev, out=buf)
    s.synchronize()
    assert _hip.LAUNCHES[0] - launches == expect and res['tensor'] is buf and torch.equal(buf.cpu(), want)
    if kind == 'jpeg':
        assert res['jpeg_status'].tolist() == [0] * 4
    # the caller's `out` from host memory on the current stream
    buf.fill_(float(fx.SENTINEL))
    assert utils.data.to_device(batch, dev(), out=buf)['tensor'] is buf and torch.equal(buf.cpu(), want)


def test_bad_tables_are_refused_before_anything_is_written():
    _, batch = make_batch('pixels')
    buf = torch.full((5, 3, 40, 56), float(fx.SENTINEL), device=dev())
    bad = batch['fixed_geom'].clone()
    bad[4, 1] += 1          # one row more than the buffer holds
    launches = _hip.LAUNCHES[0]
    with pytest.raises(ValueError, match='fixed: image 4'):
        utils.data.to_device(dict(batch, fixed_geom=bad), dev(), out=buf)
    assert _hip.LAUNCHES[0] == launches and (buf == float(fx.SENTINEL)).all()
