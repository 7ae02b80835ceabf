"""The JPEG decoder without a GPU: y2_jpeg_probe_host and y2_jpeg_decode_images_host (the host function shares csrc/jpeg.h with the device kernels) on
the committed fixtures - bit for bit against what Pillow's libjpeg-turbo decoded from them (tests/golden/jpeg/expected.npz) - on damaged streams, and
the Python layer (utils.data.JpegImage, read_image, Dataset, Collate, to_device on 'cpu') against the same samples fed as pixel arrays."""
import os
import pickle

import numpy as np
import pytest
import torch

import _hip
import jpeg_cases as jp
import utils.data


@pytest.fixture(scope='module')
def items():
    return jp.all_items()


@pytest.fixture(scope='module')
def batch(items):
    """The ragged batch of all fixtures, decoded once: (group, destination, status)."""
    group = jp.pack(items)
    code, dst, status = jp.host(group)
    assert code == 0
    return group, dst, status


# ---- the probe

@pytest.mark.parametrize('name', jp.NAMES)
def test_probe_accepts_supported_fixture(name):
    code, desc = jp.probe(jp.file_bytes(name))
    assert code == 0
    h, w, ncomp, hmax, vmax, restart = jp.SUPPORTED[name]
    head = jp.header(desc)
    assert head[:6] == [h, w, ncomp, hmax, vmax, restart]
    data = jp.file_bytes(name)
    assert 0 < head[6] and head[6] + head[7] + 2 == data.size and tuple(data[head[6] + head[7]:]) == (0xFF, 0xD9)          # the scan runs up to EOI


@pytest.mark.parametrize('name', jp.UNSUPPORTED)
def test_probe_answers_not_supported(name):
    code, desc = jp.probe(jp.file_bytes(name))
    assert code == jp.ENOSUP and not desc.any()


def find(data, marker):
    at = bytes(data).find(bytes([0xFF, marker]))
    assert at >= 0
    return at


def test_probe_refuses_what_is_no_jpeg_or_contradicts_itself():
    good = jp.file_bytes('c420_17x13')
    assert jp.probe(good)[0] == 0
    cases = {'text': np.frombuffer(b'not a JPEG file, just some text of a similar length ....', np.uint8), 'empty': np.zeros(0, np.uint8),
             'png': np.frombuffer(b'\x89PNG\r\n\x1a\n' + bytes(40), np.uint8), 'soi only': good[:2], 'cut in the headers': good[:100]}
    sof, dht, sos, dqt = (find(good, m) for m in (0xC0, 0xC4, 0xDA, 0xDB))
    zero_height, zero_width = good.copy(), good.copy()
    zero_height[sof + 5:sof + 7] = 0
    zero_width[sof + 7:sof + 9] = 0
    cases.update({'zero height': zero_height, 'zero width': zero_width})
    oversubscribed = good.copy()
    oversubscribed[dht + 5] = 3          # three codes of one bit
    cases['huffman counts over-subscribe'] = oversubscribed
    long_segment = good.copy()
    long_segment[dqt + 2:dqt + 4] = (0xFF, 0xF0)
    cases['segment length past the end'] = long_segment
    table_id = good.copy()
    table_id[sof + 12] = 7          # quantisation table 7 of component 0
    cases['quantisation table id'] = table_id
    undefined = good.copy()
    undefined[dqt + 4] = 0x03          # the first table defined becomes table 3: table 0 is never defined
    cases['undefined table'] = undefined
    bad_scan = good.copy()
    bad_scan[sos + 2 + 2 + 1 + 6 + 1] = 62          # Se
    cases['spectral selection'] = bad_scan
    for what, data in cases.items():
        code, desc = jp.probe(data)
        assert code == jp.EINVAL, what
        assert not desc.any(), what
    sampling = good.copy()
    sampling[sof + 11] = 0x12          # luma 1 x 2
    sixteen = good.copy()
    sixteen[dqt + 4] |= 0x10          # a 16-bit table
    twelve = good.copy()
    twelve[sof + 4] = 12
    for what, data in (('1 x 2 sampling', sampling), ('16-bit table', sixteen), ('12-bit samples', twelve)):
        assert jp.probe(data)[0] == jp.ENOSUP, what


def test_probe_reads_nothing_outside_the_bytes():
    """Every prefix of a file, handed over as a buffer of exactly that length at the END of an allocation followed by other values: the answer never
    depends on what follows."""
    good = jp.file_bytes('c420_rst_40x56')
    for n in list(range(0, 700, 7)) + [good.size - 1, good.size]:
        a, b = np.concatenate([good[:n], np.full(64, 0xFF, np.uint8)]), np.concatenate([good[:n], np.zeros(64, np.uint8)])
        da, db = np.zeros(jp.DESC_BYTES, np.uint8), np.zeros(jp.DESC_BYTES, np.uint8)
        ra, rb = (_hip.lib().y2_jpeg_probe_host(x.ctypes.data, n, d.ctypes.data) for x, d in ((a, da), (b, db)))
        assert ra == rb and np.array_equal(da, db), n


# ---- the host decoder

@pytest.mark.parametrize('name', jp.NAMES)
def test_host_decode_equals_pillow(name):
    data = jp.file_bytes(name)
    group = jp.pack([(data, jp.probe(data)[1])])
    code, dst, status = jp.host(group)
    assert code == 0 and status.tolist() == [0]
    np.testing.assert_array_equal(jp.image(group, dst, 0), jp.expected()[name])
    assert (jp.outside(group, dst) == jp.CANARY).all()


def test_ragged_batch_writes_only_its_images(batch):
    group, dst, status = batch
    assert status.tolist() == [0] * len(jp.NAMES)
    for b, name in enumerate(jp.NAMES):
        np.testing.assert_array_equal(jp.image(group, dst, b), jp.expected()[name], err_msg=name)
    rest = jp.outside(group, dst)
    assert rest.size > 0 and (rest == jp.CANARY).all()


def test_b0_touches_nothing():
    group = jp.pack([])
    assert _hip.lib().y2_jpeg_decode_images_host(None, 0, None, None, None, 0, None, None, None, 0, None, 0) == 0
    assert jp.host(dict(group, dst_bytes=16))[0] == 0


def damaged_batch(items, k, data, desc):
    """The ragged batch with image k replaced by a damaged file; its neighbours are whole."""
    damaged = list(items)
    damaged[k] = (data, desc)
    return jp.pack(damaged)


def check_damaged(group, k, nonzero=True):
    code, dst, status = jp.host(group)
    assert code == 0
    assert 0 <= status[k] <= 4 and (status[k] != 0 or not nonzero)
    assert [s for b, s in enumerate(status.tolist()) if b != k] == [0] * (len(jp.NAMES) - 1)
    for b, name in enumerate(jp.NAMES):
        if b != k:
            np.testing.assert_array_equal(jp.image(group, dst, b), jp.expected()[name], err_msg=name)
    assert (jp.outside(group, dst) == jp.CANARY).all()
    again = jp.host(group)
    np.testing.assert_array_equal(again[1], dst)          # what a damaged stream leaves is deterministic
    return int(status[k])


@pytest.mark.parametrize('name', jp.NAMES)
def test_truncated_inside_the_scan(items, name):
    k = jp.NAMES.index(name)
    data = items[k][0]
    start, length = jp.header(items[k][1])[6:8]
    for cut in sorted({0, 1, length // 3, length // 2, length - 1}):
        short = data[:start + cut].copy()
        code, desc = jp.probe(short)
        assert code == 0, cut          # the headers are whole: the probe accepts, the decoder reports
        status = check_damaged(damaged_batch(items, k, short, desc), k)
        assert status in (1, 2), (cut, status)          # the stream ended early (where an interval ends: as a missing restart marker)


@pytest.mark.parametrize('name', jp.NAMES)
def test_one_changed_byte_inside_the_scan(items, name):
    """One byte of the scan changed, the intact file's descriptor.  A byte set to FF in front of a byte that is neither 00 nor a restart number forms a
    marker: everything from there on is missing, which the decoder MUST report (the stream up to it is the intact one and needs that byte).  A byte
    XORed with FF is reported only where the damage does not heal: Huffman streams resynchronise, and a stream that takes the same number of bits is
    a valid stream of another picture (measured on these fixtures: between 0.4 % and 70 % of the positions give status 0).  Either way: return code 0,
    a status in range, the neighbours whole, nothing outside the image written."""
    k = jp.NAMES.index(name)
    data, desc = items[k]
    start, length = jp.header(desc)[6:8]
    at = next(i for i in range(length // 2, -1, -1) if data[start + i + 1] not in (0x00, 0xFF) and not 0xD0 <= data[start + i + 1] <= 0xD7 and data[start + i] != 0xFF)
    marker = data.copy()
    marker[start + at] = 0xFF
    assert check_damaged(damaged_batch(items, k, marker, desc), k) in (1, 2)
    for i in sorted({0, length // 4, length // 2, length - 1}):
        flipped = data.copy()
        flipped[start + i] ^= 0xFF
        check_damaged(damaged_batch(items, k, flipped, desc), k, nonzero=False)


def test_restart_marker_missing_or_out_of_order(items):
    k = jp.NAMES.index('c420_rst_40x56')
    data, desc = items[k]
    start, length = jp.header(desc)[6:8]
    first = start + bytes(data[start:]).find(b'\xff\xd0')
    wrong = data.copy()
    wrong[first + 1] = 0xD3          # the first marker carries the wrong number
    assert check_damaged(damaged_batch(items, k, wrong, desc), k) == 2
    gone = np.concatenate([data[:first], data[first + 2:]])          # the first marker removed
    code, desc2 = jp.probe(gone)
    assert code == 0
    assert check_damaged(damaged_batch(items, k, gone, desc2), k) == 2
    no_interval = desc.copy()
    no_interval[:32].view(np.int32)[5] = 0          # the stream has markers the record does not announce
    assert check_damaged(damaged_batch(items, k, data, no_interval), k) != 0


def test_host_function_checks_the_tables_first(batch, items):
    group = batch[0]
    cases = {}
    geom = group['geom'].copy()
    geom[3, 2] += 1
    cases['width differs from the record'] = dict(geom=geom)
    geom = group['geom'].copy()
    geom[5, 0] = 3 * geom[5, 2] - 1
    cases['stride below 3 w'] = dict(geom=geom)
    offset = group['dst_offset'].copy()
    offset[-1] += 32
    cases['last image past dst_bytes'] = dict(dst_offset=offset)
    offset = group['dst_offset'].copy()
    offset[0] = -1
    cases['negative offset'] = dict(dst_offset=offset)
    offset = group['src_offset'].copy()
    offset[-1] = group['src'].size - 10
    cases['file past src_bytes'] = dict(src_offset=offset)
    cases['scratch too small'] = dict(ws_bytes=group['ws_bytes'] - 16 * group['B'])
    desc = group['desc'].copy()
    desc[2, :32].view(np.int32)[3] = 3          # luma sampling 3
    cases['record is none'] = dict(desc=desc)
    for what, change in cases.items():
        code, dst, status = jp.host(group, **change)
        assert code == jp.EINVAL, what
        assert (dst == jp.CANARY).all() and (status == -7).all(), what
    assert _hip.lib().y2_jpeg_workspace_bytes(desc.ctypes.data, group['B']) == jp.EINVAL
    assert _hip.lib().y2_jpeg_workspace_bytes(group['desc'].ctypes.data, group['B']) == group['ws_bytes']


# ---- the Python layer

def test_jpeg_image_stands_in_for_the_array():
    for name in jp.NAMES:
        image = utils.data.probe_jpeg(jp.file_bytes(name))
        want = jp.expected()[name]
        assert isinstance(image, utils.data.JpegImage) and image.shape == want.shape and image.ndim == 3 and image.dtype == np.uint8
        np.testing.assert_array_equal(image.decode(), want)
        again = pickle.loads(pickle.dumps(image))          # samples cross the worker boundary pickled
        assert again.shape == image.shape and np.array_equal(again.data, image.data) and np.array_equal(again.desc, image.desc)
    assert utils.data.probe_jpeg(jp.file_bytes('prog_48x40')) is None and utils.data.probe_jpeg(np.zeros(0, np.uint8)) is None


def test_read_image_and_dataset(tmp_path):
    image = utils.data.read_image(jp.path('c422_33x47'))
    assert isinstance(image, utils.data.JpegImage) and image.shape == (33, 47, 3)
    samples = [dict(path=jp.path(name), yx_min=np.zeros((2, 2), np.float32), yx_max=np.ones((2, 2), np.float32), cls=np.array([0, 3], np.int64),
                    difficult=np.zeros(2, np.uint8)) for name in jp.NAMES] + [dict(path=str(tmp_path / 'missing.jpg'), cls=np.array([1], np.int64))]
    seen = []
    ds = utils.data.Dataset(samples, transform=lambda data: seen.append(data['image']) or data, one_hot=4, dir=str(tmp_path / 'kept'))
    assert len(ds) == len(samples)
    for k, name in enumerate(jp.NAMES):
        data = ds[k]
        assert isinstance(data['image'], utils.data.JpegImage) and seen[-1] is data['image']
        assert data['size'].tolist() == list(jp.SUPPORTED[name][:2])
        assert data['cls'].dtype == np.float32 and data['cls'].tolist() == [[1, 0, 0, 0], [0, 0, 0, 1]]
        assert 'image' not in samples[k]          # a deep copy: the cached sample is untouched
    with pytest.raises(Exception):
        ds[len(samples) - 1]
    with open(tmp_path / 'kept' / 'utils.data.Dataset.pkl', 'rb') as f:
        assert pickle.load(f)['path'].endswith('missing.jpg')


def test_read_image_on_the_host_matches_the_golden_pixels():
    """Files the device does not take, and device_decode=False: cv2.imread, or Pillow with the Exif orientation applied as cv2 would."""
    try:
        import cv2  # noqa: F401
    except ImportError:
        pytest.importorskip('PIL')
    for name, key in (('prog_48x40', 'prog_48x40'), ('exif6_20x20', 'exif6_20x20.oriented')):
        image = utils.data.read_image(jp.path(name))
        assert isinstance(image, np.ndarray)
        np.testing.assert_array_equal(image, jp.expected()[key])
    image = utils.data.read_image(jp.path('c420_17x13'), device_decode=False)
    assert isinstance(image, np.ndarray)
    np.testing.assert_array_equal(image, jp.expected()['c420_17x13'])
    turned = [utils.data._orient(np.arange(6).reshape(2, 3), k).tolist() for k in range(1, 9)]
    assert turned == [[[0, 1, 2], [3, 4, 5]], [[2, 1, 0], [5, 4, 3]], [[5, 4, 3], [2, 1, 0]], [[3, 4, 5], [0, 1, 2]],
                      [[0, 3], [1, 4], [2, 5]], [[3, 0], [4, 1], [5, 2]], [[5, 2], [4, 1], [3, 0]], [[2, 5], [1, 4], [0, 3]]]


TODAY = {'plain': {'yx_min', 'yx_max', 'cls', 'difficult', 'raw', 'offset', 'geom', 'size', 'swap_rb', 'normalize'}}
TODAY['rotated'] = TODAY['plain'] | {'src_offset', 'src_geom', 'warp', 'rot_bytes', 'rot_size'}
TODAY['jittered'] = TODAY['rotated'] | {'jitter', 'hsv_tab', 'lut_b'}
JPEG_KEYS = {'jpeg', 'jpeg_offset', 'jpeg_desc', 'jpeg_index', 'jpeg_dst', 'jpeg_geom', 'jpeg_ws_bytes', 'raw_bytes'}


@pytest.mark.parametrize('mode', ['plain', 'rotated', 'jittered'])
def test_pipeline_equals_the_pixel_arrays(golden, mode):
    g = golden('collate')
    pixels = jp.make_batch(g, 'pixels', mode)
    assert set(pixels) == TODAY[mode]          # a batch without a JpegImage has exactly today's keys
    want = utils.data.to_device(pixels, 'cpu')
    assert 'jpeg_status' not in want
    for kind in ('jpeg', 'mixed'):
        batch = jp.make_batch(g, kind, mode)
        assert set(batch) == TODAY[mode] | JPEG_KEYS
        n = len(jp.PIPELINE_NAMES) if kind == 'jpeg' else (len(jp.PIPELINE_NAMES) + 1) // 2
        assert batch['jpeg_desc'].shape == (n, jp.DESC_BYTES) and batch['jpeg_index'].tolist() == list(range(0, len(jp.PIPELINE_NAMES), 1 if kind == 'jpeg' else 2))
        host_bytes = sum(jp.expected()[name].size for k, name in enumerate(jp.PIPELINE_NAMES) if kind == 'mixed' and k % 2)
        assert batch['raw'].numel() == host_bytes < batch['raw_bytes']          # only the host-decoded pixels exist on the host
        for key in ('yx_min', 'yx_max', 'cls', 'difficult'):
            assert torch.equal(batch[key], pixels[key])
        launches = _hip.LAUNCHES[0]
        res = utils.data.to_device(batch, 'cpu')
        assert _hip.LAUNCHES[0] - launches == 1 + (mode != 'plain') + 1
        assert res['jpeg_status'].dtype == torch.int32 and res['jpeg_status'].tolist() == [0] * n
        assert res['raw'].numel() == batch['raw_bytes']
        assert torch.equal(res['tensor'], want['tensor']), kind
