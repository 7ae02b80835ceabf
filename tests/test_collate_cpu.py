"""The collate step on the library's HOST code: y2_collate_images_host against the numpy restatement of its contract (collate_cases.py), the
label transforms and Collate against tests/golden/collate.npz (labels and crop windows produced by the reference's own functions,
tools/make_golden_collate.py), and utils.data.to_device on 'cpu'."""
import random

import numpy as np
import pytest
import torch

import collate_cases as cc
from collate_cases import config_of, host, make_batch, sample
import transform.augmentation
import transform.resize.label
import utils
import utils.data


@pytest.fixture(scope='module')
def groups():
    return cc.groups()


@pytest.fixture(scope='module')
def lut():
    return cc.random_lut()


@pytest.mark.parametrize('name', ['32x32', '32x64', 'w4', 'w30', 'b1', 'b5', 'b0'])
@pytest.mark.parametrize('flags', [0, 1])
def test_host_equals_restatement(groups, lut, name, flags):
    src, offset, geom, H, W = groups[name]
    rc, out = host(src, offset, geom, lut, H, W, flags)
    assert rc == 0
    n = len(geom) * 3 * H * W
    want = cc.restate(src, offset, geom, lut, H, W, flags)
    np.testing.assert_array_equal(out[64:64 + n].view(np.uint32), want.reshape(-1).view(np.uint32))
    assert (out[:64] == cc.SENTINEL).all() and (out[64 + n:] == cc.SENTINEL).all()


def test_cases_cover_the_paths(groups):
    """The groups hold what they are there for: box-path images, one-axis 2:1, one-pixel windows, flips of odd and even width, padded rows, odd offsets."""
    src, offset, geom, H, W = groups['32x32']
    box = (geom[:, 5] == 2 * H) & (geom[:, 6] == 2 * W)
    assert box.sum() == 2 and ((geom[:, 5] == 2 * H) ^ (geom[:, 6] == 2 * W)).sum() == 2
    assert (geom[:, 6] == 1).any() and (geom[:, 5] == 1).any()
    assert {int(w) % 2 for w in geom[geom[:, 7] == 1, 2]} == {0, 1}
    assert (geom[:, 0] > 3 * geom[:, 2]).any()
    for g in groups.values():
        assert (g[1] % 2 == 1).all()
    assert len(groups['b0'][2]) == 0 and len(groups['b1'][2]) == 1 and len({tuple(r[1:3]) for r in groups['b5'][2]}) == 5


def test_restatement_within_one_level_of_fp64_bilinear(groups):
    """A property of the 11-bit recipe, not of the code under test: 1.0 level."""
    worst = 0.0
    for name, (src, offset, geom, H, W) in groups.items():
        if len(geom):
            worst = max(worst, np.abs(cc.levels(src, offset, geom, H, W).astype(np.float64) - cc.bilinear64(src, offset, geom, H, W)).max())
    print('worst |level - fp64 bilinear| = %.4f' % worst)
    assert worst <= 1.0


@pytest.mark.parametrize('v', [0, 1, 128, 254, 255])
def test_constant_image_gives_the_table_entry(lut, v):
    rng = np.random.RandomState(v)
    img = np.full((26, 34, 3), v, np.uint8)
    src, offset, geom = cc.pack(rng, [(img, None, 0, 0), (img, (1, 2, 20, 30), 1, 3), (img, (0, 0, 26, 34), 0, 0)])
    for H, W in ((32, 32), (13, 17)):          # bilinear for all three; (13, 17): the box mean for the whole image
        rc, out = host(src, offset, geom, lut, H, W, 1)
        assert rc == 0
        got = out[64:64 + 3 * 3 * H * W].reshape(3, 3, H, W)
        for c in range(3):
            assert (got[:, c].view(np.uint32) == lut[c, v:v + 1].view(np.uint32)).all()


def test_window_outside_the_image_is_refused_and_nothing_is_written(groups, lut):
    src, offset, geom, H, W = groups['b5']
    for col, value in ((5, 1000), (6, 1000), (3, -1), (4, -1), (5, 0), (0, 3), (7, 2)):
        bad = geom.copy()
        bad[3, col] = value          # (a LATER image: the tables are checked before the first image is written)
        rc, out = host(src, offset, bad, lut, H, W, 0)
        assert rc == -1, (col, value)
        assert (out == cc.SENTINEL).all()
        batch = dict(raw=torch.from_numpy(src), offset=torch.from_numpy(offset), geom=torch.from_numpy(bad), size=(H, W))
        with pytest.raises(ValueError, match='outside'):
            utils.data.to_device(batch, 'cpu')
    short = dict(raw=torch.from_numpy(src[:-1].copy()), offset=torch.from_numpy(offset), geom=torch.from_numpy(geom), size=(H, W))
    with pytest.raises(ValueError, match='outside'):
        utils.data.to_device(short, 'cpu')


# ---- reference semantics

def test_transforms_reproduce_the_reference_labels_and_windows(golden):
    g = golden('collate')
    config = config_of(g)
    plugin = lambda key: utils.parse_attr(config.get('transform', key))(config)          # the dotted names of config.ini resolve
    augmentation, crop, resize = plugin('augmentation'), plugin('resize_train'), plugin('resize_eval')
    assert isinstance(crop, transform.resize.label.RandomCrop) and isinstance(resize, transform.resize.label.Resize)
    for k in range(len(g['seed'])):
        data = sample(g, k)
        image = data['image']
        random.seed(int(g['seed'][k]))
        np.random.seed(int(g['seed'][k]))
        data = augmentation(data)
        data = (crop if g['crop'][k] else resize)(data, int(g['target'][k][0]), int(g['target'][k][1]))
        n = int(g['count'][k])
        assert data['yx_min'].dtype == np.float32 and data['yx_max'].dtype == np.float32
        np.testing.assert_array_equal(data['yx_min'].view(np.uint32), g['out_min'][k, :n].view(np.uint32), err_msg='sample %d' % k)
        np.testing.assert_array_equal(data['yx_max'].view(np.uint32), g['out_max'][k, :n].view(np.uint32), err_msg='sample %d' % k)
        assert tuple(int(v) for v in data['window']) == tuple(g['window'][k]) and bool(data['flip']) == bool(g['flip'][k]), k
        assert data['image'] is image and not image.any()
    assert 0 < g['flip'].sum() < len(g['flip'])
    # Rescale takes no config and is the whole-image window
    data = transform.resize.label.Rescale()(sample(g, 0), 64, 96)
    assert data['window'] == (0, 0) + tuple(g['size'][0]) and data['flip'] is False


def test_one_resize_transform_per_sample(golden):
    """After a resize transform the labels are in output coordinates: a second one (or a flip) on the same sample raises instead of going wrong."""
    g = golden('collate')
    config = config_of(g)
    for second in (transform.resize.label.Rescale(), transform.resize.label.Resize(config), transform.resize.label.RandomCrop(config)):
        data = transform.resize.label.RandomCrop(config)(sample(g, 1), 64, 64)
        with pytest.raises(ValueError, match='one resize transform'):
            second(data, 32, 32)
    with pytest.raises(ValueError, match='flip first'):
        transform.augmentation.flip_horizontally(transform.resize.label.Rescale()(sample(g, 1), 64, 64))


def test_image_without_labels_raises_like_the_reference(golden):
    config = config_of(golden('collate'))
    data = dict(image=np.zeros((20, 30, 3), np.uint8), yx_min=np.zeros((0, 2), np.float32), yx_max=np.zeros((0, 2), np.float32))
    with pytest.raises(ValueError):
        transform.resize.label.RandomCrop(config)(data, 32, 32)


def test_next_size_follows_the_reference_sequence(golden):
    g = golden('collate')
    collate = utils.data.Collate(transform.resize.label.Rescale(), [tuple(int(v) for v in s) for s in g['sizes']], maintain=int(g['maintain']))
    random.seed(int(g['size_seed']))
    got = [collate.next_size() for _ in range(len(g['size_sequence']))]
    np.testing.assert_array_equal(np.array(got), g['size_sequence'])
    assert len({tuple(s) for s in g['size_sequence']}) > 1


def test_padding_labels():
    data = dict(yx_min=np.ones((2, 2), np.float32), yx_max=np.ones((2, 2), np.float32) * 2, cls=np.array([3, 4], np.int64), difficult=np.array([1, 0], np.uint8), other=5)
    out = utils.data.padding_labels(data, 5)
    assert out['yx_min'].shape == (5, 2) and out['cls'].shape == (5,) and out['difficult'].dtype == np.uint8 and out['other'] == 5
    assert not out['yx_min'][2:].any() and not out['yx_max'][2:].any() and not out['cls'][2:].any() and out['cls'][:2].tolist() == [3, 4]


def test_collate_output_contract(golden):
    g = golden('collate')
    samples, batch = make_batch(g)
    B, N = 5, max(int(g['count'][k]) for k in (1, 4, 5, 9, 11))
    assert sorted(batch) == sorted(['yx_min', 'yx_max', 'cls', 'difficult', 'raw', 'offset', 'geom', 'size', 'swap_rb', 'normalize'])
    assert 'tensor' not in batch and 'image' not in batch
    assert batch['yx_min'].dtype == torch.float32 and tuple(batch['yx_min'].shape) == (B, N, 2) and tuple(batch['yx_max'].shape) == (B, N, 2)
    assert batch['cls'].dtype == torch.int64 and tuple(batch['cls'].shape) == (B, N)
    assert batch['difficult'].dtype == torch.uint8 and tuple(batch['difficult'].shape) == (B, N)
    assert batch['raw'].dtype == torch.uint8 and batch['raw'].dim() == 1
    assert batch['offset'].dtype == torch.int64 and tuple(batch['offset'].shape) == (B,)
    assert batch['geom'].dtype == torch.int32 and tuple(batch['geom'].shape) == (B, 8)
    assert batch['size'] == (40, 56) and batch['swap_rb'] is True and batch['normalize'] == (0.5, 1.0)
    for b, k in enumerate((1, 4, 5, 9, 11)):
        n = int(g['count'][k])
        assert not batch['yx_min'][b, n:].any() and not batch['yx_max'][b, n:].any() and not batch['cls'][b, n:].any()
        h, w = g['size'][k]
        o = int(batch['offset'][b])
        assert batch['geom'][b, :3].tolist() == [3 * w, h, w]
        np.testing.assert_array_equal(batch['raw'][o:o + 3 * h * w].numpy().reshape(h, w, 3), samples[b]['image'])      # the untouched source pixels
    assert batch['raw'].numel() == sum(3 * int(g['size'][k][0]) * int(g['size'][k][1]) for k in (1, 4, 5, 9, 11))


@pytest.mark.parametrize('normalize', [(0.5, 1.0), (0.4, 0.25), None])
def test_to_device_cpu_equals_table_of_restated_levels(golden, normalize):
    _, batch = make_batch(golden('collate'), seed=2)
    batch['normalize'] = normalize
    res = utils.data.to_device(batch, 'cpu')
    H, W = batch['size']
    lut = torch.arange(256).float().div(255)          # ToTensor, then Normalize, with the reference's own operations
    if normalize is not None:
        lut = lut.sub(torch.tensor([normalize[0]])).div(torch.tensor([normalize[1]]))
    lut = lut.view(1, 256).repeat(3, 1).numpy()
    want = cc.restate(batch['raw'].numpy(), batch['offset'].numpy(), batch['geom'].numpy(), lut, H, W, 1)
    assert res['tensor'].dtype == torch.float32 and tuple(res['tensor'].shape) == (5, 3, H, W)
    np.testing.assert_array_equal(res['tensor'].numpy().view(np.uint32), want.view(np.uint32))
    assert res['yx_min'] is batch['yx_min'] and 'tensor' not in batch          # no copy where none is needed; the input dict is left alone
    # out=: the supplied buffer is written and returned
    buf = torch.full((5, 3, H, W), float(cc.SENTINEL))
    res2 = utils.data.to_device(batch, 'cpu', out=buf)
    assert res2['tensor'] is buf and torch.equal(buf, res['tensor'])
    with pytest.raises(ValueError, match='out must be'):
        utils.data.to_device(batch, 'cpu', out=torch.empty(5, 3, H, W + 1))


def test_to_device_takes_a_level_table_and_a_list_normalize(golden):
    """`batch['lut']` replaces the ToTensor + Normalize table; `normalize` may arrive as a list (a config round trip)."""
    _, batch = make_batch(golden('collate'), seed=3)
    H, W = batch['size']
    lut = cc.random_lut(9)
    res = utils.data.to_device(dict(batch, lut=torch.from_numpy(lut)), 'cpu')
    want = cc.restate(batch['raw'].numpy(), batch['offset'].numpy(), batch['geom'].numpy(), lut, H, W, 1)
    np.testing.assert_array_equal(res['tensor'].numpy().view(np.uint32), want.view(np.uint32))
    for bad in (torch.zeros(3, 255), torch.zeros(3, 256, dtype=torch.float64), torch.zeros(256, 3).t()):
        with pytest.raises(ValueError, match='lut must be'):
            utils.data.to_device(dict(batch, lut=bad), 'cpu')
    a = utils.data.to_device(dict(batch, normalize=[0.4, 0.25]), 'cpu')['tensor']
    assert torch.equal(a, utils.data.to_device(dict(batch, normalize=(0.4, 0.25)), 'cpu')['tensor'])
    assert utils.data.level_table([0.4, 0.25], 'cpu') is utils.data.level_table((0.4, 0.25), torch.device('cpu'))
