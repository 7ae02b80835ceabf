"""The rotation of the device collate path on the library's HOST code: transform.augmentation.RandomRotate against tests/golden/rotate.npz (matrices,
canvas sizes and labels produced by the reference's own Rotator / random_rotate, tools/make_golden_rotate.py), y2_warp_affine_images_host against
the numpy restatement of its contract (rotate_cases.py) and against properties that hold whatever OpenCV does, and utils.data.Collate / to_device
on 'cpu' with rotated samples."""
import configparser
import random

import numpy as np
import pytest
import torch

import _hip
import collate_cases as cc
import rotate_cases as rc
import transform.augmentation as ta
import transform.resize.label
import utils
import utils.data


@pytest.fixture(scope='module')
def groups():
    return rc.groups()


# ---- reference semantics

def rotate_config(low, high):
    config = configparser.ConfigParser()
    config.read_dict({'augmentation': {'random_rotate': '%r %r' % (float(low), float(high))}, 'transform': {'augmentation': 'transform.augmentation.RandomRotate'}})
    return config


def test_random_rotate_reproduces_the_reference(golden):
    g = golden('rotate')
    assert len(g['seed']) >= 16 and {tuple(r) for r in g['angle_range'].tolist()} == {(-5, 5), (-45, 45), (0, 0), (170, 190)} and tuple(g['size'].min(0)) == (7, 5)
    for k in range(len(g['seed'])):
        config = rotate_config(*g['angle_range'][k])
        plugin = utils.parse_attr(config.get('transform', 'augmentation'))(config)          # the dotted name of config.ini resolves
        assert isinstance(plugin, ta.RandomRotate)
        n, (h, w) = int(g['count'][k]), g['size'][k]
        image = np.zeros((h, w, 3), np.uint8)
        data = dict(image=image, yx_min=g['in_min'][k, :n].copy(), yx_max=g['in_max'][k, :n].copy(), cls=np.zeros(n, np.int64), difficult=np.zeros(n, np.uint8))
        random.seed(int(g['seed'][k]))
        np.random.seed(int(g['seed'][k]))
        state = np.random.get_state()[1].copy()
        data = plugin(data)
        after = random.random()
        assert data['rotate']['matrix'].dtype == np.float64 and data['rotate']['matrix'].shape == (2, 3)
        np.testing.assert_array_equal(data['rotate']['matrix'].view(np.uint64), g['matrix'][k].view(np.uint64), err_msg='sample %d' % k)
        assert tuple(data['rotate']['size']) == tuple(g['rotated'][k]) and data['rotate']['flip'] is False, k
        assert data['yx_min'].dtype == np.float32 and data['yx_max'].dtype == np.float32
        np.testing.assert_array_equal(data['yx_min'].view(np.uint32), g['out_min'][k, :n].view(np.uint32), err_msg='sample %d' % k)
        np.testing.assert_array_equal(data['yx_max'].view(np.uint32), g['out_max'][k, :n].view(np.uint32), err_msg='sample %d' % k)
        assert after == g['next_random'][k] and (np.random.get_state()[1] == state).all(), k          # one random.uniform, nothing from numpy's generator
        assert data['image'] is image and not image.any() and image.shape == (h, w, 3)
        assert g['fill'][k] == 0          # what the reference passes as the border value: to_device's default


def test_order_rules(golden):
    g = golden('collate')
    config = rc.config_of(g)
    rotate = ta.RandomRotate(config)
    with pytest.raises(ValueError, match='rotate first'):
        rotate(transform.resize.label.Rescale()(cc.sample(g, 1), 64, 64))
    with pytest.raises(ValueError, match='one rotation per sample'):
        rotate(rotate(cc.sample(g, 1)))
    # rotate after a flip: the flip moves into the rotation's source addressing
    data = rotate(ta.flip_horizontally(cc.sample(g, 1)))
    assert data['rotate']['flip'] is True and data['flip'] is False
    # flip after rotate: the collate flip, mirrored about the ROTATED frame's centre line
    data = rotate(cc.sample(g, 1))
    width = data['rotate']['size'][1]
    assert width != data['image'].shape[1]
    x_min, x_max = data['yx_min'][:, 1].copy(), data['yx_max'][:, 1].copy()
    data = ta.flip_horizontally(data)
    assert data['flip'] is True and data['rotate']['flip'] is False
    np.testing.assert_array_equal(data['yx_min'][:, 1], width - x_max)
    np.testing.assert_array_equal(data['yx_max'][:, 1], width - x_min)
    # the resize transforms see the rotated frame
    data = transform.resize.label.Rescale()(data, 64, 96)
    assert data['window'] == (0, 0) + tuple(data['rotate']['size'])


def test_invert_affine_is_the_inverse_in_the_stated_order():
    M = np.array([[0.8, 0.6, 3.25], [-0.6, 0.8, 7.5]])
    A = utils.data.invert_affine(M)
    D = 1.0 / (M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0])
    A0, A1, A3, A4 = M[1, 1] * D, -M[0, 1] * D, -M[1, 0] * D, M[0, 0] * D
    want = np.array([A0, A1, -A0 * M[0, 2] - A1 * M[1, 2], A3, A4, -A3 * M[0, 2] - A4 * M[1, 2]])
    np.testing.assert_array_equal(A.view(np.uint64), want.view(np.uint64))
    np.testing.assert_allclose(A, rc.inverse(M), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(utils.data.invert_affine([[1, 0, 0], [0, 1, 0]]), [1, 0, 0, 0, 1, 0])
    assert not utils.data.invert_affine(np.zeros((2, 3))).any()          # a singular matrix: D = 0


# ---- the host function against the restated contract

@pytest.mark.parametrize('name', rc.GROUP_NAMES)
def test_host_equals_restatement(groups, name):
    rcode, got = rc.host(groups[name])
    assert rcode == 0
    np.testing.assert_array_equal(got, rc.restate(groups[name]))          # the sentinels on both sides and in the row padding included


def test_cases_cover_the_paths(groups):
    """The groups hold what they are there for."""
    for name in ('angles', 'widths', 'shift', 'b1', 'b5'):
        assert (groups[name]['dst_offset'] % 4 == 0).all() and (groups[name]['dst_geom'][:, 0] % 4 == 0).all(), name
        assert (groups[name]['dst_geom'][:, 0] > 3 * groups[name]['dst_geom'][:, 2]).any() or name == 'b1', name
    for name in ('small', 'angles_bytes', 'widths_bytes'):
        assert (groups[name]['dst_offset'] % 2 == 1).all(), name
    for g in groups.values():
        assert (g['src_offset'] % 2 == 1).all()
    assert groups['widths']['dst_geom'][:, 2].tolist() == [1, 3, 4, 5, 30, 64] and groups['widths_bytes']['dst_geom'][:, 2].tolist() == [1, 3, 4, 5, 30, 64]
    assert tuple(groups['small']['src_geom'][0, 1:3]) == (7, 5) and len(groups['b0']['dst_geom']) == 0 and len(groups['b1']['dst_geom']) == 1
    assert groups['b1']['dst_geom'][0, 1] > 16 and groups['b5']['max_h'] > groups['b5']['dst_geom'][:, 1].max() and len({tuple(r[1:3]) for r in groups['b5']['dst_geom']}) == 5
    assert set(groups['angles']['src_geom'][:, 3].tolist()) == {0, 1} and groups['angles_bytes']['fill'] and (groups['angles']['src_geom'][:, 0] > 3 * groups['angles']['src_geom'][:, 2]).any()
    # the shifted images: each border of the source meets the fill inside the canvas
    seen = set()
    g = groups['shift']
    for b, dg in enumerate(g['dst_geom']):
        X, Y = rc.positions(g['inv'][b], int(dg[1]), int(dg[2]))
        sx, sy, (sh, sw) = X >> 5, Y >> 5, g['src_geom'][b, 1:3]
        rows, cols = (sy >= 0) & (sy < sh), (sx >= 0) & (sx < sw)
        seen |= {k for k, m in (('left', (sx == -1) & rows), ('right', (sx == sw - 1) & rows), ('top', (sy == -1) & cols), ('bottom', (sy == sh - 1) & cols)) if m.any()}
    assert seen == {'left', 'right', 'top', 'bottom'}


# ---- properties that do not depend on OpenCV fidelity

def warp_one(img, A, size, fill=0, flip=0, aligned=True):
    """One image through the host function; uint8 [dst_h, dst_w, 3]."""
    group = rc.make_group(np.random.RandomState(1), [(img, A, size, flip, 0)], aligned, fill)
    rcode, buf = rc.host(group)
    assert rcode == 0
    stride, dh, dw = (int(v) for v in group['dst_geom'][0, :3])
    rows = np.lib.stride_tricks.as_strided(buf[rc.PAD + int(group['dst_offset'][0]):], shape=(dh, 3 * dw), strides=(stride, 1))
    return rows.reshape(dh, dw, 3).copy()


@pytest.fixture(scope='module')
def picture():
    return np.random.RandomState(3).randint(0, 256, (21, 34, 3)).astype(np.uint8)


def test_identity_is_an_exact_copy(picture):
    for aligned in (True, False):
        np.testing.assert_array_equal(warp_one(picture, (1, 0, 0, 0, 1, 0), picture.shape[:2], aligned=aligned), picture)


def test_integer_translation_is_a_shifted_copy(picture):
    h, w = picture.shape[:2]
    fill = 0x0A141E
    for dx, dy in ((3, 0), (-4, 2), (0, -5), (7, 6)):
        got = warp_one(picture, (1, 0, -dx, 0, 1, -dy), (h, w), fill)          # destination (x, y) reads source (x - dx, y - dy)
        want = np.empty_like(picture)
        want[:] = (0x1E, 0x14, 0x0A)
        want[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] = picture[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)]
        np.testing.assert_array_equal(got, want)


def test_quarter_turns_equal_rot90(picture):
    """The exact matrices of 90, 180 and 270 degrees about the centre of the pixel grid, as numbers: destination (x, y) of the turned canvas reads
    source (w - 1 - y, x), (w - 1 - x, h - 1 - y), (y, h - 1 - x)."""
    h, w = picture.shape[:2]
    for k, A, size in ((1, (0, -1, w - 1, 1, 0, 0), (w, h)), (2, (-1, 0, w - 1, 0, -1, h - 1), (h, w)), (3, (0, 1, 0, -1, 0, h - 1), (w, h))):
        np.testing.assert_array_equal(warp_one(picture, A, size, fill=0x55AA55), np.rot90(picture, k))


def test_position_and_level_bounds(groups):
    """What the fixed-point recipe promises, derived: X is the nearest multiple of 1/32 px to a sum of two terms each rounded to 1/1024 px - at most
    1/64 + 2 * (1/2048) px from A (x, y, 1); the level is the exact bilinear sum at that position rounded to nearest - at most 0.5 from it."""
    worst_p = worst_l = 0.0
    for name in ('angles', 'angles_bytes', 'widths', 'shift', 'b5'):
        g = groups[name]
        for b, dg in enumerate(g['dst_geom']):
            A, dh, dw = g['inv'][b], int(dg[1]), int(dg[2])
            X, Y = rc.positions(A, dh, dw)
            x, y = np.meshgrid(np.arange(dw, dtype=np.float64), np.arange(dh, dtype=np.float64))
            worst_p = max(worst_p, np.abs(X / 32.0 - (A[0] * x + A[1] * y + A[2])).max(), np.abs(Y / 32.0 - (A[3] * x + A[4] * y + A[5])).max())
            img = rc.source(g, b)
            if g['src_geom'][b, 3]:
                img = img[:, ::-1]
            got = rc.warp_image(rc.source(g, b), A, dh, dw, g['fill'], int(g['src_geom'][b, 3])).astype(np.float64)
            worst_l = max(worst_l, np.abs(got - rc.bilinear64(img, X / 32.0, Y / 32.0, g['fill'])).max())
    print('worst position error %.6f px (bound %.6f), worst level error %.4f' % (worst_p, 1 / 64 + 1 / 1024, worst_l))
    assert worst_p <= 1 / 64 + 1 / 1024 and worst_l <= 0.5


@pytest.mark.parametrize('v', [0, 1, 128, 254, 255])
def test_constant_image_with_its_own_fill_stays_constant(v):
    img = np.full((12, 17, 3), v, np.uint8)
    for angle in (0, 5, 45, -135):
        A, size = rc.rotation(12, 17, angle)
        assert (warp_one(img, A, size, fill=v * 0x010101) == v).all()


def test_flip_equals_warping_the_mirrored_image(picture):
    for angle in (0, 30, -135):
        A, size = rc.rotation(picture.shape[0], picture.shape[1], angle)
        np.testing.assert_array_equal(warp_one(picture, A, size, fill=0x112233, flip=1), warp_one(np.ascontiguousarray(picture[:, ::-1]), A, size, fill=0x112233))


# ---- refused tables

def test_bad_tables_are_refused_and_nothing_is_written(groups):
    g = groups['b5']
    limit = _hip.WARP_MAX_DIM

    def changed(key, b, col, value):
        t = g[key].copy()
        t[b, col] = value
        return {key: t}
    for change in (changed('inv', 3, 0, 4.5), changed('inv', 3, 4, -4.5), changed('inv', 3, 2, 2.0 ** 19 + 1), changed('inv', 3, 5, float('nan')),
                   changed('inv', 3, 1, float('inf')), changed('src_geom', 3, 1, 0), changed('src_geom', 3, 2, limit + 1), changed('src_geom', 3, 0, 3),
                   changed('src_geom', 3, 3, 2), changed('dst_geom', 3, 1, 0), changed('dst_geom', 3, 2, g['max_w'] + 1), changed('dst_geom', 3, 1, g['max_h'] + 1),
                   changed('dst_geom', 3, 0, 3), dict(dst_offset=np.where(np.arange(5) == 3, -4, g['dst_offset'])), dict(src_offset=np.where(np.arange(5) == 3, -1, g['src_offset'])),
                   dict(fill=1 << 24), dict(max_h=limit + 1), dict(max_w=0)):
        rcode, buf = rc.host(g, **change)          # (a LATER image: the tables are checked before the first image is written)
        assert rcode == -1, change
        assert (buf == rc.SENTINEL).all(), change


def test_to_device_checks_the_tables(golden):
    _, batch = rc.make_batch(golden('collate'))

    def changed(key, b, col, value):
        t = batch[key].clone()
        t[b, col] = value
        return dict(batch, **{key: t})
    for bad in (changed('warp', 2, 0, 4.5), changed('warp', 2, 2, float('nan')), changed('src_geom', 2, 3, 2), changed('src_geom', 2, 1, 1000),
                changed('geom', 2, 1, int(batch['geom'][2, 1]) + 400), dict(batch, rot_bytes=int(batch['offset'].max()) + 10), dict(batch, raw=batch['raw'][:-1].clone())):
        with pytest.raises(ValueError, match='outside'):
            utils.data.to_device(bad, 'cpu')
    with pytest.raises(ValueError, match='rot must be'):
        utils.data.to_device(batch, 'cpu', rot=torch.empty(batch['rot_bytes'] - 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match='rot must be'):
        utils.data.to_device(batch, 'cpu', rot=torch.empty(batch['rot_bytes'], dtype=torch.int8))


# ---- Collate and to_device

def test_collate_adds_the_warp_tables(golden):
    g = golden('collate')
    samples, batch = rc.make_batch(g)
    assert sorted(batch) == sorted(['yx_min', 'yx_max', 'cls', 'difficult', 'raw', 'offset', 'geom', 'size', 'swap_rb', 'normalize',
                                    'src_offset', 'src_geom', 'warp', 'rot_bytes', 'rot_size'])
    B = 5
    assert batch['src_offset'].dtype == torch.int64 and tuple(batch['src_offset'].shape) == (B,)
    assert batch['src_geom'].dtype == torch.int32 and tuple(batch['src_geom'].shape) == (B, 4)
    assert batch['warp'].dtype == torch.float64 and tuple(batch['warp'].shape) == (B, 6)
    assert batch['src_geom'][:, 3].tolist() == [1, 0, 0, 0, 0] and batch['geom'][:3, 7].tolist() == [0, 1, 0]          # a flip before / after the rotation
    pos = 0
    for b, data in enumerate(samples):
        h, w = data['image'].shape[:2]
        assert int(batch['src_offset'][b]) == pos and batch['src_geom'][b, :3].tolist() == [3 * w, h, w]
        np.testing.assert_array_equal(batch['raw'][pos:pos + 3 * h * w].numpy().reshape(h, w, 3), data['image'])          # the untouched source pixels
        pos += 3 * h * w
        rh, rw = data['rotate']['size'] if 'rotate' in data else (h, w)
        stride = int(batch['geom'][b, 0])
        assert batch['geom'][b, 1:3].tolist() == [rh, rw] and tuple(batch['geom'][b, 3:7].tolist()) == data['window']
        assert stride >= 3 * rw and stride % 4 == 0 and int(batch['offset'][b]) % 4 == 0          # the layout the 12-byte stores want
        want = utils.data.invert_affine(data['rotate']['matrix']) if 'rotate' in data else np.array([1., 0, 0, 0, 1, 0])
        np.testing.assert_array_equal(batch['warp'][b].numpy().view(np.uint64), want.view(np.uint64))
    assert batch['raw'].numel() == pos and 'rotate' not in samples[3] and batch['rot_size'] == (int(batch['geom'][:, 1].max()), int(batch['geom'][:, 2].max()))
    last = int(np.argmax(batch['offset'].numpy()))
    assert batch['rot_bytes'] >= int(batch['offset'][last]) + int(batch['geom'][last, 0]) * int(batch['geom'][last, 1])
    utils.data.check_geometry(batch['offset'].numpy(), batch['geom'].numpy(), batch['rot_bytes'])


@pytest.mark.parametrize('fill', [0, 0x3C78B4])
def test_to_device_cpu_equals_collate_of_the_restated_warp(golden, fill):
    _, batch = rc.make_batch(golden('collate'), seed=2)
    if fill:
        batch['fill'] = fill
    H, W = batch['size']
    want, rot_want = rc.restate_batch(batch, rc.reference_lut(), fill)
    launches = _hip.LAUNCHES[0]
    res = utils.data.to_device(batch, 'cpu')
    assert _hip.LAUNCHES[0] - launches == 2
    assert res['tensor'].dtype == torch.float32 and tuple(res['tensor'].shape) == (5, 3, H, W)
    np.testing.assert_array_equal(res['tensor'].numpy().view(np.uint32), want.view(np.uint32))
    assert 'tensor' not in batch and 'rot' not in batch and res['raw'] is batch['raw']
    # out= and rot=: the supplied buffers are written and returned; bytes of rot beyond the rows of the images stay
    buf = torch.full((5, 3, H, W), float(cc.SENTINEL))
    rot = torch.full((batch['rot_bytes'] + 100,), int(rc.SENTINEL), dtype=torch.uint8)
    res2 = utils.data.to_device(batch, 'cpu', out=buf, rot=rot)
    assert res2['tensor'] is buf and res2['rot'] is rot and torch.equal(buf, res['tensor'])
    got, written = rot.numpy(), np.zeros(rot.numel(), bool)
    for b, (stride, h, w) in enumerate(batch['geom'][:, :3].tolist()):
        rows = int(batch['offset'][b]) + stride * np.arange(h)[:, None] + np.arange(3 * w)[None, :]
        written[rows] = True
        np.testing.assert_array_equal(got[rows], rot_want[rows])
    assert (got[~written] == rc.SENTINEL).all() and not written[batch['rot_bytes']:].any()


def test_unrotated_batch_is_what_it_was(golden):
    """No sample carries `rotate`: the key list, the bytes and the single launch of the path without rotation; `rot` is not touched."""
    samples, batch = rc.make_batch(golden('collate'), rotated=False)
    assert list(batch) == ['yx_min', 'yx_max', 'cls', 'difficult', 'raw', 'offset', 'geom', 'size', 'swap_rb', 'normalize']
    pos = 0
    for b, data in enumerate(samples):
        h, w = data['image'].shape[:2]
        assert int(batch['offset'][b]) == pos and batch['geom'][b].tolist() == [3 * w, h, w] + list(data['window']) + [b % 2]
        np.testing.assert_array_equal(batch['raw'][pos:pos + 3 * h * w].numpy().reshape(h, w, 3), data['image'])
        pos += 3 * h * w
    assert batch['raw'].numel() == pos
    rot = torch.full((64,), int(rc.SENTINEL), dtype=torch.uint8)
    launches = _hip.LAUNCHES[0]
    res = utils.data.to_device(batch, 'cpu', rot=rot)
    assert _hip.LAUNCHES[0] - launches == 1 and 'rot' not in res and (rot == int(rc.SENTINEL)).all()
    H, W = batch['size']
    want = cc.restate(batch['raw'].numpy(), batch['offset'].numpy(), batch['geom'].numpy(), rc.reference_lut(), H, W, 1)
    np.testing.assert_array_equal(res['tensor'].numpy().view(np.uint32), want.view(np.uint32))
