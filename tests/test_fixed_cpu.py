"""The `fixed` resize and the detect-from-files workflow without a device: y2_fixed_images_host against the numpy restatement of the header (bit for
bit), against y2_warp_affine_images_host + table (mode 0, bit for bit) and against an fp64 Keys cubic convolution (mode 1, within one level); its
refusals; transform.resize.image; utils.data.collate_images / to_device('cpu'); detect.to_source; utils.visualize.DrawBBox; utils.train.load_model;
detect.main with a stubbed detector."""
import configparser
import os

import numpy as np
import pytest
import torch

import collate_cases as cc
import fixed_cases as fx
import rotate_cases as rc

import _hip
import detect
import transform.resize.image
import transform.resize.label
import utils.data
import utils.train
import utils.visualize


@pytest.fixture(scope='module')
def groups():
    return fx.groups()


def host_levels(group):
    """uint8-valued levels [B, H, W, 3] in source channel order: the host function with the table lut[c][l] = l and no channel swap."""
    lut = np.tile(np.arange(256, dtype=np.float32), (3, 1))
    code, buf = fx.host(group, lut=lut, flags=0)
    assert code == 0
    at = fx.PAD + group['misalign']
    return buf[at:at + fx.numel(group)].reshape(-1, 3, group['H'], group['W']).transpose(0, 2, 3, 1).astype(np.int64)


# ---- the kernel's arithmetic, through the host function

@pytest.mark.parametrize('name', fx.GROUP_NAMES)
def test_host_equals_the_restatement(groups, name):
    code, buf = fx.host(groups[name])
    assert code == 0
    np.testing.assert_array_equal(buf, fx.restate(groups[name]))          # every value, and every sentinel around them


def test_the_groups_cover_what_they_claim(groups):
    modes = {name: set(groups[name]['geom'][:, 3].tolist()) for name in fx.GROUP_NAMES}
    assert modes['scales'] == {0, 1} and modes['rotations'] == {0, 1} and modes['unaligned'] == {0, 1} and modes['w30'] == {0, 1}
    assert groups['w30']['W'] % 4 and groups['unaligned']['W'] % 4 == 0 and groups['unaligned']['misalign'] == 1
    assert {tuple(g[1:3]) for g in groups['tiny_cubic']['geom'].tolist()} == {(h, w) for h in range(1, 6) for w in range(1, 6)}
    assert any((g['geom'][:, 0] > 3 * g['geom'][:, 2]).any() for g in groups.values()) and all((g['offset'] % 2 == 1).all() for g in groups.values())
    assert {g['flags'] for g in groups.values()} == {0, 1}
    # scale == 1 exactly in mode 1: the last image of `scales` is copied
    g = groups['scales']
    assert np.array_equal(g['inv'][-1], [1, 0, 0, 0, 1, 0]) and g['geom'][-1, 3] == 1
    np.testing.assert_array_equal(host_levels(g)[-1], fx.source(g, len(g['geom']) - 1))


def test_the_weight_table():
    w = fx.table()
    assert (w.sum((2, 3)) == 32768).all()
    assert w[0, 0].reshape(-1).tolist() == [0] * 5 + [32768] + [0] * 10          # the identity: an exact copy
    assert np.array_equal(w, w.transpose(1, 0, 3, 2))                             # rows and columns are the same one-dimensional recipe


@pytest.mark.parametrize('name', ['tiny_linear', 'scales', 'rotations', 'w30'])
def test_mode0_is_the_warp_entry_point_and_the_table(groups, name):
    g = groups[name]
    H, W = g['H'], g['W']
    pick = np.flatnonzero(g['geom'][:, 3] == 0)
    sub = dict(g, offset=g['offset'][pick], geom=g['geom'][pick], inv=g['inv'][pick])
    n = len(pick)
    dst_geom = np.tile(np.array([3 * W, H, W, 0, 0, H, W, 0], np.int32), (n, 1))
    src_geom = sub['geom'].copy()
    src_geom[:, 3] = 0          # (the warp entry point's fourth column is its flip)
    warp = dict(src=g['src'], src_offset=sub['offset'], src_geom=src_geom, inv=sub['inv'], dst_offset=np.arange(n, dtype=np.int64) * 3 * H * W,
                dst_geom=dst_geom, nbytes=n * 3 * H * W, fill=0, max_h=H, max_w=W)
    code, buf = rc.host(warp)
    assert code == 0
    canvas = buf[rc.PAD:rc.PAD + warp['nbytes']].reshape(n, H, W, 3)
    code, out = fx.host(sub)
    assert code == 0
    at = fx.PAD + g['misalign']
    out = out[at:at + fx.numel(sub)].reshape(n, 3, H, W)
    for c in range(3):
        np.testing.assert_array_equal(out[:, c], g['lut'][c][canvas[..., 2 - c if g['flags'] & 1 else c]])


@pytest.mark.parametrize('name', ['tiny_cubic', 'scales', 'rotations', 'w30', 'unaligned'])
def test_mode1_is_keys_cubic_convolution_within_one_level(groups, name):
    """Against the fp64 convolution at the quantised position, clamped to 0 .. 255.  The bound is derived, not measured: each of the sixteen int16
    weights is off by at most 0.5 / 32768, the sum correction moves one weight by at most 8 / 32768, together at most 16 / 32768 x 255 = 0.13 level
    before the final rounding to an integer (0.5): every level within 1."""
    g = groups[name]
    got = host_levels(g)
    worst = 0.0
    for b in np.flatnonzero(g['geom'][:, 3] == 1):
        want = fx.keys64(fx.source(g, b), g['inv'][b], g['H'], g['W'])
        worst = max(worst, float(np.abs(got[b] - want).max()))
    print('%s: worst |level - fp64| = %.4f' % (name, worst))
    assert worst <= 1.0


@pytest.mark.parametrize('name', ['tiny_cubic', 'tiny_linear', 'scales', 'rotations'])
def test_pixels_without_a_tap_inside_are_level_zero(groups, name):
    g = groups[name]
    code, buf = fx.host(g)
    at = fx.PAD + g['misalign']
    out = buf[at:at + fx.numel(g)].reshape(-1, 3, g['H'], g['W'])
    seen = 0
    for b, row in enumerate(g['geom']):
        outside = fx.all_outside(fx.source(g, b), g['inv'][b], int(row[3]), g['H'], g['W'])
        seen += int(outside.sum())
        for c in range(3):
            assert (out[b, c][outside] == g['lut'][c][0]).all()
    assert seen > 0


def test_refusals_leave_out_untouched(groups):
    g = groups['scales']
    B = len(g['geom'])
    untouched = fx.new_out(g)[0]

    def refused(expect=-1, **change):
        code, buf = fx.host(g, buf=untouched.copy(), **change)
        assert code == expect, change
        np.testing.assert_array_equal(buf, untouched)

    def with_row(key, b, col, value):
        table = g[key].copy()
        table[b, col] = value
        return {key: table}
    refused(**with_row('geom', 3, 3, 2))                      # a mode outside 0 / 1
    refused(**with_row('geom', 3, 3, -1))
    refused(**with_row('geom', B - 1, 1, 0))                  # zero and negative extents
    refused(**with_row('geom', 2, 2, -5))
    refused(**with_row('geom', 0, 2, _hip.WARP_MAX_DIM + 1))
    refused(**with_row('geom', 1, 0, 3 * int(g['geom'][1, 2]) - 1))          # a row stride below 3 * src_w
    offset = g['offset'].copy()
    offset[4] = -1
    refused(offset=offset)
    for col, value in ((0, 4.5), (1, -4.5), (3, float('nan')), (4, float('inf')), (2, 2.0 ** 19 + 1), (5, -1e300)):
        refused(**with_row('inv', B - 1, col, value))
    refused(flags=2)
    refused(H=0)
    refused(W=_hip.WARP_MAX_DIM + 1)
    lib = _hip.lib()
    a = [np.ascontiguousarray(g[k]) for k in ('src', 'offset', 'geom', 'inv', 'lut')]
    out = untouched.copy()
    p = [x.ctypes.data for x in a]
    assert lib.y2_fixed_images_host(p[0], p[1], p[2], p[3], p[4], 65536, g['H'], g['W'], 1, out.ctypes.data) == -3          # Y2_ENOSUP
    assert lib.y2_fixed_images_host(p[0], p[1], p[2], p[3], p[4], -1, g['H'], g['W'], 1, out.ctypes.data) == -1
    assert lib.y2_fixed_images_host(p[0], p[1], p[2], None, p[4], B, g['H'], g['W'], 1, out.ctypes.data) == -1
    assert lib.y2_fixed_images_host(None, None, None, None, None, 0, g['H'], g['W'], 1, None) == 0                         # B == 0: nothing to do
    np.testing.assert_array_equal(out, untouched)


# ---- transform.resize.image

def reference_fixed(_height, _width, height, width):
    """The scale and interpolation branch the reference computes (transform/resize/image.py:36-46), restated."""
    scale = height / _height if _height / _width > height / width else width / _width
    return scale, 0 if scale < 1 else 1


@pytest.mark.parametrize('size', [(375, 500), (500, 375), (333, 500), (500, 500), (416, 416), (417, 416), (416, 417), (415, 416), (416, 415), (208, 100),
                                  (1, 1), (1200, 1600), (607, 608), (608, 609)])
@pytest.mark.parametrize('canvas', [(416, 416), (608, 608), (320, 480)])
def test_fixed_records_the_reference_scale_and_mode(size, canvas):
    data = dict(image=np.zeros(size + (3,), np.uint8))
    out = transform.resize.image.fixed(data, *canvas)
    scale, mode = reference_fixed(*size, *canvas)
    assert out is data and 'window' not in out
    assert out['fixed']['scale'] == scale and out['fixed']['mode'] == mode and out['fixed']['matrix'] == [[scale, 0, 0], [0, scale, 0]]
    assert transform.resize.image.Fixed()(dict(image=data['image']), *canvas)['fixed'] == out['fixed']


def test_both_sides_of_scale_one():
    modes = [transform.resize.image.fixed(dict(image=np.zeros((h, 300, 3), np.uint8)), 416, 416)['fixed'] for h in (415, 416, 417)]
    assert [m['mode'] for m in modes] == [1, 1, 0] and modes[1]['scale'] == 1.0 and modes[0]['scale'] > 1 > modes[2]['scale']
    # a 500 x 375 VOC picture: the linear branch at 416, the cubic branch at 608
    image = np.zeros((375, 500, 3), np.uint8)
    assert [transform.resize.image.fixed(dict(image=image), s, s)['fixed']['mode'] for s in (416, 608)] == [0, 1]


def test_resize_reads_the_config():
    config = configparser.ConfigParser()
    config.read_dict({'data': {'resize': 'fixed'}})
    data = transform.resize.image.Resize(config)(dict(image=np.zeros((10, 20, 3), np.uint8)), 40, 40)
    assert data['fixed']['scale'] == 2.0 and data['fixed']['mode'] == 1
    config.set('data', 'resize', 'rescale')
    data = transform.resize.image.Resize(config)(dict(image=np.zeros((10, 20, 3), np.uint8)), 40, 40)
    assert data['window'] == (0, 0, 10, 20) and data['flip'] is False and 'fixed' not in data
    assert transform.resize.image.Rescale()(dict(image=np.zeros((3, 4, 3), np.uint8)), 8, 8)['window'] == (0, 0, 3, 4)
    config.set('data', 'resize', 'padding')
    with pytest.raises(NotImplementedError, match='padding'):
        transform.resize.image.Resize(config)
    config.set('data', 'resize', 'fixed')
    with pytest.raises(NotImplementedError, match='fixed'):          # the label module has no `fixed`, as in the reference
        transform.resize.label.Resize(config)


# ---- utils.data

def test_collate_images_rescale_equals_collate(golden):
    g = golden('collate')
    rng = np.random.RandomState(3)
    samples = [cc.sample(g, k, rng) for k in (1, 4, 5, 9, 11)]
    images = [s['image'] for s in samples]
    want = utils.data.Collate(transform.resize.label.Rescale(), [(40, 56)])(samples)
    got = utils.data.collate_images([dict(image=image) for image in images], transform.resize.image.Rescale(), 40, 56)
    for key in ('raw', 'offset', 'geom'):
        assert torch.equal(got[key], want[key]), key
    assert got['size'] == want['size'] and got['swap_rb'] == want['swap_rb'] and got['normalize'] == want['normalize']
    assert 'fixed_geom' not in got and not any(key in got for key in utils.data.LABELS)
    a, b = utils.data.to_device(got, 'cpu')['tensor'], utils.data.to_device(want, 'cpu')['tensor']
    assert a.shape == (5, 3, 40, 56) and torch.equal(a, b)


def fixed_batch(seed=4, sizes=((37, 50), (50, 37), (20, 13), (40, 56), (9, 80)), canvas=(40, 56), **kw):
    rng = np.random.RandomState(seed)
    images = [fx.picture(rng, h, w) for h, w in sizes]
    samples = [dict(image=image) for image in images]
    return images, samples, utils.data.collate_images(samples, transform.resize.image.Fixed(), *canvas, **kw)


def test_collate_images_fixed_on_the_cpu_path():
    images, samples, batch = fixed_batch()
    assert batch['fixed_geom'].dtype == torch.int32 and batch['fixed_inv'].dtype == torch.float64
    assert batch['fixed_geom'].tolist() == [[3 * w, h, w, s['fixed']['mode']] for (h, w, _), s in zip((i.shape for i in images), samples)]
    assert sorted(set(batch['fixed_geom'][:, 3].tolist())) == [0, 1]
    for row, s in zip(batch['fixed_inv'].numpy(), samples):
        np.testing.assert_array_equal(row, utils.data.invert_affine(s['fixed']['matrix']))
    launches = _hip.LAUNCHES[0]
    out = torch.full((5, 3, 40, 56), float(fx.SENTINEL))
    res = utils.data.to_device(batch, 'cpu', out=out)
    assert _hip.LAUNCHES[0] - launches == 1 and res['tensor'] is out
    group = dict(src=batch['raw'].numpy(), offset=batch['offset'].numpy(), geom=batch['fixed_geom'].numpy(), inv=batch['fixed_inv'].numpy(), H=40, W=56,
                 flags=1, lut=rc.reference_lut(), misalign=0)
    want = fx.restate(group)[fx.PAD:fx.PAD + fx.numel(group)].reshape(5, 3, 40, 56)
    np.testing.assert_array_equal(out.numpy(), want)
    # the canvas outside the scaled picture is level 0: the 9 x 80 picture fills 6.3 rows of the 40
    assert (out[4, :, 9:] == float(rc.reference_lut()[0][0])).all()
    # swap_rb and normalize travel with the batch
    _, _, plain = fixed_batch(swap_rb=False, normalize=None)
    lut = np.tile((np.arange(256, dtype=np.float32) / np.float32(255)), (3, 1))
    want = fx.restate(dict(group, flags=0, lut=lut))[fx.PAD:fx.PAD + fx.numel(group)].reshape(5, 3, 40, 56)
    np.testing.assert_array_equal(utils.data.to_device(plain, 'cpu')['tensor'].numpy(), want)


def test_to_device_refuses_bad_fixed_batches():
    _, samples, batch = fixed_batch()
    out = torch.full((5, 3, 40, 56), float(fx.SENTINEL))

    def refused(match, **change):
        with pytest.raises(ValueError, match=match):
            utils.data.to_device(dict(batch, **change), 'cpu', out=out)
        assert (out == float(fx.SENTINEL)).all()

    def table(key, b, col, value):
        t = batch[key].clone()
        t[b, col] = value
        return {key: t}
    refused('fixed: image 2', **table('fixed_geom', 2, 3, 2))
    refused('fixed: image 0', **table('fixed_geom', 0, 0, 3 * 50 - 1))
    refused('fixed: image 4', **table('fixed_geom', 4, 1, 10))          # the last image would end behind the buffer
    refused('fixed: image 1', **table('fixed_geom', 1, 2, 0))
    refused('fixed: image 3', **table('fixed_inv', 3, 0, float('nan')))
    refused('fixed: image 3', **table('fixed_inv', 3, 4, 4.01))
    refused('fixed_geom', fixed_geom=batch['fixed_geom'][:4])
    refused('warp or jitter', warp=torch.zeros(5, 6, dtype=torch.float64))
    refused('warp or jitter', jitter=torch.ones(5, 4, dtype=torch.int32))
    # a batch that mixes `fixed` and windowed samples
    mixed = [dict(image=np.zeros((8, 9, 3), np.uint8)) for _ in range(2)]
    resize = lambda data, height, width: (transform.resize.image.fixed if data is mixed[0] else transform.resize.image.rescale)(data, height, width)
    with pytest.raises(ValueError, match='mixes'):
        utils.data.collate_images(mixed, resize, 16, 16)
    with pytest.raises(ValueError, match='uint8'):
        utils.data.collate_images([dict(image=np.zeros((8, 9, 3), np.float32))], transform.resize.image.Fixed(), 16, 16)


# ---- detect.to_source

@pytest.mark.parametrize('size', [(375, 500), (500, 375), (100, 100), (30, 90)])
@pytest.mark.parametrize('name', ['rescale', 'fixed'])
def test_to_source_round_trips(name, size):
    height, width, rows, cols = 416, 416, 13, 13
    src_h, src_w = size
    record = getattr(transform.resize.image, name)(dict(image=np.zeros(size + (3,), np.uint8)), height, width)
    boxes = np.array([[0, 0], [src_h, src_w], [src_h / 3, src_w / 7], [10.5, 20.25]], np.float64)          # in source pixels
    if name == 'rescale':
        cells = boxes * (height / src_h, width / src_w) / (height / rows, width / cols)
    else:
        cells = boxes * record['fixed']['scale'] / (height / rows, width / cols)          # scaled into the canvas' top-left, then pixels -> cells
    back = detect.to_source(cells.astype(np.float32), record, rows, cols, height, width)
    assert back.dtype == np.float32 and back.shape == (4, 2)
    np.testing.assert_allclose(back, boxes, rtol=0, atol=max(size) * 4e-7 * 4)          # a few fp32 roundings of values up to the picture's size
    if name == 'fixed' and src_h != src_w:
        # the reference's formula (the rescale one) would misplace the far corner of a letterboxed picture by the letterbox factor
        wrong = cells * (src_h / rows, src_w / cols)
        assert np.abs(wrong - boxes).max() > 1


# ---- host-only pieces

def test_draw_bbox_clips_and_keeps_the_thickness():
    draw = utils.visualize.DrawBBox(['a', 'b', 'c'], colors=['red', '#00ff00', (0, 0, 255)], thickness=2)
    assert draw.colors == [(0, 0, 255), (0, 255, 0), (255, 0, 0)]          # BGR
    image = np.zeros((20, 30, 3), np.uint8)
    out = draw(image, np.array([[4, 5]]), np.array([[12, 20]]), np.array([1]))
    assert out is image
    green = (image == (0, 255, 0)).all(-1)
    want = np.zeros((20, 30), bool)
    want[4:13, 5:21] = True
    want[6:11, 7:19] = False          # two pixels thick, grown inwards
    np.testing.assert_array_equal(green, want)
    # boxes that leave the image on every side: what is inside is drawn, nothing raises, nothing wraps around
    image = np.zeros((20, 30, 3), np.uint8)
    draw(image, np.array([[-5, -7], [15, 25], [-50, -50], [30, 40]]), np.array([[6, 9], [40, 60], [-10, -10], [50, 60]]), np.array([0, 2, 1, 1]))
    red, blue = (image == (0, 0, 255)).all(-1), (image == (255, 0, 0)).all(-1)
    want = np.zeros((20, 30), bool)
    want[5:7, 0:10] = True          # the bottom and right sides of the first box; its top and left sides are outside
    want[0:7, 8:10] = True
    np.testing.assert_array_equal(red, want)
    want = np.zeros((20, 30), bool)
    want[15:17, 25:30] = True
    want[15:20, 25:27] = True
    np.testing.assert_array_equal(blue, want)
    assert not (image == (0, 255, 0)).all(-1).any()          # the two boxes wholly outside
    # the seeded palette: one colour per category, the same in every run; the class picks the colour
    a, b = utils.visualize.DrawBBox(['x'] * 20), utils.visualize.DrawBBox(['x'] * 20)
    assert a.colors == b.colors and len(set(a.colors)) == 20
    image = np.zeros((10, 10, 3), np.uint8)
    a(image, [[1, 1]], [[8, 8]], [7])
    assert tuple(image[1, 1]) == a.colors[7] and tuple(image[3, 5]) == a.colors[7] and tuple(image[4, 4]) == (0, 0, 0)          # thickness 3: rows 1-3 and 6-8


def test_load_model(tmp_path):
    with pytest.raises(FileNotFoundError):
        utils.train.load_model(str(tmp_path))
    for step in (5, 100, 20):
        (tmp_path / ('%d.pth' % step)).write_bytes(b'')
    (tmp_path / 'best.pth').write_bytes(b'')
    (tmp_path / '300.txt').write_bytes(b'')
    (tmp_path / '100.epoch').write_text('7')
    (tmp_path / '20.epoch').write_text('not a number')
    logged = []
    assert utils.train.load_model(str(tmp_path), logger=logged.append) == (str(tmp_path / '100.pth'), 100, 7)
    assert len(logged) == 1
    assert utils.train.load_model(str(tmp_path), step=5, logger=None) == (str(tmp_path / '5.pth'), 5, None)
    assert utils.train.load_model(str(tmp_path), step=20, logger=None) == (str(tmp_path / '20.pth'), 20, None)
    with pytest.raises(FileNotFoundError):
        utils.train.load_model(str(tmp_path), step=6, logger=None)


def test_main_writes_pictures_and_the_table(tmp_path):
    from PIL import Image
    rng = np.random.RandomState(9)
    src, dst = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    sizes = {'a.png': (30, 40), 'b.png': (48, 21), 'c.jpg': (25, 25)}
    for name, (h, w) in sizes.items():
        Image.fromarray(fx.picture(rng, h, w)[..., ::-1].copy()).save(str(src / name))
    (src / 'notes.txt').write_text('not a picture')
    (tmp_path / 'names').write_text('cat\ndog\n')
    (tmp_path / 'config.ini').write_text('[config]\nroot = %s\n[cache]\nname = cache\ncategory = %s\n' % (tmp_path, tmp_path / 'names'))
    calls = []

    def detector(paths):
        calls.append([os.path.basename(p) for p in paths])
        out = []
        for p in paths:
            if os.path.basename(p) == 'b.png':
                out.append(None)
            else:
                out.append((np.array([[2.5, 3.5], [-4, 10]], np.float32), np.array([[12.75, 20.25], [8, 100]], np.float32), np.array([1, 0]), np.array([0.9, 0.25], np.float32)))
        return out
    argv = ['-c', str(tmp_path / 'config.ini'), '-i', str(src), '-o', str(dst), '-b', '2', '--thickness', '1', '--colors', 'red', 'blue']
    args = detect.make_args(argv)
    assert args.batch_size == 2 and args.thickness == 1 and args.colors == ['red', 'blue'] and args.logging is None and args.modify == []
    assert detect.main(argv, detector=detector) == 0
    assert calls == [['a.png', 'b.png'], ['c.jpg']]
    assert sorted(os.listdir(str(dst))) == ['a.png', 'b.png', 'c.jpg', 'detections.tsv']
    lines = (dst / 'detections.tsv').read_text().splitlines()
    assert lines[0].split('\t') == ['file', 'class', 'score', 'ymin', 'xmin', 'ymax', 'xmax']
    assert [l.split('\t') for l in lines[1:]] == [[name, cls, score, ymin, xmin, ymax, xmax] for name in ('a.png', 'c.jpg') for cls, score, ymin, xmin, ymax, xmax in
                                                  (('dog', '0.900000', '2.50', '3.50', '12.75', '20.25'), ('cat', '0.250000', '-4.00', '10.00', '8.00', '100.00'))]
    for name, (h, w) in sizes.items():
        with Image.open(str(dst / name)) as image:
            assert image.size == (w, h)
            pixels = np.asarray(image.convert('RGB'))
        with Image.open(str(src / name)) as image:
            before = np.asarray(image.convert('RGB'))
        if name == 'a.png':          # lossless: the outline of the `dog` box is blue (RGB), one pixel wide, the rest of the picture untouched
            assert (pixels[2, 3:10] == (0, 0, 255)).all() and (pixels[12, 3:21] == (0, 0, 255)).all() and (pixels[2:13, 3] == (0, 0, 255)).all()
            assert (pixels[8, 10:40] == (255, 0, 0)).all()          # the `cat` box, clipped at the top and the right
            np.testing.assert_array_equal(pixels[14:], before[14:])
        if name == 'b.png':
            np.testing.assert_array_equal(pixels, before)


def test_main_names_the_missing_cv2(tmp_path):
    (tmp_path / 'config.ini').write_text('[config]\nroot = %s\n' % tmp_path)
    for source in ('0', '-1', str(tmp_path / 'clip.MP4'), 'movie.avi'):
        with pytest.raises(NotImplementedError, match='cv2'):
            detect.main(['-c', str(tmp_path / 'config.ini'), '-i', source, '-o', str(tmp_path / 'out')], detector=lambda paths: [])
    assert detect.list_pictures(str(tmp_path / 'config.ini')) == [str(tmp_path / 'config.ini')]
