"""y2_collate_jitter_images_host, transform.image and the jitter path of utils.data without a GPU: the host function against the numpy restatement of
jitter_cases.py bit for bit (every case group, every one of the 2^24 colours through the HSV path), the restated conversions against the textbook
HSV formulas in float64, the blur against an fp64 box mean, the plugins against the reference's draws and clip arithmetic
(tests/golden/jitter.npz), and Collate / to_device('cpu') end to end.

Measured here (all 2^24 BGR colours, all 2^24 HSV byte triples), the bounds being what 12-bit division tables and one fp32 rounding allow:
  BGR2HSV against the rounded exact values: H off by at most 1 (modulo 180), S by at most 1, V by 0
  HSV2RGB against the rounded exact conversion: off by at most 1 per channel"""
import configparser
import random

import numpy as np
import pytest
import torch

import collate_cases as cc
import jitter_cases as jc
import rotate_cases as rc
import transform.image as ti
import utils.data


@pytest.fixture(scope='module')
def groups():
    return jc.groups()


@pytest.fixture(scope='module')
def all_colours():
    """uint8 [4, 1024, 4096, 3]: every BGR colour once, as four images."""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([v & 255, (v >> 8) & 255, v >> 16], -1).astype(np.uint8).reshape(4, 1024, 4096, 3)


@pytest.fixture(scope='module')
def all_hsv(all_colours):
    """The restated BGR2HSV of every colour."""
    return np.stack([jc.bgr2hsv(img) for img in all_colours])


# ---- the host function

@pytest.mark.parametrize('name', jc.GROUP_NAMES)
def test_host_equals_the_restatement(groups, name):
    code, got = jc.host(groups[name])
    assert code == 0
    np.testing.assert_array_equal(got, jc.restate(groups[name]))          # the tensor and the sentinels around it


@pytest.mark.parametrize('name', ['32x32', '32x64', 'w4', 'w30', 'b1', 'b5'])
def test_plain_1x1_equals_collate_images(name):
    src, offset, geom, H, W = cc.groups()[name]
    lut, B = cc.random_lut(), len(geom)
    for flags in (0, 1):
        code, want = cc.host(src, offset, geom, lut, H, W, flags)
        group = dict(src=src, offset=offset, geom=geom, H=H, W=W, flags=flags, shift=0, jitter=np.array([(1, 1, 0, 0)] * B, np.int32), hsv_tab=None,
                     lut=np.ascontiguousarray(np.broadcast_to(lut, (B, 3, 256))))
        code2, got = jc.host(group)
        assert code == 0 and code2 == 0
        np.testing.assert_array_equal(got[jc.PAD:len(got) - jc.PAD], want[64:len(want) - 64])


def test_every_colour_through_hsv(all_colours, all_hsv):
    ident = np.arange(256, dtype=np.uint8)
    level = np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.float32), (4, 3, 256)))          # the output IS the level
    h, w = all_colours.shape[1:3]
    group = dict(src=all_colours.reshape(-1), offset=np.arange(4, dtype=np.int64) * (3 * h * w), geom=np.array([(3 * w, h, w, 0, 0, h, w, 0)] * 4, np.int32),
                 H=h, W=w, flags=1, shift=0, jitter=np.array([(1, 1, 1, 0)] * 4, np.int32), hsv_tab=np.ascontiguousarray(np.broadcast_to(ident, (4, 3, 256))), lut=level)
    code, got = jc.host(group)
    assert code == 0
    got = got[jc.PAD:len(got) - jc.PAD].reshape(4, 3, h, w)
    for b in range(4):
        want = jc.hsv2rgb(all_hsv[b])
        assert np.array_equal(got[b].astype(np.uint8), want.transpose(2, 0, 1)), b


def exact_hsv(bgr):
    """The textbook conversion in float64: H in units of 2 degrees in [0, 180), S and V in [0, 255]."""
    b, g, r = (bgr[..., c].astype(np.float64) for c in range(3))
    v = np.maximum(np.maximum(b, g), r)
    diff = v - np.minimum(np.minimum(b, g), r)
    safe = np.where(diff == 0, 1.0, diff)
    h = np.where(v == r, (g - b) / safe, np.where(v == g, 2.0 + (b - r) / safe, 4.0 + (r - g) / safe)) * 30.0
    h = np.where(diff == 0, 0.0, np.where(h < 0, h + 180.0, h))
    s = np.where(v == 0, 0.0, 255.0 * diff / np.where(v == 0, 1.0, v))
    return h, s, v


def test_bgr2hsv_is_within_one_level_of_the_exact_conversion(all_colours, all_hsv):
    worst = np.zeros(3, np.int64)
    for img, got in zip(all_colours, all_hsv):
        h, s, v = exact_hsv(img)
        got = got.astype(np.int64)
        dh = np.abs(got[..., 0] - np.rint(h).astype(np.int64)) % 180
        dh = np.minimum(dh, 180 - dh)
        grey = img.max(-1) == img.min(-1)
        assert (got[..., 0][grey] == 0).all()
        worst = np.maximum(worst, [dh.max(), np.abs(got[..., 1] - np.rint(s).astype(np.int64)).max(), np.abs(got[..., 2] - np.rint(v).astype(np.int64)).max()])
    print('BGR2HSV: largest |H|, |S|, |V| difference from the rounded exact values: %s' % worst.tolist())
    assert (worst <= 1).all(), worst


def exact_rgb(hsv):
    """The textbook inverse in float64 of byte triples (H in units of 2 degrees, any byte: the angle wraps): R, G, B in [0, 255]."""
    h, s, v = (hsv[..., c].astype(np.float64) for c in range(3))
    h6 = (h / 30.0) % 6.0
    s = s / 255.0
    f = lambda n: v * (1.0 - s * np.clip(np.minimum((n + h6) % 6.0, 4.0 - (n + h6) % 6.0), 0.0, 1.0))
    return np.stack([f(5.0), f(3.0), f(1.0)], -1)


def test_hsv2rgb_is_within_one_level_of_the_exact_conversion(all_colours):
    worst = 0
    for hsv in all_colours:          # every byte triple, read as (H, S, V)
        got = jc.hsv2rgb(hsv).astype(np.int64)
        worst = max(worst, int(np.abs(got - np.rint(exact_rgb(hsv)).astype(np.int64)).max()))
    print('HSV2RGB: largest difference from the rounded exact conversion: %d' % worst)
    assert worst <= 1, worst


def blur_only(img, kx, ky):
    """The host function on one image at identity resize, plain path, BGR order, the output being the level: uint8 [h, w, 3]."""
    h, w = img.shape[:2]
    group = dict(src=np.ascontiguousarray(img).reshape(-1), offset=np.zeros(1, np.int64), geom=np.array([(3 * w, h, w, 0, 0, h, w, 0)], np.int32), H=h, W=w, flags=0,
                 shift=0, jitter=np.array([(kx, ky, 0, 0)], np.int32), hsv_tab=None, lut=np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.float32), (1, 3, 256))))
    code, got = jc.host(group)
    assert code == 0
    return got[jc.PAD:len(got) - jc.PAD].reshape(3, h, w).transpose(1, 2, 0).astype(np.uint8)


@pytest.mark.parametrize('kx, ky', [(1, 1), (7, 7), (4, 2), (1, 7), (7, 1), (2, 5), (6, 6)])
def test_blur(kx, ky):
    rng = np.random.RandomState(kx * 8 + ky)
    const = np.full((9, 13, 3), 0, np.uint8) + np.array([3, 200, 255], np.uint8)
    assert np.array_equal(blur_only(const, kx, ky), const)          # the blur of a constant image is that constant
    img = rng.randint(0, 256, (19, 23, 3)).astype(np.uint8)          # larger than the window: numpy's reflect padding is REFLECT_101 then
    left, top = kx // 2, ky // 2
    padded = np.pad(img.astype(np.float64), ((top, ky - 1 - top), (left, kx - 1 - left), (0, 0)), mode='reflect')
    mean = sum(padded[j:j + 19, i:i + 23] for j in range(ky) for i in range(kx)) / (kx * ky)
    assert np.array_equal(blur_only(img, kx, ky), np.rint(mean).astype(np.uint8))          # (rint: half to even; the sums are integers, exact in fp64)


def test_identity_resize_and_1x1_blur_return_the_pixels():
    img = np.random.RandomState(3).randint(0, 256, (5, 6, 3)).astype(np.uint8)
    assert np.array_equal(blur_only(img, 1, 1), img)


def test_bad_tables_are_refused_with_nothing_written(groups):
    g = groups['tile_plus']

    def refused(code, **change):
        rc_, buf = jc.host(g, **change)
        assert rc_ == code and (buf == jc.SENTINEL).all(), change

    def with_row(key, b, col, value):
        t = g[key].copy()
        t[b, col] = value
        return {key: t}
    EINVAL, ENOSUP = -1, -3          # Y2_EINVAL, Y2_ENOSUP
    for col in (0, 1):
        for value in (0, -1, jc.MAX_BLUR + 1):
            refused(EINVAL, **with_row('jitter', 2, col, value))          # a blur size outside 1 .. 7, in a later image
    refused(EINVAL, **with_row('jitter', 1, 2, 2))                        # hsv neither 0 nor 1
    refused(EINVAL, **with_row('jitter', 3, 3, 1))                        # the reserved entry
    refused(EINVAL, hsv_tab=None)                                         # an image sets hsv and there is no table
    refused(EINVAL, **with_row('geom', 3, 5, 1000))                       # the checks of y2_collate_images_host: a window outside its image
    refused(EINVAL, **with_row('geom', 0, 7, 2))
    refused(EINVAL, W=4097)
    refused(EINVAL, H=0)
    refused(EINVAL, flags=2)
    refused(EINVAL, lut=None)
    refused(EINVAL, jitter=None)
    refused(ENOSUP, B=65536)
    rc_, buf = jc.host(g, B=0)
    assert rc_ == 0 and (buf == jc.SENTINEL).all()


# ---- the plugins

def chain_config(values):
    config = configparser.ConfigParser()
    config.read_dict({'augmentation': values})
    return config


def test_plugins_replay_the_reference(golden):
    g = golden('jitter')
    keys = ('random_blur', 'random_hue', 'random_saturation', 'random_brightness', 'random_gamma')
    for k in range(len(g['seed'])):
        config = chain_config({key: ' '.join(repr(v) for v in g[key][k].tolist()) for key in keys})
        jitter = ti.get_transform(config, jc.IMAGE_TRAIN.split())
        random.seed(int(g['seed'][k]))
        record = jitter()
        assert random.random() == g['next_random'][k]          # the same number of draws from the same generator
        assert record['draws'] == [tuple(g['blur'][k].tolist()), int(g['hue'][k]), float(g['saturation'][k]), float(g['brightness'][k]), float(g['gamma'][k])]
        assert record['blur'] == tuple(g['blur'][k].tolist()) and record['hsv'] is True
        hsv = g['hsv_in'][k]
        out = np.stack([record[c][hsv[..., i]] for i, c in enumerate('hsv')], -1)
        assert out.dtype == np.uint8 and np.array_equal(out, g['hsv_out'][k])          # the tables ARE the reference's clip arithmetic
        assert np.array_equal(record['gamma'], ti.gamma_table(float(g['gamma'][k])))


def test_maps_compose_in_any_order():
    config = chain_config(jc.AUGMENTATION)
    names = ['transform.image.BGR2HSV', 'transform.image.RandomBrightness', 'transform.image.RandomHue', 'transform.image.RandomSaturation', 'transform.image.HSV2RGB']
    random.seed(5)
    record = ti.get_transform(config, names)()
    random.seed(5)
    v, h, s = random.uniform(0.5, 1.5), random.randint(0, 25), random.uniform(0.5, 1.5)
    level = np.arange(256, dtype=np.uint8)
    assert record['draws'] == [v, h, s] and record['blur'] == (1, 1)
    assert np.array_equal(record['v'], np.clip(level * v, 0, 255).astype(np.uint8)) and np.array_equal(record['h'], np.clip(level.astype(int) + h, 0, 179).astype(np.uint8))
    assert np.array_equal(record['gamma'], level)


@pytest.mark.parametrize('gamma', [0.1, 0.5, 0.9, 1.0, 1.5, 2.2, 4.0])
def test_gamma_table(gamma):
    """floor(255 * (l / 255) ** gamma) as documented: monotone, 0 -> 0, and 255 -> 255 or 254 (where the float64 power of 1.0 scaled is below 255)."""
    t = ti.gamma_table(gamma).astype(np.int64)
    assert (np.diff(t) >= 0).all() and t[0] == 0 and t[255] in (254, 255)
    assert np.array_equal(t, np.floor(255 * (np.arange(256) / 255.0) ** gamma))
    if gamma == 1.0:
        assert (np.abs(t - np.arange(256)) <= 1).all()          # truncation: l / 255.0 * 255 may fall just below l


def test_negative_gamma_is_refused():
    with pytest.raises(ValueError):
        ti.gamma_table(-0.5)


P = 'transform.image.'


@pytest.mark.parametrize('sequence', [
    'RandomGamma RandomBlur BGR2RGB', 'BGR2RGB RandomBlur', 'RandomBlur', 'RandomGamma', 'RandomBlur RandomGamma', 'BGR2HSV RandomHue', 'RandomHue HSV2RGB',
    'BGR2HSV RandomHue RandomHue HSV2RGB', 'BGR2HSV HSV2RGB BGR2RGB', 'BGR2RGB BGR2HSV RandomHue HSV2RGB', 'BGR2HSV RandomGamma HSV2RGB',
    'RandomBlur RandomBlur BGR2RGB', 'BGR2RGB RandomGamma RandomGamma', 'HSV2RGB BGR2HSV', 'BGR2HSV RandomBlur HSV2RGB', 'BGR2RGB Normalize'])
def test_get_transform_refuses(sequence):
    names = [P + n for n in sequence.split()]
    config = chain_config(jc.AUGMENTATION)
    config.read_dict({'transform': {'normalize': '0.5 1'}})
    with pytest.raises(ValueError) as e:
        ti.get_transform(config, names)
    assert names[0] in str(e.value)          # the message names the sequence


def test_get_transform_refuses_a_foreign_plugin():
    with pytest.raises(ValueError):
        ti.get_transform(chain_config(jc.AUGMENTATION), ['torchvision.transforms.ToTensor'])


@pytest.mark.parametrize('sequence, swap, hsv, active', [
    ('', False, False, False), ('BGR2RGB', True, False, False), ('RandomBlur BGR2RGB', True, False, True), ('BGR2RGB RandomGamma', True, False, True),
    ('BGR2HSV HSV2RGB', False, True, True), ('RandomBlur BGR2HSV RandomSaturation HSV2RGB RandomGamma', False, True, True)])
def test_get_transform_accepts(sequence, swap, hsv, active):
    t = ti.get_transform(chain_config(jc.AUGMENTATION), [P + n for n in sequence.split()])
    assert (t.swap_rb, t.hsv, t.active) == (swap, hsv, active)


def test_normalize_reads_the_config():
    config = configparser.ConfigParser()
    config.read_dict({'transform': {'normalize': '0.5 2'}})
    n = ti.Normalize(config)
    assert (n.mean, n.std) == (0.5, 2.0) and torch.equal(n(torch.tensor([1.5])), torch.tensor([0.5]))


# ---- Collate and to_device

def same_batch(a, b):
    assert list(a) == list(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize('rotated', [False, True])
def test_without_jitter_the_batch_is_todays(golden, rotated):
    _, today = rc.make_batch(golden('collate'), rotated=rotated)
    for sequence in (None, 'transform.image.BGR2RGB'):
        _, batch = jc.make_batch(golden('collate'), rotated=rotated, sequence=sequence)
        same_batch(batch, today)


@pytest.mark.parametrize('rotated', [False, True])
def test_to_device_cpu_equals_the_restatement(golden, rotated):
    samples, batch = jc.make_batch(golden('collate'), seed=3, rotated=rotated)
    B = len(samples)
    assert batch['jitter'].dtype == torch.int32 and tuple(batch['jitter'].shape) == (B, 4) and batch['hsv_tab'].dtype == torch.uint8
    assert tuple(batch['hsv_tab'].shape) == (B, 3, 256) and batch['lut_b'].dtype == torch.float32 and tuple(batch['lut_b'].shape) == (B, 3, 256)
    assert batch['swap_rb'] is False and ('warp' in batch) == rotated
    # lut_b[b, c, l] = level_table(normalize)[c, gamma_b[l]], and the jitter rows are the samples' records
    level = rc.reference_lut()
    for b, data in enumerate(samples):
        r = data['jitter']
        assert batch['jitter'][b].tolist() == list(r['blur']) + [1, 0]
        assert np.array_equal(batch['lut_b'][b].numpy(), level[:, r['gamma']]) and np.array_equal(batch['hsv_tab'][b].numpy(), np.stack([r['h'], r['s'], r['v']]))
    assert len({tuple(r.tolist()) for r in batch['jitter']}) > 1          # the samples drew different blurs
    res = utils.data.to_device(batch, 'cpu')
    pixels = rc.restate_batch(batch, level)[1] if rotated else batch['raw'].numpy()
    np.testing.assert_array_equal(res['tensor'].numpy(), jc.restate_batch(batch, pixels))


def test_the_draws_follow_each_samples_resize(golden):
    """The reference resizes a sample and jitters it before it turns to the next one (utils/data.py:114-121): crop, then jitter, sample by sample."""
    import transform.resize.label
    g = golden('collate')
    config = jc.config_of(g)
    crop, jitter = transform.resize.label.RandomCrop(config), ti.get_transform(config, jc.IMAGE_TRAIN.split())
    samples = [cc.sample(g, k) for k in (1, 4, 5)]
    random.seed(11)
    np.random.seed(11)
    batch = utils.data.Collate(crop, [(40, 56)], transform_image=jitter)([dict(s) for s in samples])
    random.seed(11)
    np.random.seed(11)
    random.choice([(40, 56)])
    for b, s in enumerate(samples):
        data = crop(dict(s), 40, 56)
        record = jitter()
        assert batch['geom'][b, 3:7].tolist() == list(data['window']) and batch['jitter'][b, :2].tolist() == list(record['blur'])
        assert np.array_equal(batch['hsv_tab'][b, 0].numpy(), record['h'])


def test_to_device_checks_the_tables(golden):
    _, batch = jc.make_batch(golden('collate'), rotated=False)
    for col, value in ((0, 0), (1, 8), (2, 3), (3, 1)):
        bad = dict(batch, jitter=batch['jitter'].clone())
        bad['jitter'][1, col] = value
        with pytest.raises(ValueError):
            utils.data.to_device(bad, 'cpu')
    with pytest.raises(ValueError):
        utils.data.to_device({k: v for k, v in batch.items() if k != 'hsv_tab'}, 'cpu')
    with pytest.raises(ValueError):
        utils.data.to_device(dict(batch, lut_b=batch['lut_b'][:, :2]), 'cpu')
