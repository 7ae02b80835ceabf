"""What tests/test_train_cli_cpu.py and tests/test_gpu_train_cli.py share: a small cache directory in the reference's sample layout, drawn by
the test itself, and the config.ini around it."""
import os
import pickle

import numpy as np

CATEGORY = ['aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable', 'dog', 'horse', 'motorbike', 'person',
            'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor']
ANCHORS = [(1.3221, 1.73145), (3.19275, 4.00944), (5.05587, 8.09892), (9.47112, 4.84053), (11.2364, 10.0071)]          # (width, height) in cells
SIZES_LINE = '320,320 352,352 384,384 416,416 448,448 480,480 512,512 544,544 576,576 608,608'          # the reference's `[data] sizes`


def draw(rng, height, width, boxes):
    """BGR uint8 [h, w, 3]: smooth noise with one flat rectangle per box."""
    image = (rng.rand(height // 8 + 1, width // 8 + 1, 3) * 255).astype(np.uint8).repeat(8, 0).repeat(8, 1)[:height, :width].copy()
    for (y0, x0), (y1, x1), c in boxes:
        image[int(y0):int(y1), int(x0):int(x1)] = [(37 * c + 20) % 256, (91 * c + 60) % 256, (53 * c + 100) % 256]
    return image


def make_cache(root, count=10, seed=0, classes=4):
    """<root>/cache: `category`, `train.pkl`, `test.pkl` (the same samples) and the pictures - baseline JPEG files, the third one a PNG - of 96-160
    pixels with one to three boxes each; one box of the second picture is difficult.  Returns the samples."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    cache = os.path.join(root, 'cache')
    os.makedirs(os.path.join(cache, 'images'), exist_ok=True)
    samples = []
    for i in range(count):
        height, width = (int(v) for v in rng.randint(96, 161, 2))
        n = 1 + i % 3
        lo = np.stack([rng.uniform(2, height * 0.5, n), rng.uniform(2, width * 0.5, n)], 1)
        hi = lo + np.stack([rng.uniform(20, height * 0.45, n), rng.uniform(20, width * 0.45, n)], 1)
        cls = rng.randint(0, classes, n)
        difficult = np.zeros(n, np.uint8)
        if i == 1:
            difficult[-1] = 1
        image = draw(rng, height, width, zip(lo, hi, cls))
        path = os.path.join(cache, 'images', '%02d.%s' % (i, 'png' if i == 2 else 'jpg'))
        Image.fromarray(np.ascontiguousarray(image[..., ::-1])).save(path, **({} if i == 2 else dict(quality=92, progressive=False)))
        samples.append(dict(path=path, yx_min=lo.astype(np.float32), yx_max=hi.astype(np.float32), cls=cls.astype(np.int64), difficult=difficult))
    with open(os.path.join(cache, 'category'), 'w') as f:
        f.write('\n'.join(CATEGORY) + '\n')
    for phase in ('train', 'test'):
        with open(os.path.join(cache, phase + '.pkl'), 'wb') as f:
            pickle.dump(samples, f)
    return samples


def make_config(root, **modify):
    """Writes <root>/config.ini and <root>/anchors.tsv; returns the ini's path.  modify: 'section/option' -> value (None removes the option)."""
    import configparser
    with open(os.path.join(root, 'anchors.tsv'), 'w') as f:
        f.write('width\theight\n' + ''.join('%r\t%r\n' % a for a in ANCHORS))
    config = configparser.ConfigParser()
    config.read_dict({
        'config': {'root': str(root)},
        'image': {'size': '128 128'},
        'cache': {'name': 'cache', 'category': os.path.join(str(root), 'cache', 'category')},
        'model': {'name': 'model', 'anchors': os.path.join(str(root), 'anchors.tsv'), 'dnn': 'model.yolo2.Tiny', 'pretrained': '0', 'threshold': '0.6'},
        'batch_norm': {'enable': '1', 'gamma': '1', 'beta': '1'},
        'data': {'workers': '0', 'sizes': '96,96 128,128', 'maintain': '1', 'shuffle': '0', 'resize': 'rescale'},
        'transform': {'augmentation': 'transform.augmentation.RandomRotate transform.augmentation.RandomFlipHorizontally',
                      'resize_train': 'transform.resize.label.RandomCrop', 'resize_eval': 'transform.resize.label.Resize',
                      'resize_test': 'transform.resize.image.Resize', 'image_train': 'transform.image.BGR2RGB', 'image_test': 'transform.image.BGR2RGB',
                      'tensor': 'torchvision.transforms.ToTensor transform.image.Normalize', 'normalize': '0.5 1'},
        'augmentation': {'random_rotate': '-5 5', 'random_flip_horizontally': '0.5', 'random_crop': '1'},
        'train': {'optimizer': 'lambda params, lr: utils.optim.Adam(params, lr, betas=(0.9, 0.999), eps=1e-8)', 'phase': 'train', 'cross_entropy': '1'},
        'save': {'secs': '600', 'keep': '5'},
        'summary': {'scalar': '0'},
        'hparam': {'foreground': '5', 'background': '1', 'center': '1', 'size': '1', 'cls': '1'},
        'detect': {'threshold': '0.3', 'threshold_cls': '0.005', 'fix': '0', 'overlap': '0.45'},
        'eval': {'phase': 'test', 'iou': '0.5', 'db': 'eval.json', 'metric07': '1'},
    })
    for target, value in modify.items():
        section, option = target.split('/')
        if value is None:
            config.remove_option(section, option)
        else:
            if not config.has_section(section):
                config.add_section(section)
            config.set(section, option, str(value))
    path = os.path.join(str(root), 'config.ini')
    with open(path, 'w') as f:
        config.write(f)
    return path


def load_config(path):
    import configparser
    config = configparser.ConfigParser()
    config.read(path)
    return config
