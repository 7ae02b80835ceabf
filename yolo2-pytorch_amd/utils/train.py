"""`utils.train` — the checkpoint and timing helpers of the training loop under the reference's names (utils/train.py): `load_model` (which
checkpoint of a model directory to read), `Saver` (write one, keep the newest few), `Timer` (has this many seconds passed?), `load_sizes`.

A model directory holds `<step>.pth` (a state_dict) beside `<step>.epoch` (the epoch as text), as convert_darknet_torch.py and `Saver` write them."""
import logging
import os
import time

import torch


class Timer(object):
    """Timer(max, first=True)() is True when more than `max` seconds have passed since it last was True (since construction, for the first time;
    first=True: the first call is True at once)."""

    def __init__(self, max, first=True):
        self.max = max
        self.start = 0 if first else time.time()

    def __call__(self):
        now = time.time()
        if now - self.start > self.max:
            self.start = now
            return True
        return False


def _steps(model_dir, ext):
    """[(step, stem)] of the all-digit `<step><ext>` files of a directory, ascending."""
    found = []
    for entry in os.listdir(model_dir):
        stem, suffix = os.path.splitext(entry)
        if suffix == ext and stem.isdigit():
            found.append((int(stem), stem))
    return sorted(found)


class Saver(object):
    """Saver(model_dir, keep)(obj, step, epoch) writes `<model_dir>/<step><ext>` with torch.save and, when epoch is given, `<step><ext_epoch>` holding it as
    text; then `tidy()` removes all but the `keep` checkpoints with the largest steps (a missing epoch file is reported, not an error).  Returns the
    path without extension."""

    def __init__(self, model_dir, keep, ext='.pth', ext_epoch='.epoch', logger=logging.info):
        self.model_dir, self.keep, self.ext, self.ext_epoch = model_dir, keep, ext, ext_epoch
        self.logger = logger if logger is not None else (lambda message: None)

    def __call__(self, obj, step, epoch=None):
        os.makedirs(self.model_dir, exist_ok=True)
        base = os.path.join(self.model_dir, str(step))
        torch.save(obj, base + self.ext)
        if epoch is not None:
            with open(base + self.ext_epoch, 'w') as f:
                f.write(str(epoch))
        self.logger('model saved into %s.*' % base)
        self.tidy()
        return base

    def tidy(self):
        found = _steps(self.model_dir, self.ext)
        for _, stem in found[:max(len(found) - self.keep, 0)]:
            base = os.path.join(self.model_dir, stem)
            os.remove(base + self.ext)
            if os.path.exists(base + self.ext_epoch):
                os.remove(base + self.ext_epoch)
            else:
                self.logger('%s not found' % (base + self.ext_epoch))


def load_sizes(config):
    """`[data] sizes` = "320,320 352,352 ..." -> [(height, width), ...]."""
    return [tuple(int(v) for v in pair.split(',')) for pair in config.get('data', 'sizes').split()]


def load_model(model_dir, step=None, ext='.pth', ext_epoch='.epoch', logger=logging.info):
    """(path, step, epoch) of the checkpoint `step`, or of the newest one - the largest all-digit file name with the extension `ext` - when step is
    None.  epoch is None when the `.epoch` file is missing or does not hold an integer.  A directory without a checkpoint raises FileNotFoundError."""
    if step is None:
        found = []
        for entry in os.listdir(model_dir):
            stem, suffix = os.path.splitext(entry)
            if suffix == ext and stem.isdigit():
                found.append((int(stem), stem))
        if not found:
            raise FileNotFoundError('no <step>%s checkpoint in %s' % (ext, model_dir))
        step, stem = max(found)
    else:
        stem = str(step)
    base = os.path.join(model_dir, stem)
    path = base + ext
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    if logger is not None:
        logger('load %s.*' % base)
    epoch = None
    if os.path.exists(base + ext_epoch):
        with open(base + ext_epoch) as f:
            text = f.read().strip()
        try:
            epoch = int(text)
        except ValueError:
            pass
    return path, step, epoch
