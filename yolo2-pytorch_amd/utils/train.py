"""`utils.train` — load_model under the reference's name (utils/train.py:51-76): which checkpoint of a model directory to read.

A model directory holds `<step>.pth` (a state_dict) beside `<step>.epoch` (the epoch as text), as convert_darknet_torch.py and the reference's Saver
write them."""
import logging
import os


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
