"""`utils.visualize` — DrawBBox under the reference's name (utils/visualize.py:35-62), without cv2: rectangle outlines by numpy slicing.

It draws NO text: the reference writes the class name with cv2.putText, and there is no font renderer without cv2.  The class shows as the
rectangle's colour instead - one colour per class (the reference cycles its colours over the detections)."""
import numpy as np


def palette(n, seed=0):
    """n distinct-ish BGR colours from a fixed seed: the same class has the same colour in every run."""
    rng = np.random.RandomState(seed)
    return [tuple(int(v) for v in rng.randint(64, 256, 3)) for _ in range(n)]


def parse_color(color):
    """A colour name or '#rrggbb' (Pillow's ImageColor) or an (r, g, b) triple -> a BGR tuple of 0 .. 255, the channel order of the pictures."""
    if isinstance(color, str):
        from PIL import ImageColor
        color = ImageColor.getrgb(color)
    r, g, b = (int(v) for v in color[:3])
    return (b, g, r)


class DrawBBox(object):
    """DrawBBox(category, colors=[], thickness=3)(image, yx_min, yx_max, cls): the outline of every box, `thickness` pixels wide and grown inwards
    from the box's corners, clipped to the image, in the colour of its class - colors[cls % len(colors)] of the given list, or of a fixed seeded
    palette with one entry per category.  `image` (uint8 [h, w, 3], BGR) is drawn on in place and returned; the corners are integer pixels,
    inclusive."""

    def __init__(self, category, colors=[], thickness=3):
        self.category = category
        self.colors = [parse_color(c) for c in colors] if len(colors) else palette(max(len(category), 1))
        self.thickness = max(int(thickness), 1)

    def __call__(self, image, yx_min, yx_max, cls=None):
        h, w = image.shape[:2]
        t = self.thickness
        if cls is None:
            cls = [0] * len(yx_min)
        for (ymin, xmin), (ymax, xmax), c in zip(np.asarray(yx_min).tolist(), np.asarray(yx_max).tolist(), np.asarray(cls).tolist()):
            ymin, xmin, ymax, xmax = int(ymin), int(xmin), int(ymax), int(xmax)
            if ymax < ymin or xmax < xmin:
                continue
            color = self.colors[int(c) % len(self.colors)]
            y0, y1, x0, x1 = max(ymin, 0), min(ymax + 1, h), max(xmin, 0), min(xmax + 1, w)          # the box, clipped (rows y0:y1, columns x0:x1)
            if y0 >= y1 or x0 >= x1:
                continue
            # the four sides, each cut to the clipped box: a side that lies outside the image is not drawn
            for ya, yb, xa, xb in ((ymin, ymin + t, xmin, xmax + 1), (ymax + 1 - t, ymax + 1, xmin, xmax + 1),
                                   (ymin, ymax + 1, xmin, xmin + t), (ymin, ymax + 1, xmax + 1 - t, xmax + 1)):
                ya, yb, xa, xb = max(ya, y0), min(yb, y1), max(xa, x0), min(xb, x1)
                if ya < yb and xa < xb:
                    image[ya:yb, xa:xb] = color
        return image
