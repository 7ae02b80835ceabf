"""`utils.iou.numpy` — the reference's numpy IoU of two boxes (utils/iou/numpy.py:iou), which `dimension_cluster.distance` is built on.

Boxes are (y, x) minimum and maximum corners; arrays broadcast, and the last axis holds the two coordinates.  The union is clamped from below at
`min`, by default the machine epsilon of the inputs' dtype.  The operation order here is the one include/yolo2_hip.h states for y2_anchor_kmeans
(csrc/kmeans.h: km_iou), so on float64 sizes this function and the library give the same bits."""
import numpy as np


def iou(yx_min1, yx_max1, yx_min2, yx_max2, min=None):
    yx_min1, yx_max1, yx_min2, yx_max2 = (np.asarray(a) for a in (yx_min1, yx_max1, yx_min2, yx_max2))
    assert np.all(yx_min1 <= yx_max1)
    assert np.all(yx_min2 <= yx_max2)
    if min is None:
        min = np.finfo(yx_min1.dtype).eps
    size = np.maximum(0.0, np.minimum(yx_max1, yx_max2) - np.maximum(yx_min1, yx_min2))
    intersect_area = size[..., 0] * size[..., 1]
    size1, size2 = yx_max1 - yx_min1, yx_max2 - yx_min2
    area1, area2 = size1[..., 0] * size1[..., 1], size2[..., 0] * size2[..., 1]
    union_area = np.maximum((area1 + area2) - intersect_area, min)
    return intersect_area / union_area
