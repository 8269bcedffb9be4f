"""numpy model of the class-map producer (csrc/segmap.hip): arg-max over the channels, OpenCV's nearest resize, the instance
compositing of process_yolo_segmentation (the reference's deep_learning_segmentation.py:85-124, 142-144).

The resize rule is restated from OpenCV's source (resizeNN: `ifx = 1. / fx`, `sx = min(cvFloor(x * ifx), ssize.width - 1)` with
fx = (double)dsize.width / ssize.width): cv2 is not installed where this project is built, so the rule cannot be executed
against.  Everything else is pinned by running the reference (tools/make_golden_segmap.py -> tests/golden/segmap.npz)."""
import math

import numpy as np


# ---- the three nearest-neighbour rules -----------------------------------------------------------------------------------------
def nearest_index(S, D):
    """int64 (D,): source index of every destination index, S source -> D destination pixels, OpenCV's rule: double, two
    roundings (the quotient D / S, then its reciprocal), one product per pixel"""
    inv = 1.0 / (float(D) / float(S))
    return np.minimum(np.floor(np.arange(D, dtype=np.float64) * inv).astype(np.int64), S - 1)


def nearest_index_scalar(S, D):
    """the same rule as a scalar loop over Python floats (IEEE doubles)"""
    fx = float(D) / float(S)
    ifx = 1.0 / fx
    return [min(int(math.floor(d * ifx)), S - 1) for d in range(D)]


def nearest_index_exact(S, D):
    """floor(d * S / D) in integers - NOT the reference's rule"""
    return np.minimum(np.arange(D, dtype=np.int64) * S // D, S - 1)


def nearest_index_torch(S, D):
    """torch's legacy 'nearest': floor(d * (float)S / D) in float32 - NOT the reference's rule"""
    scale = np.float32(S) / np.float32(D)
    return np.minimum(np.floor(np.arange(D, dtype=np.float32) * scale).astype(np.int64), S - 1)


def rules_disagree(S, D):
    """OpenCV's rule differs from BOTH other rules somewhere"""
    a = nearest_index(S, D)
    return bool((a != nearest_index_exact(S, D)).any() and (a != nearest_index_torch(S, D)).any())


def disagreeing_pairs(s_max=8, d_max=400):
    """[(S, D), ..] with S <= s_max, D <= d_max on which the three rules disagree, in order"""
    return [(S, D) for S in range(1, s_max + 1) for D in range(1, d_max + 1) if rules_disagree(S, D)]


def resize_nearest(a, width, height):
    """cv2.resize(a, (width, height), interpolation=cv2.INTER_NEAREST) of a 2-D array"""
    a = np.asarray(a)
    h, w = a.shape
    return a[nearest_index(h, height)][:, nearest_index(w, width)]


# ---- the two producers -----------------------------------------------------------------------------------------------------------
def argmax_channels(logits):
    """torch.argmax(dim=-3): the first index of the maximum, a NaN is the maximum and the first NaN wins, -0.0 == +0.0 -
    which is np.argmax.  logits (.., C, h, w), any numpy float dtype."""
    return np.argmax(np.asarray(logits), axis=-3)


def segmap_from_logits(logits, width, height):
    """int32 (height, width) or (n, height, width)"""
    low = argmax_channels(logits)
    if low.ndim == 2:
        return resize_nearest(low, width, height).astype(np.int32)
    return np.stack([resize_nearest(m, width, height) for m in low]).astype(np.int32)


def segmap_from_masks(masks, cls, conf, width, height):
    """the loop of process_yolo_segmentation (deep_learning_segmentation.py:101, 113-124): int32 (height, width)"""
    seg = np.full((height, width), -1, np.int32)
    K = 0 if masks is None else len(masks)
    for k in range(K):
        if np.float32(conf[k]) > 0.5:
            m = resize_nearest(np.asarray(masks[k]), width, height)
            seg = np.where(m > 0.5, np.float32(cls[k]), seg)
    return seg.astype(np.int32)
