"""Numpy model of the IoU evaluation (Image_Segmentation/evaluation.py of the reference, "ev.py"), written from its semantics:
a pixel is set iff value != 0 (ev.py:29-30), counts are integers, the quotient is one float64 division (ev.py:35).  Our own
code; tests compare it with the fixture the reference wrote (tests/golden/iou.npz) and the GPU path with both."""
import numpy as np


def set_pixels(a):
    """bool array: value != 0 on the whole element (NaN, inf, denormals set; -0.0 not)"""
    return np.asarray(a) != 0


def inter_area(masks, gts):
    """(inter int64 (M, G), area_masks int64 (M,), area_gt int64 (G,))"""
    m = np.stack([set_pixels(x).ravel() for x in masks]).astype(np.int64)
    g = np.stack([set_pixels(x).ravel() for x in gts]).astype(np.int64)
    return m @ g.T, m.sum(1), g.sum(1)


def iou_from_counts(inter, area_a, area_b):
    inter = np.asarray(inter, np.int64)
    union = np.asarray(area_a, np.int64) + np.asarray(area_b, np.int64) - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter.astype(np.float64) / union.astype(np.float64)


def iou(masks, gts):
    """float64 (M, G); NaN where both are empty"""
    inter, am, ag = inter_area(masks, gts)
    return iou_from_counts(inter, am[:, None], ag[None, :])


def best(iou_mg):
    """ev.py:44-54 -> (best float64 (M,), gt_idx int32 (M,)): strict '>' from (0, 0)"""
    iou_mg = np.asarray(iou_mg, np.float64)
    out_b, out_i = np.zeros(len(iou_mg), np.float64), np.zeros(len(iou_mg), np.int32)
    for m, row in enumerate(iou_mg):
        for i, v in enumerate(row):
            if v > out_b[m]:
                out_b[m], out_i[m] = v, i
    return out_b, out_i


def top_index(masks):
    """int32 (H, W): highest list index whose mask is set, or -1 (ev.py:65-67: the last mask drawn owns the pixel)"""
    out = np.full(np.asarray(masks[0]).shape, -1, np.int32)
    for i, m in enumerate(masks):
        out[set_pixels(m)] = i
    return out


def table(pred, gt, n_pred_classes, n_gt_classes, packed_u8=False):
    """int64 (P + 1, G + 1): pixels with pred bin a and gt bin b, bin = label + 1"""
    off = 0 if packed_u8 else 1
    a = np.asarray(pred).astype(np.int64).ravel() + off
    b = np.asarray(gt).astype(np.int64).ravel() + off
    assert a.min() >= 0 and a.max() <= n_pred_classes and b.min() >= 0 and b.max() <= n_gt_classes
    flat = np.bincount(a * (n_gt_classes + 1) + b, minlength=(n_pred_classes + 1) * (n_gt_classes + 1))
    return flat.reshape(n_pred_classes + 1, n_gt_classes + 1).astype(np.int64)


def iou_from_table(t):
    t = np.asarray(t, np.int64)
    return iou_from_counts(t, t.sum(-1, keepdims=True), t.sum(-2, keepdims=True))


def reference_loop(masks, gts):
    """The reference's arithmetic pair by pair (ev.py:29-35, 46-54), for timing: four full-frame numpy passes per pair, on
    private copies as the in-place edit demands.  Returns [(max_iou, gt_idx)]."""
    masks = [np.array(m) for m in masks]
    gts = [np.array(g) for g in gts]
    out = []
    for mask in masks:
        max_iou, gt_idx = 0, 0
        for i, gt in enumerate(gts):
            mask[np.where(mask != 0)] = 1
            gt[np.where(gt != 0)] = 1
            intersection = np.logical_and(mask, gt).astype(int)
            union = np.logical_or(mask, gt).astype(int)
            with np.errstate(invalid="ignore"):
                v = np.sum(intersection) / np.sum(union)
            if v > max_iou:
                max_iou, gt_idx = v, i
        out.append((max_iou, gt_idx))
    return out
