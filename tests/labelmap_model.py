"""fp64 model of the label frames (include/gsx.h: gsx_label_view; csrc/labelmap.hip), plain numpy, no GPU code.

The transpose of lift_model: per tile lift_model.tile_weights gives w = T * B of the tile's list (no epilogue), and where the
lift scatters w by the pixel's class into table[splat][class], this model scatters it by the splat's label into
planes[label + 1][pixel].  Per (bin, pixel) it also returns P, the number of fragments with w > 0 that fed the entry, and M, the
number of records of that bin whose box holds the pixel, counted where the pixel lies in BlendModel.mask (|q - 4| < 1e-4 lets
fp32 and fp64 disagree on `discard` there).  Plus the integer rule on integer planes, the label patterns the tests use, and the
count of list walks the kernel makes.  Planes are kept for the bins 0 .. n_classes only: every bin beyond holds nothing."""
import functools
import math

import numpy as np

import blend_cases
import lift_model
from blend_model import E4
from lift_model import ONE


class Planes:
    def __init__(self, planes, P, M):
        self.planes, self.P, self.M = planes, P, M


def packed_bins(model, labels):
    """labels in upload order -> bin = label + 1 per record in importance order, as the model keeps its records"""
    return np.asarray(labels, np.int64)[np.asarray(model.rec.order)] + 1


def tile_scatter(model, t, bins, w):
    """the index arrays that scatter tile t's (L,16,16) values into (bin, row, column), and the mask of the (record, pixel)
    pairs inside the frame and inside the record's box"""
    ids = model.lists[t]
    ys, xs, inside = model.tile_pixels(t)
    box = np.asarray([model.rec.box[i] for i in ids], np.int64).reshape(len(ids), 4)
    x0, x1, r0, r1 = (box[:, j, None, None] for j in range(4))
    inbox = inside[None] & (xs[None] >= x0) & (xs[None] <= x1) & (ys[None] >= r0) & (ys[None] <= r1)
    assert (w[~inbox] == 0.0).all()                                     # a fragment never falls outside its splat's box
    shape = inbox.shape
    b = np.broadcast_to(bins[ids][:, None, None], shape)[inbox]
    yy = np.broadcast_to(np.minimum(ys, model.H - 1)[None], shape)[inbox]
    xx = np.broadcast_to(np.minimum(xs, model.W - 1)[None], shape)[inbox]
    return (b, yy, xx), inbox


def planes(model, labels, n_classes, skip=None):
    """labels: ints in [-1, n_classes - 1], upload order.  skip: (tile, list position) of one record to leave out.  -> Planes with
    float64 planes and int32 P, M of shape (n_classes + 1, H, W)"""
    bins = packed_bins(model, labels)
    assert bins.shape == (model.rec.n,) and bins.min() >= 0 and bins.max() <= n_classes
    nb = n_classes + 1
    out = np.zeros((nb, model.H, model.W))
    P = np.zeros((nb, model.H, model.W), np.int32)
    M = np.zeros((nb, model.H, model.W), np.int32)
    for t, ids in enumerate(model.lists):
        if len(ids) == 0:
            continue
        w = lift_model.tile_weights(model, t, skip[1] if skip is not None and skip[0] == t else None)
        at, inbox = tile_scatter(model, t, bins, w)
        np.add.at(out, at, w[inbox])
        np.add.at(P, at, (w[inbox] > 0).astype(np.int32))
        np.add.at(M, at, model.mask[at[1], at[2]].astype(np.int32))
    return Planes(out, P, M)


def entry_bound(pl, tol, alpha_max, bitwise):
    """lift_model.cell_bound, term for term, per (bin, pixel): P fragments, each off by the frame tolerance of the scene and the
    rounding of one q (2^-21); M records on the `discard` threshold, each moving at most alpha_max * e^-4; where tiles reach
    the opacity cut, what the kernel leaves out: below 1e-5 per pixel"""
    return pl.P * (tol + 2.0 ** -21 + (0.0 if bitwise else 1.0e-5)) + pl.M * (alpha_max * E4)


def threshold(min_weight):
    return max(1, int(math.ceil(min_weight * ONE)))


def finalize(planes_q, min_weight):
    """the rule of gsx_label_view on integer planes (bins, H, W) -> (label int32, weight uint32, total uint32)"""
    q = np.asarray(planes_q)
    assert q.dtype.kind == "u" and q.ndim == 3
    q = q.astype(np.uint64)
    total = q.sum(0)
    arg = q.argmax(0)                                                   # the first of equal maxima: the lowest bin wins a tie
    best = q.max(0)
    keep = total >= np.uint64(min(threshold(min_weight), 2 ** 63))
    return (np.where(keep, arg - 1, -1).astype(np.int32), np.where(keep, best, 0).astype(np.uint32), total.astype(np.uint32))


def passes(model, labels, window):
    """list walks label_kernel makes: ceil(D / window) per tile with a list, D = the label bins in the tile's list"""
    bins = packed_bins(model, labels)
    return sum(-(-len(np.unique(bins[ids])) // window) for ids in model.lists if len(ids))


def tile_bins(model, labels):
    """per tile: the number of label bins in its list (0: no list)"""
    bins = packed_bins(model, labels)
    return [len(np.unique(bins[ids])) if len(ids) else 0 for ids in model.lists]


# ---- the label patterns, in upload order ------------------------------------------------------------------------------------
def pattern_names(window):
    return ("one", "none", "parity", f"mod{window - 1}", f"mod{window}", f"mod{window + 1}", f"mod{2 * window + 1}", "mod255")


def pattern(name, n):
    """-> (labels int32 (n,), n_classes): `one` all 2, `none` all -1, `parity` (i % 2) * 2, modK i % K - 1; n_classes is the
    smallest that holds the pattern, 4 for the first three, and 255 for mod255 (its largest label is 253)"""
    i = np.arange(n)
    if name == "one":
        return np.full(n, 2, np.int32), 4
    if name == "none":
        return np.full(n, -1, np.int32), 4
    if name == "parity":
        return ((i % 2) * 2).astype(np.int32), 4
    K = int(name[3:])
    return (i % K - 1).astype(np.int32), 255 if K == 255 else max(K - 1, 1)


@functools.lru_cache(maxsize=None)
def case_planes(name, pat):
    """the model's planes of one blend case under one pattern, shared by every test of a session"""
    p = blend_cases.prepared(name)
    labels, C = pattern(pat, p.model.rec.n)
    return planes(p.model, labels, C)
