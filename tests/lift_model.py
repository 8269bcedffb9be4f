"""fp64 model of the lifting labeler (include/gsx.h: gsx_lift_*; csrc/lift.hip), plain numpy, no GPU code.

Built on blend_model.BlendModel.  Per tile: tile_terms -> B over the tile's list WITHOUT the epilogue's draws of splat 0,
T = cumprod(1 - B), w = T * B - the increment of the frame's alpha channel by that fragment - scattered by the class map into
an n x (C + 1) float64 table (rows in importance order as the model keeps its records; `upload_rows` turns them).  Per cell the
model also returns P, the number of (pixel, fragment) pairs that fed it, and M, the number of its pixels inside the splat's box
that lie in BlendModel.mask, where |q - 4| < 1e-4 lets fp32 and fp64 disagree on `discard`.  Plus the finalize rule on an
integer table, and the maps the tests lift."""
import math

import numpy as np

ONE = 1 << 20           # GSX_LIFT_ONE


class Lifted:
    def __init__(self, table, P, M, order):
        self.table, self.P, self.M, self.order = table, P, M, order

    def upload_rows(self, a):
        """an array whose rows are importance-order records -> rows in upload order"""
        out = np.zeros_like(a)
        out[self.order] = a
        return out


def tile_weights(model, t, skip=None):
    """(L, 16, 16) weights of the tile's list (no epilogue), pixels outside the frame zeroed; skip: a list position left out"""
    L = len(model.lists[t])
    _, B, _ = model.tile_terms(t)
    B = B[:L]
    if skip is not None:
        B = B.copy()
        B[skip] = 0.0
    T = np.cumprod(np.concatenate([np.ones((1,) + B.shape[1:]), 1.0 - B]), 0)[:-1]
    return T * B * model.tile_pixels(t)[2][None]


def lift(model, seg, n_classes, skip=None):
    """seg: H x W ints in [-1, n_classes - 1].  skip: (tile, list position) of one record to leave out.  -> Lifted"""
    seg = np.asarray(seg)
    assert seg.shape == (model.H, model.W) and seg.min() >= -1 and seg.max() < n_classes
    n, nb = model.rec.n, n_classes + 1
    table = np.zeros((n, nb))
    P = np.zeros((n, nb), np.int64)
    M = np.zeros((n, nb), np.int64)
    for t, ids in enumerate(model.lists):
        if len(ids) == 0:
            continue
        ys, xs, inside = model.tile_pixels(t)
        w = tile_weights(model, t, skip[1] if skip is not None and skip[0] == t else None)
        bins = np.where(inside, seg[np.minimum(ys, model.H - 1), np.minimum(xs, model.W - 1)] + 1, 0)
        near = np.where(inside, model.mask[np.minimum(ys, model.H - 1), np.minimum(xs, model.W - 1)], False)
        for k, i in enumerate(ids):
            x0, x1, r0, r1 = model.rec.box[i]
            box = inside & (xs >= x0) & (xs <= x1) & (ys >= r0) & (ys <= r1)
            np.add.at(table[i], bins[box], w[k][box])
            np.add.at(P[i], bins[box], (w[k][box] > 0).astype(np.int64))
            np.add.at(M[i], bins[box], near[box].astype(np.int64))
            assert w[k][~box].sum() == 0.0                      # a fragment never falls outside its splat's box
    return Lifted(table, P, M, np.asarray(model.rec.order))


def threshold(min_weight):
    return int(math.ceil(min_weight * ONE))


def finalize(table, min_weight):
    """the rule of gsx_lift_finalize on an integer table (rows in any order) -> labels int32, shares float64"""
    table = np.asarray(table)
    assert table.dtype == np.uint64
    thr = threshold(min_weight)
    labels = np.empty(len(table), np.int32)
    share = np.zeros(len(table))
    for i, row in enumerate(table):
        vals = [int(v) for v in row]
        total = sum(vals)
        best = max(vals)
        labels[i] = -1 if total < thr else vals.index(best) - 1          # index(): the lowest bin wins a tie
        share[i] = float(np.float64(best) / np.float64(total)) if total else 0.0
    return labels, share


# ---- the maps -----------------------------------------------------------------------------------------------------------
def maps(W, H):
    """name -> (map, n_classes): uniform, all -1, a 1-pixel checker (every wave mixed), 16x16 blocks on the tiles, blocks offset
    by 8 (a wave uniform, its tile not), and 255 classes in every tile"""
    r, x = np.mgrid[0:H, 0:W]
    return {
        "uniform": (np.full((H, W), 2, np.int32), 4),
        "none": (np.full((H, W), -1, np.int32), 4),
        "checker": (((r + x) % 2).astype(np.int32) * 2, 4),
        "blocks": ((((r // 16) * 3 + x // 16) % 5 - 1).astype(np.int32), 4),
        "offset8": (((((r + 8) // 16) * 3 + (x + 8) // 16) % 5 - 1).astype(np.int32), 4),
        "c255": (((x + 7 * r) % 255 - 1).astype(np.int32), 255),
    }


def cell_bound(lifted, tol, alpha_max, bitwise):
    """the GPU table's distance from the model, per cell, in units of weight: P pairs, each off by the frame tolerance of the
    scene and the rounding of one q (2^-21); M pixels where one fragment on the `discard` threshold may exist on one side
    only, each moving at most alpha_max * e^-4 within the cell; where tiles reach the opacity cut, what the kernel leaves out:
    below 1e-5 per pixel"""
    from blend_model import E4
    return lifted.P * (tol + 2.0 ** -21 + (0.0 if bitwise else 1.0e-5)) + lifted.M * (alpha_max * E4)
