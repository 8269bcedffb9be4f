"""fp64 model of the depth frames (include/gsx.h: gsx_depth_view; csrc/depthmap.hip), plain numpy, no GPU code.

Built on lift_model.tile_weights: per tile w = T * B of the tile's list in walk order (no epilogue).  A record's depth key is
runSort's, stated as gs.js:437 states it - ((vp2 x + vp6 y + vp10 z) * 4096) | 0 on the float32 position - in numpy.  Per pixel:
    total  = sum of w                 moment = sum of w * key
    surface = the first list position whose running sum of w reaches cut / 2^20, cut = max(1, ceil(quantile * 2^20))
plus what the bounds of test_depthmap_gpu.py need, counted as labelmap_model counts it: P fragments with w > 0, M records whose
box holds the pixel where the pixel lies in BlendModel.mask, max |key| over the tile's list - and `decided`: the pixels whose
surface no kernel within the bound can place elsewhere.  And the integer rule itself on integer weights (`rule`)."""
import functools
import math

import numpy as np

import blend_cases
import lift_model
import oracle
from blend_model import E4
from lift_model import ONE


def cut_of(quantile):
    return max(1, int(math.ceil(quantile * ONE)))


def keys(scene, model):
    """runSort's int32 depth key per record, importance order (gs.js:436-441 on the float32 positions of the buffer)"""
    vp = oracle.multiply4(oracle.proj_matrix(scene.cam["fx"], scene.cam["fy"], scene.W, scene.H), oracle.view_matrix(scene.cam))
    xyz = scene.arrays()[0][np.asarray(model.rec.order)].astype(np.float64)
    d = (vp[2] * xyz[:, 0] + vp[6] * xyz[:, 1] + vp[10] * xyz[:, 2]) * 4096.0
    assert np.abs(d).max() < 2.0 ** 31                                    # `| 0` truncates, nothing wraps
    return np.trunc(d).astype(np.int64)


def pair_tol(tol, bitwise):
    """what one fragment may be off by: the scene's frame tolerance, the rounding of one q, and - where tiles reach the
    opacity cut - what the kernel leaves out"""
    return tol + 2.0 ** -21 + (0.0 if bitwise else 1.0e-5)


class Depth:
    pass


def frame(model, key, quantile, tol, alpha_max, bitwise):
    """-> Depth with (H, W) arrays: total, moment (float64), index (importance row of the surface, -1: none), P, M, kmax
    (max |key| over the tile's list, 0 without one), bound (on |moment / 2^20 - model|), decided, listed (the tile has a list),
    faint (the sum of w over all but the last list position: what stands in front of a tile's last record)"""
    H, W = model.H, model.W
    out = Depth()
    out.total, out.moment, out.faint = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    out.index = np.full((H, W), -1, np.int64)
    out.P, out.M = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    out.kmax = np.zeros((H, W))
    out.decided = np.ones((H, W), bool)
    out.listed = np.zeros((H, W), bool)
    cut = cut_of(quantile) / ONE
    per = pair_tol(tol, bitwise)
    for t, ids in enumerate(model.lists):
        if len(ids) == 0:
            continue
        ys, xs, inside = model.tile_pixels(t)
        w = lift_model.tile_weights(model, t)                             # (L, 16, 16), 0 outside the frame
        box = np.asarray([model.rec.box[i] for i in ids], np.int64).reshape(len(ids), 4)
        x0, x1, r0, r1 = (box[:, j, None, None] for j in range(4))
        inbox = inside[None] & (xs[None] >= x0) & (xs[None] <= x1) & (ys[None] >= r0) & (ys[None] <= r1)
        assert (w[~inbox] == 0.0).all()
        yy, xx = np.minimum(ys, H - 1), np.minimum(xs, W - 1)
        near = inbox & model.mask[yy, xx][None]                           # a fragment fp32 and fp64 may disagree on
        k = key[ids].astype(np.float64)[:, None, None]
        run = np.cumsum(w, 0)
        Pk, Mk = np.cumsum(w > 0, 0), np.cumsum(near, 0)
        bound_k = Pk * per + Mk * (alpha_max * E4)
        reached = run >= cut
        first = np.where(reached.any(0), reached.argmax(0), -1)
        # decided: at every position that has, or may have, a fragment the running sum stays clear of the cut by its bound
        open_ = ((w > 0) | near) & (np.abs(run - cut) <= bound_k)
        sel = inside
        out.total[ys[sel], xs[sel]] = run[-1][sel]
        out.moment[ys[sel], xs[sel]] = (w * k).sum(0)[sel]
        out.faint[ys[sel], xs[sel]] = (run[-2] if len(ids) > 1 else np.zeros((16, 16)))[sel]
        out.index[ys[sel], xs[sel]] = np.where(first >= 0, ids[np.maximum(first, 0)], -1)[sel]
        out.P[ys[sel], xs[sel]] = Pk[-1][sel]
        out.M[ys[sel], xs[sel]] = Mk[-1][sel]
        out.kmax[ys[sel], xs[sel]] = np.abs(key[ids]).max()
        out.decided[ys[sel], xs[sel]] = ~open_.any(0)[sel]
        out.listed[ys[sel], xs[sel]] = True
    out.bound = (out.P * per + out.M * (alpha_max * E4)) * out.kmax
    return out


@functools.lru_cache(maxsize=None)
def case_frame(name, quantile=0.5):
    """the model's depth frame of one blend case, shared by every test of a session"""
    p = blend_cases.prepared(name)
    return frame(p.model, keys(p.scene, p.model), quantile, p.tol, p.alpha_max, blend_cases.bitwise(name))


# ---- constructed scenes ---------------------------------------------------------------------------------------------------
BORDER_L = (1, 255, 256, 257, 512, 513)
WALL_TAGS = {"faint": 0, "discs": 1, "loud": 2, "walls": 3}


class Border:
    """one 16x16 tile whose list is L - 1 faint records (alpha 1/255 .. 4/255, reach ~1.3 px, spread over the tile) followed by
    one opaque splat that fills the frame (axes at the 1024-px cap, as blend_cases.walls'): the staged chunks of 256 end one
    record before, on and one record after the surface.  `opaque`: its upload row."""

    def __init__(self, L):
        rng = np.random.default_rng(20281 + L)
        self.L = L
        self.scene = sc = blend_cases.Scene(f"border_{L}", 16, 16)
        for _ in range(L - 1):
            sc.add(rng.uniform(1.5, 14.5), rng.uniform(1.5, 14.5), rng.uniform(3.0, 3.9), 0.45 * rng.uniform(0.95, 1.05, 3),
                   blend_cases.unit_quat(rng), int(rng.integers(1, 5)), rng.integers(0, 256, 3))
        self.opaque = sc.add(8.6, 8.5, 4.0, (30.0 * sc.f / 4.0,) * 3, (1, 0, 0, 0), 255, (200, 120, 30))
        blend_cases.add_sink(sc)


@functools.lru_cache(maxsize=None)
def border(L):
    return Border(L)


@functools.lru_cache(maxsize=None)
def border_model(L):
    import blend_model
    return blend_model.BlendModel(*border(L).scene.args())


def wall_labels(scene):
    """walls_*: labels in upload order from meta["tags"]: faint 0, discs 1, loud 2, walls 3, anything else (the sink) -1"""
    labels = np.full(len(scene.xyz), -1, np.int32)
    for faint, discs, loud in scene.meta["tags"].values():
        labels[faint], labels[discs], labels[loud] = WALL_TAGS["faint"], WALL_TAGS["discs"], WALL_TAGS["loud"]
    labels[scene.meta["walls"]] = WALL_TAGS["walls"]
    return labels


def centre_px(scene, i):
    """(u, v): where upload row i's centre projects, in pixels, v from the top (Scene.add's inverse)"""
    x, y, z = scene.xyz[i]
    return x * scene.f / z + scene.W / 2, y * scene.f / z + scene.H / 2


def behind_the_walls(sc, d, order):
    """per ordinary tile of a walls scene that has one: the upload row of a loud record whose centre lies on a decided pixel
    whose surface is one of the shared walls; order: importance row -> upload row"""
    out = {}
    for t, (_, _, ids) in sc.meta["tags"].items():
        for i in ids if t != sc.meta["hole"] and t not in sc.meta["cut"] else ():
            u, v = centre_px(sc, i)
            if d.decided[int(v), int(u)] and d.index[int(v), int(u)] >= 0 and order[d.index[int(v), int(u)]] in sc.meta["walls"]:
                out[t] = i
                break
    return out


def rule(q, key, row, quantile):
    """the integer rule on one pixel column of fragments in walk order: q (L, ...) non-negative integers, key and row (L,)
    -> total, moment (Python-integer exact: object arrays), surface_key, surface_index"""
    q = np.asarray(q).astype(np.int64)
    L = len(q)
    shape = q.shape[1:]
    k = np.asarray(key, np.int64).reshape((L,) + (1,) * len(shape))
    total = q.sum(0)
    moment = (q * k).sum(0)                                               # |q k| < 2^52 per term, a handful of terms: exact in int64
    reached = np.cumsum(q, 0) >= cut_of(quantile)
    hit = reached.any(0) if L else np.zeros(shape, bool)
    first = reached.argmax(0) if L else np.zeros(shape, np.int64)
    skey = np.where(hit, np.asarray(key, np.int64)[first] if L else 0, 0)
    srow = np.where(hit, np.asarray(row, np.int64)[first] if L else 0, -1)
    return total.astype(np.uint32), moment, skey.astype(np.int32), srow.astype(np.int32)
