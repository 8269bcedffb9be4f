"""The association rule of include/gsx.h (gsx_assoc_*) in integer numpy: the specification the GPU path is held to, exactly.

A run keeps gid[n] (int32, -1 = no instance yet), G and a dropped counter.  A view is fed as the per-Gaussian CAMERA pixel
(x, y) of the vote's projection, x = -1 where the view does not see the Gaussian (oracle.project_many, Context.project_all),
the map and the image size; the model does the vote's scale, truncation and clamp onto the map itself (dls.py:270-286).
"""
import math

import numpy as np

ONE_SHIFT = 20
MAX_SEGMENTS, MAX_INSTANCES = 254, 255


class RangeError(ValueError):
    pass


def decide(table, G, M, q, min_size):
    """Rule 3 on a (S + 1, M + 1) table -> (remap int32 (S,), G, dropped by this view).  Python integers throughout."""
    table = np.asarray(table)
    S = table.shape[0] - 1
    assert table.shape[1] == M + 1
    size = [int(table[b].sum()) for b in range(S + 1)]
    remap = np.full(S, -1, np.int32)
    taken, dropped = set(), 0
    for b in sorted(range(1, S + 1), key=lambda b: (-size[b], b)):
        if size[b] < min_size or size[b] == 0:
            continue
        best, g = 0, -1
        for k in range(G):
            if k not in taken and int(table[b, k + 1]) > best:      # strictly larger: of equal counts the lowest g stays
                best, g = int(table[b, k + 1]), k
        if g >= 0 and (best << ONE_SHIFT) >= q * size[b]:
            remap[b - 1] = g
            taken.add(g)
        elif G < M:
            remap[b - 1] = G
            taken.add(G)
            G += 1
        else:
            dropped += 1
    return remap, G, dropped


def sample(x, y, seg_w, seg_h, img_w, img_h):
    """camera pixel -> map pixel (dls.py:270-286): scale in fp64, truncate, clamp; only where x >= 0"""
    vis = np.asarray(x) >= 0
    xs = np.trunc(np.asarray(x, np.float64) * (float(seg_w) / float(img_w)))
    ys = np.trunc(np.asarray(y, np.float64) * (float(seg_h) / float(img_h)))
    xs = np.minimum(xs, seg_w - 1).astype(np.int64)
    ys = np.minimum(ys, seg_h - 1).astype(np.int64)
    return vis, np.where(vis, xs, 0), np.where(vis, ys, 0)


class Run:
    def __init__(self, n, max_segments, max_instances, min_overlap=0.3, min_size=1):
        assert 1 <= max_segments <= MAX_SEGMENTS and 1 <= max_instances <= MAX_INSTANCES
        assert 0.0 <= min_overlap <= 1.0 and min_size >= 1
        self.S, self.M = int(max_segments), int(max_instances)
        self.q = int(math.ceil(min_overlap * (1 << ONE_SHIFT)))
        self.min_size = int(min_size)
        self.gid = np.full(n, -1, np.int32)
        self.G = self.dropped = self.views = 0
        self.table = np.zeros((self.S + 1, self.M + 1), np.uint32)

    def view(self, x, y, seg, image_size=None):
        """-> (remap int32 (S,), relabelled map int32).  A value outside [-1, S - 1] raises RangeError and changes nothing."""
        seg = np.asarray(seg).astype(np.int64)
        h, w = seg.shape
        if seg.min() < -1 or seg.max() > self.S - 1:
            raise RangeError(f"map value outside [-1, {self.S - 1}]")
        iw, ih = (w, h) if image_size is None else image_size
        vis, xs, ys = sample(x, y, w, h, iw, ih)
        b = np.where(vis, seg[ys, xs] + 1, 0)
        table = np.zeros((self.S + 1, self.M + 1), np.int64)
        np.add.at(table, (b[vis], self.gid[vis].astype(np.int64) + 1), 1)
        remap, self.G, d = decide(table, self.G, self.M, self.q, self.min_size)
        self.dropped += d
        new = np.where(b >= 1, remap[np.maximum(b, 1) - 1], -1)
        take = vis & (new >= 0) & (self.gid == -1)
        self.gid[take] = new[take]
        self.table = table.astype(np.uint32)
        self.views += 1
        out = np.where(seg >= 0, remap[np.maximum(seg, 0)], -1).astype(np.int32)
        return remap, out


def same_partition(a, b):
    """two labelings describe the same partition: a bijection between their values maps one onto the other"""
    a, b = np.asarray(a), np.asarray(b)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len({p[0] for p in pairs}) == len({p[1] for p in pairs})
