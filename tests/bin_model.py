"""Plain model of one depth phase's binning (csrc/render.hip: bin_kernel COUNT -> scan -> EMIT; csrc/tile_test.hpp), numpy and
Python only, no GPU code and no wave: for every splat of the phase window, in depth order, the candidates of its rectangle
row-major, each kept or not.  The pair arrays that come out are fully ordered, so a comparison with them is bit for bit.

    window      j in [nvis // div0 (0 when div0 == 0), nvis // div1), i = by_depth[j], slot j - j0 of the phase
    candidates  the tiles of i's rectangle, or with bin32 the 32x32 bins (2x2 tiles) it meets, row-major
    kept iff    bin32: the mask of the bin's tiles inside the rectangle, less those whose `sat` byte is non-zero, is not empty;
                exact: the rectangle has one candidate, or min q over the rectangle of the tile's pixel centres is <= 4.04 (fp64;
                       a NaN keeps the tile);
                no bin32: the tile's `sat` byte is 0
    pair        key = ty * lists_x + tx (lists_x = bins or tiles per row), value = i | mask << 28
"""
import numpy as np

TILE = 16
EMPTY_RECT = 1              # tx0 = 1 > tx1 = 0: covers no tile (kEmptyRect)
Q_KEEP = 4.04               # tile_touches keeps a tile iff the minimum of q over it is <= 4.04
BAND = 1.0e-3 * Q_KEEP      # |q - 4.04| below which fp32 and fp64 may decide differently: no case may have a candidate in it
FF = np.uint32(0xFFFFFFFF)


def pack_rect(tx0, tx1, ty0, ty1):
    return int(tx0) | int(tx1) << 8 | int(ty0) << 16 | int(ty1) << 24


def unpack_rect(r):
    r = int(r)
    return r & 255, (r >> 8) & 255, (r >> 16) & 255, r >> 24


def rect_area(r, bin32=False):
    """candidates of a rectangle: its tiles, or the bins it meets"""
    tx0, tx1, ty0, ty1 = unpack_rect(r)
    if tx1 < tx0 or ty1 < ty0:
        return 0
    sh = 1 if bin32 else 0
    return ((tx1 >> sh) - (tx0 >> sh) + 1) * ((ty1 >> sh) - (ty0 >> sh) + 1)


def tile_box(cx, cy, H, tx, ty):
    """(x0, x1, y0, y1): the rectangle of the tile's pixel centres relative to the splat centre, GL window coordinates (y up)"""
    x0 = tx * TILE + 0.5 - cx
    y1 = H - (ty * TILE + 0.5) - cy
    return x0, x0 + 15.0, y1 - 15.0, y1


def rect_min_q(cx, cy, g0, g1, H, tx, ty, reverse=False):
    """fp64 minimum of q(d) = (d.g0)^2 + (d.g1)^2 = a x^2 + 2 b x y + c y^2 over the tile's rectangle of pixel centres: 0 with the
    centre inside, else the least of the four edge minima - on an edge q is a parabola in the free coordinate, its vertex clamped
    to the edge; where the parabola is flat (a or c = 0: neither axis has a component along the edge) any point serves.
    `reverse` walks the edges in the opposite order: the result may not depend on it.  NaN if an axis holds one."""
    cx, cy, H = float(cx), float(cy), float(H)
    g = [float(v) for v in (g0[0], g0[1], g1[0], g1[1])]
    if any(np.isnan(v) for v in g):
        return float("nan")
    x0, x1, y0, y1 = tile_box(cx, cy, H, tx, ty)
    if x0 <= 0.0 <= x1 and y0 <= 0.0 <= y1:
        return 0.0
    a = g[0] * g[0] + g[2] * g[2]
    b = g[0] * g[1] + g[2] * g[3]
    c = g[1] * g[1] + g[3] * g[3]
    q = lambda x, y: (x * g[0] + y * g[1]) ** 2 + (x * g[2] + y * g[3]) ** 2

    def along_x(y):
        return q(min(max(-b * y / a, x0), x1) if a > 0.0 else x0, y)

    def along_y(x):
        return q(x, min(max(-b * x / c, y0), y1) if c > 0.0 else y0)

    edges = [lambda: along_x(y0), lambda: along_x(y1), lambda: along_y(x0), lambda: along_y(x1)]
    best = float("inf")
    for e in (reversed(edges) if reverse else edges):
        best = min(best, e())
    return best


def exact_keeps(rec_i, H, tx, ty):
    """the exact test's verdict on one tested candidate: rec_i = (cx, cy, g0x, g0y, g1x, g1y, ..)"""
    q = rect_min_q(rec_i[0], rec_i[1], rec_i[2:4], rec_i[4:6], H, tx, ty)
    return not (q > Q_KEEP)


class Binned:
    """count (m_cap,), total, keys / vals (total,) in emission order; per slot `area` (candidates), per pair `rel` (its slot of the
    phase) and `local` (its candidate's rank in the rectangle) to name a mismatch by"""

    def __init__(self, count, area, keys, vals, rel, local):
        self.count, self.area = count, area
        self.total = int(count.astype(np.int64).sum())
        self.keys, self.vals, self.rel, self.local = keys, vals, rel, local

    def buffers(self, pair_cap):
        """the pair arrays as the hook returns them: 0xFF where nothing was written; nothing is written unless the total fits"""
        keys, vals = np.full(pair_cap, FF, np.uint32), np.full(pair_cap, FF, np.uint32)
        if self.total <= pair_cap:
            keys[:self.total], vals[:self.total] = self.keys, self.vals
        return keys, vals


def window(nvis, div0, div1):
    return (nvis // div0 if div0 else 0), nvis // div1


def splat_pairs(i, rect, rec, H, tiles_x, bin32, exact, sat):
    """(keys, vals, local) of splat i: its kept candidates, row-major"""
    tx0, tx1, ty0, ty1 = unpack_rect(rect)
    if tx1 < tx0 or ty1 < ty0:
        return (np.zeros(0, np.uint32),) * 3
    sh = 1 if bin32 else 0
    lists_x = (tiles_x + 1) // 2 if bin32 else tiles_x
    ty, tx = np.meshgrid(np.arange(ty0 >> sh, (ty1 >> sh) + 1), np.arange(tx0 >> sh, (tx1 >> sh) + 1), indexing="ij")
    ty, tx = ty.ravel(), tx.ravel()
    lst = ty * lists_x + tx
    keep = np.ones(len(lst), bool)
    mask = np.zeros(len(lst), np.int64)
    if bin32:
        sat4 = None if sat is None else np.asarray(sat, np.uint8).reshape(-1, 4)
        for dy in (0, 1):
            for dx in (0, 1):
                x, y = 2 * tx + dx, 2 * ty + dy
                inside = (x >= tx0) & (x <= tx1) & (y >= ty0) & (y <= ty1)
                if sat4 is not None:
                    inside &= sat4[lst, 2 * dy + dx] == 0
                mask |= inside.astype(np.int64) << (2 * dy + dx)
        keep &= mask != 0
    if exact and len(lst) > 1:
        keep &= np.array([exact_keeps(rec[i], H, int(x), int(y)) for x, y in zip(tx, ty)])
    if not bin32 and sat is not None:
        keep &= np.asarray(sat, np.uint8)[lst] == 0
    local = np.nonzero(keep)[0]
    return lst[keep].astype(np.uint32), (i | mask[keep] << 28).astype(np.uint32), local.astype(np.uint32)


def bin_phase(rect, rec, by_depth, nvis, div0, div1, m_cap, H, tiles_x, tiles_y, bin32=False, exact=False, sat=None):
    j0, j1 = window(nvis, div0, div1)
    count, area = np.zeros(m_cap, np.uint32), np.zeros(m_cap, np.uint32)
    keys, vals, rels, locs = [], [], [], []
    for j in range(j0, j1):
        i = int(by_depth[j])
        k, v, l = splat_pairs(i, rect[i], rec, H, tiles_x, bin32, exact, sat)
        count[j - j0], area[j - j0] = len(k), rect_area(rect[i], bin32)
        keys.append(k), vals.append(v), locs.append(l), rels.append(np.full(len(k), j - j0, np.int64))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return Binned(count, area, cat(keys, np.uint32), cat(vals, np.uint32), cat(rels, np.int64), cat(locs, np.int64))


def where_is(b, p):
    """slot p of the pair arrays -> (slot of the phase, wave, lane, round of the wave's walk) of the pair the model puts there"""
    rel = int(b.rel[p])
    wave = rel // 64
    start = int(b.area[wave * 64:rel].astype(np.int64).sum())
    return rel, wave, rel % 64, (start + int(b.local[p])) // 64
