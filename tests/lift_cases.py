"""Class maps placed on the structural edges of lift_kernel (csrc/lift.hip), shared by test_lift_model.py (CPU: the cases are
what they claim and every edge carries weight) and test_lift_edges_gpu.py.  Everything is derived from gsx.lift_constants():
K["cells"] LDS accumulators, K["chunk"] staged records, K["loop_max"] classes a mixed wave still reduces per class.

A pattern is a 16 x 16 array of BINS (bin = label + 1); its map is the pattern repeated over the frame, cut at the border, minus
1.  A tile is four waves of four pixel rows.  For a tile with D bins present the kernel walks a chunk in rounds of
sub = min(chunk, cells // D) records; a wave whose pixels inside the frame hold 1 / 2..loop_max / more classes takes the
full-wave reduction / the per-class loop / per-lane LDS atomics.

Every pattern is a function f of a FINE map, pixel by pixel (pos256: every pixel of a tile its own bin; or the 255-class map of
lift_model.maps for the one pair that is not periodic in the tiles), and q = rint(w * 2^20) does not depend on the map: the
coarse table is the fine table with its columns summed by f, as integers (`coarsen`)."""
import numpy as np

TILE = 16
WAVES = 4               # per tile: wave w holds pixel rows 4 w .. 4 w + 3
WORD_EDGES = (0, 31, 32, 33, 63, 64, 95, 96, 127, 128, 159, 160, 191, 192, 224, 255)


def units(K):
    """(R, Lm): the largest D whose round is a whole chunk, and loop_max"""
    assert K["tile"] == TILE and K["chunk"] == TILE * TILE and K["cells"] % K["chunk"] == 0
    return K["cells"] // K["chunk"], K["loop_max"]


def sub_of(K, D):
    return min(K["chunk"], K["cells"] // D)


def path_of(K, count):
    return "none" if count == 0 else "uniform" if count == 1 else "loop" if count <= K["loop_max"] else "lanes"


class Pattern:
    """bins: 16x16 ints in [0, n_classes]; want = (D, per-wave class counts, sub) as the constants say they must come out (the
    CPU test computes them again from `bins` alone); fine: the pattern it is a function of; f = bins.ravel(): fine bin -> bin"""

    def __init__(self, name, bins, n_classes, want, holds, fine="pos256"):
        self.name, self.bins, self.n_classes, self.want, self.holds, self.fine = name, np.asarray(bins, np.int64), n_classes, want, holds, fine
        self.f = self.bins.reshape(-1)
        assert self.bins.shape == (TILE, TILE) and self.bins.min() >= 0 and self.bins.max() <= n_classes <= 255

    def map(self, W, H):
        reps = ((H + TILE - 1) // TILE, (W + TILE - 1) // TILE)
        return (np.tile(self.bins, reps)[:H, :W] - 1).astype(np.int32)


def structure(bins, K, inside=None):
    """from a tile's 16x16 bins alone (and the pixels inside the frame): D, the per-wave class counts, sub"""
    bins = np.asarray(bins)
    inside = np.ones((TILE, TILE), bool) if inside is None else inside
    D = len(np.unique(bins[inside]))
    waves = tuple(len(np.unique(bins[4 * w:4 * w + 4][inside[4 * w:4 * w + 4]])) for w in range(WAVES))
    return D, waves, sub_of(K, D)


def patterns(K):
    """name -> Pattern, pos256 first"""
    R, Lm = units(K)
    r, x = np.mgrid[0:TILE, 0:TILE]
    w = r // 4
    out = {}

    def put(name, bins, n_classes, D, waves, holds):
        out[name] = Pattern(name, bins, n_classes, (D, tuple(waves), sub_of(K, D)), holds)

    put("pos256", 16 * r + x, 255, 256, (64,) * 4, "the fine map: every bin, label -1 included; the shortest round")
    for j in (1, 2, Lm - 1, Lm, Lm + 1):
        put(f"wave_{j}", 1 + (r + x) % j, j, j, (j,) * 4,
            {1: "the full-wave reduction", Lm: "the loop path at its last count", Lm + 1: "the per-lane path at its first count"}.get(j, "the loop path"))
    assert Lm >= 2
    mixed = np.select([w == 0, w == 1, w == 2], [0 * r, 1 + (r + x) % 2, 3 + (r + x) % Lm], 3 + Lm + (r + x) % (Lm + 1))
    put("mixed_waves", mixed, 2 * Lm + 3, 2 * Lm + 4, (1, 2, Lm, Lm + 1), "all three paths write one round's cells; label -1 in the uniform wave")
    for N in (R, R + 1, 16, 100, 255):
        put(f"d_{N}", (16 * r + x) % N, N - 1, N, (min(N, 64),) * 4,        # a wave's pixels are 64 consecutive values of 16 r + x
            {R: "the last D with a whole-chunk round", R + 1: "the first D with a remainder round", 100: "a sub that does not divide the chunk",
             255: "sub = cells // 255"}.get(N, "per-lane path, sub a power of two"))
    last = R + 1 - 2 * (WAVES - 1)                                       # classes left for the fourth wave
    assert 2 <= last <= Lm, "d9_loop needs three waves of 2 classes and one of 2 .. loop_max"
    put(f"d{R + 1}_loop", np.where(w < 3, 2 * w + (r + x) % 2, 6 + (r + x) % last), R, R + 1, (2, 2, 2, last),
        "a remainder round with every wave on the loop path")
    put("word_edges", np.asarray(WORD_EDGES)[x], 255, 16, (16,) * 4, "rank256 at the word boundaries, bin 0 among them")
    for name in (f"wave_{Lm + 1}", "d_100"):                             # nbins enters only the addressing
        p = out[name]
        out[name + "_c255"] = Pattern(name + "_c255", p.bins, 255, p.want, p.holds + ", table 256 bins wide")
    return out


# ---- the pair that is not periodic in the tiles ---------------------------------------------------------------------------
HALVES_N = 22


def halves_f():
    """bin of the 255-class map -> bin: a modulus per quarter of the bin range (2, 3, 7, 11 classes, disjoint).  A tile of that
    map holds 121 consecutive bins (mod 255) starting at 16 tx + 112 ty, so neighbouring tiles see different quarters and hold
    different numbers of classes, on either side of cells // chunk."""
    b = np.arange(256)
    return np.select([b < 64, b < 128, b < 192], [b % 2, 2 + b % 3, 5 + b % 7], 12 + b % 11)


def halves_pair(W, H):
    """-> (fine map, 255), (coarse map, HALVES_N), f"""
    import lift_model
    fine, C = lift_model.maps(W, H)["c255"]
    f = halves_f()
    return (fine, C), ((f[fine + 1] - 1).astype(np.int32), HALVES_N), f


def tile_structures(seg, K):
    """per tile of an H x W map, row-major: (D, per-wave class counts over the pixels inside the frame, sub, inside mask)"""
    H, W = seg.shape
    out = []
    for ty in range((H + TILE - 1) // TILE):
        for tx in range((W + TILE - 1) // TILE):
            ys, xs = np.mgrid[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE]
            inside = (ys < H) & (xs < W)
            bins = np.where(inside, seg[np.minimum(ys, H - 1), np.minimum(xs, W - 1)] + 1, 0)
            out.append(structure(bins, K, inside) + (inside, bins))
    return out


def coarsen(table, f, nbins):
    """columns of a uint64 table summed by f: out[:, a] = sum of table[:, b] over f[b] == a, as integers"""
    table = np.asarray(table)
    assert table.dtype == np.uint64 and table.shape[1] <= len(f)
    out = np.zeros((len(table), nbins), np.uint64)
    for b in range(table.shape[1]):
        out[:, f[b]] += table[:, b]
    return out


def widen(table, nbins):
    """the same table with zero columns up to nbins"""
    out = np.zeros((len(table), nbins), np.uint64)
    out[:, :table.shape[1]] = table
    return out
