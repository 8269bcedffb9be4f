"""Scenes and CPU-side conditions shared by tests/test_kmeans_gpu.py and tests/test_oracle_kmeans.py.  Plain numpy; the
reference of every comparison is oracle/kmeans_oracle.py."""
from fractions import Fraction

import numpy as np

SMALL_SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 19, 20, 21, 63, 64, 65]
STAGE = 1920                                # kSumRows of csrc/kmeans.hip: member rows per LDS stage of the sum kernel
STAGE_SIZES = [1919, 1920, 1921, STAGE + 1, STAGE + 3, STAGE + 4, STAGE + 16, STAGE + 17, 3839, 3840, 3841,
               2 * STAGE + 5, 5 * STAGE, 5 * STAGE + 1919]


def same_bits(a, b):
    """float32 arrays equal bit for bit (tells -0.0 from +0.0 and one NaN from another, which == does not)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def split(data):
    return np.ascontiguousarray(data[:, :3]), np.ascontiguousarray(data[:, 3:])


def blobs(n, seed):
    """the mixture of tests/test_kmeans_gpu.py::test_kmeans_large_vs_oracle: 12 centres, wide in xyz, narrow in colour"""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(12, 6)) * np.array([5, 5, 5, 1, 1, 1])
    return (centres[rng.integers(0, 12, size=n)] + rng.normal(size=(n, 6)) * np.array([0.8, 0.8, 0.8, 0.3, 0.3, 0.3])).astype(np.float32)


def sized_scene(sizes, seed):
    """Clusters of exactly the given member counts.  Cluster c sits at x = 1000 c; its other five coordinates are drawn with
    magnitudes 10^U(-3, 3) on both signs, so that a float32 running sum depends on the order of its terms.  A row drawn
    farther than 499 from the x axis is scaled back onto that radius: member counts can only be exact if no row ever changes
    cluster, and with x 1000 apart that needs |row - own centroid|^2 < 1000^2 for every centroid in the hull of its
    cluster, i.e. all rows within a tube of diameter < 1000.  So the magnitudes within a cluster span 1e-3 to about 5e2,
    not 1e3 (the test asserts the membership itself).  The rows of a cluster are scattered through the index space by a
    seeded permutation.  Returns (data (n, 6) float32, members: list of ascending row-index arrays, init: one member of
    every cluster)."""
    rng = np.random.default_rng(seed)
    n, k = int(sum(sizes)), len(sizes)
    perm = rng.permutation(n)
    data = np.empty((n, 6), np.float32)
    members, init, pos = [], np.empty(k, np.int64), 0
    for c, m in enumerate(sizes):
        rows = np.sort(perm[pos:pos + m])
        pos += m
        y = 10.0 ** rng.uniform(-3.0, 3.0, size=(m, 5)) * rng.choice([-1.0, 1.0], size=(m, 5))
        norm = np.sqrt((y * y).sum(axis=1, keepdims=True))
        y = y * np.minimum(1.0, 499.0 / norm)
        data[rows, 0] = 1000.0 * c
        data[rows, 1:] = y
        members.append(rows)
        init[c] = rows[rng.integers(m)]
    return data, members, init


def order_sensitive(data, members):
    """Section-1 condition: for every cluster of at least 16 members the float32 sum in index order differs, in at least
    one column, from the sum in reverse index order AND from the float64 sum rounded to float32.  Returns the list of
    clusters that miss it (empty = the condition holds)."""
    bad = []
    for c, rows in enumerate(members):
        if len(rows) < 16:
            continue
        fwd = np.add.reduce(data[rows], axis=0, dtype=np.float32)
        rev = np.add.reduce(data[rows[::-1]], axis=0, dtype=np.float32)
        f64 = np.add.reduce(data[rows].astype(np.float64), axis=0).astype(np.float32)
        if same_bits(fwd, rev) or same_bits(fwd, f64):
            bad.append(c)
    return bad


# ---- section 4: rows on the diagonal against coordinate permutations of one centroid ----------------------------------------
DIAG_ROWS = 20_000
DIAG_A = np.array([0.0015837, 0.0116954, 0.2458701, 6.763615, 29.543817, 195.55253], np.float32)
DIAG_PERMS = ([0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0], [1, 0, 3, 2, 5, 4], [4, 5, 0, 1, 2, 3])   # a, reversed, swapped, rotated by 2


def diagonal_scene(seed=0):
    """20 000 rows (t,)*6, t float32 uniform in +-50, then the four centroid rows: a and three coordinate permutations of it.
    In exact arithmetic every diagonal row is equally far from all four; in float64 the association of the six squares
    decides.  Returns (data (20 004, 6) float32, init = the last four row indices)."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-50.0, 50.0, size=DIAG_ROWS).astype(np.float32)
    cent = np.stack([DIAG_A[p] for p in DIAG_PERMS])
    data = np.concatenate((np.repeat(t[:, None], 6, axis=1), cent)).astype(np.float32)
    return data, np.arange(DIAG_ROWS, DIAG_ROWS + 4)


def _squares(data32, cent32):
    d = data32.astype(np.float64)[:, None, :] - cent32.astype(np.float64)[None, :, :]
    return d, d * d


def labels_pairwise(data32, cent32):
    _, q = _squares(data32, cent32)
    return np.argmin(((q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])) + (q[..., 4] + q[..., 5]), axis=1)


def labels_reversed(data32, cent32):
    _, q = _squares(data32, cent32)
    return np.argmin(((((q[..., 5] + q[..., 4]) + q[..., 3]) + q[..., 2]) + q[..., 1]) + q[..., 0], axis=1)


def labels_float32(data32, cent32):
    d = data32[:, None, :] - cent32[None, :, :]
    q = d * d
    return np.argmin(((((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]) + q[..., 4]) + q[..., 5], axis=1)


def labels_fma_tail(data32, cent32):
    """the prescribed association, but with the last term folded in as fma(d5, d5, s): one rounding of the exact s + d5^2
    (exact rational arithmetic; Fraction -> float rounds to nearest even)"""
    d, q = _squares(data32, cent32)
    s = (((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]) + q[..., 4]
    out = np.empty(s.shape, np.float64)
    for idx in np.ndindex(*s.shape):
        d5 = Fraction(float(d[idx + (5,)]))
        out[idx] = float(Fraction(float(s[idx])) + d5 * d5)
    return np.argmin(out, axis=1)


# ---- section 3: empty clusters at index 0, at k - 1 and in a run of three -----------------------------------------------------
FAR = np.array([1e4, 1e4, 1e4, 8.0, 8.0, 8.0], np.float32)     # small integers: the float32 mean of any number of copies is exact


def empty_scene(where, seed=11):
    """Blob rows near the origin with a few rows overwritten far away, k = 7.  Returns (data, init, empty cluster indices).

    "last", "run": copies of one far row.  The first copy in `init` takes them all under the first-minimum rule and its mean is
    the row itself, so the later copies (index k - 1; indices 3, 4, 5) never win a row in any pass.

    "first": index 0 cannot be empty in the first pass - its own init row is at distance 0 and index 0 wins every tie - so it
    is emptied from the second pass on.  On a far line parallel to x: A (x = 0, centroid 0), B (3, centroid 1), E (-200,
    centroid 2), D (-99) and nine rows F around -120.  Pass 1: D goes to A (99 < 101), the F go to E; centroid 0 moves to
    -49.5, centroid 2 to -128.  From pass 2 on A belongs to B (3 < 49.5) and D to centroid 2 (29 < 49.5): cluster 0 is empty,
    offsets[0] == offsets[1] == 0, and keeps the centroid of pass 1."""
    data = blobs(20_003, seed)
    rng = np.random.default_rng(seed + 1)
    spots = rng.choice(len(data), 16, replace=False)            # scattered row indices to overwrite
    blob_rows = [int(v) for v in np.setdiff1d(np.arange(len(data)), spots)[[5, 700, 4242, 9001, 15_000]]]
    if where == "first":
        xs = [0.0, 3.0, -200.0, -99.0] + [-120.0 + 0.25 * (j - 4) for j in range(9)]
        for r, x in zip(spots, xs):
            data[r] = [x, 1e4, 1e4, 0.0, 0.0, 0.0]
        return data, np.array([spots[0], spots[1], spots[2]] + blob_rows[:4], np.int64), [0]
    if where == "last":
        data[spots[:2]] = FAR
        return data, np.array(blob_rows + [spots[0], spots[1]], np.int64), [6]
    assert where == "run"
    data[spots[:4]] = FAR
    return data, np.array(blob_rows[:2] + [int(v) for v in spots[:4]] + blob_rows[2:3], np.int64), [3, 4, 5]


# ---- section 6: the sign of a zero mean ----------------------------------------------------------------------------------------
def zero_sign_scene(seed=3):
    """Four clusters 100 apart in x, f_dc_1 (column 4) chosen per cluster: cluster 0 (1921 members, more than one stage of
    the sum kernel) has -0.0 in every member; cluster 1 (40 members) mixes +0.0 and -0.0 and its first member in index order
    has -0.0; cluster 2 is one row with -0.0; cluster 3 (300 members) is ordinary.  Returns (data, init, members)."""
    rng = np.random.default_rng(seed)
    sizes = [1921, 40, 1, 300]
    n = sum(sizes)
    perm = rng.permutation(n)
    data = np.empty((n, 6), np.float32)
    members, init, pos = [], [], 0
    for c, m in enumerate(sizes):
        rows = np.sort(perm[pos:pos + m])
        pos += m
        data[rows] = rng.normal(size=(m, 6))
        data[rows, 0] += 100.0 * c
        if c == 0 or c == 2:
            data[rows, 4] = -0.0
        elif c == 1:
            data[rows, 4] = np.where(np.arange(m) % 3 == 0, -0.0, 0.0)        # the first member: -0.0
        members.append(rows)
        init.append(int(rows[m // 2]))
    return data, np.array(init, np.int64), members
