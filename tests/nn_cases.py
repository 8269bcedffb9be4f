"""Constructed scenes that put the k-NN, normal and residual kernels (csrc/normals.hip) at the places where their control
flow changes: the two caps of the grid sizing, the sampled bounding box, the ring that widens by one or doubles, the radix
select among equal distances, the Jacobi solver on exactly zero off-diagonals.  Used by test_nn_grid.py (CPU: the grid
hook proves that every scene reaches the edge it was built for) and test_nn_edges_gpu.py.

A scene is a Scene: float32 points, the k values gsx_normals and gsx_knn are called with, the rows the model answers
(None: all) and whether the PCA normal is defined on those rows (an eigen-gap nearly everywhere).  Everything is seeded."""
import functools
from collections import namedtuple

import numpy as np

import region_growing_model as model

Scene = namedtuple("Scene", "name pts k_normals k_knn queries normals_defined")

PERMS = {"x": (0, 1, 2), "y": (2, 0, 1), "z": (1, 2, 0)}        # column a of the permuted scene = column PERMS[.][a]


def scene(name, pts, k_normals, k_knn, queries=None, normals_defined=False):
    pts = np.ascontiguousarray(pts, np.float32)
    pts.setflags(write=False)
    return Scene(name, pts, tuple(k_normals), tuple(k_knn), queries, normals_defined)


def permuted(sc, axis):
    """the scene with its x axis moved to `axis`: the per-axis code is unrolled and cells are x-fastest"""
    return scene(f"{sc.name}-{axis}", sc.pts[:, PERMS[axis]], sc.k_normals, sc.k_knn, sc.queries, sc.normals_defined)


def axis_of(name):
    """index of the axis that carries a permuted scene's x extent"""
    return "xyz".index(name.rsplit("-", 1)[1])


# ---- grid sizing ---------------------------------------------------------------------------------------------------------------
def line():
    """one-dimensional extent: the 1024-cells-per-axis cap grows the edge"""
    rng = np.random.default_rng(101)
    pts = np.zeros((5000, 3), np.float32)
    pts[:, 0] = rng.uniform(0, 100, 5000)
    return scene("line", pts, (10, 100), (10, 64))


def needle():
    """three live axes, the x cap hits"""
    rng = np.random.default_rng(102)
    return scene("needle", rng.uniform(0, 1, (5000, 3)) * [1, 1e-3, 1e-3], (10, 100), (10, 64))


def slab():
    """the total-cells cap hits"""
    rng = np.random.default_rng(103)
    return scene("slab", rng.uniform(0, 1, (5000, 3)) * [1, 1, 1e-4], (10, 100), (10, 64))


def faces():
    """h = 1 exactly: every integer-x query lies on its cell's lower face, so its first inscribed radius is negative;
    the neighbours at +-0.5 and +-1 tie pairwise at a non-zero distance"""
    rng = np.random.default_rng(104)
    x = np.concatenate((np.arange(514.0), np.arange(512.0) + 0.5))
    pts = np.zeros((1026, 3), np.float32)
    pts[:, 0] = x[rng.permutation(1026)]
    return scene("faces", pts, (3, 4, 5, 64), (2, 3, 4, 5, 64))


# ---- ties ----------------------------------------------------------------------------------------------------------------------
def lattice():
    """12^3 integer lattice, shells of 1, 6, 12, 8, 6, 24, ... points: k = 7 takes a shell whole, 5, 20, 64 cut one"""
    rng = np.random.default_rng(105)
    g = np.arange(12.0)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return scene("lattice", pts[rng.permutation(len(pts))], (5, 7, 20, 200), (5, 7, 20, 64))


SMALL_NORMALS = [(3, 3), (4, 3), (4, 4), (5, 5), (7, 3), (64, 64), (65, 64), (65, 65), (300, 300)]
SMALL_KNN = [(2, 2), (3, 2), (5, 5), (64, 64), (65, 64), (129, 63)]


def small(n, k, dup, knn):
    """fewer points than a workgroup has waves, n no multiple of 4, k = n; dup: the second half repeats rows of the first"""
    rng = np.random.default_rng(1000 * n + 2 * k + dup)
    pts = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    if dup:
        pts[n - n // 2:] = pts[rng.integers(0, n - n // 2, n // 2)]
    return scene(f"small-{'knn' if knn else 'normals'}-{n}-{k}-{'dup' if dup else 'uniform'}", pts, () if knn else (k,), (k,) if knn else ())


# ---- bounding box from a sample --------------------------------------------------------------------------------------------------
def noisy_planes(rng, n, lo, hi, noise):
    """three tilted planar patches inside [lo, hi]^3 with Gaussian noise along the normal, in random row order"""
    parts = []
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    for j, m in enumerate(np.array_split(np.arange(n), 3)):
        w = np.float64([[0.2, 0.1, 1.0], [1.0, 0.3, 0.2], [0.1, 1.0, -0.3]][j])
        w /= np.linalg.norm(w)
        u = np.cross(w, [0.0, 0.0, 1.0] if j else [1.0, 0.0, 0.0])
        u /= np.linalg.norm(u)
        v = np.cross(w, u)
        a = rng.uniform(-0.5, 0.5, (len(m), 2)) * half
        c = mid + (np.float64([[0.0, 0.0, -0.2], [0.2, 0.0, 0.1], [0.0, -0.2, 0.1]][j])) * half
        parts.append(c + a[:, :1] * u + a[:, 1:] * v + rng.normal(0, noise, (len(m), 1)) * w)
    pts = np.vstack(parts)
    assert pts.min() >= lo and pts.max() < hi
    return pts[rng.permutation(n)]


OUTLIER = 400.0


def sampling_cloud():
    """4097 rows; 30 of the first 4096 are outliers at +-400, 15 at either end of every axis (fewer than the 20 rows the
    sampled box of n = 4097 cuts off at either end)"""
    rng = np.random.default_rng(106)
    pts = noisy_planes(rng, 4097, -1.0, 1.0, 0.004)
    rows = np.sort(rng.choice(4096, 30, replace=False))
    sign = np.where((np.arange(30)[:, None] >> np.arange(3)) & 1, 1.0, -1.0)
    sign[15:] = -sign[:15]
    pts[rows] = OUTLIER * sign + rng.uniform(-1, 1, (30, 3))
    return pts, rows


def sampling(n):
    if n in (4096, 4097):
        pts, rows = sampling_cloud()
        return scene(f"sampling-{n}", pts[:n], (30,), (10, 64), normals_defined=True), rows
    rng = np.random.default_rng(n)
    if n == 65537:                                                    # m = 65536, step 1: the last row is never sampled
        pts = noisy_planes(rng, n, -1.0, 1.0, 0.004)
        pts[-1] = [OUTLIER, -OUTLIER, OUTLIER]
        special = np.array([n - 1])
    else:                                                             # step 2: the even rows are the sample
        assert n == 131073
        pts = rng.uniform(-1, 1, (n, 3))
        pts[::2] = rng.uniform(-0.01, 0.01, (len(pts[::2]), 3))
        special = np.array([n - 1])                                   # even, and past the last sampled row n - 3
    rest = np.setdiff1d(np.arange(n), special)
    q = np.sort(np.concatenate((special, rng.choice(rest[::2], 300, replace=False), rng.choice(rest[1::2], 300 - len(special), replace=False))))
    assert len(np.unique(q)) == 600
    return scene(f"sampling-{n}", pts, (30,), (10, 64), q, normals_defined=True), special


# ---- ring ------------------------------------------------------------------------------------------------------------------------
def sparse_core():
    """two dense patches in opposite corners of [0, 1]^3 and 24 isolated points around the centre - isolated from the
    patches and from each other: a jittered lattice three cells apart (the cell edge is about 0.07), without its centre and
    the two corners next to the patches, so that a sphere of four cells' radius holds at most 7 < k / 8 points.  Their ring
    counts fewer than k / 8 points at r = 0, 1 and 3 and doubles each time (test_nn_grid.py re-runs the ring rule and asserts
    it).  Returns the scene and the rows of the patches."""
    rng = np.random.default_rng(107)
    a = noisy_planes(rng, 2400, 0.0, 0.12, 0.0004)
    b = noisy_planes(rng, 2400, 0.88, 1.0, 0.0004)
    g = np.float64([-1, 0, 1])
    core = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    core = core[(np.abs(core).sum(axis=1) > 0) & (np.abs(core.sum(axis=1)) < 3)]
    assert len(core) == 24
    core = 0.5 + 0.21 * core + rng.uniform(-0.01, 0.01, (24, 3))
    pts = np.vstack((a, b, core))
    order = rng.permutation(len(pts))
    blobs = np.sort(np.flatnonzero(order < 4800))
    return scene("sparse_core", pts[order], (64,), (64,)), blobs


# ---- Jacobi ----------------------------------------------------------------------------------------------------------------------
def axis_plane(axis):
    """a plane at a non-zero constant coordinate: the off-diagonals touching that axis are exactly zero"""
    rng = np.random.default_rng(108 + axis)
    pts = rng.uniform(-1, 1, (2000, 3))
    pts[:, axis] = (0.7, -1.3, 2.1)[axis]
    return scene(f"axis_plane-{'xyz'[axis]}", pts, (30,), (10,))


COLLINEAR_DIR = np.float64([1.0, 2.0, 3.0]) / 4


def collinear():
    """500 distinct points exactly on a line in a general direction: rank-1 covariance"""
    rng = np.random.default_rng(111)
    t = rng.choice(np.arange(-1000, 1000), 500, replace=False).astype(np.float64)
    return scene("collinear", t[:, None] * COLLINEAR_DIR, (10,), (10,))


def identical():
    return scene("identical", np.tile(np.float32([1.5, -2.0, 0.25]), (300, 1)), (3, 300), (2, 64))


def bowl(sign):
    """z = +-0.8 (x^2 + y^2): the centroid of the neighbours lies on one side of every point, the flip rule decides"""
    rng = np.random.default_rng(112 if sign > 0 else 113)
    xy = rng.uniform(-1, 1, (4000, 2))
    z = sign * 0.8 * (xy * xy).sum(axis=1)
    return scene("bowl" if sign > 0 else "dome", np.column_stack((xy, z)), (30,), (10,), normals_defined=True)


OFFSET = 32768.0


def offset():
    """three noisy planes on the 2^-8 lattice inside [0, 16)^3, and the same scene moved by 32768 along every axis - exact
    in float32 (2^-8 is the spacing of float32 in [32768, 65536)).  Returns (scene at the origin, translated scene)."""
    rng = np.random.default_rng(114)
    pts = np.round(noisy_planes(rng, 3000, 0.5, 15.5, 0.03) * 256) / 256
    near = scene("offset-origin", pts, (50,), (10, 50), normals_defined=True)
    far = scene("offset-far", near.pts + np.float32(OFFSET), (50,), (10, 50), normals_defined=True)
    assert np.array_equal(far.pts.astype(np.float64) - OFFSET, near.pts.astype(np.float64))
    return near, far


# ---- the list ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scenes():
    """{name: Scene} of every scene, permutations included"""
    out = []
    for base in (line(), needle(), slab(), faces()):
        out += [permuted(base, a) for a in "xyz"]
    out.append(lattice())
    out += [small(n, k, dup, False) for n, k in SMALL_NORMALS for dup in (0, 1)]
    out += [small(n, k, dup, True) for n, k in SMALL_KNN for dup in (0, 1)]
    out += [sampling(n)[0] for n in (4096, 4097, 65537, 131073)]
    out.append(sparse_core()[0])
    out += [axis_plane(a) for a in range(3)]
    out += [collinear(), identical(), bowl(+1), bowl(-1)]
    out += list(offset())
    return {s.name: s for s in out}


NAMES = [s for s in scenes()]


@functools.lru_cache(maxsize=None)
def model_lists(name):
    """(index, d2) of the model for the scene's queries at the largest k the scene uses, plus one column where n allows: every
    smaller k is a prefix, the order (d2, index) being total.  Computed once per scene and shared; read-only."""
    sc = scenes()[name]
    k = min(max(sc.k_normals + sc.k_knn) + 1, len(sc.pts))
    nbr, d2 = model.knn(sc.pts, k, sc.queries)
    nbr.setflags(write=False)
    d2.setflags(write=False)
    return nbr, d2


def tie_share(name, k):
    """share of the queries whose k-th and (k+1)-th neighbour are equally far"""
    _, d2 = model_lists(name)
    return float((d2[:, k - 1] == d2[:, k]).mean())
