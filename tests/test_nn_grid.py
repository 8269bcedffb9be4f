"""CPU: the search grid of gsx_normals / gsx_knn (csrc/normals.hip: sizing rule with its two caps, robust bounding box,
counting sort) through the context-free hook gsx_debug_nn_grid, on the constructed scenes of tests/nn_cases.py.

Three things are pinned here so that test_nn_edges_gpu.py means what it says: the invariants the kernels rely on (the
cells tile the box, the sorted order is the kernels' own cell expression, index order inside a cell); that every scene
reaches the edge it was built for (a change of the sizing rule that makes one miss fails here, not silently there); and
that the scenes discriminate - the model with the tie rule reversed, or the covariance without the shift by the query,
gives another answer than the real one by more than the GPU test's bound."""
import numpy as np
import pytest

import nn_cases as cases
import region_growing_model as model
from conftest import load_pkg
from region_growing_checks import U

MAX_DIM = 1024                                                       # kNnMaxDim
SCENES = cases.scenes()


def grid(pts, k, brute=False):
    return load_pkg().debug_nn_grid(pts, k, brute)


def box(pts):
    """the rule's bounding box, restated: exact below 4097 rows, else the 0.5 % .. 99.5 % range of min(n, 65536) rows taken
    n // m apart"""
    P = pts.astype(np.float64)
    n = len(P)
    if n <= 4096:
        return P.min(axis=0), P.max(axis=0)
    m = min(n, 65536)
    sm = np.sort(P[np.arange(m) * (n // m)], axis=0)
    cut = m // 200
    return sm[cut], sm[m - 1 - cut]


def initial_edge(pts, k):
    """(extent, edge before the caps, cells per axis at that edge)"""
    lo, hi = box(pts)
    ext = hi - lo
    live = ext > 0
    cells = max(1.0, len(pts) / max(2.0, k / 113.0))
    h0 = float(np.prod(ext[live]) / cells) ** (1.0 / live.sum())
    return ext, h0, np.floor(ext / h0) + 1


def growths(h, h0):
    """how often the edge grew by 1.26; asserts that h is h0 times a whole power of it"""
    j = np.log(h / h0) / np.log(1.26)
    assert abs(j - round(j)) < 1e-9, (h, h0)
    return int(round(j))


def ks_of(sc):
    return sorted(set(sc.k_normals + sc.k_knn))


@pytest.mark.parametrize("name", cases.NAMES)
def test_grid_invariants(name):
    sc = SCENES[name]
    P = sc.pts.astype(np.float64)
    n = len(P)
    lo, hi = box(sc.pts)
    for k in ks_of(sc):
        o, h, dims, start, order = grid(sc.pts, k)
        assert np.array_equal(o, lo), (name, k)
        assert (dims >= 1).all() and (dims <= MAX_DIM).all() and int(np.prod(dims.astype(np.int64))) <= 4 * n + 64, (name, k, dims)
        assert h > 0 and np.isfinite(h)
        if n <= 4096:                                                # the box is the exact one: the cells tile it
            assert ((dims - 1) * h <= hi - lo).all() and (hi - lo < dims * h).all(), (name, k, dims, h)
        assert start[0] == 0 and start[-1] == n and (np.diff(start.astype(np.int64)) >= 0).all()
        assert np.array_equal(np.sort(order), np.arange(n))
        # the kernels' own expression puts every point into the cell the counting sort put it in
        c = np.clip(np.floor((P - o) * (1.0 / h)), 0, dims - 1).astype(np.int64)
        cell = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
        at = np.searchsorted(start, np.arange(n), side="right") - 1  # cell of every sorted position
        assert np.array_equal(cell[order], at), (name, k)
        same = at[1:] == at[:-1]
        assert (np.diff(order)[same] > 0).all(), (name, k)           # index order inside a cell
    o, h, dims, start, order = grid(sc.pts, ks_of(sc)[0], brute=True)
    assert dims.tolist() == [1, 1, 1] and start.tolist() == [0, n] and np.array_equal(order, np.arange(n))


def test_hook_errors():
    g = load_pkg()
    lib = g.lib()
    pts = np.zeros((8, 3), np.float32)
    o, h, d = np.empty(3), np.empty(1), np.empty(3, np.int32)
    ok = (8, pts.ctypes.data, 3, 0, o.ctypes.data, h.ctypes.data, d.ctypes.data, None, None)
    assert lib.gsx_debug_nn_grid(*ok) == 0
    for i in (1, 4, 5, 6):
        assert lib.gsx_debug_nn_grid(*ok[:i], None, *ok[i + 1:]) == g._lib.GSX_E_INVALID
    assert lib.gsx_debug_nn_grid(0, *ok[1:]) == g._lib.GSX_E_INVALID
    assert lib.gsx_debug_nn_grid(*ok[:2], 0, *ok[3:]) == g._lib.GSX_E_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        pts[5, 2] = bad
        with pytest.raises(ValueError, match="finite"):
            grid(pts, 3)


# ---- every scene reaches its edge ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["line-x", "line-y", "line-z"])
def test_line_hits_the_axis_cap(name):
    sc, a = SCENES[name], cases.axis_of(name)
    for k in ks_of(sc):                                              # every k the GPU tests run the scene with
        ext, h0, g0 = initial_edge(sc.pts, k)
        assert (np.delete(ext, a) == 0).all() and g0[a] > MAX_DIM         # one live axis, more cells than the cap allows
        o, h, dims, _, _ = grid(sc.pts, k)
        assert np.delete(dims, a).tolist() == [1, 1] and MAX_DIM / 1.26 < dims[a] <= MAX_DIM
        assert growths(h, h0) >= 1
        print(f"{name}, k = {k}: {dims.tolist()} after {growths(h, h0)} growths of the edge")


@pytest.mark.parametrize("name", ["needle-x", "needle-y", "needle-z"])
def test_needle_hits_the_axis_cap_with_three_live_axes(name):
    sc, a = SCENES[name], cases.axis_of(name)
    for k in ks_of(sc):                                              # every k the GPU tests run the scene with
        ext, h0, g0 = initial_edge(sc.pts, k)
        assert (ext > 0).all() and g0[a] > MAX_DIM and np.prod(np.minimum(g0, MAX_DIM)) <= 4 * len(sc.pts) + 64   # the axis cap alone
        o, h, dims, _, _ = grid(sc.pts, k)
        assert MAX_DIM / 1.26 < dims[a] <= MAX_DIM and growths(h, h0) >= 1
        print(f"{name}, k = {k}: {dims.tolist()} after {growths(h, h0)} growths of the edge")


@pytest.mark.parametrize("name", ["slab-x", "slab-y", "slab-z"])
def test_slab_hits_the_total_cap(name):
    sc = SCENES[name]
    n = len(sc.pts)
    for k in ks_of(sc):                                              # every k the GPU tests run the scene with
        ext, h0, g0 = initial_edge(sc.pts, k)
        assert (ext > 0).all() and (g0 <= MAX_DIM).all() and np.prod(g0) > 4 * n + 64      # the total cap alone
        o, h, dims, _, _ = grid(sc.pts, k)
        total = int(np.prod(dims.astype(np.int64)))
        assert (4 * n + 64) / 1.26 ** 2 < total <= 4 * n + 64 and growths(h, h0) >= 1   # two axes shrink by 1.26 per growth
        print(f"{name}, k = {k}: {dims.tolist()} after {growths(h, h0)} growths of the edge, {int(np.prod(g0))} cells at the first edge")


@pytest.mark.parametrize("name", ["faces-x", "faces-y", "faces-z"])
def test_faces_queries_lie_on_cell_faces(name):
    sc, a = SCENES[name], cases.axis_of(name)
    want = [1, 1, 1]
    want[a] = 514
    for k in ks_of(sc):
        o, h, dims, _, _ = grid(sc.pts, k)
        assert h == 1.0 and dims.tolist() == want and (o == 0).all()
    x = sc.pts[:, a].astype(np.float64)
    on_face = (x == np.floor(x)) & (x > 0)                            # (x - o) / h is a whole number: the lower face of its cell
    assert on_face.sum() == 513
    # the first inscribed radius of such a query is its distance to that face less the margin, 0 - 1e-5 h < 0: no count, widen
    assert ((x[on_face] - (o[a] + np.floor(x[on_face]) * h)) - 1e-5 * h < 0).all()
    assert cases.tie_share(name, 2) > 0.99 and cases.tie_share(name, 4) > 0.99     # +-0.5 and +-1: the index decides


def test_lattice_ties():
    """measured: 0.93, 0.42, 0.995, 1.0"""
    for k, least in ((5, 0.9), (7, 0.4), (20, 0.9), (64, 0.9)):
        share = cases.tie_share("lattice", k)
        print(f"lattice: k = {k}: the k-th and the next neighbour tie for {share:.3f} of the queries")
        assert share >= least
    # k = 7 is one point and its shell of 6, whole: the select ends at need == before + inside
    _, d2 = cases.model_lists("lattice")
    whole = (d2[:, 6] == 1.0) & (d2[:, 7] > 1.0) & (d2[:, 1] == 1.0)
    assert whole.mean() > 0.5


def test_small_sizes():
    nk = cases.SMALL_NORMALS + cases.SMALL_KNN
    assert any(n < 4 for n, k in nk) and any(n % 4 for n, k in nk) and any(k == n > 64 for n, k in nk) and (64, 64) in cases.SMALL_KNN
    for name, sc in SCENES.items():
        if name.startswith("small") and name.endswith("dup"):
            n = len(sc.pts)
            assert len(np.unique(sc.pts, axis=0)) <= n - n // 2


def test_sampling_switch():
    (s96, rows), (s97, _) = cases.sampling(4096), cases.sampling(4097)
    assert np.array_equal(s96.pts, s97.pts[:4096]) and (np.abs(s97.pts[rows]) > 390).all() and len(rows) == 30
    o96, h96, d96, _, _ = grid(s96.pts, 10)
    o97, h97, d97, start, _ = grid(s97.pts, 10)
    assert (o96 < -390).all() and (o96 + d96 * h96 > 390).all()      # exact box: the outliers stretch it
    assert (o97 > -1).all() and (o97 + d97 * h97 < 1.5).all()        # sampled box: the outliers are cut off and clamped
    assert h96 > 100 * h97


def test_sampling_leaves_rows_unseen():
    sc, last = cases.sampling(65537)
    o, h, dims, _, _ = grid(sc.pts, 10)
    assert last.tolist() == [65536] and last[0] in sc.queries and (np.abs(sc.pts[-1]) == cases.OUTLIER).all()
    assert (o > -1).all() and (o + dims * h < 1.5).all()
    without = sc.pts.copy()
    without[-1] = without[0]
    assert np.array_equal(grid(without, 10)[0], o) and grid(without, 10)[1] == h      # the sample never saw the last row
    sc, last = cases.sampling(131073)
    o, h, dims, _, _ = grid(sc.pts, 10)
    assert last[0] == 131072 and last[0] in sc.queries
    assert (o >= -0.01).all() and (o + dims * h < 0.011).all()       # the box of the even rows
    inside = ((sc.pts >= o) & (sc.pts < o + dims * h)).all(axis=1)
    assert not inside[1::2].mean() > 1e-4 and (~inside).mean() > 0.49   # the odd rows are clamped into border cells
    assert (sc.queries % 2 == 0).sum() >= 300 and (sc.queries % 2 == 1).sum() >= 299


def ring_walk(P, cell, i, o, h, dims, k):
    """the ring rule of nn_threshold for query i, restated: [(r, points counted, doubled)] of every step that widened the cube;
    cell: the clamped cell of every point"""
    q, c = P[i], cell[i]
    steps, r = [], 0
    while True:
        lo, hi = np.maximum(c - r, 0), np.minimum(c + r, dims - 1)
        R = np.inf
        for a in range(3):
            if lo[a] > 0:
                R = min(R, q[a] - (o[a] + lo[a] * h))
            if hi[a] < dims[a] - 1:
                R = min(R, (o[a] + (hi[a] + 1) * h) - q[a])
        if R == np.inf:                                              # the cube is the whole grid
            return steps
        R -= 1e-5 * h
        cnt = 0
        if R > 0.0:
            d = P[((cell >= lo) & (cell <= hi)).all(axis=1)] - q
            cnt = int(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= R * R).sum())
            if cnt >= k:
                return steps
        doubled = cnt < k // 8
        steps.append((r, cnt, doubled))
        r = 2 * r + 1 if doubled else r + 1


def test_sparse_core_rings_double():
    sc, blobs = cases.sparse_core()
    core = np.setdiff1d(np.arange(len(sc.pts)), blobs)
    assert len(blobs) == 4800 and len(core) == 24
    k = 64
    o, h, dims, _, _ = grid(sc.pts, k)
    P = sc.pts.astype(np.float64)
    cell = np.clip(np.floor((P - o) * (1.0 / h)), 0, dims - 1).astype(np.int64)
    fewest = 99
    for i in core:
        steps = ring_walk(P, cell, i, o, h, dims, k)
        real = [r for r, cnt, doubled in steps if doubled and r >= 1]  # at r = 0 doubling and widening by one are the same step
        fewest = min(fewest, len(real))
        assert len(real) >= 2, (i, steps)
    print(f"sparse_core: grid {dims.tolist()}, h {h:.4f}: every isolated query doubles its ring at least {fewest} times at r >= 1")
    # and a patch point does not: its own cell and the next ring hold its k neighbours
    for i in blobs[::400]:
        assert not any(doubled and r >= 1 for r, cnt, doubled in ring_walk(P, cell, i, o, h, dims, k)), i


def test_axis_planes_collinear_identical():
    for a in range(3):
        sc = SCENES[f"axis_plane-{'xyz'[a]}"]
        assert len(np.unique(sc.pts[:, a])) == 1 and sc.pts[0, a] != 0
        assert grid(sc.pts, 30)[2][a] == 1 and (np.delete(grid(sc.pts, 30)[2], a) > 1).all()
    sc = SCENES["collinear"]
    P = sc.pts.astype(np.float64)
    t = P[:, 0] / cases.COLLINEAR_DIR[0]
    assert len(np.unique(t)) == 500 and np.array_equal(t, np.round(t)) and np.array_equal(P, t[:, None] * cases.COLLINEAR_DIR)
    sc = SCENES["identical"]
    assert len(sc.pts) == 300 and len(np.unique(sc.pts, axis=0)) == 1


@pytest.mark.parametrize("name", ["bowl", "dome"])
def test_bowl_and_dome_have_a_decided_flip(name):
    sc = SCENES[name]
    nbr, _ = cases.model_lists(name)
    nbr = nbr[:, :30]
    _, _, dot, gap = model.normals_from_neighbours(sc.pts, nbr)
    P = sc.pts.astype(np.float64)
    vnorm = np.linalg.norm(P - P[nbr].mean(axis=1), axis=1)
    assert (gap > 1e-3).all() and (np.abs(dot) >= 1e-12 * vnorm).all()


# ---- the scenes discriminate -------------------------------------------------------------------------------------------------------
def knn_higher_index_first(pts, k):
    """the model with the tie rule reversed: the same model on the rows in reverse order"""
    n = len(pts)
    nbr, _ = model.knn(pts[::-1], k)
    return (n - 1 - nbr)[::-1]


@pytest.mark.parametrize("name,k", [("lattice", 5), ("lattice", 20), ("lattice", 64), ("faces-x", 2), ("faces-x", 4)])
def test_reversed_tie_rule_gives_other_lists(name, k):
    sc = SCENES[name]
    real = cases.model_lists(name)[0][:, :k]
    other = knn_higher_index_first(sc.pts, k)
    differ = (real != other).any(axis=1).mean()
    sets_differ = (np.sort(real, axis=1) != np.sort(other, axis=1)).any(axis=1).mean()
    print(f"{name}, k = {k}: reversed tie rule changes {differ:.3f} of the lists, {sets_differ:.3f} of the neighbour sets")
    assert differ > 0.5 and sets_differ > 0.5


def test_offset_scene_needs_the_shift():
    near, far = cases.offset()
    k = 50
    nbr = cases.model_lists("offset-origin")[0][:, :k]
    assert np.array_equal(nbr, cases.model_lists("offset-far")[0][:, :k])                # the translation is exact
    _, _, _, gap = model.normals_from_neighbours(near.pts, nbr)
    assert (gap > 1e-3).all()
    _, cov, r2 = model.moments(near.pts, nbr)
    N = far.pts.astype(np.float64)[nbr]
    c = N.mean(axis=1)
    unshifted = np.einsum("bki,bkj->bij", N, N) - k * c[:, :, None] * c[:, None, :]       # S2 - k m m^T at the far coordinates
    err = np.abs(unshifted - cov).max(axis=(1, 2))
    bound = 8 * k * U * k * r2                                                            # test_nn_edges_gpu.py holds the GPU to this
    print(f"offset: the unshifted covariance is off by {np.median(err / bound):.3e} bounds in the median, {(err > bound).mean():.3f} of "
          "the rows beyond it")
    assert (err > bound).mean() > 0.99
