"""GPU: gsx_knn, gsx_normals and the front of gsx_region_growing (csrc/normals.hip) on the constructed scenes of
tests/nn_cases.py - the places where the kernels' control flow changes, which random clouds rarely or never reach: both
caps of the grid sizing, a query on a cell face (first inscribed radius below zero), a ring that doubles, a bounding
box taken from a sample that never saw some rows, the radix select deciding among equal non-zero distances by the index
digits and ending early on a shell taken whole, n below one workgroup's four queries, k = n, exactly zero off-diagonals
and rank-1 input in the Jacobi solver, moments far from the origin.  test_nn_grid.py (CPU) proves through the grid hook
that every scene reaches its edge.

Every scene runs with the grid and again with option nn_brute.  Lists: equal to the model's, no tolerance.  Neighbour
sets of gsx_normals: centroid and covariance (gsx_debug_normals_moments) against the model's under the bounds derived in
test_region_growing_gpu.py, |centroid difference| <= 4 k u S and |covariance difference| <= 8 k u k R2.  Normals and
residuals where the eigen-gap defines them: 1e-9 rad, 1e-9 relative, as there.  Grid against brute force: the same lists
bit for bit, normals within 1e-9 rad and residuals within 1e-9 of the scene's scale where the gap exceeds 1e-3.

The translated scene "offset-far" is held to the model of the scene at the origin: the translation is exact in float32,
so lists, covariance, normals and residuals are those of the untranslated scene, while the model evaluated at the far
coordinates rounds its own centroid at 32 768 (its residuals lie up to 3.0e-7 of themselves from the GPU's, measured,
where the model at the origin lies 6.5e-11 away).  The kernels subtract the query before they add anything up, so
they give both scenes the same normals, residuals and covariances to the last bit, which is asserted.

Measured (MI355X), worst over all scenes, grid and brute force: angle to the model 1.8e-14 rad (sampling-4096), relative
residual error 6.5e-11 (offset), centroid 0.10 of its bound (7 points, k = 3, duplicated rows), covariance 0.028 of its
bound (faces, k = 3); grid against brute force 7.7e-14 rad and 2.1e-14 of the scale (both sparse_core);
collinear: |dot(normal, direction)| 2.0e-16, residual 4.7e-18 of the scale.  Lists, regions and the axis planes: exact."""
import math

import numpy as np
import pytest

import nn_cases as cases
import region_growing_model as model
from region_growing_checks import U, angles, check_against_model, check_lists, moments_against_model

pytestmark = pytest.mark.gpu

SCENES = cases.scenes()
_RESULTS = {}
_BROKEN = []


def gpu(ctx, name, brute=False):
    """every call the scene asks for, made once per (scene, search) and shared by the tests that look at it from different sides
    (so a scene's cost is paid by whichever of them runs first): {("knn", k): lists, ("normals", k): (normals, residuals,
    centroids, covariances)}.  Once a call has raised, no test of this module goes to the GPU again: they fail at once."""
    if _BROKEN:
        pytest.fail(f"an earlier GPU call of this module failed ({_BROKEN[0]}): nothing more is started")
    if (name, brute) not in _RESULTS:
        sc = SCENES[name]
        out = {}
        try:
            ctx.set_option("nn_brute", int(brute))
            for k in sc.k_knn:
                out["knn", k] = ctx.knn(sc.pts, k)
            for k in sc.k_normals:
                out["normals", k] = ctx.normals(sc.pts, k) + ctx.debug_normals_moments(sc.pts, k)
            ctx.set_option("nn_brute", 0)
        except BaseException as e:
            _BROKEN.append(f"{name}, {'brute force' if brute else 'grid'}: {type(e).__name__}: {e}")
            raise
        _RESULTS[name, brute] = out
    return _RESULTS[name, brute]


def rows(sc):
    return np.arange(len(sc.pts)) if sc.queries is None else sc.queries


@pytest.mark.parametrize("name", cases.NAMES)
def test_lists_and_neighbour_sets(ctx, name):
    sc = SCENES[name]
    q = rows(sc)
    m_nbr, _ = cases.model_lists(name)
    # the far scene's model adds up the scene at the origin: the same lists, the same covariance, the centroid moved in fp64
    far = name == "offset-far"
    for brute in (False, True):
        what = f"{name}, {'brute force' if brute else 'grid'}"
        got = gpu(ctx, name, brute)
        for k in sc.k_knn:
            assert np.array_equal(got["knn", k][q], m_nbr[:, :k]), (what, k)
            if not brute and name != "identical":                    # there k copies with lower indices precede the point itself
                check_lists(sc.pts, got["knn", k])
        for k in sc.k_normals:
            nrm, res, cen, cov = got["normals", k]
            assert np.isfinite(nrm).all() and np.isfinite(res).all() and (res >= 0).all(), (what, k)
            assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-12), (what, k)
            moments_against_model(cen, cov, sc.pts, k, m_nbr[:, :k], sc.queries, f"{what}, k = {k}",
                                  model_pts=SCENES["offset-origin"].pts if far else None, shift=cases.OFFSET if far else 0.0)
    grid, brute = gpu(ctx, name, False), gpu(ctx, name, True)
    scale = float(np.abs(sc.pts).max())
    for k in sc.k_knn:
        assert np.array_equal(grid["knn", k], brute["knn", k]), (name, k)      # every row, bit for bit
    for k in sc.k_normals:
        (nrm, res, _, _), (b_nrm, b_res, _, _) = grid["normals", k], brute["normals", k]
        _, _, _, gap = model.normals_from_neighbours(sc.pts, m_nbr[:, :k], sc.queries)
        ok = gap > 1e-3
        if ok.any():
            ang = angles(nrm[q], b_nrm[q], sign_free=res[q] < 1e-12 * scale)[ok].max()
            dres = np.abs(res - b_res)[q][ok].max()
            print(f"{name}, k = {k}: grid vs brute force over {ok.sum()} points: max angle {ang:.3e} rad, max residual difference "
                  f"{dres / scale if scale else 0:.3e} of the scale")
            assert ang <= 1e-9 and dres <= 1e-9 * scale, (name, k)


def test_offset_results_do_not_depend_on_the_translation(ctx):
    for brute in (False, True):
        near, far = gpu(ctx, "offset-origin", brute), gpu(ctx, "offset-far", brute)
        for k in SCENES["offset-far"].k_knn:
            assert np.array_equal(near["knn", k], far["knn", k])
        # moments shifted by the query: every difference p_j - p_i is the same number in both scenes, added up in the same order
        (nrm, res, cen, cov), (f_nrm, f_res, f_cen, f_cov) = near["normals", 50], far["normals", 50]
        assert np.array_equal(nrm, f_nrm) and np.array_equal(res, f_res) and np.array_equal(cov, f_cov)


DEFINED = [n for n in cases.NAMES if SCENES[n].normals_defined] + ["sparse_core"]


@pytest.mark.parametrize("name", DEFINED)
def test_normals_and_residuals(ctx, name):
    sc = SCENES[name]
    m_nbr, _ = cases.model_lists(name)
    q = sc.queries
    if name == "sparse_core":                                        # the isolated points' 64 nearest span both patches
        q = cases.sparse_core()[1]
        m_nbr = m_nbr[q]
    # the translated scene against the model of the scene at the origin (module docstring): the same lists, the same answer
    pts = SCENES["offset-origin"].pts if name == "offset-far" else sc.pts
    for brute in (False, True):
        for k in sc.k_normals:
            nrm, res, _, _ = gpu(ctx, name, brute)["normals", k]
            check_against_model(pts, k, nrm, res, q, f"{name}, {'brute force' if brute else 'grid'}, k = {k}", nbr=m_nbr[:, :k])


@pytest.mark.parametrize("name", ["bowl", "dome"])
def test_flip_rule_decides_the_sign(ctx, name):
    sc = SCENES[name]
    nbr = cases.model_lists(name)[0][:, :30]
    m_nrm, _, _, _ = model.normals_from_neighbours(sc.pts, nbr)
    P = sc.pts.astype(np.float64)
    v = P - P[nbr].mean(axis=1)
    for brute in (False, True):
        nrm, _, _, _ = gpu(ctx, name, brute)["normals", 30]
        assert (np.einsum("ij,ij->i", nrm, m_nrm) > 0).all()
        assert (np.einsum("ij,ij->i", nrm, v) <= 0).all()


@pytest.mark.parametrize("axis", range(3))
def test_axis_planes_are_exact(ctx, axis):
    """the off-diagonals that touch the constant axis are exactly zero, no rotation mixes its column, its diagonal entry 0
    is the smallest: the normal is that axis to the last bit and the residual is 0"""
    name = f"axis_plane-{'xyz'[axis]}"
    for brute in (False, True):
        nrm, res, _, cov = gpu(ctx, name, brute)["normals", 30]
        assert (cov[:, axis, :] == 0).all() and (cov[:, :, axis] == 0).all()
        assert (np.abs(nrm[:, axis]) == 1.0).all()
        assert (np.delete(nrm, axis, axis=1) == 0.0).all()
        assert (res == 0.0).all()


def test_collinear_and_identical(ctx):
    sc = SCENES["collinear"]
    scale = float(np.abs(sc.pts).max())
    d = cases.COLLINEAR_DIR / np.linalg.norm(cases.COLLINEAR_DIR)
    for brute in (False, True):
        nrm, res, _, _ = gpu(ctx, "collinear", brute)["normals", 10]
        assert np.isfinite(nrm).all() and np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-12)
        print(f"collinear: max |dot(normal, direction)| {np.abs(nrm @ d).max():.3e}, max residual {res.max() / scale:.3e} of the scale")
        assert np.abs(nrm @ d).max() <= 1e-9 and res.max() <= 1e-9 * scale
        for k in SCENES["identical"].k_normals:
            nrm, res, cen, cov = gpu(ctx, "identical", brute)["normals", k]
            assert np.isfinite(nrm).all() and np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-12)
            assert (res == 0.0).all() and (cov == 0.0).all() and (cen == SCENES["identical"].pts[0].astype(np.float64)).all()
        for k in SCENES["identical"].k_knn:                          # equal keys: the k lowest indices, in order, for every query
            assert (gpu(ctx, "identical", brute)["knn", k] == np.arange(k)).all()


@pytest.mark.parametrize("name", [n for n in cases.NAMES if n.startswith("small-normals") and SCENES[n].k_normals[0] == len(SCENES[n].pts)])
def test_small_k_equals_n_every_query_has_the_same_set(ctx, name):
    sc = SCENES[name]
    n, k = len(sc.pts), sc.k_normals[0]
    P = sc.pts.astype(np.float64)
    mean = np.array([math.fsum(P[:, a]) / n for a in range(3)])
    S = float(np.abs(sc.pts).max())
    for brute in (False, True):
        _, _, cen, _ = gpu(ctx, name, brute)["normals", k]
        assert np.abs(cen - mean).max() <= 4 * k * U * S


CHAINS = [("small-normals-3-3-uniform", 3, 2), ("small-normals-3-3-dup", 3, 2), ("faces-x", 5, 4), ("faces-y", 5, 4), ("faces-z", 5, 4),
          ("lattice", 20, 7), ("lattice", 7, 5)]


@pytest.mark.parametrize("name,kn,k", CHAINS)
def test_chain(ctx, name, kn, k):
    """gsx_region_growing is gsx_normals, gsx_knn and the host growth: the labels are the model's growth from the GPU's own
    normals, residuals and lists, exactly"""
    pts = SCENES[name].pts
    assert not _BROKEN, _BROKEN
    nrm, res = ctx.normals(pts, kn)
    nbr = ctx.knn(pts, k)
    assert np.array_equal(nbr, model.knn(pts, k)[0])
    labels, nrm2, res2, nreg = ctx.region_growing(pts, k_normals=kn, k=k, residual_threshold=0.1, angle_threshold=0.05)
    assert np.array_equal(nrm2, nrm) and np.array_equal(res2, res)
    want, wreg = model.grow(nrm, res, nbr, 0.1, 0.05)
    assert nreg == wreg and np.array_equal(labels, want)
