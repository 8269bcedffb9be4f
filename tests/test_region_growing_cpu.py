"""CPU: the host growth of the region-growing labeler (gsx_region_grow, csrc/region_grow.cpp) against the reference's own
regions (tests/golden/region_growing.npz, made by tools/make_golden_region_growing.py from
3D_clustering/region_growing.py), and the numpy model (tests/region_growing_model.py) against the same fixture."""
import json
import os

import numpy as np
import pytest

import region_growing_model as model
from conftest import GOLDEN, load_pkg

Z = np.load(os.path.join(GOLDEN, "region_growing.npz"))
CASES = [str(c) for c in Z["cases"]]


def case(name):
    return {k.split("/", 1)[1]: Z[k] for k in Z.files if k.startswith(name + "/")}


@pytest.fixture(scope="module")
def g():
    pkg = load_pkg()
    pkg.build()
    return pkg


def test_fixture_holds_what_the_tests_rest_on():
    assert len(CASES) >= 4
    notes = json.loads(str(Z["notes"]))
    assert notes["scenes"] == CASES
    for name in CASES:
        c = case(name)
        assert c["points"].dtype == np.float32 and c["normals"].dtype == np.float64
        assert float(c["margin"]) >= 1e-9 and float(c["low_gap"]) < 0.01
        assert 0 < float(c["tol_angle"]) < 1e-4 and 0 < float(c["tol_residual"]) < 1e-4   # a float32 effect, not a bug
        assert int(c["n_regions"]) == int(c["labels"].max()) + 1


@pytest.mark.parametrize("name", CASES)
def test_region_grow_reproduces_the_reference_regions(g, name):
    """fed with the reference's OWN normals, residuals and k-NN lists: the same sets, the same size order"""
    c = case(name)
    labels, nreg = g.region_grow(c["normals"], c["residuals"], c["knn"], float(c["residual_threshold"]), float(c["angle_threshold"]))
    assert labels.dtype == np.int32 and nreg == int(c["n_regions"])
    assert model.same_regions(c["labels"], labels)
    sizes = np.bincount(labels)
    assert (np.diff(sizes) <= 0).all()                       # largest first


@pytest.mark.parametrize("name", CASES)
def test_model_against_the_fixture(name):
    c = case(name)
    pts, kn, k = c["points"], int(c["k_normals"]), int(c["k"])
    nbr, _ = model.knn(pts, k)
    assert np.array_equal(nbr, c["knn"])
    nrm, res, _, gap = model.normals(pts, kn)
    assert (gap <= 1e-3).mean() < 0.01
    cosang = np.einsum("ij,ij->i", nrm, c["normals"])
    cosang = np.where(c["residuals"] < 1e-6, np.abs(cosang), cosang)
    ang = np.arctan2(np.linalg.norm(np.cross(nrm, c["normals"]), axis=1), cosang)
    assert ang.max() <= float(c["tol_angle"]) and np.abs(res - c["residuals"]).max() <= float(c["tol_residual"])
    labels, nreg = model.grow(nrm, res, nbr, float(c["residual_threshold"]), float(c["angle_threshold"]))
    assert nreg == int(c["n_regions"]) and model.same_regions(c["labels"], labels)


def test_region_grow_equals_the_model_on_random_input(g):
    rng = np.random.default_rng(5)
    n, k = 3000, 7
    pts = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    nbr, _ = model.knn(pts, k)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    res = rng.uniform(0, 1, n)
    want, wreg = model.grow(nrm, res, nbr, 0.5, 0.9)
    got, greg = g.region_grow(nrm, res, nbr, 0.5, 0.9)
    assert greg == wreg and np.array_equal(got, want)        # equal sizes keep creation order in both


def test_corner_cases(g):
    c = case(CASES[0])
    n = len(c["points"])
    # angle pi/2: cos = 6e-17, every neighbour is accepted; no residual bound: one region per connected component of the
    # k-NN graph - the three separated patches
    labels, nreg = g.region_grow(c["normals"], c["residuals"], c["knn"], np.inf, np.pi / 2)
    want, wreg = model.grow(c["normals"], c["residuals"], c["knn"], np.inf, np.pi / 2)
    assert nreg == wreg and np.array_equal(labels, want)
    # one region: a ring of neighbours connects everything
    ring = np.stack([(np.arange(n) + 1) % n, (np.arange(n) + 2) % n], axis=1).astype(np.int32)
    labels, nreg = g.region_grow(c["normals"], c["residuals"], ring, np.inf, np.pi / 2)
    assert nreg == 1 and (labels == 0).all()
    # angle 0: cos = 1 and |dot| > 1 never holds for unit normals that differ: every point its own region, in the order
    # of ascending residual (equal sizes keep creation order)
    nrm = np.zeros((n, 3))
    nrm[:, 2] = 1.0
    nrm[:, 0] = 1e-3 * np.arange(n)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    labels, nreg = g.region_grow(nrm, c["residuals"], c["knn"], 0.1, 0.0)
    assert nreg == n and np.array_equal(labels[np.argsort(c["residuals"], kind="stable")], np.arange(n))
    # equal residuals: the lowest index starts first
    labels, nreg = g.region_grow(nrm, np.zeros(n), c["knn"], 0.1, 0.0)
    assert nreg == n and np.array_equal(labels, np.arange(n))


def test_argument_errors(g):
    lib = g.lib()
    E = g._lib.GSX_E_INVALID
    nrm = np.zeros((4, 3))
    nrm[:, 2] = 1
    res = np.zeros(4)
    nbr = np.zeros((4, 2), np.int32)
    lab = np.zeros(4, np.int32)
    ok = (4, nrm.ctypes.data, res.ctypes.data, nbr.ctypes.data, 2, 0.1, 0.05, lab.ctypes.data, None)
    assert lib.gsx_region_grow(*ok) == 0
    for i in (1, 2, 3, 7):
        bad = list(ok)
        bad[i] = None
        assert lib.gsx_region_grow(*bad) == E
    assert lib.gsx_region_grow(0, *ok[1:]) == E
    assert lib.gsx_region_grow(*ok[:4], 0, *ok[5:]) == E
    nbr[2, 1] = 4
    with pytest.raises(ValueError, match="out of range"):
        g.region_grow(nrm, res, nbr)
    nbr[2, 1] = -1
    with pytest.raises(ValueError):
        g.region_grow(nrm, res, nbr)
    nbr[2, 1] = 0
    with pytest.raises(ValueError):
        g.region_grow(nrm, np.array([0, np.nan, 0, 0]), nbr)
    with pytest.raises(ValueError):
        g.region_grow(nrm, res[:3], nbr)
    # the context entry points refuse a NULL context like every other one
    assert lib.gsx_normals(None, 4, nrm.ctypes.data, 3, None, None) == E
    assert lib.gsx_knn(None, 4, nrm.ctypes.data, 2, None) == E
    assert lib.gsx_region_growing(None, 4, nrm.ctypes.data, 3, 2, 0.1, 0.05, lab.ctypes.data, None, None, None) == E
    assert lib.gsx_knn_device(None) is None
