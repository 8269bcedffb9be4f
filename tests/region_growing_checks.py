"""Checks of the region-growing kernels' results (csrc/normals.hip) against tests/region_growing_model.py, shared by
test_region_growing_gpu.py (whose docstring derives the bounds) and test_nn_edges_gpu.py."""
import numpy as np

import region_growing_model as model

U = 2.0 ** -53


def angles(a, b, sign_free=None):
    cosang = np.einsum("ij,ij->i", a, b)
    if sign_free is not None:
        cosang = np.where(sign_free, np.abs(cosang), cosang)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), cosang)


def check_against_model(pts, k, nrm, res, queries=None, what="", nbr=None):
    """normals / residuals of the GPU against the model on `queries` (default: all); nbr: the model's lists of these
    queries where the caller has them already.  Returns the lists."""
    q = np.arange(len(pts)) if queries is None else queries
    if nbr is None:
        nbr, _ = model.knn(pts, k, q)
    m_nrm, m_res, m_dot, gap = model.normals_from_neighbours(pts, nbr, q)
    ok = gap > 1e-3
    assert (~ok).mean() < 0.01, f"{what}: {(~ok).mean():.2%} of the points have a degenerate eigen-gap: not a scene for this test"
    P = pts.astype(np.float64)
    vnorm = np.linalg.norm(P[q] - P[nbr].mean(axis=1), axis=1)
    ang = angles(nrm[q], m_nrm, sign_free=np.abs(m_dot) < 1e-12 * vnorm)
    rel = np.abs(res[q] - m_res) / np.maximum(m_res, 1e-300)
    print(f"{what}: GPU vs model over {ok.sum()} points: max angle {ang[ok].max():.3e} rad, max relative residual error {rel[ok].max():.3e}")
    assert np.isfinite(nrm).all() and np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-12)
    assert ang[ok].max() <= 1e-9 and rel[ok].max() <= 1e-9, what
    return nbr


def moments_against_model(cen, cov, pts, k, nbr, queries=None, what="", model_pts=None, shift=0.0):
    """centroid and covariance as gsx_normals formed them for `pts` against the model's over the lists `nbr`.  model_pts,
    shift: the model adds up model_pts (pts = model_pts + shift exactly, the same lists) and its centroid is moved by
    `shift` in fp64 - the covariance of a translated scene is the covariance of the scene."""
    q = np.arange(len(pts)) if queries is None else queries
    m_cen, m_cov, r2 = model.moments(pts if model_pts is None else model_pts, nbr, q)
    S = float(np.abs(pts).max())
    dc = np.abs(cen[q] - (m_cen + shift)).max(axis=1)
    dv = np.abs(cov[q] - m_cov).max(axis=(1, 2))
    ratio = np.divide(dv, k * r2, out=np.zeros_like(dv), where=r2 > 0)
    print(f"{what}: moments: centroid off by {dc.max():.3e} (bound {4 * k * U * S:.3e}), covariance by {ratio.max():.3e} of k R2 "
          f"(bound {8 * k * U:.3e})")
    assert dc.max() <= 4 * k * U * S and (dv <= 8 * k * U * k * r2).all(), what
    return dc.max() / (4 * k * U * S) if S > 0 else 0.0, ratio.max() / (8 * k * U)


def check_moments(ctx, pts, k, nbr, queries=None, what=""):
    """the neighbour SET of a large k, through the centroid and the covariance gsx_normals forms (bounds: the docstring of
    test_region_growing_gpu.py)"""
    cen, cov = ctx.debug_normals_moments(pts, k)
    return moments_against_model(cen, cov, pts, k, nbr, queries, what)


def check_lists(pts, nbr, queries=None):
    """every row of a k-NN result on its own: the point itself is there, (d2, index) ascends strictly"""
    P = pts.astype(np.float64)
    q = np.arange(len(pts)) if queries is None else queries
    d = P[nbr] - P[q][:, None, :]
    d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
    assert (nbr == q[:, None]).any(axis=1).all()
    step = np.diff(d2, axis=1)
    assert ((step > 0) | ((step == 0) & (np.diff(nbr, axis=1) > 0))).all()
    return d2
