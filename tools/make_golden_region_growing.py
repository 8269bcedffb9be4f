#!/usr/bin/env python3
"""Generate the region-growing labeler's golden vectors (tests/golden/region_growing.npz).

Runs ONLY in the build container, where /root/reference exists.  It imports the reference's own
3D_clustering/region_growing.py (plyfile, which is not installed, is replaced by an inert empty module; scipy is the
real one), runs compute_normals, compute_residuals and segmentation_3D on seeded scenes and records inputs, normals,
residuals, regions (as labels: position in the reference's size-sorted list) and the k-NN lists of the reference's own
KD-tree (scipy.spatial.KDTree.query, recorded from segmentation_3D's calls and completed for the points it never
queries).  Only inputs and outputs are stored; no reference source travels.

On every scene it also runs the numpy model (tests/region_growing_model.py) and ASSERTS
  (a) no two candidate distances of any query are equal (the k + 1 nearest are strictly ascending),
  (b) the model reproduces the reference's regions exactly as sets, and its k-NN lists equal the KD-tree's,
and records
  (c) the model's largest normal angle and residual difference to the reference (the float32 effect: the tolerance
      the GPU test derives its bound from),
  (d) the smallest accept / reject margin met during the growth (must be >= 1e-9),
  (e) the fraction of points whose eigen-gap (l1 - l0) / l2 is below 1e-3 (must be < 1 %).
A scene that fails is replaced by another seed, not waived.
Usage:  python tools/make_golden_region_growing.py
"""
import contextlib
import importlib.util
import io
import json
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/3D_clustering/region_growing.py"
OUT = os.path.join(HERE, "..", "tests", "golden", "region_growing.npz")
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import region_growing_model as model  # noqa: E402


def import_reference():
    if "plyfile" not in sys.modules:
        try:
            __import__("plyfile")
        except ImportError:
            m = types.ModuleType("plyfile")
            m.PlyData = m.PlyElement = object
            sys.modules["plyfile"] = m
    spec = importlib.util.spec_from_file_location("ref_region_growing", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def plane_patch(rng, n, centre, u, v, size, noise):
    u, v = np.asarray(u, float), np.asarray(v, float)
    w = np.cross(u, v)
    w /= np.linalg.norm(w)
    a = rng.uniform(-size, size, (n, 2))
    return np.asarray(centre) + a[:, :1] * u + a[:, 1:] * v + rng.normal(0, noise, (n, 1)) * w


def make_scene(name, rng):
    if name == "patches":      # separated planar patches of different orientation
        pts = np.vstack([plane_patch(rng, 600, (0, 0, 0), (1, 0, 0), (0, 1, 0), 1.0, 0.004),
                         plane_patch(rng, 500, (4, 0, 1), (1, 0, 0.3), (0, 1, 0.2), 1.0, 0.004),
                         plane_patch(rng, 500, (0, 4, -1), (0, 1, 1), (1, 0, 0), 1.0, 0.004)])
    elif name == "touching":   # two sheets that meet along an edge
        pts = np.vstack([plane_patch(rng, 900, (0, 0, 0), (1, 0, 0), (0, 1, 0), 1.0, 0.003),
                         plane_patch(rng, 900, (1, 0, 1), (0, 0, 1), (0, 1, 0), 1.0, 0.003)])
    elif name == "sphere":     # noisy sphere: the normal turns everywhere
        d = rng.normal(size=(2400, 3))
        pts = d / np.linalg.norm(d, axis=1, keepdims=True) * (1.0 + rng.normal(0, 0.01, (2400, 1)))
    elif name == "cli":        # the front-end's thresholds (rg.py:278) on a box corner
        pts = np.vstack([plane_patch(rng, 700, (0, 0, 0), (1, 0, 0), (0, 1, 0), 1.0, 0.01),
                         plane_patch(rng, 700, (1, 0, 1), (0, 0, 1), (0, 1, 0), 1.0, 0.01),
                         plane_patch(rng, 700, (0, 1, 1), (1, 0, 0), (0, 0, 1), 1.0, 0.01)])
    else:
        raise KeyError(name)
    return np.ascontiguousarray(pts[rng.permutation(len(pts))], np.float32)


SPECS = [  # name, k_normals, k, residual_threshold, angle_threshold
    ("patches", 30, 8, 0.02, 0.15),
    ("touching", 40, 10, 0.02, 0.12),
    ("sphere", 60, 10, 0.02, 0.2),
    ("cli", 50, 10, 0.1, 0.05),
]


def run_scene(rg, name, kn, k, rt, at, seed):
    rng = np.random.default_rng(seed)
    pts = make_scene(name, rng)
    n = len(pts)
    assert len(np.unique(pts, axis=0)) == n, "duplicated position"
    recorded = {}
    where = {p.tobytes(): i for i, p in enumerate(pts)}
    real_tree = rg.KDTree

    class RecordingTree(real_tree):
        def query(self, x, k=1, *a, **kw):
            d, i = super().query(x, k, *a, **kw)
            x = np.asarray(x)
            if x.ndim == 1 and x.dtype == np.float32:
                recorded.setdefault((where[x.tobytes()], int(k)), np.asarray(i).copy())
            return d, i

    rg.KDTree = RecordingTree
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            nrm = rg.compute_normals(pts, kn)
            res = rg.compute_residuals(pts, nrm, kn)
            regions = rg.segmentation_3D(pts, nrm, res, rt, at, k)
    finally:
        rg.KDTree = real_tree
    ref_labels = model.labels_from_regions(regions, n)
    ref_knn = np.asarray(real_tree(pts).query(pts, k)[1], np.int32)
    for (i, kk), lst in recorded.items():
        if kk == k:
            assert np.array_equal(ref_knn[i], lst), "the KD-tree answered one query in two ways"
    ref_knn_normals = np.stack([recorded[(i, kn)] for i in range(n)])
    # ---- the model ----
    m_knn, d2 = model.knn(pts, k, with_next=True)
    m_knn_n, d2n = model.knn(pts, kn, with_next=True)
    assert (np.diff(d2, axis=1) > 0).all() and (np.diff(d2n, axis=1) > 0).all(), "(a) equal candidate distances"
    assert np.array_equal(m_knn, ref_knn), "(b) k-NN lists differ from the KD-tree's"
    assert np.array_equal(np.sort(m_knn_n, axis=1), np.sort(ref_knn_normals, axis=1)), "(b) neighbour sets differ"
    m_nrm, m_res, _, gap = model.normals_from_neighbours(pts, m_knn_n)
    m_labels, m_nreg, margin = model.grow(m_nrm, m_res, m_knn, rt, at, with_margin=True)
    assert model.same_regions(ref_labels, m_labels), "(b) the model's regions differ from the reference's"
    r_labels, _ = model.grow(nrm, res, ref_knn, rt, at)
    assert model.same_regions(ref_labels, r_labels), "the model's growth differs from the reference's on its own inputs"
    assert margin >= 1e-9, f"(d) margin {margin}"
    low_gap = float((gap <= 1e-3).mean())
    assert low_gap < 0.01, f"(e) {low_gap:.3%} of the points have a degenerate eigen-gap"
    cosang = np.einsum("ij,ij->i", m_nrm, nrm)
    free = res < 1e-6                      # the flip rule's dot product is within rounding of zero: sign-free there
    cosang = np.where(free, np.abs(cosang), cosang)
    cross = np.linalg.norm(np.cross(m_nrm, nrm), axis=1)
    ang = np.arctan2(cross, cosang)        # accurate for small angles, pi for a flipped sign
    tol_angle, tol_res = float(ang.max()), float(np.abs(m_res - res).max())
    print(f"{name}: n {n} regions {len(regions)} sizes {[len(r) for r in regions[:6]]} | model vs reference: angle {tol_angle:.3e} rad, "
          f"residual {tol_res:.3e} | margin {margin:.3e} | low gap {low_gap:.3%}")
    return dict(points=pts, k_normals=kn, k=k, residual_threshold=rt, angle_threshold=at, normals=nrm, residuals=res,
                labels=ref_labels, knn=ref_knn, n_regions=len(regions), tol_angle=tol_angle, tol_residual=tol_res, margin=margin,
                low_gap=low_gap)


def time_reference(rg):
    """seconds per point of compute_normals + compute_residuals on a 20 000-point scene"""
    rng = np.random.default_rng(7)
    pts = rng.uniform(-1, 1, (20000, 3)).astype(np.float32)
    out = {}
    for k in (2000, 64):
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.perf_counter()
            nrm = rg.compute_normals(pts, k)
            rg.compute_residuals(pts, nrm, k)
            out[f"reference_seconds_per_point_k{k}"] = (time.perf_counter() - t0) / len(pts)
    return out


def main():
    rg = import_reference()
    flat, names = {}, []
    for j, (name, kn, k, rt, at) in enumerate(SPECS):
        seed = 20250100 + j
        for attempt in range(5):
            try:
                case = run_scene(rg, name, kn, k, rt, at, seed + 1000 * attempt)
                break
            except AssertionError as e:
                print(f"{name}: seed {seed + 1000 * attempt} rejected: {e}")
        else:
            raise SystemExit(f"{name}: no seed passed")
        names.append(name)
        for key, val in case.items():
            flat[f"{name}/{key}"] = np.asarray(val)
    notes = {"scenes": names}
    if "--no-timing" not in sys.argv:
        notes.update(time_reference(rg))
    print(notes)
    flat["cases"] = np.asarray(names)
    flat["notes"] = np.asarray(json.dumps(notes))
    np.savez_compressed(OUT, **flat)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
