#!/usr/bin/env python3
"""Smoothness-constrained region growing on libgsx.so (MI355X): the geometry-only segmentation of the reference's
3D_clustering/region_growing.py, written as `property int label` into the PLY - the same field the majority-vote and
the k-means labelers fill (label 0 = the largest region).

The exact k-NN search, the PCA normals and the residuals run as HIP kernels (csrc/normals.hip), the sequential growth
on the host (csrc/region_grow.cpp).  Defaults are the reference's: 2000 neighbours for the normals, 10 for the growth,
residual threshold 0.1, angle threshold 0.05 rad.  `--recolor` additionally overwrites f_dc_0..2 with one uniform random
colour per region, which is all the reference's own output file carries.
There is no CPU path: without libgsx.so and a gfx950 GPU this raises."""
import argparse
import importlib
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)
_ply = importlib.import_module("3d_gaussian_splatting_project_amd.ply_io")
_labeler = importlib.import_module("3d_gaussian_splatting_project_amd.labeler")


def get_pos(plydata):
    """(N, 3) float32 positions of the vertex element."""
    v = plydata["vertex"]
    return np.column_stack((v["x"], v["y"], v["z"])).astype(np.float32)


def segment(points, k_normals=2000, k=10, residual_threshold=0.1, angle_threshold=0.05, ctx=None):
    """-> (labels int32 (N,), normals (N, 3), residuals (N,), number of regions)"""
    own = ctx is None
    if own:
        ctx = _labeler.Context(0)
    try:
        return ctx.region_growing(points, k_normals=min(int(k_normals), len(points)), k=k, residual_threshold=residual_threshold,
                                  angle_threshold=angle_threshold)
    finally:
        if own:
            ctx.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description="Region-growing segmentation of a point cloud / 3DGS PLY.")
    ap.add_argument("--file_path", required=True, help="input PLY")
    ap.add_argument("--save_path", required=True, help="output PLY: every vertex property plus `label`")
    ap.add_argument("--k_normals", type=int, default=2000, help="neighbours of the PCA normals and residuals (capped at N)")
    ap.add_argument("--k", type=int, default=10, help="neighbours the growth visits (2..64)")
    ap.add_argument("--residual_threshold", type=float, default=0.1)
    ap.add_argument("--angle_threshold", type=float, default=0.05, help="radians")
    ap.add_argument("--recolor", action="store_true", help="overwrite f_dc_0..2 with one random colour per region")
    ap.add_argument("--seed", type=int, default=None, help="seed of the --recolor colours")
    args = ap.parse_args(argv)
    plydata = _ply.PlyData.read(args.file_path)
    labels, _, _, n_regions = segment(get_pos(plydata), args.k_normals, args.k, args.residual_threshold, args.angle_threshold)
    print(f"number of segments: {n_regions}")
    if args.recolor:
        colours = np.random.default_rng(args.seed).random((n_regions, 3)).astype(np.float32)
        vertex = plydata["vertex"]
        for ch in range(3):
            vertex[f"f_dc_{ch}"] = colours[labels, ch]
    plydata.write(args.save_path, labels=labels)
    return labels


if __name__ == "__main__":
    main()
