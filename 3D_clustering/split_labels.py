#!/usr/bin/env python3
"""Classes into objects on libgsx.so (MI355X): the connected components of every label over the k-nearest-neighbour graph,
applied to the `property int label` one of the three labelers (majority vote, k-means, region growing) wrote into a PLY.

The viewer selects, recolours, hides and moves the splats that share one label value.  A semantic class (SegFormer,
`--mask2former_map classes`) gives every chair of a scene the same value, and a k-means cluster can hold pieces that do not
touch.  Here two points are joined when one is among the other's k nearest points, both carry the same label and (with
--max_dist) they are no farther apart than that; a connected component is an object.  The largest object gets id 0, objects
below --min_size points or behind --max_instances get -1 (3D_clustering/smooth_labels.py --ignore_label -1 --fill_only
repairs those), and so do the points whose label is --ignore_label.  include/gsx.h states the rule in full.  The search and
the components run as HIP kernels (csrc/normals.hip, csrc/split.hip); every other property of the file is written back
unchanged.  There is no CPU path: without libgsx.so and a gfx950 GPU this raises."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)
_ply = importlib.import_module("3d_gaussian_splatting_project_amd.ply_io")
_labeler = importlib.import_module("3d_gaussian_splatting_project_amd.labeler")

LABEL_LIMIT = 1 << 24   # the element's item assignment goes through float32: integers beyond +-2^24 would not survive it


def get_pos(plydata):
    """(N, 3) float32 positions of the vertex element."""
    v = plydata["vertex"]
    return np.column_stack((v["x"], v["y"], v["z"])).astype(np.float32)


def get_labels(plydata):
    """int32 (N,) labels of the vertex element; raises when the file carries none or they do not fit the write path."""
    v = plydata["vertex"]
    if "label" not in v.properties:
        raise ValueError("the PLY has no `label` property: run one of the labelers first")
    raw = np.asarray(v["label"])
    labels = raw.astype(np.int32)
    if not np.array_equal(labels, raw) or (np.abs(labels.astype(np.int64)) > LABEL_LIMIT).any():
        raise ValueError(f"labels must be integers within +-2^24 ({LABEL_LIMIT}): the PLY write path goes through float32")
    return labels


def split(points, labels, k=16, max_dist=None, min_size=1, max_instances=0, ignore_label=None, ctx=None):
    """-> (instance ids int32 (N,), table {"label", "size", "rep"})"""
    own = ctx is None
    if own:
        ctx = _labeler.Context(0)
    try:
        return ctx.split_labels(points, labels, k=min(int(k), len(points)), max_dist=max_dist, min_size=min_size,
                                max_instances=max_instances, ignore_label=ignore_label)
    finally:
        if own:
            ctx.close()


def table_rows(table):
    """the instance table as the JSON list --table_path writes"""
    return [{"id": m, "label": int(l), "size": int(s)} for m, (l, s) in enumerate(zip(table["label"], table["size"]))]


def parser():
    def at_least(low, high=None):
        def parse(text):
            v = int(text)
            if v < low or (high is not None and v > high):
                raise argparse.ArgumentTypeError(f"must be at least {low}" + (f" and at most {high}" if high is not None else ""))
            return v
        return parse

    def positive(text):
        v = float(text)
        if not v > 0:
            raise argparse.ArgumentTypeError("must be positive")
        return v

    ap = argparse.ArgumentParser(description="Connected components of every `label` of a point cloud / 3DGS PLY over its "
                                 "k-nearest-neighbour graph: classes into objects.")
    ap.add_argument("--file_path", required=True, help="input PLY with a `label` property")
    ap.add_argument("--save_path", required=True, help="output PLY: every vertex property unchanged, `label` = the instance id")
    ap.add_argument("--k", type=at_least(2, 64), default=16, help="nearest points a point may be joined to, itself included (2 .. 64, capped at N)")
    ap.add_argument("--max_dist", type=positive, default=None, help="neighbours farther apart than this are not joined (default: no cut)")
    ap.add_argument("--min_size", type=at_least(1), default=1, help="objects of fewer points become -1")
    ap.add_argument("--max_instances", type=at_least(0), default=0, help="keep only this many of the largest objects (0: all)")
    ap.add_argument("--ignore_label", type=int, default=None, help="points with this label join nothing and stay -1 (e.g. -1)")
    ap.add_argument("--table_path", default=None, help="write the instance table here: a JSON list of {id, label, size}")
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    plydata = _ply.PlyData.read(args.file_path)
    labels, table = split(get_pos(plydata), get_labels(plydata), args.k, args.max_dist, args.min_size, args.max_instances, args.ignore_label)
    if len(table["size"]) > LABEL_LIMIT:
        raise ValueError(f"{len(table['size'])} instances: ids beyond 2^24 would not survive the PLY write path (raise --min_size)")
    print(f"{len(table['size'])} instances, {int((labels < 0).sum())} points without one")
    plydata["vertex"]["label"] = labels   # in place: the property keeps its position and type
    plydata.write(args.save_path)
    if args.table_path:
        with open(args.table_path, "w") as f:
            json.dump(table_rows(table), f, indent=1)
    return labels


if __name__ == "__main__":
    main()
