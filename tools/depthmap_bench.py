#!/usr/bin/env python3
"""What a depth view costs, against the frame and the label view of the same build, on one GPU.

tools/labelmap_bench.py's scene and cameras (3 M splats, SH degree 3, 1080p, the viewer's cameras; labels from a Voronoi
partition of space into 150 classes).  Per view, one at a time, from the same run:

  render_view          gsx_render_view with the default options, image left on the device
  label_view           gsx_label_view, map left on the device: the frame's front in one depth phase, label_kernel
  label_view_host      ... with map, weight and total copied to the host (12 bytes per pixel)
  depth_view_surface   gsx_depth_view in surface-only mode, maps left on the device: the same front, depth_kernel stopping at
                       the last surface of a tile
  depth_view_full      gsx_depth_view in full: total, moment and both surface maps copied to the host (20 bytes per pixel) -
                       the sums have no device form, so a full view always carries its copies

Then, with the per-kernel HIP events on, label_kernel and depth_kernel themselves (full and surface-only), and the records
each walk staged.  Writes JSON.

  python tools/depthmap_bench.py [--splats 3000000 --views 8 --width 1920 --height 1080 --classes 150 --repeats 5
                                  --quantile 0.5 --out profiles/depthmap_bench.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splats", type=int, default=3_000_000)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--classes", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quantile", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depthmap_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("depthmap_bench: no GPU; nothing is measured without one")
    from labelmap_bench import voronoi_labels
    pkg = importlib.import_module("3d_gaussian_splatting_project_amd")
    scene = pkg.scene
    W, H, V, C, Q = args.width, args.height, args.views, args.classes, args.quantile
    seed = scene.BASE_SEED + 3
    xyz = scene.make_positions(args.splats, seed)
    a = scene.make_splat_attributes(args.splats, seed, sh_degree=3)
    cams = [pkg.Camera.from_dict(c) for c in scene.make_cameras(max(V, 8), W, H, convention="c2w")[:V]]
    dev = torch.device("cuda", 0)
    labels = voronoi_labels(torch, dev, np.asarray(xyz, np.float32).reshape(-1, 3), C, seed + 11)
    ctx = pkg.Context(0)
    ctx.upload_splats(xyz, a["scale"], a["rot"], a["opacity"], a["f_dc"], labels=labels)
    ctx.upload_sh(a["f_rest"], 3)

    paths = {
        "render_view": lambda cam: ctx.render_view(cam, W, H, to_host=False),
        "label_view": lambda cam: ctx.label_view(cam, W, H, C, to_host=False),
        "label_view_host": lambda cam: ctx.label_view(cam, W, H, C, return_weights=True),
        "depth_view_surface": lambda cam: ctx.depth_view(cam, W, H, Q, to_host=False),
        "depth_view_full": lambda cam: ctx.depth_view(cam, W, H, Q),
    }

    def all_views(fn):
        for cam in cams:
            fn(cam)

    def timed(fn):
        torch.cuda.synchronize()
        ctx.synchronize()
        t0 = time.perf_counter()
        all_views(fn)
        ctx.synchronize()
        return (time.perf_counter() - t0) / V

    def kernel_ms(fn):   # per-kernel events serialise the launches: these times explain, the ones above measure
        ctx.profile(True)
        all_views(fn)
        ctx.synchronize()
        out = {}
        for nm in ctx.profile_names():
            n, ms = ctx.profile_get(nm)
            if n:
                out[nm] = {"launches_per_view": n / V, "ms_per_view": ms / V}
        ctx.profile(False)
        return out

    for fn in paths.values():             # warm-up: sizes the pair buffers of every path, checks the labels once
        all_views(fn)
    t = {k: [] for k in paths}
    for _ in range(max(3, args.repeats)):
        for k, fn in paths.items():
            t[k].append(timed(fn))
    staged, surfaces = {"label": [], "depth_full": [], "depth_surface": []}, []
    for cam in cams:
        paths["label_view"](cam)
        staged["label"].append(ctx.render_num_pairs_consumed())
        paths["depth_view_surface"](cam)
        staged["depth_surface"].append(ctx.render_num_pairs_consumed())
        surfaces.append(ctx.depth_num_surface())
        paths["depth_view_full"](cam)
        staged["depth_full"].append(ctx.render_num_pairs_consumed())
    frame = ctx.depth_view(cams[0], W, H, Q)
    kernels = {k: kernel_ms(paths[k]) for k in ("label_view", "depth_view_surface", "depth_view_full")}
    ctx.close()
    med = {k: 1e3 * float(np.median(v)) for k, v in t.items()}
    has = frame.surface_index >= 0
    res = {"what": "one depth view against one rendered frame and one label view of the same context, scene and cameras; one view at a time",
           "splats": args.splats, "views": V, "image": [W, H], "classes": C, "quantile": Q, "repeats": max(3, args.repeats),
           "ms_per_view": {k: [1e3 * x for x in v] for k, v in t.items()}, "median_ms": med,
           "depth_surface_over_label": med["depth_view_surface"] / med["label_view"],
           "depth_full_over_label_host": med["depth_view_full"] / med["label_view_host"],
           "depth_surface_over_render": med["depth_view_surface"] / med["render_view"],
           "label_kernel_ms": kernels["label_view"].get("label", {}).get("ms_per_view", 0.0),
           "depth_kernel_full_ms": kernels["depth_view_full"].get("depth", {}).get("ms_per_view", 0.0),
           "depth_kernel_surface_ms": kernels["depth_view_surface"].get("depth", {}).get("ms_per_view", 0.0),
           "records_staged_per_view": {k: float(np.mean(v)) for k, v in staged.items()},
           "pixels_with_a_surface_per_view": float(np.mean(surfaces)),
           "first_frame": {"surface_share": float(has.mean()), "median_surface_z": float(np.nanmedian(frame.surface_z)) if has.any() else None,
                           "median_expected_z": float(np.nanmedian(frame.expected_z)) if (frame.total > 0).any() else None},
           "kernels": kernels}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    brief = {k: res[k] for k in ("median_ms", "depth_surface_over_label", "depth_full_over_label_host", "label_kernel_ms",
                                 "depth_kernel_full_ms", "depth_kernel_surface_ms", "records_staged_per_view")}
    print(json.dumps(brief), flush=True)


if __name__ == "__main__":
    main()
