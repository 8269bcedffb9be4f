#!/usr/bin/env python3
"""What a label view costs, against the frame and the lift view of the same build, on one GPU.

tools/lift_bench.py's scene (3 M splats, SH degree 3, 1080p, the viewer's cameras).  The splats carry labels from a Voronoi
partition of SPACE into 150 classes (each splat takes the class of the nearest of 150 random sites inside the cloud); a second
run gives every splat one class.  Per view, one at a time, no per-kernel events:

  label_view    gsx_label_view with label_out left on the device: the frame's front in one depth phase, label_kernel
  render_view   gsx_render_view of the same context, scene and cameras with the default options
  lift_view     gsx_lift_view_device of Voronoi class maps (400 sites, 150 classes) at 1080p, device-resident

Next to the times: the walks per tile with a list (gsx_label_num_passes over the one-class run's count of such tiles) and the
share of those tiles whose list holds a single label.  Then, with the per-kernel HIP events on, label_kernel and lift_kernel
themselves.  Writes JSON.

  python tools/labelmap_bench.py [--splats 3000000 --views 8 --width 1920 --height 1080 --classes 150 --repeats 5
                                  --out profiles/labelmap_bench.json]
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


def voronoi_labels(torch, dev, xyz, classes, seed):
    """int32 (n,): the index of the nearest of `classes` sites drawn from the splats themselves"""
    rng = np.random.default_rng(seed)
    sites = torch.from_numpy(np.ascontiguousarray(xyz[rng.choice(len(xyz), classes, replace=False)])).to(dev)
    out = np.empty(len(xyz), np.int32)
    for lo in range(0, len(xyz), 1 << 18):
        pts = torch.from_numpy(np.ascontiguousarray(xyz[lo:lo + (1 << 18)])).to(dev)
        out[lo:lo + len(pts)] = torch.cdist(pts, sites).argmin(1).to(torch.int32).cpu().numpy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splats", type=int, default=3_000_000)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--classes", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "labelmap_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("labelmap_bench: no GPU; nothing is measured without one")
    pkg = importlib.import_module("3d_gaussian_splatting_project_amd")
    scene = pkg.scene
    W, H, V, C = args.width, args.height, args.views, args.classes
    seed = scene.BASE_SEED + 3
    xyz = scene.make_positions(args.splats, seed)
    a = scene.make_splat_attributes(args.splats, seed, sh_degree=3)
    cams = [pkg.Camera.from_dict(c) for c in scene.make_cameras(max(V, 8), W, H, convention="c2w")[:V]]
    dev = torch.device("cuda", 0)
    maps = [torch.from_numpy(scene.make_segmap_gpu(torch, 0, H, W, C, 3000 + v)).to(dev) for v in range(V)]
    labelings = {"voronoi": voronoi_labels(torch, dev, np.asarray(xyz, np.float32).reshape(-1, 3), C, seed + 11),
                 "one_class": np.zeros(args.splats, np.int32)}
    ctx = pkg.Context(0)
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)

    def render_all():
        for cam in cams:
            ctx.render_view(cam, W, H, to_host=False)

    def lift_all():
        for cam, m in zip(cams, maps):
            ctx.lift_view(cam, m)

    def label_all():
        for cam in cams:
            ctx.label_view(cam, W, H, C, to_host=False)

    def timed(fn):
        torch.cuda.synchronize()
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) / V

    def kernel_ms(fn):   # per-kernel events serialise the launches: these times explain, the ones above measure
        ctx.profile(True)
        fn()
        ctx.synchronize()
        out = {}
        for nm in ctx.profile_names():
            n, ms = ctx.profile_get(nm)
            if n:
                out[nm] = {"launches_per_view": n / V, "ms_per_view": ms / V}
        ctx.profile(False)
        return out

    runs = {}
    for name, labels in labelings.items():
        ctx.upload_splats(xyz, a["scale"], a["rot"], a["opacity"], a["f_dc"], labels=labels)
        ctx.upload_sh(a["f_rest"], 3)
        ctx.lift_begin(C)
        render_all()                      # warm-up: sizes the pair buffers of every path, checks the labels once
        lift_all()
        label_all()
        t = {"render_view": [], "lift_view": [], "label_view": []}
        for _ in range(max(3, args.repeats)):
            t["render_view"].append(timed(render_all))
            t["lift_view"].append(timed(lift_all))
            t["label_view"].append(timed(label_all))
        passes, single, staged, pairs = [], [], [], []
        for cam in cams:
            ctx.label_view(cam, W, H, C, to_host=False)
            passes.append(ctx.label_num_passes())
            single.append(ctx.label_num_single_tiles())
            staged.append(ctx.render_num_pairs_consumed())
            pairs.append(ctx.render_num_pairs())
        frame = ctx.label_view(cams[0], W, H, C)
        k_label, k_lift = kernel_ms(label_all), kernel_ms(lift_all)
        med = {k: 1e3 * float(np.median(v)) for k, v in t.items()}
        runs[name] = {
            "ms_per_view": {k: [1e3 * x for x in v] for k, v in t.items()}, "median_ms": med,
            "label_over_render": med["label_view"] / med["render_view"], "label_over_lift": med["label_view"] / med["lift_view"],
            "walks_per_view": float(np.mean(passes)), "one_label_tiles_per_view": float(np.mean(single)), "tiles": ntiles,
            "pairs_per_view": float(np.mean(pairs)), "records_staged_first_walk_per_view": float(np.mean(staged)),
            "label_kernel_ms": k_label.get("label", {}).get("ms_per_view", 0.0),
            "lift_kernel_ms": k_lift.get("lift", {}).get("ms_per_view", 0.0),
            "labels_in_first_frame": int(len(np.unique(frame))), "unlabelled_share_first_frame": float((frame == -1).mean()),
            "kernels_label_view": k_label,
        }
    ctx.close()
    listed = runs["one_class"]["walks_per_view"]          # one class: every tile with a list walks it once
    for r in runs.values():
        r["tiles_with_a_list_per_view"] = listed
        r["walks_per_listed_tile"] = r["walks_per_view"] / listed if listed else 0.0
        r["one_label_share_of_listed_tiles"] = r["one_label_tiles_per_view"] / listed if listed else 0.0
    res = {"what": "one label view against one rendered frame and one lift view of the same context, scene and cameras; label map left "
                   "on the device; one view at a time",
           "splats": args.splats, "views": V, "image": [W, H], "classes": C, "repeats": max(3, args.repeats),
           "window": pkg.labelmap_constants()["window"], "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    brief = {name: {k: r[k] for k in ("median_ms", "label_over_render", "label_over_lift", "walks_per_listed_tile",
                                      "one_label_share_of_listed_tiles", "label_kernel_ms", "lift_kernel_ms")} for name, r in runs.items()}
    print(json.dumps(brief), flush=True)


if __name__ == "__main__":
    main()
