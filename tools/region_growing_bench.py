#!/usr/bin/env python3
"""Times the region-growing labeler's pieces on the benchmark scene's positions and prints ONE JSON line:
gsx_normals with k = 2000 and k = 64, gsx_knn with k = 10, and the host growth, each as the median of --runs runs
after --warmup warm-up runs.  `wall` is the whole call as a user sees it (host binning, upload, kernel, download; the
calls end synchronised), `kernel` the search kernel alone between HIP events on the context's stream
(gsx_profile_get).  Nothing is promised: the capability is new, the figures are a record.
Kernel times are HIP events recorded around the launch on the context's stream, not a rocprofv3 kernel trace.  The line
also carries the device name, the scene, the commit (--commit, for a tree that travels without its .git; else git's HEAD
plus a dirty flag) and the reference's own seconds per point as the fixture generator measured them
(tests/golden/region_growing.npz notes).
Usage:  python tools/region_growing_bench.py [--n 3000000] [--runs 5] [--warmup 1] [--skip-k2000] [--commit ID]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-k2000", action="store_true")
    ap.add_argument("--commit", default=None, help="commit id to record when the tree has no .git")
    args = ap.parse_args()
    pkg = importlib.import_module("3d_gaussian_splatting_project_amd")
    pts = np.ascontiguousarray(pkg.scene.make_positions(args.n, pkg.scene.BASE_SEED), np.float32)
    out = {"n": args.n, "runs": args.runs, "warmup": args.warmup,
           "scene": f"scene.make_positions({args.n}, BASE_SEED): the benchmark scene's positions",
           "kernel_clock": "HIP events around the launch (gsx_profile_get)", "wall_clock": "time.perf_counter around the synchronous call"}
    out["commit"] = args.commit
    if out["commit"] is None:
        try:
            head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
            dirty = bool(subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True).stdout.strip())
            out["commit"] = (head + ("+dirty" if dirty else "")) or None
        except OSError:
            pass
    try:
        import torch
        out["device"] = torch.cuda.get_device_name(0)
    except Exception:
        out["device"] = None
    try:
        notes = json.loads(str(np.load(os.path.join(ROOT, "tests", "golden", "region_growing.npz"))["notes"]))
        out["reference_seconds_per_point"] = {k.rsplit("_", 1)[1]: v for k, v in notes.items() if k.startswith("reference_seconds_per_point")}
    except (OSError, KeyError, ValueError):
        out["reference_seconds_per_point"] = None
    with pkg.Context(0) as ctx:
        lib = ctx._lib
        lib.gsx_profile_enable(ctx.h, 1)

        def timed(name, kernel, fn):
            wall, kern = [], []
            res = None
            for r in range(args.warmup + args.runs):
                lib.gsx_profile_reset(ctx.h)
                t0 = time.perf_counter()
                res = fn()
                dt = time.perf_counter() - t0
                launches, ms = C.c_int64(0), C.c_double(0.0)
                lib.gsx_profile_get(ctx.h, kernel.encode(), C.byref(launches), C.byref(ms))
                if r >= args.warmup:
                    wall.append(dt)
                    kern.append(ms.value / 1e3)
                print(f"{name} run {r}: wall {dt:.3f} s, kernel {ms.value / 1e3:.3f} s", file=sys.stderr, flush=True)
            out[name] = {"wall_s_median": statistics.median(wall), "kernel_s_median": statistics.median(kern),
                         "wall_s": [round(v, 4) for v in wall]}
            return res

        nbr = timed("knn_k10", "nn_knn", lambda: ctx.knn(pts, 10))
        nrm, res = timed("normals_k64", "nn_normals", lambda: ctx.normals(pts, 64))
        if not args.skip_k2000:
            nrm, res = timed("normals_k2000", "nn_normals", lambda: ctx.normals(pts, 2000))
    grow = []
    for r in range(args.warmup + args.runs):
        t0 = time.perf_counter()
        labels, nreg = pkg.region_grow(nrm, res, nbr, 0.1, 0.05)
        if r >= args.warmup:
            grow.append(time.perf_counter() - t0)
    out["region_grow_host"] = {"wall_s_median": statistics.median(grow), "wall_s": [round(v, 4) for v in grow], "n_regions": nreg,
                               "normals_from": "k2000" if not args.skip_k2000 else "k64"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
