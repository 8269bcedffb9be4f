#!/usr/bin/env python3
"""Times the label split (csrc/split.hip) on the MI355X: bench.py's 3 M-point blob scene, a Voronoi-like class field (256
random sites, site s carries class s % 8, a point takes the class of its nearest site), k = 16.

    python tools/split_bench.py   -> profiles/split_bench.json   (needs the GPU)

After one warm-up run, the median of 5 runs of each of
  split          the whole gsx_split_labels call (wall): host checks, binning, the lists, the components, labels up and down
  split_lists    gsx_split_labels_lists over the device lists that call left behind (wall): the components alone
  split_lists_d  the same with max_dist = 0.05, i.e. with the coordinate gathers (wall)
  kernels        per profile name (split_hook = init + hook, split_flatten, split_sizes = count + compact, split_relabel =
                 scatter + relabel, and nn_knn next to them): HIP-event milliseconds of one call, without and with max_dist
A first record of a new capability on the named scene: not part of bench.py, and no threshold is attached to any of it."""
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, K, SITES, CLASSES, MAX_DIST, REPS = 3_000_000, 16, 256, 8, 0.05, 5
KERNELS = ("split_hook", "split_flatten", "split_sizes", "split_relabel")


def make_labels(pos, rng):
    sites = rng.uniform(-4.0, 4.0, (SITES, 3)).astype(np.float32)
    lab = np.empty(len(pos), np.int32)
    for s in range(0, len(pos), 1 << 16):
        d = pos[s:s + (1 << 16), None, :] - sites[None, :, :]
        lab[s:s + (1 << 16)] = (d * d).sum(axis=2).argmin(axis=1) % CLASSES
    return lab


def median_of(fn):
    fn()
    out = [fn() for _ in range(REPS)]
    return statistics.median(out), out


def main():
    g = importlib.import_module("3d_gaussian_splatting_project_amd")
    pos = g.scene.make_positions(N, g.scene.BASE_SEED + 3)
    lab = make_labels(pos, np.random.default_rng(5))
    res = {"workload": f"{N} points (bench.py's blob scene), Voronoi class field of {SITES} sites in {CLASSES} classes, k = {K}",
           "measured_on": "one MI355X", "reps": REPS, "statistic": "median of 5 after 1 warm-up", "max_dist": MAX_DIST}
    with g.Context(0) as ctx:
        def wall(fn):
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3

        def kernels(max_dist):
            ctx.profile(True)
            ctx.split_labels(pos, lab, k=K, max_dist=max_dist)
            ms = {name: ctx.profile_get(name)[1] for name in KERNELS + ("nn_knn",)}
            ctx.profile(False)
            return ms

        res["split_ms"], res["split_ms_runs"] = median_of(lambda: wall(lambda: ctx.split_labels(pos, lab, k=K)))
        res["split_lists_ms"], res["split_lists_ms_runs"] = median_of(lambda: wall(lambda: ctx.split_labels_lists(None, lab, k=K)))
        res["split_lists_d_ms"], res["split_lists_d_ms_runs"] = median_of(
            lambda: wall(lambda: ctx.split_labels_lists(None, lab, points=pos, max_dist=MAX_DIST, k=K)))
        for tag, d in (("kernel_ms", None), ("kernel_ms_max_dist", MAX_DIST)):
            runs = [kernels(d) for _ in range(REPS + 1)][1:]
            res[tag] = {name: statistics.median(r[name] for r in runs) for name in runs[0]}
            res[tag + "_runs"] = runs
        ctx.profile(True)
        ctx.split_labels(pos, lab, k=K)
        res["launches"] = {name: ctx.profile_get(name)[0] for name in KERNELS}
        ctx.profile(False)
        for tag, d in (("result", None), ("result_max_dist", MAX_DIST)):
            _, table = ctx.split_labels(pos, lab, k=K, max_dist=d)
            res[tag] = {"components": ctx.split_components, "instances_of_100_points_or_more": int((table["size"] >= 100).sum()),
                        "largest_sizes": [int(s) for s in table["size"][:8]]}
        res["hook_model_bytes"] = {"lists": N * K * 4, "label_gathers": N * K * 4, "coordinate_gathers_with_max_dist": N * K * 12,
                                   "parent_init": N * 4}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    json.dump(res, open(os.path.join(ROOT, "profiles", "split_bench.json"), "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
