#!/usr/bin/env python3
"""Times the label filter (csrc/smooth.hip) on the MI355X: bench.py's 3 M-point blob scene, labels = the octant of the
point (8 classes) with 10 % redrawn at random, k = 16, rounds = 3.

    python tools/smooth_bench.py   -> profiles/smooth_bench.json   (needs the GPU)

After one warm-up run, the median of 5 runs of each of
  knn           gsx_knn alone at k = 16 (wall time of the call)
  smooth        the whole gsx_smooth_labels call (wall), the default path: lists once, then list rounds
  list_round    one list round, from the context's profile counters (kernel "smooth_list": total / launches)
  search_round  one search-form round under option "smooth_search" = 1 (kernel "smooth_search")
and next to them scipy's cKDTree.query(workers=16) plus a numpy mode over the same lists, if scipy imports - one run, on
whatever CPU this host has.  Not part of bench.py; no threshold is attached to any of it."""
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, K, ROUNDS, CLASSES, NOISE, REPS = 3_000_000, 16, 3, 8, 0.10, 5


def make_labels(pos, rng):
    lab = ((pos[:, 0] > 0).astype(np.int32) | ((pos[:, 1] > 0).astype(np.int32) << 1) | ((pos[:, 2] > 0).astype(np.int32) << 2))
    flip = rng.random(len(pos)) < NOISE
    lab[flip] = rng.integers(0, CLASSES, int(flip.sum()))
    return lab.astype(np.int32)


def median_of(fn):
    fn()
    out = []
    for _ in range(REPS):
        out.append(fn())
    return statistics.median(out), out


def cpu_side(pos, lab):
    try:
        from scipy.spatial import cKDTree
    except ImportError as e:
        return {"ran": False, "why": f"scipy does not import here ({e})"}
    t0 = time.perf_counter()
    tree = cKDTree(pos.astype(np.float64))
    t_build = time.perf_counter() - t0
    t0 = time.perf_counter()
    _, idx = tree.query(pos.astype(np.float64), K, workers=16)
    t_query = time.perf_counter() - t0
    t0 = time.perf_counter()
    cur = lab
    for _ in range(ROUNDS):                            # a plain mode (most frequent, smallest among equals): not the filter's tie rule
        new = np.empty_like(cur)
        for s in range(0, len(cur), 1 << 18):
            votes = np.sort(cur[idx[s:s + (1 << 18)]], axis=1)
            counts = (votes[:, :, None] == votes[:, None, :]).sum(axis=2)
            new[s:s + (1 << 18)] = votes[np.arange(len(votes)), counts.argmax(axis=1)]
        cur = new
    t_mode = time.perf_counter() - t0
    return {"ran": True, "what": f"scipy cKDTree.query(k={K}, workers=16) + a numpy mode per round, {ROUNDS} rounds", "cpus": len(os.sched_getaffinity(0)),
            "tree_build_s": t_build, "query_s": t_query, "mode_rounds_s": t_mode}


def main():
    g = importlib.import_module("3d_gaussian_splatting_project_amd")
    pos = g.scene.make_positions(N, g.scene.BASE_SEED + 3)
    lab = make_labels(pos, np.random.default_rng(5))
    res = {"workload": f"{N} points (bench.py's blob scene), {CLASSES} classes, {NOISE:.0%} noise, k = {K}, rounds = {ROUNDS}", "reps": REPS,
           "statistic": "median"}
    with g.Context(0) as ctx:
        def wall(fn):
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3

        def per_round(name, search):
            ctx.set_option("smooth_search", search)
            ctx.profile(True)
            _, changed = ctx.smooth_labels(pos, lab, k=K, rounds=ROUNDS)
            launches, ms = ctx.profile_get(name)
            ctx.profile(False)
            ctx.set_option("smooth_search", 0)
            return ms / max(launches, 1)

        res["knn_ms"], res["knn_ms_runs"] = median_of(lambda: wall(lambda: ctx.knn(pos, K)))
        res["smooth_ms"], res["smooth_ms_runs"] = median_of(lambda: wall(lambda: ctx.smooth_labels(pos, lab, k=K, rounds=ROUNDS)))
        res["list_round_ms"], res["list_round_ms_runs"] = median_of(lambda: per_round("smooth_list", 0))
        res["search_round_ms"], res["search_round_ms_runs"] = median_of(lambda: per_round("smooth_search", 1))
        out, changed = ctx.smooth_labels(pos, lab, k=K, rounds=ROUNDS)
        res["changed_per_round"] = changed
        res["list_round_model_bytes"] = N * K * 4 + N * K * 4 + 8 * N
    res["cpu"] = cpu_side(pos, lab)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    json.dump(res, open(os.path.join(ROOT, "profiles", "smooth_bench.json"), "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
