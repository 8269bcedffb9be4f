#!/usr/bin/env python3
"""Cost of the viewer's label edits (gsx_render_set_edits) on the benchmark's render scene: 3 M splats, SH degree 3, 1080p,
four cameras - views/s through gsx_render_views (four frames in flight) without an edit state and with a representative one
(labels = Morton-cell ids modulo 150; 10 classes hidden, 10 recoloured, 2 displaced, highlight on), measured in ONE process, the
two forms interleaved; the time of the edit-code kernel; (bin, splat) pairs of one view with and without the hidden classes.
Prints one JSON line.

    python tools/render_edits_cost.py [--splats N] [--rounds R]
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


def morton_labels(xyz, classes):
    q = np.clip(((xyz + 8.0) / 16.0 * 32.0).astype(np.int64), 0, 31)
    code = np.zeros(len(xyz), np.int64)
    for b in range(5):
        for a in range(3):
            code |= ((q[:, a] >> b) & 1) << (3 * b + a)
    return (code % classes).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splats", type=int, default=3_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    pkg = importlib.import_module("3d_gaussian_splatting_project_amd")
    scene = pkg.scene
    n, W, H = args.splats, args.width, args.height
    seed = scene.BASE_SEED + 3
    xyz = scene.make_positions(n, seed)
    a = scene.make_splat_attributes(n, seed, sh_degree=3)
    labels = morton_labels(xyz, 150)
    cams = scene.make_cameras(8, W, H, convention="c2w")[:4]
    state = dict(selected=30, selection_mode=True, colours={k: (k / 20.0, 1.0 - k / 20.0, 0.5) for k in range(10, 20)},
                 displacements={20: (0.5, 0.0, 0.0), 21: (0.0, -0.5, 0.25)}, hidden=tuple(range(10)))
    with pkg.Context(0) as ctx:
        ctx.upload_splats(xyz, a["scale"], a["rot"], a["opacity"], a["f_dc"], labels=labels)
        ctx.upload_sh(a["f_rest"], 3)
        ctx.render_view(cams[0], W, H, to_host=False)
        ctx.render_views(cams * 2, W, H, to_host=False)

        def views_per_s():
            ctx.render_views(cams * 6, W, H, to_host=False)   # warm-up of the same shape
            t0 = time.perf_counter()
            for _ in range(2):
                ctx.render_views(cams * 6, W, H, to_host=False)
            return 48 / (time.perf_counter() - t0)

        plain, edited, set_ms = [], [], []
        for _ in range(args.rounds):                          # interleaved: drift hits both forms alike
            ctx.clear_render_edits()
            plain.append(views_per_s())
            t0 = time.perf_counter()
            ctx.set_render_edits(**state)
            set_ms.append((time.perf_counter() - t0) * 1e3)
            edited.append(views_per_s())
        ctx.clear_render_edits()
        ctx.render_view(cams[0], W, H, to_host=False)
        pairs_plain = ctx.render_num_pairs()
        ctx.set_render_edits(hidden=state["hidden"])
        hidden_splats = ctx.render_num_hidden()
        ctx.render_view(cams[0], W, H, to_host=False)
        pairs_hidden = ctx.render_num_pairs()
        ctx.profile(True)
        for _ in range(5):
            ctx.set_render_edits(**state)
        cnt, ms = ctx.profile_get("render_edit_code")
        ctx.render_view(cams[0], W, H, to_host=False)
        pairs_state = ctx.render_num_pairs()
        pre_cnt, pre_ms = ctx.profile_get("render_pre")
        ctx.profile(False)
    r2 = lambda v: [round(float(x), 1) for x in v]
    print(json.dumps({"splats": n, "width": W, "height": H, "sh_degree": 3, "views_per_s_no_edits": r2(plain),
                      "views_per_s_edits": r2(edited), "median_no_edits": round(float(np.median(plain)), 1),
                      "median_edits": round(float(np.median(edited)), 1), "set_edits_wall_ms": r2(set_ms),
                      "edit_code_kernel_ms": round(ms / max(cnt, 1), 4), "pre_kernel_edit_ms_one_frame": round(pre_ms / max(pre_cnt, 1), 4),
                      "hidden_splats": int(hidden_splats), "pairs_one_view_no_edits": int(pairs_plain),
                      "pairs_one_view_10_classes_hidden": int(pairs_hidden), "pairs_one_view_full_state": int(pairs_state)}))


if __name__ == "__main__":
    main()
