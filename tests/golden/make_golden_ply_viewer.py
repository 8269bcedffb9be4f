#!/usr/bin/env python3
"""Generate tests/golden/ply_viewer.npz: a seeded 3DGS PLY (300 splats, SH degree 3) labelled by the package's own PLY
writer, run through the reference viewer's processPlyBuffer under node (tools/make_golden_js.js).

Stores the columns and labels that were written, the sha256 of the labelled file the reference parsed, and what the
reference's worker posted for it: the 32-byte splat rows and the RGBA32UI texture words (the label word among them).
tests/test_ply_and_frontends.py writes the same file again and checks it against these.
Build-container only (needs the reference and node).  Usage: python tests/golden/make_golden_ply_viewer.py
"""
import base64
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
from test_ply_and_frontends import make_3dgs_ply, pio, scene  # noqa: E402

N = 300


def main():
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "in.ply"), os.path.join(tmp, "labelled.ply")
        cols = make_3dgs_ply(src, n=N, sh_degree=3)
        labels = np.random.default_rng(1).integers(-1, 150, N).astype(np.int32)
        pio.PlyData.read(src).write(out, labels=labels)
        cams = scene.make_cameras(1, 320, 180, convention="c2w")
        cams[0]["render_width"], cams[0]["render_height"] = 320, 180
        cj, oj = os.path.join(tmp, "cams.json"), os.path.join(tmp, "out.json")
        json.dump(cams, open(cj, "w"))
        subprocess.check_call(["node", os.path.join(ROOT, "tools", "make_golden_js.js"), out, cj, oj])
        res = json.load(open(oj))
        sha = hashlib.sha256(open(out, "rb").read()).hexdigest()
    buf = np.frombuffer(base64.b64decode(res["buffer"]), np.uint8).reshape(N, 32)
    tex = np.frombuffer(base64.b64decode(res["texdata"]), np.uint32)[:N * 8].reshape(N, 8)
    np.savez_compressed(os.path.join(HERE, "ply_viewer.npz"), names=np.array(list(cols)), labels=labels, ply_sha256=np.array(sha),
                        vertex_count=np.int64(res["vertexCount"]), buffer=buf, texdata=tex,
                        **{"col_" + k: np.asarray(v, np.float32) for k, v in cols.items()})
    print(f"ply_viewer.npz: {N} splats, {len(cols)} columns, sha256 {sha[:16]}")


if __name__ == "__main__":
    main()
