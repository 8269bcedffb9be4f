#!/usr/bin/env python3
"""Generate the IoU-evaluation golden vectors (tests/golden/iou.npz).

Runs ONLY in the build container, where /root/reference exists.  It imports the reference's own
Image_Segmentation/evaluation.py with `transformers`, `requests` and `PIL` replaced by inert modules (the module imports
them at the top and uses them only under __main__), calls its three functions - IoU, get_ious_from_masks,
generate_segmentation_map - on private copies of the inputs (IoU writes 1 into the set pixels of its arguments) and
records inputs and results.  The labelme ground truth the reference ships (Image_Segmentation/labels/*/label.png) is
stored as uint8 label maps: data, read here with the real PIL.  No reference source travels.
Usage:  python tools/make_golden_iou.py
"""
import importlib.util
import os
import random
import sys
import types
import warnings

import numpy as np

REF_DIR = "/root/reference/Image_Segmentation"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "iou.npz")
LABELME = ("0001_2", "0001_3", "DSCF4667", "street")


def read_label_png(name):
    from PIL import Image   # the real one, before the inert stand-in goes in
    a = np.array(Image.open(os.path.join(REF_DIR, "labels", name, "label.png")))
    assert a.ndim == 2 and a.max() <= 255
    return a.astype(np.uint8)


def import_reference():
    saved = {k: sys.modules.get(k) for k in ("transformers", "requests", "PIL", "PIL.Image")}
    t = types.ModuleType("transformers")
    t.pipeline = None
    pil = types.ModuleType("PIL")
    pil.Image = types.ModuleType("PIL.Image")
    sys.modules.update({"transformers": t, "requests": types.ModuleType("requests"), "PIL": pil, "PIL.Image": pil.Image})
    try:
        spec = importlib.util.spec_from_file_location("ref_evaluation", os.path.join(REF_DIR, "evaluation.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def copies(arrs):
    return [np.array(a) for a in arrs]


def main():
    labelme = {n: read_label_png(n) for n in LABELME}
    ev = import_reference()
    rng = np.random.default_rng(20250218)
    flat = {}
    names = []

    def mask_case(name, masks, gts):
        """all pairs through IoU, the list through get_ious_from_masks; every call on fresh copies"""
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")   # 0 / 0: the reference warns and returns nan
            iou = np.array([[ev.IoU(np.array(m), np.array(g)) for g in gts] for m in masks], np.float64)
            best = ev.get_ious_from_masks(copies(masks), copies(gts))
        names.append(name)
        flat[f"{name}/n_masks"], flat[f"{name}/n_gt"] = np.int64(len(masks)), np.int64(len(gts))
        for i, m in enumerate(masks):
            flat[f"{name}/mask{i}"] = m
        for i, g in enumerate(gts):
            flat[f"{name}/gt{i}"] = g
        flat[f"{name}/iou"] = iou
        flat[f"{name}/best_iou"] = np.array([float(b[0]) for b in best], np.float64)
        flat[f"{name}/best_gt"] = np.array([int(b[1]) for b in best], np.int64)
        print(name, "iou", iou.ravel()[:6], "best", best[:3])

    # the reference's own example; IoU edits its arguments in place: keep what they look like afterwards
    a, b = np.array(ev.img1), np.array(ev.img2)
    mask_case("example", [np.array(ev.img1)], [np.array(ev.img2)])
    v = ev.IoU(a, b)
    assert v == 4 / 14
    flat["example/after1"], flat["example/after2"] = a, b

    f = np.zeros((5, 7), np.float32)
    f[0, :] = [np.nan, -0.0, np.inf, 1e-45, -1.5, 0.0, 2.0]
    f[2, 1:4] = [-np.inf, -1e-45, 0.25]
    g = np.zeros((5, 7), np.float32)
    g[0, :] = [1.0, 1.0, -np.inf, np.nan, 0.0, -0.0, -1e-45]
    g[2, :] = 3.0
    mask_case("float_edges", [f, f.astype(np.float64), np.zeros((5, 7), np.float32)], [g, g.astype(np.float64)])

    i32 = np.zeros((6, 5), np.int32)
    i32[1, 1], i32[2, 3], i32[5, 4] = 256, -1, 65536
    j32 = np.zeros((6, 5), np.int32)
    j32[1, 1], j32[5, 4], j32[0, 0] = 1, -256, 7
    mask_case("int32_256", [i32], [j32])
    i64 = np.zeros((6, 5), np.int64)
    i64[1, 1], i64[2, 3], i64[4, 0] = 2 ** 32, -2 ** 40, 1
    j64 = np.zeros((6, 5), np.int64)
    j64[1, 1], j64[4, 0], j64[3, 3] = 2 ** 32, 2 ** 33, 5
    mask_case("int64_2p32", [i64], [j64])

    z = np.zeros((4, 4), np.int64)
    mask_case("empty", [z], [z.copy(), z.copy()])
    m = (rng.random((9, 11)) < 0.4).astype(np.uint8)
    g0 = (rng.random((9, 11)) < 0.4).astype(np.uint8)
    mask_case("ties", [m], [g0, g0.copy(), m.copy(), m.copy()])     # two identical ground truths twice: the first wins
    mask_case("equal", [m], [m.copy()])
    mask_case("random_5x4", [(rng.random((37, 53)) < d).astype(np.uint8) * rng.integers(1, 255, (37, 53), dtype=np.uint8)
                             for d in (0.1, 0.3, 0.5, 0.7, 0.0)],
              [(rng.random((37, 53)) < d).astype(np.uint8) for d in (0.5, 0.05, 0.9, 0.3)])

    # generate_segmentation_map: overlapping masks, the last one that covers a pixel owns it
    sm = [np.zeros((12, 15), np.uint8) for _ in range(4)]
    sm[0][1:8, 1:9] = 1
    sm[1][4:11, 5:14] = 200
    sm[2][0:3, 0:15] = 1
    sm[3][6:7, 0:15] = 9
    random.seed(7)
    seg = ev.generate_segmentation_map(copies(sm))
    for i, x in enumerate(sm):
        flat[f"segmap/mask{i}"] = x
    flat["segmap/n_masks"], flat["segmap/seed"], flat["segmap/map"] = np.int64(len(sm)), np.int64(7), seg

    # the labelme ground truth, as label maps
    for n, a in labelme.items():
        flat[f"labelme/{n}"] = a
        print("labelme", n, a.shape, "labels", np.unique(a).tolist())
    a, b = labelme["0001_2"], labelme["0001_3"]
    ka, kb = int(a.max()) + 1, int(b.max()) + 1
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        flat["labelme/0001_2_vs_0001_3/iou"] = np.array([[ev.IoU(a == i, b == j) for j in range(kb)] for i in range(ka)], np.float64)
        bm = ev.get_ious_from_masks([a == i for i in range(ka)], [b == j for j in range(kb)])
        flat["labelme/0001_2_vs_0001_3/best_iou"] = np.array([float(x[0]) for x in bm], np.float64)
        flat["labelme/0001_2_vs_0001_3/best_gt"] = np.array([int(x[1]) for x in bm], np.int64)
        for n in ("DSCF4667", "street"):
            a = labelme[n]
            b = np.roll(a, 3, axis=1)          # the same map shifted by 3 pixels
            k = int(a.max()) + 1
            flat[f"labelme/{n}_shift3/iou"] = np.array([[ev.IoU(a == i, b == j) for j in range(k)] for i in range(k)], np.float64)
    flat["cases"] = np.array(names)
    np.savez_compressed(OUT, **flat)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
