#!/usr/bin/env python3
"""Generate the class-map golden vectors (tests/golden/segmap.npz).

Runs ONLY in the build container, where /root/reference exists.  It imports the reference's own
deep_learning_segmentation.py with `plyfile`, `ultralytics` and `transformers` replaced by inert modules (the module imports
them at the top and uses them only in load_gaussians / initialize_model), its `plt` replaced by no-ops (the comparison PNG is
out of scope) and a stand-in `cv2` whose `resize` is the numpy model of OpenCV's nearest rule (tests/segmap_model.py): cv2 is
not installed here, so that one rule is restated from OpenCV's source and cannot be executed against.  Then it drives
  - the reference's process_yolo_segmentation with stub result objects (torch CPU tensors), and
  - the SegFormer branch of the reference's segment_image with a stub processor and a stub model that returns seeded logits,
    on tiny PNGs written with PIL,
and records inputs and outputs.  No reference source travels.
Usage:  python tools/make_golden_segmap.py
"""
import importlib.util
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import segmap_model as M  # noqa: E402

REF = "/root/reference/deep_learning_segmentation.py"
OUT = os.path.join(HERE, "..", "tests", "golden", "segmap.npz")


class _Nothing:
    """matplotlib.pyplot that draws nothing"""

    def __getattr__(self, name):
        return lambda *a, **k: None


def import_reference():
    names = ("plyfile", "ultralytics", "transformers", "cv2")
    saved = {k: sys.modules.get(k) for k in names}
    ply = types.ModuleType("plyfile")
    ply.PlyData = ply.PlyElement = object
    ultra = types.ModuleType("ultralytics")
    ultra.YOLO = object
    tr = types.ModuleType("transformers")
    for a in ("AutoImageProcessor", "Mask2FormerForUniversalSegmentation", "SegformerImageProcessor", "SegformerForSemanticSegmentation"):
        setattr(tr, a, object)
    cv2 = types.ModuleType("cv2")
    cv2.INTER_NEAREST = 0

    def resize(src, dsize, interpolation=None):
        assert interpolation == cv2.INTER_NEAREST and np.asarray(src).ndim == 2
        return M.resize_nearest(np.asarray(src), int(dsize[0]), int(dsize[1]))

    cv2.resize = resize
    sys.modules.update({"plyfile": ply, "ultralytics": ultra, "transformers": tr, "cv2": cv2})
    try:
        spec = importlib.util.spec_from_file_location("ref_dls", REF)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    mod.plt = _Nothing()
    return mod


# ---- stub network outputs ------------------------------------------------------------------------------------------------------------
class _Box:
    def __init__(self, c, p):
        self.cls, self.conf = torch.tensor([c], dtype=torch.float32), torch.tensor([p], dtype=torch.float32)


class _Masks:
    def __init__(self, data):
        self.data = torch.from_numpy(np.ascontiguousarray(data))


class _Result:
    def __init__(self, masks, cls, conf, size):
        self.orig_shape = (size[1], size[0])
        self.masks = None if masks is None else _Masks(masks)
        self.boxes = None if masks is None else [_Box(float(c), float(p)) for c, p in zip(cls, conf)]


class _Yolo:
    def __init__(self, result):
        self.result = result

    def __call__(self, image, verbose=False):
        return [self.result]


class _Processor:
    def __call__(self, images=None, return_tensors=None):
        return {"pixel_values": torch.zeros(1, 3, 2, 2)}


class _Segformer:
    def __init__(self):
        self.next = None

    def __call__(self, pixel_values=None):
        return types.SimpleNamespace(logits=torch.from_numpy(self.next)[None])


def main():
    dls = import_reference()
    rng = np.random.default_rng(20251019)
    flat, lnames, mnames = {}, [], []
    up = np.nextafter(np.float32(0.5), np.float32(1))

    # ---- instances: process_yolo_segmentation ------------------------------------------------------------------------------------
    def mask_case(name, masks, cls, conf, size):
        masks = None if masks is None else np.asarray(masks, np.float32)
        cls, conf = np.asarray(cls, np.float32), np.asarray(conf, np.float32)
        got = dls.process_yolo_segmentation(_Yolo(_Result(masks, cls, conf, size)), None)
        assert got.dtype == np.int32 and got.shape == (size[1], size[0])
        assert np.array_equal(got, M.segmap_from_masks(masks, cls, conf, *size)), name
        mnames.append(name)
        flat[f"masks/{name}/masks"] = np.zeros((0, 1, 1), np.float32) if masks is None else masks
        flat[f"masks/{name}/cls"], flat[f"masks/{name}/conf"] = cls, conf
        flat[f"masks/{name}/size"], flat[f"masks/{name}/map"] = np.array(size, np.int64), got
        print("masks", name, got.shape, "labels", np.unique(got).tolist())

    def blobs(K, mh, mw, density=0.4):
        return (rng.random((K, mh, mw)) < density).astype(np.float32) * rng.uniform(0.51, 1.0, (K, mh, mw)).astype(np.float32)

    mask_case("k0", None, [], [], (9, 7))
    mask_case("overlaps", blobs(5, 8, 8), [3, 17, 3, 79, 0], [0.9, 0.8, 0.95, 0.6, 0.99], (21, 13))
    mask_case("conf_half", blobs(3, 6, 5, 0.6), [1, 2, 3], [0.9, 0.5, 0.9], (11, 12))
    mask_case("conf_half_up", blobs(3, 6, 5, 0.6), [1, 2, 3], [0.2, up, 0.1], (11, 12))
    m = np.zeros((2, 4, 4), np.float32)
    m[0], m[1, :2] = 0.9, 0.5
    m[1, 2] = up
    mask_case("mask_half", m, [4, 5], [0.9, 0.9], (8, 8))
    mask_case("all_rejected", blobs(4, 5, 5), [1, 2, 3, 4], [0.5, 0.1, np.nan, 0.49999997], (7, 7))
    full = np.ones((2, 3, 3), np.float32)
    mask_case("low_over_high", full, [10, 20], [0.99, 0.51], (5, 4))
    mask_case("nan_conf_between", blobs(3, 7, 7, 0.7), [6, 7, 8], [0.8, np.nan, 0.7], (10, 9))
    mask_case("fraction_class", blobs(3, 4, 6, 0.5), [2.9, 0.99, 41.5], [0.9, 0.9, 0.9], (9, 10))
    mask_case("rows2_to_98", blobs(3, 2, 3, 0.5), [1, 2, 3], [0.9, 0.9, 0.9], (7, 98))
    mask_case("down", blobs(4, 8, 8, 0.3), [9, 8, 7, 6], [0.9, 0.9, 0.6, 0.7], (3, 5))
    mask_case("k9", blobs(9, 8, 8, 0.15), np.arange(9) * 7, [0.9, 0.3, 0.8, 0.7, 0.5, 0.6, up, 0.2, 0.4], (19, 17))

    # ---- logits: the SegFormer branch of segment_image ------------------------------------------------------------------------------
    tmp = tempfile.mkdtemp(prefix="segmap_golden_")
    model, proc = _Segformer(), _Processor()

    def logits_case(name, logits, size):
        logits = np.ascontiguousarray(logits, np.float32)
        assert logits.ndim == 3 and logits.shape[0] <= 16 and logits.shape[1] <= 8 and logits.shape[2] <= 8
        path = os.path.join(tmp, name + ".png")
        Image.fromarray(rng.integers(0, 255, (size[1], size[0], 3), dtype=np.uint8)).save(path)
        model.next = logits
        got = dls.segment_image(path, os.path.join(tmp, "out"), proc, model, torch.device("cpu"), "segformer")
        saved = np.load(os.path.join(tmp, "out", name + "_segmap.npy"))
        assert got.shape == (size[1], size[0]) and np.array_equal(saved, got)
        assert np.array_equal(got, M.segmap_from_logits(logits, *size)), name
        lnames.append(name)
        flat[f"logits/{name}/logits"], flat[f"logits/{name}/size"] = logits, np.array(size, np.int64)
        flat[f"logits/{name}/map"] = got.astype(np.int32)
        print("logits", name, logits.shape, "->", got.shape, "labels", np.unique(got).tolist())

    logits_case("c16_8x8", rng.standard_normal((16, 8, 8)), (20, 13))
    logits_case("c1", rng.standard_normal((1, 3, 4)), (6, 5))
    logits_case("c3_rows2_to_98", rng.standard_normal((3, 2, 3)), (7, 98))
    logits_case("c3_cols2_to_98", rng.standard_normal((3, 3, 2)), (98, 7))
    logits_case("down", rng.standard_normal((7, 8, 8)), (3, 5))
    logits_case("same", rng.standard_normal((5, 8, 8)), (8, 8))
    logits_case("one_to_many", rng.standard_normal((4, 1, 1)), (4, 3))
    logits_case("many_to_one", rng.standard_normal((4, 8, 8)), (1, 1))
    sp = rng.integers(-2, 3, (9, 6, 7)).astype(np.float32)        # small integers: ties everywhere
    sp[:, 0, 0] = -np.inf                                         # all -inf -> 0
    sp[:, 0, 1] = [0.0, -0.0, 0.0, -0.0, -1, -1, -0.0, 0.0, -2]   # -0.0 == +0.0: the first wins
    sp[:, 0, 2] = [-0.0, 0.0, -3, -3, -3, -3, -3, -3, -3]
    sp[:, 0, 3] = [1, np.inf, np.nan, np.inf, np.nan, 2, 2, 2, 2]  # a NaN is the maximum, the first NaN wins
    sp[:, 0, 4] = [np.inf, 1, 1, 1, 1, 1, 1, 1, np.nan]           # ... also behind +inf
    sp[:, 0, 5] = np.nan
    sp[:, 1, 0] = [-np.inf] * 8 + [-3e38]
    sp[:, 1, 1] = [5, 5, 5, 5, 5, 5, 5, 5, 5]
    logits_case("special", sp, (9, 11))
    shutil.rmtree(tmp, ignore_errors=True)
    flat["cases_logits"], flat["cases_masks"] = np.array(lnames), np.array(mnames)
    np.savez_compressed(OUT, **flat)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
