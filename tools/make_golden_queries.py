#!/usr/bin/env python3
"""Generate the Mask2Former query golden vectors (tests/golden/segmap_queries.npz).

Runs ONLY in the build container, where /root/reference exists.  Like tools/make_golden_segmap.py it imports the reference's
own deep_learning_segmentation.py with inert stand-ins, then drives the Mask2Former branch of the reference's segment_image
with
  - a stub model that returns seeded class_queries_logits / masks_queries_logits (torch CPU tensors), and
  - the real Mask2FormerImageProcessor() of the installed transformers (without torchvision it is the PIL-backed class; it is
    constructed from its defaults, nothing is downloaded),
on tiny PNGs written with PIL.  Per case it records the inputs, the slot order torch's own softmax / top-k produced (the same
calls post_process_instance_segmentation makes, sorted=False), the target size, the map and segments_info.  Every case must
hold no knife-edge slot and at most 1e-3 knife-edge pixels (tests/queries_model.py), on the reference alone; the numpy model
must then equal the reference off the knife-edge pixels.  No reference source travels.
Usage:  python tools/make_golden_queries.py
"""
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import queries_model as QM  # noqa: E402
from make_golden_segmap import import_reference  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "segmap_queries.npz")
MID = (384, 384)


class _Model:
    def __init__(self):
        self.cls = self.masks = None

    def __call__(self, **inputs):
        assert "pixel_values" in inputs
        return types.SimpleNamespace(class_queries_logits=torch.from_numpy(self.cls)[None], masks_queries_logits=torch.from_numpy(self.masks)[None])


def torch_slots(cls):
    """the selection of post_process_instance_segmentation, call for call"""
    mask_cls = torch.from_numpy(cls)
    num_classes = mask_cls.shape[-1] - 1
    scores = torch.nn.functional.softmax(mask_cls, dim=-1)[:, :-1]
    s, idx = scores.flatten(0, 1).topk(mask_cls.shape[0], sorted=False)
    q = torch.div(idx, num_classes, rounding_mode="floor")
    return q.numpy().astype(np.int32), s.numpy().astype(np.float32), (idx % num_classes).numpy().astype(np.int32)


def seeded(rng, Q, C, h, w, dup=2):
    """class logits with one clear class per query (and `dup` queries with two), smooth-ish mask logits of mixed sign"""
    cls = rng.standard_normal((Q, C + 1)).astype(np.float32)
    for q in range(Q):
        cls[q, rng.integers(C)] += rng.uniform(2.0, 7.0)
    for q in rng.choice(Q, size=min(dup, Q), replace=False):
        a, b = rng.choice(C, size=2, replace=False)
        cls[q, a] = cls[q, b] = 9.0
    coarse = rng.standard_normal((Q, (h + 2) // 3 + 1, (w + 2) // 3 + 1)).astype(np.float32)
    masks = np.repeat(np.repeat(coarse, 3, axis=1), 3, axis=2)[:, :h, :w] * 6 + rng.standard_normal((Q, h, w)).astype(np.float32) * 2
    masks += rng.uniform(-6, 3, (Q, 1, 1)).astype(np.float32)
    return cls, np.ascontiguousarray(masks, np.float32)


def main():
    from transformers import Mask2FormerImageProcessor
    dls = import_reference()
    proc, model = Mask2FormerImageProcessor(), _Model()
    print("processor:", type(proc).__name__)
    tmp = tempfile.mkdtemp(prefix="queries_golden_")
    flat, names = {}, []

    def case(name, seed, Q, C, h, w, size):
        assert Q <= 20 and C <= 8 and h <= 24 and w <= 24 and size[0] <= 64 and size[1] <= 48
        rng = np.random.default_rng(seed)
        cls, masks = seeded(rng, Q, C, h, w)
        path = os.path.join(tmp, name + ".png")
        Image.fromarray(rng.integers(0, 255, (size[1], size[0], 3), dtype=np.uint8)).save(path)
        model.cls, model.masks = cls, masks
        got = dls.segment_image(path, os.path.join(tmp, "out"), proc, model, torch.device("cpu"), "mask2former")
        assert got.dtype == np.int32 and got.shape == (size[1], size[0])
        assert np.array_equal(np.load(os.path.join(tmp, "out", name + "_segmap.npy")), got)
        # segments_info is not returned by segment_image: the same processor call, made again on the same outputs
        info = proc.post_process_instance_segmentation(model(pixel_values=None), target_sizes=[(size[1], size[0])])[0]
        assert np.array_equal(info["segmentation"].numpy().astype(np.int32), got)
        ids = np.array([s["label_id"] for s in info["segments_info"]], np.int32)
        scores = np.array([s["score"] for s in info["segments_info"]], np.float64)
        sq, ss, sl = torch_slots(cls)
        res = QM.segmap_from_queries(masks, sq, ss, size, sl, MID)
        knife = QM.knife_pixels(res, masks, sq, size)
        assert not QM.knife_slots(res, sq, Q).any(), name
        assert knife.mean() <= 1e-3, (name, knife.mean())
        diff = res["map"] != got
        assert not (diff & ~knife).any(), (name, int(diff.sum()))
        acc = res["slot_segment"] >= 0
        assert int(acc.sum()) == len(ids) == got.max() + 1 and np.array_equal(sl[acc], ids), name
        assert np.abs(res["slot_pred"][acc] - scores).max(initial=0) <= 1e-5, name
        names.append(name)
        P = f"{name}/"
        flat[P + "class_logits"], flat[P + "masks"] = cls, masks
        flat[P + "slot_query"], flat[P + "slot_score"], flat[P + "slot_label"] = sq, ss, sl
        flat[P + "size"], flat[P + "map"] = np.array(size, np.int64), got
        flat[P + "label_ids"], flat[P + "scores"] = ids, scores
        print(name, masks.shape, "->", got.shape, "accepted", len(ids), "of", Q, "duplicated queries", Q - len(set(sq.tolist())),
              "differing pixels", int(diff.sum()), "knife share", float(knife.mean()))

    case("q20_c8_16x16", 101, 20, 8, 16, 16, (64, 48))
    case("q12_c5_24x9", 102, 12, 5, 24, 9, (37, 48))
    case("q7_c3_5x24", 103, 7, 3, 5, 24, (64, 11))
    case("q16_c8_1x13", 104, 16, 8, 1, 13, (50, 33))
    case("q9_c2_12x12", 105, 9, 2, 12, 12, (3, 5))
    case("q20_c4_7x7", 106, 20, 4, 7, 7, (1, 1))
    shutil.rmtree(tmp, ignore_errors=True)
    flat["cases"], flat["mid"] = np.array(names), np.array(MID, np.int64)
    np.savez_compressed(OUT, **flat)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
