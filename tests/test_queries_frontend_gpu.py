"""GPU: the front-end (deep_learning_segmentation.py) with a stub Mask2Former: the query outputs go from the network to the vote
on the device, the labels and the saved <image>_segmap.npy are the numpy model's (tests/queries_model.py), and no map goes
through the host packer.  No test needs transformers: the stub processor only hands out pixel values."""
import importlib
import os
import types

import numpy as np
import pytest

import queries_model as QM
from conftest import golden_assign_cases

pytestmark = pytest.mark.gpu

MID = (384, 384)
KERNELS = ("queries_sampled", "queries_mask", "queries_accept", "queries_compose", "segmap_resize")


@pytest.fixture(scope="module")
def scene():
    """three views of a golden scene whose maps have the image's size"""
    name, positions, cams, segs, sizes, _ = next(c for c in golden_assign_cases() if c[0].startswith("rand3"))
    assert len(cams) == 3
    return positions, cams, sizes


def write_pngs(tmp_path, cams, sizes):
    from PIL import Image
    rng = np.random.default_rng(1)
    d = tmp_path / "images"
    d.mkdir()
    for cam, (W, H) in zip(cams, sizes):
        Image.fromarray(rng.integers(0, 255, (H, W, 3), dtype=np.uint8)).save(str(d / (cam["img_name"] + ".png")))
    return str(d)


class StubProcessor:
    def __call__(self, images=None, return_tensors=None):
        import torch
        assert return_tensors == "pt" and images is not None
        return {"pixel_values": torch.zeros(1, 3, 4, 4)}

    def post_process_instance_segmentation(self, *a, **k):
        raise AssertionError("the front-end must not post-process in torch")


class StubMask2Former:
    """returns the next seeded query outputs, on the device the inputs were moved to"""

    def __init__(self, items):
        self.items, self.calls = list(items), 0

    def __call__(self, pixel_values=None):
        import torch
        assert pixel_values.is_cuda
        cls, masks = self.items[self.calls]
        self.calls += 1
        dev = pixel_values.device
        return types.SimpleNamespace(class_queries_logits=torch.from_numpy(cls)[None].to(dev), masks_queries_logits=torch.from_numpy(masks)[None].to(dev))


def seeded_outputs(rng, Q, C, h, w):
    """class logits with clear winners (and two queries with two), smooth mask logits of mixed sign"""
    cls = rng.standard_normal((Q, C + 1)).astype(np.float32)
    for q in range(Q):
        cls[q, rng.integers(C)] += rng.uniform(2.0, 7.0)
    for q in rng.choice(Q, size=2, replace=False):
        a, b = rng.choice(C, size=2, replace=False)
        cls[q, a] = cls[q, b] = 9.0
    coarse = rng.standard_normal((Q, (h + 3) // 4, (w + 3) // 4)).astype(np.float32)
    masks = np.repeat(np.repeat(coarse, 4, 1), 4, 2)[:, :h, :w] * 6 + rng.standard_normal((Q, h, w)).astype(np.float32) - 3
    return cls, np.ascontiguousarray(masks, np.float32)


def expected(dls, items, sizes, labels):
    """the model's maps, fed the slot order the front-end's own helper returns; its slot SET must be numpy's top-Q"""
    import torch
    maps = []
    for (cls, masks), size in zip(items, sizes):
        sq, ss, sl = (t.cpu().numpy() for t in dls.select_query_slots(torch.from_numpy(cls).cuda()))
        top, p = QM.select_slots(cls)
        flat = sq.astype(np.int64) * (cls.shape[1] - 1) + sl
        assert len(flat) == cls.shape[0] and set(int(i) for i in flat) == top and np.abs(p[flat] - ss).max() <= 1e-6
        assert len(set(sq.tolist())) < len(sq)                    # some query fills two slots
        res = QM.segmap_from_queries(masks, sq, ss, size, sl, MID, 0.5, labels)
        assert not QM.knife_slots(res, sq, len(masks)).any()
        acc = res["slot_segment"] >= 0
        assert acc.any() and not acc.all() and (res["map"] == -1).any()
        maps.append(res["map"])
    return maps


@pytest.mark.parametrize("mode", ["segments", "classes"])
def test_mask2former_front_end(ctx, gsx, monkeypatch, tmp_path, scene, mode):
    positions, cams, sizes = scene
    dls = importlib.import_module("deep_learning_segmentation")
    rng = np.random.default_rng(11)
    items = [seeded_outputs(rng, 20, 150, 12, 16), seeded_outputs(rng, 33, 150, 9, 7), seeded_outputs(rng, 8, 150, 24, 24)]
    maps = expected(dls, items, sizes, mode == "classes")
    model = StubMask2Former(items)
    monkeypatch.setattr(dls, "initialize_model", lambda mt, device: (StubProcessor(), model))
    input_dir, output_dir = write_pngs(tmp_path, cams, sizes), str(tmp_path / "out")
    want = gsx.assign_labels_from_maps(positions, cams, maps, sizes, n_classes=150, ctx=ctx)
    ctx.profile(True)
    got = dls.assign_labels(positions, cams, input_dir, output_dir, model_type="mask2former", ctx=ctx, mask2former_map=mode)
    assert model.calls == 3
    assert got.dtype == np.int32 and np.array_equal(got, want) and (got >= 0).any()
    for cam, m in zip(cams, maps):
        saved = np.load(os.path.join(output_dir, cam["img_name"] + "_segmap.npy"))
        assert saved.dtype == np.int32 and np.array_equal(saved, m)
    for name in KERNELS:                                           # one launch of each kernel per view
        assert ctx.profile_get(name)[0] == 3, name
    assert ctx.vote_link_bytes() == 0 and ctx.profile_get("seg_expand")[0] == 0
    ctx.profile(False)
    if mode == "classes":
        return
    # the class map is the label lookup of the segment map
    for (cls, masks), size, m in zip(items, sizes, maps):
        import torch
        sq, ss, sl = (t.cpu().numpy() for t in dls.select_query_slots(torch.from_numpy(cls).cuda()))
        res = QM.segmap_from_queries(masks, sq, ss, size, sl, MID)
        lut = np.concatenate([sl[res["slot_segment"] >= 0], [-1]]).astype(np.int32)
        assert np.array_equal(QM.segmap_from_queries(masks, sq, ss, size, sl, MID, 0.5, True)["map"], lut[m])
    # the public function: the reference's signature, the numpy map, the .npy
    import torch
    one = StubMask2Former(items[1:2])
    path = os.path.join(input_dir, cams[1]["img_name"] + ".png")
    out2 = str(tmp_path / "out2")
    seg = dls.segment_image(path, out2, StubProcessor(), one, torch.device("cuda"), "mask2former", ctx=ctx)
    assert isinstance(seg, np.ndarray) and seg.dtype == np.int32 and np.array_equal(seg, maps[1])
    assert np.array_equal(np.load(os.path.join(out2, cams[1]["img_name"] + "_segmap.npy")), maps[1])


def test_segment_ids_must_fit_the_vote(ctx, monkeypatch, tmp_path, scene):
    """segment mode: more queries than the vote has classes is an error, not a silent overflow"""
    positions, cams, sizes = scene
    dls = importlib.import_module("deep_learning_segmentation")
    rng = np.random.default_rng(13)
    model = StubMask2Former([seeded_outputs(rng, 12, 150, 6, 6)] * 3)
    monkeypatch.setattr(dls, "initialize_model", lambda mt, device: (StubProcessor(), model))
    input_dir = write_pngs(tmp_path, cams, sizes)
    with pytest.raises(ValueError):
        dls.assign_labels(positions, cams, input_dir, str(tmp_path / "out"), model_type="mask2former", ctx=ctx, n_classes=11)
