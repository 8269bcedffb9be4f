"""GPU: the front-end (deep_learning_segmentation.py) with stub networks: the class map goes from the network's output to the
vote on the device, the labels and the saved <image>_segmap.npy are the numpy model's, and no map goes through the host packer."""
import importlib
import os
import types

import numpy as np
import pytest

import segmap_model as M
from conftest import golden_assign_cases
from segmap_cases import seeded_logits, seeded_masks

pytestmark = pytest.mark.gpu


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


class StubSegformer:
    """returns the next seeded logits volume, on the device the inputs were moved to"""

    def __init__(self, vols):
        self.vols, self.calls = list(vols), 0

    def __call__(self, pixel_values=None):
        import torch
        assert pixel_values.is_cuda
        vol = self.vols[self.calls]
        self.calls += 1
        return types.SimpleNamespace(logits=torch.from_numpy(vol)[None].to(pixel_values.device))


class StubYolo:
    """returns the next seeded instances as an Ultralytics result: masks.data, boxes.cls, boxes.conf on the device"""

    def __init__(self, items, sizes):
        self.items, self.sizes, self.calls = list(items), list(sizes), 0

    def __call__(self, image, verbose=False):
        import torch
        item, (W, H) = self.items[self.calls], self.sizes[self.calls]
        assert image.size == (W, H)
        self.calls += 1
        if item is None:
            return [types.SimpleNamespace(orig_shape=(H, W), masks=None, boxes=None)]
        m, cls, conf = (torch.from_numpy(a).cuda() for a in item)
        return [types.SimpleNamespace(orig_shape=(H, W), masks=types.SimpleNamespace(data=m), boxes=types.SimpleNamespace(cls=cls, conf=conf))]


def run_front_end(ctx, gsx, monkeypatch, tmp_path, scene, model_type, model, want_maps, kernel):
    positions, cams, sizes = scene
    dls = importlib.import_module("deep_learning_segmentation")
    monkeypatch.setattr(dls, "initialize_model", lambda mt, device: (StubProcessor(), model))
    input_dir, output_dir = write_pngs(tmp_path, cams, sizes), str(tmp_path / "out")
    n_classes = dls.N_CLASSES[model_type]
    want = gsx.assign_labels_from_maps(positions, cams, want_maps, sizes, n_classes=n_classes, ctx=ctx)
    ctx.profile(True)
    got = dls.assign_labels(positions, cams, input_dir, output_dir, model_type=model_type, ctx=ctx)
    assert model.calls == 3
    assert got.dtype == np.int32 and np.array_equal(got, want)
    for cam, m in zip(cams, want_maps):
        saved = np.load(os.path.join(output_dir, cam["img_name"] + "_segmap.npy"))
        assert saved.dtype == np.int32 and np.array_equal(saved, m)
    # one launch of the producer per view, and nothing through the host packer: no byte of a host map crossed the link, no
    # kernel rebuilt a map from host records
    assert ctx.profile_get(kernel)[0] == 3 and ctx.profile_get("segmap_resize")[0] == 3
    assert ctx.vote_link_bytes() == 0 and ctx.profile_get("seg_expand")[0] == 0
    ctx.profile(False)
    return dls, input_dir, output_dir


def test_segformer_front_end(ctx, gsx, monkeypatch, tmp_path, scene):
    positions, cams, sizes = scene
    rng = np.random.default_rng(7)
    vols = [seeded_logits(rng, (150, 9, 11), ties=False), seeded_logits(rng, (150, 9, 11)), seeded_logits(rng, (150, 2, 3), ties=False)]
    maps = [M.segmap_from_logits(v, W, H) for v, (W, H) in zip(vols, sizes)]
    dls, input_dir, output_dir = run_front_end(ctx, gsx, monkeypatch, tmp_path, scene, "segformer", StubSegformer(vols), maps, "segmap_argmax")
    # the public function: the reference's signature, the numpy map, the .npy
    import torch
    model = StubSegformer(vols[1:2])
    path = os.path.join(input_dir, cams[1]["img_name"] + ".png")
    out2 = str(tmp_path / "out2")
    seg = dls.segment_image(path, out2, StubProcessor(), model, torch.device("cuda"), "segformer", ctx=ctx)
    assert isinstance(seg, np.ndarray) and seg.dtype == np.int32 and np.array_equal(seg, maps[1])
    assert np.array_equal(np.load(os.path.join(out2, cams[1]["img_name"] + "_segmap.npy")), maps[1])


def test_yolo_front_end(ctx, gsx, monkeypatch, tmp_path, scene):
    positions, cams, sizes = scene
    rng = np.random.default_rng(9)
    items = [seeded_masks(rng, 12, 9, 16, density=0.3), seeded_masks(rng, 37, 6, 10, density=0.1), seeded_masks(rng, 3, 2, 3, density=0.6)]
    maps = [M.segmap_from_masks(m, c, p, W, H) for (m, c, p), (W, H) in zip(items, sizes)]
    assert all((m >= 0).any() and (m == -1).any() for m in maps[:2])
    run_front_end(ctx, gsx, monkeypatch, tmp_path, scene, "yolo", StubYolo(items, sizes), maps, "segmap_masks")


def test_yolo_front_end_without_detections(ctx, gsx, monkeypatch, tmp_path, scene):
    positions, cams, sizes = scene
    rng = np.random.default_rng(13)
    items = [None, seeded_masks(rng, 5, 4, 4, density=0.5), None]
    maps = [np.full((H, W), -1, np.int32) if it is None else M.segmap_from_masks(*it, W, H) for it, (W, H) in zip(items, sizes)]
    run_front_end(ctx, gsx, monkeypatch, tmp_path, scene, "yolo", StubYolo(items, sizes), maps, "segmap_masks")
