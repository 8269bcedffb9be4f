"""The front-end (deep_learning_segmentation.py) with --depth_maps_dir and --depth_quantile.

CPU: the flags parse, their defaults, and what they refuse (a quantile without a directory, a quantile outside (0, 1], more
than one rank) - all before anything is loaded.

GPU (marked): on the edge scene edges_47x41 written as a PLY, with two cameras that have an image and a class map at half the
cameras' size and a third that has neither: the files written are <img_name>_depth.npy and <img_name>_surface.npy of the two
views; _surface.npy is Context.depth_view's surface_index at the map's size; _depth.npy equals, bit for bit, the float32 of
surface_z recomputed from _surface.npy, the splats' depth keys in the view (gsx_debug_render_pre) and gsx_depth_key_to_z; the
labelled PLY does not change with the flag."""
import importlib
import json
import os

import numpy as np
import pytest

import blend_cases

C = 5


def dls():
    return importlib.import_module("deep_learning_segmentation")


def test_flags_parse():
    p = dls().make_parser()
    a = p.parse_args([])
    assert a.depth_maps_dir is None and a.depth_quantile is None
    a = p.parse_args(["--depth_maps_dir", "d", "--depth_quantile", "0.25"])
    assert a.depth_maps_dir == "d" and a.depth_quantile == 0.25
    assert p.parse_args(["--depth_maps_dir", "d"]).depth_quantile is None
    assert "--depth_maps_dir DIR" in dls().__doc__ and "_depth.npy" in dls().__doc__ and "_surface.npy" in dls().__doc__


@pytest.mark.parametrize("argv, message", [
    (["--depth_quantile", "0.5"], "--depth_quantile needs --depth_maps_dir"),
    (["--depth_maps_dir", "d", "--depth_quantile", "0"], "must be in"),
    (["--depth_maps_dir", "d", "--depth_quantile", "1.5"], "must be in"),
    (["--depth_maps_dir", "d", "--depth_quantile", "nan"], "must be in"),
])
def test_flags_are_checked_before_anything_is_loaded(argv, message, capsys):
    with pytest.raises(SystemExit):
        dls().main(["--ply_file", "/nonexistent.ply", "--camera_file", "/nonexistent.json", *argv])
    assert message in capsys.readouterr().err


def test_one_gpu_only(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="--depth_maps_dir runs on one GPU"):
        dls().main(["--ply_file", "/nonexistent.ply", "--camera_file", "/nonexistent.json", "--depth_maps_dir", "d"])


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    from PIL import Image
    ply_io = importlib.import_module("3d_gaussian_splatting_project_amd.ply_io")
    d = tmp_path_factory.mktemp("depth_front_end")
    sc = blend_cases.prepared("edges_47x41").scene
    W, H = sc.W, sc.H
    xyz, scale, rot, opacity, f_dc = sc.arrays()
    cols = {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "nx": np.zeros(len(xyz), np.float32)}
    cols.update({f"f_dc_{k}": f_dc[:, k] for k in range(3)})
    cols["opacity"] = opacity
    cols.update({f"scale_{k}": scale[:, k] for k in range(3)})
    cols.update({f"rot_{k}": rot[:, k] for k in range(4)})
    ply = str(d / "scene.ply")
    ply_io.write_vertex_ply(ply, cols)
    cams = [dict(sc.cam, id=k, img_name=f"view_{k}", position=pos) for k, pos in enumerate(([0.0, 0.0, 0.0], [0.2, -0.1, 0.3], [0.0, 0.1, 0.0]))]
    cam_file = str(d / "cameras.json")
    with open(cam_file, "w") as f:
        json.dump(cams, f)
    (d / "images").mkdir()
    (d / "maps").mkdir()
    rng = np.random.default_rng(20292)
    size = (W // 2, H // 2)
    for cam in cams[:2]:
        Image.fromarray(rng.integers(0, 255, (H, W, 3), dtype=np.uint8)).save(str(d / "images" / (cam["img_name"] + ".png")))
        r, x = np.mgrid[0:size[1], 0:size[0]]
        np.save(str(d / "maps" / (cam["img_name"] + "_segmap.npy")), ((r // 5 + x // 7) % (C + 1) - 1).astype(np.int32))
    return dict(dir=d, ply=ply, cam_file=cam_file, cams=cams, arrays=sc.arrays(), size=size)


def run_cli(job, out, *extra):
    path = str(job["dir"] / out)
    dls().main(["--ply_file", job["ply"], "--camera_file", job["cam_file"], "--input_dir", str(job["dir"] / "images"), "--output_dir",
                str(job["dir"] / "out"), "--output_file", path, "--segmap_dir", str(job["dir"] / "maps"), "--n_classes", str(C), *extra])
    return path


@pytest.mark.gpu
@pytest.mark.parametrize("quantile", (None, 0.2))
def test_depth_maps_dir_writes_what_the_context_gives(gsx, job, quantile):
    out = job["dir"] / f"depth_{quantile}"
    flags = ["--depth_maps_dir", str(out)] + ([] if quantile is None else ["--depth_quantile", str(quantile)])
    with_flag = run_cli(job, f"with_{quantile}.ply", *flags)
    assert sorted(os.listdir(out)) == ["view_0_depth.npy", "view_0_surface.npy", "view_1_depth.npy", "view_1_surface.npy"]
    w, h = job["size"]
    q = 0.5 if quantile is None else quantile
    with gsx.Context(0) as c:
        c.upload_splats(*job["arrays"])
        order = c.render_debug()[1].astype(np.int64)
        for k, cam in enumerate(job["cams"][:2]):
            depth, surface = np.load(str(out / f"view_{k}_depth.npy")), np.load(str(out / f"view_{k}_surface.npy"))
            assert depth.dtype == np.float32 and surface.dtype == np.int32 and depth.shape == surface.shape == (h, w)
            frame = c.depth_view(cam, w, h, q)
            assert np.array_equal(surface, frame.surface_index) and (surface >= 0).sum() > 10 and (surface < 0).sum() > 10
            # surface_z from the rows and the keys: fx, fy scaled to the map's size, as the front-end scales them
            half = dict(cam, fx=cam["fx"] * (w / cam["width"]), fy=cam["fy"] * (h / cam["height"]), width=w, height=h)
            key = np.zeros(len(order), np.int64)
            key[order] = c.debug_render_pre([half], w, h)[0]["depth"]
            scale, offset = gsx.depth_key_to_z(half, w, h)
            z = np.where(surface >= 0, key[np.maximum(surface, 0)].astype(np.float64) * scale + offset, np.nan)
            assert np.array_equal(depth, z.astype(np.float32), equal_nan=True), k
            assert np.array_equal(np.isnan(depth), surface < 0)
        frames = gsx.depth_maps(job["arrays"], job["cams"][:2], [job["size"]] * 2, q, ctx=c)
        assert np.array_equal(frames[1].surface_index, surface) and np.array_equal(frames[1].surface_z.astype(np.float32), depth, equal_nan=True)
    plain = run_cli(job, f"plain_{quantile}.ply")
    assert open(plain, "rb").read() == open(with_flag, "rb").read()
