"""GPU: the front-end (deep_learning_segmentation.py) with --associate on the value scene of tests/assoc_cases.py: the labelled
PLY holds what assign_instances_from_maps gives, the side files stay raw maps, and several ranks are refused."""
import importlib
import json

import numpy as np
import pytest

import assoc_cases as ac
import assoc_model as am

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    from PIL import Image
    ply_io = importlib.import_module("3d_gaussian_splatting_project_amd.ply_io")
    d = tmp_path_factory.mktemp("assoc_front_end")
    pos, blob, cams, maps, sizes = ac.value_scene()
    ply = str(d / "scene.ply")
    rng = np.random.default_rng(6106)
    n = len(pos)
    cols = {"x": pos[:, 0], "y": pos[:, 1], "z": pos[:, 2]}                # ... and splat attributes, for --labeler lift
    cols.update({f"f_dc_{k}": rng.normal(size=n).astype(np.float32) for k in range(3)})
    cols["opacity"] = np.full(n, 2.0, np.float32)
    cols.update({f"scale_{k}": np.full(n, np.log(0.05), np.float32) for k in range(3)})
    cols.update({f"rot_{k}": np.full(n, 1.0 if k == 0 else 0.0, np.float32) for k in range(4)})
    ply_io.write_vertex_ply(ply, cols)
    cam_file = str(d / "cameras.json")
    with open(cam_file, "w") as f:
        json.dump(cams, f)
    (d / "images").mkdir()
    (d / "maps").mkdir()
    for cam, seg in zip(cams, maps):
        Image.fromarray(np.zeros((ac.H, ac.W, 3), np.uint8)).save(str(d / "images" / (cam["img_name"] + ".png")))
        np.save(str(d / "maps" / (cam["img_name"] + "_segmap.npy")), seg)
    return dict(dir=d, ply=ply, cam_file=cam_file, pos=pos, blob=blob, cams=cams, maps=maps, sizes=sizes)


def run_cli(job, out, *extra):
    dls = importlib.import_module("deep_learning_segmentation")
    path = str(job["dir"] / out)
    dls.main(["--ply_file", job["ply"], "--camera_file", job["cam_file"], "--input_dir", str(job["dir"] / "images"), "--output_dir",
              str(job["dir"] / "out"), "--output_file", path, "--segmap_dir", str(job["dir"] / "maps"), *extra])
    return path


def labels_of(path):
    ply_io = importlib.import_module("3d_gaussian_splatting_project_amd.ply_io")
    data = ply_io.PlyData.read(path)
    assert data["vertex"].properties[-1] == "label"
    return np.array(data["vertex"]["label"])


def test_associate_writes_what_the_labeler_gives(gsx, job, capsys):
    want, n_instances = gsx.assign_instances_from_maps(job["pos"], job["cams"], job["maps"], job["sizes"])
    assert n_instances == ac.K and am.same_partition(want, job["blob"])
    got = labels_of(run_cli(job, "assoc.ply", "--associate"))
    assert f"Association: {ac.K} instances found, 0 segments dropped" in capsys.readouterr().out
    assert got.dtype == np.int32 and np.array_equal(got, want)
    for cam, seg in zip(job["cams"], job["maps"]):                       # the side files are still the raw maps
        assert np.array_equal(np.load(str(job["dir"] / "maps" / (cam["img_name"] + "_segmap.npy"))), seg)
    # the parameters reach the run: with room for three instances only, the other blobs' segments are dropped
    few, n_few = gsx.assign_instances_from_maps(job["pos"], job["cams"], job["maps"], job["sizes"], max_instances=3)
    assert n_few == 3 and (few == -1).any()
    assert np.array_equal(labels_of(run_cli(job, "few.ply", "--associate", "--assoc_max_instances", "3")), few)
    assert "3 instances found" in capsys.readouterr().out
    # without the flag the ids are voted as they are and mix the blobs
    assert not am.same_partition(labels_of(run_cli(job, "raw.ply", "--n_classes", "254")), job["blob"])


def test_associate_in_front_of_the_lift(gsx, job):
    dls = importlib.import_module("deep_learning_segmentation")
    gaussians, plydata = dls.load_gaussians(job["ply"])
    with gsx.Context(0) as c:
        c.upload_splats(*dls.load_splat_attributes(plydata))
        c.upload_positions(gaussians)
        c.assoc_begin(254, 255, 0.3, 1)
        c.lift_begin(255)
        for cam, seg, size in zip(job["cams"], job["maps"], job["sizes"]):
            c.lift_view(cam, c.assoc_view(cam, seg, size)[1])
        want = c.lift_finalize(0.0)
        assert c.assoc_num_instances() == ac.K
    got = labels_of(run_cli(job, "assoc_lift.ply", "--associate", "--labeler", "lift"))
    assert np.array_equal(got, want) and (want >= 0).sum() > len(want) // 2


def test_associate_refuses_several_ranks(job, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="--associate runs on one GPU"):
        run_cli(job, "never.ply", "--associate")
