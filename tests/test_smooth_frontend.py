"""The label filter's surface.  CPU: the numpy model (tests/smooth_model.py) on hand-worked cases and against its own
row-by-row restatement, the two C symbols (declared, exported, bound, NULL context refused), the argument surface of
3D_clustering/smooth_labels.py and the new flags of deep_learning_segmentation.py.  GPU: smooth_labels.py end to end on a
small labelled PLY, and --fill_unlabeled through the vote front-end."""
import importlib
import importlib.util
import json
import os
import re

import numpy as np
import pytest

import smooth_model as sm
from conftest import ROOT

pio = importlib.import_module("3d_gaussian_splatting_project_amd.ply_io")
scene = importlib.import_module("3d_gaussian_splatting_project_amd.scene")


def load_cli():
    spec = importlib.util.spec_from_file_location("cli_smooth_labels", os.path.join(ROOT, "3D_clustering", "smooth_labels.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_model_tie_rule_by_hand():
    L = np.array([7, 5, 5, 9, 9, 9, 1], np.int32)
    row = lambda *j: np.array([j], np.int32)
    one = lambda nbr, i, **kw: tuple(int(v[0]) for v in sm.round_rows(nbr, L, [i], **kw))
    assert one(row(1, 2, 3, 4), 0) == (5, 2)              # 5 and 9 tie at 2, the own label 7 is not among them: the smaller
    assert one(row(1, 2, 3, 4), 3) == (9, 2)              # the own label is among them: it stays
    assert one(row(1, 2, 3, 4), 1) == (5, 2)
    assert one(row(1, 3, 4, 5), 0) == (9, 3)              # a plain majority
    assert one(row(1, 3, 4, 5), 0, min_votes=4) == (7, 0)   # ... that misses min_votes: kept, and 7 has no vote
    assert one(row(1, 1, 1, 3, 4), 0) == (5, 3)           # a point named three times votes three times
    assert one(row(3, 4, 5, 1), 0, ignore_label=9) == (5, 1)
    assert one(row(3, 4, 5), 0, ignore_label=9) == (7, 0)   # nobody votes
    assert one(row(3, 4, 5, 1), 0, ignore_label=9, fill_only=True) == (7, 0)   # 7 is no hole
    assert one(row(0, 1, 2, 6), 3, ignore_label=9, fill_only=True) == (5, 2)   # 9 is one
    assert one(row(0, 3, 6), 0) == (7, 1) and one(row(0, 3, 6), 1) == (1, 1)   # three-way tie: own, else the smallest


def test_model_ring_by_hand():
    i = np.arange(64)
    nbr = np.stack(((i - 1) % 64, i, (i + 1) % 64), axis=1)
    L = np.where(i % 2 == 0, 11, 22).astype(np.int32)
    labels, changed, done, sup = sm.run(nbr, L, rounds=1)
    assert np.array_equal(labels, np.where(i % 2 == 0, 22, 11)) and changed == [64] and done == 1 and (sup == 2).all()
    labels, changed, done, sup = sm.run(nbr, L, rounds=2)
    assert np.array_equal(labels, L) and changed == [64, 64] and done == 2
    labels, changed, done, _ = sm.run(nbr, np.full(64, 3, np.int32), rounds=5)
    assert changed == [0, 0, 0, 0, 0] and done == 1


def test_model_vectorised_equals_row_by_row():
    rng = np.random.default_rng(0)
    for n, k, values in ((50, 1, 2), (200, 7, 3), (300, 33, 5), (120, 64, 40)):
        nbr = rng.integers(0, n, (n, k))
        L = rng.integers(-2, values - 2, n).astype(np.int32)
        L[:3] = [np.iinfo(np.int32).min, np.iinfo(np.int32).max, -1]
        for kw in (dict(), dict(min_votes=3), dict(ignore_label=-1), dict(ignore_label=-1, fill_only=True), dict(fill_only=True, fill_label=0),
                   dict(ignore_label=-1, min_votes=k + 1)):
            a, b = sm.round_rows(nbr, L, **kw), sm.round_slow(nbr, L, **kw)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (n, k, kw)


def test_symbols_declared_exported_bound(gsx):
    gsx.build()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsx.h")).read(), flags=re.S)
    lib = gsx.lib()
    for name in ("gsx_smooth_labels", "gsx_smooth_labels_lists"):
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert name in gsx._lib.declared_symbols() and hasattr(lib, name)
    assert "#define GSX_SMOOTH_IGNORE 1" in header and "#define GSX_SMOOTH_FILL_ONLY 2" in header
    assert (gsx._lib.GSX_SMOOTH_IGNORE, gsx._lib.GSX_SMOOTH_FILL_ONLY) == (1, 2)
    assert lib.gsx_abi_version() == 2
    a = np.zeros(3, np.int32)
    p = np.zeros((3, 3), np.float32)
    E = gsx._lib.GSX_E_INVALID
    assert lib.gsx_smooth_labels(None, 3, p.ctypes.data, a.ctypes.data, 1, 1, 1, 0, 0, a.ctypes.data, None, None, None) == E
    assert b"NULL" in lib.gsx_last_error(None)
    assert lib.gsx_smooth_labels_lists(None, 3, 1, a.ctypes.data, a.ctypes.data, 1, 1, 0, 0, a.ctypes.data, None, None, None) == E
    assert callable(gsx.Context.smooth_labels) and callable(gsx.Context.smooth_labels_lists)


def test_smooth_labels_cli_surface(tmp_path, capsys):
    cli = load_cli()
    args = cli.parser().parse_args(["--file_path", "a.ply", "--save_path", "b.ply"])
    assert (args.k, args.rounds, args.min_votes, args.ignore_label, args.fill_only) == (16, 1, 1, None, False)
    args = cli.parser().parse_args(["--file_path", "a", "--save_path", "b", "--k", "9", "--rounds", "3", "--min_votes", "2", "--ignore_label",
                                    "-1", "--fill_only"])
    assert (args.k, args.rounds, args.min_votes, args.ignore_label, args.fill_only) == (9, 3, 2, -1, True)
    for bad in (["--save_path", "b"], ["--file_path", "a"], ["--file_path", "a", "--save_path", "b", "--fill_only"]):
        with pytest.raises(SystemExit):
            cli.main(bad)
    capsys.readouterr()
    # refused before any GPU work: a file without labels, and labels the float32 write path would not keep
    xyz = scene.make_positions(20, 1)
    cols = {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2]}
    pio.write_vertex_ply(str(tmp_path / "plain.ply"), cols)
    with pytest.raises(ValueError, match="label"):
        cli.main(["--file_path", str(tmp_path / "plain.ply"), "--save_path", str(tmp_path / "o.ply")])
    for v in ((1 << 24) + 1, -(1 << 24) - 1):
        lab = np.zeros(20, np.int32)
        lab[7] = v
        pio.write_vertex_ply(str(tmp_path / "big.ply"), dict(cols, label=lab))
        with pytest.raises(ValueError, match="2\\^24"):
            cli.main(["--file_path", str(tmp_path / "big.ply"), "--save_path", str(tmp_path / "o.ply")])
    assert not os.path.exists(tmp_path / "o.ply")


def test_vote_frontend_flags_default_to_off():
    dls = importlib.import_module("deep_learning_segmentation")
    args = dls.make_parser().parse_args([])
    assert (args.smooth_k, args.smooth_rounds, args.fill_unlabeled) == (0, 1, False)
    args = dls.make_parser().parse_args(["--smooth_k", "12", "--smooth_rounds", "2", "--fill_unlabeled"])
    assert (args.smooth_k, args.smooth_rounds, args.fill_unlabeled) == (12, 2, True)
    with pytest.raises(SystemExit):
        dls.main(["--fill_unlabeled"])


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_smooth_labels_cli_end_to_end(ctx, tmp_path, capsys):
    n = 2000
    rng = np.random.default_rng(11)
    xyz = scene.make_positions(n, 11)
    labels = rng.integers(-1, 6, n).astype(np.int32)
    cols = {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "opacity": rng.normal(size=n).astype(np.float32), "label": labels,
            "f_dc_0": rng.normal(size=n).astype(np.float32), "tag": rng.integers(0, 255, n).astype(np.uint8)}
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    pio.write_vertex_ply(src, cols)
    before = open(src, "rb").read()
    cli = load_cli()
    cli.main(["--file_path", src, "--save_path", dst, "--k", "12", "--rounds", "3", "--ignore_label", "-1", "--min_votes", "2"])
    want, changed = ctx.smooth_labels(xyz, labels, k=12, rounds=3, ignore_label=-1, min_votes=2)
    assert changed[0] > 0
    printed = capsys.readouterr().out
    for r, ch in enumerate(changed):
        assert f"round {r + 1}: {ch} labels changed" in printed
    assert open(src, "rb").read() == before
    head_in, body_in = before.split(b"end_header\n", 1)
    head_out, body_out = open(dst, "rb").read().split(b"end_header\n", 1)
    assert head_out == head_in                                          # the same properties, types and order
    dt = pio.PlyData.read(src)["vertex"].data.dtype
    a, b = np.frombuffer(body_in, dt), np.frombuffer(body_out, dt)
    for name in cols:
        if name != "label":
            assert a[name].tobytes() == b[name].tobytes(), name
    assert np.array_equal(b["label"], want)
    # fill only: every label that is not -1 survives
    cli.main(["--file_path", src, "--save_path", dst, "--k", "12", "--ignore_label", "-1", "--fill_only"])
    out = pio.PlyData.read(dst)["vertex"]["label"]
    assert np.array_equal(out[labels != -1], labels[labels != -1]) and (out[labels == -1] != -1).any()
    assert np.array_equal(out, ctx.smooth_labels(xyz, labels, k=12, ignore_label=-1, fill_only=True)[0])


@pytest.mark.gpu
def test_fill_unlabeled_through_the_vote_frontend(ctx, tmp_path):
    """the scene of the vote front-end's own end-to-end test (test_render_gpu.py::test_cli_end_to_end), voted plain and with
    --smooth_k 8 --fill_unlabeled"""
    from PIL import Image
    dls = importlib.import_module("deep_learning_segmentation")
    n, V, W, H = 20_000, 6, 320, 180
    pos, cams, segs = scene.make_scene(n, V, W, H, config_id=21, convention="w2c")
    ply_in = str(tmp_path / "in.ply")
    pio.write_vertex_ply(ply_in, {"x": pos[:, 0], "y": pos[:, 1], "z": pos[:, 2], "opacity": np.zeros(n, np.float32)})
    json.dump(cams, open(tmp_path / "cameras.json", "w"))
    img_dir, seg_dir = tmp_path / "images", tmp_path / "segmaps"
    img_dir.mkdir(); seg_dir.mkdir()
    for cam, seg in zip(cams, segs):
        np.save(seg_dir / f"{cam['img_name']}_segmap.npy", seg)
        Image.new("L", (W, H)).save(img_dir / f"{cam['img_name']}.png")
    common = ["--ply_file", ply_in, "--camera_file", str(tmp_path / "cameras.json"), "--input_dir", str(img_dir), "--output_dir",
              str(tmp_path / "segout"), "--model", "segformer", "--segmap_dir", str(seg_dir)]
    dls.main(common + ["--output_file", str(tmp_path / "plain.ply")])
    dls.main(common + ["--output_file", str(tmp_path / "filled.ply"), "--smooth_k", "8", "--fill_unlabeled"])
    plain = pio.PlyData.read(str(tmp_path / "plain.ply"))["vertex"]
    filled = pio.PlyData.read(str(tmp_path / "filled.ply"))["vertex"]
    a, b = np.array(plain["label"]), np.array(filled["label"])
    assert filled.properties == plain.properties and np.array_equal(filled["x"], pos[:, 0])
    assert (a == -1).any(), "the scene has Gaussians no view sees"
    assert np.array_equal(b[a != -1], a[a != -1])
    assert (b[a == -1] != -1).any()
    assert np.array_equal(b, ctx.smooth_labels(pos, a, k=8, ignore_label=-1, fill_only=True)[0])
