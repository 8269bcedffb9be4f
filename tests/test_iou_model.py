"""CPU: the numpy model of the IoU evaluation (tests/iou_model.py) and the library's two host-only helpers against what the
reference's own evaluation.py computed (tests/golden/iou.npz).  Every comparison is exact."""
import random

import numpy as np
import pytest

import iou_model as M
from conftest import load_pkg
from iou_cases import LABELME, copies, fixture, mask_cases, same_doubles

CASES = mask_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_model_matches_the_reference(case):
    name, masks, gts, iou, best_iou, best_gt = case
    got = M.iou(masks, gts)
    assert same_doubles(got, iou)
    b, i = M.best(got)
    assert same_doubles(b, best_iou) and np.array_equal(i, best_gt)


def test_fixture_holds_the_cases_the_semantics_rest_on():
    z = fixture()
    assert z["example/iou"][0, 0] == 4 / 14
    # the in-place edit: every set pixel of both arguments became 1
    assert np.array_equal(z["example/after1"], (z["example/mask0"] != 0).astype(z["example/mask0"].dtype))
    assert np.array_equal(z["example/after2"], (z["example/gt0"] != 0).astype(z["example/gt0"].dtype))
    f = z["float_edges/mask0"]
    assert np.isnan(f[0, 0]) and np.signbit(f[0, 1]) and f[0, 1] == 0 and np.isinf(f[0, 2]) and 0 < f[0, 3] < 1e-38
    assert M.set_pixels(f)[0].tolist() == [True, False, True, True, True, False, True]
    assert z["int32_256/mask0"][1, 1] == 256 and z["int64_2p32/mask0"][1, 1] == 2 ** 32
    assert np.isnan(z["empty/iou"]).all() and z["empty/best_iou"][0] == 0 and z["empty/best_gt"][0] == 0
    assert z["ties/iou"][0, 0] == z["ties/iou"][0, 1] and z["ties/iou"][0, 2] == z["ties/iou"][0, 3] == 1 and z["ties/best_gt"][0] == 2
    assert z["equal/iou"][0, 0] == 1.0
    assert z["random_5x4/iou"].shape == (5, 4) and z["random_5x4/mask0"].shape == (37, 53)
    assert z["random_5x4/best_iou"][4] == 0 and z["random_5x4/best_gt"][4] == 0      # an empty mask: no positive IoU
    shapes = {"0001_2": (1920, 1080), "0001_3": (1920, 1080), "DSCF4667": (1038, 1557), "street": (415, 612)}
    tops = {"0001_2": 2, "0001_3": 6, "DSCF4667": 18, "street": 6}
    for n in LABELME:
        a = z[f"labelme/{n}"]
        assert a.dtype == np.uint8 and a.shape == shapes[n] and a.min() == 0 and a.max() == tops[n]


def test_model_segmentation_map_matches_the_reference():
    z = fixture()
    masks = [z[f"segmap/mask{i}"] for i in range(int(z["segmap/n_masks"]))]
    random.seed(int(z["segmap/seed"]))
    palette = np.array([[random.random(), random.random(), random.random()] for _ in masks])
    owner = M.top_index(masks)
    img = np.zeros(owner.shape + (3,))
    img[owner >= 0] = palette[owner[owner >= 0]]
    assert img.dtype == z["segmap/map"].dtype and np.array_equal(img.view(np.int64), z["segmap/map"].view(np.int64))
    assert (owner == -1).any() and len(np.unique(owner)) == len(masks) + 1


def labelme_pairs():
    z = fixture()
    yield "0001_2_vs_0001_3", z["labelme/0001_2"], z["labelme/0001_3"], z["labelme/0001_2_vs_0001_3/iou"]
    for n in ("DSCF4667", "street"):
        yield f"{n}_shift3", z[f"labelme/{n}"], np.roll(z[f"labelme/{n}"], 3, axis=1), z[f"labelme/{n}_shift3/iou"]


@pytest.mark.parametrize("pair", list(labelme_pairs()), ids=[p[0] for p in labelme_pairs()])
def test_model_table_gives_the_reference_iou_on_the_labelme_maps(pair):
    name, a, b, iou = pair
    ka, kb = iou.shape
    t = M.table(a, b, ka, kb)
    assert t.sum() == a.size and (t[0] == 0).all() and (t[:, 0] == 0).all()
    assert same_doubles(M.iou_from_table(t)[1:, 1:], iou)
    g = load_pkg()
    assert same_doubles(g.iou_from_table(t)[1:, 1:], iou)        # the library's own quotient, through ctypes
    if name == "0001_2_vs_0001_3":
        z = fixture()
        for best, idx in (M.best(iou), g.iou_best(iou)):
            assert same_doubles(best, z[f"labelme/{name}/best_iou"]) and np.array_equal(idx, z[f"labelme/{name}/best_gt"])


def test_table_equals_inter_area_on_indicator_masks():
    rng = np.random.default_rng(5)
    a = rng.integers(-1, 4, (23, 31)).astype(np.int32)
    b = rng.integers(-1, 6, (23, 31)).astype(np.int64)
    t = M.table(a, b, 4, 6)
    inter, am, ag = M.inter_area([a == i for i in range(-1, 4)], [b == j for j in range(-1, 6)])
    assert np.array_equal(t, inter) and np.array_equal(t.sum(1), am) and np.array_equal(t.sum(0), ag)
    assert same_doubles(M.iou_from_table(t), M.iou([a == i for i in range(-1, 4)], [b == j for j in range(-1, 6)]))
    u8 = (a + 1).astype(np.uint8)
    assert np.array_equal(M.table(u8, (b + 1).astype(np.uint8), 4, 6, packed_u8=True), t)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_helpers_match_the_reference(case):
    """gsx_iou_from_counts and gsx_iou_best through ctypes: no GPU, no context"""
    g = load_pkg()
    name, masks, gts, iou, best_iou, best_gt = case
    inter, am, ag = M.inter_area(masks, gts)
    got = g.iou_from_counts(inter, am[:, None], ag[None, :])
    assert same_doubles(got, iou)
    b, i = g.iou_best(got)
    assert i.dtype == np.int32 and same_doubles(b, best_iou) and np.array_equal(i, best_gt)


def test_host_helpers_on_nan_tie_and_zero_rows():
    g = load_pkg()
    nan = float("nan")
    iou = np.array([[nan, nan, nan], [0.0, 0.0, 0.0], [0.25, 0.5, 0.5], [nan, 0.75, nan], [1.0, 1.0, 0.0], [0.0, nan, 5e-324]])
    b, i = g.iou_best(iou)
    mb, mi = M.best(iou)
    assert same_doubles(b, mb) and np.array_equal(i, mi)
    assert b.tolist() == [0.0, 0.0, 0.5, 0.75, 1.0, 5e-324] and i.tolist() == [0, 0, 1, 1, 0, 2]
    inter = np.array([0, 0, 3, 2 ** 40, 1], np.int64)
    a = np.array([0, 5, 3, 2 ** 40 + 1, 2 ** 52], np.int64)
    c = np.array([0, 0, 3, 2 ** 41, 1], np.int64)
    got = g.iou_from_counts(inter, a, c)
    assert same_doubles(got, M.iou_from_counts(inter, a, c))
    assert np.isnan(got[0]) and got[1] == 0 and got[2] == 1 and got[3] == 2.0 ** 40 / (2.0 ** 41 + 1)
    assert g.iou_best(np.zeros((0, 3)))[0].shape == (0,)
    L = g.lib()
    assert L.gsx_iou_from_counts(2, None, None, None, None) == g._lib.GSX_E_INVALID and b"iou_from_counts" in L.gsx_last_error(None)
    assert L.gsx_iou_best(1, 1, None, None, None) == g._lib.GSX_E_INVALID
    assert L.gsx_debug_iou_constants(None) == g._lib.GSX_E_INVALID
    with pytest.raises(ValueError):
        g.iou_best(np.zeros(3))


def test_reference_loop_agrees_with_the_model():
    name, masks, gts, iou, best_iou, best_gt = [c for c in CASES if c[0] == "random_5x4"][0]
    before = copies(masks)
    got = M.reference_loop(masks, gts)
    assert all(np.array_equal(x, y) for x, y in zip(before, masks))      # it works on copies
    assert [int(g[1]) for g in got] == best_gt.tolist() and same_doubles([float(g[0]) for g in got], best_iou)


def test_input_normalisation_picks_exact_conversions():
    g = load_pkg()
    L, lib = g.labeler, g._lib
    f16 = np.array([[np.nan, -0.0, 6e-8, 0.0]], np.float16)
    dev, items, code = L._iou_list([f16], "masks")
    assert not dev and code == lib.GSX_MASK_F32 and np.array_equal(M.set_pixels(items[0]), M.set_pixels(f16))
    for arr, want in ((np.array([[True, False]]), lib.GSX_MASK_U8), (np.array([[-1, 0]], np.int8), lib.GSX_MASK_U8),
                      (np.array([[2 ** 31, 0]], np.uint32), lib.GSX_MASK_I32), (np.array([[2 ** 63, 0]], np.uint64), lib.GSX_MASK_I64),
                      (np.array([[-256, 0]], np.int16), lib.GSX_MASK_I32), (np.array([[65535, 0]], np.uint16), lib.GSX_MASK_I32)):
        _, items, code = L._iou_list([arr], "masks")
        assert code == want and np.array_equal(M.set_pixels(items[0]), M.set_pixels(arr)), arr.dtype
    _, items, code = L._iou_list([np.array([[2 ** 32, 0]], np.int64), np.array([[-0.0, 1e-45]], np.float32)], "masks")
    assert code == lib.GSX_MASK_F64 and [M.set_pixels(t).tolist() for t in items] == [[[True, False]], [[False, True]]]
    _, items, code = L._iou_list(np.zeros((3, 4, 5), np.float64)[:, ::2], "masks")
    assert len(items) == 3 and all(t.flags.c_contiguous and t.shape == (2, 5) for t in items)
    with pytest.raises(ValueError):
        L._iou_shape([np.zeros((2, 3)), np.zeros((3, 2))])
    with pytest.raises(ValueError):
        L._iou_list([], "masks")
    with pytest.raises(ValueError):
        L._iou_list([np.zeros(3)], "masks")
