"""CPU: the numpy model of the class-map producer (tests/segmap_model.py) against the reference-made fixture
(tests/golden/segmap.npz), its resize rule against a scalar double-precision loop, and the new entry points' argument checks."""
import ctypes as C

import numpy as np
import pytest

import segmap_model as M
from segmap_cases import boundary_volume, logits_cases, masks_cases

LOGITS, MASKS = logits_cases(), masks_cases()


@pytest.mark.parametrize("case", LOGITS, ids=[c[0] for c in LOGITS])
def test_model_reproduces_logits_fixture(case):
    name, logits, (W, H), want = case
    got = M.segmap_from_logits(logits, W, H)
    assert got.dtype == np.int32 and want.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(M.segmap_from_logits(logits[None], W, H), want[None])


@pytest.mark.parametrize("case", MASKS, ids=[c[0] for c in MASKS])
def test_model_reproduces_masks_fixture(case):
    name, masks, cls, conf, (W, H), want = case
    got = M.segmap_from_masks(masks, cls, conf, W, H)
    assert got.dtype == np.int32 and want.dtype == np.int32 and np.array_equal(got, want)


def test_fixture_holds_the_cases_the_kernels_are_pinned_on():
    names = {c[0]: c for c in MASKS}
    assert names["k0"][1].shape[0] == 0 and (names["k0"][5] == -1).all()
    assert (names["all_rejected"][5] == -1).all()
    assert (names["low_over_high"][5] == 20).all()                      # the later, less confident instance owns the pixels
    assert 2 not in names["conf_half"][5] and set(np.unique(names["conf_half_up"][5])) == {-1, 2}
    assert float(names["conf_half_up"][3][1]) == float(np.nextafter(np.float32(0.5), np.float32(1)))
    assert (names["mask_half"][1] == 0.5).any() and set(np.unique(names["mask_half"][5])) == {4, 5}
    assert set(np.unique(names["fraction_class"][5])) <= {-1, 0, 2, 41}   # 0.99 -> 0, 2.9 -> 2, 41.5 -> 41
    assert names["rows2_to_98"][1].shape[1] == 2 and names["rows2_to_98"][5].shape[0] == 98
    sp = {c[0]: c for c in LOGITS}["special"]
    assert np.isnan(sp[1]).any() and np.isinf(sp[1]).any() and np.signbit(sp[1][sp[1] == 0]).any()
    for n, logits, size, m in LOGITS:
        assert logits.shape[0] <= 16 and logits.shape[1] <= 8 and logits.shape[2] <= 8


def test_argmax_rule_is_torch_argmax():
    """the model's arg-max is torch.argmax on the CPU, for fp32, fp16 and bf16 (bf16 has no numpy dtype: its values are fp32 values)"""
    import torch
    K = {"step": 4, "slices": 8}
    vols = [boundary_volume(c, K) for c in (1, 5, 37)] + [c[1] for c in LOGITS]
    for v in vols:
        t = torch.from_numpy(v)
        assert np.array_equal(M.argmax_channels(v), t.argmax(dim=0).numpy())
        h = t.to(torch.float16)
        assert np.array_equal(M.argmax_channels(h.numpy()), h.argmax(dim=0).numpy())
        b = t.to(torch.bfloat16)
        assert np.array_equal(M.argmax_channels(b.to(torch.float32).numpy()), b.argmax(dim=0).numpy())


def test_index_table_equals_a_scalar_double_loop():
    for S in range(1, 9):
        for D in range(1, 401):
            t = M.nearest_index(S, D)
            assert t.tolist() == M.nearest_index_scalar(S, D), (S, D)
            assert t[0] == 0 and t.max() <= S - 1 and (np.diff(t) >= 0).all()


def test_the_three_rules_disagree_where_the_issue_says():
    pairs = M.disagreeing_pairs()
    assert len(pairs) >= 20 and (2, 98) in pairs
    t = M.nearest_index(2, 98)
    assert t[49] == 0 and M.nearest_index_exact(2, 98)[49] == 1 and M.nearest_index_torch(2, 98)[49] == 1
    for S, D in ((160, 1920), (160, 1080), (160, 3114), (448, 2075)):      # the sizes of real runs: all three agree
        a = M.nearest_index(S, D)
        assert np.array_equal(a, M.nearest_index_exact(S, D)) and np.array_equal(a, M.nearest_index_torch(S, D))


def test_resize_covers_up_and_down():
    a = np.arange(12).reshape(3, 4)
    assert np.array_equal(M.resize_nearest(a, 4, 3), a)
    assert np.array_equal(M.resize_nearest(a, 8, 6), np.repeat(np.repeat(a, 2, 0), 2, 1))
    assert np.array_equal(M.resize_nearest(a, 2, 1), a[:1, ::2])
    assert np.array_equal(M.resize_nearest(a, 1, 1), a[:1, :1])


# ---- the C ABI: symbols and argument checks (no GPU: every call below fails before anything touches a device) --------------------------
def test_library_exports_the_segmap_symbols_and_rejects_bad_arguments(gsx):
    gsx.build()
    lib = gsx.lib()
    for n in ("gsx_segmap_from_logits", "gsx_segmap_from_masks", "gsx_debug_segmap_constants"):
        assert hasattr(lib, n)
    L = gsx._lib
    assert (L.GSX_F32, L.GSX_F16, L.GSX_BF16) == (0, 1, 2)
    INV = L.GSX_E_INVALID
    buf = (C.c_float * 64)()
    out = (C.c_int32 * 64)()
    p, o = C.addressof(buf), C.addressof(out)
    ok = dict(logits=p, dtype=L.GSX_F32, n=1, C=2, h=2, w=2, out_w=3, out_h=3, maps=o)

    def logits(**kw):
        a = dict(ok, **kw)
        return lib.gsx_segmap_from_logits(None, a["logits"], a["dtype"], a["n"], a["C"], a["h"], a["w"], a["out_w"], a["out_h"], a["maps"])

    assert logits() == INV and b"NULL" in lib.gsx_last_error(None)       # the NULL ctx itself
    for bad in (dict(logits=None), dict(maps=None), dict(n=0), dict(C=0), dict(h=0), dict(w=-1), dict(out_w=0), dict(out_h=-5),
                dict(dtype=3), dict(dtype=-1), dict(logits=p + 2), dict(logits=p + 1, dtype=L.GSX_F16), dict(maps=o + 2)):
        assert logits(**bad) == INV, bad
    okm = dict(masks=p, dtype=L.GSX_F32, K=2, mh=2, mw=2, cls=p + 32, conf=p + 64, out_w=3, out_h=3, map=o)

    def masks(**kw):
        a = dict(okm, **kw)
        return lib.gsx_segmap_from_masks(None, a["masks"], a["dtype"], a["K"], a["mh"], a["mw"], a["cls"], a["conf"], a["out_w"], a["out_h"],
                                         a["map"])

    assert masks() == INV
    for bad in (dict(masks=None), dict(cls=None), dict(conf=None), dict(map=None), dict(K=-1), dict(mh=0), dict(mw=0), dict(out_w=0),
                dict(out_h=0), dict(dtype=7), dict(masks=p + 2), dict(masks=p + 1, dtype=L.GSX_BF16), dict(cls=p + 34), dict(conf=p + 66),
                dict(map=o + 1)):
        assert masks(**bad) == INV, bad
    assert masks(K=0, masks=None, cls=None, conf=None) == INV              # allowed arguments: what is left is the NULL ctx
    assert lib.gsx_debug_segmap_constants(None) == INV
    K = gsx.segmap_constants()
    assert K["pix_wg"] == 64 * K["vec"] and K["block"] == 64 * K["slices"] and K["step"] >= 1 and K["resize_vec"] >= 1
