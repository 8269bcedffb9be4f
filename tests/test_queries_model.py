"""CPU: the numpy model of the Mask2Former query post-processing (tests/queries_model.py) against the reference-made fixture
(tests/golden/segmap_queries.npz), its index rules against scalar loops, and the new entry point's argument checks."""
import ctypes as C
import math

import numpy as np
import pytest

import queries_model as QM
from queries_cases import constructed_cases, fixture_cases, model

FIX = fixture_cases()
F = np.float32


@pytest.mark.parametrize("case", FIX, ids=[c["name"] for c in FIX])
def test_model_equals_the_reference_off_the_knife_edge(case):
    c = case
    assert c["masks"].shape[0] <= 20 and c["class_logits"].shape[1] <= 9 and max(c["masks"].shape[1:]) <= 24
    assert c["size"][0] <= 64 and c["size"][1] <= 48 and c["mid"] == (384, 384)
    res = model(c)
    # the conditions every committed case must meet, on the reference alone
    assert not QM.knife_slots(res, c["slot_query"], len(c["masks"])).any()
    knife = QM.knife_pixels(res, c["masks"], c["slot_query"], c["size"])
    assert knife.mean() <= 1e-3
    diff = res["map"] != c["map"]
    print(c["name"], "differing pixels", int(diff.sum()), "knife-edge pixels", int(knife.sum()))
    assert res["map"].dtype == np.int32 and res["map"].shape == c["map"].shape and not (diff & ~knife).any()
    # segments_info: count, label ids in acceptance order, scores (transformers rounds them to six places)
    acc = res["slot_segment"] >= 0
    assert int(acc.sum()) == len(c["label_ids"]) and np.array_equal(c["slot_label"][acc], c["label_ids"])
    assert np.array_equal(res["slot_segment"][acc], np.arange(acc.sum()))
    assert np.abs(res["slot_pred"][acc].astype(np.float64) - c["scores"]).max(initial=0) <= 1e-6 + 5e-7
    # labels mode: the lookup of the reference's segments
    lut = np.concatenate([c["label_ids"], [-1]]).astype(np.int32)
    want = lut[c["map"]]
    got = model(c, labels=True)["map"]
    assert not ((got != want) & ~knife).any()


@pytest.mark.parametrize("case", FIX, ids=[c["name"] for c in FIX])
def test_fixture_slots_are_the_largest_probabilities(case):
    """the recorded slot order is torch's; its SET is numpy's top-Q of the Q * C class probabilities"""
    c = case
    Q, C1 = c["class_logits"].shape
    top, p = QM.select_slots(c["class_logits"])
    flat = c["slot_query"].astype(np.int64) * (C1 - 1) + c["slot_label"]
    assert len(flat) == Q and set(int(i) for i in flat) == top
    assert np.abs(p[flat] - c["slot_score"]).max() <= 1e-6


def test_index_rules_against_scalar_loops():
    for S, D in [(1, 1), (1, 7), (7, 1), (3, 384), (96, 384), (384, 384), (500, 384), (2, 98), (24, 384), (384, 1080), (384, 37)]:
        scale = F(S) / F(D)
        i0, i1, l0, l1 = QM.bilinear_axis(S, D)
        for d in range(D):
            src = max(F(scale * F(d + 0.5)) - F(0.5), F(0))
            a = int(src)
            assert (i0[d], i1[d]) == (a, a + (a < S - 1)) and l1[d] == F(src - F(a)) and l0[d] == F(F(1) - l1[d]), (S, D, d)
        assert i1.max() <= S - 1
        near = QM.nearest_torch(S, D)
        assert [int(v) for v in near] == [min(int(math.floor(F(F(d) * scale))), S - 1) for d in range(D)]
    pairs = QM.differing_pairs()
    assert len(pairs) >= 6
    S, D = pairs[0]
    assert (QM.nearest_torch(S, D) != QM.nearest_exact(S, D)).any() and (QM.nearest_torch(S, D) != QM.nearest_opencv(S, D)).any()


def test_model_on_the_constructed_edges(gsx):
    """what the constructed cases are built to show, on the model alone"""
    gsx.build()
    cases = {c["name"]: c for c in constructed_cases(gsx.queries_constants())}
    c = cases["v_zero"]
    r = model(c)
    assert np.array_equal(r["v"][0], np.array([[-3, -2, 0, 1]], F)) and np.array_equal(r["map"], [[-1, -1, -1, 0]])
    c = cases["on_threshold"]
    r = model(c)
    assert np.array_equal(r["slot_pred"], c["slot_score"]) and r["slot_segment"].tolist() == [-1, 0, -1] and (r["map"] == 0).all()
    c = cases["unsampled"]
    r = model(c)
    assert r["slot_segment"].tolist() == [-1, 0, -1, -1, 1] and (r["slot_pred"] > 0.5).all()
    assert set(np.unique(r["map"])) == {-1, 1} and set(np.unique(model(c, labels=True)["map"])) == {-1, int(c["slot_label"][4])}
    c = cases["nan_inf"]
    r = model(c)
    assert r["slot_segment"].tolist() == [0, -1, 1, -1, 2] and np.isnan(r["slot_pred"][[1, 3]]).all() and (r["map"] == 2).all()
    assert np.isinf(c["masks"][1]).sum() == 1 and np.isnan(r["v"][1]).any()
    r = model(cases["neg_inf"])
    assert r["slot_segment"].tolist() == [-1, 0] and np.isnan(r["slot_pred"][0])
    c = cases["bad_query"]
    r = model(c)
    assert r["slot_segment"][1] == -1 and r["slot_segment"][4] == -1 and r["slot_pred"][1] == 0 and (r["slot_segment"] >= 0).sum() >= 3
    r = model(cases["rejected_after"])
    assert r["slot_segment"].tolist() == [0, -1, -1] and (r["map"] == 0).all()
    r = model(cases["all_rejected"])
    assert (r["slot_segment"] == -1).all() and (r["map"] == -1).all()
    for c in cases.values():
        r = model(c)
        if not c["exact"]:
            assert not QM.knife_slots(r, c["slot_query"], len(c["masks"]), c["threshold"]).any(), c["name"]
        if c["name"].startswith(("mid_", "src_", "nearest_")) or c["name"] in ("k63", "k64", "k65", "k129"):
            assert (r["slot_segment"] >= 0).any() and (r["slot_segment"] < 0).any(), c["name"]     # both kinds of slot


# ---- the C ABI: symbols and argument checks (no GPU: every call below fails before anything touches a device) --------------------------
def test_library_exports_the_queries_symbols_and_rejects_bad_arguments(gsx):
    gsx.build()
    lib, L = gsx.lib(), gsx._lib
    for n in ("gsx_segmap_from_queries", "gsx_debug_queries_constants"):
        assert hasattr(lib, n)
    assert (L.GSX_QUERIES_SEGMENTS, L.GSX_QUERIES_LABELS) == (0, 1)
    INV = L.GSX_E_INVALID
    buf, out = (C.c_float * 256)(), (C.c_int32 * 256)()
    p, o = C.addressof(buf), C.addressof(out)
    ok = dict(masks=p, dtype=L.GSX_F32, Q=2, h=2, w=2, K=2, sq=o + 64, ss=p + 64, sl=o + 128, mid_w=4, mid_h=4, thr=0.5, mode=0, out_w=3,
              out_h=3, map=o, seg=o + 192, pred=p + 192)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gsx_segmap_from_queries(None, a["masks"], a["dtype"], a["Q"], a["h"], a["w"], a["K"], a["sq"], a["ss"], a["sl"], a["mid_w"],
                                           a["mid_h"], a["thr"], a["mode"], a["out_w"], a["out_h"], a["map"], a["seg"], a["pred"])

    assert call() == INV and b"NULL" in lib.gsx_last_error(None)       # the NULL ctx itself
    for bad in (dict(masks=None), dict(map=None), dict(sq=None), dict(ss=None), dict(sl=None, mode=1), dict(Q=0), dict(h=0), dict(w=-1),
                dict(mid_w=0), dict(mid_h=0), dict(out_w=0), dict(out_h=-3), dict(K=-1), dict(dtype=3), dict(mode=2), dict(mode=-1),
                dict(masks=p + 2), dict(masks=p + 1, dtype=L.GSX_F16), dict(sq=o + 66), dict(ss=p + 65), dict(sl=o + 130), dict(map=o + 2),
                dict(seg=o + 194), dict(pred=p + 193), dict(thr=float("nan")), dict(thr=float("inf")), dict(K=1025),
                dict(Q=1 << 16, h=1 << 8, w=1 << 7), dict(mid_w=1 << 16, mid_h=1 << 15), dict(out_w=1 << 16, out_h=1 << 15)):
        assert call(**bad) == INV, bad
    assert lib.gsx_debug_queries_constants(None) == INV
    U = gsx.queries_constants()
    assert U["cols"] == 64 and U["rows_wg"] % U["rows_wave"] == 0 and U["block"] == 64 * U["rows_wg"] // U["rows_wave"]
    assert U["scan_word"] == 64 and U["max_slots"] == 1024 == U["scan_word"] * U["accept_waves"]
