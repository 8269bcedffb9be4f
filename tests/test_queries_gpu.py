"""GPU: the Mask2Former query post-processing (csrc/queries.hip, Context.segmap_from_queries) against the numpy model
(tests/queries_model.py) and the reference-made fixture (tests/golden/segmap_queries.npz), at the edges of the units its kernels
are built on (gsx_debug_queries_constants), and chained into the vote.  Maps and segment ids are compared with np.array_equal,
scores within 1e-6; every case asserts on the model that its inputs hold no knife-edge slot."""
import numpy as np
import pytest

import queries_model as QM
from conftest import golden_assign_cases
from queries_cases import constructed_cases, fixture_cases, model, reference_shape_case, seeded

pytestmark = pytest.mark.gpu

FIX = fixture_cases()
DTYPES = ("float32", "float16", "bfloat16")
F = np.float32


@pytest.fixture(scope="module")
def U(gsx):
    """the units the kernels are built on, exported from the source"""
    return gsx.queries_constants()


def seen_by(c, dtype):
    """the case with its mask logits rounded to `dtype` -> (torch CPU tensor of that dtype, the case the model sees)"""
    import torch
    t = torch.from_numpy(c["masks"]).to(getattr(torch, dtype))
    return t, dict(c, masks=t.to(torch.float32).numpy())


def device(ctx, c, t, labels):
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out, seg, pred = ctx.segmap_from_queries(t.cuda(), dev(c["slot_query"]), dev(c["slot_score"]), c["size"], slot_label=dev(c["slot_label"]),
                                             mid=c["mid"], threshold=c["threshold"], labels=labels, return_slots=True)
    return out.cpu().numpy(), seg.cpu().numpy(), pred.cpu().numpy()


def check(ctx, c, dtype="float32"):
    """both modes and both optional outputs against the model; returns the model's result in segment mode"""
    t, c = seen_by(c, dtype)
    first = None
    for labels in (False, True):
        want = model(c, labels)
        if not c.get("exact"):
            assert not QM.knife_slots(want, c["slot_query"], len(c["masks"]), c["threshold"]).any(), c["name"]
        got, seg, pred = device(ctx, c, t, labels)
        assert got.dtype == np.int32 and seg.dtype == np.int32 and pred.dtype == F
        assert np.array_equal(seg, want["slot_segment"]), (c["name"], labels)
        assert np.array_equal(np.isnan(pred), np.isnan(want["slot_pred"])), c["name"]
        err = np.abs(np.nan_to_num(pred).astype(np.float64) - np.nan_to_num(want["slot_pred"])).max(initial=0)
        print(c["name"], dtype, "labels" if labels else "segments", "max score error", err)
        assert err <= 1e-6, (c["name"], err)
        if c.get("exact"):
            assert np.array_equal(pred, want["slot_pred"]), c["name"]
        assert np.array_equal(got, want["map"]), (c["name"], labels, int((got != want["map"]).sum()))
        first = first or want
    return first


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", FIX, ids=[c["name"] for c in FIX])
def test_fixture(ctx, c, dtype):
    want = check(ctx, c, dtype)
    if dtype == "float32":                       # the reference's own output, off the knife-edge pixels (none in these cases)
        knife = QM.knife_pixels(want, c["masks"], c["slot_query"], c["size"])
        assert not ((want["map"] != c["map"]) & ~knife).any()
        acc = want["slot_segment"] >= 0
        assert np.array_equal(c["slot_label"][acc], c["label_ids"])


def test_constructed_edges(ctx, U):
    cases = constructed_cases(U)
    names = [c["name"] for c in cases]
    for mw in (1, U["cols"] - 1, U["cols"], U["cols"] + 1, 2 * U["cols"] + 1):
        assert f"mid_{mw}x1" in names and f"mid_{mw}x5" in names
    for K in (1, U["scan_word"] - 1, U["scan_word"], U["scan_word"] + 1, 2 * U["scan_word"] + 1):
        assert f"k{K}" in names
    for c in cases:
        check(ctx, c)


@pytest.mark.parametrize("dtype", DTYPES[1:])
def test_constructed_edges_in_half_formats(ctx, U, dtype):
    for c in constructed_cases(U):
        if c["name"].startswith(("mid_", "src_")) or c["name"] in ("v_zero", "nan_inf", "on_threshold", "unsampled"):
            check(ctx, c, dtype)


def test_k0_writes_the_background(ctx):
    import torch
    m = torch.ones(2, 3, 3, device="cuda")
    e = torch.zeros(0, device="cuda")
    for labels in (False, True):
        out, seg, pred = ctx.segmap_from_queries(m, e.to(torch.int32), e, (7, 5), slot_label=e.to(torch.int32), mid=(70, 9), labels=labels,
                                                 return_slots=True)
        assert out.shape == (5, 7) and (out.cpu().numpy() == -1).all() and seg.numel() == 0 and pred.numel() == 0
    assert (ctx.segmap_from_queries(m, [], [], (3, 2)).cpu().numpy() == -1).all()


def test_no_stale_bit_planes_and_two_runs_agree(ctx, U):
    """K = 129 and then K = 3 on the same context, at the same mid grid; every call twice, bit for bit"""
    big = seeded("k129_then", 2100, 9, 6, 6, 2 * U["scan_word"] + 1, (21, 13), (70, 9))
    small = seeded("k3_after", 2101, 9, 6, 6, 3, (21, 13), (70, 9))
    for c in (big, small, big, small):
        check(ctx, c)
    t, c = seen_by(big, "float32")
    a, b = device(ctx, c, t, False), device(ctx, c, t, False)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_limits(ctx, gsx):
    """K > 1024 and the 2^31 limits fail with GSX_E_UNSUPPORTED before any launch (the pointers are never read)"""
    import torch
    lib, L = gsx.lib(), gsx._lib
    t = torch.zeros(16, device="cuda")
    o = torch.zeros(16, dtype=torch.int32, device="cuda")
    out = torch.zeros(16, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def call(Q=1, h=2, w=2, K=1, mid_w=4, mid_h=4, thr=0.5, mode=0, out_w=2, out_h=2, masks=t.data_ptr(), dtype=L.GSX_F32):
        return lib.gsx_segmap_from_queries(ctx.h, masks, dtype, Q, h, w, K, o.data_ptr(), t.data_ptr(), o.data_ptr(), mid_w, mid_h, thr, mode,
                                           out_w, out_h, out.data_ptr(), None, None)

    UNS, INV = L.GSX_E_UNSUPPORTED, L.GSX_E_INVALID
    assert call(K=1025) == UNS and call(Q=1 << 16, h=1 << 8, w=1 << 7) == UNS and call(mid_w=1 << 16, mid_h=1 << 15) == UNS
    assert call(out_w=1 << 16, out_h=1 << 15) == UNS and call(K=1024, mid_w=64, mid_h=1 << 21) == UNS
    assert call(K=-1) == INV and call(Q=0) == INV and call(mid_w=0) == INV and call(mode=2) == INV and call(dtype=5) == INV
    assert call(thr=float("nan")) == INV and call(thr=float("-inf")) == INV and call(masks=None) == INV and call(masks=t.data_ptr() + 2) == INV
    assert call() == L.GSX_OK
    ctx.synchronize()
    with pytest.raises(ValueError):
        ctx.segmap_from_queries(torch.zeros(2, 2, 2, dtype=torch.float64, device="cuda"), [0], [0.9], (2, 2))
    with pytest.raises(ValueError):
        ctx.segmap_from_queries(torch.zeros(2, 2, 2, device="cuda"), [0, 1], [0.9], (2, 2))
    with pytest.raises(ValueError):
        ctx.segmap_from_queries(torch.zeros(2, 2, 2, device="cuda"), [0], [0.9], (2, 2), labels=True)


def test_write_only_the_outputs(ctx, gsx):
    """map, slot_segment and slot_pred_score inside larger allocations prefilled with a sentinel: nothing else is written"""
    import torch
    c = seeded("guards", 2200, 5, 4, 6, 7, (13, 9), (70, 5))
    want = model(c)
    W, H = c["size"]
    K = len(c["slot_query"])
    lib, L = gsx.lib(), gsx._lib
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    m, sq, ss, sl = dev(c["masks"]), dev(c["slot_query"]), dev(c["slot_score"]), dev(c["slot_label"])
    for shift in (0, 1):
        big = torch.full((H * W + 64,), -77, dtype=torch.int32, device="cuda")
        seg = torch.full((K + 64,), -77, dtype=torch.int32, device="cuda")
        pred = torch.full((K + 64,), -77.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        off = 32 + shift
        gsx._lib.check(lib.gsx_segmap_from_queries(ctx.h, m.data_ptr(), L.GSX_F32, 5, 4, 6, K, sq.data_ptr(), ss.data_ptr(), sl.data_ptr(), 70, 5,
                                                   0.5, 0, W, H, big.data_ptr() + 4 * off, seg.data_ptr() + 4 * off, pred.data_ptr() + 4 * off), ctx.h)
        ctx.synchronize()
        b, s, p = big.cpu().numpy(), seg.cpu().numpy(), pred.cpu().numpy()
        assert np.array_equal(b[off:off + H * W].reshape(H, W), want["map"]) and np.array_equal(s[off:off + K], want["slot_segment"])
        assert (b[:off] == -77).all() and (b[off + H * W:] == -77).all() and (s[:off] == -77).all() and (s[off + K:] == -77).all()
        assert (p[:off] == -77).all() and (p[off + K:] == -77).all() and np.abs(p[off:off + K] - want["slot_pred"]).max() <= 1e-6


def test_kernels_are_the_ones_that_ran(ctx):
    import torch
    ctx.profile(True)
    ctx.segmap_from_queries(torch.ones(2, 4, 4, device="cuda"), [0, 1, 1], [0.9, 0.9, 0.2], (8, 8), mid=(16, 16))
    ctx.synchronize()
    for name in ("queries_sampled", "queries_mask", "queries_accept", "queries_compose", "segmap_resize"):
        assert ctx.profile_get(name)[0] == 1, name
    ctx.profile(False)


def test_reference_shape(ctx):
    """Q = K = 100, masks 96 x 96, mid 384 x 384, target 480 x 270"""
    c = reference_shape_case()
    want = check(ctx, c)
    acc = want["slot_segment"] >= 0
    assert 10 <= acc.sum() < 100 and len(set(c["slot_query"][acc].tolist())) < acc.sum()      # accepted, rejected, repeated queries


# ---- chained into the vote ----------------------------------------------------------------------------------------------------------------
def test_vote_takes_the_device_map(ctx, gsx):
    """vote_view(cam, ctx.segmap_from_queries(...)) labels the scene as assign_labels_from_maps does on the model's host maps"""
    import torch
    name, positions, cams, segs, sizes, _ = next(c for c in golden_assign_cases() if c[0].startswith("rand3"))
    cs, maps = [], []
    for v, seg in enumerate(segs):
        H, W = seg.shape
        c = seeded(f"vote{v}", 2300 + 10 * v, 12, 7, 9, 12, (W, H), (96, 80))
        cs.append(c)
        maps.append(model(c)["map"])
        assert len(np.unique(maps[-1])) >= 3
    want = gsx.assign_labels_from_maps(positions, cams, maps, sizes, n_classes=150, ctx=ctx)
    ctx.upload_positions(positions)
    ctx.vote_begin(150, 0, max(1, len(cams)))
    for cam, c, size in zip(cams, cs, sizes):
        dev = ctx.segmap_from_queries(torch.from_numpy(c["masks"]).cuda(), c["slot_query"], c["slot_score"], c["size"], mid=c["mid"])
        ctx.vote_view(cam, dev, size)
    got = ctx.vote_finalize()
    assert got.dtype == np.int32 and np.array_equal(got, want) and (got >= 0).any()
    assert ctx.vote_link_bytes() == 0               # no map went through the host packer
