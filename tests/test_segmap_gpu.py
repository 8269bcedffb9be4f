"""GPU: the class-map producer (csrc/segmap.hip) against the reference-made fixture (tests/golden/segmap.npz) and the numpy
model (tests/segmap_model.py), at the edges of the units its kernels are built on (gsx_debug_segmap_constants), and chained
into the vote.  Every comparison is np.array_equal on int32."""
import numpy as np
import pytest

import segmap_model as M
from conftest import golden_assign_cases
from segmap_cases import boundary_volume, channel_counts, logits_cases, masks_cases, seeded_logits, seeded_masks

pytestmark = pytest.mark.gpu

LOGITS, MASKS = logits_cases(), masks_cases()
DTYPES = ("float32", "float16", "bfloat16")
SENTINEL = -77


@pytest.fixture(scope="module")
def K(gsx):
    """the units the kernels are built on, exported from the source"""
    return gsx.segmap_constants()


def as_dtype(a, dtype):
    """(torch CPU tensor of `dtype`, the same values as float32 numpy - what the model compares)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(getattr(torch, dtype))
    return t, t.to(torch.float32).numpy()


def run_logits(ctx, vol, size, dtype="float32"):
    """-> (device result as numpy, the model's map for the values the device saw)"""
    t, seen = as_dtype(vol, dtype)
    got = ctx.segmap_from_logits(t.cuda(), size).cpu().numpy()
    assert got.dtype == np.int32
    return got, M.segmap_from_logits(seen, *size)


def run_masks(ctx, masks, cls, conf, size, dtype="float32"):
    import torch
    t, seen = as_dtype(masks, dtype)
    got = ctx.segmap_from_masks(t.cuda(), torch.from_numpy(np.asarray(cls, np.float32)).cuda(),
                                torch.from_numpy(np.asarray(conf, np.float32)).cuda(), size).cpu().numpy()
    assert got.dtype == np.int32
    return got, M.segmap_from_masks(seen, cls, conf, *size)


# ---- logits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", LOGITS, ids=[c[0] for c in LOGITS])
def test_logits_fixture(ctx, case, dtype):
    name, logits, size, want = case
    got, model = run_logits(ctx, logits, size, dtype)
    assert np.array_equal(got, model)
    if dtype == "float32":
        assert np.array_equal(got, want)            # the reference's own output


def test_logits_resize_where_the_three_rules_disagree(ctx):
    """(S, D) pairs on which OpenCV's rule differs from floor(d S / D) and from torch's float32 rule, on both axes, C = 3"""
    pairs = M.disagreeing_pairs()
    assert (2, 98) in pairs
    pick = [(2, 98)] + [p for p in pairs if p != (2, 98)][:: max(1, len(pairs) // 23)][:23]
    assert len(pick) >= 20
    rng = np.random.default_rng(5)
    for i, (S, D) in enumerate(pick):
        S2, D2 = pick[(i + 7) % len(pick)]
        vol = seeded_logits(rng, (3, S, S2), ties=False)
        got, want = run_logits(ctx, vol, (D2, D))
        assert np.array_equal(got, want), (S, D, S2, D2)


@pytest.mark.parametrize("shape,size", [((5, 9), (4, 3)), ((7, 6), (6, 7)), ((8, 8), (1, 1)), ((1, 1), (9, 5)), ((1, 6), (13, 1)),
                                        ((6, 1), (1, 11)), ((3, 200), (7, 2)), ((2, 3), (301, 98))],
                         ids=lambda v: "x".join(str(x) for x in v))
def test_logits_sizes_down_same_one(ctx, shape, size):
    """S > D, S == D, D == 1, S == 1, per axis"""
    rng = np.random.default_rng(11)
    got, want = run_logits(ctx, seeded_logits(rng, (6,) + shape, ties=False), size)
    assert got.shape == (size[1], size[0]) and np.array_equal(got, want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_logits_channel_counts_and_boundaries(ctx, K, dtype):
    """C = 1, step and round of slices +-1, 255, 256, 1000: ties everywhere, and ties, NaNs, infinities and signed zeros on both
    sides of every channel-step / channel-slice boundary - an earlier tie wins, an earlier NaN beats a later +inf"""
    rng = np.random.default_rng(3)
    for Cn in channel_counts(K):
        got, want = run_logits(ctx, seeded_logits(rng, (Cn, 5, 7)), (13, 9), dtype)
        assert np.array_equal(got, want), Cn
        vol = boundary_volume(Cn, K)
        got, want = run_logits(ctx, vol, (vol.shape[2], 1), dtype)
        assert np.array_equal(got, want), (Cn, np.flatnonzero(got != want)[:8])
        assert got[0, -4] == 0 and got[0, -3] == 0 and got[0, -2] == 0      # all -inf, zeros of both signs, all NaN -> 0


def test_boundary_volume_says_what_it_should(K):
    """the constructed patterns, read back through the model: who must win"""
    vol = boundary_volume(K["step"] * K["slices"] + 2, K)
    low = M.argmax_channels(vol)[0]
    b = K["step"]
    assert low[:8].tolist() == [b - 1, 0, b - 1, b, b - 1, b - 1, b - 1, b]


@pytest.mark.parametrize("dtype", DTYPES)
def test_logits_pixel_tiles_widths_and_views(ctx, K, dtype):
    """h * w at pixels-per-workgroup +-1, w not a multiple of the load width, and a volume that starts one element into a larger
    tensor (aligned to its element only)"""
    import torch
    rng = np.random.default_rng(17)
    P = K["pix_wg"]
    shapes = [(1, P - 1), (1, P), (1, P + 1), (3, 43), (2, P), (2 * P + 1, 1), (7, K["vec"] * 9 + 1), (5, 5)]
    for h, w in shapes:
        for Cn in (3, K["step"] * K["slices"] + K["step"] + 1):
            vol = seeded_logits(rng, (Cn, h, w))
            size = (w + 3, h + 2)
            got, want = run_logits(ctx, vol, size, dtype)
            assert np.array_equal(got, want), (h, w, Cn)
            t, seen = as_dtype(vol, dtype)
            big = torch.zeros(t.numel() + 3, dtype=t.dtype, device="cuda")
            for off in (1, 2, 3):
                view = big[off:off + t.numel()].view(t.shape)
                view.copy_(t)
                assert view.data_ptr() == big.data_ptr() + off * t.element_size()
                assert np.array_equal(ctx.segmap_from_logits(view, size).cpu().numpy(), want), (h, w, Cn, off)


def test_logits_batches(ctx):
    """n = 1, 2, 3 with different volumes, one call"""
    import torch
    rng = np.random.default_rng(23)
    for n in (1, 2, 3):
        vol = seeded_logits(rng, (n, 11, 9, 15))
        got = ctx.segmap_from_logits(torch.from_numpy(vol).cuda(), (31, 20)).cpu().numpy()
        assert got.shape == (n, 20, 31) and np.array_equal(got, M.segmap_from_logits(vol, 31, 20))
        assert n == 1 or not np.array_equal(got[0], got[1])


def raw_call(ctx, gsx, fn, W, H, n, guard=3):
    """run fn(out pointer) with the n maps inside a larger allocation prefilled with a sentinel -> (maps, guards intact?)"""
    import torch
    results = []
    for shift in (0, 1):                          # the maps start 16-byte aligned, and not
        rows = n * H + 2 * guard
        big = torch.full((rows * W + shift + 4,), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        off = guard * W + shift + (-(guard * W) % 4)
        gsx._lib.check(fn(big.data_ptr() + 4 * off), ctx.h)
        ctx.synchronize()
        host = big.cpu().numpy()
        maps = host[off:off + n * H * W].reshape(n, H, W)
        rest = np.concatenate([host[:off], host[off + n * H * W:]])
        results.append((maps.copy(), bool((rest == SENTINEL).all())))
    return results


@pytest.mark.parametrize("size", [(13, 9), (16, 4), (5, 31)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_logits_write_only_the_maps(ctx, gsx, size):
    import torch
    W, H = size
    rng = np.random.default_rng(29)
    vol = seeded_logits(rng, (2, 9, 7, 10))
    t = torch.from_numpy(vol).cuda()
    lib, L = gsx.lib(), gsx._lib
    for maps, intact in raw_call(ctx, gsx, lambda p: lib.gsx_segmap_from_logits(ctx.h, t.data_ptr(), L.GSX_F32, 2, 9, 7, 10, W, H, p), W, H, 2):
        assert intact, "the call wrote outside its maps"
        assert (maps != SENTINEL).all() and np.array_equal(maps, M.segmap_from_logits(vol, W, H))


def test_unsupported_sizes(ctx, gsx):
    """C > 65535 and the 2^31 limits fail with GSX_E_UNSUPPORTED before any launch (the pointers are never read)"""
    import torch
    lib, L = gsx.lib(), gsx._lib
    t = torch.zeros(16, device="cuda")
    o = torch.zeros(16, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    call = lambda n, Cn, h, w, ow, oh: lib.gsx_segmap_from_logits(ctx.h, t.data_ptr(), L.GSX_F32, n, Cn, h, w, ow, oh, o.data_ptr())
    assert call(1, 65536, 1, 1, 1, 1) == L.GSX_E_UNSUPPORTED
    assert call(1, 2, 65536, 32768, 1, 1) == L.GSX_E_UNSUPPORTED
    assert call(1, 2, 1, 1, 65536, 32768) == L.GSX_E_UNSUPPORTED
    assert call(3, 2, 1, 1, 32768, 32768) == L.GSX_E_UNSUPPORTED
    assert call(0, 2, 1, 1, 1, 1) == L.GSX_E_INVALID and call(1, 2, 1, 1, 1, 1) == L.GSX_OK
    assert lib.gsx_segmap_from_masks(ctx.h, t.data_ptr(), L.GSX_F32, 1, 65536, 32768, t.data_ptr(), t.data_ptr(), 1, 1,
                                     o.data_ptr()) == L.GSX_E_UNSUPPORTED
    ctx.synchronize()
    with pytest.raises(ValueError):
        ctx.segmap_from_logits(torch.zeros(2, 2, 2, dtype=torch.float64, device="cuda"), (2, 2))
    with pytest.raises(ValueError):
        ctx.segmap_from_logits(torch.zeros(2, 2, 2), (2, 2))


# ---- masks --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", MASKS, ids=[c[0] for c in MASKS])
def test_masks_fixture(ctx, case, dtype):
    name, masks, cls, conf, size, want = case
    if masks.shape[0] == 0:
        got = ctx.segmap_from_masks(None, None, None, size).cpu().numpy()
        import torch
        empty = ctx.segmap_from_masks(torch.zeros((0, 4, 4), dtype=getattr(torch, dtype), device="cuda"), torch.zeros(0, device="cuda"),
                                      torch.zeros(0, device="cuda"), size).cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, want) and np.array_equal(empty, want)
        return
    got, model = run_masks(ctx, masks, cls, conf, size, dtype)
    assert np.array_equal(got, model)
    if dtype == "float32":
        assert np.array_equal(got, want)            # the reference's own output


@pytest.mark.parametrize("dtype", DTYPES)
def test_masks_instance_counts(ctx, K, dtype):
    """K around the step and the round of the slices, and K = 300; more than one workgroup of pixels, an odd plane"""
    rng = np.random.default_rng(31)
    step, rnd = K["step"], K["step"] * K["slices"]
    for n in sorted({1, 2, step - 1, step, step + 1, rnd - 1, rnd, rnd + 1, 2 * rnd + 1, 300}):
        m, cls, conf = seeded_masks(rng, n, 9, 15, density=0.2 if n < 100 else 0.01)
        got, want = run_masks(ctx, m, cls, conf, (31, 23), dtype)
        assert np.array_equal(got, want), n


def test_masks_edges(ctx, K):
    rng = np.random.default_rng(37)
    rnd = K["step"] * K["slices"]
    n = rnd + K["step"] + 2
    m, cls, conf = seeded_masks(rng, n, 2, 67, density=0.3)
    cls = np.arange(n, dtype=np.float32)
    conf[:] = 0.9
    # the last instance covers everything: every wave may stop at its first step, and no lower slice may override it
    m[n - 1] = 1.0
    got, want = run_masks(ctx, m, cls, conf, (67, 98))
    assert np.array_equal(got, want) and (got == n - 1).all()
    # ... and once it is rejected, or its mask is exactly 0.5, the one below shows through - from another slice
    for k in range(n - 1, n - 1 - K["step"] - 2, -1):
        conf[k] = 0.5
        m[k - 1] = 0.75
        got, want = run_masks(ctx, m, cls, conf, (67, 98))
        assert np.array_equal(got, want) and (got == k - 1).all(), k
    m[:] = 0.5
    conf[:] = 0.9
    got, want = run_masks(ctx, m, cls, conf, (5, 98))
    assert np.array_equal(got, want) and (got == -1).all()
    # rows 2 -> 98: destination row 49 reads source row 0
    m2 = np.zeros((1, 2, 3), np.float32)
    m2[0, 1] = 1.0
    got, want = run_masks(ctx, m2, [5], [0.9], (3, 98))
    assert np.array_equal(got, want) and (got[49] == -1).all() and (got[50] == 5).all()
    # pixels-per-workgroup +-1 and an odd width, class ids beyond a byte and negative
    for hw in (K["pix_wg"] - 1, K["pix_wg"], K["pix_wg"] + 1):
        m, cls, conf = seeded_masks(rng, 7, 1, hw)
        cls[:] = [300, -5, 70000, 0, 1, 2, 65535]
        got, want = run_masks(ctx, m, cls, conf, (hw + 5, 3))
        assert np.array_equal(got, want), hw


def test_masks_write_only_the_map(ctx, gsx):
    import torch
    rng = np.random.default_rng(41)
    m, cls, conf = seeded_masks(rng, 6, 5, 7)
    tm, tc, tp = (torch.from_numpy(a).cuda() for a in (m, cls, conf))
    lib, L = gsx.lib(), gsx._lib
    for W, H in ((13, 9), (8, 5)):
        fn = lambda p: lib.gsx_segmap_from_masks(ctx.h, tm.data_ptr(), L.GSX_F32, 6, 5, 7, tc.data_ptr(), tp.data_ptr(), W, H, p)
        for maps, intact in raw_call(ctx, gsx, fn, W, H, 1):
            assert intact, "the call wrote outside its map"
            assert np.array_equal(maps[0], M.segmap_from_masks(m, cls, conf, W, H))


def test_kernels_are_the_ones_that_ran(ctx):
    import torch
    ctx.profile(True)
    ctx.segmap_from_logits(torch.zeros(3, 4, 4, device="cuda"), (8, 8))
    ctx.segmap_from_masks(torch.ones(2, 4, 4, device="cuda"), torch.zeros(2, device="cuda"), torch.ones(2, device="cuda"), (8, 8))
    ctx.synchronize()
    assert ctx.profile_get("segmap_argmax")[0] == 1 and ctx.profile_get("segmap_masks")[0] == 1 and ctx.profile_get("segmap_resize")[0] == 2
    ctx.profile(False)


# ---- chained into the vote ----------------------------------------------------------------------------------------------------------------
ASSIGN = golden_assign_cases()


@pytest.mark.parametrize("case", ASSIGN, ids=[c[0] for c in ASSIGN])
def test_vote_takes_the_device_map(ctx, gsx, case):
    """vote_view(cam, ctx.segmap_from_logits(...)) labels the scene as assign_labels_from_maps does on the model's host maps"""
    import torch
    name, positions, cams, segs, sizes, _ = case
    rng = np.random.default_rng(43)
    vols, maps = [], []
    for seg in segs:
        H, W = seg.shape
        vol = seeded_logits(rng, (12, max(1, H // 3), max(1, W // 4)), ties=False)
        vols.append(vol)
        maps.append(M.segmap_from_logits(vol, W, H))
    want = gsx.assign_labels_from_maps(positions, cams, maps, sizes, n_classes=150, ctx=ctx)
    ctx.upload_positions(positions)
    ctx.vote_begin(150, 0, max(1, len(cams)))
    for cam, vol, seg, size in zip(cams, vols, segs, sizes):
        dev = ctx.segmap_from_logits(torch.from_numpy(vol).cuda(), (seg.shape[1], seg.shape[0]))
        ctx.vote_view(cam, dev, size)
    got = ctx.vote_finalize()
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert ctx.vote_link_bytes() == 0               # no map went through the host packer
