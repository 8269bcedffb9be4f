"""GPU: the IoU evaluation (csrc/iou.hip) against the reference-made fixture (tests/golden/iou.npz) and the numpy model
(tests/iou_model.py), and its kernels at the edges of the units they are built on.  Every comparison is exact: integers with
np.array_equal, doubles by bit pattern with NaNs in the same places."""
import ctypes as C
import importlib.util
import os
import random
import re

import numpy as np
import pytest

import iou_model as M
from conftest import ROOT
from iou_cases import copies, fixture, mask_cases, same_doubles

pytestmark = pytest.mark.gpu

CASES = mask_cases()


@pytest.fixture(scope="module")
def K(gsx):
    """the units the kernels are built on, exported from the source (gsx_debug_iou_constants)"""
    return gsx.iou_constants()


@pytest.fixture(scope="module")
def ev():
    """the drop-in front-end at the reference's own path"""
    spec = importlib.util.spec_from_file_location("gsx_evaluation", os.path.join(ROOT, "Image_Segmentation", "evaluation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def check_counts(got, masks, gts):
    """(iou, inter, area_masks, area_gt) of Context.iou_masks against the model"""
    iou, inter, am, ag = got
    wi, wm, wg = M.inter_area(masks, gts)
    assert inter.dtype == np.int64 and np.array_equal(inter, wi)
    assert np.array_equal(am, wm) and np.array_equal(ag, wg)
    assert same_doubles(iou, M.iou_from_counts(wi, wm[:, None], wg[None, :]))


# ---- 1. the fixture ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fixture_case(ctx, ev, case):
    import torch
    name, masks, gts, iou, best_iou, best_gt = case
    before = copies(masks) + copies(gts)
    got = ctx.iou_masks(masks, gts)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, masks + gts))   # inputs are not written
    assert same_doubles(got[0], iou)
    check_counts(got, masks, gts)
    best = ctx.best_ious(masks, gts)
    assert [int(b[1]) for b in best] == best_gt.tolist() and same_doubles([float(b[0]) for b in best], best_iou)
    assert all(type(b[0]) is int for b in best if b[0] == 0)           # the reference's untouched `max_iou = 0`
    # device tensors give the same numbers
    dev = ctx.iou_masks([torch.from_numpy(m).cuda() for m in masks], [torch.from_numpy(g).cuda() for g in gts])
    assert same_doubles(dev[0], iou) and np.array_equal(dev[1], got[1])
    assert np.array_equal(ctx.masks_top_index(masks + gts), M.top_index(masks + gts))
    # the front-end's functions, on copies: they edit their arguments as the reference's do
    fm, fg = copies(masks), copies(gts)
    fb = ev.get_ious_from_masks(fm, fg, ctx=ctx)
    assert [int(b[1]) for b in fb] == best_gt.tolist() and same_doubles([float(b[0]) for b in fb], best_iou)
    for a, b in zip(fm + fg, masks + gts):
        assert np.array_equal(a, (b != 0).astype(b.dtype))
    for i, m in enumerate(masks):
        for j, g in enumerate(gts):
            assert same_doubles([ev.IoU(np.array(m), np.array(g), ctx=ctx)], [iou[i, j]])


def test_fixture_front_end_example_and_segmentation_map(ctx, ev):
    z = fixture()
    a, b = np.array(ev.img1), np.array(ev.img2)
    assert np.array_equal(a, z["example/mask0"]) and np.array_equal(b, z["example/gt0"])
    v = ev.IoU(a, b, ctx=ctx)
    assert isinstance(v, np.float64) and v == 4 / 14
    assert np.array_equal(a, z["example/after1"]) and np.array_equal(b, z["example/after2"])      # the in-place side effect
    ro = np.array(ev.img1)
    ro.flags.writeable = False
    assert ev.IoU(ro, b, ctx=ctx) == 4 / 14
    masks = [z[f"segmap/mask{i}"] for i in range(int(z["segmap/n_masks"]))]
    random.seed(int(z["segmap/seed"]))
    img = ev.generate_segmentation_map(copies(masks), ctx=ctx)
    want = z["segmap/map"]
    assert img.dtype == want.dtype and img.shape == want.shape and np.array_equal(img.view(np.int64), want.view(np.int64))
    random.seed(int(z["segmap/seed"]))
    cols = [[random.random(), random.random(), random.random()] for _ in masks]
    assert np.array_equal(ev.generate_segmentation_map(masks, colors=cols, ctx=ctx), want)
    assert ev.get_ious_from_masks([], masks, ctx=ctx) == [] and ev.get_ious_from_masks(masks[:2], [], ctx=ctx) == [(0, 0), (0, 0)]


def labelme_pairs():
    z = fixture()
    yield "0001_2_vs_0001_3", z["labelme/0001_2"], z["labelme/0001_3"], z["labelme/0001_2_vs_0001_3/iou"]
    for n in ("DSCF4667", "street"):
        yield f"{n}_shift3", z[f"labelme/{n}"], np.roll(z[f"labelme/{n}"], 3, axis=1), z[f"labelme/{n}_shift3/iou"]


@pytest.mark.parametrize("pair", list(labelme_pairs()), ids=[p[0] for p in labelme_pairs()])
def test_fixture_labelme_maps(ctx, gsx, pair):
    """the reference's own ground truth as label maps: through the table and through indicator masks"""
    import torch
    name, a, b, iou = pair
    ka, kb = iou.shape
    want = M.table(a, b, ka, kb)
    for lds in (1, 0):
        ctx.set_option("iou_table_lds", lds)
        t = ctx.label_map_tables([a], [b], ka, kb)
        assert t.dtype == np.int64 and t.shape == (1, ka + 1, kb + 1) and np.array_equal(t[0], want)
        td = ctx.label_map_tables([torch.from_numpy(a).cuda()], [torch.from_numpy(b).cuda().long()], ka, kb)
        assert np.array_equal(td[0], want)
    ctx.set_option("iou_table_lds", 1)
    assert same_doubles(gsx.iou_from_table(t[0])[1:, 1:], iou)
    ma, mb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    got = ctx.iou_masks([ma == i for i in range(ka)], [mb == j for j in range(kb)])
    assert same_doubles(got[0], iou) and np.array_equal(got[1], want[1:, 1:])
    if name == "0001_2_vs_0001_3":
        z = fixture()
        best = ctx.best_ious([ma == i for i in range(ka)], [mb == j for j in range(kb)])
        assert [int(x[1]) for x in best] == z[f"labelme/{name}/best_gt"].tolist()
        assert same_doubles([float(x[0]) for x in best], z[f"labelme/{name}/best_iou"])


# ---- 2. the pack kernel ---------------------------------------------------------------------------------------------------------------
EDGE_VALUES = {
    "bool": [False, True],
    "uint8": [0, 1, 255, 128],
    "int32": [0, 256, -1, 65536, -2 ** 31],
    "int64": [0, 2 ** 32, -1, 2 ** 40, -2 ** 63],
    "float32": [0.0, np.nan, -0.0, np.inf, 1e-45, -1.5, -np.inf, -1e-45],
    "float64": [0.0, np.nan, -0.0, np.inf, 5e-324, 2.0, -np.inf, -5e-324],
}


def pack_masks(dtype, h, w, rng):
    """edge-value noise, all ones, one set pixel at the first / at the last position, all zero"""
    vals = np.array(EDGE_VALUES[dtype], dtype=dtype)
    noise = vals[rng.integers(0, len(vals), (h, w))]
    first, last = np.zeros((h, w), dtype), np.zeros((h, w), dtype)
    first.flat[0] = vals[1]
    last.flat[-1] = vals[-1]
    return [noise, np.ones((h, w), dtype), first, last, np.zeros((h, w), dtype)]


def pack_sizes(K, itemsize):
    out = []
    for unit in (K["load_bytes"] // itemsize, K["word_bits"], K["wave_tile"], K["block_tile"]):
        out += [unit - 1, unit, unit + 1]
    return sorted({n for n in out if n >= 1})


@pytest.mark.parametrize("dtype", list(EDGE_VALUES))
def test_pack_kernel_edges(ctx, K, dtype):
    import torch
    rng = np.random.default_rng(11)
    itemsize = np.dtype(dtype).itemsize
    assert (K["load_bytes"], K["word_bits"]) == (16, 64) and K["block_tile"] % K["wave_tile"] == 0
    shapes = [(1, n) for n in pack_sizes(K, itemsize)] + [(1, 1), (1, 65), (65, 1), (415, 612), (1038, 1557)]
    for h, w in shapes:
        masks = pack_masks(dtype, h, w, rng)
        gts = [masks[0][::-1, ::-1].copy(), masks[1]]
        got = ctx.iou_masks(masks, gts)
        check_counts(got, masks, gts)
        assert got[2][1] == h * w and got[1][1, 1] == h * w          # all ones: the padding bits of the last word are zero
        assert got[2][2] == 1 and got[2][3] == 1 and got[2][4] == 0
        # the device path: identical counts, also from views that start 1, 3 and 7 elements into a buffer
        for off in (0, 1, 3, 7):
            dm = []
            for m in masks + gts:
                buf = torch.zeros(h * w + 8, dtype=torch.from_numpy(m).dtype, device="cuda")
                buf[off:off + h * w] = torch.from_numpy(m).cuda().reshape(-1)
                dm.append(buf[off:off + h * w].view(h, w))
                assert dm[-1].data_ptr() % itemsize == 0 and (off == 0) == (dm[-1].data_ptr() % 16 == 0)
            dev = ctx.iou_masks(dm[:len(masks)], dm[len(masks):])
            for x, y in zip(dev[1:], got[1:]):
                assert np.array_equal(x, y), (dtype, h, w, off)
            assert same_doubles(dev[0], got[0])
            if (h, w) in ((415, 612), (1038, 1557)) and off >= 1:
                break                                                 # one unaligned view of the large frames is enough


# ---- 3. the pair kernel ---------------------------------------------------------------------------------------------------------------
def test_pair_kernel_tile_edges(ctx, K):
    rng = np.random.default_rng(12)
    T = K["pair_tile"]
    h, w = 7, 19
    pool = [rng.random((h, w)) < d for d in rng.random(2 * T + 1)]
    pool_g = [rng.random((h, w)) < d for d in rng.random(2 * T + 1)]
    for nm in (1, T - 1, T, T + 1, 2 * T + 1):
        for ng in (1, T - 1, T, T + 1, 2 * T + 1):
            check_counts(ctx.iou_masks(pool[:nm], pool_g[:ng]), pool[:nm], pool_g[:ng])
    wide = [rng.random((h, w)) < 0.5 for _ in range(40)]
    check_counts(ctx.iou_masks(pool[:1], wide), pool[:1], wide)
    check_counts(ctx.iou_masks(wide, pool_g[:1]), wide, pool_g[:1])


def test_pair_kernel_slice_edges(ctx, K):
    rng = np.random.default_rng(13)
    S = K["pair_chunk_words"]                                        # small problems: a slice is exactly one chunk
    for words in (1, S - 1, S, S + 1, 5 * S + 3):
        for npix in (words * 64, words * 64 - 5):
            masks = [rng.random((1, npix)) < 0.5 for _ in range(3)] + [np.ones((1, npix), bool)]
            gts = [rng.random((1, npix)) < 0.5, np.ones((1, npix), bool)]
            got = ctx.iou_masks(masks, gts)
            check_counts(got, masks, gts)
            assert got[1][3, 1] == npix


def test_pair_kernel_loses_no_slice_at_1080p(ctx, K):
    """all-ones masks, 17 x 17 of them (four tiles, so slices of several chunks): EVERY entry is 1920 * 1080"""
    import torch
    T = K["pair_tile"]
    ones = torch.ones((2 * (T + 1), 1080, 1920), dtype=torch.uint8, device="cuda")
    iou, inter, am, ag = ctx.iou_masks(ones[:T + 1], ones[T + 1:])
    assert inter.shape == (T + 1, T + 1) and (inter == 2073600).all() and (am == 2073600).all() and (ag == 2073600).all()
    assert (iou == 1.0).all()
    iou, inter, am, ag = ctx.iou_masks(ones[:1], ones[1:2])           # 1 x 1: one tile, as many slices as there are chunks
    assert inter.tolist() == [[2073600]] and am.tolist() == [2073600]


def test_pair_kernel_densities_and_a_smaller_second_call(ctx):
    rng = np.random.default_rng(14)
    h, w = 415, 612
    for d in (0.01, 0.5, 0.99):
        masks = [rng.random((h, w)) < d for _ in range(5)]
        gts = [rng.random((h, w)) < d for _ in range(3)]
        check_counts(ctx.iou_masks(masks, gts), masks, gts)
    # fewer masks, fewer pixels on the same context: stale planes or counters of the call before would show
    masks = [rng.random((37, 53)) < 0.5 for _ in range(2)]
    gts = [rng.random((37, 53)) < 0.5]
    check_counts(ctx.iou_masks(masks, gts), masks, gts)
    check_counts(ctx.iou_masks(np.stack(masks), np.stack(gts)), masks, gts)       # one 3-D array each


# ---- 4. the table kernel --------------------------------------------------------------------------------------------------------------
def table_maps(h, w, n, rng, kind):
    if kind == "uniform":
        return np.full((h, w), n - 1, np.int32)
    if kind == "stripes":
        return np.broadcast_to((np.arange(w) % (n + 1) - 1).astype(np.int32), (h, w)).copy()
    if kind == "noise":
        return rng.integers(-1, n, (h, w)).astype(np.int32)
    return np.full((h, w), -1, np.int32)


def check_tables(ctx, preds, gts, P, G, packed_u8=False):
    want = np.stack([M.table(a, b, P, G, packed_u8=packed_u8) for a, b in zip(preds, gts)])
    out = []
    for lds in (1, 0):
        ctx.set_option("iou_table_lds", lds)
        out.append(ctx.label_map_tables(preds, gts, P, G, packed_u8=packed_u8))
    ctx.set_option("iou_table_lds", 1)
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], want)
    off = 0 if packed_u8 else 1
    for t, a, b in zip(out[0], preds, gts):                            # row and column sums are the maps' own histograms
        assert np.array_equal(t.sum(1), np.bincount(np.asarray(a).astype(np.int64).ravel() + off, minlength=P + 1))
        assert np.array_equal(t.sum(0), np.bincount(np.asarray(b).astype(np.int64).ravel() + off, minlength=G + 1))
    return out[0]


def table_class_counts(K):
    L = K["table_lds_max"]

    def split(n):
        return [(a - 1, n // a - 1) for a in range(2, 257) if n % a == 0 and n // a <= 256][0]
    return [(1, 1), (2, 3), (150, 150), (255, 255), split(L - 1), split(L), split(L + 1)]


@pytest.mark.parametrize("which", range(7))
def test_table_kernel_edges(ctx, K, which):
    P, G = table_class_counts(K)[which]
    if which >= 4:
        assert (P + 1) * (G + 1) == K["table_lds_max"] + which - 5 and 1 <= P <= 255 and 1 <= G <= 255
    rng = np.random.default_rng(20 + which)
    h, w = 33, 47                                                    # 1551 pixels: no multiple of a lane's run, of a wave, of a workgroup
    for kp, kg in (("uniform", "uniform"), ("stripes", "stripes"), ("noise", "noise"), ("minus", "minus"), ("uniform", "noise"),
                   ("stripes", "uniform")):
        check_tables(ctx, [table_maps(h, w, P, rng, kp)], [table_maps(h, w, G, rng, kg)], P, G)
    preds = [table_maps(h, w, P, rng, k) for k in ("noise", "uniform", "stripes", "minus", "noise")]
    gts = [table_maps(h, w, G, rng, k) for k in ("noise", "noise", "uniform", "stripes", "minus")]
    check_tables(ctx, preds, gts, P, G)                              # n_pairs = 5
    big = check_tables(ctx, [table_maps(415, 612, P, rng, "noise")], [table_maps(415, 612, G, rng, "noise")], P, G)
    assert big.sum() == 415 * 612


def test_table_kernel_dtypes_host_and_device(ctx):
    import torch
    rng = np.random.default_rng(30)
    P, G, h, w = 5, 7, 29, 31
    a, b = rng.integers(-1, P, (h, w)), rng.integers(-1, G, (h, w))
    want = M.table(a, b, P, G)
    forms = lambda x: [(x.astype(np.int32), False), (x.astype(np.int64), False), ((x + 1).astype(np.uint8), True)]
    for fa, pa in forms(a):
        for fb, pb in forms(b):
            packed = pa or pb                                        # it only concerns the uint8 maps of a call
            for la, lb in (([fa], [fb]), ([torch.from_numpy(fa).cuda()], [torch.from_numpy(fb).cuda()])):
                assert np.array_equal(ctx.label_map_tables(la, lb, P, G, packed_u8=packed)[0], want), (fa.dtype, fb.dtype)
    # uint8 holding the label itself: it cannot express -1
    a8, b8 = np.maximum(a, 0).astype(np.uint8), np.maximum(b, 0).astype(np.uint8)
    assert np.array_equal(check_tables(ctx, [a8], [b8], P, G)[0], M.table(a8, b8, P, G))
    # views that start 1, 3 and 7 elements into a device buffer
    for off in (1, 3, 7):
        bufa = torch.zeros(h * w + 8, dtype=torch.int32, device="cuda")
        bufb = torch.zeros(h * w + 8, dtype=torch.int64, device="cuda")
        bufa[off:off + h * w] = torch.from_numpy(a.astype(np.int32)).cuda().reshape(-1)
        bufb[off:off + h * w] = torch.from_numpy(b.astype(np.int64)).cuda().reshape(-1)
        t = ctx.label_map_tables([bufa[off:off + h * w].view(h, w)], [bufb[off:off + h * w].view(h, w)], P, G)
        assert np.array_equal(t[0], want)


def test_table_kernel_range_errors(ctx):
    rng = np.random.default_rng(31)
    P, G, h, w = 4, 6, 21, 37
    good = [rng.integers(-1, P, (h, w)).astype(np.int32) for _ in range(3)]
    gts = [rng.integers(-1, G, (h, w)).astype(np.int32) for _ in range(3)]
    for lds in (1, 0):
        ctx.set_option("iou_table_lds", lds)
        for bad_value, in_gt in ((P, False), (-2, False), (G, True), (-2, True), (2 ** 31 - 1, False)):
            preds, g2 = copies(good), copies(gts)
            tgt = g2 if in_gt else preds
            tgt[1].flat[500] = bad_value
            tgt[1].flat[123] = bad_value
            tgt[2].flat[7] = bad_value
            with pytest.raises(ValueError) as e:
                ctx.label_map_tables(preds, g2, P, G)
            msg = str(e.value)
            assert re.search(r"pair 1\b", msg) and re.search(r"index 123\b", msg), msg
            assert np.array_equal(ctx.label_map_tables(good, gts, P, G)[1], M.table(good[1], gts[1], P, G))   # the ctx goes on
    ctx.set_option("iou_table_lds", 1)
    u8 = np.full((h, w), P + 1, np.uint8)                             # packed: bin P + 1 does not exist
    with pytest.raises(ValueError):
        ctx.label_map_tables([u8], [np.zeros((h, w), np.uint8)], P, G, packed_u8=True)


# ---- 5. argument errors -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_context_usable(ctx, gsx):
    L, lib = ctx._lib, gsx._lib
    m = np.ones((4, 5), np.uint8)
    one = (C.c_void_p * 1)(m.ctypes.data)
    null = (C.c_void_p * 1)(None)
    out = np.zeros(1, np.int64)
    d = np.zeros(1, np.float64)
    o = (out.ctypes.data, out.ctypes.data, out.ctypes.data, d.ctypes.data)
    U8 = lib.GSX_MASK_U8
    bad = [(1, None, U8, 1, one, U8, 4, 5), (1, one, U8, 1, None, U8, 4, 5), (1, null, U8, 1, one, U8, 4, 5), (1, one, U8, 1, null, U8, 4, 5),
           (0, one, U8, 1, one, U8, 4, 5), (1, one, U8, -1, one, U8, 4, 5), (1, one, U8, 1, one, U8, 0, 5), (1, one, U8, 1, one, U8, 4, -5),
           (1, one, 5, 1, one, U8, 4, 5), (1, one, U8, 1, one, -1, 4, 5)]
    for args in bad:
        for fn in (L.gsx_iou_masks, L.gsx_iou_masks_device):
            assert fn(ctx.h, *args, *o) == lib.GSX_E_INVALID, args
    assert L.gsx_iou_masks(None, 1, one, U8, 1, one, U8, 4, 5, *o) == lib.GSX_E_INVALID
    assert L.gsx_iou_masks(ctx.h, 1, one, U8, 1, one, U8, 65536, 65536, *o) == lib.GSX_E_UNSUPPORTED
    assert L.gsx_iou_masks(ctx.h, 65536, one, U8, 1, one, U8, 4, 5, *o) == lib.GSX_E_UNSUPPORTED
    odd = (C.c_void_p * 1)(0x7f0000000002)                                # not aligned to a 4-byte element: refused, never read
    assert L.gsx_iou_masks_device(ctx.h, 1, odd, lib.GSX_MASK_I32, 1, odd, lib.GSX_MASK_I32, 4, 5, *o) == lib.GSX_E_INVALID
    I32 = lib.GSX_SEG_I32
    tab = np.zeros(9, np.int64)
    for args in ((1, None, I32, 2, one, I32, 2, 4, 5, tab.ctypes.data), (1, one, I32, 2, one, I32, 2, 4, 5, None), (0, one, I32, 2, one, I32, 2, 4, 5, tab.ctypes.data),
                 (1, one, I32, 0, one, I32, 2, 4, 5, tab.ctypes.data), (1, one, I32, 2, one, I32, 256, 4, 5, tab.ctypes.data),
                 (1, one, 9, 2, one, I32, 2, 4, 5, tab.ctypes.data), (1, one, I32, 2, one, I32, 2, 4, 0, tab.ctypes.data), (1, one, I32, 2, null, I32, 2, 4, 5, tab.ctypes.data)):
        for fn in (L.gsx_iou_label_maps, L.gsx_iou_label_maps_device):
            assert fn(ctx.h, *args) == lib.GSX_E_INVALID, args
    idx = np.zeros(20, np.int32)
    for args in ((1, None, U8, 4, 5, idx.ctypes.data), (1, one, U8, 4, 5, None), (0, one, U8, 4, 5, idx.ctypes.data), (1, one, U8, 0, 5, idx.ctypes.data),
                 (1, one, 7, 4, 5, idx.ctypes.data), (1, null, U8, 4, 5, idx.ctypes.data)):
        assert L.gsx_masks_top_index(ctx.h, *args) == lib.GSX_E_INVALID, args
    # the wrapper: mismatched shapes, empty lists, unequal pair counts
    with pytest.raises(ValueError):
        ctx.iou_masks([m], [np.ones((5, 4), np.uint8)])
    with pytest.raises(ValueError):
        ctx.iou_masks([m, np.ones((4, 6), np.uint8)], [m])
    with pytest.raises(ValueError):
        ctx.iou_masks([], [m])
    with pytest.raises(ValueError):
        ctx.label_map_tables([m, m], [m], 3, 3)
    with pytest.raises(ValueError):
        ctx.label_map_tables([m], [m], 0, 3)
    with pytest.raises(ValueError):
        ctx.masks_top_index([m, np.ones((2, 2), np.uint8)])
    # ... and the context is as good as before
    iou, inter, am, ag = ctx.iou_masks([m], [m])
    assert iou.tolist() == [[1.0]] and inter.tolist() == [[20]] and am.tolist() == [20] and ag.tolist() == [20]
    assert np.array_equal(ctx.masks_top_index([m, np.zeros((4, 5))]), np.zeros((4, 5), np.int32))
    names = set(ctx.profile_names())
    ctx.profile(True)
    ctx.iou_masks([m], [m])
    ctx.label_map_tables([m], [m], 3, 3)
    ctx.masks_top_index([m])
    ctx.synchronize()
    for k in ("iou_pack", "iou_pairs", "iou_table", "iou_top_index"):
        assert ctx.profile_get(k)[0] >= 1, (k, names)
    ctx.profile(False)
