"""lift_kernel (csrc/lift.hip) held at its structural edges, bit for bit, with the constructed maps of tests/lift_cases.py on the
scenes of tests/blend_cases.py.  test_lift_model.py shows on the CPU that the maps are what they claim and that every edge below
is reached by records with q > 0.

q = rint(w * 2^20) is formed per (pixel, record) before the map is looked at, and neither the early `continue`, the opacity vote
nor the staging depend on the map.  So for one scene and one camera the row totals of any two maps are the same integers, and
the table of a map A = f(B) is the table of B with its columns summed by f - no tolerance.  That compares the three reduction
paths (full-wave, per-class loop, per-lane LDS atomics) and every round length with each other; ONE tolerance comparison, the
fine map pos256 against the fp64 model under the bound of test_lift_gpu.py (lift_model.cell_bound, nothing new), anchors the
family: on the in-tile scenes each of its cells is a single fragment.

With cells = 2048, chunk = 256, loop_max = 4 (the tests take them from gsx.lift_constants()):
    pattern        D    classes per wave   sub   holds
    pos256         256  64 64 64 64        8     the fine map: every bin, label -1 included; the shortest round; per-lane
    wave_1         1    1 1 1 1            256   the full-wave reduction
    wave_2         2    2 2 2 2            256   the loop path
    wave_3         3    3 3 3 3            256   the loop path
    wave_4         4    4 4 4 4            256   the loop path at its last count
    wave_5         5    5 5 5 5            256   the per-lane path at its first count       (again 256 bins wide: wave_5_c255)
    mixed_waves    12   1 2 4 5            170   all three paths write one round's cells; label -1 in the uniform wave
    d_8            8    8 8 8 8            256   the last D with a whole-chunk round
    d_9            9    9 9 9 9            227   the first D with a remainder round (29 records)
    d_16           16   16 16 16 16        128   per-lane, sub a power of two
    d_100          100  64 64 64 64        20    a sub that does not divide the chunk (12 rounds of 20, one of 16)  (d_100_c255)
    d_255          255  64 64 64 64        8     sub = cells // 255
    d9_loop        9    2 2 2 3            227   a remainder round with every wave on the loop path
    word_edges     16   16 16 16 16        128   rank256 at the word boundaries: bins 0 31 32 33 63 64 95 96 127 128 159 160 ..
    halves / c255  1 .. 21 by tile / 121   -     not periodic in the tiles: D differs between neighbours, on both sides of 8
On frames the border cuts, the cut tiles hold fewer classes and waves with pixels on both sides of the border.

Measured on an MI355X.  The anchor, worst |table / 2^20 - model| over the cells of pos256 as a multiple of the cell's bound:
    lengths            0.127     edges (ten frames)  0.320 (17x17) .. 0.509 (47x47)
    needles            0.378     epilogue_1, _3      0.261, 0.233
    walls_80x48        0.027     epilogue_3_opaque   0.034
    walls_65x53        0.025
- the distances of the 255-class map in test_lift_gpu.py, as they should be: both maps put single pixels into their cells.
Every exact comparison holds on all 17 scenes.  The slowest test is test_finalize_thresholds_past_two_to_the_24, 1.4 s (4657
views of walls_80x48, 1.3 s); lifting the 23 maps of a scene and its fp64 model take 0.6 s at the most, the whole file 5.4 s.

What the exact tests see that the tolerance does not, tried with two deliberately wrong builds of lift_kernel: a loop path that
skips its last class when a wave holds exactly loop_max fails the coarsening and the row totals on every scene (the six general
maps notice it on the five frames with W % 16 = 1 only, whose cut tiles happen to leave four pixels of a wave inside); a
remainder round that does not flush its last record fails 49 of the 59 tests here.

Also here: labels at the extremes of int32 / int64 / uint8 through host and device maps (2^32 - 1 and 2^32 read as -1 and 0 if
narrowed to 32 bits before the range test; 2^63 - 1 must not be incremented), and gsx_lift_finalize on rows past 2^44.
"""
import time

import numpy as np
import pytest

import blend_cases
import lift_cases
import lift_model
from lift_model import ONE

pytestmark = pytest.mark.gpu

NAMES = list(blend_cases.all_cases())
GENERAL = ("uniform", "none", "checker", "blocks", "offset8")            # lift_model.maps; its sixth, c255, is the pair's fine map
_LIFTED = {}


def the_maps(gsx, W, H):
    """key -> (map, n_classes): every pattern, the non-periodic pair, the general maps of lift_model.maps"""
    out = {name: (p.map(W, H), p.n_classes) for name, p in lift_cases.patterns(gsx.lift_constants()).items()}
    out["c255"], out["halves"], _ = lift_cases.halves_pair(W, H)
    general = lift_model.maps(W, H)
    assert np.array_equal(general["c255"][0], out["c255"][0])
    out.update({key: general[key] for key in GENERAL})
    return out


def lift_once(c, sc, seg, C):
    c.lift_begin(C)
    c.lift_view(sc.cam, seg)
    assert c.lift_num_views() == 1
    return c.lift_table()


def lifted(gsx, name):
    """every map of the_maps lifted on one case in ONE fresh context: key -> (uint64 table, pairs consumed, global atomics)"""
    if name not in _LIFTED:
        sc = blend_cases.prepared(name).scene
        out = {}
        with gsx.Context(0) as c:
            c.upload_splats(*sc.arrays())
            for key, (seg, C) in the_maps(gsx, sc.W, sc.H).items():
                table = lift_once(c, sc, seg, C)
                assert table.dtype == np.uint64 and table.shape == (len(sc.xyz), C + 1)
                table.setflags(write=False)
                out[key] = (table, c.render_num_pairs_consumed(), c.lift_num_atomics())
        _LIFTED[name] = out
    return _LIFTED[name]


def first_difference(got, want):
    """None, or "n cells differ, first (row, bin, got, want)" """
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    diff = got != want
    if not diff.any():
        return None
    r, b = (int(v) for v in np.argwhere(diff)[0])
    return f"{int(diff.sum())} cells differ, first (row {r}, bin {b}, got {int(got[r, b])}, want {int(want[r, b])})"


# ---- the anchor: the fine map against the fp64 model ---------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fine_map_against_the_model(gsx, name):
    p = blend_cases.prepared(name)
    m = p.model
    seg, C = the_maps(gsx, m.W, m.H)["pos256"]
    L = lift_model.lift(m, seg, C)
    got = lifted(gsx, name)["pos256"][0]
    want = L.upload_rows(L.table)
    bound = L.upload_rows(lift_model.cell_bound(L, p.tol, p.alpha_max, blend_cases.bitwise(name)))
    dist = np.abs(got.astype(np.float64) / ONE - want)
    fed = bound > 0
    worst = float((dist[fed] / bound[fed]).max())
    print(f"{name}: pos256, worst |table / 2^20 - model| as a multiple of its bound: {worst:.3f} over {int(fed.sum())} cells, "
          f"{int((got > 0).sum())} of them hold weight")
    assert (got[~fed] == 0).all() and fed.sum() > 100 and (got > 0).sum() > 100
    assert (dist <= bound).all(), worst


# ---- exact: coarsening, row totals, atomics ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_coarse_tables_are_the_fine_table_summed(gsx, name):
    T = lifted(gsx, name)
    fine = T["pos256"][0]
    assert fine.sum(dtype=np.uint64) > ONE
    wrong = {}
    for key, p in lift_cases.patterns(gsx.lift_constants()).items():
        wrong[key] = first_difference(T[key][0], lift_cases.coarsen(fine, p.f, p.n_classes + 1))
    wrong["halves"] = first_difference(T["halves"][0], lift_cases.coarsen(T["c255"][0], lift_cases.halves_f(), lift_cases.HALVES_N + 1))
    wrong = {k: v for k, v in wrong.items() if v}
    assert not wrong, wrong


@pytest.mark.parametrize("name", NAMES)
def test_row_totals_and_pairs_do_not_depend_on_the_map(gsx, name):
    T = lifted(gsx, name)
    totals, consumed = T["pos256"][0].sum(1, dtype=np.uint64), T["pos256"][1]
    assert totals.dtype == np.uint64 and consumed > 0 and len(T) == len(lift_cases.patterns(gsx.lift_constants())) + 2 + len(GENERAL)
    wrong = {}
    for key, (table, pairs, _) in T.items():
        t = table.sum(1, dtype=np.uint64)
        if not np.array_equal(t, totals):
            r = int(np.flatnonzero(t != totals)[0])
            wrong[key] = f"{int((t != totals).sum())} rows differ, first (row {r}, got {int(t[r])}, want {int(totals[r])})"
        elif pairs != consumed:
            wrong[key] = f"{pairs} pairs consumed, pos256 {consumed}"
    assert not wrong, wrong


def test_one_atomic_per_record_and_class(gsx):
    """lengths: every record lies inside one tile, so a (record, class) cell is one round's cell of one tile - one global atomic
    where the sum is not zero, none where it is"""
    T = lifted(gsx, "lengths")
    wrong = {key: (atomics, int(np.count_nonzero(table))) for key, (table, _, atomics) in T.items() if atomics != np.count_nonzero(table)}
    assert not wrong, wrong
    assert T["pos256"][2] > T["wave_2"][2] > T["wave_1"][2] == T["uniform"][2] > 0
    assert T["pos256"][1] == sum(blend_cases.LENGTHS)


@pytest.mark.parametrize("name", ["lengths", "walls_65x53", "edges_47x47"])
def test_views_of_different_round_lengths_add(gsx, name):
    K = gsx.lift_constants()
    R, Lm = lift_cases.units(K)
    sc = blend_cases.prepared(name).scene
    keys = (f"d_{R + 1}", f"wave_{Lm + 1}", "pos256")
    maps = the_maps(gsx, sc.W, sc.H)
    want = sum(lift_cases.widen(lifted(gsx, name)[key][0], 256) for key in keys)
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays())
        c.lift_begin(255)
        for key in keys:
            c.lift_view(sc.cam, maps[key][0])
        assert c.lift_num_views() == 3
        wrong = first_difference(c.lift_table(), want)
    assert wrong is None, wrong


def test_a_fresh_context_repeats_the_tables(gsx):
    sc = blend_cases.prepared("needles").scene
    assert blend_cases.bitwise("needles")
    maps = the_maps(gsx, sc.W, sc.H)
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays())
        for key in ("d_100", "mixed_waves"):
            wrong = first_difference(lift_once(c, sc, *maps[key]), lifted(gsx, "needles")[key][0])
            assert wrong is None, (key, wrong)


# ---- the label range at the integer extremes -----------------------------------------------------------------------------
def extreme_maps(W, H):
    """(what, clean map, n_classes, packed_u8, bad value): one pixel (row 9, column 4) of the clean map will hold the value.
    2^32 - 1 and 2^32 read as -1 and 0 once narrowed to 32 bits; 2^63 - 1 + 1 leaves 64 bits."""
    r, x = np.mgrid[0:H, 0:W]
    clean = ((r // 3 + x) % 5 - 1).astype(np.int64)
    out = [("int64", clean, 4, False, v) for v in (2 ** 32 - 1, 2 ** 32, -2 ** 32, 2 ** 63 - 1, -2 ** 63, -2)]
    out += [("int32", clean.astype(np.int32), 4, False, v) for v in (2 ** 31 - 1, -2 ** 31)]
    out.append(("uint8 labels", ((r + x) % 255).astype(np.uint8), 255, False, 255))
    out.append(("uint8 packed", ((r + x) % 255).astype(np.uint8), 254, True, 255))
    return out


def test_host_maps_at_the_integer_extremes_fail_before_the_view_counts(gsx):
    sc = blend_cases.prepared("edges_17x17").scene
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays())
        for what, clean, C, packed, value in extreme_maps(sc.W, sc.H):
            c.lift_begin(C)
            c.lift_view(sc.cam, clean, packed_u8=packed)
            before = c.lift_table()
            assert before.sum(dtype=np.uint64) > ONE
            bad = clean.copy()
            bad[9, 4] = value
            assert int(bad[9, 4]) == value and bad.dtype == clean.dtype
            with pytest.raises(ValueError, match="view 1: the label at row 9, column 4 "):
                c.lift_view(sc.cam, bad, packed_u8=packed)
            assert c.lift_num_views() == 1 and np.array_equal(c.lift_table(), before), (what, value)
            c.lift_begin(C)                                              # a following clean run
            c.lift_view(sc.cam, clean, packed_u8=packed)
            assert np.array_equal(c.lift_table(), before), (what, value)


def test_device_maps_at_the_integer_extremes_fail_naming_the_view(gsx):
    import torch
    sc = blend_cases.prepared("edges_17x17").scene
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays())
        for what, clean, C, packed, value in extreme_maps(sc.W, sc.H):
            bad = clean.copy()
            bad[9, 4] = value
            d_clean, d_bad = torch.from_numpy(clean).to("cuda:0"), torch.from_numpy(bad).to("cuda:0")
            assert int(d_bad[9, 4]) == value
            c.lift_begin(C)
            c.lift_view(sc.cam, clean, packed_u8=packed)
            before = c.lift_table()
            c.lift_begin(C)
            c.lift_view(sc.cam, d_clean, packed_u8=packed)
            assert np.array_equal(c.lift_table(), before), (what, value)
            c.lift_view(sc.cam, d_bad, packed_u8=packed)
            c.lift_view(sc.cam, d_clean, packed_u8=packed)
            with pytest.raises(ValueError, match="view 1 held"):
                c.lift_table()
            with pytest.raises(ValueError, match="view 1 held"):
                c.lift_finalize()
            c.lift_begin(C)                                              # a following clean run
            c.lift_view(sc.cam, d_clean, packed_u8=packed)
            assert np.array_equal(c.lift_table(), before), (what, value)
            c.lift_finalize()


# ---- lift_finalize at large totals and thresholds ------------------------------------------------------------------------
def test_finalize_thresholds_past_two_to_the_24(gsx):
    """rows whose weight passes 2^24 (2^44 in the table's units), where anything narrowed to fp32 on the way loses the last
    unit: the threshold just below and just above 2^44 / ONE, at a row's own total and one unit to either side, and saturated"""
    import torch
    sc = blend_cases.prepared("walls_80x48").scene
    single = lifted(gsx, "walls_80x48")["wave_1"][0]
    top = int(single.sum(1, dtype=np.uint64).max())
    views = 2 ** 44 // top + 1
    assert views < 8192, views
    seg = torch.from_numpy(the_maps(gsx, sc.W, sc.H)["wave_1"][0]).to("cuda:0")
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays())
        c.lift_begin(1)
        t0 = time.perf_counter()
        for _ in range(views):
            c.lift_view(sc.cam, seg)
        print(f"walls_80x48: {views} views of a row total of {top / ONE:.1f} in {time.perf_counter() - t0:.2f} s")
        table = c.lift_table()
        assert first_difference(table, single * np.uint64(views)) is None
        totals = [int(v) for v in table.sum(1, dtype=np.uint64)]
        r = int(np.argmax(totals))
        T = totals[r]
        assert 2 ** 44 <= T < 2 ** 45 and sum(t >= 2 ** 44 for t in totals) < sum(t > 0 for t in totals)
        below, above = float(np.nextafter(2.0 ** 24, 0.0)), float(np.nextafter(2.0 ** 24, np.inf))
        assert lift_model.threshold(below) == 2 ** 44 and lift_model.threshold(above) == 2 ** 44 + 1
        for mw in (below, 2.0 ** 24, above, (T - 1) / ONE, T / ONE, (T + 1) / ONE, 1e300):
            labels, share = c.lift_finalize(mw, return_share=True)
            want_l, want_s = lift_model.finalize(table, mw)
            assert np.array_equal(labels, want_l) and np.array_equal(share, want_s), mw
        assert (T - 1) / ONE < T / ONE < (T + 1) / ONE                   # exact in fp64; fp32 would merge them
        assert c.lift_finalize(T / ONE)[r] == 0 and c.lift_finalize((T + 1) / ONE)[r] == -1
        assert c.lift_finalize(below)[r] == 0 and (c.lift_finalize(1e300) == -1).all()
