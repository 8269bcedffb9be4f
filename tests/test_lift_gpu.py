"""The lifting labeler (csrc/lift.hip, include/gsx.h: gsx_lift_*) against the fp64 model of tests/lift_model.py on the scenes of
tests/blend_cases.py, under six maps: one class, all -1, a 1-pixel checker (every wave mixed), 16x16 blocks on the tiles,
blocks offset by 8 (a wave uniform, its tile not) and 255 classes in every tile.  test_lift_model.py shows on the CPU that the
model is what it claims and that removing ANY single record moves a cell by more than ten of the tolerances used here.

Tolerance per cell: |table / 2^20 - model| <= P (tol + 2^-21) + M alpha_max e^-4, plus P 1e-5 where tiles reach the opacity cut.
P = (pixel, fragment) pairs that fed the cell, tol = the scene's frame tolerance (blend_cases.Prepared.tol: w is the same
arithmetic as the alpha channel, so per pair this is generous), 2^-21 the rounding of one q, M = the cell's pixels where fp32
and fp64 may disagree on `discard`, each moving at most one fragment of alpha_max e^-4 (as in test_blend_gpu.py).  Nothing
is excluded.  Every test prints the worst distance per case as a multiple of its bound.

Measured on an MI355X, worst distance over the cells as a multiple of the cell's bound, one-class map / worst map (always the
255-class one, whose cells are single pixels, except edges_47x47: 0.48 under the tile-aligned blocks as well):
    lengths            0.030 / 0.127        edges (ten frames)  0.053 .. 0.068 / 0.319 .. 0.509 (47x47)
    needles            0.135 / 0.378        epilogue_1, _3      0.067, 0.050 / 0.261, 0.233
    walls_80x48        0.018 / 0.027        epilogue_3_opaque   0.008 / 0.034
    walls_65x53        0.023 / 0.024
The kernel lies within half a bound of the model everywhere; the wall scenes' bound carries the cut's 1e-5 per pair and is
used to 3 %.  A second draw of splat 0 (the epilogue) would add 16.7 to its row on the two bare tiles, 300 .. 7000 x the row's
bound.

Exact properties are compared bit for bit: two fresh contexts, views added together, host against device maps of all four
dtypes, the rasterizer's options, tables of a context whose pair buffers had to grow."""
import numpy as np
import pytest

import blend_cases
import lift_model
from blend_model import TILE
from lift_model import ONE

pytestmark = pytest.mark.gpu

NAMES = list(blend_cases.all_cases())
BITWISE = [n for n in NAMES if blend_cases.bitwise(n)]
MAPS = ("uniform", "none", "checker", "blocks", "offset8", "c255")
_TABLES = {}


def lift_once(c, scene, seg, C, views=1):
    c.lift_begin(C)
    for _ in range(views):
        c.lift_view(scene.cam, seg)
    return c.lift_table()


def tables(gsx, name):
    """every map lifted on one case, in a fresh context with the default options: map -> uint64 table in upload order"""
    if name not in _TABLES:
        sc = blend_cases.prepared(name).scene
        out = {}
        with gsx.Context(0) as c:
            c.upload_splats(*sc.arrays())
            for key, (seg, C) in lift_model.maps(sc.W, sc.H).items():
                out[key] = lift_once(c, sc, seg, C)
                assert c.lift_num_views() == 1
        _TABLES[name] = out
    return _TABLES[name]


def test_constants(gsx):
    k = gsx.lift_constants()
    assert k["one"] == ONE == 1 << k["shift"] and k["tile"] == TILE and k["chunk"] == 256 and k["max_classes"] == 255
    assert k["cells"] // 256 >= 1 and 256 * k["one"] * 256 // 256 <= 2 ** 28        # a record's partial sum fits 32 bits


@pytest.mark.parametrize("name", NAMES)
def test_table_against_the_model(gsx, name):
    p = blend_cases.prepared(name)
    m = p.model
    n = m.rec.n
    assert not np.array_equal(p.packed, np.arange(n))                    # importance order is not upload order
    kept = np.zeros(n, bool)
    kept[m.walk[:n - m.n_epilogue]] = True
    dropped = np.asarray(m.rec.order)[~kept]                             # upload rows of the splats runSort drops
    assert len(dropped) == m.n_epilogue >= 1
    worst = {}
    for key in MAPS:
        seg, C = lift_model.maps(m.W, m.H)[key]
        L = lift_model.lift(m, seg, C)
        got = tables(gsx, name)[key]
        assert got.shape == (n, C + 1) and got.dtype == np.uint64
        want = L.upload_rows(L.table)
        bound = L.upload_rows(lift_model.cell_bound(L, p.tol, p.alpha_max, blend_cases.bitwise(name)))
        dist = np.abs(got.astype(np.float64) / ONE - want)
        assert (got[dropped] == 0).all(), key
        fed = bound > 0
        assert (got[~fed] == 0).all(), key                               # no pair in the model's lists: nothing at all
        worst[key] = float((dist[fed] / bound[fed]).max())
        assert (dist <= bound).all(), (key, worst[key])
    print(f"{name}: worst |table / 2^20 - model| as a multiple of its bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("name", [n for n in NAMES if blend_cases.family(n) == "epilogue"])
def test_epilogue_leaves_no_trace(gsx, name):
    """splat 0 is drawn again once per dropped splat, last: its row holds what its ONE place in the lists gives.  One more
    draw would add the weights below on the tiles that hold nothing else - far beyond the bound."""
    p = blend_cases.prepared(name)
    m, meta = p.model, p.scene.meta
    seg, C = lift_model.maps(m.W, m.H)["uniform"]
    L = lift_model.lift(m, seg, C)
    row = tables(gsx, name)["uniform"][meta["zero"]].astype(np.float64) / ONE
    bound = lift_model.cell_bound(L, p.tol, p.alpha_max, blend_cases.bitwise(name))[0]
    extra = 0.0
    for t in meta["bare"]:                                               # tiles whose list is [0]: a second draw adds (1 - B) B
        _, B, _ = m.tile_terms(t)
        extra += float(((1 - B[0]) * B[0])[m.tile_pixels(t)[2]].sum())
    print(f"{name}: splat 0 holds {row.sum():.3f}, one more draw would add {extra:.3f} on the bare tiles, bound {bound.sum():.2e}")
    assert extra > 100 * bound.sum()
    assert np.abs(row - L.table[0]).sum() <= bound.sum()


@pytest.mark.parametrize("name", BITWISE)
def test_two_fresh_contexts_agree_bit_for_bit(gsx, name):
    sc = blend_cases.prepared(name).scene
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays())
        for key in ("checker", "offset8", "c255"):
            seg, C = lift_model.maps(sc.W, sc.H)[key]
            assert np.array_equal(lift_once(c, sc, seg, C), tables(gsx, name)[key]), key


@pytest.mark.parametrize("name", ["needles", "walls_65x53", "edges_47x47"])
def test_views_add_exactly(gsx, name):
    sc = blend_cases.prepared(name).scene
    a, b = tables(gsx, name)["checker"], tables(gsx, name)["blocks"]
    ma, mb = (lift_model.maps(sc.W, sc.H)[k][0] for k in ("checker", "blocks"))
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays())
        c.lift_begin(4)
        c.lift_view(sc.cam, ma)
        c.lift_view(sc.cam, mb)
        assert c.lift_num_views() == 2
        both = c.lift_table()
        c.lift_view(sc.cam, ma)
        again = c.lift_table()
    assert np.array_equal(both, a + b) and np.array_equal(again, a + b + a) and a.sum() > 0 and not np.array_equal(a, b)


def test_host_and_device_maps_of_every_dtype(gsx):
    import torch
    sc = blend_cases.prepared("edges_47x41").scene
    blocks, checker = tables(gsx, "edges_47x41")["blocks"], tables(gsx, "edges_47x41")["checker"]
    mb, mc = (lift_model.maps(sc.W, sc.H)[k][0] for k in ("blocks", "checker"))
    forms = [(mb.astype(np.int32), False, blocks), (mb.astype(np.int64), False, blocks), ((mb + 1).astype(np.uint8), True, blocks),
             (mc.astype(np.uint8), False, checker)]                      # uint8 labels cannot say -1: the checker has none
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays())
        for seg, packed, want in forms:
            c.lift_begin(4)
            c.lift_view(sc.cam, seg, packed_u8=packed)
            host = c.lift_table()
            c.lift_begin(4)
            c.lift_view(sc.cam, torch.from_numpy(seg).to("cuda:0"), packed_u8=packed)
            dev = c.lift_table()
            assert np.array_equal(host, want) and np.array_equal(dev, want), (seg.dtype, packed)


@pytest.mark.parametrize("name", BITWISE)
def test_rasterizer_options_do_not_change_a_table(gsx, name):
    sc = blend_cases.prepared(name).scene
    seg, C = lift_model.maps(sc.W, sc.H)["offset8"]
    want = tables(gsx, name)["offset8"]
    for opts in ({"exact_cull": 1}, {"render_bin32": 0}, {"render_phases": 1}, {"render_phases": 3}, {"blend_pk2": 0}, {"blend_pk2": 1},
                 {"render_wide_sort": 0}):
        with gsx.Context(0) as c:
            for k, v in opts.items():
                c.set_option(k, v)
            c.upload_splats(*sc.arrays())
            assert np.array_equal(lift_once(c, sc, seg, C), want), opts


def test_frames_and_lift_views_interleave(gsx):
    """a lift view leaves the context able to render, and a rendered frame does not disturb a run"""
    sc = blend_cases.prepared("lengths").scene
    seg, C = lift_model.maps(sc.W, sc.H)["blocks"]
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays())
        before = c.render_view(sc.cam, sc.W, sc.H)
        c.lift_begin(C)
        c.lift_view(sc.cam, seg)
        # one class per tile and every record inside its tile: one atomic per record
        assert c.lift_num_atomics() == c.render_num_pairs() == c.render_num_pairs_consumed() == sum(blend_cases.LENGTHS)
        assert np.array_equal(c.render_view(sc.cam, sc.W, sc.H), before)
        c.lift_view(sc.cam, seg)
        assert np.array_equal(c.lift_table(), 2 * tables(gsx, "lengths")["blocks"])


# ---- finalize -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lengths", "walls_80x48", "epilogue_3_opaque"])
def test_finalize_is_the_rule_on_the_gpus_own_table(gsx, name):
    sc = blend_cases.prepared(name).scene
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays())
        for key in ("checker", "c255", "none"):
            seg, C = lift_model.maps(sc.W, sc.H)[key]
            table = lift_once(c, sc, seg, C)
            totals = table.sum(1)
            fed = np.flatnonzero(totals > 1)
            r = int(fed[np.argsort(totals[fed])[len(fed) // 2]])         # a row with a middling total among those that hold any
            assert len(fed) > 10
            for mw in (0.0, 1e-3, int(totals[r]) / ONE, (int(totals[r]) - 1) / ONE, (int(totals[r]) + 1) / ONE):
                labels, share = c.lift_finalize(mw, return_share=True)
                want_l, want_s = lift_model.finalize(table, mw)
                assert np.array_equal(labels, want_l) and np.array_equal(share, want_s), (key, mw)
                assert np.array_equal(c.lift_finalize(mw), want_l)
            assert c.lift_finalize(int(totals[r]) / ONE)[r] == int(table[r].argmax()) - 1      # exactly at the total: kept
            assert c.lift_finalize((int(totals[r]) + 1) / ONE)[r] == -1
    if name == "walls_80x48":                                            # what the vote cannot do
        meta = sc.meta
        hidden = np.array([i for t, (_, _, loud) in meta["tags"].items() if t != meta["hole"] for i in loud])
        with gsx.Context(0) as c:
            c.upload_splats(*sc.arrays())
            lift_once(c, sc, *lift_model.maps(sc.W, sc.H)["uniform"])
            labels = c.lift_finalize(1e-3)
        assert (labels[hidden] == -1).all() and (labels[meta["walls"][0]] == 2)


def tie_scene():
    """32x32, one splat whose centre is the frame's centre, the common corner of the four tiles: its fragments are point-symmetric
    in fp32 as well (dx = +-0.5, +-1.5, ..), so two half-planes through the centre collect exactly the same integers"""
    sc = blend_cases.Scene("tie", 32, 32)
    sc.add(16.0, 16.0, 3.0, (4.0, 2.5, 3.0), (0.9, 0.1, 0.2, 0.38), 120, (200, 40, 90))
    sc.add(5.0, 26.0, 3.5, (0.8, 0.8, 0.8), (1, 0, 0, 0), 90, (20, 40, 250))
    blend_cases.add_sink(sc)
    return sc


def test_finalize_ties(gsx):
    sc = tie_scene()
    r, x = np.mgrid[0:32, 0:32]
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays())
        for seg, label in ((np.where(x < 16, -1, 0), -1), (np.where(x < 16, 3, 1), 1), (np.where(r < 16, 2, 0), 0)):
            seg = seg.astype(np.int32)
            t = lift_once(c, sc, seg, 4)
            lo, hi = sorted(set(int(v) + 1 for v in np.unique(seg)))
            assert t[0, lo] == t[0, hi] > ONE // 10, (t[0], lo, hi)         # a constructed tie between two bins
            labels, share = c.lift_finalize(0.0, return_share=True)
            want_l, want_s = lift_model.finalize(t, 0.0)
            assert labels[0] == label == want_l[0] and share[0] == 0.5
            assert np.array_equal(labels, want_l) and np.array_equal(share, want_s)


# ---- errors: argument checks, nothing is launched on bad data ----------------------------------------------------------------
def test_errors(gsx):
    GsxError, E_STATE = gsx._lib.GsxError, gsx._lib.GSX_E_STATE
    sc = blend_cases.prepared("edges_17x17").scene
    seg, C = lift_model.maps(sc.W, sc.H)["blocks"]
    with gsx.Context(0) as c:
        with pytest.raises(GsxError) as e:                               # before upload_splats
            c.lift_begin(4)
        assert e.value.code == E_STATE
        c.upload_splats(*sc.arrays())
        for call in (lambda: c.lift_view(sc.cam, seg), lambda: c.lift_finalize(), lambda: c.lift_table()):
            with pytest.raises(GsxError) as e:                           # before lift_begin
                call()
            assert e.value.code == E_STATE
        assert c.lift_num_views() == 0
        for bad in (0, 256, -3):
            with pytest.raises(ValueError):
                c.lift_begin(bad)
        c.lift_begin(C)
        c.lift_view(sc.cam, seg)
        before = c.lift_table()
        wrong = seg.copy()
        wrong[9, 4] = C                                                  # one label past the range, on the host
        for m in (wrong, wrong.astype(np.int64), np.where(wrong < 0, 0, wrong).astype(np.uint8), np.full(seg.shape, -2, np.int32)):
            with pytest.raises(ValueError, match="view 1"):
                c.lift_view(sc.cam, m)
        assert c.lift_num_views() == 1 and np.array_equal(c.lift_table(), before)
        with pytest.raises(ValueError):
            c.lift_finalize(-1.0)
        with pytest.raises(ValueError):
            c.lift_finalize(float("nan"))
        c.set_render_edits(hidden=[3])                                   # an edit state
        with pytest.raises(GsxError) as e:
            c.lift_view(sc.cam, seg)
        assert e.value.code == E_STATE
        c.clear_render_edits()
        c.lift_view(sc.cam, seg)
        assert np.array_equal(c.lift_table(), 2 * before)
        c.upload_splats(*sc.arrays())                                    # a new upload ends the run
        with pytest.raises(GsxError) as e:
            c.lift_table()
        assert e.value.code == E_STATE and c.lift_num_views() == 0


def test_device_map_out_of_range_fails_finalize_naming_the_view(gsx):
    import torch
    sc = blend_cases.prepared("edges_17x17").scene
    seg, C = lift_model.maps(sc.W, sc.H)["blocks"]
    wrong = seg.copy()
    wrong[3, 3] = C
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays())
        c.lift_begin(C)
        c.lift_view(sc.cam, torch.from_numpy(seg).to("cuda:0"))
        c.lift_view(sc.cam, torch.from_numpy(wrong).to("cuda:0"))
        c.lift_view(sc.cam, torch.from_numpy(wrong).to("cuda:0"))
        with pytest.raises(ValueError, match="view 1 "):
            c.lift_finalize()
        with pytest.raises(ValueError, match="view 1 "):
            c.lift_table()
        c.lift_begin(C)                                                  # a new run starts clean
        c.lift_view(sc.cam, seg)
        assert np.array_equal(c.lift_table(), tables(gsx, "edges_17x17")["blocks"])


# ---- pair-buffer growth ---------------------------------------------------------------------------------------------------
N_FAINT = 66000


def faint_scene():
    """66 000 faint splats (alpha 1/255, 3 sigma = 280 .. 320 px) centred on a 64x64 frame: each covers all 16 tiles,
    1 056 000 pairs, more than the 2^20 the pair buffers start with for a scene of this size"""
    rng = np.random.default_rng(20271)
    n = N_FAINT
    sc = blend_cases.Scene("faint", 64, 64)
    u, v, z = rng.uniform(28, 36, n), rng.uniform(28, 36, n), rng.uniform(3.0, 5.0, n)
    sig = rng.uniform(280.0, 320.0, n)
    f = sc.f
    sc.xyz = [((a - 32) * c / f, (b - 32) * c / f, c) for a, b, c in zip(u, v, z)]
    sc.scale = [[float(np.log(s * c / f))] * 3 for s, c in zip(sig, z)]
    sc.rot = [[1.0, 0.0, 0.0, 0.0]] * n
    sc.opacity = [float(np.log((1 / 255) / (1 - 1 / 255)))] * n
    sc.f_dc = [[0.3, -0.2, 0.1]] * n
    blend_cases.add_sink(sc)
    return sc


def one_tile_totals(sc, t):
    """per packed record: sum over tile t's pixels of w, and the pairs with a fragment - the model's arithmetic on ONE tile, walked
    in chunks (the whole frame of this scene is 17 M pairs)"""
    import blend_model
    R = blend_model.Records(*sc.args())
    n, nd = R.n, R.dropped
    walk = R.depth_index.astype(np.int64)[:n - nd]
    ty, tx = divmod(t, R.tiles_x)
    ys, xs = np.mgrid[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE]
    total, pairs = np.zeros(n), np.zeros(n, np.int64)
    T = np.ones((TILE, TILE))
    for s in range(0, len(walk), 2048):
        ids = walk[s:s + 2048]
        ids = ids[[R.box[i][1] >= R.box[i][0] for i in ids]]
        c, g0, g1, col = (a[ids].astype(np.float64) for a in (R.c, R.g0, R.g1, R.color))
        dx = (xs + 0.5)[None] - c[:, 0, None, None]
        dy = (sc.H - (ys + 0.5))[None] - c[:, 1, None, None]
        vx = dx * g0[:, 0, None, None] + dy * g0[:, 1, None, None]
        vy = dx * g1[:, 0, None, None] + dy * g1[:, 1, None, None]
        q = vx * vx + vy * vy
        assert (np.abs(q - 4.0) > blend_model.NEAR).all()                # no fragment near the threshold: M = 0
        B = np.where(q <= 4.0, np.exp(-q) * col[:, 3, None, None], 0.0)
        Tk = T[None] * np.cumprod(np.concatenate([np.ones((1, TILE, TILE)), 1.0 - B]), 0)
        total[ids] = (Tk[:-1] * B).sum((1, 2))
        pairs[ids] = (B > 0).sum((1, 2))
        T = Tk[-1]
    return total, pairs, np.asarray(R.order), float(R.color[R.drawn, 3].max())


def test_pair_buffers_grow_before_anything_is_counted(gsx):
    sc = faint_scene()
    t0 = 6                                                               # the one tile the model evaluates; class 0 there, -1 elsewhere
    seg = np.full((64, 64), -1, np.int32)
    seg[16:32, 32:48] = 0
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays())
        fresh = lift_once(c, sc, seg, 1)
        pairs = c.render_num_pairs()
        assert pairs > 2 ** 20                                           # more than the buffers start with
    with gsx.Context(0) as c:
        for k, v in {"render_phases": 1, "render_bin32": 0}.items():    # the frame bins every pair at once, as a lift frame does
            c.set_option(k, v)
        c.upload_splats(*sc.arrays())
        c.render_view(sc.cam, sc.W, sc.H, to_host=False)                 # overflows, grows the buffers, redoes the frame
        assert c.render_num_pairs() == pairs
        grown = lift_once(c, sc, seg, 1)
        twice = lift_once(c, sc, seg, 1, views=2)
    assert np.array_equal(fresh, grown) and np.array_equal(twice, 2 * fresh)
    total, pairs, order, alpha_max = one_tile_totals(sc, t0)
    want, P = np.zeros(len(order)), np.zeros(len(order), np.int64)
    want[order], P[order] = total, pairs
    # tiles reach the opacity cut here (1 - 1/255 to the power of 66 000): the kernel's 1e-5 per pixel comes on top; the frame
    # tolerance of the blend scenes is capped at 1e-5 (blend_cases.Prepared.tol) and this scene gets the cap
    bound = P * (1.0e-5 + 2.0 ** -21 + 1.0e-5)
    dist = np.abs(fresh[:, 1].astype(np.float64) / ONE - want)
    print(f"faint: {int((fresh[:, 1] > 0).sum())} of {len(order)} splats reach tile {t0} before it is opaque; worst distance "
          f"{float((dist[P > 0] / bound[P > 0]).max()):.3f} x bound; the nearest splat holds {want.max():.4f}")
    assert (dist <= bound).all() and (fresh[:, 1] > 0).sum() > 1000 and want.max() > 0.5
