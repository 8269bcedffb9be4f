"""Depth frames (csrc/depthmap.hip, include/gsx.h: gsx_depth_view, gsx_depth_pick) on the 17 scenes of tests/blend_cases.py and the
constructed scenes of tests/depthmap_model.py.  test_depthmap_model.py shows on the CPU that the model is what it claims and
that the margins used here exist.

Exact, with no tolerance:
(a) total == gsx_label_view's total_out;
(b) sum over {p: seg[p] = c} of moment[p] == sum over i of key_i * gsx_lift_table[i][c + 1] for the six maps of lift_model.maps,
    in Python integers, key from gsx_debug_render_pre turned to upload order;
(c) on needles and the ten edge frames (n <= 255: one label per splat makes gsx_label_view's planes q[i][p] exactly) all four
    outputs equal the integer rule stated in numpy over the model's per-tile list order and the GPU's keys, at quantiles 0.5,
    0.1, 2^-21, 1 and two built from the GPU's own q so that the cut equals a running sum and exceeds it by one;
(d) the surface-only mode gives the same surface maps;
(e) two fresh contexts, the rasterizer's options, frames / lift tables / label maps around depth views, grown pair buffers;
(f) gsx_depth_pick against the device maps at every pixel of an edge frame, misses, GSX_E_STATE;
(g) the error codes one by one, a 1x1 frame, a frame none of whose tiles has a list.
Constructed: the chunk-border scenes (the surface is the opaque splat behind L - 1 faint records, L around the staged chunk)
and walls_80x48 under the tags' labels (the pick is the wall where gsx_hit_test gives what stands behind it).

Against the fp64 model, per pixel, nothing excluded:
    |moment / 2^20 - model| <= (P (tol + 2^-21 [+ 1e-5 where tiles reach the cut]) + M alpha_max e^-4) max |key| over the tile's list
- the label frames' bound, term for term - and the surface's upload row at the model's DECIDED pixels of walls_80x48,
walls_65x53 and epilogue_3_opaque at quantile 0.5.  No reference implements depth frames: nothing here is pinned to one."""
import math

import numpy as np
import pytest

import blend_cases
import depthmap_model
import labelmap_model
import lift_model
import test_lift_gpu as lift_gpu
from lift_model import ONE

pytestmark = pytest.mark.gpu

NAMES = list(blend_cases.all_cases())
BITWISE = [n for n in NAMES if blend_cases.bitwise(n)]
SMALL = [n for n in NAMES if n == "needles" or blend_cases.family(n) == "edges"]
NO_SELECTION = -999999
_VIEWS = {}


class View:
    pass


def upload_keys(c, sc):
    """the view's depth key per splat in upload order, and the importance permutation (importance row -> upload row)"""
    depth = c.debug_render_pre([sc.cam], sc.W, sc.H)[0]["depth"]
    order = c.render_debug()[1].astype(np.int64)
    key = np.zeros(len(order), np.int64)
    key[order] = depth
    return key, order


def views(gsx, name):
    """one case in a fresh context with the default options: the depth frame at quantile 0.5, the surface-only maps, the label
    view's total (parity labels), the keys in upload order"""
    if name not in _VIEWS:
        sc = blend_cases.prepared(name).scene
        v = View()
        with gsx.Context(0) as c:
            c.upload_splats(*sc.arrays(), labels=labelmap_model.pattern("parity", len(sc.xyz))[0])
            v.frame = c.depth_view(sc.cam, sc.W, sc.H, 0.5)
            v.surfaces = c.depth_num_surface()
            v.only = c.depth_view(sc.cam, sc.W, sc.H, 0.5, surface_only=True)
            v.label_total = c.label_view(sc.cam, sc.W, sc.H, 4, return_weights=True)[2]
            v.key, v.order = upload_keys(c, sc)
        _VIEWS[name] = v
    return _VIEWS[name]


def same(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("total", "moment", "surface_key", "surface_index"))


def test_constants(gsx):
    k, l = gsx.depth_constants(), gsx.lift_constants()
    assert k["one"] == ONE == l["one"] and k["shift"] == l["shift"] and k["tile"] == l["tile"] == 16 and k["chunk"] == l["chunk"] == 256


@pytest.mark.parametrize("name", NAMES)
def test_totals_are_the_label_views(gsx, name):
    sc = blend_cases.prepared(name).scene
    v = views(gsx, name)
    f = v.frame
    assert f.total.dtype == np.uint32 and f.moment.dtype == np.int64 and f.surface_key.dtype == f.surface_index.dtype == np.int32
    assert all(a.shape == (sc.H, sc.W) for a in (f.total, f.moment, f.surface_key, f.surface_index))
    assert np.array_equal(f.total, v.label_total) and f.total.max() > 0
    has = f.surface_index >= 0
    assert np.array_equal(has, f.total >= ONE // 2) and v.surfaces == int(has.sum())
    assert (f.surface_key[~has] == 0).all() and (f.surface_index[~has] == -1).all() and f.surface_index.max() < len(sc.xyz)
    assert np.array_equal(f.surface_key[has], v.key[f.surface_index[has]])                      # the surface's key is its splat's key
    assert np.isnan(f.expected_z[f.total == 0]).all() and np.isnan(f.surface_z[~has]).all()
    fed = f.total > 0
    z = np.asarray(sc.xyz)[:, 2]                                                                # the identity camera: z_view = z
    assert (f.expected_z[fed] > z.min() - 1e-3).all() and (f.expected_z[fed] < z.max() + 1e-3).all()
    assert (np.abs(f.surface_z[has] - z[f.surface_index[has]]) <= f.scale).all()


@pytest.mark.parametrize("name", NAMES)
def test_moment_identity_with_the_lift_table(gsx, name):
    """sum over {p: seg[p] = c} of moment[p] == sum over i of key_i * gsx_lift_table[i][c + 1], as Python integers"""
    sc = blend_cases.prepared(name).scene
    v = views(gsx, name)
    moment = v.frame.moment.reshape(-1).astype(object)
    checked = 0
    for mkey, (seg, C) in lift_model.maps(sc.W, sc.H).items():
        table = lift_gpu.tables(gsx, name)[mkey]
        fed = np.flatnonzero(table.any(1))
        keys = v.key[fed].astype(object)
        flat = seg.reshape(-1)
        for c in range(-1, C):
            col = table[fed, c + 1]
            nz = np.flatnonzero(col)
            right = sum((int(k) * int(t) for k, t in zip(keys[nz], col[nz])), 0)
            left = sum((int(m) for m in moment[flat == c]), 0)
            assert left == right, (mkey, c, left, right)
            checked += int(right != 0)
    assert checked >= 10
    print(f"{name}: {checked} non-zero class sums of moment agree exactly with key x lift table")


def numpy_rule(sc, model, order, key, planes, quantile):
    """the integer rule over the model's per-tile list order on q[i][p] = planes[upload row i][p] -> the four maps"""
    H, W = sc.H, sc.W
    total, moment = np.zeros((H, W), np.uint32), np.zeros((H, W), np.int64)
    skey, srow = np.zeros((H, W), np.int32), np.full((H, W), -1, np.int32)
    for t, ids in enumerate(model.lists):
        if len(ids) == 0:
            continue
        ys, xs, inside = model.tile_pixels(t)
        y, x = ys[inside], xs[inside]
        rows = order[ids]
        total[y, x], moment[y, x], skey[y, x], srow[y, x] = depthmap_model.rule(planes[rows][:, y, x], key[rows], rows, quantile)
    return total, moment, skey, srow


@pytest.mark.parametrize("name", SMALL)
def test_per_fragment_rule(gsx, name):
    p = blend_cases.prepared(name)
    sc, m = p.scene, p.model
    n = len(sc.xyz)
    assert n <= 255
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays(), labels=np.arange(n, dtype=np.int32))
        planes = c.label_view(sc.cam, sc.W, sc.H, 255, planes=np.arange(n))[1]               # q[i][p], i = upload row
        key, order = upload_keys(c, sc)
        assert np.array_equal(order, np.asarray(m.rec.order))
        # a pixel with many fragments, and the running sum at its middle fragment: the cut on it, and one beyond
        py, px = np.unravel_index((planes > 0).sum(0).argmax(), (sc.H, sc.W))
        t = (py // 16) * m.tiles_x + px // 16
        q = planes[order[m.lists[t]], py, px].astype(np.int64)
        pos = np.flatnonzero(q)
        assert len(pos) >= 3
        mid = pos[len(pos) // 2]
        R = int(q[:mid + 1].sum())
        assert 0 < R < ONE
        quantiles = (0.5, 0.1, 2.0 ** -21, 1.0, R / ONE, (R + 1) / ONE)
        assert [depthmap_model.cut_of(x) for x in quantiles[2:]] == [1, ONE, R, R + 1]
        at = {}
        for quantile in quantiles:
            want = numpy_rule(sc, m, order, key, planes, quantile)
            f = c.depth_view(sc.cam, sc.W, sc.H, quantile)
            got = (f.total, f.moment, f.surface_key, f.surface_index)
            for what, g, w in zip(("total", "moment", "surface_key", "surface_index"), got, want):
                assert g.dtype == w.dtype and np.array_equal(g, w), (quantile, what, int((g != w).sum()))
            only = c.depth_view(sc.cam, sc.W, sc.H, quantile, surface_only=True)
            assert np.array_equal(only.surface_key, want[2]) and np.array_equal(only.surface_index, want[3]), quantile
            at[quantile] = int(f.surface_index[py, px])
        rows = order[m.lists[t]]
        assert at[R / ONE] == rows[mid]                                                       # the cut equals the running sum: this fragment
        assert at[(R + 1) / ONE] == rows[pos[len(pos) // 2 + 1]]                              # one more: the next fragment with q > 0
        assert at[2.0 ** -21] == rows[pos[0]]                                                  # cut 1: the first fragment with q >= 1


@pytest.mark.parametrize("name", NAMES)
def test_surface_only_mode(gsx, name):
    sc = blend_cases.prepared(name).scene
    v = views(gsx, name)
    assert v.only.total is None and v.only.moment is None and v.only.expected_z is None
    assert np.array_equal(v.only.surface_key, v.frame.surface_key) and np.array_equal(v.only.surface_index, v.frame.surface_index)
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays())
        for quantile in (0.1, 0.9, 1.0):
            full, only = c.depth_view(sc.cam, sc.W, sc.H, quantile), c.depth_view(sc.cam, sc.W, sc.H, quantile, surface_only=True)
            assert np.array_equal(only.surface_key, full.surface_key) and np.array_equal(only.surface_index, full.surface_index), quantile
            assert c.depth_num_surface() == int((full.surface_index >= 0).sum())
            assert np.array_equal(full.total, v.frame.total) and np.array_equal(full.moment, v.frame.moment)


@pytest.mark.parametrize("name", NAMES)
def test_two_fresh_contexts_agree_bit_for_bit(gsx, name):
    sc = blend_cases.prepared(name).scene
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays())                                                         # labels are not needed
        assert same(c.depth_view(sc.cam, sc.W, sc.H, 0.5), views(gsx, name).frame)


@pytest.mark.parametrize("name", BITWISE)
def test_rasterizer_options_do_not_change_a_frame(gsx, name):
    sc = blend_cases.prepared(name).scene
    for opts in ({"render_bin32": 0}, {"render_compact": 0}, {"render_phases": 1}, {"render_phases": 3}):
        with gsx.Context(0) as c:
            for k, v in opts.items():
                c.set_option(k, v)
            c.upload_splats(*sc.arrays())
            assert same(c.depth_view(sc.cam, sc.W, sc.H, 0.5), views(gsx, name).frame), opts


def test_depth_views_leave_frames_lift_runs_and_label_maps_alone(gsx):
    sc = blend_cases.prepared("lengths").scene
    seg, Cm = lift_model.maps(sc.W, sc.H)["blocks"]
    labels, C = labelmap_model.pattern("mod255", len(sc.xyz))
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays(), labels=labels)
        before = c.render_view(sc.cam, sc.W, sc.H)
        label = c.label_view(sc.cam, sc.W, sc.H, C, return_weights=True)
        first = c.depth_view(sc.cam, sc.W, sc.H, 0.5)
        assert c.render_num_pairs() == c.render_num_pairs_consumed() == sum(blend_cases.LENGTHS)
        assert np.array_equal(c.render_view(sc.cam, sc.W, sc.H), before)
        c.lift_begin(Cm)
        c.lift_view(sc.cam, seg)
        assert same(c.depth_view(sc.cam, sc.W, sc.H, 0.5), first)
        c.depth_view(sc.cam, sc.W, sc.H, 0.25, surface_only=True)
        c.lift_view(sc.cam, seg)
        assert c.lift_num_views() == 2 and np.array_equal(c.lift_table(), 2 * lift_gpu.tables(gsx, "lengths")["blocks"])
        again = c.label_view(sc.cam, sc.W, sc.H, C, return_weights=True)
        assert all(np.array_equal(a, b) for a, b in zip(label, again))
        assert np.array_equal(c.render_view(sc.cam, sc.W, sc.H), before)
    assert same(first, views(gsx, "lengths").frame)


def test_pair_buffers_grow_before_anything_is_walked(gsx):
    sc = lift_gpu.faint_scene()
    labels = labelmap_model.pattern("parity", len(sc.xyz))[0]
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays(), labels=labels)
        fresh = c.depth_view(sc.cam, sc.W, sc.H, 0.5)                                          # grows the buffers itself
        assert c.render_num_pairs() > 2 ** 20
        total = c.label_view(sc.cam, sc.W, sc.H, 4, return_weights=True)[2]
        grown = c.depth_view(sc.cam, sc.W, sc.H, 0.5)
    assert np.array_equal(fresh.total, total) and same(fresh, grown) and (fresh.total > ONE // 2).all() and (fresh.surface_index >= 0).all()


def test_pick(gsx):
    GsxError, lib = gsx._lib.GsxError, gsx._lib
    sc = blend_cases.prepared("edges_17x17").scene
    n = len(sc.xyz)
    labels = (np.arange(n, dtype=np.int32) * 7919) % 100003 - 5                                # exact int32 labels, no class range
    W, H = sc.W, sc.H
    with gsx.Context(0) as c:
        def state_error():
            with pytest.raises(GsxError) as e:
                c.pick(1.0, 1.0)
            assert e.value.code == lib.GSX_E_STATE
        state_error()                                                                          # before any upload
        c.upload_splats(*sc.arrays(), labels=labels)
        state_error()                                                                          # before any view
        with pytest.raises(RuntimeError):
            c.depth_surface_index_device()
        f = c.depth_view(sc.cam, W, H, 0.3)
        index, key = c.depth_surface_index_device().cpu().numpy(), c.depth_surface_key_device().cpu().numpy()
        assert np.array_equal(index, f.surface_index) and np.array_equal(key, f.surface_key)
        assert (index >= 0).sum() > 20 and (index < 0).sum() > 20
        for r in range(H):
            for x in range(W):
                lab, row, z = c.pick(x + 0.25, (H - 1 - r) + 0.75)                              # y runs from the bottom
                if index[r, x] < 0:
                    assert (lab, row) == (NO_SELECTION, -1) and math.isnan(z), (r, x)
                else:
                    assert (lab, row, z) == (int(labels[index[r, x]]), int(index[r, x]), float(key[r, x]) * f.scale + f.offset), (r, x)
        x0, r0 = (int(v) for v in np.argwhere(index >= 0)[0][::-1])
        assert c.pick(float(x0), float(H - 1 - r0))[1] == index[r0, x0] and c.pick(x0 + 0.999, H - 1 - r0 + 0.999)[1] == index[r0, x0]
        for x, y in ((-0.001, 1.0), (float(W), 1.0), (1.0, -0.001), (1.0, float(H)), (1e30, 1.0), (float("nan"), 1.0), (1.0, float("nan")),
                     (float("-inf"), float("inf"))):
            lab, row, z = c.pick(x, y)
            assert (lab, row) == (NO_SELECTION, -1) and math.isnan(z), (x, y)
        c.upload_splats(*sc.arrays())                                                          # a new upload invalidates the view
        state_error()
        with pytest.raises(RuntimeError):
            c.depth_surface_key_device()
        assert c.depth_num_surface() == 0
        g = c.depth_view(sc.cam, W, H, 0.3)
        assert same(f, g)
        lab, row, z = c.pick(x0 + 0.5, H - 1 - r0 + 0.5)
        assert (lab, row) == (NO_SELECTION, int(index[r0, x0])) and z == float(key[r0, x0]) * f.scale + f.offset   # uploaded without labels


def test_errors_and_degenerate_frames(gsx):
    GsxError, lib = gsx._lib.GsxError, gsx._lib
    sc = blend_cases.prepared("edges_17x17").scene
    view = lambda c, **kw: c.depth_view(sc.cam, kw.pop("W", sc.W), kw.pop("H", sc.H), kw.pop("q", 0.5), **kw)

    def fails(call, code):
        if code == lib.GSX_E_INVALID:
            with pytest.raises(ValueError, match=f"libgsx error {code}:") as e:
                call()
        else:
            with pytest.raises(GsxError) as e:
                call()
            assert e.value.code == code
        return str(e.value)

    with gsx.Context(0) as c:
        assert "no splats uploaded" in fails(lambda: view(c), lib.GSX_E_STATE)
        c.upload_splats(*sc.arrays())                                                          # without labels: not needed
        good = view(c)
        kept = lambda: (np.array_equal(c.depth_surface_index_device().cpu().numpy(), good.surface_index) and
                        np.array_equal(c.depth_surface_key_device().cpu().numpy(), good.surface_key) and
                        c.pick(8.5, 8.5)[1] == good.surface_index[sc.H - 1 - 8, 8])
        assert kept()
        c.set_render_edits(hidden=[0])
        assert "edit state" in fails(lambda: view(c), lib.GSX_E_STATE)
        c.clear_render_edits()
        assert kept()
        for kw in ({"W": 0}, {"H": 0}, {"W": -5}, {"q": 0.0}, {"q": -0.1}, {"q": 1.0 + 1e-12}, {"q": float("nan")}, {"q": float("inf")},
                   {"q": float("-inf")}):
            fails(lambda: view(c, **kw), lib.GSX_E_INVALID)
            fails(lambda: view(c, surface_only=True, **kw), lib.GSX_E_INVALID)
            assert kept(), kw
        assert "4097x16" in fails(lambda: view(c, W=4097, H=16), lib.GSX_E_UNSUPPORTED)
        assert "16x4097" in fails(lambda: view(c, W=16, H=4097), lib.GSX_E_UNSUPPORTED)
        assert kept()
        assert same(view(c), good)                                                             # later calls work
        # a 1x1 frame: fx, fy are scaled to it, its one pixel looks down the axis
        one = view(c, W=1, H=1)
        assert all(a.shape == (1, 1) for a in (one.total, one.moment, one.surface_key, one.surface_index))
        assert tuple(c.depth_surface_index_device().shape) == (1, 1) and c.pick(0.5, 0.5)[1] == one.surface_index[0, 0]
        assert c.pick(1.0, 0.5)[1] == -1
        # a frame none of whose tiles has a list: the camera looks the other way
        away = dict(sc.cam, rotation=np.diag([-1.0, 1.0, -1.0]).tolist())
        for only in (False, True):
            f = c.depth_view(away, sc.W, sc.H, 0.5, surface_only=only)
            assert (f.surface_index == -1).all() and (f.surface_key == 0).all() and c.depth_num_surface() == 0
            assert only or ((f.total == 0).all() and (f.moment == 0).all() and np.isnan(f.expected_z).all())
        lab, row, z = c.pick(8.5, 8.5)
        assert c.render_num_pairs() == 0 and (lab, row) == (NO_SELECTION, -1) and math.isnan(z)
        assert same(view(c), good)


@pytest.mark.parametrize("L", depthmap_model.BORDER_L)
def test_chunk_border(gsx, L):
    b = depthmap_model.border(L)
    sc = b.scene
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays())
        f = c.depth_view(sc.cam, sc.W, sc.H, 0.5)
        assert c.render_num_pairs() == L and c.render_num_pairs_consumed() == L
        assert (f.surface_index == b.opaque).all() and c.depth_num_surface() == 256             # its own B >= 0.9 on every pixel (CPU test)
        key, _ = upload_keys(c, sc)
        assert (f.surface_key == key[b.opaque]).all() and (f.total <= ONE + L).all() and (f.total > 0.9 * ONE).all()
        only = c.depth_view(sc.cam, sc.W, sc.H, 0.5, surface_only=True)
        assert np.array_equal(only.surface_index, f.surface_index) and np.array_equal(only.surface_key, f.surface_key)
        if L > 1:                                                                              # below the faint sum the surface is a faint record
            low = c.depth_view(sc.cam, sc.W, sc.H, 2.0 ** -21)
            assert (low.surface_index != b.opaque).any() and (low.surface_index >= 0).all()


def test_walls_pick_the_wall_where_hit_test_picks_what_stands_behind_it(gsx):
    p = blend_cases.prepared("walls_80x48")
    sc, m = p.scene, p.model
    labels = depthmap_model.wall_labels(sc)
    d = depthmap_model.case_frame("walls_80x48")
    ys, xs, _ = m.tile_pixels(sc.meta["hole"])
    in_hole = np.zeros((sc.H, sc.W), bool)
    in_hole[ys, xs] = True
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays(), labels=labels)
        f = c.depth_view(sc.cam, sc.W, sc.H, 0.5)
        lab = np.where(f.surface_index >= 0, labels[np.maximum(f.surface_index, 0)], NO_SELECTION)
        assert not ((lab == 2) & d.decided & ~in_hole).any()                                   # never loud in an ordinary tile
        model_lab = np.where(d.index >= 0, labels[np.asarray(m.rec.order)[np.maximum(d.index, 0)]], NO_SELECTION)
        corners = (model_lab == 2) & d.decided & in_hole                                       # the open corner pixels of the hole tile
        assert corners.sum() >= 4 and (lab[corners] == 2).all()
        for r, x in np.argwhere(corners):
            assert c.pick(x + 0.5, sc.H - 1 - r + 0.5)[0] == 2
        order = np.asarray(m.rec.order)
        behind = depthmap_model.behind_the_walls(sc, d, order)
        assert len(behind) >= 5
        for t, i in behind.items():
            u, v = depthmap_model.centre_px(sc, i)
            hit_label, hit_row = c.hit_test(sc.cam, sc.W, sc.H, u, sc.H - v)
            pick_label, pick_row, z = c.pick(u, sc.H - v)
            assert hit_label == 2 and labels[order[hit_row]] == 2, t                            # the nearest centre: a loud record behind the wall
            assert pick_label == 3 and pick_row in sc.meta["walls"] and abs(z - 4.0) < 0.05, (t, pick_label)   # what the frame shows


@pytest.mark.parametrize("name", NAMES)
def test_moment_against_the_model(gsx, name):
    d = depthmap_model.case_frame(name)
    f = views(gsx, name).frame
    dist = np.abs(f.moment.astype(np.float64) / ONE - d.moment)
    fed = d.bound > 0
    assert (f.moment[~fed] == 0).all() and (f.total[~fed] == 0).all()                          # P = M = 0: exactly nothing
    worst = float((dist[fed] / d.bound[fed]).max()) if fed.any() else 0.0
    print(f"{name}: worst |moment / 2^20 - model| = {worst:.3f} x the pixel's bound")
    assert (dist <= d.bound).all(), worst


@pytest.mark.parametrize("name", ("walls_80x48", "walls_65x53", "epilogue_3_opaque"))
def test_surface_against_the_model(gsx, name):
    m = blend_cases.prepared(name).model
    d = depthmap_model.case_frame(name)
    f = views(gsx, name).frame
    surf = d.index >= 0
    undecided = int((surf & ~d.decided).sum())
    assert undecided <= 0.05 * surf.sum()
    want = np.where(surf, np.asarray(m.rec.order, np.int64)[np.maximum(d.index, 0)], -1)
    wrong = d.decided & (f.surface_index != want)
    print(f"{name}: {int((d.decided & surf).sum())} decided pixels with a surface, {undecided} undecided, "
          f"{int((~d.decided & (f.surface_index != want)).sum())} of the undecided differ from the model")
    assert not wrong.any(), np.argwhere(wrong)[:5]
