"""Label frames (csrc/labelmap.hip, include/gsx.h: gsx_label_view) on the scenes of tests/blend_cases.py under the label patterns
of tests/labelmap_model.py (given in upload order): one label, all -1, two labels by parity, i % K - 1 for K = WL - 1, WL,
WL + 1, 2 WL + 1 (WL = the labels of one LDS window) and K = 255, which puts all 255 labels into single lists.
test_labelmap_model.py shows on the CPU that the model is what it claims and that removing any single record moves an entry
by more than ten of the bounds used here.

Exact, with no tolerance: the transpose identity against the lift kernel's own table (both kernels sum the same integers
q = rint(w * 2^20)); label, weight and total against the integer rule applied in numpy to the GPU's own planes; two fresh
contexts; the rasterizer's options; a context whose pair buffers had to grow; frames and lift runs around label views; the
count of list walks; the device map; the error codes (all but "gsx_render_views is running", which a single caller thread
cannot bring about).

Against the fp64 model, per (bin, pixel), nothing excluded:
    |planes / 2^20 - model| <= P (tol + 2^-21) + M alpha_max e^-4,  plus P 1e-5 where tiles reach the opacity cut
- lift_model.cell_bound term for term (labelmap_model.entry_bound), tol = the scene's frame tolerance (blend_cases.Prepared.tol).
An entry with P = M = 0 must be exactly 0.  test_planes_against_the_model prints the worst distance per scene as a multiple of
the entry's bound.

Measured on an MI355X, worst distance over the entries as a multiple of the entry's bound, one-label pattern / worst pattern
(mod255 wherever the patterns differ; under `none` the planes are those of `one` in bin 0):
    lengths            0.126 / 0.127        edges (ten frames)  0.294 .. 0.509 / 0.320 .. 0.509 (47x47, every pattern)
    needles            0.286 / 0.378        epilogue_1, _3      0.270, 0.242 / the same
    walls_80x48        0.024 / 0.029        epilogue_3_opaque   0.034 / 0.037
    walls_65x53        0.018 / 0.026
The kernel lies within 0.51 of a bound of the model everywhere, where the lift kernel lies (test_lift_gpu.py): the two share
their fragments.  The one-label figures are larger than the lift's one-class figures because an entry here is a single pixel
under every pattern, as the lift's cells are only under its 255-class map."""
import numpy as np
import pytest

import blend_cases
import labelmap_model
import lift_model
import test_lift_gpu as lift_gpu
from lift_model import ONE

pytestmark = pytest.mark.gpu

NAMES = list(blend_cases.all_cases())
BITWISE = [n for n in NAMES if blend_cases.bitwise(n)]
_VIEWS = {}


class View:
    def __init__(self, label, weight, total, planes, passes):
        self.label, self.weight, self.total, self.planes, self.passes = label, weight, total, planes, passes


def patterns(gsx):
    return labelmap_model.pattern_names(gsx.labelmap_constants()["window"])


def label_once(c, sc, labels, C, min_weight=0.0):
    """upload with the labels, one label view with the planes of all C + 1 bins"""
    c.upload_splats(*sc.arrays(), labels=labels)
    label, weight, total, planes = c.label_view(sc.cam, sc.W, sc.H, C, min_weight, planes=np.arange(-1, C), return_weights=True)
    return View(label, weight, total, planes, c.label_num_passes())


def views(gsx, name):
    """every pattern on one case, in a fresh context with the default options: pattern -> View"""
    if name not in _VIEWS:
        sc = blend_cases.prepared(name).scene
        out = {}
        with gsx.Context(0) as c:
            for pat in patterns(gsx):
                labels, C = labelmap_model.pattern(pat, len(sc.xyz))
                out[pat] = label_once(c, sc, labels, C)
        _VIEWS[name] = out
    return _VIEWS[name]


def test_constants(gsx):
    k, l = gsx.labelmap_constants(), gsx.lift_constants()
    assert k["one"] == ONE == l["one"] and k["shift"] == l["shift"] and k["tile"] == l["tile"] == 16 and k["chunk"] == l["chunk"] == 256
    assert k["max_classes"] == 255 and 2 <= k["window"] <= 128


@pytest.mark.parametrize("name", NAMES)
def test_transpose_identity_with_the_lift_table(gsx, name):
    """sum over {p: seg[p] = c} of planes[b][p] == sum over {i: label[i] = b - 1} of gsx_lift_table[i][c + 1], as integers"""
    sc = blend_cases.prepared(name).scene
    n = len(sc.xyz)
    checked = 0
    for pat in patterns(gsx):
        labels, C = labelmap_model.pattern(pat, n)
        v = views(gsx, name)[pat]
        assert v.planes.shape == (C + 1, sc.H, sc.W) and v.planes.dtype == np.uint32
        by_bin = np.zeros((n, C + 1))
        by_bin[np.arange(n), labels + 1] = 1.0
        for key, (seg, Cm) in lift_model.maps(sc.W, sc.H).items():
            table = lift_gpu.tables(gsx, name)[key]
            by_class = np.zeros((sc.W * sc.H, Cm + 1))
            by_class[np.arange(sc.W * sc.H), seg.reshape(-1) + 1] = 1.0
            # float64 sums of integers below 2^53 are exact: at most 2^21 per entry, 2^13 pixels, 2^13 splats
            left = v.planes.reshape(C + 1, -1).astype(np.float64) @ by_class
            right = by_bin.T @ table.astype(np.float64)
            assert left.max() < 2.0 ** 52 and np.array_equal(left, right), (pat, key, float(np.abs(left - right).max()))
            checked += int((left > 0).sum())
    assert checked > 100
    print(f"{name}: {checked} non-zero (bin, class) sums agree exactly with the lift table")


@pytest.mark.parametrize("name", NAMES)
def test_integer_rule_on_the_gpus_own_planes(gsx, name):
    sc = blend_cases.prepared(name).scene
    for pat, v in views(gsx, name).items():
        label, weight, total = labelmap_model.finalize(v.planes, 0.0)
        assert np.array_equal(v.label, label) and np.array_equal(v.weight, weight) and np.array_equal(v.total, total), pat
        assert v.label.dtype == np.int32 and v.label.shape == (sc.H, sc.W)
    WL = gsx.labelmap_constants()["window"]
    with gsx.Context(0) as c:
        for pat in ("parity", f"mod{WL + 1}", "mod255"):
            labels, C = labelmap_model.pattern(pat, len(sc.xyz))
            v = views(gsx, name)[pat]
            c.upload_splats(*sc.arrays(), labels=labels)
            fed = np.unique(v.total[v.total > 0])
            assert len(fed) > 10
            mid = int(fed[len(fed) // 2])                                 # a total with pixels below and above it
            for mw in (0.0, mid / ONE, (mid + 0.5) / ONE, 1e-3, 1.0, 1.5, 4.0):
                want = labelmap_model.finalize(v.planes, mw)
                got = c.label_view(sc.cam, sc.W, sc.H, C, mw, return_weights=True)                 # no planes
                assert all(np.array_equal(g, w) for g, w in zip(got, want)), (pat, mw)
                assert np.array_equal(c.label_view(sc.cam, sc.W, sc.H, C, mw), want[0]), (pat, mw)   # the map alone
                some = c.label_view(sc.cam, sc.W, sc.H, C, mw, planes=[C - 1, -1, C - 1])
                assert np.array_equal(some[0], want[0]) and np.array_equal(some[1], v.planes[[C, 0, C]]), (pat, mw)
            at, above = labelmap_model.finalize(v.planes, mid / ONE)[1], labelmap_model.finalize(v.planes, (mid + 0.5) / ONE)[1]
            assert ((above == 0) & (at > 0) & (v.total == mid)).any()      # the threshold is met exactly at the total
            assert (labelmap_model.finalize(v.planes, 4.0)[0] == -1).all()


@pytest.mark.parametrize("name", NAMES)
def test_two_fresh_contexts_agree_bit_for_bit(gsx, name):
    sc = blend_cases.prepared(name).scene
    WL = gsx.labelmap_constants()["window"]
    with gsx.Context(0) as c:
        for pat in ("one", f"mod{WL + 1}", "mod255"):
            labels, C = labelmap_model.pattern(pat, len(sc.xyz))
            a, b = label_once(c, sc, labels, C), views(gsx, name)[pat]
            assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("label", "weight", "total", "planes")) and a.passes == b.passes, pat


@pytest.mark.parametrize("name", BITWISE)
def test_rasterizer_options_do_not_change_a_map(gsx, name):
    sc = blend_cases.prepared(name).scene
    pat = f"mod{gsx.labelmap_constants()['window'] + 1}"
    labels, C = labelmap_model.pattern(pat, len(sc.xyz))
    want = views(gsx, name)[pat]
    for opts in ({"exact_cull": 1}, {"render_bin32": 0}, {"render_phases": 1}, {"render_phases": 3}, {"blend_pk2": 0}, {"blend_pk2": 1},
                 {"render_wide_sort": 0}):
        with gsx.Context(0) as c:
            for k, v in opts.items():
                c.set_option(k, v)
            got = label_once(c, sc, labels, C)
            assert np.array_equal(got.label, want.label) and np.array_equal(got.planes, want.planes) and np.array_equal(got.weight, want.weight), opts


def test_pair_buffers_grow_before_anything_is_walked(gsx):
    sc = lift_gpu.faint_scene()
    n = len(sc.xyz)
    labels, C = labelmap_model.pattern(f"mod{gsx.labelmap_constants()['window'] + 1}", n)
    with gsx.Context(0) as c:
        fresh = label_once(c, sc, labels, C)
        pairs = c.render_num_pairs()
        assert pairs > 2 ** 20                                           # more than the buffers start with
    with gsx.Context(0) as c:
        for k, v in {"render_phases": 1, "render_bin32": 0}.items():    # the frame bins every pair at once, as a label frame does
            c.set_option(k, v)
        c.upload_splats(*sc.arrays(), labels=labels)
        c.render_view(sc.cam, sc.W, sc.H, to_host=False)                 # overflows, grows the buffers, redoes the frame
        assert c.render_num_pairs() == pairs
        grown = label_once(c, sc, labels, C)
    assert all(np.array_equal(getattr(fresh, k), getattr(grown, k)) for k in ("label", "weight", "total", "planes"))
    assert fresh.passes == grown.passes == 16 * 2 and (fresh.total > ONE // 2).all()          # every tile: 17 labels, two walks
    assert (fresh.planes > 0).all((1, 2)).sum() >= 17                    # every label of the pattern reaches every pixel


def test_label_views_leave_frames_and_lift_runs_alone(gsx):
    sc = blend_cases.prepared("lengths").scene
    seg, Cm = lift_model.maps(sc.W, sc.H)["blocks"]
    labels, C = labelmap_model.pattern("mod255", len(sc.xyz))
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays(), labels=labels)
        before = c.render_view(sc.cam, sc.W, sc.H)
        first = c.label_view(sc.cam, sc.W, sc.H, C)
        assert c.render_num_pairs() == c.render_num_pairs_consumed() == sum(blend_cases.LENGTHS)   # the first walk's records
        assert np.array_equal(c.render_view(sc.cam, sc.W, sc.H), before)
        c.lift_begin(Cm)
        c.lift_view(sc.cam, seg)
        assert np.array_equal(c.label_view(sc.cam, sc.W, sc.H, C), first)
        c.lift_view(sc.cam, seg)
        assert np.array_equal(c.label_view(sc.cam, sc.W, sc.H, C, 0.5), labelmap_model.finalize(views(gsx, "lengths")["mod255"].planes, 0.5)[0])
        assert c.lift_num_views() == 2 and np.array_equal(c.lift_table(), 2 * lift_gpu.tables(gsx, "lengths")["blocks"])
        assert np.array_equal(c.render_view(sc.cam, sc.W, sc.H), before)
    assert np.array_equal(first, views(gsx, "lengths")["mod255"].label)


@pytest.mark.parametrize("name", NAMES)
def test_pass_count(gsx, name):
    m = blend_cases.prepared(name).model
    WL = gsx.labelmap_constants()["window"]
    for pat, v in views(gsx, name).items():
        labels, _ = labelmap_model.pattern(pat, m.rec.n)
        assert v.passes == labelmap_model.passes(m, labels, WL), pat
    assert views(gsx, name)["one"].passes == sum(1 for ids in m.lists if len(ids))


def test_device_map_goes_into_the_table_kernel(gsx):
    import torch
    p = blend_cases.prepared("edges_47x41")
    sc = p.scene
    seg, Cm = lift_model.maps(sc.W, sc.H)["blocks"]
    labels, C = labelmap_model.pattern("parity", len(sc.xyz))
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays(), labels=labels)
        assert c.label_view(sc.cam, sc.W, sc.H, C, to_host=False) is None
        dev = c.label_map_device()
        assert dev.is_cuda and dev.dtype == torch.int32 and tuple(dev.shape) == (sc.H, sc.W)
        host = views(gsx, "edges_47x41")["parity"].label
        assert np.array_equal(dev.cpu().numpy(), host)
        got = c.label_map_tables([dev], [torch.from_numpy(seg).to("cuda:0")], C, Cm)[0]
        want = np.zeros((C + 1, Cm + 1), np.int64)
        np.add.at(want, (host.reshape(-1) + 1, seg.reshape(-1) + 1), 1)
        assert np.array_equal(got, want) and got.sum() == sc.W * sc.H and (np.count_nonzero(got) > 4)
        # ... and into a lift view and a vote view, as a class map like any other
        c.lift_begin(C)
        c.lift_view(sc.cam, dev)
        from_dev = c.lift_table()
        c.lift_begin(C)
        c.lift_view(sc.cam, host)
        assert np.array_equal(from_dev, c.lift_table()) and from_dev.sum() > 0


def test_errors(gsx):
    GsxError, lib = gsx._lib.GsxError, gsx._lib
    sc = blend_cases.prepared("edges_17x17").scene
    n = len(sc.xyz)
    labels, C = labelmap_model.pattern("parity", n)
    view = lambda c, **kw: c.label_view(sc.cam, kw.pop("W", sc.W), kw.pop("H", sc.H), kw.pop("C", C), **kw)

    def fails(call, code):
        if code in (lib.GSX_E_INVALID, lib.GSX_E_RANGE):
            with pytest.raises(ValueError, match=f"libgsx error {code}:") as e:
                call()
        else:
            with pytest.raises(GsxError) as e:
                call()
            assert e.value.code == code
        return str(e.value)

    with gsx.Context(0) as c:
        assert "no splats uploaded" in fails(lambda: view(c), lib.GSX_E_STATE)                      # before upload_splats
        c.upload_splats(*sc.arrays())
        assert "without labels" in fails(lambda: view(c), lib.GSX_E_STATE)                          # uploaded without labels
        with pytest.raises(RuntimeError):
            c.label_map_device()
        c.upload_splats(*sc.arrays(), labels=labels)
        good = view(c, to_host=True)
        kept = lambda: np.array_equal(c.label_map_device().cpu().numpy(), good)
        c.set_render_edits(hidden=[0])
        assert "edit state" in fails(lambda: view(c), lib.GSX_E_STATE)
        c.clear_render_edits()
        assert kept()
        for kw in ({"W": 0}, {"H": 0}, {"W": -5}, {"C": 0}, {"C": 256}, {"C": -1}, {"min_weight": -1e-9}, {"min_weight": float("nan")},
                   {"min_weight": float("inf")}, {"planes": [C]}, {"planes": [0, -2]}, {"planes": [0] * 257}):
            fails(lambda: view(c, **kw), lib.GSX_E_INVALID)
            assert kept(), kw
        assert "plane 1 " in fails(lambda: view(c, planes=[0, 7]), lib.GSX_E_INVALID)
        assert "4097x16" in fails(lambda: view(c, W=4097, H=16), lib.GSX_E_UNSUPPORTED)
        assert "16x4097" in fails(lambda: view(c, W=16, H=4097), lib.GSX_E_UNSUPPORTED)
        assert kept()
        assert np.array_equal(view(c), good)                                                       # later calls work
        # an uploaded label out of range: the first offending upload row is named, for either side of the range
        for row, value, classes in ((5, C, C), (n - 2, 300, 255), (3, -2, C)):
            wrong = labels.copy()
            wrong[row] = value
            wrong[n - 1] = value if row != n - 2 else wrong[n - 1]                                 # a later offender is not the one named
            c.upload_splats(*sc.arrays(), labels=wrong)
            for _ in range(2):                                                                     # nothing is cached for a failed check
                assert f"upload row {row} " in fails(lambda: view(c, C=classes), lib.GSX_E_RANGE)
            assert kept()
        wrong = labels.copy()
        wrong[7] = C                                                                               # in range for C + 1 classes
        c.upload_splats(*sc.arrays(), labels=wrong)
        assert view(c, C=C + 1).shape == (sc.H, sc.W)
        assert "upload row 7 " in fails(lambda: view(c), lib.GSX_E_RANGE)                           # the check is per n_classes
        assert view(c, C=C + 1).shape == (sc.H, sc.W)
        c.upload_splats(*sc.arrays(), labels=labels)
        assert np.array_equal(view(c), good)
        planes = view(c, planes=[0] * 256, to_host=False)                                          # the most planes a call takes
        assert planes.shape == (256, sc.H, sc.W) and (planes == planes[0]).all() and planes.sum() > 0


@pytest.mark.parametrize("name", NAMES)
def test_planes_against_the_model(gsx, name):
    p = blend_cases.prepared(name)
    m = p.model
    kept = np.zeros(m.rec.n, bool)
    kept[m.walk[:m.rec.n - m.n_epilogue]] = True
    assert m.n_epilogue >= 1 and not kept.all()                          # runSort drops a splat, and the epilogue draws splat 0 again
    worst = {}
    for pat, v in views(gsx, name).items():
        pl = labelmap_model.case_planes(name, pat)
        assert v.planes.shape == pl.planes.shape
        bound = labelmap_model.entry_bound(pl, p.tol, p.alpha_max, blend_cases.bitwise(name))
        dist = np.abs(v.planes.astype(np.float64) / ONE - pl.planes)
        fed = bound > 0
        assert (v.planes[~fed] == 0).all(), pat                          # P = M = 0: exactly nothing
        worst[pat] = float((dist[fed] / bound[fed]).max()) if fed.any() else 0.0
        print(f"{name}: {pat}: worst |planes / 2^20 - model| = {worst[pat]:.3f} x the entry's bound")
        assert (dist <= bound).all(), (pat, worst[pat])
    print(f"{name}: worst |planes / 2^20 - model| as a multiple of its bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
