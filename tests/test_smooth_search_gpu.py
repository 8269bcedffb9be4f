"""GPU: gsx_smooth_labels on geometry - both forms of a round (csrc/smooth.hip) at the structural edges of the search they
share with gsx_knn / gsx_normals, i.e. on every scene of tests/nn_cases.py: both caps of the grid sizing, queries on cell
faces, a ring that doubles, a sampled bounding box, duplicated positions where only the index decides the neighbour set,
n below one workgroup's four queries, k = n and k > 64.  The neighbour sets are the model's (nn_cases.model_lists /
region_growing_model.knn), the rule is tests/smooth_model.py, and everything is integers: equal, no tolerance.

The default path runs lists for k <= 64 and searches for k > 64; option "smooth_search" forces the search form, option
"nn_brute" the exhaustive grid.  Neither may change a label, a support count or a changed count."""
import numpy as np
import pytest

import nn_cases as cases
import region_growing_model as model
import smooth_model as sm

pytestmark = pytest.mark.gpu

SCENES = cases.scenes()
VALUES = np.array([3, 7, -5, 40, 12], np.int32)
_RESULTS = {}
_BROKEN = []


def scene_labels(name):
    """a seeded draw from 5 values, 10 % of the points unlabelled"""
    rng = np.random.default_rng(sum(name.encode()))
    n = len(SCENES[name].pts)
    L = VALUES[rng.integers(0, 5, n)]
    L[rng.random(n) < 0.1] = -1
    return L


def ks_of(sc):
    return sorted(set(sc.k_knn + sc.k_normals))


def gpu(ctx, name, k, search=False, brute=False):
    """one round with -1 ignored, made once per (scene, k, form, grid) and shared: (labels, changed, support).  Once a call has
    raised, no test of this module goes to the GPU again."""
    if _BROKEN:
        pytest.fail(f"an earlier GPU call of this module failed ({_BROKEN[0]}): nothing more is started")
    key = (name, k, search, brute)
    if key not in _RESULTS:
        try:
            ctx.set_option("nn_brute", int(brute))
            ctx.set_option("smooth_search", int(search))
            _RESULTS[key] = ctx.smooth_labels(SCENES[name].pts, scene_labels(name), k=k, ignore_label=-1, return_support=True)
            ctx.set_option("nn_brute", 0)
            ctx.set_option("smooth_search", 0)
        except BaseException as e:
            _BROKEN.append(f"{name}, k = {k}, search {search}, brute {brute}: {type(e).__name__}: {e}")
            raise
    return _RESULTS[key]


@pytest.mark.parametrize("name", cases.NAMES)
def test_scenes_against_the_model(ctx, name):
    sc = SCENES[name]
    q = np.arange(len(sc.pts)) if sc.queries is None else sc.queries
    L = scene_labels(name)
    nbr, _ = cases.model_lists(name)
    for k in ks_of(sc):
        want, w_sup = sm.round_rows(nbr[:, :k], L, q, ignore_label=-1)
        got, changed, sup = gpu(ctx, name, k)
        assert np.array_equal(got[q], want), (name, k, int((got[q] != want).sum()))
        assert np.array_equal(sup[q], w_sup), (name, k)
        assert changed == [int((got != L).sum())]
        if sc.queries is None:
            assert changed == [int((want != L).sum())]


@pytest.mark.parametrize("name", cases.NAMES)
def test_both_forms_agree_with_the_grid_and_without(ctx, name):
    sc = SCENES[name]
    for k in (k for k in ks_of(sc) if k <= 64):
        ref = gpu(ctx, name, k)
        for search, brute in ((True, False), (False, True), (True, True)):
            got = gpu(ctx, name, k, search, brute)
            assert np.array_equal(got[0], ref[0]) and got[1] == ref[1] and np.array_equal(got[2], ref[2]), (name, k, search, brute)


def blobs():
    """3000 points in four blobs, labelled by blob, 10 % of the labels redrawn"""
    rng = np.random.default_rng(77)
    which = rng.integers(0, 4, 3000)
    centres = np.float64([[0, 0, 0], [3, 0, 0], [0, 3, 0], [0, 0, 3]])
    pts = (centres[which] + rng.normal(0, 0.5, (3000, 3))).astype(np.float32)
    L = (10 * (which + 1)).astype(np.int32)
    flip = rng.random(3000) < 0.1
    L[flip] = 10 * rng.integers(1, 5, int(flip.sum()))
    return pts, L


MULTI = [n for n in cases.NAMES if n.startswith("small-")] + ["blobs"]
_LISTS = {}


def full_lists(name, pts, k):
    """the model's lists of every point, computed once at the largest k asked for (a smaller k is a prefix)"""
    if name not in _LISTS:
        _LISTS[name] = model.knn(pts, min(65, len(pts)))[0]
    return _LISTS[name][:, :k]


@pytest.mark.parametrize("name", MULTI)
def test_rounds_against_the_model(ctx, name):
    pts, L = blobs() if name == "blobs" else (SCENES[name].pts, scene_labels(name))
    n = len(pts)
    any_change = False
    for k in sorted({min(8, n), min(65, n)}):
        nbr = full_lists(name, pts, k)
        for kw in (dict(), dict(ignore_label=-1, min_votes=2), dict(ignore_label=-1, fill_only=True)):
            want, w_changed, w_done, w_sup = sm.run(nbr, L, rounds=4, **kw)
            any_change = any_change or w_changed[0] > 0
            for search in ((False, True) if k <= 64 else (False,)):
                ctx.set_option("smooth_search", int(search))
                got, changed, sup = ctx.smooth_labels(pts, L, k=k, rounds=4, return_support=True, **kw)
                ctx.set_option("smooth_search", 0)
                what = (name, k, kw, search)
                assert np.array_equal(got, want), what
                assert changed == w_changed and ctx.smooth_rounds_done == w_done, (what, changed, w_changed)
                assert np.array_equal(sup, w_sup), what
    if name == "blobs":
        assert any_change                                                # the scene does exercise a change


def test_class_limit(ctx, gsx):
    rng = np.random.default_rng(78)
    n = 4200
    pts = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    nbr = model.knn(pts, 65)[0]
    spread = rng.permutation(np.arange(-3000, 3000, dtype=np.int32))     # distinct, negative ones among them
    for distinct in (4096, 4097):
        L = spread[rng.permutation(n) % distinct]
        assert len(np.unique(L)) == distinct
        if distinct == 4096:
            got, changed, sup = ctx.smooth_labels(pts, L, k=65, return_support=True)
            want, w_sup = sm.round_rows(nbr, L)
            assert np.array_equal(got, want) and np.array_equal(sup, w_sup) and changed == [int((want != L).sum())]
        else:
            ctx.profile(True)
            try:
                for k, forced in ((65, 0), (64, 1)):
                    ctx.set_option("smooth_search", forced)
                    with pytest.raises(gsx.GsxError) as e:
                        ctx.smooth_labels(pts, L, k=k)
                    ctx.set_option("smooth_search", 0)
                    assert e.value.code == gsx._lib.GSX_E_UNSUPPORTED and "4097" in str(e.value)
                assert ctx.profile_get("smooth_search")[0] == 0           # refused before a launch
            finally:
                ctx.set_option("smooth_search", 0)
                ctx.profile(False)
            got, changed, sup = ctx.smooth_labels(pts, L, k=64, return_support=True)   # lists compare raw labels: no limit
            want, w_sup = sm.round_rows(nbr[:, :64], L)
            assert np.array_equal(got, want) and np.array_equal(sup, w_sup) and changed == [int((want != L).sum())]


def test_two_runs_are_identical(ctx):
    pts, L = blobs()
    for k, search in ((16, 0), (16, 1), (100, 0)):
        ctx.set_option("smooth_search", search)
        a = ctx.smooth_labels(pts, L, k=k, rounds=3, ignore_label=-1, return_support=True)
        b = ctx.smooth_labels(pts, L, k=k, rounds=3, ignore_label=-1, return_support=True)
        ctx.set_option("smooth_search", 0)
        assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2].tobytes() == b[2].tobytes()
