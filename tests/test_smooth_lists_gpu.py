"""GPU: the list form of the label filter (csrc/smooth.hip: smooth_list_kernel behind gsx_smooth_labels_lists) on constructed
lists, no geometry: every lanes-per-query width (k = 1, 2, 3, 31 .. 64) at sizes around a wave and a workgroup, ties decided
by the own label and by the smallest value, the extremes of int32 as labels, the two flags, min_votes around the winner's
count, the Jacobi update, the early stop, labels_out on top of labels, the context's device lists, and every error.
Everything is integers: equal to tests/smooth_model.py, no tolerance."""
import numpy as np
import pytest

import smooth_model as sm
from smooth_checks import FILL_ONLY, IGNORE, lists_against_model, raw_lists, raw_points

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max
KS = (1, 2, 3, 31, 32, 33, 63, 64)


def model_labels(nbr, L, **kw):
    return sm.run(nbr, np.asarray(L, np.int32), **kw)[0]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_shapes(ctx, n):
    rng = np.random.default_rng(n)
    for k in (k for k in KS if k <= n):
        nbr = rng.integers(0, n, (n, k)).astype(np.int32)                  # repeats inside a row are the rule here
        for values in (2, 3, 300):
            pool = rng.choice(np.arange(-150, 150), values, replace=False).astype(np.int32)
            L = pool[rng.integers(0, values, n)]
            lists_against_model(ctx, nbr, L, f"n {n}, k {k}, {values} values", rounds=3)
            lists_against_model(ctx, nbr, L, f"n {n}, k {k}, {values} values, ignore", rounds=2, ignore_label=int(pool[0]), min_votes=2)


def focus(neighbour_labels, own):
    """point 0 with the given own label, its neighbours 1 .. k carrying neighbour_labels; every other point lists itself k
    times and so keeps its label.  Returns (nbr, L)."""
    k = len(neighbour_labels)
    n = k + 1
    nbr = np.repeat(np.arange(n, dtype=np.int32)[:, None], k, axis=1)
    nbr[0] = np.arange(1, n)
    return nbr, np.array([own] + list(neighbour_labels), np.int32)


TIES = [  # (neighbour labels, own, label after one round)
    ([5, 5, 9, 9], 9, 9), ([5, 5, 9, 9], 5, 5), ([5, 5, 9, 9], 7, 5), ([9, 9, 5, 5], 7, 5),
    ([4, 8, 6, 8, 4, 6], 6, 6), ([4, 8, 6, 8, 4, 6], 8, 8), ([8, 6, 4, 8, 4, 6], 1, 4), ([8, 6, 4, 8, 4, 6, 8], 4, 8),
    ([-3, -3, -8, -8], 0, -8), ([-3, -8, -3, -8], -3, -3), ([-1, 2, -1, 2], 7, -1),
    ([I32_MIN, I32_MAX, I32_MAX, I32_MIN], 0, I32_MIN), ([I32_MAX, I32_MAX, 3], 3, I32_MAX), ([I32_MAX, 3, 3, I32_MAX], 7, 3),
    ([I32_MIN, I32_MAX], I32_MAX, I32_MAX), ([I32_MAX], 0, I32_MAX), ([I32_MIN, I32_MIN, I32_MAX, I32_MAX, 0, 0], 1, I32_MIN),
]


@pytest.mark.parametrize("case", range(len(TIES)))
def test_ties(ctx, case):
    nb_labels, own, want = TIES[case]
    nbr, L = focus(nb_labels, own)
    got, changed, sup = lists_against_model(ctx, nbr, L, TIES[case])
    assert got[0] == want and np.array_equal(got[1:], L[1:])
    assert sup[0] == nb_labels.count(want) and changed == [int(want != own)]


def test_ignore(ctx):
    # own label ignored: it cannot win, however many neighbours carry it
    nbr, L = focus([-1, -1, -1, 4, 6, 6], -1)
    got, _, sup = lists_against_model(ctx, nbr, L, "own ignored", ignore_label=-1)
    assert got[0] == 6 and sup[0] == 2
    got, _, sup = lists_against_model(ctx, nbr, L, "own not ignored")
    assert got[0] == -1 and sup[0] == 3
    # every neighbour ignored: the label is kept, support 0 - also for the points that list only themselves
    nbr, L = focus([-1, -1, -1], 5)
    got, changed, sup = lists_against_model(ctx, nbr, L, "all ignored", ignore_label=-1)
    assert got[0] == 5 and sup[0] == 0 and changed == [0] and (sup[1:] == 0).all()
    nbr, L = focus([-1, -1, -1], -1)
    got, _, sup = lists_against_model(ctx, nbr, L, "all ignored, own too", ignore_label=-1)
    assert got[0] == -1 and sup[0] == 0
    # ignore_label absent from the data: the same answer as without it
    rng = np.random.default_rng(5)
    nbr = rng.integers(0, 257, (257, 9)).astype(np.int32)
    L = rng.integers(0, 4, 257).astype(np.int32)
    a = lists_against_model(ctx, nbr, L, "ignore absent", ignore_label=99, rounds=2)
    b = lists_against_model(ctx, nbr, L, "no ignore", rounds=2)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])


def test_fill_only(ctx):
    rng = np.random.default_rng(6)
    n, k = 1025, 7
    nbr = rng.integers(0, n, (n, k)).astype(np.int32)
    L = rng.integers(-1, 5, n).astype(np.int32)
    got, changed, _ = lists_against_model(ctx, nbr, L, "fill only", ignore_label=-1, fill_only=True, rounds=3)
    assert np.array_equal(got[L != -1], L[L != -1]) and changed[0] > 0 and (got[L == -1] != -1).any()
    with pytest.raises(ValueError):
        ctx.smooth_labels_lists(nbr, L, fill_only=True)
    # the flag on its own: holes are -1, but -1 neighbours vote like any other
    rc, out, sup, ch, done = raw_lists(ctx, n, k, nbr, L, ignore_label=-1, flags=FILL_ONLY)
    want, w_sup = sm.round_rows(nbr, L, fill_only=True, fill_label=-1)
    assert rc == 0 and np.array_equal(out, want) and np.array_equal(sup, w_sup) and ch[0] == (want != L).sum() and done == 1
    rc, out2, _, _, _ = raw_lists(ctx, n, k, nbr, L, ignore_label=-1, flags=FILL_ONLY | IGNORE)
    assert rc == 0 and np.array_equal(out2, sm.round_rows(nbr, L, ignore_label=-1, fill_only=True)[0]) and not np.array_equal(out2, out)


def test_min_votes(ctx):
    nbr, L = focus([3, 3, 3, 8, 8], 1)                                  # the winner 3 has m = 3 votes, k = 5
    k, m = 5, 3
    for mv in (1, m, m + 1, k, k + 1):
        got, changed, sup = lists_against_model(ctx, nbr, L, f"min_votes {mv}", min_votes=mv)
        assert got[0] == (3 if mv <= m else 1) and sup[0] == (3 if mv <= m else 0)
        assert np.array_equal(got[1:], L[1:])
    rng = np.random.default_rng(7)
    nbr = rng.integers(0, 300, (300, 10)).astype(np.int32)
    L = rng.integers(0, 3, 300).astype(np.int32)
    for mv in (1, 4, 5, 6, 10, 11):
        lists_against_model(ctx, nbr, L, f"random, min_votes {mv}", min_votes=mv, rounds=2)


def test_jacobi_ring(ctx):
    """alternating labels on a ring, lists {i-1, i, i+1}: every point is outvoted 2:1 in every round.  An update in place
    would let point 1 see point 0's new label and stay."""
    i = np.arange(64)
    nbr = np.stack(((i - 1) % 64, i, (i + 1) % 64), axis=1).astype(np.int32)
    L = np.where(i % 2 == 0, 11, 22).astype(np.int32)
    one, changed, _ = lists_against_model(ctx, nbr, L, "ring, 1 round")
    assert np.array_equal(one, np.where(i % 2 == 0, 22, 11)) and changed == [64]
    two, changed, sup = lists_against_model(ctx, nbr, L, "ring, 2 rounds", rounds=2)
    assert np.array_equal(two, L) and changed == [64, 64] and (sup == 2).all() and ctx.smooth_rounds_done == 2


def test_early_stop(ctx):
    i = np.arange(64)
    nbr = np.stack(((i - 1) % 64, i, (i + 1) % 64), axis=1).astype(np.int32)
    L = np.full(64, 4, np.int32)
    got, changed, _ = lists_against_model(ctx, nbr, L, "uniform", rounds=5)
    assert changed == [0, 0, 0, 0, 0] and ctx.smooth_rounds_done == 1 and np.array_equal(got, L)
    L[20] = 9                                                            # gone after round 1, round 2 finds nothing to do
    got, changed, _ = lists_against_model(ctx, nbr, L, "one outlier", rounds=5)
    assert changed == [1, 0, 0, 0, 0] and ctx.smooth_rounds_done == 2 and (got == 4).all()
    rc, _, _, ch, done = raw_lists(ctx, 64, 3, nbr, L, rounds=5)
    assert rc == 0 and done == 2 and ch.tolist() == [1, 0, 0, 0, 0]      # the entries behind the last round are written too


def test_labels_out_may_be_labels(ctx):
    rng = np.random.default_rng(8)
    nbr = rng.integers(0, 500, (500, 12)).astype(np.int32)
    L = rng.integers(0, 4, 500).astype(np.int32)
    want, w_changed, w_done, w_sup = sm.run(nbr, L, rounds=3)
    buf = L.copy()
    rc, out, sup, ch, done = raw_lists(ctx, 500, 12, nbr, buf, rounds=3, out=buf)
    assert rc == 0 and out is buf and np.array_equal(buf, want) and np.array_equal(sup, w_sup) and ch.tolist() == w_changed and done == w_done
    rc, out, sup, ch, done = raw_lists(ctx, 500, 12, nbr, L, rounds=3, want_support=False, want_changed=False)   # optional outputs NULL
    assert rc == 0 and np.array_equal(out, want) and done == w_done


def test_device_lists(ctx, gsx):
    rng = np.random.default_rng(9)
    pts = rng.uniform(-1, 1, (700, 3)).astype(np.float32)
    L = rng.integers(-1, 4, 700).astype(np.int32)
    nbr = ctx.knn(pts, 9)
    host = ctx.smooth_labels_lists(nbr, L, rounds=3, ignore_label=-1, return_support=True)
    dev = ctx.smooth_labels_lists(None, L, k=9, rounds=3, ignore_label=-1, return_support=True)
    assert np.array_equal(host[0], dev[0]) and host[1] == dev[1] and np.array_equal(host[2], dev[2])
    assert np.array_equal(host[0], model_labels(nbr, L, rounds=3, ignore_label=-1))
    for n, k in ((700, 8), (699, 9)):                                    # the lists on the context are of another k, another n
        with pytest.raises(gsx.GsxError) as e:
            ctx.smooth_labels_lists(None, L[:n], k=k)
        assert e.value.code == gsx._lib.GSX_E_STATE
    ctx.knn(pts[:699], 9)
    with pytest.raises(gsx.GsxError) as e:
        ctx.smooth_labels_lists(None, L, k=9)
    assert e.value.code == gsx._lib.GSX_E_STATE
    got = ctx.smooth_labels_lists(None, L[:699], k=9)[0]
    assert np.array_equal(got, model_labels(ctx.knn(pts[:699], 9), L[:699]))


def test_errors(ctx, gsx):
    E = gsx._lib
    n, k = 100, 5
    rng = np.random.default_rng(10)
    nbr = rng.integers(0, n, (n, k)).astype(np.int32)
    L = rng.integers(0, 3, n).astype(np.int32)
    pts = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    ctx.profile(True)
    try:
        def lists(code, **kw):
            a = dict(n=n, k=k, knn=nbr, labels=L)
            a.update(kw)
            rc, out, _, _, _ = raw_lists(ctx, **a)
            assert rc == code, (kw, rc, ctx._lib.gsx_last_error(ctx.h))
            assert (out == -77).all()                                       # nothing was written

        lists(E.GSX_E_INVALID, labels=None)
        rc = ctx._lib.gsx_smooth_labels_lists(ctx.h, n, k, nbr.ctypes.data, L.ctypes.data, 1, 1, 0, 0, None, None, None, None)
        assert rc == E.GSX_E_INVALID
        lists(E.GSX_E_INVALID, n=0)
        lists(E.GSX_E_INVALID, k=0)
        lists(E.GSX_E_INVALID, n=4, k=5)                                    # k > n
        lists(E.GSX_E_INVALID, n=n, k=65, knn=rng.integers(0, n, (n, 65)).astype(np.int32))
        lists(E.GSX_E_INVALID, rounds=0)
        lists(E.GSX_E_INVALID, min_votes=0)
        lists(E.GSX_E_INVALID, flags=4)
        lists(E.GSX_E_UNSUPPORTED, n=1 << 31)                               # refused before an array is read
        for bad in (-1, n, I32_MAX, I32_MIN):
            b = nbr.copy()
            b[n - 1, k - 1] = bad
            lists(E.GSX_E_INVALID, knn=b)
            assert b"row 99, column 4" in ctx._lib.gsx_last_error(ctx.h)
        ctx.knn(pts, 6)
        lists(E.GSX_E_STATE, knn=None)

        def points(code, **kw):
            a = dict(n=n, points=pts, labels=L, k=k)
            a.update(kw)
            rc, out, _, _, _ = raw_points(ctx, **a)
            assert rc == code, (kw, rc, ctx._lib.gsx_last_error(ctx.h))
            assert (out == -77).all()

        ctx.profile(True)                                                   # forget the knn above
        points(E.GSX_E_INVALID, points=None)
        points(E.GSX_E_INVALID, labels=None)
        points(E.GSX_E_INVALID, n=0)
        points(E.GSX_E_INVALID, k=0)
        points(E.GSX_E_INVALID, k=n + 1)
        points(E.GSX_E_INVALID, rounds=0)
        points(E.GSX_E_INVALID, min_votes=0)
        points(E.GSX_E_INVALID, flags=8)
        points(E.GSX_E_UNSUPPORTED, n=1 << 31)
        for v in (np.nan, np.inf, -np.inf):
            bad = pts.copy()
            bad[n - 1, 2] = v
            points(E.GSX_E_INVALID, points=bad)
            points(E.GSX_E_INVALID, points=bad, k=70)
        big = np.zeros((65537, 3), np.float32)
        points(E.GSX_E_UNSUPPORTED, n=65537, points=big, labels=np.zeros(65537, np.int32), k=65536)
        # every error came back before a launch: no kernel of the search or of the filter has run
        for name in ("smooth_list", "smooth_search", "nn_knn"):
            assert ctx.profile_get(name)[0] == 0, name
        rc, out, _, _, _ = raw_points(ctx, n, pts, L, k)                    # ... and the counters would have seen one
        assert rc == 0 and ctx.profile_get("smooth_list")[0] == 1 and ctx.profile_get("nn_knn")[0] == 1
        assert np.array_equal(out, model_labels(ctx.knn(pts, k), L))
    finally:
        ctx.profile(False)
    assert ctx._lib.gsx_smooth_labels_lists(None, n, k, nbr.ctypes.data, L.ctypes.data, 1, 1, 0, 0, L.ctypes.data, None, None, None) == E.GSX_E_INVALID
