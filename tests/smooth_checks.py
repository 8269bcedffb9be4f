"""What the label filter's GPU tests share: the two C entry points called through ctypes with every argument in the test's
hand (return code and all four outputs come back), and the comparison of a call with tests/smooth_model.py."""
import ctypes as C

import numpy as np

import smooth_model as sm

IGNORE, FILL_ONLY = 1, 2


def ptr(a):
    return None if a is None else a.ctypes.data


def raw_lists(ctx, n, k, knn, labels, rounds=1, min_votes=1, ignore_label=0, flags=0, out=None, want_support=True, want_changed=True):
    """gsx_smooth_labels_lists as it is -> (rc, labels_out, support, changed, rounds_done); out: the labels_out array to use"""
    size = min(max(n, 0), 1 << 20)                    # an n the call must refuse gets no array of its size
    out = np.full(size, -77, np.int32) if out is None else out
    sup = np.full(size, -77, np.int32) if want_support else None
    ch = np.full(max(rounds, 0), -77, np.int64) if want_changed else None
    done = C.c_int32(-77)
    rc = ctx._lib.gsx_smooth_labels_lists(ctx.h, n, k, ptr(knn), ptr(labels), rounds, min_votes, ignore_label, flags, ptr(out), ptr(sup),
                                          ptr(ch), C.byref(done))
    return rc, out, sup, ch, done.value


def raw_points(ctx, n, points, labels, k, rounds=1, min_votes=1, ignore_label=0, flags=0, out=None):
    size = min(max(n, 0), 1 << 20)
    out = np.full(size, -77, np.int32) if out is None else out
    sup = np.full(size, -77, np.int32)
    ch = np.full(max(rounds, 0), -77, np.int64)
    done = C.c_int32(-77)
    rc = ctx._lib.gsx_smooth_labels(ctx.h, n, ptr(points), ptr(labels), k, rounds, min_votes, ignore_label, flags, ptr(out), ptr(sup),
                                    ptr(ch), C.byref(done))
    return rc, out, sup, ch, done.value


def lists_against_model(ctx, nbr, L, what, **kw):
    """Context.smooth_labels_lists on every row against the model: labels, support, changed per round, rounds executed"""
    got, changed, sup = ctx.smooth_labels_lists(nbr, L, return_support=True, **kw)
    want, w_changed, w_done, w_sup = sm.run(nbr, L, **kw)
    assert np.array_equal(got, want), (what, int((got != want).sum()))
    assert np.array_equal(sup, w_sup), what
    assert changed == w_changed and ctx.smooth_rounds_done == w_done, (what, changed, w_changed)
    return got, changed, sup
