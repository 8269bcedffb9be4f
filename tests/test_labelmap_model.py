"""The label frames' fp64 model (tests/labelmap_model.py) is what it claims, CPU only, before test_labelmap_gpu.py holds the HIP
kernel to it on the same scenes (tests/blend_cases.py) and label patterns.

Transpose identity: the model's planes and lift_model's table scatter the same weights, one by the splat's label, the other by
the pixel's class, so for every scene, every map of lift_model.maps and every pattern
    sum over {p: seg[p] = c} of plane[b][p]  ==  sum over {i: label[i] = b - 1} of table[i][c + 1]      to 1e-12 relative.

Leave-one-out (lengths, needles, edges - the families whose every listed record with a fragment is visible; behind the walls'
closed faces a record's weight is zero by construction): the list is evaluated again without the record, and some
(bin, pixel) entry moves by at least ten times the bound test_labelmap_gpu.py allows that entry.  Under mod255, as the lift's
model test uses its 255-class map: an entry's bound grows with P, the fragments it sums, and one record's weight does not, so
one record can only stand out of an entry that holds about one record per pixel.  Where a 513-record list shares one label the
entry is the frame's alpha and a record deep in the list moves it by less than its bound (measured on `lengths`, smallest
best-entry change in bounds: one 0.36, parity 0.85, mod15 .. mod17 6.4 .. 7.4, mod33 14, mod255 112) - there the exact
tests of test_labelmap_gpu.py hold the kernel, not the bound.

The integer rule: ties go to the lowest bin, bin 0 = label -1 among them; the threshold is max(1, ceil(min_weight 2^20)), met
exactly at the total; an all-zero pixel is -1 with weight 0 at any min_weight."""
import functools

import numpy as np
import pytest

import blend_cases
import labelmap_model
import lift_model

NAMES = list(blend_cases.all_cases())


@functools.lru_cache(maxsize=None)
def lifted(name, key):
    m = blend_cases.prepared(name).model
    seg, C = lift_model.maps(m.W, m.H)[key]
    return lift_model.lift(m, seg, C)


def one_hot(values, n):
    out = np.zeros((len(values), n))
    out[np.arange(len(values)), values] = 1.0
    return out


def test_patterns(gsx):
    WL = gsx.labelmap_constants()["window"]
    names = labelmap_model.pattern_names(WL)
    assert len(names) == len(set(names)) == 8 and WL >= 2
    for pat in names:
        labels, C = labelmap_model.pattern(pat, 1000)
        assert labels.dtype == np.int32 and labels.min() >= -1 and labels.max() < C and 1 <= C <= 255
    assert len(np.unique(labelmap_model.pattern("mod255", 1000)[0])) == 255
    for K in (WL - 1, WL, WL + 1, 2 * WL + 1):
        assert len(np.unique(labelmap_model.pattern(f"mod{K}", 1000)[0])) == K
    # importance order is not upload order: a pattern given per upload row is a different one per record
    p = blend_cases.prepared("lengths")
    assert not np.array_equal(p.packed, np.arange(p.model.rec.n))
    # the tiles hold what the kernel's window edges need: lists with fewer, exactly and more bins than one window, and all 255
    for name, want in (("lengths", 255), ("walls_80x48", 255), ("walls_65x53", 255)):
        m = blend_cases.prepared(name).model
        assert max(labelmap_model.tile_bins(m, labelmap_model.pattern("mod255", m.rec.n)[0])) == want
    m = blend_cases.prepared("lengths").model
    for K in (WL - 1, WL, WL + 1, 2 * WL + 1):
        assert max(labelmap_model.tile_bins(m, labelmap_model.pattern(f"mod{K}", m.rec.n)[0])) == K
    D = labelmap_model.tile_bins(m, labelmap_model.pattern("mod255", m.rec.n)[0])
    assert labelmap_model.passes(m, labelmap_model.pattern("mod255", m.rec.n)[0], WL) == sum(-(-d // WL) for d in D) > len(D)


@pytest.mark.parametrize("name", NAMES)
def test_transpose_identity(gsx, name):
    m = blend_cases.prepared(name).model
    worst = 0.0
    for pat in labelmap_model.pattern_names(gsx.labelmap_constants()["window"]):
        labels, nc = labelmap_model.pattern(pat, m.rec.n)
        pl = labelmap_model.case_planes(name, pat)
        by_bin = one_hot(labelmap_model.packed_bins(m, labels), nc + 1)               # (n, bins)
        assert (pl.planes >= 0).all() and (pl.planes[pl.P == 0] == 0).all()
        for key, (seg, C) in lift_model.maps(m.W, m.H).items():
            left = pl.planes.reshape(nc + 1, -1) @ one_hot(seg.reshape(-1) + 1, C + 1)  # (bins, classes)
            right = by_bin.T @ lifted(name, key).table
            scale = np.maximum(np.abs(left), np.abs(right))
            assert (np.abs(left - right) <= 1e-12 * scale).all(), (pat, key)
            if scale.max() > 0:
                worst = max(worst, float((np.abs(left - right)[scale > 0] / scale[scale > 0]).max()))
    print(f"{name}: largest relative distance between the two scatters {worst:.2e}")


@pytest.mark.parametrize("name", [n for n in NAMES if blend_cases.family(n) in ("lengths", "needles", "edges")])
def test_every_record_moves_an_entry_by_ten_bounds(gsx, name):
    p = blend_cases.prepared(name)
    m = p.model
    least, checked = {}, 0
    for pat in ("mod255",):
        labels, nc = labelmap_model.pattern(pat, m.rec.n)
        bins = labelmap_model.packed_bins(m, labels)
        pl = labelmap_model.case_planes(name, pat)
        bound = labelmap_model.entry_bound(pl, p.tol, p.alpha_max, blend_cases.bitwise(name))
        least[pat] = np.inf
        for t, ids in enumerate(m.lists):
            if len(ids) == 0:
                continue
            ys, xs, inside = m.tile_pixels(t)
            w = lift_model.tile_weights(m, t)
            frag = m.has_fragment(t)
            present, slot = np.unique(bins[ids], return_inverse=True)
            hot = one_hot(slot, len(present)).T                                       # (bins in the list, L)
            tile_bound = bound[present][:, np.minimum(ys, m.H - 1), np.minimum(xs, m.W - 1)]    # (bins, 16, 16)
            for k in np.flatnonzero(frag):
                moved = np.abs(hot @ (lift_model.tile_weights(m, t, skip=k) - w).reshape(len(ids), -1)).reshape(tile_bound.shape)
                hit = inside[None] & (tile_bound > 0)
                assert (moved[~hit] == 0).all()
                least[pat] = min(least[pat], float((moved[hit] / tile_bound[hit]).max()))
                checked += 1
    print(f"{name}: {checked} records with a fragment; the best entry moves by at least " +
          ", ".join(f"{k} {v:.0f}" for k, v in least.items()) + " x its bound")
    assert checked and min(least.values()) >= 10.0


def test_integer_rule():
    ONE = lift_model.ONE
    q = np.zeros((4, 1, 6), np.uint32)
    q[:, 0, 1] = (5, 5, 1, 0)           # a tie of bins 0 and 1: label -1 wins it
    q[:, 0, 2] = (1, 7, 7, 0)           # a tie of bins 1 and 2: label 0
    q[:, 0, 3] = (0, 0, 0, 3)           # one bin
    q[:, 0, 4] = (0, 0, ONE, 700)       # beyond 2^20: half a unit per fragment on top
    q[:, 0, 5] = (0, 1, 0, 0)           # the smallest total there is
    label, weight, total = labelmap_model.finalize(q, 0.0)
    assert label.dtype == np.int32 and weight.dtype == np.uint32 and total.dtype == np.uint32
    assert label.tolist() == [[-1, -1, 0, 2, 1, 0]] and weight.tolist() == [[0, 5, 7, 3, ONE, 1]]
    assert total.tolist() == [[0, 11, 15, 3, ONE + 700, 1]]
    # the threshold: max(1, ceil(min_weight * 2^20)) - kept exactly at the total, dropped one above; the total is reported either way
    assert labelmap_model.threshold(0.0) == 1 and labelmap_model.threshold(1e-3) == 1049 and labelmap_model.threshold(1.0) == ONE
    for mw, want_l, want_w in ((3 / ONE, [-1, -1, 0, 2, 1, -1], [0, 5, 7, 3, ONE, 0]), (3.5 / ONE, [-1, -1, 0, -1, 1, -1], [0, 5, 7, 0, ONE, 0]),
                               (15 / ONE, [-1, -1, 0, -1, 1, -1], [0, 0, 7, 0, ONE, 0]), (1.0, [-1, -1, -1, -1, 1, -1], [0, 0, 0, 0, ONE, 0]),
                               (1.5, [-1] * 6, [0] * 6)):
        label, weight, again = labelmap_model.finalize(q, mw)
        assert label.tolist() == [want_l] and weight.tolist() == [want_w] and np.array_equal(again, total), mw
    # all zero: -1 and 0 everywhere, at any min_weight
    for mw in (0.0, 0.5, 2.0):
        label, weight, total = labelmap_model.finalize(np.zeros((256, 3, 5), np.uint32), mw)
        assert (label == -1).all() and (weight == 0).all() and (total == 0).all()
