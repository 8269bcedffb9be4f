"""The lifting labeler's fp64 model (tests/lift_model.py) is what it claims, CPU only, before test_lift_gpu.py holds the HIP
kernel to it on the same scenes (tests/blend_cases.py).

Alpha identity: the weights are the increments of the frame's alpha channel, so a table sums to the alpha the tiles' lists
leave behind - on every case, against the alpha before the epilogue's draws of splat 0 (which add to the frame but not to the
table), and against BlendModel.frame itself on a scene whose epilogue reaches no pixel.

Walls, measured on the model (uniform map): behind the closed walls of walls_80x48 / walls_65x53 the largest row total of a
loud record is 2.4e-6 / 1.0e-6 (bound 1e-3; 4200 / 5700 records), 400 x below it.  Through the hole the loud records in FRONT
show: the three nearest of each corner hold 0.45 .. 0.98 / 0.40 .. 1.03, 400 x above it, and 89 / 91 of the 300 more than
1e-2 - 75 opaque records share each corner pixel and hide one another in turn, which is the rule at work, not a leak.
min_weight = 1e-3 labels every record behind a wall -1 and every one in front with its class.  A centre-projecting vote gives
all of them the class at their centre.

Leave-one-out (lengths, needles, edges; the map with 255 classes, own row, closed form): the removed record's own cells lose
its weights; the best cell lies at least 223 x its GPU tolerance away (lengths; needles 336 x, edges 522 .. 2277 x)."""
import numpy as np
import pytest

import blend_cases
import lift_model
from blend_model import BlendModel

NAMES = list(blend_cases.all_cases())


def alpha_before_epilogue(m):
    return sum(float(m.alpha_after(t)[len(m.lists[t])][m.tile_pixels(t)[2]].sum()) for t in range(len(m.lists)))


def plain_scene():
    """40x24, in-tile records on three tiles; splat 0 (the largest importance) lies far outside the frame, so the epilogue's
    draws of it reach no pixel"""
    rng = np.random.default_rng(20270)
    sc = blend_cases.Scene("plain", 40, 24)
    sc.add(-900.0, 12.0, 3.0, (40.0, 40.0, 40.0), (1, 0, 0, 0), 200, (10, 200, 30))
    for tx, ty, cnt in ((0, 0, 30), (1, 0, 70), (2, 1, 20), (1, 1, 45)):
        blend_cases.add_in_tile(sc, rng, tx, ty, cnt, 3.2, 5.0, lambda r: int(r.integers(2, 60)))
    blend_cases.add_sink(sc)
    return sc


@pytest.mark.parametrize("name", NAMES)
def test_table_sums_to_the_alpha_the_lists_leave(name):
    m = blend_cases.prepared(name).model
    for key in ("uniform", "c255"):
        seg, C = lift_model.maps(m.W, m.H)[key]
        L = lift_model.lift(m, seg, C)
        want = alpha_before_epilogue(m)
        assert want > 1.0 and abs(L.table.sum() - want) <= 1e-9 * want, (key, L.table.sum(), want)
        assert (L.table >= 0).all() and (L.table[L.P == 0] == 0).all()


def test_table_sums_to_the_frames_alpha_without_an_epilogue():
    sc = plain_scene()
    m = BlendModel(*sc.args())
    assert m.n_epilogue == 1 and np.argsort(m.rec.order)[0] == 0
    for t in range(len(m.lists)):                                        # the epilogue's record puts no fragment anywhere
        assert 0 not in m.lists[t]
        assert (m.tile_terms(t)[1][len(m.lists[t]):] == 0).all()
    seg, C = lift_model.maps(m.W, m.H)["blocks"]
    L = lift_model.lift(m, seg, C)
    want = float(m.frame[..., 3].sum())
    assert want > 10.0 and abs(L.table.sum() - want) <= 1e-9 * want


@pytest.mark.parametrize("name", ["needles", "walls_65x53", "edges_47x41", "epilogue_3_opaque"])
def test_a_map_splits_and_never_loses(name):
    m = blend_cases.prepared(name).model
    all_maps = lift_model.maps(m.W, m.H)
    base = lift_model.lift(m, *all_maps["uniform"])
    for key, (seg, C) in all_maps.items():
        L = lift_model.lift(m, seg, C)
        np.testing.assert_allclose(L.table.sum(1), base.table.sum(1), rtol=1e-12, atol=1e-15, err_msg=key)
        assert (L.P.sum(1) == base.P.sum(1)).all() and (L.M.sum(1) == base.M.sum(1)).all()
    # class 1 of `blocks` split in two by pixel parity (classes 1 and 4; C = 5): its cells split, nothing else moves
    seg, C = all_maps["blocks"]
    r, x = np.mgrid[0:m.H, 0:m.W]
    split = np.where((seg == 1) & ((r + x) % 2 == 1), 4, seg)
    assert (split == 4).any() and (split == 1).any()
    a, b = lift_model.lift(m, seg, 5), lift_model.lift(m, split, 5)
    np.testing.assert_allclose(b.table[:, 2] + b.table[:, 5], a.table[:, 2], rtol=1e-12, atol=1e-15)
    assert a.table[:, 2].sum() > 1.0 and b.table[:, 5].sum() > 0.1 and (a.table[:, 5] == 0).all()
    for col in (0, 1, 3, 4):
        assert np.array_equal(a.table[:, col], b.table[:, col])


@pytest.mark.parametrize("name", ["walls_80x48", "walls_65x53"])
def test_walls_hide_what_the_vote_would_label(name):
    p = blend_cases.prepared(name)
    m, meta = p.model, p.scene.meta
    seg, C = lift_model.maps(m.W, m.H)["uniform"]
    L = lift_model.lift(m, seg, C)
    total = L.upload_rows(L.table).sum(1)
    hidden = np.array([i for t, (_, _, loud) in meta["tags"].items() if t != meta["hole"] for i in loud])
    loud = np.array(meta["tags"][meta["hole"]][2])                    # 75 per corner of the hole, record k on corner k % 4
    z = np.array(p.scene.xyz)[:, 2]
    seen = np.concatenate([loud[c::4][np.argsort(z[loud[c::4]])[:3]] for c in range(4)])   # the three nearest of each corner
    assert len(hidden) >= 4000 and len(loud) == blend_cases.N_LOUD
    print(f"{name}: {len(hidden)} loud records behind closed walls, largest row total {total[hidden].max():.2e}; through the "
          f"hole the three nearest of each corner hold {total[seen].min():.2f} .. {total[seen].max():.2f}, "
          f"{int((total[loud] > 1e-2).sum())} of {len(loud)} more than 1e-2")
    assert total[hidden].max() < 1e-3
    # the hole shows its loud records - those in FRONT: 75 opaque records share a corner pixel and hide one another in turn
    assert total[seen].min() > 0.3 and (total[loud] > 1e-2).sum() >= 80
    ints = np.rint(L.upload_rows(L.table) * lift_model.ONE).astype(np.uint64)
    labels, share = lift_model.finalize(ints, 1e-3)
    assert (labels[hidden] == -1).all() and (labels[seen] == 2).all() and (share[seen] == 1.0).all()
    assert np.array_equal(labels[loud] == 2, ints[loud].sum(1) >= lift_model.threshold(1e-3))
    assert (lift_model.finalize(ints, 0.0)[0][hidden][ints[hidden].sum(1) > 0] == 2).all()


@pytest.mark.parametrize("name", [n for n in NAMES if blend_cases.family(n) in ("lengths", "needles", "edges")])
def test_every_record_moves_a_cell_by_ten_tolerances(name):
    p = blend_cases.prepared(name)
    m = p.model
    seg, C = lift_model.maps(m.W, m.H)["c255"]
    L = lift_model.lift(m, seg, C)
    bound = lift_model.cell_bound(L, p.tol, p.alpha_max, blend_cases.bitwise(name))
    least, checked = np.inf, 0
    for t, ids in enumerate(m.lists):
        if len(ids) == 0:
            continue
        ys, xs, inside = m.tile_pixels(t)
        w = lift_model.tile_weights(m, t)
        bins = np.where(inside, seg[np.minimum(ys, m.H - 1), np.minimum(xs, m.W - 1)] + 1, 0)
        frag = m.has_fragment(t)
        for k, i in enumerate(ids):
            if not frag[k]:
                assert w[k].sum() == 0.0
                continue
            lost = np.zeros(C + 1)                      # what row i loses when the record leaves this tile's list
            np.add.at(lost, bins[inside], w[k][inside])
            hit = lost > 0
            least = min(least, float((lost[hit] / bound[i][hit]).max()))
            checked += 1
    print(f"{name}: {checked} records with a fragment, smallest best-cell change {least:.1f} x the cell's tolerance")
    assert checked and least >= 10.0


def test_closed_form_is_a_second_evaluation():
    """leaving a record out of the model moves its own row by exactly its weights, and rows in front of it by nothing"""
    m = blend_cases.prepared("edges_33x40").model
    seg, C = lift_model.maps(m.W, m.H)["checker"]
    full = lift_model.lift(m, seg, C)
    t = max(range(len(m.lists)), key=lambda t: len(m.lists[t]))
    k = len(m.lists[t]) // 2
    less = lift_model.lift(m, seg, C, skip=(t, k))
    i = m.lists[t][k]
    ys, xs, inside = m.tile_pixels(t)
    lost = np.zeros(C + 1)
    np.add.at(lost, seg[ys[inside], xs[inside]] + 1, lift_model.tile_weights(m, t)[k][inside])
    np.testing.assert_allclose(full.table[i] - less.table[i], lost, rtol=0, atol=1e-13)
    for j in m.lists[t][:k]:
        assert np.array_equal(full.table[j], less.table[j])
    assert any(not np.array_equal(full.table[j], less.table[j]) for j in m.lists[t][k + 1:])


def test_finalize_rule():
    t = np.array([[0, 0, 0], [5, 5, 1], [1, 7, 7], [3, 0, 0], [0, 0, 2 ** 40]], np.uint64)
    labels, share = lift_model.finalize(t, 0.0)
    assert labels.tolist() == [-1, -1, 0, -1, 1]        # an empty row: bin 0; ties: the lowest bin, -1 among them
    assert share.tolist() == [0.0, 5 / 11, 7 / 15, 1.0, 1.0]
    assert lift_model.finalize(t, 3 / lift_model.ONE)[0].tolist() == [-1, -1, 0, -1, 1]
    assert lift_model.finalize(t, 12 / lift_model.ONE)[0].tolist() == [-1, -1, 0, -1, 1]
    assert lift_model.finalize(t, 15.5 / lift_model.ONE)[0].tolist() == [-1, -1, -1, -1, 1]
    assert lift_model.threshold(1e-3) == 1049 and lift_model.threshold(0.0) == 0 and lift_model.threshold(1.0) == lift_model.ONE
