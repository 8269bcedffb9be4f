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
its weights; the best cell lies at least 223 x its GPU tolerance away (lengths; needles 336 x, edges 522 .. 2277 x).

The constructed maps of tests/lift_cases.py (test_lift_edges_gpu.py holds lift_kernel's reduction paths and round lengths to
them bit for bit): D, the classes per wave and the round length of every pattern are computed from the pattern alone and are
what the kernel's constants say; and with q = rint(w * 2^20) of the model, every edge is reached by at least 10 records with
q > 0 - the loop path at loop_max classes and the per-lane path one above (1150 .. 2866 records on `lengths`), remainder rounds
in the first and second chunk (d_9: 827 and 222, d_100: 196 and 29), waves the frame cuts with two or more classes inside
(23 .. 54 on the edge frames, 365 .. 396 on walls_65x53), tiles with a wave wholly outside the frame (32 .. 84)."""
import numpy as np
import pytest

import blend_cases
import lift_cases
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


# ---- the constructed maps of lift_cases.py: the cases are what they claim, and every edge carries weight -------------------
def test_patterns_are_what_they_claim(gsx):
    K = gsx.lift_constants()
    R, Lm = lift_cases.units(K)
    chunk, cells = K["chunk"], K["cells"]
    P = lift_cases.patterns(K)
    for name, p in P.items():
        D, waves, sub = lift_cases.structure(p.bins, K)
        print(f"{name}: D {D}, classes per wave {waves} ({', '.join(lift_cases.path_of(K, c) for c in waves)}), sub {sub}, n_classes {p.n_classes}")
        assert (D, waves, sub) == p.want and sub == min(chunk, cells // D) and sub * D <= cells, name
        assert p.n_classes == (255 if name.endswith("_c255") else p.bins.max()), name        # the smallest that fits
        assert np.array_equal(p.f[P["pos256"].bins], p.bins) and np.array_equal(P["pos256"].bins.reshape(-1), np.arange(256))
    assert P["pos256"].want == (256, (64,) * 4, cells // 256) and P["pos256"].bins.min() == 0
    for j in (1, 2, Lm - 1, Lm, Lm + 1):
        assert P[f"wave_{j}"].want == (j, (j,) * 4, chunk)
    path = lambda name: [lift_cases.path_of(K, c) for c in P[name].want[1]]
    assert path("wave_1") == ["uniform"] * 4 and path(f"wave_{Lm}") == ["loop"] * 4 and path(f"wave_{Lm + 1}") == ["lanes"] * 4
    assert path("mixed_waves") == ["uniform", "loop", "loop", "lanes"] and P["mixed_waves"].want[1] == (1, 2, Lm, Lm + 1)
    rows = [set(P["mixed_waves"].bins[4 * w:4 * w + 4].reshape(-1)) for w in range(4)]
    assert sum(len(s) for s in rows) == len(set.union(*rows)) == P["mixed_waves"].want[0]      # disjoint between the waves
    assert P[f"d_{R}"].want[2] == chunk and R * chunk == cells                                 # the last whole-chunk round
    sub = P[f"d_{R + 1}"].want[2]
    assert sub == cells // (R + 1) < chunk and 0 < chunk - sub < sub                           # one full round, one remainder round
    assert path(f"d_{R}") == ["lanes"] * 4 and path(f"d_{R + 1}") == ["lanes"] * 4
    loop = P[f"d{R + 1}_loop"]
    assert loop.want[0] == R + 1 and loop.want[2] == sub and path(loop.name) == ["loop"] * 4
    rows = [set(loop.bins[4 * w:4 * w + 4].reshape(-1)) for w in range(4)]
    assert sum(len(s) for s in rows) == R + 1 == len(set.union(*rows))
    assert P["d_16"].want == (16, (16,) * 4, cells // 16)
    assert P["d_100"].want[2] == cells // 100 and chunk % (cells // 100) != 0                  # a sub that does not divide the chunk
    assert P["d_255"].want == (255, (64,) * 4, cells // 255) and P["d_255"].n_classes == 254
    we = P["word_edges"]
    assert sorted(set(we.bins.reshape(-1))) == sorted(lift_cases.WORD_EDGES) and we.want[0] == 16 and (we.bins == we.bins[0]).all()
    assert {b // 32 for b in lift_cases.WORD_EDGES} == set(range(8)) and {0, 31, 255} <= set(lift_cases.WORD_EDGES)
    assert all({32 * j - 1, 32 * j} <= set(lift_cases.WORD_EDGES) for j in range(1, 7))       # both sides of six word boundaries
    for name in (f"wave_{Lm + 1}", "d_100"):
        assert np.array_equal(P[name + "_c255"].bins, P[name].bins) and P[name].n_classes < 255
    # the map: the pattern repeated, cut at the border, minus 1 - and a function of the fine map pixel by pixel
    fine = P["pos256"].map(33, 45)
    for p in P.values():
        seg = p.map(33, 45)
        assert seg.shape == (45, 33) and seg.dtype == np.int32 and seg.min() >= -1 and seg.max() < p.n_classes
        assert np.array_equal(seg[16:32, 16:32] + 1, p.bins) and np.array_equal(seg[32:45, 32:33] + 1, p.bins[:13, :1])
        assert np.array_equal(p.f[fine + 1] - 1, seg)


def test_the_pair_that_is_not_periodic(gsx):
    K = gsx.lift_constants()
    R, _ = lift_cases.units(K)
    for W, H in ((96, 48), (65, 53), (47, 47)):
        (fine, C), (coarse, n), f = lift_cases.halves_pair(W, H)
        assert C == 255 and n == lift_cases.HALVES_N == f.max() and np.array_equal(f[fine + 1] - 1, coarse) and coarse.min() == -1
        assert np.array_equal(fine, lift_model.maps(W, H)["c255"][0])
        Ds = np.array([s[0] for s in lift_cases.tile_structures(coarse, K)]).reshape((H + 15) // 16, (W + 15) // 16)
        print(f"{W}x{H}: classes per tile\n{Ds}")
        assert (Ds[:, 1:] != Ds[:, :-1]).any() and (Ds[1:] != Ds[:-1]).any() and len(np.unique(Ds)) >= 4
        assert (Ds <= R).any() and (Ds > R).any()                         # whole-chunk rounds and shorter ones in one frame
    whole = np.array([s[0] for s in lift_cases.tile_structures(lift_model.maps(96, 48)["c255"][0], K)])
    assert (whole == 121).all()                                          # 121 consecutive bins in every whole tile of the fine map


def staged_q(m, t, K):
    """q = rint(w * ONE) of tile t's records on its pixels, (L,16,16) ints - of the records the kernel stages: the list up to the
    chunk after which every pixel inside is opaque"""
    L = m.consumed(t, K["chunk"])[0]
    return np.rint(lift_model.tile_weights(m, t)[:L] * lift_model.ONE).astype(np.int64)


def loaded(m, seg, K, pick, positions=None):
    """how many records (tile, list position) put q > 0 on a pixel of pick(D, waves, inside) -> 16x16 mask or None; positions:
    (list length) -> the list positions that count"""
    count = 0
    for t, (D, waves, sub, inside, _) in enumerate(lift_cases.tile_structures(seg, K)):
        if len(m.lists[t]) == 0:
            continue
        mask = pick(D, waves, inside)
        if mask is None:
            continue
        q = staged_q(m, t, K)
        hit = (q * (mask & inside)[None] > 0).any((1, 2))
        if positions is not None:
            keep = np.zeros(len(hit), bool)
            keep[[k for k in positions(len(m.lists[t]), sub) if k < len(hit)]] = True
            hit &= keep
        count += int(hit.sum())
    return count


def waves_with(cond):
    """pick: the pixel rows of the waves for which cond(class count, pixels inside) holds"""
    def pick(D, waves, inside):
        rows = [w for w in range(4) if cond(waves[w], int(inside[4 * w:4 * w + 4].sum()))]
        if not rows:
            return None
        mask = np.zeros((16, 16), bool)
        for w in rows:
            mask[4 * w:4 * w + 4] = True
        return mask
    return pick


def remainder_positions(chunk, which):
    """list positions of chunk `which` that fall into its remainder round: position within the chunk >= sub * (cnt // sub)"""
    def positions(L, sub):
        cnt = min(chunk, L - which * chunk)
        return [] if cnt <= 0 else [which * chunk + k for k in range(sub * (cnt // sub), cnt)]
    return positions


def test_every_edge_carries_weight(gsx):
    """conditions, not measurements: each structural edge is reached by at least 10 records with q > 0"""
    K = gsx.lift_constants()
    R, Lm = lift_cases.units(K)
    P = lift_cases.patterns(K)
    m = blend_cases.prepared("lengths").model
    seen = {}
    for name in (f"wave_{Lm}", "mixed_waves"):
        seen[f"loop path at {Lm} classes, {name}, lengths"] = loaded(m, P[name].map(m.W, m.H), K, waves_with(lambda c, n: c == Lm))
    for name in (f"wave_{Lm + 1}", "mixed_waves"):
        seen[f"per-lane path at {Lm + 1} classes, {name}, lengths"] = loaded(m, P[name].map(m.W, m.H), K, waves_with(lambda c, n: c == Lm + 1))
    assert max(blend_cases.LENGTHS) > 2 * K["chunk"] and sorted(blend_cases.LENGTHS)[-4] > K["chunk"]
    for name in (f"d_{R + 1}", f"d{R + 1}_loop", "d_100"):
        for which in (0, 1):
            seen[f"remainder round of chunk {which}, {name}, lengths"] = loaded(m, P[name].map(m.W, m.H), K, lambda D, w, i: i,
                                                                             remainder_positions(K["chunk"], which))
    for scene in ("edges_33x33", "edges_17x17", "walls_65x53"):
        m = blend_cases.prepared(scene).model
        assert m.W % 16 and m.H % 16
        for name in ("pos256", "wave_2", f"wave_{Lm + 1}", "mixed_waves"):
            seen[f"wave cut by the frame with >= 2 classes inside, {name}, {scene}"] = loaded(
                m, P[name].map(m.W, m.H), K, waves_with(lambda c, n: c >= 2 and 0 < n < 64))
        seen[f"tile with a wave wholly outside the frame, pos256, {scene}"] = loaded(
            m, P["pos256"].map(m.W, m.H), K, lambda D, w, i: i if any(not i[4 * k:4 * k + 4].any() for k in range(4)) else None)
    for what, count in seen.items():
        print(f"{count:6d} records with q > 0: {what}")
    assert all(count >= 10 for count in seen.values()), {k: v for k, v in seen.items() if v < 10}
