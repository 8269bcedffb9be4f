"""CPU: the clump scenes of tests/smooth_cases.py against the models, so that tests/test_smooth_table_gpu.py can trust them.
For every case of at most 5000 points: region_growing_model.knn confirms that N(i) is i's clump; the closed form
(smooth_cases.expected) equals smooth_model.round_rows over those lists; and the case reaches the edge it names - its
classes rank where stated and sit on the stated dword, half, lane and trip of the search form's count table
(gsx_debug_smooth_constants), the claimed counts are in the data, and C is what the name says."""
import numpy as np
import pytest

import region_growing_model as model
import smooth_cases as sc
import smooth_model as sm

CASES = sc.all_cases()
_LISTS = {}


def lists(case):
    """the model's neighbour lists of a scene; scenes of one shape share positions and shuffle, and so their lists"""
    key = (case.k, len(case.clumps))
    if key not in _LISTS:
        _LISTS[key] = model.knn(sc.scene(case)[0], case.k)[0]
    return _LISTS[key]


def test_constants():
    K = sc.constants()
    assert K == {"list_max_k": 64, "max_classes": 4096, "counter_bits": 16, "lanes": 64, "waves": 4}
    assert sc.words(128) == K["lanes"] and sc.words(129) == K["lanes"] + 1     # the scan's second trip starts at C = 129
    assert sc.words(K["max_classes"]) * 4 * K["waves"] <= 64 * 1024 - 4 * K["waves"] * 256   # the tables and the search's histograms fit in LDS
    assert sc.geometry(0) == (0, 0, 0, 0) and sc.geometry(K["max_classes"] - 1) == (2047, 1, 63, 31)
    assert max(c.k for c in CASES if c.name.endswith("k16")) <= K["list_max_k"] < 65


def test_names_are_unique_and_sizes_small():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    assert max(c.n for c in CASES) <= 5000


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_neighbours_are_the_clump(case):
    _, _, clump = sc.scene(case)
    nbr = lists(case)
    assert (clump[nbr] == clump[:, None]).all()
    assert (np.sort(nbr, axis=1)[:, 1:] != np.sort(nbr, axis=1)[:, :-1]).all()   # k distinct members of a clump of k: all of it


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_closed_form_is_the_model(case):
    _, L, clump = sc.scene(case)
    nbr = lists(case)
    for kw in case.kws:
        new, sup, changed, done = sc.expected(case, kw)
        if case.k > 65:
            # round_rows is quadratic in k: one point of every (clump, own label) - the closed form gives all points of such a
            # group one answer, and their lists are the same set (test_neighbours_are_the_clump) - and the first 64 points
            _, rep = np.unique(clump.astype(np.int64) * 2 ** 32 + (L.astype(np.int64) - sc.I32_MIN), return_index=True)
            rows = np.union1d(rep, np.arange(64))
            want, w_sup = sm.round_rows(nbr[rows], L, rows, **kw)
            assert np.array_equal(new[rows], want) and np.array_equal(sup[rows], w_sup), (case.name, kw)
            same = np.unique(np.stack([clump, L, new, sup], axis=1), axis=0)
            assert len(same) == len(rep) and done == 1                    # one answer per group
            continue
        want, w_sup = sm.round_rows(nbr, L, **kw)
        assert np.array_equal(new, want) and np.array_equal(sup, w_sup), (case.name, kw)
        assert changed == [int((want != L).sum())] and done == 1
        w_run = sm.run(nbr, L, rounds=1, **kw)
        assert np.array_equal(w_run[0], new) and w_run[1] == changed and w_run[2] == done and np.array_equal(w_run[3], sup)


def check_claims(case):
    """every claim of a case against its data; returns the kinds of claim seen"""
    _, L, clump = sc.scene(case)
    hist = [dict(zip(*(a.tolist() for a in np.unique(L[clump == g], return_counts=True)))) for g in range(len(case.clumps))]
    assert hist == [dict(sorted(h.items())) for h in case.clumps]
    uniq = np.unique(L).tolist()
    rank = uniq.index
    new, sup, changed, _ = sc.expected(case, case.kws[0])
    seen = set()
    for claim in case.claims:
        kind, a = claim[0], claim[1:]
        seen.add(kind)
        if kind == "C":
            assert len(uniq) == a[0]
        elif kind == "tie":
            g, ids, m = a
            h = hist[g]
            assert all(h[v] == m for v in ids) and max(h.values()) == m and sorted(v for v in h if h[v] == m) == sorted(ids)
            neither = (clump == g) & ~np.isin(L, ids)
            assert neither.any() and (new[neither] == min(ids)).all() and (sup[neither] == m).all()
            for v in ids:                                                 # a tied own label stays, the larger ones included
                own = (clump == g) & (L == v)
                assert own.sum() == m and (new[own] == v).all() and (sup[own] == m).all()
        elif kind == "near":
            g, top, m, losers = a
            h = hist[g]
            assert h[top] == m and all(h[v] == m - 1 for v in losers) and sorted(h.values())[-1 - len(losers)] == m - 1
            assert sorted(h.values())[-2 - len(losers)] < m - 1 if len(h) > 1 + len(losers) else True
            assert (new[clump == g] == top).all() and (sup[clump == g] == m).all()
        elif kind == "top":
            g, v, m = a
            assert hist[g][v] == m and sorted(hist[g].values())[-2:] != [m, m]
        elif kind == "count":
            g, v, m = a
            assert hist[g].get(v, 0) == m
        elif kind == "place":
            assert sc.geometry(rank(a[0])) == tuple(a[1]), (a, sc.geometry(rank(a[0])))
        elif kind == "same-dword":
            p, q = sc.geometry(rank(a[0])), sc.geometry(rank(a[1]))
            assert p[0] == q[0] and p[1] != q[1]
        elif kind == "words":
            assert sc.words(len(uniq)) == (a[0] + 1) // 2 and rank(a[0] - 1) == a[0] - 1
        elif kind == "ignore":
            assert (a[0] in uniq) == a[1] and all(kw["ignore_label"] == a[0] for kw in case.kws)
        elif kind == "tie-ignoring":
            g, (w, x), m, ign = a
            h = {v: c for v, c in hist[g].items() if v != ign}
            assert h[w] == m and h[x] == m and sorted(h.values())[-3] < m and hist[g][ign] >= 1
        elif kind == "last-lo":
            assert rank(a[0]) == len(uniq) - 1 and len(uniq) % 2 == 1 and sc.geometry(rank(a[0]))[1] == 0
        elif kind == "n-mod-waves":
            assert case.n % sc.constants()["waves"] == a[0]
        else:
            raise AssertionError(f"unknown claim {claim}")
    return seen


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_reaches_its_edge(case):
    assert case.claims
    check_claims(case)


def test_tie_table_is_the_issue_list():
    """the pairs, both k, the class counts, and what the places say: the larger class in the lower lane, one lane on two trips"""
    assert [t[0] for t in sc.TIES] == [(0, 1), (1, 2), (126, 128), (127, 128), (2, 130), (129, 254), (129, 130), (130, 131), (0, 4095),
                                       (5, 128, 4095)]
    assert sc.TIE_KS == (16, 65) and sc.C_SIZES == (1, 2, 3, 127, 128, 129, 130, 4095, 4096)
    for ids, C, places in sc.TIES:
        assert [sc.geometry(v) for v in ids] == [tuple(p) for p in places] and max(ids) < C
    for i in (2, 3):
        (_, _, (a, b)) = sc.TIES[i]
        assert a[2] == 63 and a[3] == 0 and b[2] == 0 and b[3] == 1        # the smaller class in the higher lane
    (_, _, (a, b)) = sc.TIES[4]
    assert a[2] == b[2] and a[3] != b[3]
    assert sc.TIES[6][1] % 2 == 1 and sc.TIES[7][1] % 2 == 0 and all(t[0][-2:] == (t[1] - 2, t[1] - 1) for t in sc.TIES[6:8])


def test_ignore_cases_cover_their_list():
    for k in sc.TIE_KS:
        cases = {c.name: c for c in sc.ignore_cases(k)}
        _, L, clump = sc.scene(cases[f"ignore-rank0-k{k}"])
        new, sup, changed, _ = sc.expected(cases[f"ignore-rank0-k{k}"], {"ignore_label": 0})
        assert (new[clump == 2] == 0).all() and (sup[clump == 2] == 0).all()          # every vote ignored: own stays, support 0
        assert ((L == 0) & (clump == 0)).any() and (new[clump == 0] == 1).all()       # the ignored majority does not win
        keep = sc.expected(cases[f"ignore-rank0-k{k}"], {"ignore_label": 0, "min_votes": 5})
        mine = clump <= 2                                                 # a filler clump's padding may still reach 5 votes
        assert np.array_equal(keep[0][mine], L[mine]) and (keep[1][mine & (L == 0)] == 0).all()   # a kept ignored label: support 0
        fill = sc.expected(cases[f"ignore-rank0-k{k}"], {"ignore_label": 0, "fill_only": True})[0]
        assert (fill[(clump == 0) & (L == 0)] == 1).all() and (fill[(clump == 0) & (L == 2)] == 2).all()   # filled; loses and stays
        for name in ("absent-below", "absent-above", "absent-between"):
            c = cases[f"ignore-{name}-k{k}"]
            ign, labels = c.kws[0]["ignore_label"], c.labels_present()
            assert ign not in labels
            assert {"absent-below": ign < labels[0], "absent-above": ign > labels[-1], "absent-between": labels[0] < ign < labels[1]}[name]


def test_count_and_min_votes_cases():
    for m in sc.COUNT_MS:
        c = sc.count_case(m)
        assert c.k == sc.COUNT_K > sc.constants()["list_max_k"] and c.kws == [{}, {"min_votes": m}, {"min_votes": m + 1}]
        _, L, clump = sc.scene(c)
        mine = clump < len(c.clumps) - c.filler                           # the filler clump's padding reaches more than m + 1
        kept = sc.expected(c, c.kws[2])
        assert np.array_equal(kept[0][mine], L[mine]) and {m, m - 1} <= set(kept[1][mine].tolist())
        at_m = sc.expected(c, c.kws[1])
        assert all(np.array_equal(a, b) for a, b in zip(at_m[:2], sc.expected(c, {}))) and at_m[2][0] > 0
    for k in sc.TIE_KS:
        c = sc.min_votes_case(k)
        assert [kw["min_votes"] for kw in c.kws] == [2, 3, 65536, 2 ** 31 - 1]
        ch = [sc.expected(c, kw)[2] for kw in c.kws]
        assert ch[0][0] >= k - 2 and ch[3] == [0] and ch[2] == [0]
        _, L, clump = sc.scene(c)
        assert np.array_equal(sc.expected(c, c.kws[1])[0][clump == 0], L[clump == 0])


def test_top_bit_cases_closed_form_on_a_small_twin():
    """the k = n cases are too large for round_rows; the same histogram shape scaled down runs through it"""
    for h in sc.TOP_COUNTS:
        c = sc.top_bit_case(h)
        assert c.n == c.k == sc.TOP_N and sum(c.clumps[0].values()) == c.n and c.clumps[0][1] == h and len(c.clumps) == 1
        assert sc.geometry(c.rank(1))[:2] == (0, 1) and h < 2 ** sc.constants()["counter_bits"]
        new, sup, changed, done = sc.expected(c, {})
        assert (new == 1).all() and (sup == h).all() and changed == [c.n - h]
        new, sup, changed, done = sc.expected(c, c.kws[1])
        _, L, _ = sc.scene(c)
        assert np.array_equal(new, L) and changed == [0] and sorted(set(sup.tolist())) == sorted(set(c.clumps[0].values()))
    twin = sc.Case("twin", 40, [{0: 3, 1: 33, 2: 4}])
    nbr = model.knn(sc.scene(twin)[0], 40)[0]
    for kw in ({}, {"min_votes": 34}):
        want, w_sup = sm.round_rows(nbr, sc.scene(twin)[1], **kw)
        new, sup, _, _ = sc.expected(twin, kw)
        assert np.array_equal(new, want) and np.array_equal(sup, w_sup)


def test_high_id_blobs_rank_as_stated():
    from test_smooth_search_gpu import blobs
    pts, L = sc.high_id_blobs(*blobs())
    uniq = np.unique(L).tolist()
    assert len(pts) == len(L) == 3000 + 136 and len(uniq) == 140
    assert {v: uniq.index(v) for v in sc.ROUND_RANKS} == sc.ROUND_RANKS and sc.ROUND_RANKS[40] == len(uniq) - 1
    assert [sc.geometry(r)[2:] for r in (127, 128)] == [(63, 0), (0, 1)]
