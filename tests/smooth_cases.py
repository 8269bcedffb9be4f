"""Constructed votes for gsx_smooth_labels, which takes only geometry: clump scenes (tests/test_smooth_cases_model.py holds
them to the models on the CPU, tests/test_smooth_table_gpu.py runs them).

A scene is G clumps of exactly k points.  Clump g is centred at (4 (g % 8), 4 ((g // 8) % 8), 4 (g // 64)) and its points sit
at x + j 2^-10, j = 0 .. k-1: exact in fp32, and for k <= 1024 a clump is shorter than 1 while clumps are 4 apart, so N(i) is
exactly i's own clump (the model test confirms it with region_growing_model.knn).  Every point of a clump then sees the same
multiset of votes - the clump's own labels - and a case is a list of histograms {label: count}, one per clump; the own labels
that occur in a clump are the keys of its histogram.  The points are shuffled by a seeded permutation.

The expected result is closed form from the contract (include/gsx.h, tests/smooth_model.py): expected() below.

The search form ranks the distinct labels of the call into class ids, so a case that wants its labels at chosen class ids
needs a label set of chosen size C: filler clumps hold one point of every label no other clump uses (the last one is padded
with copies of its first label).  Filler clumps are checked like any other.  Where a class id sits in the count table -
(dword, half, lane of the winner scan, trip of that lane) - is geometry(), computed from gsx_debug_smooth_constants; the
tables below STATE where the ids of a case are meant to sit, and the model test holds the statement to geometry()."""
import numpy as np

from conftest import load_pkg

I32_MIN, I32_MAX = int(np.iinfo(np.int32).min), int(np.iinfo(np.int32).max)
_K = {}


def constants():
    """gsx_debug_smooth_constants (host only; the library must be built)"""
    if not _K:
        _K.update(load_pkg().smooth_constants())
    return _K


def geometry(c):
    """class id -> (dword of the count table, half of the dword, lane that scans the dword, trip of that lane)"""
    K = constants()
    per = 32 // K["counter_bits"]
    d = c // per
    return d, c % per, d % K["lanes"], d // K["lanes"]


def words(C):
    """dwords of the count table a call with C classes uses"""
    per = 32 // constants()["counter_bits"]
    return (C + per - 1) // per


class Case:
    """name; k; clumps: [{label: count}], every histogram sums to k; kws: the argument sets the case runs with (rounds is 1);
    claims: what the case says it reaches, checked by the model test"""

    def __init__(self, name, k, clumps, kws=({},), claims=(), filler=0):
        self.name, self.k, self.clumps, self.kws, self.claims, self.filler = name, k, clumps, [dict(kw) for kw in kws], list(claims), filler
        assert all(sum(h.values()) == k and min(h.values()) >= 1 for h in clumps), name
        self.n = k * len(clumps)

    def labels_present(self):
        return sorted(set().union(*self.clumps))

    def rank(self, label):
        return self.labels_present().index(label)


def with_filler(name, k, clumps, universe, kws=({},), claims=()):
    """a Case whose distinct labels are exactly `universe`: filler clumps carry the labels `clumps` leave out"""
    used = set().union(*clumps) if clumps else set()
    assert used <= set(universe), name
    rest = [v for v in universe if v not in used]
    fill = []
    for s in range(0, len(rest), k):
        part = rest[s:s + k]
        h = {v: 1 for v in part}
        h[part[0]] += k - len(part)
        fill.append(h)
    c = Case(name, k, list(clumps) + fill, kws, claims, filler=len(fill))
    assert c.labels_present() == sorted(universe), name
    return c


def positions(k, G):
    """the G * k points in clump order, before the shuffle: float32 (G k, 3)"""
    assert k <= 1024 or G == 1
    g = np.arange(G)
    centre = np.stack([4.0 * (g % 8), 4.0 * ((g // 8) % 8), 4.0 * (g // 64)], axis=1)
    P = np.repeat(centre, k, axis=0)
    P[:, 0] += np.tile(np.arange(k) * 2.0 ** -10, G)
    P32 = P.astype(np.float32)
    assert np.array_equal(P32.astype(np.float64), P)
    return P32


def permutation(k, G):
    """the shuffle of a (k, G) scene: seeded by the shape alone, so that scenes of one shape share their neighbour lists"""
    return np.random.default_rng(1000 * k + G).permutation(k * G)


def scene(case):
    """(pts float32 (n, 3), labels int32 (n,), clump of every point (n,))"""
    G = len(case.clumps)
    L = np.concatenate([np.repeat(np.array(list(h), np.int64), list(h.values())) for h in case.clumps])
    perm = permutation(case.k, G)
    return positions(case.k, G)[perm], L[perm].astype(np.int32), np.repeat(np.arange(G), case.k)[perm]


def clump_rule(hist, own, min_votes=1, ignore_label=None, fill_only=False):
    """the contract for one point with own label `own` whose neighbours carry `hist`: (new label, support)"""
    count = {c: v for c, v in hist.items() if ignore_label is None or c != ignore_label}
    new = own
    if count:
        m = max(count.values())
        W = [c for c, v in count.items() if v == m]
        if m >= min_votes:
            new = own if own in W else min(W)
    if fill_only and own != ignore_label:
        new = own
    return new, count.get(new, 0)


def expected(case, kw):
    """(labels int32 (n,), support int32 (n,), changed [count], rounds done) of one round with the arguments kw"""
    _, L, clump = scene(case)
    new, sup = np.empty(case.n, np.int32), np.empty(case.n, np.int32)
    for g, h in enumerate(case.clumps):
        for own in h:
            sel = (clump == g) & (L == own)
            new[sel], sup[sel] = clump_rule(h, own, **kw)
    return new, sup, [int((new != L).sum())], 1


def spread(total, labels, cap):
    """`total` votes over `labels` in order, at most `cap` each: {label: count}"""
    h = {}
    for v in labels:
        if total == 0:
            break
        h[v] = min(cap, total)
        total -= h[v]
    assert total == 0, "the labels given cannot take the remainder under the cap"
    return h


# ---- ties and near-ties ------------------------------------------------------------------------------------------------------
# (class ids that tie, C, where each id is meant to sit: (dword, half, lane, trip))
TIES = [
    ((0, 1), 5, ((0, 0, 0, 0), (0, 1, 0, 0))),                            # one dword
    ((1, 2), 5, ((0, 1, 0, 0), (1, 0, 1, 0))),                            # hi half against the next dword's lo half
    ((126, 128), 130, ((63, 0, 63, 0), (64, 0, 0, 1))),                   # lane 63, trip 0 against lane 0, trip 1: the larger
    ((127, 128), 130, ((63, 1, 63, 0), (64, 0, 0, 1))),                   # class sits in the LOWER lane
    ((2, 130), 132, ((1, 0, 1, 0), (65, 0, 1, 1))),                       # one lane, two trips
    ((129, 254), 256, ((64, 1, 0, 1), (127, 0, 63, 1))),
    ((129, 130), 131, ((64, 1, 0, 1), (65, 0, 1, 1))),                    # (C-2, C-1), C odd: the last dword's hi half is unused
    ((130, 131), 132, ((65, 0, 1, 1), (65, 1, 1, 1))),                    # (C-2, C-1), C even
    ((0, 4095), 4096, ((0, 0, 0, 0), (2047, 1, 63, 31))),
    ((5, 128, 4095), 4096, ((2, 1, 2, 0), (64, 0, 0, 1), (2047, 1, 63, 31))),
]
TIE_KS = (16, 65)                                                          # every form runs at 16; 65 is the search default


def tie_m(k):
    return 5 if k == 16 else 20


def tie_case(ids, C, places, k):
    """labels are the class ids 0 .. C-1.  Clump 0: the ids tie at m, so it holds points whose own label is each of the tied ids
    (they stay) and points of other labels (they take the smallest id).  Clump 1 + t: id t at m, the others at m - 1."""
    m = tie_m(k)
    others = [v for v in range(C) if v not in ids]
    clumps = []
    for top in [None] + list(range(len(ids))):
        h = {v: (m if top is None or ids[top] == v else m - 1) for v in ids}
        h.update(spread(k - sum(h.values()), others, m - 2))
        clumps.append(h)
    claims = [("C", C), ("tie", 0, ids, m)] + [("near", 1 + t, ids[t], m, [v for v in ids if v != ids[t]]) for t in range(len(ids))]
    claims += [("place", v, p) for v, p in zip(ids, places)]
    return with_filler(f"tie-{'-'.join(map(str, ids))}-C{C}-k{k}", k, clumps, range(C), claims=claims)


# ---- the number of classes -----------------------------------------------------------------------------------------------------
C_SIZES = (1, 2, 3, 127, 128, 129, 130, 4095, 4096)                        # words goes from 64 to 65 between 128 and 129


def size_case(C, k):
    """class C-1 wins its clump with a majority; every other own label of the clump changes to it"""
    if C == 1:
        return with_filler(f"classes-1-k{k}", k, [{0: k}, {0: k}], range(1), claims=[("C", 1), ("top", 0, 0, k)])
    m = k // 2 + 1
    others = [v for v in (C - 2, 0, 1, C - 3) if 0 <= v < C - 1]
    h = {C - 1: m}
    h.update(spread(k - m, list(dict.fromkeys(others)), -(-(k - m) // len(set(others)))))
    return with_filler(f"classes-{C}-k{k}", k, [h], range(C), claims=[("C", C), ("top", 0, C - 1, m), ("words", C)])


# ---- counts around 8 bits (search form only) -----------------------------------------------------------------------------------
COUNT_K = 600
COUNT_MS = (255, 256, 257)
# (winner, the other half of its dword, where the winner is meant to sit)
COUNT_PAIRS = [(128, 129, (64, 0, 0, 1)), (131, 130, (65, 1, 1, 1))]


def count_case(m):
    """C = 140.  Per pair two clumps: the winner at m with its dword's other half at m - 1, and with that half at 0.  Run once
    as it is, once with min_votes = m (the same result) and once with min_votes = m + 1, where every point of these clumps keeps
    its label and so reports its own label's count."""
    C, k = 140, COUNT_K
    clumps, claims = [], [("C", C)]
    for w, nb, place in COUNT_PAIRS:
        others = [v for v in (0, 1, 127, 132, 133, 139) if v not in (w, nb)]
        for nb_count in (m - 1, 0):
            h = {w: m}
            if nb_count:
                h[nb] = nb_count
            h.update(spread(k - sum(h.values()), others, 100))
            claims += [("top", len(clumps), w, m), ("count", len(clumps), nb, nb_count)]
            clumps.append(h)
        claims.append(("place", w, place))
        claims.append(("same-dword", w, nb))
    kws = ({}, {"min_votes": m}, {"min_votes": m + 1})
    return with_filler(f"count-{m}", k, clumps, range(C), kws=kws, claims=claims)


# ---- the top bit of a hi half: one clump, k = n (closed form only: round_rows is quadratic in k) ------------------------------------
TOP_N = 33000                                                              # 32769 + two more classes fit; "about 33 000"
TOP_COUNTS = (32767, 32768, 32769)


def top_bit_case(h):
    """classes 0 (lo), 1 (hi half of dword 0) and 2 (lo half of dword 1); class 1 gets h votes, the rest is split over 0 and 2"""
    rest = TOP_N - h
    return Case(f"top-bit-{h}", TOP_N, [{0: rest // 2, 1: h, 2: rest - rest // 2}], kws=({}, {"min_votes": h + 1}),
                claims=[("C", 3), ("top", 0, 1, h), ("place", 1, (0, 1, 0, 0)), ("place", 2, (1, 0, 1, 0))])


# ---- the ignored label ---------------------------------------------------------------------------------------------------------
def ignore_case(name, k, universe, ign, w, x, present, claims=()):
    """m = 4.  Clump 0: the ignored label holds most of the clump, w wins with m over x with m - 1.  Clump 1: w and x tie at m
    (w < x), some points are ignored.  Clump 2 (only when the label is in the data): every vote is ignored.
    Arguments: ignore; ignore + min_votes = m + 1 (nothing changes; a point that keeps an ignored own label reports support 0);
    ignore + fill_only (an ignored own label is filled, x stays although it loses)."""
    m = 4
    assert w < x
    big = ign if present else [v for v in universe if v not in (w, x)][0]
    others = [v for v in universe if v not in (w, x, big)]
    c0 = {big: k - (2 * m - 1) - 2, w: m, x: m - 1}
    c0.update(spread(2, others, 1))
    c1 = {w: m, x: m, big: 3}
    c1.update(spread(k - 2 * m - 3, others, 2))
    clumps = [c0, c1] + ([{ign: k}] if present else [])
    kws = [{"ignore_label": ign}, {"ignore_label": ign, "min_votes": m + 1}, {"ignore_label": ign, "fill_only": True}]
    cl = [("C", len(universe)), ("ignore", ign, present)] + list(claims)
    if present:
        cl += [("top", 0, ign, c0[ign]), ("count", 0, w, m), ("count", 0, x, m - 1), ("tie-ignoring", 1, (w, x), m, ign)]
    return with_filler(f"ignore-{name}-k{k}", k, clumps, universe, kws=kws, claims=cl)


def ignore_cases(k):
    C = 2 * k                                                             # enough labels to fill the remainders
    odd = list(range(C + 1))
    gaps = [10 * (v + 1) for v in range(C)]
    return [
        ignore_case("rank0", k, list(range(C)), 0, 1, 2, True, [("place", 0, (0, 0, 0, 0)), ("same-dword", 0, 1)]),
        ignore_case("last-odd", k, odd, C, 2, 3, True, [("last-lo", C)]),
        ignore_case("hi-beside-winner", k, list(range(C)), 7, 6, 9, True, [("place", 7, (3, 1, 3, 0)), ("same-dword", 6, 7)]),
        ignore_case("absent-below", k, gaps, -7, 10, 20, False),
        ignore_case("absent-above", k, gaps, 10 * C + 5, 10, 20, False),
        ignore_case("absent-between", k, gaps, 15, 10, 20, False),
    ]


# ---- min_votes ----------------------------------------------------------------------------------------------------------------
def min_votes_case(k):
    """m = 2 over singles: changes at min_votes 2, nothing at 3, 65536 and 2^31 - 1"""
    C = k + 6
    h = {3: 2}
    h.update(spread(k - 2, [v for v in range(C) if v != 3], 1))
    kws = [{"min_votes": v} for v in (2, 3, 65536, 2 ** 31 - 1)]
    return with_filler(f"min-votes-2-k{k}", k, [h], range(C), kws=kws, claims=[("C", C), ("top", 0, 3, 2)])


# ---- label values as ranks -----------------------------------------------------------------------------------------------------
def value_case(k):
    m = tie_m(k)
    U = [I32_MIN, -1, 0, 7, 100, I32_MAX] + list(range(1000, 1000 + k))
    rest = U[6:]
    c0 = {I32_MIN: m, 7: m}
    c0.update(spread(k - 2 * m, rest, m - 2))
    c1 = {-1: m, 0: m}
    c1.update(spread(k - 2 * m, rest, m - 2))
    c2 = {I32_MAX: m, 100: m - 1}
    c2.update(spread(k - 2 * m + 1, rest, m - 2))
    claims = [("C", len(U)), ("tie", 0, (I32_MIN, 7), m), ("tie", 1, (-1, 0), m), ("near", 2, I32_MAX, m, [100])]
    return with_filler(f"values-k{k}", k, [c0, c1, c2], U, claims=claims)


# ---- n = 1 modulo the queries of a workgroup -----------------------------------------------------------------------------------
def odd_size_case():
    k, waves = 65, constants()["waves"]
    G = next(G for G in range(3, 3 + 2 * waves) if (G * k) % waves == 1)
    clumps = [{g: 33, g + 1: 32} for g in range(G)]
    return Case(f"size-{G * k}", k, clumps, claims=[("C", G + 1), ("n-mod-waves", 1)])


def reuse_cases():
    """a 4096-class call and a 3-class call for one context: the second must not see the first one's table"""
    return tie_case(*TIES[8], 65), size_case(3, 65)


def all_cases():
    """every clump case but the k = n ones (top_bit_case), in a fixed order"""
    out = [tie_case(ids, C, places, k) for k in TIE_KS for ids, C, places in TIES]
    out += [size_case(C, k) for k in TIE_KS for C in C_SIZES]
    out += [count_case(m) for m in COUNT_MS]
    for k in TIE_KS:
        out += ignore_cases(k) + [min_votes_case(k), value_case(k)]
    out.append(odd_size_case())
    return out


# ---- rounds at high class ids ----------------------------------------------------------------------------------------------------
ROUND_KWS = (dict(), dict(ignore_label=-1, min_votes=2), dict(ignore_label=-1, fill_only=True))
ROUND_RANKS = {10: 127, 20: 128, 30: 129, 40: 139}                         # C = 140: 40 is class C - 1


def high_id_blobs(pts, L):
    """the blobs() scene of test_smooth_search_gpu.py plus a detached group, one point per filler label, so that the four live
    labels 10, 20, 30, 40 rank 127, 128, 129 and C - 1: 127 labels below 10 (-127 .. -1) and 31 .. 39 between 30 and 40"""
    fill = np.array(list(range(-127, 0)) + list(range(31, 40)), np.int32)
    P = np.zeros((len(fill), 3), np.float32)
    P[:, 0] = 100.0 + np.arange(len(fill)) * 2.0 ** -10
    P[:, 1] = 100.0
    return np.concatenate([pts, P]), np.concatenate([L, fill])
