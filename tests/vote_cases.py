"""Constructed votes for the majority-vote kernels (csrc/vote.hip): the test authors the vote MATRIX, not the scene.

B[n, V] is an int matrix: B[i, v] = b >= 0 means Gaussian i votes bin b in view v (bin 0 = an unlabelled pixel, bin b = label b - 1),
-1 means it casts no vote there.  vote_model(B, bins) is the labeler on that matrix in plain integer numpy; realise() turns the
matrix into a scene (positions, cameras, maps, image sizes) whose every projection is exact in float32, so that the oracle and the
kernels must read exactly B out of it.  tests/test_vote_model.py proves oracle == model for every case on the CPU;
tests/test_vote_edges_gpu.py then pins the kernels to the model.

No GPU import here, and everything is deterministic (seeded where random).

The scene: Gaussian i sits on pixel (col[i], row[i]) of an unbounded canvas, on the sheet z = +1 ("front", sheet 0) or z = -1
("back", sheet 1); fx = fy = 64, position ((col + phase) / 64, (row + phase) / 64, +-1).  A view is a camera without tilt that sees
the rectangle [c0, c0 + w) x [r0, r0 + h) of ONE sheet (identity rotation for the front, diag(1, 1, -1) for the back), so a Gaussian
abstains exactly where its sheet or its pixel is outside the view: B's -1 entries must be such a pattern, and realise() asserts it.
phase = 0.5 puts every projection on a pixel centre (the fp32 filter certifies it), phase = 0.0 exactly on the pixel's corner (the
filter must hand every wave to the exact divisions).
"""
import numpy as np

F = 64.0          # focal length in pixels: a power of two, so (col + phase) / F and every product with F are exact
PHASES = (0.5, 0.0)
FLIP = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]]
EYE = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
MAX_BATCH = 255   # kMaxBatch of vote.hip


# ---- the model --------------------------------------------------------------------------------------------------------------------
def vote_model(B, bins, total_views=None):
    """-> dict(labels int32 (n,), winner (n,) bin or -1, cnt (bins, n), first (bins, n) view of the first vote or V, fv (bins, n)).
    The winner is the bin of largest count whose first vote is earliest (the reference's dict keeps insertion order and max()
    returns the first maximum); no vote at all -> label -1.  fv = FVMAX - first where voted, 0 elsewhere; FVMAX = 255 for a run
    of <= 255 views, 65535 beyond (the planes the library documents)."""
    B = np.asarray(B)
    n, V = B.shape
    total = V if total_views is None else total_views
    assert B.min(initial=0) >= -1 and B.max(initial=0) < bins
    cnt = np.zeros((bins, n), np.int64)
    first = np.full((bins, n), V, np.int64)
    idx = np.arange(n)
    for v in range(V - 1, -1, -1):
        b = B[:, v]
        m = b >= 0
        cnt[b[m], idx[m]] += 1
        first[b[m], idx[m]] = v
    top = cnt.max(axis=0)
    cand = (cnt == top[None, :]) & (cnt > 0)
    winner = np.where(cand, first, V + 1).argmin(axis=0)
    winner = np.where(top > 0, winner, -1)
    fvmax = 255 if total <= 255 else 65535
    fv = np.where(cnt > 0, fvmax - first, 0)
    labels = np.where(winner >= 0, winner - 1, -1).astype(np.int32)
    return {"labels": labels, "winner": winner, "cnt": cnt, "first": first, "fv": fv, "top": top}


# ---- the realisation ----------------------------------------------------------------------------------------------------------------
def view(sheet, c0, r0, w, h, map_shape=None, img_size=None):
    """A view of the rectangle [c0, c0 + w) x [r0, r0 + h) of a sheet.  map_shape (h, w) and img_size (w, h) default to the frame:
    another map size runs the scale of dls.py:281-282, an image size smaller than the frame its clamp (:285)."""
    return {"sheet": sheet, "c0": int(c0), "r0": int(r0), "w": int(w), "h": int(h),
            "map_shape": (int(h), int(w)) if map_shape is None else (int(map_shape[0]), int(map_shape[1])),
            "img_size": (int(w), int(h)) if img_size is None else (int(img_size[0]), int(img_size[1]))}


def map_pixel(vw, x, y):
    """Frame pixel -> map pixel, the reference's arithmetic (dls.py:270-271, :281-286) in the same order, in fp64."""
    mh, mw = vw["map_shape"]
    iw, ih = vw["img_size"]
    xs = np.trunc(x.astype(np.float64) * (float(mw) / float(iw))).astype(np.int64)
    ys = np.trunc(y.astype(np.float64) * (float(mh) / float(ih))).astype(np.int64)
    return np.clip(xs, 0, mw - 1), np.clip(ys, 0, mh - 1)


def visible(cols, rows, sheets, vw):
    return (sheets == vw["sheet"]) & (cols >= vw["c0"]) & (cols < vw["c0"] + vw["w"]) & (rows >= vw["r0"]) & (rows < vw["r0"] + vw["h"])


def mask_votes(want, cols, rows, sheets, views):
    """The votes `want` (n, V) where the view sees the Gaussian, -1 elsewhere."""
    B = np.array(want, dtype=np.int64)
    for v, vw in enumerate(views):
        B[~visible(cols, rows, sheets, vw), v] = -1
    return B


def realise(B, cols, rows, sheets, views, phase, seg_dtype=np.int32):
    """-> positions (n, 3) float32, cams, segs, sizes: a scene in which Gaussian i votes B[i, v] in view v and nothing else."""
    B = np.asarray(B)
    n, V = B.shape
    assert len(views) == V and phase in PHASES
    assert np.abs(cols).max(initial=0) < 1 << 16 and np.abs(rows).max(initial=0) < 1 << 16   # (k + 0.5) / 64 exact in float32
    pos = np.empty((n, 3), np.float32)
    pos[:, 0] = (cols + phase) / F
    pos[:, 1] = (rows + phase) / F
    pos[:, 2] = np.where(sheets == 0, 1.0, -1.0)
    assert np.array_equal(pos[:, 0].astype(np.float64) * F, cols + phase) and np.array_equal(pos[:, 1].astype(np.float64) * F, rows + phase)
    taken = set(zip(cols.tolist(), rows.tolist(), sheets.tolist()))
    assert len(taken) == n, "two Gaussians on one pixel"
    cams, segs, sizes = [], [], []
    for v, vw in enumerate(views):
        vis = visible(cols, rows, sheets, vw)
        assert np.array_equal(vis, B[:, v] >= 0), f"view {v}: the matrix abstains where the scene cannot"
        cams.append({"fx": F, "fy": F, "width": vw["w"], "height": vw["h"], "rotation": EYE if vw["sheet"] == 0 else FLIP,
                     "position": [(vw["c0"] + vw["w"] / 2.0) / F, (vw["r0"] + vw["h"] / 2.0) / F, 0.0]})
        seg = np.full(vw["map_shape"], -1, np.int64)
        owner = np.full(vw["map_shape"], -2, np.int64)
        mx, my = map_pixel(vw, cols[vis] - vw["c0"], rows[vis] - vw["r0"])
        lab = B[vis, v] - 1
        owner[my, mx] = lab
        assert np.array_equal(owner[my, mx], lab), f"view {v}: Gaussians that share a map pixel must share their vote"
        seg[my, mx] = lab
        segs.append(np.ascontiguousarray(seg.astype(seg_dtype)))
        sizes.append(vw["img_size"])
    return pos, cams, segs, sizes


def grid(n, W):
    """Gaussian i on pixel (i % W, i // W) of the front sheet."""
    assert W % 2 == 0
    i = np.arange(n)
    return i % W, i // W, np.zeros(n, np.int64)


def all_of(cols, rows, sheet=0):
    """The view that sees every Gaussian of the sheet (and a margin of empty pixels round them)."""
    return view(sheet, cols.min() - 1, rows.min() - 1, cols.max() - cols.min() + 3, rows.max() - rows.min() + 3)


def nothing():
    return view(0, -40, -40, 2, 3)     # an empty window: no Gaussian ever sits at negative rows


def early_permille(V, E):
    """The value of option early_vote_at that starts the early stage after exactly E of V announced views
    (vote.hip: at = max(1, ceil(V * permille / 1000)))."""
    for p in range(1, 1001):
        if max(1, -(-V * p // 1000)) == E:
            return p
    raise ValueError((V, E))


def balanced_bounds(V):
    S = -(-V // MAX_BATCH)
    return [V * s // S for s in range(S + 1)]


def early_bounds(V):
    """The early cut of more than 255 announced views (vote.hip: early_batch_bounds): balanced batches, then a short tail."""
    tail = min(max(V // 16, 16), 64)
    Sb = -(-(V - tail) // MAX_BATCH)
    return [(V - tail) * s // Sb for s in range(Sb + 1)] + [V]


class Case(dict):
    """name, family, B, bins, n_classes, place (cols, rows, sheets), views, E (split points), options, guard."""

    def scene(self, phase):
        key = ("scene", phase)
        if key not in self:
            self[key] = realise(self["B"], *self["place"], self["views"], phase, self.get("seg_dtype", np.int32))
        return self[key]

    def model(self):
        if "model" not in self:
            self["model"] = vote_model(self["B"], self["bins"])
        return self["model"]

    def check_guard(self):
        g = self.get("guard")
        if g is not None:
            g(self, self.model())

    def __repr__(self):
        return self["name"]


def _case(name, family, B, C, place, views, E=(), guard=None, **extra):
    B = np.ascontiguousarray(B, dtype=np.int64)
    assert B.shape[1] == len(views)
    return Case(name=name, family=family, B=B, n_classes=C, bins=C + 1, place=place, views=views, E=tuple(E), guard=guard, **extra)


# ---- family 1 (and 6): view counts ------------------------------------------------------------------------------------------------
def _tied_votes(rng, nv, bins):
    """nv votes over `bins` bins in random order in which 1, 2 or 3 bins share the largest count."""
    if nv == 0:
        return np.zeros(0, np.int64)
    k = int(rng.choice([1, 2, 3], p=[0.25, 0.45, 0.30]))
    k = min(k, bins, nv)
    while True:
        m_min, m_max = -(-(nv + bins - k) // bins), nv // k
        if m_min <= m_max:
            break
        k -= 1
    m = int(rng.integers(m_min, min(m_max, m_min + 2) + 1))
    order = rng.permutation(bins)
    pool = rng.permutation(np.repeat(order[k:], m - 1))          # every other bin stays below m
    votes = np.concatenate([np.repeat(order[:k], m), pool[:nv - k * m]])
    return rng.permutation(votes.astype(np.int64))


def _tie_guard(case, m):
    """>= 30 % of the Gaussians have two or more bins at the maximum; for >= 5 % the winner is not the lowest tied bin; for
    >= 5 % it is not the bin that reaches the maximum first.  (One view cannot tie; with two, the first voter both wins and reaches
    the maximum first - the shares that arithmetic allows are asked of V < 7.)"""
    B, V, n = case["B"], case["B"].shape[1], case["B"].shape[0]
    tied = ((m["cnt"] == m["top"][None, :]) & (m["cnt"] > 0)).sum(axis=0) >= 2
    lowest = np.where(m["top"] > 0, ((m["cnt"] == m["top"][None, :]) & (m["cnt"] > 0)).argmax(axis=0), -1)
    reach = np.full(n, -1)
    run = np.zeros((case["bins"], n), np.int64)
    idx = np.arange(n)
    for v in range(V):
        b = B[:, v]
        ok = b >= 0
        run[b[ok], idx[ok]] += 1
        hit = ok & (reach < 0)
        hit[ok] &= run[b[ok], idx[ok]] == m["top"][ok]
        reach[hit] = b[hit]
    share = lambda x: float(np.mean(x))
    if V >= 2:
        assert share(tied) >= 0.30, share(tied)
        assert share(m["winner"] != lowest) >= 0.05
    if V >= 7:
        assert share(m["winner"] != reach) >= 0.05, share(m["winner"] != reach)
    if V >= 7:
        assert 0.03 < share(B < 0) < 0.25, share(B < 0)


def _view_count_case(V, n=257, C=5, W=16, E=(), family=1, cull=False, two_sheets=False):
    """two_sheets: every other row of Gaussians lies on the back sheet, every third view looks at it, and view 5 at nothing."""
    rng = np.random.default_rng(1000 * family + V + (7 if cull else 0) + (13 if two_sheets else 0))
    cols, rows, sheets = grid(n, W)
    if two_sheets:
        sheets = rows % 2
    R = int(rows.max()) + 1
    views = []
    for v in range(V):
        if two_sheets and v == 5:
            views.append(nothing())
        elif two_sheets:
            views.append(view(1 if v % 3 == 2 else 0, -1, int(rng.integers(0, 2)), W + 2, R))
        elif cull and v % 2 == 1:
            views.append(view(0, -1, 0, W + 2, 1))                 # alternate views see the first row only: whole waves lie outside
        else:
            r0, r1 = int(rng.integers(0, 3)), R - int(rng.integers(0, 3))   # ~10 % of the pairs lie outside the window of rows
            views.append(view(0, -1, r0, W + 2, r1 - r0))
    vis = np.stack([visible(cols, rows, sheets, vw) for vw in views], axis=1)
    B = np.full((n, V), -1, np.int64)
    for i in range(n):
        B[i, vis[i]] = _tied_votes(rng, int(vis[i].sum()), C + 1)
    name = f"f{family}-V{V}" + ("-cull" if cull else "") + ("-sheets" if two_sheets else "")

    def sheet_guard(case, m):
        assert 0.4 < np.mean(case["B"] < 0) < 0.7 and (case["B"][:, 5] < 0).all()
        assert (((m["cnt"] == m["top"][None]) & (m["cnt"] > 0)).sum(0) >= 2).mean() >= 0.30
    return _case(name, family, B, C, (cols, rows, sheets), views, E=E, guard=sheet_guard if two_sheets else None if cull else _tie_guard, cull=cull)


def family1():
    out = []
    for V in (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 254, 255):
        out.append(_view_count_case(V, E=sorted({V - 1, 64} & set(range(1, V))) if V >= 63 else ()))
    # the other way to abstain: a sheet the view does not look at, and a view that looks at nothing
    out += [_view_count_case(17, two_sheets=True, E=(9,)), _view_count_case(65, two_sheets=True, E=(64,))]
    return out


def family1_cull():
    return [_view_count_case(V, cull=True) for V in (63, 64, 65, 129)]


def family6():
    return [_view_count_case(40, E=(1, 15, 16, 17, 31, 32, 33, 39), family=6)]


# ---- family 2: wave and block raggedness ----------------------------------------------------------------------------------------------
def family2():
    out = []
    V, C = 9, 150
    for n in (1, 63, 64, 65, 255, 256, 257, 1025):
        cols, rows, sheets = grid(n, 16)
        i = np.arange(n)
        own = 1 + (i * 7) % C
        B = np.empty((n, V), np.int64)
        for v in range(V):
            major = ((v + i) % 9) < 5                               # five of the nine views, another five for every Gaussian
            B[:, v] = np.where(major, own, 1 + (own + 11 * v + 3) % C)
        views = [all_of(cols, rows)] * V

        def guard(case, m, own=own, n=n):
            assert np.array_equal(m["labels"], own - 1)
            for w in range(0, n - 63, 64):
                assert len(set(own[w:w + 64].tolist())) == 64     # 64 lanes, 64 answers
        out.append(_case(f"f2-n{n}", 2, B, C, (cols, rows, sheets), views, guard=guard))
    return out


# ---- family 3: workgroup order ------------------------------------------------------------------------------------------------------
def family3():
    out = []
    C = 254
    for g in (6, 7, 8, 14, 15, 16, 17, 32):          # grids of g + 1 workgroups
        n = 256 * g + 1
        cols, rows, sheets = grid(n, 64)
        i = np.arange(n)
        ans = (i * 37) % C
        B = np.stack([np.where(i % 3 == v, 1 + (ans + 100) % C, 1 + ans) for v in range(3)], axis=1)
        views = [all_of(cols, rows)] * 3

        def guard(case, m, ans=ans):
            assert np.array_equal(m["labels"], ans) and len(np.unique(m["labels"])) == 254
        out.append(_case(f"f3-g{g}", 3, B, C, (cols, rows, sheets), views, E=(1,), guard=guard))
    return out


# ---- family 4: bin counts ------------------------------------------------------------------------------------------------------------
def family4():
    """n = 320 = five waves (spatial_sort 0), V = 12.  Odd waves see all views and pile ten votes onto one of the bins 0..2; even waves see
    four views (0, 2, 6, 7) and give no bin more than three votes.  The last stage reads the planes in rows of four bins; the row
    behind the last bin of a wave's block is the next wave's bins 0..2 - without the `4 q + g < bins` mask an even wave would
    import the ten votes of its odd neighbour.  In every wave some winners are the last bin, some the last bin of a full row."""
    out = []
    V, n, W = 12, 320, 16
    even_views = (0, 2, 6, 7)
    for C in (1, 2, 3, 4, 150, 151, 152, 153, 155, 156, 207, 208, 254, 255):
        bins = C + 1
        i = np.arange(n)
        wave, lane = i // 64, i % 64
        odd = wave % 2 == 1
        # canvas: the odd waves on rows 0..7, the even ones behind them
        slot = np.where(odd, (wave // 2) * 64 + lane, 128 + (wave // 2) * 64 + lane)
        cols, rows, sheets = slot % W, slot // W, np.zeros(n, np.int64)
        views = [view(0, -1, -1, W + 2, (20 if v in even_views else 8) + 1) for v in range(V)]
        last = bins - 1
        full = 4 * (bins // 4) - 1 if bins >= 4 else last            # the last bin of a full row of four
        other = lambda b, k: (b + 1 + k % (bins - 1)) % bins         # a bin != b (bins >= 2)
        want = np.zeros((n, V), np.int64)
        for k in range(n):
            l = int(lane[k])
            if odd[k]:
                if l < 48:
                    pile = min(l % 3, bins - 1)
                    want[k, :10] = pile
                    want[k, 10:] = last
                else:
                    top = last if l % 2 else full
                    want[k, :] = [top if v % 2 == 0 or v == 11 else other(top, v + l) for v in range(V)]
            else:
                top = (last, full, last, full)[l % 4]
                if l % 8 < 4:                                        # X, top, top, top: the vote in view 0 is a loser's
                    seq = [other(top, l), top, top, top]
                else:                                                # top, X, X, top: a tie, the first vote decides
                    seq = [top, other(top, l), other(top, l), top]
                want[k, list(even_views)] = seq
        B = mask_votes(want, cols, rows, sheets, views)

        def guard(case, m, bins=bins, last=last, full=full, odd=odd):
            cnt, win = m["cnt"], m["winner"]
            for w in range(5):
                s = slice(64 * w, 64 * w + 64)
                assert (win[s] == last).any() and (win[s] == full).any()
            assert cnt[:, ~odd].max() <= 3
            if bins % 4:
                for w in (0, 2):                                     # the even waves that have an odd wave behind them
                    hits = 0
                    for l in range(64):
                        a, b = 64 * w + l, 64 * (w + 1) + l
                        for j in range(4 - bins % 4):                # the bins a read past the last row would take from wave w + 1
                            if j < bins and cnt[j, b] >= 10 > 3 >= cnt[:, a].max():
                                # ... and the first vote of that bin points at a view where Gaussian a did not vote its winner
                                hits += int(case["B"][a, m["first"][j, b]] != win[a])
                    assert hits >= 8, (w, hits)
        out.append(_case(f"f4-C{C}", 4, B, C, (cols, rows, sheets), views, E=() if C == 255 else (5,), guard=guard))
    return out


# ---- family 5: the orderings of the last stage ------------------------------------------------------------------------------------------
F5_PATTERNS = ("early_vs_late_equal", "late_one_more", "both_vs_late_equal", "two_late_tied_above_early", "two_early_first_0_and_Em1",
               "three_way", "unlabelled_wins_tie", "no_vote")


def f5_feasible(V, E):
    """Which of the listed patterns the split allows: a bin voted only in [E, V) needs V - E >= 2 views to lead an early bin by
    one, two late votes beside a late vote of the other bin need V - E >= 3, two late bins above an early one V - E >= 4; two
    early bins with first votes at views 0 and E - 1 need E >= 2.  (E = 8 and E = 12 allow every pattern.)"""
    out = set(F5_PATTERNS)
    if V - E < 2:
        out -= {"late_one_more"}
    if V - E < 3:
        out -= {"both_vs_late_equal"}      # A early + late against B late twice
    if V - E < 4:
        out -= {"two_late_tied_above_early"}   # two late bins with two votes each above an early bin's one
    if E < 2:
        out -= {"two_early_first_0_and_Em1"}
    return out


def _f5_votes(name, E, K, A, Bb, Cc, flip):
    """The votes {view: bin} that make the named pattern out of the views K a sparse Gaussian is seen by."""
    early, late = [v for v in K if v < E], [v for v in K if v >= E]
    s = {}
    if name == "early_vs_late_equal":
        s[early[0]], s[late[0]] = A, Bb
    elif name == "unlabelled_wins_tie":
        s[early[0]], s[late[0]] = 0, A
    elif name == "three_way":
        s[early[0]], s[late[0]] = A, Bb
        s[late[-1] if len(late) > 1 else early[-1]] = Cc
    elif name == "two_early_first_0_and_Em1":
        s[0], s[E - 1] = A, Bb
        if len(late) >= 2:
            s[late[0]], s[late[-1]] = (Bb, A) if flip else (A, Bb)
    elif name == "both_vs_late_equal":
        s[early[0]], s[late[1]], s[late[0]], s[late[2]] = A, A, Bb, Bb
    elif name == "late_one_more":
        t = min(2, len(early))
        for v in early[:t]:
            s[v] = A
        for v in late[:t + 1]:
            s[v] = Bb
    elif name == "two_late_tied_above_early":
        x, y = (Bb, A) if flip else (A, Bb)
        s[early[0]] = Cc
        s[late[0]], s[late[1]], s[late[2]], s[late[3]] = x, y, x, y
    else:
        raise ValueError(name)
    # a sparse Gaussian cannot abstain in a view that sees its row: the other views of K go to bins the pattern does not use
    spare = [b for b in range(7) if b not in s.values()]
    for j, v in enumerate(v for v in K if v not in s):
        s[v] = spare[j % len(spare)]
    return s


F5_GROUP = {"early_vs_late_equal": 0, "unlabelled_wins_tie": 0, "three_way": 0, "two_early_first_0_and_Em1": 0,
            "both_vs_late_equal": 1, "late_one_more": 1, "two_late_tied_above_early": 1}


def family5():
    """V = 24, C = 6, n = 256 = four waves of 64 patterns; one case per split point E (early = [0, E), late = [E, V)).
    Four groups of Gaussians by what sees them: `S1` only the views 0, E - 1, E, V - 1; `S2` those and 1, E - 2, E + 1, E + 2, V - 2;
    `full` every view; `parked` none.  Lanes 0..23 of a wave (rotated by five lanes from wave to wave) hold the named patterns,
    three times with other bins; the other 40 a five-to-five tie of two bins in the full group whose winner starts at a view of
    its own."""
    out = []
    V, C, n, W = 24, 6, 256, 16
    for E in (1, 8, 12, 23):
        K1 = sorted({0, E - 1, E, V - 1} & set(range(V)))
        K2 = sorted((set(K1) | {1, E - 2, E + 1, E + 2, V - 2}) & set(range(V)))
        feas = f5_feasible(V, E)
        group = np.zeros(n, np.int64)               # 0 S1, 1 S2, 2 full, 3 parked
        want = np.zeros((n, V), np.int64)
        for k in range(n):
            w, l = k // 64, (k % 64 + 5 * (k // 64)) % 64
            if l < 24:
                name = F5_PATTERNS[l % 8]
                if name == "no_vote":
                    group[k] = 3
                    continue
                if name not in feas:
                    name = ("early_vs_late_equal", "three_way", "unlabelled_wins_tie")[l % 3]
                group[k] = F5_GROUP[name]
                A, Bb, Cc = 1 + (l + w) % 6, 1 + (l + w + 1 + l // 8) % 6, 1 + (l + w + 4) % 6
                if Bb == A:
                    Bb = 1 + (A + 1) % 6
                if Cc in (A, Bb):
                    Cc = next(b for b in range(1, 7) if b not in (A, Bb))
                for v, b in _f5_votes(name, E, K2 if group[k] else K1, A, Bb, Cc, flip=(l // 8) % 2 == 1).items():
                    want[k, v] = b
            else:
                group[k] = 2
                j = l - 24
                f = 1 + j % 14
                A = 1 + (2 * (j // 14) + j + 2 * w) % 6
                Bb = 1 + A % 6
                rest = [b for b in range(7) if b not in (A, Bb)]
                s = np.full(V, -2, np.int64)
                s[[f, f + 2, f + 4, f + 6, f + 8]] = A
                s[[f + 1, f + 3, f + 5, f + 7, f + 9]] = Bb
                fill = np.flatnonzero(s == -2)
                s[fill] = [rest[(i + l) % 5] for i in range(len(fill))]
                want[k] = s
        # canvas rows: S1, S2, full, and the parked ones far away
        order = np.argsort(group, kind="stable")
        slot = np.empty(n, np.int64)
        slot[order] = np.arange(n)
        cnt_g = [int((group == g).sum()) for g in range(4)]
        rows_g = [-(-c // W) for c in cnt_g]
        start = np.cumsum([0] + cnt_g)
        row0 = [0, rows_g[0], rows_g[0] + rows_g[1], rows_g[0] + rows_g[1] + rows_g[2] + 50]
        local = slot - start[group]
        cols, rows, sheets = local % W, np.asarray(row0)[group] + local // W, np.zeros(n, np.int64)
        r_all = row0[2] + rows_g[2]
        first_row = lambda v: 0 if v in K1 else row0[1] if v in K2 else row0[2]
        views = [view(0, -1, first_row(v), W + 2, r_all - first_row(v)) for v in range(V)]
        B = mask_votes(want, cols, rows, sheets, views)

        def guard(case, m, E=E, feas=feas, B=B):
            cnt, first, win, top = m["cnt"], m["first"], m["winner"], m["top"]
            e_only = lambda b, i: cnt[b, i] > 0 and (B[i, E:] != b).all()
            l_only = lambda b, i: cnt[b, i] > 0 and first[b, i] >= E
            seen = set()
            for i in range(len(win)):
                if top[i] == 0:
                    seen.add("no_vote")
                    continue
                t = [b for b in range(7) if cnt[b, i] == top[i]]
                if len(t) >= 2 and e_only(win[i], i) and any(l_only(b, i) for b in t):
                    seen.add("early_vs_late_equal")
                if len(t) == 1 and l_only(win[i], i) and any(e_only(b, i) and cnt[b, i] == top[i] - 1 for b in range(7)):
                    seen.add("late_one_more")
                if len(t) >= 2 and first[win[i], i] < E and (B[i, E:] == win[i]).any() and any(l_only(b, i) for b in t):
                    seen.add("both_vs_late_equal")
                if len(t) >= 2 and all(l_only(b, i) for b in t) and any(first[b, i] < E for b in range(7) if cnt[b, i]):
                    seen.add("two_late_tied_above_early")
                if E >= 2 and len(t) >= 2 and sorted(int(first[b, i]) for b in t)[:2] == [0, E - 1]:
                    seen.add("two_early_first_0_and_Em1")
                if len(t) >= 3:
                    seen.add("three_way")
                if win[i] == 0 and len(t) >= 2:
                    seen.add("unlabelled_wins_tie")
            assert seen >= feas, (E, sorted(feas - seen))
            for w in range(4):
                idx = range(64 * w, 64 * w + 64)
                pairs = {(int(win[i]), int(first[win[i], i]) if win[i] >= 0 else -1) for i in idx}
                assert len(pairs) >= 48, (E, w, len(pairs))
                assert (top[64 * w:64 * w + 64] == 0).any()             # abstainers next to voters in every wave
        out.append(_case(f"f5-E{E}", 5, B, C, (cols, rows, sheets), views, E=(E,), guard=guard))
    return out


# ---- family 7: saturation ------------------------------------------------------------------------------------------------------------
def family7():
    V, C, n = 255, 5, 128
    cols, rows, sheets = grid(n, 16)
    v = np.arange(V)
    B = np.zeros((n, V), np.int64)
    for i in range(n):
        A, Bb = 1 + i % 5, 1 + (i + 1 + (i // 6) % 3) % 5
        if (i // 6) % 2:
            A, Bb = Bb, A
        kind = i % 6
        if kind == 0:
            B[i] = A                                     # 255 votes for one bin
        elif kind == 1:
            B[i] = A                                     # another bin in view 0, then 254
            B[i, 0] = Bb
        elif kind == 2:
            B[i] = np.where(v % 2 == 0, A, Bb)           # 128 : 127, the larger one first
        elif kind == 3:
            B[i] = np.where(v % 2 == 0, A, Bb)           # 128 : 127, the smaller one first
            B[i, 0], B[i, 1] = Bb, A
        elif kind == 4:
            B[i] = np.where(v % 2 == 0, A, Bb)           # 127 : 127 and one unlabelled pixel: the first voter wins
            B[i, 254 - 2 * (i % 7)] = 0
        else:
            B[i] = 0                                     # 254 unlabelled pixels and one label
            B[i, i % 255] = A
    views = [all_of(cols, rows)] * V

    def guard(case, m):
        assert m["cnt"].max() == 255 and (m["cnt"] == 254).any()
        two = np.sort(m["cnt"], axis=0)[-2:]
        assert ((two[1] == 128) & (two[0] == 127)).any()
        assert ((m["cnt"] == m["top"][None]) & (m["cnt"] > 0)).sum(0).max() >= 2
    return [_case("f7-saturation", 7, B, C, (cols, rows, sheets), views, E=(1, 128, 254), guard=guard)]


# ---- family 8: more than 255 views ---------------------------------------------------------------------------------------------------
def family8():
    """n = 300, C = 5.  `sparse` Gaussians are seen only by the views next to a batch boundary of either cut and by the last eight
    views; `full` ones by every view."""
    out = []
    n, C, W, PAD = 300, 5, 16, 8
    for V in (256, 257, 510, 511):
        cuts = sorted(set(balanced_bounds(V)[1:-1]) | set(early_bounds(V)[1:-1]))
        K = sorted({b - 1 for b in cuts} | set(cuts) | set(range(V - PAD, V)))
        names = np.empty(n, object)
        group = np.zeros(n, np.int64)                 # 0 sparse, 1 full
        want = np.zeros((n, V), np.int64)
        va = np.arange(V)
        for i in range(n):
            A, Bb = 1 + i % 5, 1 + (i + 2) % 5
            rest = [b for b in range(6) if b not in (A, Bb)]
            kind = i % 10
            if kind < 6:
                # sparse: A and B tie, first votes on either side of a boundary (kind even: A first; odd: B votes first and wins),
                # or both behind the first batch
                b = cuts[(i // 10) % len(cuts)]
                fa, fb = (b - 1, b) if kind < 4 else (b, min(v for v in K if v > b))
                if kind % 2:
                    fa, fb = fb, fa
                s = np.full(V, -1, np.int64)
                s[fa], s[fb] = A, Bb
                tail = [v for v in K if v > max(fa, fb)]
                for j, v in enumerate(tail[len(tail) % 2:]):
                    s[v] = A if j % 2 == 0 else Bb
                holes = [v for v in K if s[v] < 0]
                for j, v in enumerate(holes):
                    s[v] = rest[(j + i) % 4]
                want[i] = s
                names[i] = "straddle" if kind < 4 else "none_in_first_batch"
            else:
                group[i] = 1
                if kind == 6:
                    want[i] = A                                       # one bin in every view: a total beyond 255
                    names[i] = "every_view"
                elif kind == 7:
                    want[i] = np.where(va < balanced_bounds(V)[1], A, np.asarray(rest)[(va + i) % 4])     # decided by batch 0
                    want[i, V - 3:] = Bb
                    names[i] = "decided_by_batch0"
                elif kind == 8:
                    want[i] = np.where(va % 2 == 0, A, Bb)            # level until the end: the last view decides
                    if V % 2:
                        want[i, V - 2] = rest[0]
                    want[i, V - 1] = Bb
                    names[i] = "decided_by_last"
                else:
                    want[i] = np.where(va % 3 == 0, A, np.where(va % 3 == 1, Bb, rest[i % 4]))   # three-way, thirds
                    names[i] = "thirds"
        order = np.argsort(group, kind="stable")
        slot = np.empty(n, np.int64)
        slot[order] = np.arange(n)
        n_sparse = int((group == 0).sum())
        r_sparse = -(-n_sparse // W)
        slot = np.where(group == 1, r_sparse * W + (slot - n_sparse), slot)
        cols, rows, sheets = slot % W, slot // W, np.zeros(n, np.int64)
        r_all = int(rows.max()) + 1
        views = [view(0, -1, 0, W + 2, r_all) if v in K else view(0, -1, r_sparse, W + 2, r_all - r_sparse) for v in range(V)]
        B = mask_votes(want, cols, rows, sheets, views)

        def guard(case, m, V=V, cuts=cuts, names=names, B=B):
            cnt, first, win, top = m["cnt"], m["first"], m["winner"], m["top"]
            assert cnt.max() == V > 255
            ntied = ((cnt == top[None]) & (cnt > 0)).sum(0)
            b0 = balanced_bounds(V)[1]
            for b in cuts:                                            # a tie decided across every boundary, in both directions
                for lo_bin_wins in (True, False):
                    ok = False
                    for i in np.flatnonzero(ntied >= 2):
                        t = [x for x in range(6) if cnt[x, i] == top[i]]
                        f = sorted(int(first[x, i]) for x in t)
                        if f[0] == b - 1 and f[1] == b and (win[i] == min(t, key=lambda x: first[x, i])):
                            ok = ok or ((win[i] == 1 + i % 5) == lo_bin_wins)
                    assert ok, (V, b, lo_bin_wins)
            late = [i for i in np.flatnonzero(ntied >= 2) if min(first[x, i] for x in range(6) if cnt[x, i] == top[i]) >= min(cuts)]
            assert late, "no tie whose bins all start behind the first batch"
            # decided by batch 0: the winner's count there alone exceeds every other bin's total of the whole run
            c0 = vote_model(B[:, :b0], 6)["cnt"]
            others = np.where(np.arange(6)[:, None] == win[None, :], -1, cnt).max(axis=0)
            assert (c0[np.maximum(win, 0), np.arange(len(win))] > others).any()
            assert (vote_model(B[:, :V - 1], 6)["winner"] != win).any()
        out.append(_case(f"f8-V{V}", 8, B, C, (cols, rows, sheets), views, guard=guard))
    return out


# ---- family 9: map geometry --------------------------------------------------------------------------------------------------------------
def _cell_map(mw, mh, v, C):
    """Labels built from 4x4 cells: uniform, mixed, uniform with the top label C - 1, uniform -1; cells that stick out of the map
    at the right and bottom edge are uniform on their in-map part (and, two of them, mixed)."""
    y, x = np.mgrid[0:mh, 0:mw]
    cx, cy = x // 4, y // 4
    kind = (cx + 2 * cy + v + 3) % 5
    uni = (7 * cx + 13 * cy + 5 * v) % (C - 1)
    mixed = (31 * x + 17 * y + 3 * v) % C
    seg = np.where(kind == 0, uni, np.where(kind == 1, mixed, np.where(kind == 2, C - 1, np.where(kind == 3, -1, uni + (x % 4 == 3) * (cx % 2)))))
    ragged = (cx == (mw - 1) // 4) & (mw % 4 != 0) | (cy == (mh - 1) // 4) & (mh % 4 != 0)
    seg = np.where(ragged & (kind != 1), np.where(kind == 2, C - 1, uni), seg)
    return seg.astype(np.int64)


def family9():
    out = []
    V = 3
    for (mw, mh) in ((15, 7), (16, 8), (17, 9), (33, 5), (64, 32), (65, 33)):
        for variant in ("same", "half", "x1.5", "top255"):
            C = 255 if variant == "top255" else 254
            if variant == "top255" and (mw, mh) not in ((17, 9), (64, 32)):
                continue
            if variant in ("same", "top255"):
                fw, fh, img = mw, mh, (mw, mh)
            elif variant == "half":                      # the map is half the image; the frame is two pixels wider: clamp at the last column / row
                img = (2 * mw, 2 * mh)
                fw, fh = 2 * mw + 2, 2 * mh + 2
            else:                                        # the map is ~1.5 x the image; the frame two pixels more: clamp again
                img = (-(-2 * mw // 3), -(-2 * mh // 3))
                fw, fh = img[0] + 2, img[1] + 2
            n = fw * fh
            i = np.arange(n)
            cols, rows, sheets = i % fw, i // fw, np.zeros(n, np.int64)
            views = [view(0, 0, 0, fw, fh, map_shape=(mh, mw), img_size=img) for _ in range(V)]
            B = np.empty((n, V), np.int64)
            maps = []
            for v in range(V):
                seg = _cell_map(mw, mh, v, C)
                mx, my = map_pixel(views[v], cols, rows)
                B[:, v] = seg[my, mx] + 1
                maps.append(seg)

            def guard(case, m, maps=maps, C=C, mw=mw, mh=mh, variant=variant, views=views, cols=cols, rows=rows):
                cells = {"uniform": 0, "mixed": 0, "top": 0, "none": 0}
                for v, seg in enumerate(maps):
                    for cy in range(0, mh, 4):
                        for cx in range(0, mw, 4):
                            c = seg[cy:cy + 4, cx:cx + 4]
                            u = np.unique(c)
                            cells["mixed" if len(u) > 1 else "top" if u[0] == C - 1 else "none" if u[0] == -1 else "uniform"] += 1
                    mx, my = map_pixel(views[v], cols, rows)
                    assert (mx == mw - 1).any() and (my == mh - 1).any()
                    if variant in ("half", "x1.5"):      # the clamp really runs: the unclamped column is past the map
                        iw = views[v]["img_size"][0]
                        assert (np.trunc(cols.astype(np.float64) * (mw / iw)) > mw - 1).any()
                assert all(cells.values()), cells
                assert (m["labels"] == C - 1).any() and (m["labels"] == -1).any()
            out.append(_case(f"f9-{mw}x{mh}-{variant}", 9, B, C, (cols, rows, sheets), views, guard=guard, maps=maps,
                             seg_dtype=np.int64 if variant == "x1.5" else np.int32))
    return out


_ALL = None


def all_cases():
    """Every case, built once."""
    global _ALL
    if _ALL is None:
        _ALL = family1() + family1_cull() + family2() + family3() + family4() + family5() + family6() + family7() + family8() + family9()
    return _ALL


def cases_of(family, cull=False):
    return [c for c in all_cases() if c["family"] == family and bool(c.get("cull")) == cull]
