"""The four multi-rank vote exchanges (3d_gaussian_splatting_project_amd/dist.py, include/gsx.h) restated in integer numpy ON THE
VOTE MATRIX of tests/vote_cases.py, and the constructed cases that meet their constants: candidate words of 32 bins, slabs of
ceil(ceil(n / W) / 256) * 256 Gaussians, u8 counters at 255, totals above 255, the switch to 16-bit planes, the tie order
"lowest rank that voted a candidate, then its earliest local view".

exchange_model(B, bins, world, spans) takes no scene and no projection: rank r owns the columns spans[r] of B.  Every protocol's
final labels must be vote_model(B, bins)["labels"]; the model asserts that itself.  tests/test_exchange_model.py proves the
model equal to the oracle's numpy stand-ins array for array on the CPU; tests/test_exchange_edges_gpu.py pins the kernels to it.

No GPU import here, and everything is deterministic."""
import numpy as np

import vote_cases as vc

CAND_WORDS = 8     # kCandWords of vote.hip: 256 bins in words of 32


def view_range(V, rank, world):
    """dist.view_range, restated (the CPU test holds the two together)."""
    base, rem = divmod(V, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def slab_size(n, world):
    return ((n + world - 1) // world + 255) // 256 * 256 or 256


def first_view_of(lo, total):
    """What the front-end announces for a rank (deep_learning_segmentation.py): a rank without views still names a view inside the run."""
    return min(lo, max(total - 1, 0))


def _slab_major(plane, world, sn):
    """[bins][world * sn] -> [slab][bins][sn]"""
    bins = plane.shape[0]
    return np.ascontiguousarray(plane.reshape(bins, world, sn).transpose(1, 0, 2))


def _padded(a, width):
    out = np.zeros(a.shape[:-1] + (width,), a.dtype)
    out[..., :a.shape[-1]] = a
    return out


def _sum_words(words):
    """SUM of int32 words as an all-reduce does it: modulo 2^32, carries run from byte to byte."""
    return (np.sum([w.view(np.uint32).astype(np.uint64) for w in words], axis=0) & 0xffffffff).astype(np.uint32).view(np.int32)


def exchange_model(B, bins, world, spans=None, protocols=("v1", "v2", "v3", "v4")):
    B = np.asarray(B)
    n, V = B.shape
    spans = [view_range(V, r, world) for r in range(world)] if spans is None else [tuple(s) for s in spans]
    assert len(spans) == world and spans[0][0] == 0 and spans[-1][1] == V and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    whole = vc.vote_model(B, bins)
    want = whole["labels"]
    ranks = []
    for lo, hi in spans:
        m = vc.vote_model(B[:, lo:hi], bins)
        voted = m["cnt"] > 0
        ranks.append({"lo": lo, "hi": hi, "first_view": first_view_of(lo, V), "cnt": m["cnt"], "first": m["first"], "voted": voted})
    total = np.sum([r["cnt"] for r in ranks], axis=0)
    assert np.array_equal(total, whole["cnt"])
    top = total.max(axis=0, initial=0)
    cand = (total == top[None, :]) & (total > 0)
    out = {"spans": spans, "ranks": ranks, "labels": want, "total": total, "cand": cand, "n": n, "bins": bins, "world": world}
    idx = np.arange(n)

    if "v1" in protocols:
        wide = V > 255
        fvmax, dt = (65535, np.uint16) if wide else (255, np.uint8)
        n_pad = slab_size(n, 1)
        v1 = {"wide": wide, "n_pad": n_pad, "words": [], "fv": [], "keys": []}
        for r in ranks:
            assert r["cnt"].max(initial=0) <= fvmax
            v1["words"].append(_padded(r["cnt"].astype(dt), n_pad).reshape(-1).view(np.int32))
            gcode = np.where(r["voted"], fvmax - (r["lo"] + r["first"]), 0)
            assert gcode.min(initial=0) >= 0 and (gcode[r["voted"]] > 0).all()
            v1["fv"].append(gcode)
            key = np.where(cand & r["voted"], (gcode << 8) | np.arange(bins)[:, None], 0).max(axis=0, initial=0)
            v1["keys"].append(_padded(key.astype(np.int32), n_pad))
        v1["sum"] = _sum_words(v1["words"])
        assert np.array_equal(v1["sum"].view(dt).reshape(bins, n_pad)[:, :n], total), "a counter carried into its neighbour"
        v1["max"] = np.max(v1["keys"], axis=0) if ranks else np.zeros(n_pad, np.int32)
        k = v1["max"][:n]
        v1["labels"] = np.where(k != 0, (k & 0xff) - 1, -1).astype(np.int32)
        assert np.array_equal(v1["labels"], want)
        out["v1"] = v1

    sn = slab_size(n, world)
    out["sn"] = sn
    inside = (np.arange(world * sn) < n).reshape(world, sn)       # [slab][sn]: a Gaussian, not a pad entry
    out["inside"] = inside
    local_ok = all(hi - lo <= 255 for lo, hi in spans)

    if local_ok and ("v2" in protocols or "v3" in protocols):
        cnt_pl, fv_pl = [], []
        for r in ranks:
            code = np.where(r["voted"], 255 - r["first"], 0)
            cnt_pl.append(_slab_major(_padded(r["cnt"].astype(np.uint8), world * sn), world, sn))
            fv_pl.append(_slab_major(_padded(code.astype(np.uint8), world * sn), world, sn))
        recv_cnt = [np.stack([cnt_pl[s][j] for s in range(world)]) for j in range(world)]      # rank j: [src][bins][sn]
        recv_fv = [np.stack([fv_pl[s][j] for s in range(world)]) for j in range(world)]
        want_slabs = _padded(want, world * sn).reshape(world, sn)
        want_slabs = np.where(inside, want_slabs, -1).astype(np.int32)

    if local_ok and "v2" in protocols:
        slabs = []
        for j in range(world):
            rc, rf = recv_cnt[j].astype(np.int64), recv_fv[j].astype(np.int64)
            tot = rc.sum(0)
            first_r = np.argmax(rc > 0, axis=0)
            key = np.where(tot > 0, ((world - first_r) << 8) | np.take_along_axis(rf, first_r[None], 0)[0], 0)
            M = tot.max(0, initial=0)
            c = (tot == M[None]) & (tot > 0)
            ck = np.where(c, key, -1)
            assert ((ck == ck.max(0)[None]).sum(0)[M > 0] == 1).all()          # one vote per view: no two bins share a key
            slabs.append(np.where(M > 0, ck.argmax(0) - 1, -1).astype(np.int32))
        assert np.array_equal(np.stack(slabs), want_slabs)
        out["v2"] = {"cnt": cnt_pl, "fv": fv_pl, "recv_cnt": recv_cnt, "recv_fv": recv_fv, "slabs": slabs}

    if local_ok and "v3" in protocols:
        tied_labels, masks = [], []
        for j in range(world):
            tot = recv_cnt[j].astype(np.int64).sum(0)
            M = tot.max(0, initial=0)
            c = (tot == M[None]) & (M[None] > 0)
            nmax = c.sum(0)
            tied_labels.append(np.where(nmax == 0, -1, np.where(nmax == 1, c.argmax(0) - 1, -2)).astype(np.int32))
            words = np.zeros((CAND_WORDS, sn), np.uint32)
            for b in range(bins):
                words[b >> 5] |= c[b].astype(np.uint32) << np.uint32(b & 31)
            masks.append(words)
        ntied = cand.sum(axis=0) >= 2
        codes = []
        for r in ranks:
            Br = B[:, r["lo"]:r["hi"]]
            hit = (Br >= 0) & cand[np.maximum(Br, 0), idx[:, None]] if Br.shape[1] else np.zeros((n, 0), bool)
            v = hit.argmax(axis=1) if Br.shape[1] else np.zeros(n, np.int64)
            any_hit = hit.any(axis=1) & ntied
            b = Br[idx, v] if Br.shape[1] else np.zeros(n, np.int64)
            code = np.where(any_hit, ((255 - v) << 8) | b, 0).astype(np.uint16)
            codes.append(_padded(code, world * sn))                             # u16 [world][sn], flat; pad entries are zero
        recv_codes = [np.stack([codes[s].reshape(world, sn)[j] for s in range(world)]) for j in range(world)]
        resolved, decider = [], np.full(world * sn, -1)
        for j in range(world):
            lab = tied_labels[j].copy()
            rc = recv_codes[j]
            has = rc != 0
            fr = has.argmax(0)
            pick = (rc[fr, np.arange(sn)].astype(np.int64) & 0xff) - 1
            t = lab == -2
            lab[t] = np.where(has.any(0), pick, -1)[t]
            decider[j * sn:(j + 1) * sn][t] = fr[t]
            resolved.append(lab.astype(np.int32))
        assert np.array_equal(np.stack(resolved), want_slabs)
        out["v3"] = {"cnt": cnt_pl, "recv_cnt": recv_cnt, "tied": tied_labels, "masks": masks, "codes": codes, "recv_codes": recv_codes,
                     "slabs": resolved, "decider": decider[:n]}

    if "v4" in protocols:
        slices = [(min(n, r * sn), min(n, (r + 1) * sn)) for r in range(world)]
        out["v4"] = {"slices": slices, "slabs": [want[a:b] for a, b in slices]}
        assert np.array_equal(np.concatenate(out["v4"]["slabs"]) if world else want, want)
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def _xcase(name, family, B, C, place, views, worlds, guard=None, spans=None, protocols=("v1", "v2", "v3", "v4"), **extra):
    """A vote_cases.Case with the ranks it is split over: worlds (the world sizes it runs at), spans (world -> the ranks' view
    blocks where they are not view_range's), protocols."""
    c = vc._case(name, family, B, C, place, views, guard=guard, **extra)
    c["worlds"], c["spans"], c["protocols"] = tuple(worlds), dict(spans or {}), tuple(protocols)
    return c


def xmodel(case, world):
    key = ("xmodel", world)
    if key not in case:
        case[key] = exchange_model(case["B"], case["bins"], world, case["spans"].get(world), case["protocols"])
    return case[key]


def spans_of(case, world):
    V = case["B"].shape[1]
    return case["spans"].get(world) or [view_range(V, r, world) for r in range(world)]


def _tied(m):
    return ((m["cnt"] == m["top"][None, :]) & (m["cnt"] > 0)).sum(axis=0) >= 2


def x1_cases():
    """Ranks and views: V round the chunk of 8 and below the world size, windows of rows that make ~10 % of the pairs abstain,
    tied maxima as in family 1."""
    out = []
    n, C, W = 257, 5, 16
    for V in (1, 2, 3, 7, 8, 9, 16, 17):
        rng = np.random.default_rng(7100 + V)
        cols, rows, sheets = vc.grid(n, W)
        R = int(rows.max()) + 1
        views = []
        for v in range(V):
            r0, r1 = int(rng.integers(0, 3)), R - int(rng.integers(0, 3))
            views.append(vc.view(0, -1, r0, W + 2, r1 - r0))
        vis = np.stack([vc.visible(cols, rows, sheets, vw) for vw in views], axis=1)
        B = np.full((n, V), -1, np.int64)
        for i in range(n):
            B[i, vis[i]] = vc._tied_votes(rng, int(vis[i].sum()), C + 1)

        def guard(case, m, V=V):
            if V >= 2:
                assert _tied(m).mean() >= 0.30, _tied(m).mean()
            if V >= 7:
                assert 0.03 < np.mean(case["B"] < 0) < 0.25
            for world in case["worlds"]:
                sizes = [hi - lo for lo, hi in spans_of(case, world)]
                if V < world:
                    assert min(sizes) == 0
        out.append(_xcase(f"x1-V{V}", "x1", B, C, (cols, rows, sheets), views, worlds=(1, 2, 3, 8), guard=guard))
    return out


def x2_cases():
    """Slab geometry: n at the edges of sn = ceil(ceil(n / W) / 256) * 256; every Gaussian an answer of its own (family 2)."""
    out = []
    V, C = 9, 150
    for world in (2, 3, 8):
        for n in (1, 255, 256, 257, 256 * world - 1, 256 * world, 256 * world + 1):
            cols, rows, sheets = vc.grid(n, 16)
            i = np.arange(n)
            own = 1 + (i * 7) % C
            B = np.empty((n, V), np.int64)
            for v in range(V):
                major = ((v + i) % 9) < 5
                B[:, v] = np.where(major, own, 1 + (own + 11 * v + 3) % C)
            views = [vc.all_of(cols, rows)] * V

            def guard(case, m, own=own, n=n, world=world):
                assert np.array_equal(m["labels"], own - 1)
                for w in range(0, n - 63, 64):
                    assert len(set(own[w:w + 64].tolist())) == 64
                sn = slab_size(n, world)
                sizes = [max(0, min(n, (r + 1) * sn) - r * sn) for r in range(world)]
                assert sum(sizes) == n
                if n <= 256 * (world - 1):
                    assert sizes[-1] == 0                       # an empty slab
            out.append(_xcase(f"x2-W{world}-n{n}", "x2", B, C, (cols, rows, sheets), views, worlds=(world,), guard=guard))
    return out


def _spread(V, cand_views, fillers, cap):
    """A row of B: the candidates' votes where cand_views = {bin: views} puts them, every other view a filler bin, round robin,
    no filler more than `cap` times."""
    s = np.full(V, -1, np.int64)
    for b, vs in cand_views.items():
        for v in vs:
            assert s[v] < 0
            s[v] = b
    holes = np.flatnonzero(s < 0)
    assert len(holes) <= cap * len(fillers), (len(holes), cap, len(fillers))
    for j, v in enumerate(holes):
        s[v] = fillers[j % len(fillers)]
    return s


def x3_patterns(bins):
    """The candidate-word patterns a plane of `bins` bins allows: (name, maximal bins, decoys one vote below the maximum)."""
    nw = (bins + 31) // 32
    lo = lambda k: 32 * k
    hi = lambda k: min(32 * k + 31, bins - 1)
    mid = lambda k: min(32 * k + 13, bins - 1)
    pats = []
    for k in range(nw):
        top = sorted({lo(k), hi(k)})                      # bits 0 and 31 of the word where it is a full one
        decoys = ([mid(k - 1)] if k > 0 else []) + ([mid(k + 1)] if k + 1 < nw else [])
        pats.append((f"only{k}", top, decoys))
    if nw > 1:
        pats.append((f"span0-{nw - 1}", [hi(0), lo(nw - 1)], [mid(nw // 2)] if nw > 2 else []))
    if nw > 4:
        pats.append(("span3-4", [hi(3), lo(4)], [mid(2), mid(5)]))
        pats.append(("span3-4-inner", [lo(3) + 1, hi(4) - 1 if hi(4) - 1 > lo(4) else lo(4)], [mid(0), mid(7 if nw > 7 else nw - 1)]))
    if nw > 1:
        # an early word that looks tied at M - 1 until one bin of a later word overtakes it: that Gaussian is NOT tied
        pats.append(("overtaken", [mid(nw - 1)], [lo(0), hi(0)]))
    else:
        pats.append(("overtaken", [hi(0)], [lo(0), mid(0)]))
    return pats


def x3_cases():
    """Candidate words: C at the bin counts where a word of 32 starts or ends (V = 12), and 256 bins with every word index (V = 18)."""
    out = []
    n, W, world = 700, 16, 3
    for C, V in [(c, 12) for c in (31, 32, 33, 63, 64, 65, 254, 255)] + [(255, 18)]:
        bins = C + 1
        pats = x3_patterns(bins)
        M = 3 if V == 12 else 4
        cols, rows, sheets = vc.grid(n, W)
        B = np.empty((n, V), np.int64)
        for i in range(n):
            wave, lane = divmod(i, 64)
            name, top, decoys = pats[(lane + 3 * wave) % len(pats)]
            rot = (5 * i + wave) % V
            order = [(rot + 7 * k) % V for k in range(V)]        # 7 is coprime to 12 and 18: every view once
            slots = iter(order)
            cv = {}
            bs = list(top) if (i // len(pats)) % 2 == 0 else list(top)[::-1]       # either candidate may come first
            for b in bs:
                cv[b] = [next(slots) for _ in range(M)]
            for d in decoys:
                cv[d] = [next(slots) for _ in range(M - 1)]
            used = set(top) | set(decoys)
            fillers = [b for b in ((11 * i + 37 * k + 5) % bins for k in range(3 * V)) if b not in used]
            fillers = list(dict.fromkeys(fillers))[:V]
            B[i] = _spread(V, cv, fillers, 1)
        views = [vc.all_of(cols, rows)] * V

        def guard(case, m, bins=bins, pats=pats, n=n):
            cnt, top = m["cnt"], m["top"]
            cand = (cnt == top[None]) & (cnt > 0)
            nw = (bins + 31) // 32
            assert _tied(m).mean() >= 0.30
            wordset = [frozenset((np.flatnonzero(cand[:, i]) >> 5).tolist()) for i in range(n)]
            # the running maximum as the totals kernel meets it: a word that held the maximum so far and is overtaken later
            run = np.maximum.accumulate(cnt, axis=0)
            for w0 in range(0, n - 63, 64):
                ws = set(wordset[w0:w0 + 64])
                for k in range(nw):
                    assert frozenset({k}) in ws, (w0, k)
                if nw > 1:
                    assert frozenset({0, nw - 1}) in ws, w0
                if nw > 4:
                    assert frozenset({3, 4}) in ws, w0
                sl = slice(w0, w0 + 64)
                full = [k for k in range(nw) if 32 * k + 31 < bins]
                assert any((cand[32 * k, sl] & cand[32 * k + 31, sl]).any() for k in full) or not full, w0       # bits 0 and 31
                voided = before = after = False
                for i in range(w0, w0 + 64):
                    cw = sorted(wordset[i])
                    dec = np.flatnonzero(cnt[:, i] == top[i] - 1) >> 5
                    before |= bool((dec < cw[0]).any())
                    after |= bool((dec > cw[-1]).any())
                    for k in range(cw[0]):
                        end = run[min(32 * k + 31, bins - 1), i]
                        voided |= bool(end > 0 and (cnt[32 * k:32 * k + 32, i] == end).sum() >= 1 and end < top[i])
                assert nw == 1 or (voided and before and after), (w0, voided, before, after)
            untied_over = [i for i in range(n) if not _tied(m)[i] and (cnt[:, i] == top[i] - 1).sum() >= 2]
            assert len(untied_over) >= n // (2 * len(pats))
        out.append(_xcase(f"x3-C{C}-V{V}", "x3", B, C, (cols, rows, sheets), views, worlds=(world,), guard=guard))
    return out


X4_SPARSE = (  # 12 votes of the ranks 0, 1 and last, four each: A, B the candidates (three votes each), x a filler (<= 2 a bin)
    ("last_vs_rank1", "xxxx" "BxBx" "AAAB", "B"),          # A voted by the last rank only, B first by rank 1, rank 0 no candidate
    ("rank0_a_first", "xABx" "xABx" "xABx", "A"),
    ("rank0_b_first", "xBAx" "xABx" "xABx", "B"),
    ("rank1_b_first", "xxxx" "xBAx" "ABAB", "B"),
    ("rank0_last_view", "xxxA" "BBBx" "AAxx", "A"),
)
X4_PAIRS = {6: [(0, 3), (5, 1), (2, 4), (4, 2), (1, 5), (3, 0), (0, 5), (5, 0)],
            256: [(0, 200), (255, 1), (31, 32), (224, 7), (7, 255), (100, 0), (0, 255), (255, 0), (64, 63), (96, 160)]}
X4_FILL = {6: list(range(6)), 256: [64, 130, 250, 33, 1, 2, 191, 95]}


def x4_cases():
    """Tie order across ranks.  Four views a rank.  Rows of `sparse` Gaussians are seen by the ranks 0, 1 and last only (at world 3:
    by all), `full` ones by every view, `late` ones by the last rank alone; the patterns say in which rank and local view each
    candidate is voted first."""
    out = []
    W, n_sparse, n_full, n_late = 16, 192, 129, 32
    n = n_sparse + n_full + n_late
    for world in (3, 8):
        for C in (5, 255):
            bins, V, last = C + 1, 4 * world, world - 1
            i = np.arange(n)
            slot = np.where(i < n_sparse + n_full, i, (-(-(n_sparse + n_full) // W)) * W + i - n_sparse - n_full)
            cols, rows, sheets = slot % W, slot // W, np.zeros(n, np.int64)   # the sparse ones fill the first 12 rows, the late ones the last 2
            r_all = int(rows.max()) + 1
            r_full, r_late = n_sparse // W, -(-(n_sparse + n_full) // W)
            active = [0, 1, 2, 3, 4, 5, 6, 7] + list(range(4 * last, 4 * last + 4))
            views = [vc.view(0, -1, 0, W + 2, r_all if v >= 4 * last else r_late) if v in active else
                     vc.view(0, -1, r_full, W + 2, r_late - r_full) for v in range(V)]
            want = np.zeros((n, V), np.int64)
            kinds = np.empty(n, object)
            for k in range(n):
                win, lose = X4_PAIRS[bins][(k // 3) % len(X4_PAIRS[bins])]
                fill = [b for b in X4_FILL[bins] if b not in (win, lose)][:4]
                if k < n_sparse:
                    name, pat, winner = X4_SPARSE[k % len(X4_SPARSE)]
                    A, Bb = (win, lose) if winner == "A" else (lose, win)
                    j = 0
                    for s, v in zip(pat, active):
                        if s == "x":
                            want[k, v] = fill[(j + k) % 4]
                            j += 1                                # six fillers over four bins in turn: no bin more than twice
                        else:
                            want[k, v] = A if s == "A" else Bb
                    kinds[k] = name
                elif k >= n_sparse + n_full:                     # seen by the last rank alone: every other rank holds no vote at all
                    want[k, 4 * last:] = (win, lose, win, lose) if k % 2 else (win, lose, lose, win)
                    kinds[k] = "late"
                else:
                    g = k % 3
                    rest = np.arange(4, V)
                    s = np.empty(V, np.int64)
                    if g == 0:                                   # rank 0 votes four fillers, rank 1 starts with the winner
                        s[:4] = fill
                        s[rest] = np.where((rest - 4) % 2 == 0, win, lose)
                    elif g == 1:                                 # ... the winner comes second in rank 1's block, the loser third
                        s[:4] = fill
                        s[rest] = np.where((rest - 4) % 2 == 0, lose, win)
                        s[4], s[5], s[6], s[7] = fill[0], win, lose, fill[1]
                    else:                                        # the winner's only early vote is view 0 of rank 0
                        s[:4] = [win, fill[0], fill[1], fill[2]]
                        s[rest] = np.where((rest - 4) % 2 == 0, lose, win)
                        s[V - 1] = fill[3]
                    want[k] = s
                    kinds[k] = f"full{g}"
            B = vc.mask_votes(want, cols, rows, sheets, views)

            def guard(case, m, world=world, bins=bins, kinds=kinds):
                xm = xmodel(case, world)
                tied = _tied(m)
                assert tied.mean() >= 0.9
                cand = xm["cand"]
                dec = xm["v3"]["decider"]
                assert np.mean(dec[tied] != 0) >= 0.20
                lowest = cand.argmax(axis=0)
                assert np.mean(m["winner"][tied] != lowest[tied]) >= 0.10
                largest = np.where(cand, np.arange(bins)[:, None], -1).max(axis=0)
                assert np.mean(m["winner"][tied] == largest[tied]) >= 0.10 and np.mean(m["winner"][tied] == lowest[tied]) >= 0.10
                r0 = xm["ranks"][0]
                no_cand = (r0["cnt"].sum(0) > 0) & ~(r0["voted"] & cand).any(0)
                assert np.mean(no_cand[tied]) >= 0.10
                assert (m["winner"][tied] == 0).any() and (m["winner"][tied] == bins - 1).any()
                code0 = xm["v3"]["codes"][0][:len(tied)]          # rank 0 emits code 0 exactly where it voted no candidate
                assert np.array_equal(code0[tied] != 0, (r0["voted"] & cand).any(0)[tied]) and (code0[no_cand] == 0).all()
                assert set(kinds.tolist()) == {p[0] for p in X4_SPARSE} | {"full0", "full1", "full2", "late"}
                assert (dec[kinds == "late"] == world - 1).all() and (dec[tied] == 1).any()
            out.append(_xcase(f"x4-W{world}-C{C}", "x4", B, C, (cols, rows, sheets), views, worlds=(world,), guard=guard))
    return out


def x5_cases():
    out = []
    C, W = 5, 16
    # (a) world 2: rank 0 owns 255 views, rank 1 one.  `sparse` rows are seen by the views 254 and 255 only.
    n, V = 160, 256
    cols, rows, sheets = vc.grid(n, W)
    r_all, r_sparse = int(rows.max()) + 1, 2
    views = [vc.view(0, -1, 0, W + 2, r_all) if v >= 254 else vc.view(0, -1, r_sparse, W + 2, r_all - r_sparse) for v in range(V)]
    want = np.zeros((n, V), np.int64)
    va = np.arange(V)
    for i in range(n):
        A, Bb = 1 + i % 5, 1 + (i + 2) % 5
        if i < r_sparse * W:
            want[i, 254], want[i, 255] = (A, Bb) if i % 2 else (Bb, A)       # the only candidate vote of rank 0 is its local view 254
            if i % 8 == 7:
                want[i, 254] = want[i, 255] = 0
        else:
            kind = i % 4
            if kind == 0:
                want[i] = A                                                    # rank counter 255, total 256
            elif kind == 1:
                want[i] = A
                want[i, 255] = Bb                                              # rank counter 255, total 255
            elif kind == 2:
                want[i] = np.where(va % 2 == 0, A, Bb)                         # 128 : 128, first votes at local views 0 and 1
            else:
                want[i] = np.where(va % 2 == 0, Bb, A)
                want[i, 0] = 0                                                 # 127 : 128 and one unlabelled pixel
    B = vc.mask_votes(want, cols, rows, sheets, views)

    def guard_a(case, m):
        xm = xmodel(case, 2)
        assert xm["ranks"][0]["cnt"].max() == 255 and m["cnt"].max() == 256 and (m["cnt"] == 255).any()
        codes0 = xm["v3"]["codes"][0][:len(m["top"])]
        assert ((codes0 >> 8) == 1).sum() >= 8                                 # code 1 << 8 | b: local view 254
        assert xm["v1"]["wide"] and xm["ranks"][1]["first_view"] == 255
    out.append(_xcase("x5a-255+1", "x5", B, C, (cols, rows, sheets), views, worlds=(2,), spans={2: [(0, 255), (255, 256)]}, guard=guard_a))

    # (b) world 8, 33 views a rank: totals above 255 out of u8 rank counters; 16-bit planes under v1
    n, V = 300, 264
    cols, rows, sheets = vc.grid(n, W)
    views = [vc.all_of(cols, rows)] * V
    B = np.zeros((n, V), np.int64)
    va = np.arange(V)
    for i in range(n):
        A, Bb = 1 + i % 5, 1 + (i + 1 + i // 5 % 3) % 5
        kind = i % 5
        if kind == 0:
            B[i] = A                                                           # 264
        elif kind == 1:
            B[i] = np.where(va % 33 == i % 33, Bb, A)                          # 256 : 8
        elif kind == 2:
            B[i] = np.where(va % 2 == 0, A, Bb)                                # 132 : 132
        elif kind == 3:
            B[i] = np.where(va % 2 == 0, Bb, A)
            B[i, :33] = 0                                                      # rank 0 votes the unlabelled bin only; 115 : 116 ...
            B[i, 33 + 2 * (i % 16)] = 0                                        # ... level again at 115 : 115, rank 1 decides
        else:
            B[i] = np.where(va < 128, A, np.where(va < 256, Bb, 0))            # 128 : 128, the candidates' ranks do not overlap
    def guard_b(case, m):
        assert m["cnt"].max() == 264 and ((m["cnt"] > 255) & (m["cnt"] < 264)).any() and _tied(m).mean() >= 0.30
        xm = xmodel(case, 8)
        assert max(r["cnt"].max() for r in xm["ranks"]) == 33 and xm["v1"]["wide"]
        assert (xm["v3"]["decider"][_tied(m)] == 1).any()
    out.append(_xcase("x5b-8x33", "x5", B, C, (cols, rows, sheets), views, worlds=(8,), guard=guard_b))

    # (c) v1 only: the packed SUM at 255 a byte, the switch to 16-bit planes at 256, a rank with more than 255 views of its own
    n = 128
    cols, rows, sheets = vc.grid(n, W)
    for V, worlds, spans in ((255, (2, 3), None), (256, (2, 3), None), (400, (2,), {2: [(0, 300), (300, 400)]})):
        views = [vc.all_of(cols, rows)] * V
        B = np.zeros((n, V), np.int64)
        va = np.arange(V)
        for i in range(n):
            A, Bb = 1 + i % 5, 1 + (i + 2) % 5
            kind = i % 8
            if kind in (0, 2):
                B[i] = 1 + (i // 8) % 5                                        # byte V (255: saturated) twice in a word of four ...
            elif kind == 1:
                B[i] = 0                                                       # ... with a neighbour's 0 between them
            elif kind == 3:
                B[i] = A
                B[i, (37 * i) % V] = Bb                                        # V - 1 and 1
            elif kind == 4:
                B[i] = np.where(va % 2 == 0, A, Bb)                            # level (or one apart): the first views decide
            elif kind == 5:
                B[i] = np.where(va % 2 == 0, Bb, A)
                B[i, 0] = 0
                if V % 2 == 0:
                    B[i, 2] = 0
            elif V >= 400 and kind in (6, 7):
                # candidates voted from view 254 (kind 6: on either side of a rank's own batch boundary 254 | 255) or 255 on only,
                # 73 : 73 or 72 : 72 above four other bins of at most 64 votes
                start = 254 if kind == 6 else 255
                rest = np.asarray([b for b in range(6) if b not in (A, Bb)])
                B[i] = np.where(va < start, rest[va % 4], np.where((va - start) % 2 == 0, Bb, A))
                if (V - start) % 2:
                    B[i, V - 1] = rest[0]
            elif kind == 6:
                B[i] = np.where(va % 2 == 0, Bb, A)
                B[i, V - 1] = B[i, V - 2] = 0
            else:
                B[i] = np.where(va < V // 3, A, np.where(va < 2 * (V // 3), Bb, 0))   # three blocks, level where 3 | V
        def guard_c(case, m, V=V, worlds=worlds):
            assert m["cnt"].max() == V
            for world in worlds:
                xm = xmodel(case, world)
                assert xm["v1"]["wide"] == (V > 255)
                if V == 255:                                                   # bytes of 255 next to bytes of 0 and of 255 in one word
                    w = xm["v1"]["sum"].view(np.uint8).reshape(-1, 4)
                    assert ((w == 255).any(1) & (w == 0).any(1)).any() and ((w == 255).sum(1) >= 2).any()
                if V == 400:
                    assert xm["spans"][0] == (0, 300)
                    cnt0, first0 = xm["ranks"][0]["cnt"], xm["ranks"][0]["first"]
                    assert (cnt0 > 255).any() and ((first0 >= 255) & (cnt0 > 0)).any()      # bins the second batch votes first
        out.append(_xcase(f"x5c-V{V}", "x5", B, C, (cols, rows, sheets), views, worlds=worlds, spans=spans, protocols=("v1",), guard=guard_c))
    return out


def x6_cases():
    """Workgroup order: family 3's grids of g + 1 workgroups at world 2, now with ties (vote_tie_kernel walks them)."""
    out = []
    C, V = 254, 4
    for g in (6, 7, 8, 14, 15, 16, 17, 32):
        n = 256 * g + 1
        cols, rows, sheets = vc.grid(n, 64)
        i = np.arange(n)
        a = 1 + (i * 37) % C
        o = 1 + (i * 37 + 100) % C
        x, y = 1 + (i * 37 + 31) % C, 1 + (i * 37 + 57) % C
        k = i % 4
        B = np.stack([np.where(k == 0, a, np.where(k == 1, o, x)),
                      np.where(k == 0, o, np.where(k == 1, a, np.where(k == 2, y, a))),
                      np.where(k == 0, a, np.where(k == 1, o, np.where(k == 2, a, y))),
                      np.where(k == 0, o, a)], axis=1)
        views = [vc.all_of(cols, rows)] * V

        def guard(case, m):
            assert _tied(m).mean() >= 0.30 and len(np.unique(m["labels"])) == 254
        out.append(_xcase(f"x6-g{g}", "x6", B, C, (cols, rows, sheets), views, worlds=(2,), protocols=("v3", "v4"), guard=guard))
    return out


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = x1_cases() + x2_cases() + x3_cases() + x4_cases() + x5_cases() + x6_cases()
    return _ALL


def cases_of(family):
    return [c for c in all_cases() if c["family"] == family]
