"""CPU: the model of tests/bin_model.py and the cases of tests/bin_cases.py that tests/test_bin_gpu.py holds the bin kernels to.
The cases are what they claim (wave totals, straddle offsets, windows, no exact candidate in the unsure band); the fp64 minimum
of q is the true one (both edge orders, dense sampling) and exact culling never loses a fragment; a second model that walks a wave
the way the kernel does - 64 candidates a round, owner search, verdict masks, kept_run - gives the plain model's arrays on every
case, and six deliberately wrong variants of it each differ on a case named here.  Models only: no kernel is built or run."""
import numpy as np
import pytest

import bin_cases as bc
import bin_model as bm

FF = bm.FF


# ---- a wave-level model: the kernel's structure, with switches for six mistakes -------------------------------------------------
WRONG = ("first_owner", "kept_run_dropped", "mask_bits_swapped", "sat_is_one", "window_to_wave_end", "column_major")


def wave_model(c, wrong=None):
    """-> (count (m_cap,), total, keys, vals (total,), 0xFF where nothing was written): COUNT, scan and EMIT of bin_kernel as 64
    lanes in numpy.  The tile test itself is bin_model's.  A mutant's out-of-range slot or index is dropped, not written."""
    assert wrong in (None,) + WRONG
    bin32, exact, sat = c.bin32, c.exact, c.sat
    sh = 1 if bin32 else 0
    lists_x = (c.tiles_x + 1) // 2 if bin32 else c.tiles_x
    j0, j1 = bm.window(c.nvis, c.div0, c.div1)
    if wrong == "window_to_wave_end":
        j1 = min(j0 + -(-(j1 - j0) // 64) * 64, len(c.by_depth)) if j1 > j0 else j1
    lane = np.arange(64)
    nwaves = -(-c.m_cap // bc.KRB) * 4
    fast = not exact and sat is None
    sat_ok = (lambda b: b != 1) if wrong == "sat_is_one" else (lambda b: b == 0)

    def run(emit, offset, keys, vals):
        count = np.full(c.m_cap, FF, np.uint32)
        for w in range(nwaves):
            rel = w * 64 + lane
            j = j0 + rel
            live, slot = j < j1, rel < c.m_cap
            i = np.where(live, c.by_depth[np.minimum(j, len(c.by_depth) - 1)], 0).astype(np.int64)
            rect = np.where(live, c.rect[i], bm.EMPTY_RECT).astype(np.int64)
            tx0, tx1, ty0, ty1 = rect & 255, (rect >> 8) & 255, (rect >> 16) & 255, rect >> 24
            wdt = np.where(tx1 >= tx0, (tx1 >> sh) - (tx0 >> sh) + 1, 0)
            hgt = np.where(ty1 >= ty0, (ty1 >> sh) - (ty0 >> sh) + 1, 0)
            area = wdt * hgt
            cstart = np.cumsum(area) - area
            total = int(area.sum())
            if total == 0:
                if not emit:
                    count[rel[slot]] = 0
                continue
            if not emit and fast:
                count[rel[slot]] = area[slot]
                continue
            my_off = np.where(live, offset[np.minimum(rel, c.m_cap - 1)], 0).astype(np.int64) if emit else None
            kept_run = np.zeros(64, np.int64)
            for base in range(0, total, 64):
                e = base + lane
                valid = e < total
                target = np.where(valid, e, total - 1)
                lo, hi = np.zeros(64, np.int64), np.full(64, 63, np.int64)
                for _ in range(6):                                  # the LAST lane whose candidates start at or before target
                    mid = (lo + hi + 1) >> 1
                    le = cstart[mid] <= target
                    lo, hi = np.where(le, mid, lo), np.where(le, hi, mid - 1)
                if wrong == "first_owner":
                    lo = np.searchsorted(cstart, cstart[lo], side="left")
                s_start, s_w, s_h = cstart[lo], np.maximum(wdt[lo], 1), np.maximum(hgt[lo], 1)
                local = target - s_start
                if wrong == "column_major":
                    rx, ry = local // s_h, local % s_h
                else:
                    ry, rx = local // s_w, local % s_w
                tx, ty = (tx0[lo] >> sh) + rx, (ty0[lo] >> sh) + ry
                tile = ty * lists_x + tx
                keep = valid.copy()
                m = np.zeros(64, np.int64)
                if bin32:
                    for dy in (0, 1):
                        for dx in (0, 1):
                            x, y = 2 * tx + dx, 2 * ty + dy
                            inside = (x >= tx0[lo]) & (x <= tx1[lo]) & (y >= ty0[lo]) & (y <= ty1[lo])
                            if sat is not None:
                                inside &= sat_ok(sat.reshape(-1, 4)[np.minimum(tile, len(sat) // 4 - 1), 2 * dy + dx])
                            m |= inside.astype(np.int64) << (2 * dy + dx)
                    keep &= m != 0
                    if wrong == "mask_bits_swapped":
                        m = (m & 9) | (m & 2) << 1 | (m & 4) >> 1
                if exact:
                    for k in np.nonzero(keep & (area[lo] > 1))[0]:
                        keep[k] = bm.exact_keeps(c.rec[i[lo[k]]], c.H, int(tx[k]), int(ty[k]))
                if not bin32 and sat is not None:
                    keep &= sat_ok(sat[np.minimum(tile, len(sat) - 1)])
                val = i[lo] | m << 28
                if emit and fast:
                    pos = my_off[lo] + local
                else:
                    before = np.concatenate([[0], np.cumsum(keep)])            # kept candidates of this round below bit b
                    blo, bhi = np.clip(cstart - base, 0, 64), np.clip(cstart - base + area, 0, 64)
                    mine = before[bhi] - before[blo]
                    pos = my_off[lo] + kept_run[lo] + before[lane] - before[np.clip(s_start - base, 0, 64)] if emit else None
                    kept_run = mine if wrong == "kept_run_dropped" else kept_run + mine
                if emit:
                    ok = keep & (pos >= 0) & (pos < len(keys))
                    keys[pos[ok]], vals[pos[ok]] = tile[ok], val[ok]
            if not emit:
                count[rel[slot]] = kept_run[slot]
        return count

    count = run(False, None, None, None)
    total = int(count.astype(np.int64).sum())
    offset = np.cumsum(count.astype(np.int64)) - count
    keys, vals = np.full(total, FF, np.uint32), np.full(total, FF, np.uint32)
    run(True, offset, keys, vals)
    return count, total, keys, vals


def same(c, b, got):
    count, total, keys, vals = got
    return np.array_equal(count, b.count) and total == b.total and np.array_equal(keys, b.keys) and np.array_equal(vals, b.vals)


@pytest.mark.parametrize("group", list(bc.GROUPS))
def test_wave_model_gives_the_plain_models_arrays(group):
    for name in bc.group(group):
        c, b, _ = bc.expected(name)
        assert same(c, b, wave_model(c)), name


# each mistake and the cases that must show it
CAUGHT_BY = {
    "first_owner": ["empty_lane0/fast", "empty_run_1/zero_sat", "empty_run_62/fast", "only_lane63/zero_sat"],
    "kept_run_dropped": ["straddle_60_70/zero_sat", "straddle_60_70/sat", "big64_lane31/zero_sat", "big256/zero_sat", "exact_diagonal"],
    "mask_bits_swapped": ["rects441_x6_bin32", "rects441_x7_bin32_sat", "corner256_bin32_sat"],
    "sat_is_one": ["rects441_x6_sat", "rects441_x7_bin32_sat", "corner256_sat", "corner256_bin32_sat", "straddle_60_70/sat",
                   "exact_all_sat"],
    "window_to_wave_end": ["window_63_0_1_n", "window_65_0_1_n", "window_1000_0_4_n", "window_1000_4_2_n", "window_65_2_1_n", "window_1_0_1_n"],
    "column_major": ["rects441_x6", "rects441_x7_bin32", "straddle_60_70/fast", "exact_diagonal", "corner256"],
}


@pytest.mark.parametrize("wrong", WRONG)
def test_the_cases_tell_a_wrong_binner_from_a_right_one(wrong):
    assert set(CAUGHT_BY) == set(WRONG)
    for name in CAUGHT_BY[wrong]:
        c, b, _ = bc.expected(name)
        assert not same(c, b, wave_model(c, wrong)), f"{wrong} passes {name}"


# ---- the cases are what they claim ----------------------------------------------------------------------------------------------
def lane_areas(c):
    """candidates per slot of the phase, in depth order"""
    return bc.expected(c.name)[1].area.astype(np.int64)


def test_round_cases_are_what_they_claim():
    g = bc.group("rounds")
    for T in bc.WAVE_TOTALS:
        for kind in ("fast", "zero_sat"):
            c = g[f"wave_total_{T}/{kind}"]
            assert c.n == 64 and lane_areas(c).sum() == T and (c.sat is None) == (kind == "fast")
            assert bc.expected(c.name)[1].total == T                                   # nothing is culled: every candidate is a pair
    for lane in (0, 31, 63):
        a = lane_areas(g[f"big64_lane{lane}/fast"])
        assert a[lane] == 4096 and (np.delete(a, lane) == 1).all()
    c = g["big256/fast"]
    b = bc.expected(c.name)[1]
    assert c.tiles_x == 256 and b.total == 65536 == 1024 * 64 and b.keys[-1] == 65535
    a = lane_areas(g["straddle_60_70/fast"])
    start = np.cumsum(a) - a
    assert (start[60], start[60] + a[60]) == (60, 70) and g["straddle_60_70/fast"].meta["straddle"] == (60, 60, 70)
    c, b, _ = bc.expected("straddle_60_70/sat")
    lost = sorted(set(range(10)) - set(b.local[b.rel == 60].tolist()))                  # ranks of the straddler's lost candidates
    assert lost == [1, 3, 5, 7] and {60 + k < 64 for k in lost} == {True, False}         # on both sides of the round's end
    for lane in (0, 63):
        a = lane_areas(g[f"empty_lane{lane}/fast"])
        assert a[lane] == 0 and (np.delete(a, lane) > 0).all()
        a = lane_areas(g[f"only_lane{lane}/zero_sat"])
        assert a[lane] == 9 and a.sum() == 9
    for run in (1, 2, 62):
        a = lane_areas(g[f"empty_run_{run}/fast"])
        assert a[0] > 0 and (a[1:1 + run] == 0).all() and a[1 + run] > 0 and (a > 0).sum() == 64 - run
    a = lane_areas(g["waves_empty_full/fast"]).reshape(4, 64)
    assert (a[0] == 0).all() and (a[2] == 0).all() and (a[1] == 2).all() and (a[3] == 2).all()
    c = g["ragged_833/zero_sat"]
    assert c.n == 3 * bc.KRB + 65 and c.m_cap == c.n and (lane_areas(c) == 0).sum() > 100
    for name, c in g.items():                                                          # every case in both forms
        assert name.endswith(("/fast", "/zero_sat", "/sat")) and (c.sat is None or name.endswith("sat"))
        if name.endswith("/zero_sat"):
            assert not c.sat.any() and name[:-9] + "/fast" in g
            assert same(c, bc.expected(name[:-9] + "/fast")[1], wave_model(c))          # the ballot path must give the fast path's arrays


def test_window_cases_are_what_they_claim():
    g = bc.group("windows")
    assert len(g) == len(bc.NVIS) * len(bc.DIVS) * 2
    ends_inside_a_wave = lengths = 0
    for name, c in g.items():
        j0, j1 = bm.window(c.nvis, c.div0, c.div1)
        L = max(0, j1 - j0)
        assert c.meta["window"] == (j0, j1) and len(c.by_depth) == c.n > c.nvis and c.m_cap >= max(1, L)
        decoy = c.n - 1
        assert c.rect[decoy] == bc.DECOY_RECT
        outside = np.ones(c.n, bool)
        outside[j0:j0 + L] = False
        assert (c.by_depth[outside] == decoy).all() and (c.by_depth[~outside] < c.nvis).all()
        b = bc.expected(name)[1]
        assert (b.count[L:] == 0).all() and b.total < 256 + 4 * L and (b.vals != decoy).all()
        if name.endswith("_n"):
            assert c.m_cap == max(1, c.n // c.div1)
        else:
            assert c.m_cap == max(1, L)
        ends_inside_a_wave += L % 64 != 0
        lengths += L > 0
    assert ends_inside_a_wave > 40 and lengths > 60


def test_rect_cases_are_what_they_claim():
    g = bc.group("rects")
    r = bc.rects441()
    assert len(r) == len(set(r)) == 441 and all(bm.unpack_rect(v)[1] <= 5 and bm.unpack_rect(v)[3] <= 5 for v in r)
    for tiles_x in (6, 7):
        plain, b32 = bc.expected(f"rects441_x{tiles_x}")[1], bc.expected(f"rects441_x{tiles_x}_bin32")[1]
        assert plain.total == sum(bm.rect_area(v) for v in r) == 3136
        assert b32.total == sum(bm.rect_area(v, True) for v in r)
        assert sorted(set((b32.vals >> 28).tolist())) == [1, 2, 3, 4, 5, 8, 10, 12, 15]     # every mask a rectangle can leave
        bits = sum(int(bin(m).count("1")) for m in (b32.vals >> 28).tolist())
        assert bits == plain.total                                                      # the masks name the tiles, each once
        c = g[f"rects441_x{tiles_x}_sat"]
        assert sorted(set(c.sat.tolist())) == sorted(bc.SAT_BYTES) and c.lists() == len(c.sat)
        cb = g[f"rects441_x{tiles_x}_bin32_sat"]
        assert cb.lists() == len(cb.sat) == 4 * ((tiles_x + 1) // 2) * 3
        sat_plain, sat_b32 = bc.expected(c.name)[1], bc.expected(cb.name)[1]
        bits = sum(int(bin(m).count("1")) for m in (sat_b32.vals >> 28).tolist())
        assert bits == sat_plain.total < plain.total                                    # the same pattern per tile
        full = (b32.vals >> 28)[np.isin(b32.vals & 0xFFFFFFF, sat_b32.vals & 0xFFFFFFF)]
        assert sat_b32.total < b32.total                                                # some bins lose all of their mask
        assert len(full) and (np.sort(sat_b32.vals >> 28) != np.sort(b32.vals >> 28)[:sat_b32.total]).any()   # some a part
    b = bc.expected("corner256")[1]
    assert b.keys.tolist() == [254 * 256 + 254, 254 * 256 + 255, 255 * 256 + 254, 255 * 256 + 255]
    b = bc.expected("corner256_bin32")[1]
    assert b.keys.tolist() == [127 * 128 + 127] and b.vals.tolist() == [15 << 28]
    assert bc.expected("corner256_bin32_sat")[1].vals.tolist() == [11 << 28] and bc.expected("corner256_sat")[1].total == 3


def test_capacity_cases_are_what_they_claim():
    for name, c in bc.group("capacity").items():
        _, b, cap = bc.expected(name)
        assert b.total == c.meta["total"] and cap == c.pair_cap
        keys, vals = b.buffers(cap)
        if "short_by_one" in name:
            assert cap == b.total - 1 and (keys == FF).all() and (vals == FF).all()
        else:
            assert cap == b.total and np.array_equal(keys, b.keys) and np.array_equal(vals, b.vals)


# ---- exact culling --------------------------------------------------------------------------------------------------------------
def candidates_of(c):
    """(splat, tx, ty) of every candidate of the phase"""
    for j in range(*bm.window(c.nvis, c.div0, c.div1)):
        i = int(c.by_depth[j])
        tx0, tx1, ty0, ty1 = bm.unpack_rect(c.rect[i])
        for ty in range(ty0, ty1 + 1):
            for tx in range(tx0, tx1 + 1):
                yield i, tx, ty


def pixel_q(rec_i, H, tx, ty):
    """fp64 q at the tile's 16x16 pixel centres"""
    x0, _, _, y1 = bm.tile_box(float(rec_i[0]), float(rec_i[1]), H, tx, ty)
    x, y = np.meshgrid(x0 + np.arange(16.0), y1 - np.arange(16.0))
    r = rec_i.astype(np.float64)
    return (x * r[2] + y * r[3]) ** 2 + (x * r[4] + y * r[5]) ** 2


def test_no_exact_candidate_lies_in_the_unsure_band():
    """|q - 4.04| < 1e-3 * 4.04 is where the kernel's fp32 minimum and the model's fp64 one may fall on different sides: no
    (splat, tile) candidate of any exact case is there, tested or not, so every one of them is compared"""
    seen = 0
    nearest = np.inf
    for name, c in bc.group("exact").items():
        assert c.exact and not c.bin32 and c.H % 16 != 0 and c.rec.shape == (c.n, 12)
        for i, tx, ty in candidates_of(c):
            q = bm.rect_min_q(c.rec[i][0], c.rec[i][1], c.rec[i][2:4], c.rec[i][4:6], c.H, tx, ty)
            assert not abs(q - bm.Q_KEEP) < bm.BAND, (name, i, tx, ty, q)
            nearest = min(nearest, abs(q - bm.Q_KEEP)) if q == q else nearest
            seen += 1
    print(f"{seen} exact candidates, the nearest {nearest:.3f} from 4.04")
    assert seen > 400 and nearest >= bm.BAND


def test_exact_cases_are_what_they_claim():
    g = bc.group("exact")

    def kept(name, which):
        c, b, _ = bc.expected("exact_" + name)
        i = int(np.nonzero(c.rect == bc.EXACT_SPLATS[which][0])[0][0])
        return c, b.keys[(b.vals == i)].tolist(), bm.rect_area(c.rect[i])

    c, keys, area = kept("diagonal", "diagonal")
    assert area == 64 and 16 <= len(keys) <= 32                                        # a band along the diagonal of 8x8 tiles
    c, keys, area = kept("axis", "axis")
    assert area == 24 and 0 < len(keys) < 8 and {k // 8 for k in keys} == {3}
    c, keys, area = kept("huge_g", "huge_g")
    assert area == 9 and keys == [4 * 8 + 3]
    c, keys, area = kept("one_tile_far", "one_tile_far")
    assert area == 1 and keys == [7] and bm.rect_min_q(8.0, bc.EXACT_H - 100.0, (1, 0), (0, 1), c.H, 7, 0) > 1000
    c, keys, area = kept("zero_g", "zero_g")
    assert len(keys) == area == 16
    c, keys, area = kept("den0", "den0")
    assert area == 48 and sorted({k // 8 for k in keys}) == [3, 4] and len(keys) == 16
    c, keys, area = kept("nan_g", "nan_g")
    assert len(keys) == area == 16
    a, s = bc.expected("exact_all")[1], bc.expected("exact_all_sat")[1]
    assert 0 < s.total < a.total and len(g["exact_all"].rect) == 40 + len(bc.EXACT_SPLATS)
    for c in g.values():                                                               # centres on eighths, axes dyadic
        ok = np.isfinite(c.rec)
        assert (np.where(ok, c.rec * 1024, 0) % 1 == 0).all() and (np.where(ok[:, :2], c.rec[:, :2] * 8, 0) % 1 == 0).all()


def test_exact_culling_never_loses_a_fragment():
    """the kept tiles are a superset of the tiles in which some pixel centre has q <= 4"""
    with_fragment = culled = 0
    for name, c in bc.group("exact").items():
        if c.sat is not None:
            continue
        b = bc.expected(name)[1]
        kept = set(zip((b.vals & 0xFFFFFFF).tolist(), b.keys.tolist()))
        for i, tx, ty in candidates_of(c):
            frag = bool((pixel_q(c.rec[i], c.H, tx, ty) <= 4.0).any())
            with_fragment += frag
            culled += (i, ty * c.tiles_x + tx) not in kept
            assert not frag or (i, ty * c.tiles_x + tx) in kept, (name, i, tx, ty)
    assert with_fragment > 50 and culled > 100


def test_rect_min_q_is_the_minimum_over_the_rectangle():
    """both edge orders give the same number; a dense sampling of the rectangle never goes below it and comes as close as its
    spacing allows: with q = |G d|^2, a sample within delta of the minimiser has sqrt(q) <= sqrt(qmin) + |G|_F |delta|"""
    rng = np.random.default_rng(20276)
    recs = [np.asarray(s[1], np.float64) for s in bc.EXACT_SPLATS.values() if np.isfinite(s[1]).all()]
    for _ in range(60):
        t = rng.uniform(0, np.pi)
        a, b = 2.0 ** rng.uniform(-6, 1, 2)
        recs.append(np.array([rng.uniform(-20, 150), rng.uniform(-20, 150), a * np.cos(t), a * np.sin(t), -b * np.sin(t), b * np.cos(t)]))
    inside = outside = 0
    for r in recs:
        for tx, ty in ((0, 0), (3, 4), (7, 7), (int(r[0]) // 16 % 8, int(bc.EXACT_H - r[1]) // 16 % 8)):
            q = bm.rect_min_q(r[0], r[1], r[2:4], r[4:6], bc.EXACT_H, tx, ty)
            assert q == bm.rect_min_q(r[0], r[1], r[2:4], r[4:6], bc.EXACT_H, tx, ty, reverse=True)
            x0, x1, y0, y1 = bm.tile_box(r[0], r[1], bc.EXACT_H, tx, ty)
            step = 15.0 / 240
            x, y = np.meshgrid(np.linspace(x0, x1, 241), np.linspace(y0, y1, 241))
            dense = float(((x * r[2] + y * r[3]) ** 2 + (x * r[4] + y * r[5]) ** 2).min())
            reach = np.sqrt((r[2:6] ** 2).sum()) * step / np.sqrt(2.0)
            assert dense >= q - 1e-9 * max(1.0, q), (r, tx, ty, dense, q)
            assert np.sqrt(dense) <= np.sqrt(q) + reach + 1e-9, (r, tx, ty, dense, q)
            inside += q == 0.0
            outside += q > 0.0
    assert inside > 20 and outside > 100
    assert np.isnan(bm.rect_min_q(1.0, 1.0, (float("nan"), 0.0), (0.0, 1.0), 123, 2, 2))
    assert np.isnan(bm.rect_min_q(1.0, 1.0, (float("nan"), 0.0), (0.0, 1.0), 123, 2, 2, reverse=True))
    assert bm.exact_keeps(np.array([1.0, 1.0, float("nan"), 0, 0, 1.0]), 123, 2, 2)
