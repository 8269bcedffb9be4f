"""GPU: the bin kernels (csrc/render.hip: bin_kernel<EMIT, BIN32>, COUNT -> exclusive_scan_u32 -> EMIT; csrc/tile_test.hpp) through
gsx_debug_bin, which launches them with a frame's grids and arguments on the caller's arrays, against the plain model of
tests/bin_model.py on the cases of tests/bin_cases.py: wave totals around a 64-candidate round, one splat of 4096 and one of
65536 candidates, a splat straddling a round's end, empty splats at a wave's ends and in runs, phase windows that end inside a
wave under launches sized for more, all 441 rectangles of a 6x6 grid with and without 32x32 bins and `sat` bytes, exact culling
on needles and degenerate axes, and pair buffers one slot too small.  test_bin_model.py shows on the CPU that the cases are what
they claim, that no exact candidate lies where fp32 and fp64 could disagree, and that six wrong binners each fail a named case.

The comparison is exact: count, the 64-bit total, keys[:total] and vals[:total] are np.array_equal to the model's fully ordered
arrays, and everything behind them is still 0xFF.  The composition test chains the hooks of the pre pass, the level-1 sort,
the binning, the pair sort and the ranges on two scenes of blend_cases and compares every tile's list with blend_model's.

Measured on an MI355X, pairs binned of candidates walked, per group - the model's totals, every array reproduced bit for bit:
    rounds    45 cases  164351 of 164355 (big256: 65536, the fast path and the ballot path each)
    windows  108 cases   17732 of  17732 (no slot outside a window counted, the decoy's 256 tiles never seen)
    rects     12 cases   14256 of  18030      exact      9 cases     283 of    649
    capacity   6 cases   11406 of  15282, totals reported in full, nothing emitted where the buffers are one slot short
    composition: lengths 2866 pairs = the model's lists, with and without bins; needles 845 pairs = the model's q <= 4.04 set
    (0 within 1e-3 of it; 841 with a fragment, 848 with q <= 4.1, 1229 in the bounding boxes)"""
import numpy as np
import pytest

import bin_cases as bc
import bin_model as bm
import blend_cases

pytestmark = pytest.mark.gpu

U32 = np.uint32
FF = bm.FF
INVALID = "libgsx error -1"
_TOTALS = {}


def first_difference(name, c, b, cap, count, total, keys, vals):
    """None, or a sentence naming the first slot that differs from the model, with its splat, round and lane"""
    if not np.array_equal(count, b.count):
        rel = int(np.nonzero(count != b.count)[0][0])
        j = bm.window(c.nvis, c.div0, c.div1)[0] + rel
        return (f"{name}: count[{rel}] = {int(count[rel])}, model {int(b.count[rel])} of {int(b.area[rel])} candidates "
                f"(wave {rel // 64} lane {rel % 64}, splat {int(c.by_depth[j]) if j < len(c.by_depth) else None})")
    if total != b.total:
        return f"{name}: total {total}, model {b.total}"
    want_k, want_v = b.buffers(cap)
    for what, got, want in (("keys", keys, want_k), ("vals", vals, want_v)):
        if not np.array_equal(got, want):
            p = int(np.nonzero(got != want)[0][0])
            if p >= b.total or b.total > cap:
                return f"{name}: {what}[{p}] = {int(got[p]):#x} behind the {b.total} pairs (capacity {cap}): must stay 0xFF"
            rel, wave, lane, rnd = bm.where_is(b, p)
            return (f"{name}: {what}[{p}] = {int(got[p]):#x}, model {int(want[p]):#x}: splat {int(b.vals[p]) & 0xFFFFFFF}, slot {rel} "
                    f"(wave {wave} lane {lane}), candidate {int(b.local[p])} of its rectangle, round {rnd} of the wave's walk")
    return None


@pytest.mark.parametrize("name", list(bc.all_cases()))
def test_every_case_bit_for_bit(ctx, name):
    c, b, cap = bc.expected(name)
    count, total, keys, vals = ctx.debug_bin(**c.hook_args(cap))
    _TOTALS[name] = total
    print(f"{name}: {c.n} splats, window {bm.window(c.nvis, c.div0, c.div1)}, m_cap {c.m_cap}: {total} pairs of "
          f"{int(b.area.astype(np.int64).sum())} candidates, capacity {cap}")
    diff = first_difference(name, c, b, cap, count, total, keys, vals)
    if diff:
        print(diff)
    assert diff is None, diff


def test_totals_per_group(ctx):
    """the figures of the module docstring"""
    for g in bc.GROUPS:
        names = list(bc.group(g))
        for name in names:
            if name not in _TOTALS:
                c, b, cap = bc.expected(name)
                _TOTALS[name] = ctx.debug_bin(**c.hook_args(cap))[1]
        cands = sum(int(bc.expected(n)[1].area.astype(np.int64).sum()) for n in names)
        print(f"{g}: {len(names)} cases, {sum(_TOTALS[n] for n in names)} pairs of {cands} candidates")
        assert sum(_TOTALS[n] for n in names) == sum(bc.expected(n)[1].total for n in names)


# ---- the refusals ---------------------------------------------------------------------------------------------------------------
def valid_args():
    rect = np.array([bm.pack_rect(0, 1, 0, 1), bm.EMPTY_RECT, bm.pack_rect(3, 3, 2, 3), bm.pack_rect(1, 2, 1, 1)], U32)
    rec = np.zeros((4, 12), np.float32)
    return dict(tile_rect=rect, rec=rec, by_depth=np.array([2, 0, 3, 1], U32), nvis=3, div0=0, div1=1, m_cap=3, H=60, tiles_x=4,
                tiles_y=4, bin32=False, exact=False, sat=None, pair_cap=16)


def outside(tx0, tx1, ty0, ty1):
    rect = valid_args()["tile_rect"]
    rect[3] = bm.pack_rect(tx0, tx1, ty0, ty1)
    return rect


REFUSED = {
    "an index of by_depth[0, nvis) >= n": dict(by_depth=np.array([2, 0, 4, 1], U32)),
    "an index far beyond n": dict(by_depth=np.array([0xFFFFFFFF, 0, 3, 1], U32)),
    "nvis > len": dict(nvis=5, m_cap=5),
    "a rectangle beyond tiles_x": dict(tile_rect=outside(3, 4, 0, 0)),
    "a rectangle beyond tiles_y": dict(tile_rect=outside(0, 0, 2, 4)),
    "a rectangle of a splat the window does not reach": dict(tile_rect=outside(0, 255, 0, 255), nvis=2, m_cap=2),
    "tiles_x above 256": dict(tiles_x=257),
    "tiles_y above 256": dict(tiles_y=257),
    "tiles_x below 1": dict(tiles_x=0),
    "m_cap below the window's length": dict(m_cap=2),
    "m_cap below a later window's length": dict(by_depth=np.array([2, 0, 3, 1, 0, 0, 0, 0], U32), nvis=8, div0=4, div1=1, m_cap=5),
    "m_cap < 1": dict(nvis=0, m_cap=0),
    "div1 < 1": dict(div1=0),
    "div1 negative": dict(div1=-1),
    "pair_cap < 1": dict(pair_cap=0),
    "bin32 with exact": dict(bin32=True, exact=True),
    "exact without rec": dict(exact=True, rec=None),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_the_hook_refuses(ctx, what):
    with pytest.raises(ValueError, match=INVALID):
        ctx.debug_bin(**dict(valid_args(), **REFUSED[what]))


def test_the_hook_refuses_a_pair_cap_above_2_31_minus_1(ctx, gsx):
    """straight at the C entry: no array of 2^31 entries is made for a call that must not get that far"""
    a = valid_args()
    count, keys, total = np.empty(3, U32), np.empty(4, U32), np.zeros(1, np.uint64)
    call = lambda cap: gsx.lib().gsx_debug_bin(
        ctx.h, 4, a["tile_rect"].ctypes.data, None, a["by_depth"].ctypes.data, 4, 3, 0, 1, 3, 60, 4, 4, 0, 0, None, cap,
        count.ctypes.data, total.ctypes.data_as(gsx._lib.C.POINTER(gsx._lib.C.c_uint64)), keys.ctypes.data, keys.ctypes.data)
    assert call(1 << 31) == gsx._lib.GSX_E_INVALID and call(1 << 40) == gsx._lib.GSX_E_INVALID


def test_the_hook_accepts_what_the_refusals_start_from(ctx):
    a = valid_args()
    for exact in (False, True):
        count, total, keys, vals = ctx.debug_bin(**dict(a, exact=exact))          # (zero axes: q = 0, every tile is kept)
        assert count.tolist() == [2, 4, 2] and total == 8
        assert keys[:8].tolist() == [11, 15, 0, 1, 4, 5, 5, 6] and vals[:8].tolist() == [2, 2, 0, 0, 0, 0, 3, 3]
        assert (keys[8:] == FF).all() and (vals[8:] == FF).all()


# ---- the hooks of a frame's front half, chained -----------------------------------------------------------------------------------
def binned_lists(ctx, name, bin32, exact):
    """pre pass -> level-1 sort -> binning -> pair sort -> ranges, each through its hook -> (per tile the splats listed, in list
    order; position of every splat in the depth order; the pair total)"""
    p = blend_cases.prepared(name)
    sc, m = p.scene, p.model
    ctx.upload_splats(*sc.arrays())
    out = ctx.debug_render_pre([sc.cam], sc.W, sc.H)[0]
    n = len(out["key"])
    _, by_depth = ctx.sort_pairs_drop(out["key"], np.arange(n, dtype=U32), 16)
    boxes = sum(len(l) for l in m.lists)
    count, total, keys, vals = ctx.debug_bin(out["rect_bucket"], out["rec"], by_depth, len(by_depth), 0, 1, n, sc.H, m.tiles_x, m.tiles_y,
                                             bin32=bin32, exact=exact, pair_cap=boxes + 7)
    assert total <= boxes and int(count.astype(np.int64).sum()) == total
    assert (keys[total:] == FF).all() and (vals[total:] == FF).all()
    lists_x = (m.tiles_x + 1) // 2 if bin32 else m.tiles_x
    nlists = lists_x * ((m.tiles_y + 1) // 2 if bin32 else m.tiles_y)
    bits = max(1, int(nlists - 1).bit_length())
    k, v = ctx.sort_pairs(keys[:total], vals[:total], bits)
    ranges = ctx.ranges(k, total, nlists)
    pos = np.full(n, -1, np.int64)
    pos[by_depth] = np.arange(len(by_depth))
    lists = []
    for t in range(m.tiles_x * m.tiles_y):
        ty, tx = divmod(t, m.tiles_x)
        lo, hi = ranges[(ty // 2) * lists_x + tx // 2 if bin32 else t]
        mine = v[lo:hi]
        if bin32:
            mine = mine[(mine >> 28) & (1 << (2 * (ty & 1) + (tx & 1))) != 0]
        lists.append((mine & U32(0xFFFFFFF)).astype(np.int64))
    return lists, pos, total


@pytest.mark.parametrize("bin32", [False, True])
def test_composition_lengths_lists_are_the_models(ctx, bin32):
    m = blend_cases.prepared("lengths").model
    lists, pos, total = binned_lists(ctx, "lengths", bin32, False)
    print(f"lengths bin32={bin32}: {total} pairs binned, {sum(len(l) for l in m.lists)} in the model's lists")
    for t, got in enumerate(lists):
        want = sorted(set(m.lists[t].tolist()), key=lambda i: pos[i])
        assert len(want) == len(m.lists[t]) == blend_cases.LENGTHS[t] and (pos[want] >= 0).all()
        assert got.tolist() == want, f"tile {t}"
    if not bin32:
        assert total == sum(blend_cases.LENGTHS)


def test_composition_needles_lists_under_exact_culling(ctx):
    """a pair is kept iff q <= 4.04 somewhere on the rectangle of the tile's pixel centres: every list holds the model's pairs with
    a fragment, holds none with q > 4.1, equals the q <= 4.04 set when no pair is within 1e-3 of 4.04, and is in depth order"""
    m = blend_cases.prepared("needles").model
    lists, pos, total = binned_lists(ctx, "needles", False, True)
    unsure = n_exact = n_lo = n_hi = 0
    per_tile = []
    for t, ids in enumerate(m.lists):
        frag = m.has_fragment(t)
        lo, hi, exact = set(), set(), set()
        for k, i in enumerate(ids.tolist()):
            x0, x1, r0, r1 = m.rec.box[i]
            one_tile = x0 // 16 == x1 // 16 and r0 // 16 == r1 // 16          # a one-tile rectangle is not tested
            q = 0.0 if one_tile else m.rect_min_q(t, i)
            if frag[k]:
                lo.add(i)
            if q <= 4.1:
                hi.add(i)
            if q <= 4.04:
                exact.add(i)
            unsure += abs(q - 4.04) < 1e-3
        per_tile.append((lo, hi, exact))
        n_lo, n_hi, n_exact = n_lo + len(lo), n_hi + len(hi), n_exact + len(exact)
    print(f"needles, exact culling: {total} pairs binned; model: {n_exact} with q <= 4.04 ({unsure} within 1e-3 of it), {n_lo} with a "
          f"fragment, {n_hi} with q <= 4.1, {sum(len(l) for l in m.lists)} in the bounding boxes")
    for t, got in enumerate(lists):
        lo, hi, exact = per_tile[t]
        g = got.tolist()
        assert len(set(g)) == len(g) and lo <= set(g) <= hi, f"tile {t}"
        assert g == sorted(g, key=lambda i: pos[i]), f"tile {t}: not in depth order"
        if unsure == 0:
            assert set(g) == exact, f"tile {t}"
