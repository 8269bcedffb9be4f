"""Rectangles and records placed on the structural edges of the bin kernels (csrc/render.hip: bin_kernel<EMIT, BIN32>;
csrc/tile_test.hpp), shared by test_bin_model.py (CPU: the cases are what they claim) and test_bin_gpu.py.  No scene and no
camera: a case is the arrays gsx_debug_bin takes.  A workgroup is 256 splats (kRB), a wave 64, a round of the wave's walk 64
candidates; a splat's lane is its slot of the phase mod 64.  The largest case holds 1300 splats or 65536 pairs."""
import functools

import numpy as np

import bin_model as bm

WAVE = 64
KRB = 256
EMPTY = bm.EMPTY_RECT
WAVE_TOTALS = (0, 1, 63, 64, 65, 127, 128, 129)
NVIS = (0, 1, 63, 64, 65, 255, 256, 257, 1000)
DIVS = ((0, 1), (0, 4), (4, 2), (2, 1), (16, 4), (0, 1 << 40))
SAT_BYTES = (0, 0x01, 0x80, 0xFF)
EXACT_TILES, EXACT_H = 8, 8 * 16 - 5          # exact cases: 8x8 tiles, the bottom row of tiles cut by the frame


class Case:
    """the arguments of Context.debug_bin plus `meta`; pair_cap None: the model's total + 5 (a tail that must stay 0xFF)"""

    def __init__(self, name, rect, by_depth, tiles=(16, 16), nvis=None, div=(0, 1), m_cap=None, H=None, bin32=False, exact=False,
                 rec=None, sat=None, pair_cap=None, **meta):
        self.name = name
        self.rect = np.asarray(rect, np.uint32)
        self.by_depth = np.asarray(by_depth, np.uint32)
        self.n = len(self.rect)
        self.tiles_x, self.tiles_y = tiles
        self.nvis = len(self.by_depth) if nvis is None else nvis
        self.div0, self.div1 = div
        j0, j1 = bm.window(self.nvis, *div)
        self.m_cap = max(1, j1 - j0) if m_cap is None else m_cap
        self.H = self.tiles_y * 16 if H is None else H
        self.bin32, self.exact = bin32, exact
        self.rec = None if rec is None else np.asarray(rec, np.float32)
        self.sat = None if sat is None else np.asarray(sat, np.uint8).ravel()
        self.pair_cap = pair_cap
        self.meta = meta

    def model(self):
        return bm.bin_phase(self.rect, self.rec, self.by_depth, self.nvis, self.div0, self.div1, self.m_cap, self.H, self.tiles_x,
                            self.tiles_y, self.bin32, self.exact, self.sat)

    def hook_args(self, pair_cap):
        return dict(tile_rect=self.rect, rec=self.rec, by_depth=self.by_depth, nvis=self.nvis, div0=self.div0, div1=self.div1,
                    m_cap=self.m_cap, H=self.H, tiles_x=self.tiles_x, tiles_y=self.tiles_y, bin32=self.bin32, exact=self.exact,
                    sat=self.sat, pair_cap=pair_cap)

    def lists(self):
        """bytes of `sat`: one per tile, or four per bin"""
        return ((self.tiles_x + 1) // 2) * ((self.tiles_y + 1) // 2) * 4 if self.bin32 else self.tiles_x * self.tiles_y


def in_depth_order(rects, seed, rec=None):
    """rects (and records) given in depth order -> (rect, by_depth, rec) indexed by splat: the splats are a permutation of the
    slots, so that a kernel that mistook a slot for a splat shows"""
    n = len(rects)
    perm = np.random.default_rng(seed).permutation(n).astype(np.uint32)
    rect = np.zeros(n, np.uint32)
    rect[perm] = np.asarray(rects, np.uint32)
    out = None
    if rec is not None:
        out = np.zeros((n, 12), np.float32)
        out[perm] = np.asarray(rec, np.float32)
    return rect, perm, out


def rect_of_area(rng, a, tiles_x, tiles_y):
    """a rectangle of exactly `a` tiles somewhere in the frame (w x h a random factorisation that fits)"""
    if a == 0:
        return EMPTY
    fits = [(w, a // w) for w in range(1, a + 1) if a % w == 0 and w <= tiles_x and a // w <= tiles_y]
    w, h = fits[int(rng.integers(len(fits)))]
    x, y = int(rng.integers(0, tiles_x - w + 1)), int(rng.integers(0, tiles_y - h + 1))
    return bm.pack_rect(x, x + w - 1, y, y + h - 1)


def small_rects(rng, n, tiles_x, tiles_y, empty=0.0, top=6):
    areas = rng.integers(1, top + 1, size=n)
    areas[rng.random(n) < empty] = 0
    return [rect_of_area(rng, int(a), tiles_x, tiles_y) for a in areas]


def one_tile(rng, tiles_x, tiles_y):
    return rect_of_area(rng, 1, tiles_x, tiles_y)


# ---- rounds ---------------------------------------------------------------------------------------------------------------------
def round_cases():
    out = {}
    rng = np.random.default_rng(20271)

    def add(name, rects, tiles=(16, 16), **meta):
        rect, order, _ = in_depth_order(rects, len(out) + 1)
        out[name] = Case(name, rect, order, tiles, **meta)

    for T in WAVE_TOTALS:                                  # one wave whose candidates add up to T, spread over its lanes at random
        areas = rng.multinomial(T, np.full(WAVE, 1.0 / WAVE))
        add(f"wave_total_{T}", [rect_of_area(rng, int(a), 16, 16) for a in areas], wave_total=T)
    for lane in (0, 31, 63):                               # 4096 candidates of one splat: 64 rounds with one owner
        rects = [one_tile(rng, 64, 64) for _ in range(WAVE)]
        rects[lane] = bm.pack_rect(0, 63, 0, 63)
        add(f"big64_lane{lane}", rects, (64, 64), big_lane=lane)
    add("big256", [bm.pack_rect(0, 255, 0, 255)], (256, 256), rounds=1024)
    rects = [one_tile(rng, 16, 16) for _ in range(WAVE)]   # lanes 0..59 one candidate each, lane 60 candidates 60..69: rounds 0 and 1
    rects[60] = bm.pack_rect(3, 7, 9, 10)
    add("straddle_60_70", rects, straddle=(60, 60, 70))
    for lane in (0, 63):
        rects = small_rects(rng, WAVE, 16, 16)
        rects[lane] = EMPTY
        add(f"empty_lane{lane}", rects, empty_lanes=[lane])
    for run in (1, 2, 62):                                 # empty splats share their candidate offset with the next non-empty one
        rects = small_rects(rng, WAVE, 16, 16)
        rects[0] = bm.pack_rect(2, 3, 4, 5)
        rects[1:1 + run] = [EMPTY] * run
        add(f"empty_run_{run}", rects, empty_lanes=list(range(1, 1 + run)))
    for lane in (0, 63):
        rects = [EMPTY] * WAVE
        rects[lane] = bm.pack_rect(5, 7, 1, 3)
        add(f"only_lane{lane}", rects, empty_lanes=[k for k in range(WAVE) if k != lane])
    rects = []
    for w in range(4):                                     # one workgroup: waves empty / full / empty / full
        rects += [EMPTY] * WAVE if w % 2 == 0 else [rect_of_area(rng, 2, 16, 16) for _ in range(WAVE)]
    add("waves_empty_full", rects)
    add("ragged_833", small_rects(rng, 3 * KRB + 65, 16, 16, empty=0.2))
    both = {}
    for name, c in out.items():                            # without sat: the fast path; with an all-zero one: the ballot path
        c.name = name + "/fast"
        both[c.name] = c
        both[name + "/zero_sat"] = Case(name + "/zero_sat", c.rect, c.by_depth, (c.tiles_x, c.tiles_y),
                                        sat=np.zeros(c.tiles_x * c.tiles_y, np.uint8), **c.meta)
    c = out["straddle_60_70"]                               # and the straddling splat losing candidates on both sides of the round's end
    sat = np.zeros((16, 16), np.uint8)
    sat[9, 4], sat[9, 6], sat[10, 3], sat[10, 5] = 1, 0x80, 0xFF, 2
    both["straddle_60_70/sat"] = Case("straddle_60_70/sat", c.rect, c.by_depth, sat=sat, **c.meta)
    return both


# ---- phase windows --------------------------------------------------------------------------------------------------------------
DECOY_RECT = bm.pack_rect(0, 15, 0, 15)


def window_cases():
    """the splats of the window hold small rectangles; every entry of by_depth before the window and at or behind nvis names the
    decoy, a valid splat with all 256 tiles of the frame: a read outside the window shows as 256 pairs too many"""
    out = {}
    for nvis in NVIS:
        n = nvis + 300
        rng = np.random.default_rng(20272 + nvis)
        rect = np.full(n, bm.pack_rect(15, 15, 15, 15), np.uint32)
        rect[:nvis] = small_rects(rng, nvis, 16, 16, empty=0.15, top=4)
        decoy = n - 1
        rect[decoy] = DECOY_RECT
        for div0, div1 in DIVS:
            j0, j1 = bm.window(nvis, div0, div1)
            order = np.full(n, decoy, np.uint32)
            order[j0:max(j0, j1)] = rng.permutation(nvis)[:max(0, j1 - j0)]
            for kind, m_cap in (("fit", max(1, j1 - j0)), ("n", max(1, n // div1))):
                name = f"window_{nvis}_{div0}_{div1}_{kind}"
                out[name] = Case(name, rect, order, nvis=nvis, div=(div0, div1), m_cap=m_cap, window=(j0, j1))
    return out


# ---- rectangles and masks -------------------------------------------------------------------------------------------------------
def rects441():
    return [bm.pack_rect(x0, x1, y0, y1) for y0 in range(6) for y1 in range(y0, 6) for x0 in range(6) for x1 in range(x0, 6)]


def sat_pattern(seed, tiles_x, tiles_y, bin32):
    """per tile a byte of SAT_BYTES (half of them 0); bin32: the same pattern as four bytes per bin, 0 for a tile outside the frame"""
    rng = np.random.default_rng(seed)
    tile = np.where(rng.random((tiles_y, tiles_x)) < 0.5, 0, rng.choice(SAT_BYTES[1:], size=(tiles_y, tiles_x))).astype(np.uint8)
    if not bin32:
        return tile
    bx, by = (tiles_x + 1) // 2, (tiles_y + 1) // 2
    padded = np.zeros((2 * by, 2 * bx), np.uint8)
    padded[:tiles_y, :tiles_x] = tile
    return padded.reshape(by, 2, bx, 2).transpose(0, 2, 1, 3).reshape(by * bx, 4)      # [bin, 2 * (ty & 1) + (tx & 1)]


def rect_cases():
    out = {}
    for tiles_x in (6, 7):                                 # 7: the last column of bins is half outside the frame
        for bin32 in (False, True):
            for with_sat in (False, True):
                name = f"rects441_x{tiles_x}" + ("_bin32" if bin32 else "") + ("_sat" if with_sat else "")
                rect, order, _ = in_depth_order(rects441(), 441 + tiles_x)
                out[name] = Case(name, rect, order, (tiles_x, 6), bin32=bin32,
                                 sat=sat_pattern(20273, tiles_x, 6, bin32) if with_sat else None)
    for bin32 in (False, True):
        name = "corner256" + ("_bin32" if bin32 else "")
        out[name] = Case(name, [bm.pack_rect(254, 255, 254, 255)], [0], (256, 256), bin32=bin32)
        sat = np.zeros((128 * 128, 4) if bin32 else (256, 256), np.uint8)
        sat[-1, -2] = 0x80                                 # tile (254, 255): bit 2 of the last bin
        out[name + "_sat"] = Case(name + "_sat", [bm.pack_rect(254, 255, 254, 255)], [0], (256, 256), bin32=bin32, sat=sat)
    return out


# ---- exact culling --------------------------------------------------------------------------------------------------------------
def record(u, v, g0, g1):
    """a pre-pass record: centre at pixel coordinates (u, v) (image, y down), axes g0, g1 in window coordinates (y up)"""
    return [u, EXACT_H - v, g0[0], g0[1], g1[0], g1[1]] + [0.0] * 6


# name -> (rectangle, record).  Centres at multiples of 1/8, axes small dyadic rationals: the fp32 evaluation is exact or nearly so
EXACT_SPLATS = {
    "diagonal": (bm.pack_rect(0, 7, 0, 7), record(64.125, 61.5, (1 / 64, 1 / 64), (0.5, -0.5))),      # 90 px long, 2.8 px wide
    "axis": (bm.pack_rect(0, 7, 2, 4), record(40.25, 50.125, (1 / 32, 0.0), (0.0, 1.0))),             # 64 px long, 2 px high
    "huge_g": (bm.pack_rect(2, 4, 3, 5), record(56.0, 72.0, (64.0, 0.0), (0.0, 64.0))),               # only the centre's tile (3, 4)
    "one_tile_far": (bm.pack_rect(7, 7, 0, 0), record(8.0, 100.0, (1.0, 0.0), (0.0, 1.0))),           # not tested: kept
    "zero_g": (bm.pack_rect(1, 4, 1, 4), record(30.0, 40.0, (0.0, 0.0), (0.0, 0.0))),                 # q = 0 everywhere
    "den0": (bm.pack_rect(0, 7, 1, 6), record(70.5, 60.25, (0.0, 1 / 8), (0.0, 1 / 4))),              # q does not depend on x
    "nan_g": (bm.pack_rect(2, 5, 2, 5), record(20.0, 20.0, (float("nan"), 0.5), (0.25, 0.0))),
}


def exact_cases():
    out = {}
    rng = np.random.default_rng(20274)

    def fillers(k):
        """one-tile splats (never tested) around the named ones"""
        return [(one_tile(rng, EXACT_TILES, EXACT_TILES), record(rng.integers(0, 128) + 0.5, rng.integers(0, 123) + 0.5, (1.0, 0.0),
                                                                  (0.0, 1.0))) for _ in range(k)]

    def add(name, splats, sat=None):
        rect, order, rec = in_depth_order([s[0] for s in splats], len(out) + 7, [s[1] for s in splats])
        out[name] = Case(name, rect, order, (EXACT_TILES, EXACT_TILES), H=EXACT_H, exact=True, rec=rec, sat=sat)

    for name, splat in EXACT_SPLATS.items():
        f = fillers(5)
        add("exact_" + name, f[:2] + [splat] + f[2:])
    every = fillers(40)
    for k, splat in enumerate(EXACT_SPLATS.values()):
        every.insert(3 + 6 * k, splat)
    add("exact_all", every)
    add("exact_all_sat", every, sat_pattern(20275, EXACT_TILES, EXACT_TILES, False))
    return out


# ---- capacity -------------------------------------------------------------------------------------------------------------------
def capacity_cases():
    out = {}
    for base in ("rects441_x6", "rects441_x6_sat", "rects441_x7_bin32_sat"):
        c = group("rects")[base]
        total = c.model().total
        for kind, cap in (("short_by_one", total - 1), ("exactly", total)):
            name = f"capacity_{kind}_{base}"
            out[name] = Case(name, c.rect, c.by_depth, (c.tiles_x, c.tiles_y), bin32=c.bin32, sat=c.sat, pair_cap=cap, total=total)
    return out


GROUPS = {"rounds": round_cases, "windows": window_cases, "rects": rect_cases, "exact": exact_cases, "capacity": capacity_cases}


@functools.lru_cache(maxsize=None)
def group(name):
    """name -> Case of one group, built once"""
    return GROUPS[name]()


@functools.lru_cache(maxsize=None)
def all_cases():
    """name -> Case, in the order of GROUPS"""
    out = {}
    for g in GROUPS:
        assert not set(group(g)) & set(out)
        out.update(group(g))
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """(case, the model's Binned, pair_cap): computed once per session and left unchanged"""
    c = all_cases()[name]
    b = c.model()
    return c, b, (b.total + 5 if c.pair_cap is None else c.pair_cap)
