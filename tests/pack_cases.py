"""Scenes and expectations for the scene upload (csrc/render_scene.hip: splat_importance_kernel, splat_pack_kernel,
labels_pack_kernel, sh_pack_kernel) and constructed cases for the hit test (hit_partial_kernel, hit_final_kernel), shared by
tests/test_pack_model.py (CPU: the cases against the oracle) and tests/test_pack_gpu.py (the kernels against the same
expectations).  numpy and `oracle` only.

Expectations: buffer and order from oracle.pack_splats, the texture from oracle.texture(buf, labels[order]), the labels
labels[order], the SH planes a numpy gather by order.  Everything is compared byte for byte.

Rule 1 - no NaN importance.  exp(s0) * exp(s1) * exp(s2) overflowing to Infinity while the sigmoid is 0 gives NaN; the
reference's comparator (gs.js:527) then returns NaN and the order is implementation-defined.  Every builder asserts that its
scene has none.

Rule 2 - robust to the last bits of exp.  The device's fp64 exp need not round as the host's does.  Every stored quantity
that goes through exp - the three f32 scales, the f32 importance (it decides the order), the alpha byte - must keep its value
when each exp result moves by +-8 double ulps (`robust_rows`).  The product e0 * e1 * e2 / (1 + eo) is monotone in each exp
result and every fp operation involved is monotone, so the two extreme combinations bound all 3^4.  exp of +-0 and of
+-Infinity is exact by definition (1, 0, Infinity: C Annex F.10.3.1) and is not moved.  A RANDOM row that fails is redrawn, at
most 0.1 % of a scene's random exp arguments (asserted); a hand-PLACED row must pass as written (asserted)."""
import functools

import numpy as np

import oracle

NO_SELECTION = -999999
ULPS = 8
REDRAW_CAP = 0.001
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 70_001]      # a wave, a block, a 4096-key sort tile, several tiles
SH_CASES = [(d, n) for d in range(4) for n in (1, 257, 4097)]
F32_MIN_NORMAL = float(np.finfo(np.float32).tiny)


# ---- rule 2 ----------------------------------------------------------------------------------------------------------------
def _exp_nudged(x32, k):
    """exp of the f32 arguments in fp64, moved by k double ulps (not below 0, not past the largest finite double); exact
    results (argument +-0 or not finite) and overflowed ones stay"""
    x = np.asarray(x32, np.float32).astype(np.float64)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        e = np.exp(x)
    moved = np.clip(e.view(np.int64) + k, 0, 0x7FEFFFFFFFFFFFFF).view(np.float64)
    keep = (x == 0) | ~np.isfinite(x) | ~np.isfinite(e)
    return np.where(keep, e, moved)


def _u8clamp(x):
    """Uint8ClampedArray store: NaN and negatives 0, clamp, round half to even"""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, np.rint(np.minimum(x, 255.0)), 0.0).astype(np.uint8)


def _stored(scale, opacity, k):
    """what the upload stores through exp, with every exp result moved by k ulps in the direction that raises (k > 0) or lowers
    (k < 0) the value: (f32 scales (n,3), f32 importance (n,), alpha byte (n,))"""
    e = _exp_nudged(scale, k)
    eo = _exp_nudged(-np.asarray(opacity, np.float32), -k)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        op = 1.0 / (1.0 + eo)
        imp = (e[:, 0] * e[:, 1] * e[:, 2] * op).astype(np.float32)
        return e.astype(np.float32), imp, _u8clamp(op * 255.0)


def importance(scale, opacity):
    """the f32 importance of gs.js:520-522 as numpy evaluates it (bit-equal to every exp within +-8 ulps on robust rows)"""
    return _stored(scale, opacity, 0)[1]


def robust_rows(scale, opacity):
    """rows whose stored scales, importance and alpha byte are the same for every exp within +-8 double ulps"""
    lo, mid, hi = (_stored(scale, opacity, k) for k in (-ULPS, 0, ULPS))
    ok = np.ones(len(opacity), bool)
    for a, b, c in zip(lo, mid, hi):
        bits = [np.ascontiguousarray(v).view(np.uint32 if v.dtype == np.float32 else np.uint8).reshape(len(ok), -1) for v in (a, b, c)]
        ok &= (bits[0] == bits[1]).all(1) & (bits[1] == bits[2]).all(1)
    return ok


# ---- scenes ----------------------------------------------------------------------------------------------------------------
class Scene:
    """raw attributes (source order) + the builder's bookkeeping; expectations through expect()"""

    def __init__(self, name, xyz, scale, rot, opacity, f_dc, labels, random_values=0, redrawn=0, placed=()):
        self.name = name
        self.xyz, self.scale, self.rot, self.opacity, self.f_dc, self.labels = xyz, scale, rot, opacity, f_dc, labels
        self.n = len(xyz)
        self.random_values, self.redrawn = random_values, redrawn        # exp arguments drawn at random / drawn again
        self.placed = np.asarray(placed, np.int64)                       # hand-placed source rows
        self._expect = None

    def attrs(self):
        return self.xyz, self.scale, self.rot, self.opacity, self.f_dc

    def check_rules(self):
        assert self.redrawn <= REDRAW_CAP * self.random_values, f"{self.name}: {self.redrawn} of {self.random_values} random values redrawn"
        if self.scale is None:
            if self.opacity is not None:                                 # only the alpha byte goes through exp
                zero = np.zeros((self.n, 3), np.float32)
                lo, mid, hi = (_stored(zero, self.opacity, k)[2] for k in (-ULPS, 0, ULPS))
                assert np.array_equal(lo, mid) and np.array_equal(mid, hi), f"{self.name}: an alpha byte changes with the last bits of exp"
            return
        imp = importance(self.scale, self.opacity)
        assert not np.isnan(imp).any(), f"{self.name}: NaN importance at source rows {np.nonzero(np.isnan(imp))[0][:8]}"
        ok = robust_rows(self.scale, self.opacity)
        assert ok.all(), f"{self.name}: source rows {np.nonzero(~ok)[0][:8]} change with the last bits of exp " \
                         f"(placed: {np.intersect1d(np.nonzero(~ok)[0], self.placed)[:8]})"

    def expect(self):
        """(buffer (n,32) u8, order (n,) u32, texture (8n,) u32, labels (n,) i32) - computed once, never modified"""
        if self._expect is None:
            self.check_rules()
            buf, order = oracle.pack_splats(*self.attrs())
            lab = np.full(self.n, NO_SELECTION, np.int32) if self.labels is None else self.labels[order]
            tex = oracle.texture(buf, None if self.labels is None else lab)
            if self.scale is not None:
                imp64 = importance(self.scale, self.opacity).astype(np.float64)
                want = np.argsort(-imp64, kind="stable")
                assert np.array_equal(order, want), f"{self.name}: the oracle's order is not the stable descending order, first at " \
                                                    f"{np.nonzero(order != want)[0][:4]}"
            else:
                assert np.array_equal(order, np.arange(self.n))
            for a in (buf, order, tex, lab):
                a.setflags(write=False)
            self._expect = (buf, order, tex, lab)
        return self._expect


def sh_planes(f_dc, f_rest, order, degree):
    """the layout of sh_pack_kernel: coef[k][c][j], k = 0 the f_dc plane, j the importance-order row"""
    K = (degree + 1) ** 2
    rest = np.asarray(f_rest, np.float32).reshape(len(order), 3, K - 1)[order] if K > 1 else np.zeros((len(order), 3, 0), np.float32)
    return np.ascontiguousarray(np.concatenate([f_dc[order][:, :, None], rest], axis=2).transpose(2, 1, 0))


def random_attributes(n, seed, labels=True):
    """plain random attributes with every row robust (rule 2): -> (attribute dict, redrawn exp arguments)"""
    rng = np.random.default_rng(seed)
    a = dict(xyz=rng.normal(0, 2, (n, 3)).astype(np.float32),
             scale=rng.uniform(-20.0, 2.5, (n, 3)).astype(np.float32),
             rot=rng.normal(0, 1, (n, 4)).astype(np.float32),
             opacity=rng.normal(0, 3, n).astype(np.float32),
             f_dc=rng.normal(0, 1.5, (n, 3)).astype(np.float32),
             labels=rng.integers(-1, 150, n).astype(np.int32) if labels else None)
    redrawn = 0
    for _ in range(8):
        bad = np.nonzero(~robust_rows(a["scale"], a["opacity"]))[0]
        if len(bad) == 0:
            break
        redrawn += 4 * len(bad)
        a["scale"][bad] = rng.uniform(-20.0, 2.5, (len(bad), 3)).astype(np.float32)
        a["opacity"][bad] = rng.normal(0, 3, len(bad)).astype(np.float32)
    return a, redrawn


def tie_run(a, rows):
    """the rows take the (scale, opacity) of the first of them: one importance, everything else still differs"""
    a["scale"][rows] = a["scale"][rows[0]]
    a["opacity"][rows] = a["opacity"][rows[0]]


@functools.lru_cache(maxsize=None)
def size_scene(n):
    """random attributes; a quarter of the rows, scattered over the source, share one importance, and (n >= 64) a few more tie
    at +0 and at +Infinity - the sort must keep each run in source order through every pass and tile"""
    a, redrawn = random_attributes(n, 1000 + n)
    rng = np.random.default_rng(n)
    placed = []
    if n >= 2:
        tie_run(a, np.sort(rng.choice(n, max(2, n // 4), replace=False)))
    if n >= 64:
        rows = rng.choice(n, 10, replace=False)
        a["opacity"][rows[:5]] = -np.inf                                    # importance +0: the largest key
        a["scale"][rows[5:]] = 30.0                                         # e^90 * 0.73 > f32 max: +Infinity, the smallest key
        a["opacity"][rows[5:]] = 1.0
        placed = rows
    return Scene(f"size_{n}", a["xyz"], a["scale"], a["rot"], a["opacity"], a["f_dc"], a["labels"], 4 * n, redrawn, placed)


@functools.lru_cache(maxsize=None)
def value_edge_scene():
    """1025 splats: a random bulk and hand-placed rows at the value edges of the pack.  Placed rows are spread over the source
    at a stride of 3 from row 1, so they sit in different lanes, waves and blocks."""
    n = 1025
    a, redrawn = random_attributes(n, 0xED6E)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    nxt = iter(range(1, n, 3))
    placed, rows = [], {}

    def place(name, scale=None, opacity=None, rot=None, f_dc=None, label=None):
        r = next(nxt)
        placed.append(r)
        rows[name] = r
        for key, v in (("scale", scale), ("opacity", opacity), ("rot", rot), ("f_dc", f_dc), ("labels", label)):
            if v is not None:
                a[key][r] = v
        return r

    # ties: 300 rows of one (scale, opacity) - 300 packed rows in a row cross a 256 boundary wherever they land - and 20 rows of
    # importance exactly 1
    run = np.arange(400, 1000, 2)
    tie_run(a, run)
    ones = np.arange(401, 441, 2)
    a["scale"][ones] = 0.0
    a["opacity"][ones] = inf
    # importance extremes
    for i in range(4):
        place(f"imp_zero_{i}", opacity=-inf)                    # sigmoid 0: +0, a tie at the far end
    place("opacity_-104", opacity=-104.0)
    place("opacity_-800", opacity=-800.0)                       # exp(800) overflows fp64: sigmoid 0 again
    place("imp_e-105", scale=(-35, -35, -35))                   # importance below every f32 subnormal: +0
    place("imp_e-120", scale=(-40, -40, -40))                   # ... likewise
    place("imp_inf_0", scale=(30, 30, 30), opacity=0.5)         # +Infinity with sigmoid > 0
    place("imp_inf_1", scale=(30, 30, 30), opacity=3.0)
    place("imp_-91", scale=(-30, -30, -31))                     # e^-91 * sigmoid: f32-subnormal importance
    # scale stores
    place("scale_-88", scale=(-88, 0, 0))                       # subnormal f32 scale
    place("scale_-100", scale=(0, -100, 0))
    place("scale_-104", scale=(0, 0, -104))                     # below half the smallest subnormal
    place("scale_88.7", scale=(88.7, -3, -3))                   # just below f32 overflow
    place("scale_89", scale=(89, -3, -3))                       # Infinity
    place("sigma_shift_51", scale=(-23, -23, -23))              # 4 * sigma ~ 2^-64: floatToHalf shifts by 51, i.e. 19
    place("sigma_subnormal", scale=(-45, -45, -45))             # 4 * sigma is f32-subnormal: floatToHalf's exp == 0
    place("sigma_shift_36", scale=(-18, -18, -18))              # shift 36, i.e. 4: the half is NOT zero
    place("sigma_shift_mixed", scale=(-17, -19, -18))
    # quaternions
    place("quat_zero", rot=(0, 0, 0, 0))                        # 0 / 0: four 0 bytes
    place("quat_w", rot=(1, 0, 0, 0))
    place("quat_-w", rot=(-1, 0, 0, 0))
    place("quat_tiny", rot=(0, 0, 0, 1e-30))
    place("quat_huge", rot=(3e38, 3e38, 0, 0))
    place("quat_ones", rot=(1, 1, 1, 1))
    place("quat_nan", rot=(0.5, nan, 0.5, 0.5))
    place("quat_inf", rot=(inf, 1, 0, 0))                       # inf / inf and 1 / inf
    # colour and alpha
    place("dc_nonfinite", f_dc=(inf, -inf, nan))
    place("half_way", f_dc=(0, 0, 0), opacity=0.0)              # 127.5 four times: 128
    place("opacity_inf", opacity=inf)
    # labels: beyond +-2^24 the texture word is rounded, labels_out is not
    for lab in (2 ** 24 + 1, 2 ** 24 + 3, -2 ** 24 - 1, INT32_MAX, INT32_MIN, NO_SELECTION):
        place(f"label_{lab}", label=lab)
    placed = np.concatenate([placed, run, ones])
    s = Scene("value_edge", a["xyz"], a["scale"], a["rot"], a["opacity"], a["f_dc"], a["labels"], 4 * n, redrawn, placed)
    s.rows, s.run, s.ones = rows, run, ones                                # where the placed values sit (source rows)
    return s


@functools.lru_cache(maxsize=None)
def fallback_scene(kind):
    """the viewer's fallbacks (gs.js:519, 559-563, 576, 579) at 257 splats"""
    a, redrawn = random_attributes(257, 77)
    if kind == "no_scale":          # identity order, scale 0.01, quaternion bytes 255,0,0,0; opacity still gives alpha
        return Scene(kind, a["xyz"], None, None, a["opacity"], a["f_dc"], a["labels"], 4 * 257, redrawn)
    if kind == "no_scale_no_opacity":
        return Scene(kind, a["xyz"], None, None, None, a["f_dc"], a["labels"])
    assert kind == "no_labels"
    return Scene(kind, a["xyz"], a["scale"], a["rot"], a["opacity"], a["f_dc"], None, 4 * 257, redrawn)


FALLBACKS = ["no_scale", "no_scale_no_opacity", "no_labels"]


@functools.lru_cache(maxsize=None)
def sh_scene(degree, n):
    """f_dc[r, c] and f_rest[r, c * (K - 1) + (k - 1)] hold 64 r + 4 k + c (exact in f32): a transposed or shifted plane cannot
    pass.  Random scales with a tie run, so the order is not the identity."""
    a, redrawn = random_attributes(n, 5000 + 16 * n + degree)
    if n >= 2:
        tie_run(a, np.arange(0, n, 3))
    K = (degree + 1) ** 2
    r, c, k = np.arange(n)[:, None, None], np.arange(3)[None, :, None], np.arange(1, K)[None, None, :]
    a["f_dc"] = (64 * r + c)[:, :, 0].astype(np.float32)                       # k = 0
    f_rest = (64 * r + 4 * k + c).astype(np.float32).reshape(n, 3 * (K - 1))
    s = Scene(f"sh{degree}_{n}", a["xyz"], a["scale"], a["rot"], a["opacity"], a["f_dc"], a["labels"], 4 * n, redrawn)
    s.f_rest, s.degree = f_rest, degree
    return s


def all_pack_scenes():
    """every scene with scales or fallbacks, by name (the SH scenes are separate: sh_scene)"""
    out = {"value_edge": value_edge_scene}
    out.update({f"size_{n}": functools.partial(size_scene, n) for n in SIZES})
    out.update({k: functools.partial(fallback_scene, k) for k in FALLBACKS})
    return out


# ---- where two packs differ ------------------------------------------------------------------------------------------------
BUFFER_FIELDS = [("position", 0, 12), ("scale", 12, 24), ("rgba", 24, 28), ("quaternion", 28, 32)]
TEX_FIELDS = ["position x", "position y", "position z", "label word", "halves 0|1", "halves 2|3", "halves 4|5", "rgba"]


def first_difference(got, want):
    """got, want: (buffer, order, texture, labels).  None if equal, else a sentence naming the first differing packed row, its
    source row and the field"""
    gb, go, gt, gl = got
    wb, wo, wt, wl = want
    if gb.shape != wb.shape or go.shape != wo.shape or gt.shape != wt.shape or gl.shape != wl.shape:
        return f"shapes differ: {gb.shape} {go.shape} {gt.shape} {gl.shape} != {wb.shape} {wo.shape} {wt.shape} {wl.shape}"
    n = len(wo)
    bad = np.nonzero(go != wo)[0]
    if len(bad):
        j = int(bad[0])
        return f"order differs at {len(bad)} packed rows, first {j}: source row {go[j]}, expected {wo[j]}"
    gt, wt = gt.reshape(n, 8), wt.reshape(n, 8)
    rows = (gb != wb).any(1) | (gt != wt).any(1) | (gl != wl)
    if not rows.any():
        return None
    j = int(np.nonzero(rows)[0][0])
    what = []
    for name, lo, hi in BUFFER_FIELDS:
        if (gb[j, lo:hi] != wb[j, lo:hi]).any():
            what.append(f"buffer {name} {gb[j, lo:hi].tobytes().hex()} != {wb[j, lo:hi].tobytes().hex()}")
    for k, name in enumerate(TEX_FIELDS):
        if gt[j, k] != wt[j, k]:
            half = ""
            if 4 <= k <= 6:
                half = " (" + ", ".join(f"half {2 * (k - 4) + h}" for h in (0, 1) if (gt[j, k] ^ wt[j, k]) >> (16 * h) & 0xFFFF) + ")"
            what.append(f"texture {name}{half} {gt[j, k]:#010x} != {wt[j, k]:#010x}")
    if gl[j] != wl[j]:
        what.append(f"label {gl[j]} != {wl[j]}")
    return f"{int(rows.sum())} packed rows differ, first {j} (source row {wo[j]}): " + "; ".join(what)


# ---- floatToHalf, gs.js:248-275, with Python ints -----------------------------------------------------------------------------
def js_float_to_half(bits):
    """bits: the uint32 pattern of the Float32Array store.  JavaScript's >> works on int32 and takes its count mod 32; | 0 is
    where the int32 wraps."""
    f = bits - (1 << 32) if bits & 0x80000000 else bits          # _int32View[0]
    sign = (f >> 31) & 0x0001
    exp = (f >> 23) & 0x00FF
    frac = f & 0x007FFFFF
    if exp == 0:
        new_exp = 0
    elif exp < 113:
        new_exp = 0
        frac |= 0x00800000
        frac = frac >> ((113 - exp) & 31)
        if frac & 0x01000000:
            new_exp = 1
            frac = 0
    elif exp < 142:
        new_exp = exp - 112
    else:
        new_exp = 31
        frac = 0
    return ((sign << 15) | (new_exp << 10) | (frac >> 13)) & 0xFFFFFFFF


def four_sigma(buffer):
    """generateTexture's 4 * sigma (gs.js:322-350) of packed rows in fp64 numpy, as the f32 bit patterns floatToHalf sees: (n, 6)
    uint32.  Same operations in the same order as the JavaScript; numpy never fuses."""
    buffer = np.ascontiguousarray(buffer)
    n = len(buffer)
    sc = buffer[:, 12:24].copy().view(np.float32).astype(np.float64)
    rot = (buffer[:, 28:32].astype(np.float64) - 128.0) / 128.0
    r0, r1, r2, r3 = rot.T
    with np.errstate(all="ignore"):
        M = np.stack([1.0 - 2.0 * (r2 * r2 + r3 * r3), 2.0 * (r1 * r2 + r0 * r3), 2.0 * (r1 * r3 - r0 * r2),
                      2.0 * (r1 * r2 - r0 * r3), 1.0 - 2.0 * (r1 * r1 + r3 * r3), 2.0 * (r2 * r3 + r0 * r1),
                      2.0 * (r1 * r3 + r0 * r2), 2.0 * (r2 * r3 - r0 * r1), 1.0 - 2.0 * (r1 * r1 + r2 * r2)], axis=1)
        M = M * np.repeat(sc, 3, axis=1)
        pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
        sig = np.stack([M[:, a] * M[:, b] + M[:, 3 + a] * M[:, 3 + b] + M[:, 6 + a] * M[:, 6 + b] for a, b in pairs], axis=1)
        return np.ascontiguousarray((4 * sig).astype(np.float32)).view(np.uint32).reshape(n, 6)


# ---- hit test: constructed cases -----------------------------------------------------------------------------------------------
HIT_W, HIT_H = 640, 480
HIT_CAM = {"fx": 500.0, "fy": 500.0, "width": HIT_W, "height": HIT_H, "rotation": [[1, 0, 0], [0, 1, 0], [0, 0, 1]],
           "position": [0.0, 0.0, 0.0]}
CENTRE = (320.0, 240.0)             # where (0, 0, z) projects: (0 / z + 1) * 0.5 * 640, exactly
AWAY = (1000.0, 1000.0, 1.0)        # half a million pixels off the frame
P = (0.0, 0.0, 2.0)
NEAR, FAR = (0.0, 0.0, 2.0), (0.0, 0.0, 3.0)     # both project exactly onto CENTRE; NDC depth grows with z
TRIP = 1024 * 256                   # rows the hit test's grid covers per grid-stride trip


class HitCase:
    """n splats uploaded with scale=None (the order is the identity: a row is its source index), all AWAY except `rows`
    {row: (x, y, z)}; labels[r] = 1000 + r except `labels` {row: label} (labels=None: no labels are uploaded).  `want` is the
    (label, row) the reference's sequential loop returns for a click at `click`, written by hand."""

    def __init__(self, name, n, rows, want, click=CENTRE, labels=()):
        self.name, self.n, self.rows, self.want, self.click, self.labels = name, n, rows, want, click, labels

    def arrays(self):
        xyz = np.tile(np.asarray(AWAY, np.float32), (self.n, 1))
        for r, p in self.rows.items():
            xyz[r] = p
        labels = None
        if self.labels is not None:
            labels = (1000 + np.arange(self.n)).astype(np.int32)
            for r, v in dict(self.labels).items():
                labels[r] = v
        return xyz, np.zeros((self.n, 3), np.float32), labels


def _hit_cases():
    c = []
    add = lambda *a, **k: c.append(HitCase(*a, **k))
    last = 256 * 1023 + 3
    # full tie (same position: same distance, same depth): the lowest row wins; then the low row is moved away
    add("tie_lanes", 256, {3: P, 40: P, 63: P}, (1003, 3))
    add("tie_lanes_moved", 256, {40: P, 63: P}, (1040, 40))
    add("tie_waves", 256, {0: P, 64: P, 128: P, 192: P}, (1000, 0))
    add("tie_waves_moved", 256, {64: P, 128: P, 192: P}, (1064, 64))
    add("tie_waves_moved_twice", 256, {128: P, 192: P}, (1128, 128))
    add("tie_waves_5_69", 256, {5: P, 69: P}, (1005, 5))
    add("tie_waves_69", 256, {69: P}, (1069, 69))
    add("tie_blocks", TRIP, {10: P, 266: P, last: P}, (1010, 10))
    add("tie_blocks_moved", TRIP, {266: P, last: P}, (1266, 266))
    add("tie_blocks_moved_twice", TRIP, {last: P}, (1000 + last, last))
    add("tie_trips", TRIP + 300, {7: P, 7 + TRIP: P}, (1007, 7))
    add("tie_trips_moved", TRIP + 300, {7 + TRIP: P}, (1000 + 262151, 262151))
    add("tie_trips_last", TRIP + 300, {299: P, 299 + TRIP: P}, (1299, 299))
    add("tie_trips_last_moved", TRIP + 300, {299 + TRIP: P}, (1000 + 262443, 262443))
    add("tie_trips_blocks", TRIP + 300, {300: P, 100 + TRIP: P}, (1300, 300))      # second trip of block 0 against block 1
    # equal distance, different depth: the nearer wins, also at the higher row
    add("depth_lanes", 256, {3: FAR, 40: NEAR}, (1040, 40))
    add("depth_waves", 256, {5: FAR, 69: NEAR}, (1069, 69))
    add("depth_blocks", 1024, {10: FAR, 266: NEAR, 700: FAR}, (1266, 266))
    add("depth_off_centre", 1024, {10: FAR, 266: NEAR}, (1266, 266), click=(323.0, 244.0))      # both exactly 5 px away
    # a smaller distance beats a nearer depth: row 0 lies 1 px off and nearer, row 300 on the click and deeper
    add("distance_first", 512, {0: (0.004, 0.0, 2.0), 300: (0.0, 0.0, 5.0)}, (1300, 300))
    # threshold, gs.js:387: dist < 10
    add("threshold_10", 1, {0: P}, (NO_SELECTION, -1), click=(330.0, 240.0))
    add("threshold_9.999", 1, {0: P}, (1000, 0), click=(329.999, 240.0))
    add("threshold_10_y", 1, {0: P}, (NO_SELECTION, -1), click=(320.0, 230.0))
    # clip, gs.js:402: w <= 0 is skipped; z < 0 mirrors onto the click; a NaN or Inf coordinate gives a NaN distance
    add("clip", 8, {0: (0.0, 0.0, 0.0), 1: (0.0, 0.0, -2.0), 2: (np.nan, 0.0, 2.0), 3: (np.inf, 0.0, 2.0), 4: (0.0, -np.inf, 2.0),
                    5: (0.0, np.nan, 2.0), 7: FAR}, (1007, 7))
    add("clip_nothing_left", 8, {0: (0.0, 0.0, 0.0), 1: (0.0, 0.0, -2.0), 2: (np.nan, 0.0, 2.0), 3: (np.inf, 0.0, 2.0)}, (NO_SELECTION, -1))
    # sizes: the winner in the last row
    for n in (1, 255, 256, 257):
        add(f"last_row_{n}", n, {n - 1: P}, (1000 + n - 1, n - 1))
    # labels: the call returns the exact int32, not the texture's fp32 copy (2^24 + 1 rounds to 2^24)
    add("label_2^24+1", 300, {299: P}, (16777217, 299), labels={299: 2 ** 24 + 1})
    add("label_-2^24-1", 300, {299: P}, (-16777217, 299), labels={299: -2 ** 24 - 1})
    add("label_int32_max", 300, {299: P}, (2147483647, 299), labels={299: INT32_MAX})
    add("label_int32_min", 300, {299: P}, (-2147483648, 299), labels={299: INT32_MIN})
    add("label_no_selection", 300, {299: P}, (-999999, 299), labels={299: NO_SELECTION})
    add("label_none", 300, {299: P}, (-999999, 299), labels=None)
    return c


HIT_CASES = _hit_cases()


@functools.lru_cache(maxsize=None)
def hit_order_scene():
    """a scene WITH scales (the order is not the identity) in front of HIT_CAM: a 300-row tie run whose rows share positions in
    pairs, so that which of two coincident splats is picked depends on the stable order; labels beyond 2^24, all odd"""
    n = 600
    a, redrawn = random_attributes(n, 0x417)
    rng = np.random.default_rng(0x418)
    a["xyz"] = np.stack([rng.uniform(-1, 1, n), rng.uniform(-0.8, 0.8, n), rng.uniform(2, 6, n)], axis=1).astype(np.float32)
    run = np.arange(100, 400)
    tie_run(a, run)
    a["xyz"][run[1::2]] = a["xyz"][run[0::2]]
    a["labels"] = (2 ** 24 + 1 + 2 * rng.permutation(n)).astype(np.int32)
    s = Scene("hit_order", a["xyz"], a["scale"], a["rot"], a["opacity"], a["f_dc"], a["labels"], 4 * n, redrawn, run)
    p = a["xyz"][run[0::6]].astype(np.float64)
    s.clicks = [(float(320.0 + 500.0 * x / z), float(240.0 - 500.0 * y / z)) for x, y, z in p] + [(1.0, 1.0)]
    return s
