"""Keys, scenes and numpy models shared by tests/test_sort_gpu.py and tests/test_sort_models.py: the radix sorts of
csrc/sort.hip, the scan and the ranges of csrc/render.hip and the Morton order of the positions.  Plain numpy, integer
work: every comparison built on these is exact."""
import numpy as np

ROUND = 64                                  # keys a wave ranks per ballot round
WAVE_CHUNK = 1024                           # consecutive keys of one wave (16 rounds)
TILE = 4096                                 # keys per workgroup (kSortTile); also the scan's tile (kScanTile)
SCAN_ROUND = 256                            # tiles radix_rowscan_kernel scans per round / workgroups scan_down_kernel re-adds per stride
DROP_KEY = 0xFFFFFFFF                       # radix_sort_pairs_drop leaves these out

RAGGED = TILE + WAVE_CHUNK + 65             # a ragged tile, a ragged wave and a ragged round behind one full tile
DIST_N = 3 * TILE + 777
SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193]
TWO_ROUNDS = [SCAN_ROUND * TILE - 1, SCAN_ROUND * TILE, SCAN_ROUND * TILE + 1]     # 255.99.., 256 and 257 tiles
THREE_ROUNDS = 2 * SCAN_ROUND * TILE + 1


def random_keys(n, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)


def garbage_above(keys, bits, seed):
    """the same keys with random bits at [bits, 32): they must never take part"""
    if bits >= 32:
        return keys.copy()
    junk = random_keys(len(keys), seed) & np.uint32((0xFFFFFFFF << bits) & 0xFFFFFFFF)
    return (keys & np.uint32((1 << bits) - 1)) | junk


# ---- key distributions: name -> f(n, bits, seed) ------------------------------------------------------------------------------
def _all_equal(n, bits, seed):
    return np.full(n, 0x9E3779B1, np.uint32)


def _digit_per_round(n, bits, seed):
    """the 64 keys of a wave round share one key: `peers` is all ones, the rank is popcount(lt), lane 63's counts 63"""
    r = (np.arange(n, dtype=np.uint64) // ROUND) % 251
    return (r * 0x01010101 & 0xFFFFFFFF).astype(np.uint32)


def _digit_per_tile(n, bits, seed):
    """one key per 4096-key tile, another in every tile (an odd multiplier keeps the low digits distinct): every histogram row
    has a single non-zero"""
    t = np.arange(n, dtype=np.uint64) // TILE + 1
    return (t * 0x9E3779B1 & 0xFFFFFFFF).astype(np.uint32)


def _ascending(n, bits, seed):
    return np.sort(random_keys(n, seed))


def _descending(n, bits, seed):
    return np.sort(random_keys(n, seed))[::-1].copy()


def _alternating(n, bits, seed):
    """two digits alternating by lane: peers = 0x5555.. / 0xaaaa.., in every pass"""
    return np.where(np.arange(n) & 1, np.uint32(0xAAAAAAAA), np.uint32(0x55555555)).astype(np.uint32)


def _bit31(n, bits, seed):
    top = np.random.default_rng(seed).integers(0, 2, size=n, dtype=np.uint64) << np.uint64(31)
    return (top | np.uint64(0x12345)).astype(np.uint32)


def _above_bits(n, bits, seed):
    """keys that differ only in bits >= `bits`: the expected order is the identity (at 32 bits: all equal)"""
    return garbage_above(np.full(n, 0x2D, np.uint32), bits, seed)


def _skew(n, bits, seed):
    """geometric: about 90 % of the keys hold digit 0 of the first pass, 9 % digit 1, ...; the higher bits are random"""
    rng = np.random.default_rng(seed)
    g = np.minimum(rng.geometric(0.9, size=n) - 1, 15).astype(np.uint32)
    return (random_keys(n, seed + 1) & np.uint32(0xFFFFFF00)) | g


DISTRIBUTIONS = {"all_equal": _all_equal, "digit_per_round": _digit_per_round, "digit_per_tile": _digit_per_tile,
                 "ascending": _ascending, "descending": _descending, "alternating": _alternating, "bit31": _bit31,
                 "above_bits": _above_bits, "skew": _skew}
WIDE_DISTRIBUTIONS = ["all_equal", "digit_per_tile", "ascending", "skew"]


def dist_keys(name, n, bits, seed=0):
    keys = DISTRIBUTIONS[name](n, bits, seed + 7919 * bits)
    assert keys.dtype == np.uint32 and keys.shape == (n,)
    return keys


def drop_marks(kind, n, seed):
    """which pairs radix_sort_pairs_drop is told to leave out"""
    i = np.arange(n)
    if kind == "none":
        return np.zeros(n, bool)
    if kind == "half":
        return np.random.default_rng(seed).random(n) < 0.5
    if kind == "all_but_one":
        m = np.ones(n, bool)
        m[(seed * 2654435761 + 12345) % n] = False
        return m
    if kind == "first_rounds":              # exactly every wave's first round of 64
        return i % WAVE_CHUNK < ROUND
    if kind == "only_last":                 # the only kept pair is the last element (of a ragged last tile)
        return i != n - 1
    raise KeyError(kind)


# ---- models ---------------------------------------------------------------------------------------------------------------------
def key_mask(bits):
    return np.uint32(0xFFFFFFFF) if bits >= 32 else np.uint32((1 << bits) - 1)


def stable_order(keys, bits):
    """the order a stable sort by key bits [0, bits) leaves"""
    return np.argsort(np.asarray(keys, np.uint32) & key_mask(bits), kind="stable")


def ranges_of(sorted_keys, nranges, empty_zero=False):
    """(nranges, 2) int32: [first, last + 1) slot of every key d < nranges in the ascending `sorted_keys`.  An absent key's range
    is empty AT its place (what radix_sort_values_wide writes: the digit's base twice), or (0, 0) with empty_zero (what
    ranges_kernel leaves of the zeroed table)."""
    k = np.asarray(sorted_keys, np.uint32)
    d = np.arange(nranges, dtype=np.uint32)
    out = np.stack([np.searchsorted(k, d, "left"), np.searchsorted(k, d, "right")], 1).astype(np.int32)
    if empty_zero:
        out[out[:, 0] == out[:, 1]] = 0
    return out


def effective_count(count, capacity):
    """actual_count of sort.hip / ranges_kernel: a device-side count above the capacity reads as 0"""
    return 0 if count > capacity else count


def spread21(v):
    """21 bits -> every third bit of a 63-bit word (uint64 arrays)"""
    v = np.asarray(v, np.uint64) & np.uint64(0x1FFFFF)
    for s, m in ((32, 0x1F00000000FFFF), (16, 0x1F0000FF0000FF), (8, 0x100F00F00F00F00F), (4, 0x10C30C30C30C30C3),
                 (2, 0x1249249249249249)):
        v = (v | (v << np.uint64(s))) & np.uint64(m)
    return v


def morton_codes(xyz):
    """bbox_partial_kernel / bbox_final_kernel / morton_kernel restated: the 63-bit code of every position (uint64)"""
    xyz = np.asarray(xyz, np.float32)
    n = len(xyz)
    code = np.zeros(n, np.uint64)
    with np.errstate(all="ignore"):
        for a in range(3):
            v = xyz[:, a]
            fin = v[np.isfinite(v)]
            lo = np.float32(3.0e38) if len(fin) == 0 else min(np.float32(3.0e38), fin.min())
            hi = np.float32(-3.0e38) if len(fin) == 0 else max(np.float32(-3.0e38), fin.max())
            ext = np.float64(hi) - np.float64(lo)
            if ext > 0.0:
                t = (v.astype(np.float64) - np.float64(lo)) / ext * 2097151.0
                t = np.where(np.isfinite(t), np.minimum(np.maximum(t, 0.0), 2097151.0), 0.0)   # non-finite positions sort first
            else:
                t = np.zeros(n, np.float64)
            code |= spread21(t.astype(np.uint64)) << np.uint64(a)
    return code


def morton_model(xyz):
    """perm[i] = index of the position in slot i of the Morton order: the stable order of the 63-bit codes (the library sorts by
    the low 32 bits, then stably by the high 31)"""
    return np.argsort(morton_codes(xyz), kind="stable").astype(np.uint32)


# ---- Morton scenes: name -> f(n, seed) -> (n, 3) float32 ---------------------------------------------------------------------
MORTON_SIZES = [2, 65, 4097, 300_001]


def _cube(n, seed):
    return np.random.default_rng(seed).uniform(-4.0, 4.0, size=(n, 3)).astype(np.float32)


def _identical(n, seed):
    return np.tile(np.array([[0.5, -1.25, 2.0]], np.float32), (n, 1))


def _flat_axis(n, seed):
    p = _cube(n, seed)
    p[:, 1] = 0.75                          # ext == 0 on y
    return p


def _floaters(n, seed):
    """a dense cluster (radius ~0.1) with up to ten floaters at 1e4 radii: the cluster's cells differ only in low code bits"""
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal((n, 3)) * 0.03).astype(np.float32)
    m = min(10, n // 2)
    at = rng.choice(n, size=m, replace=False)
    d = rng.standard_normal((m, 3))
    p[at] = (d / np.linalg.norm(d, axis=1, keepdims=True) * 1.0e3).astype(np.float32)
    return p


def _non_finite(n, seed):
    """NaN, +inf, -inf in single coordinates of a few points, and one point that is all NaN"""
    rng = np.random.default_rng(seed)
    p = _cube(n, seed)
    bad = [np.nan, np.inf, -np.inf]
    for j in range(min(n - 1, 9)):
        p[rng.integers(n), j % 3] = bad[(j // 3) % 3]
    p[rng.integers(n)] = np.nan
    return p


def _dead_axis(n, seed):
    p = _cube(n, seed)
    p[:, 2] = np.where(np.arange(n) % 3 == 0, np.nan, np.where(np.arange(n) % 3 == 1, np.inf, -np.inf))
    return p


def _huge(n, seed):
    """coordinates near +-3e38, on both sides of the 3.0e38 the box starts from; ext is finite only in float64"""
    rng = np.random.default_rng(seed)
    p = (rng.uniform(2.6e38, 3.39e38, size=(n, 3)) * rng.choice([-1.0, 1.0], size=(n, 3))).astype(np.float32)
    p[:, 2] = np.abs(p[:, 2])               # one axis on one side only: lo stays at most 3.0e38
    return p


def _duplicates(n, seed):
    rng = np.random.default_rng(seed)
    sites = _cube(max(1, n // 50), seed)
    return sites[rng.integers(len(sites), size=n)]


MORTON_SCENES = {"cube": _cube, "identical": _identical, "flat_axis": _flat_axis, "floaters": _floaters,
                 "non_finite": _non_finite, "dead_axis": _dead_axis, "huge": _huge, "duplicates": _duplicates}
