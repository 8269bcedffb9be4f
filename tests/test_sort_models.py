"""CPU: the numpy models of tests/sort_cases.py that tests/test_sort_gpu.py holds the sort, scan, ranges and Morton kernels to
are themselves checked against the plainest form of each operation, and are quick enough for a test to compute."""
import time

import numpy as np
import pytest

import sort_cases as sc


def test_bit_interleave_against_a_per_bit_loop():
    rng = np.random.default_rng(1)
    q = rng.integers(0, 1 << 21, size=(300, 3), dtype=np.uint64)
    q[:4] = [[0, 0, 0], [0x1FFFFF] * 3, [0x1FFFFF, 0, 0], [0, 0, 0x100000]]
    got = sc.spread21(q[:, 0]) | (sc.spread21(q[:, 1]) << np.uint64(1)) | (sc.spread21(q[:, 2]) << np.uint64(2))
    for row, code in zip(q.tolist(), got.tolist()):
        want = 0
        for b in range(21):
            for a in range(3):
                want |= ((row[a] >> b) & 1) << (3 * b + a)
        assert code == want and code < 1 << 63


@pytest.mark.parametrize("name", sorted(sc.MORTON_SCENES))
def test_morton_model_is_a_stable_order_of_its_codes(name):
    for n in sc.MORTON_SIZES[:3]:
        xyz = sc.MORTON_SCENES[name](n, 5)
        assert xyz.dtype == np.float32 and xyz.shape == (n, 3)
        perm = sc.morton_model(xyz).astype(np.int64)
        code = sc.morton_codes(xyz)
        assert np.array_equal(np.sort(perm), np.arange(n))
        c = code[perm]
        assert (c[1:] >= c[:-1]).all()
        ties = c[1:] == c[:-1]
        assert (perm[1:][ties] > perm[:-1][ties]).all()        # equal codes keep the index order
    # the scenes are what their names say
    if name == "identical":
        assert np.array_equal(perm, np.arange(n))
    if name in ("flat_axis", "dead_axis"):
        axis = 1 if name == "flat_axis" else 2
        assert not (code & (np.uint64(0x1249249249249249) << np.uint64(axis))).any() and len(np.unique(code)) > n // 2
    if name == "non_finite":
        bad = ~np.isfinite(xyz)
        assert bad.all(axis=1).sum() >= 1 and (bad.sum(axis=1) == 1).sum() >= 3
        assert code[bad.all(axis=1)].max() == 0                  # an all-NaN point sorts first
    if name == "huge":
        assert np.isfinite(xyz).all() and np.abs(xyz).min() > 2.5e38 and np.abs(xyz).max() > 3.0e38 and len(np.unique(code)) > n // 2
    if name == "duplicates":
        assert len(np.unique(code)) <= n // 50
    if name == "floaters":
        far = np.abs(xyz).max(axis=1) > 100
        assert far.sum() == 10 and len(np.unique(code[~far])) > n // 2     # 21 bits per axis still tell the cluster's points apart


def test_morton_quantisation_reaches_both_ends():
    xyz = np.array([[0, 0, 0], [1, 2, 4], [0.5, 1, 2], [1, 0, 4]], np.float32)
    code = sc.morton_codes(xyz)
    assert code[0] == 0 and code[1] == (1 << 63) - 1
    half = 1048575                                              # trunc(0.5 * 2097151)
    assert int(code[2]) == int(sc.spread21(np.uint64(half))) * 7
    assert np.array_equal(sc.morton_model(xyz), [0, 2, 3, 1])


def test_ranges_of_against_a_dictionary_count():
    rng = np.random.default_rng(2)
    for nranges, n in ((1, 50), (7, 0), (40, 300), (2048, 5000), (2040, 100)):
        keys = np.sort(rng.integers(0, nranges + 3, size=n, dtype=np.uint64).astype(np.uint32))
        count = {}
        for k in keys.tolist():
            count[k] = count.get(k, 0) + 1
        start, want, want0 = 0, np.zeros((nranges, 2), np.int32), np.zeros((nranges, 2), np.int32)
        for d in range(nranges):
            c = count.get(d, 0)
            want[d] = (start, start + c)
            if c:
                want0[d] = (start, start + c)
            start += c
        assert np.array_equal(sc.ranges_of(keys, nranges), want)
        assert np.array_equal(sc.ranges_of(keys, nranges, empty_zero=True), want0)


def test_stable_order_ignores_the_bits_above():
    keys = np.array([0x80000001, 0x00000101, 0x00000001, 0xFFFFFF00, 0x00000000], np.uint32)
    assert np.array_equal(sc.stable_order(keys, 8), [3, 4, 0, 1, 2])
    assert np.array_equal(sc.stable_order(keys, 1), [3, 4, 0, 1, 2])
    assert np.array_equal(sc.stable_order(keys, 9), [4, 0, 2, 3, 1])
    assert np.array_equal(sc.stable_order(keys, 32), [4, 2, 1, 0, 3])
    assert np.array_equal(sc.garbage_above(keys, 8, 3) & np.uint32(0xFF), keys & np.uint32(0xFF))
    assert np.array_equal(sc.garbage_above(keys, 32, 3), keys)


@pytest.mark.parametrize("bits", [8, 11, 32])
def test_distributions_are_what_their_names_say(bits):
    n = sc.DIST_N
    width = {8: 8, 11: 6, 32: 8}[bits]                          # the first pass's digit width (radix_sort_pairs_drop)
    digit = lambda k: k & np.uint32((1 << width) - 1)
    k = {name: sc.dist_keys(name, n, bits) for name in sc.DISTRIBUTIONS}
    assert len(np.unique(k["all_equal"])) == 1
    r = digit(k["digit_per_round"])[:n // 64 * 64].reshape(-1, 64)
    assert (r == r[:, :1]).all() and (r[1:, 0] != r[:-1, 0]).all()
    t = digit(k["digit_per_tile"])
    assert all(len(np.unique(t[i:i + sc.TILE])) == 1 for i in range(0, n, sc.TILE)) and len(np.unique(t)) == 4
    assert (np.diff(k["ascending"].astype(np.int64)) >= 0).all() and (np.diff(k["descending"].astype(np.int64)) <= 0).all()
    a = digit(k["alternating"])
    assert len(np.unique(a)) == 2 and (a[::2] == a[0]).all() and (a[1::2] == a[1]).all()
    assert len(np.unique(k["bit31"])) == 2 and len(np.unique(k["bit31"] & np.uint32(0x7FFFFFFF))) == 1
    assert np.array_equal(sc.stable_order(k["above_bits"], bits), np.arange(n))
    assert (bits == 32) == (len(np.unique(k["above_bits"])) == 1)
    share = (digit(k["skew"]) == 0).mean()
    assert 0.87 < share < 0.93
    for kind, kept in (("none", n), ("all_but_one", 1), ("first_rounds", n - 13 * 64), ("only_last", 1)):
        assert (~sc.drop_marks(kind, n, 1)).sum() == kept
    assert 0.45 < sc.drop_marks("half", n, 1).mean() < 0.55 and not sc.drop_marks("only_last", n, 1)[-1]
    m = sc.drop_marks("first_rounds", n, 1)
    assert m[:64].all() and not m[64:1024].any() and m[1024:1088].all()


def test_models_are_quick_enough_for_a_test():
    """every expected array of tests/test_sort_gpu.py comes from here: the largest of each kind must cost a few seconds at most"""
    t0 = time.perf_counter()
    keys = sc.random_keys(sc.THREE_ROUNDS, 1)
    order = sc.stable_order(keys, 8)
    t1 = time.perf_counter()
    assert len(order) == sc.THREE_ROUNDS and t1 - t0 < 5.0
    sc.ranges_of((keys[order] & np.uint32(0x7FF))[np.argsort(keys[order] & np.uint32(0x7FF), kind="stable")], 2048)
    t2 = time.perf_counter()
    assert t2 - t1 < 5.0
    perm = sc.morton_model(sc.MORTON_SCENES["cube"](sc.MORTON_SIZES[-1], 1))
    t3 = time.perf_counter()
    assert len(perm) == sc.MORTON_SIZES[-1] and t3 - t2 < 5.0
    for name in sc.DISTRIBUTIONS:
        sc.stable_order(sc.dist_keys(name, sc.DIST_N, 32), 32)
    assert time.perf_counter() - t3 < 5.0
