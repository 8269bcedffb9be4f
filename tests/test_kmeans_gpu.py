"""k-means labeler (csrc/kmeans.hip, gsx_kmeans) against the vectors of the reference itself (tests/golden/kmeans.npz)
and against the oracle (oracle/kmeans_oracle.py) on larger inputs and at the structural edges of the two kernels: labels
equal, float32 centroids equal bit for bit (the sign of a zero included), iteration count and converged flag equal.
No tolerance appears anywhere in this file."""
import functools
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import kmeans_cases as kc
from kmeans_cases import same_bits
from oracle import kmeans_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "kmeans.npz")


def golden_cases():
    z = np.load(GOLD)
    names = sorted({k.split("/")[0] for k in z.files})
    return [(n, {k.split("/")[1]: z[k] for k in z.files if k.startswith(n + "/")}) for n in names]


@pytest.fixture(scope="module")
def gsx():
    return importlib.import_module("3d_gaussian_splatting_project_amd.labeler")


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c[0])
def test_kmeans_matches_reference_golden(gsx, case):
    name, g = case
    with gsx.Context(0) as c:
        cent, labels, iters, conv = c.kmeans(g["points"], g["colors"], int(g["k"]), g["init"], max_iter=int(g["max_iter"]))
    assert np.array_equal(labels, g["labels"]), name
    assert same_bits(cent, g["centroids"]), name
    assert conv == bool(g["converged"])


def test_kmeans_large_vs_oracle(gsx):
    """300 k rows, k = 10 and k = 37 (more than one KD-tree leaf in the reference), CLI iteration count; also k = 1,
    an empty cluster (a far-away initial centroid that loses all its members) and max_iter = 0."""
    rng = np.random.default_rng(4)
    n = 300_000
    centres = rng.normal(size=(12, 6)) * np.array([5, 5, 5, 1, 1, 1])
    data = (centres[rng.integers(0, 12, size=n)] + rng.normal(size=(n, 6)) * np.array([0.8, 0.8, 0.8, 0.3, 0.3, 0.3])).astype(np.float32)
    pts, col = np.ascontiguousarray(data[:, :3]), np.ascontiguousarray(data[:, 3:])
    with gsx.Context(0) as c:
        for k, iters in ((10, 10), (37, 4), (1, 3)):
            init = rng.choice(n, k, replace=False)
            want_c, want_l, want_it, want_conv = kmeans_oracle.k_means_with_color(pts, k, col, init, max_iter=iters)
            cent, labels, it, conv = c.kmeans(pts, col, k, init, max_iter=iters)
            assert np.array_equal(labels, want_l) and same_bits(cent, want_c) and (it, conv) == (want_it, want_conv), k
        # empty cluster: row 0 is moved far away and used as a centroid; after one update it has only itself ... make it lose
        # even that by duplicating a second centroid closer to it
        far, farc = pts.copy(), col.copy()
        far[0] = [1e4, 1e4, 1e4]
        far[1] = [1e4, 1e4, 1e4]
        farc[1] = farc[0]
        init = np.array([0, 1, 5, 9], np.int64)                     # centroids 0 and 1 coincide: 1 never wins the first-minimum rule
        want = kmeans_oracle.k_means_with_color(far, 4, farc, init, max_iter=5)
        got = c.kmeans(far, farc, 4, init, max_iter=5)
        assert np.array_equal(got[1], want[1]) and same_bits(got[0], want[0]) and (got[1] != 1).all()
        want0 = kmeans_oracle.k_means_with_color(pts, 6, col, init=np.arange(6), max_iter=0)
        got0 = c.kmeans(pts, col, 6, np.arange(6), max_iter=0)
        assert np.array_equal(got0[1], want0[1]) and got0[2] == 0
        with pytest.raises(ValueError):
            c.kmeans(pts[:5], col[:5], 6, np.arange(6))             # k > n
        with pytest.raises(ValueError):
            c.kmeans(pts, col, 3, np.array([0, 1, n]))              # index out of range


def test_kmeans_cli_writes_labelled_ascii_ply(tmp_path, gsx):
    g = dict(golden_cases())["blobs_k10"]
    ply_io = importlib.import_module("3d_gaussian_splatting_project_amd.ply_io")
    src = tmp_path / "in.ply"
    cols = {"x": g["points"][:, 0], "y": g["points"][:, 1], "z": g["points"][:, 2], "f_dc_0": g["colors"][:, 0],
            "f_dc_1": g["colors"][:, 1], "f_dc_2": g["colors"][:, 2], "opacity": np.zeros(len(g["points"]), np.float32)}
    ply_io.write_vertex_ply(str(src), cols)
    out = tmp_path / "out.ply"
    init = ",".join(str(int(v)) for v in g["init"])
    subprocess.check_call([sys.executable, os.path.join(ROOT, "3D_clustering", "k_means.py"), "--file_path", str(src),
                           "--save_path", str(out), "--k", str(int(g["k"])), "--init", init], stdout=subprocess.DEVNULL)
    head = out.read_bytes()[:400].decode("ascii", "replace")
    assert "format ascii 1.0" in head and "property int label" in head
    back = ply_io.PlyData.read(str(out))
    assert np.array_equal(np.asarray(back["vertex"]["label"]).astype(np.int64), g["labels"])   # the CLI's max_iter is 10
    assert np.array_equal(np.asarray(back["vertex"]["opacity"]), cols["opacity"])


# ---- the two kernels at their structural edges ---------------------------------------------------------------------------------
def agrees(got, want, what=""):
    """(centroids, labels, iterations, converged) of Context.kmeans against the oracle's: everything, exactly"""
    assert np.array_equal(got[1], want[1]), f"{what}: {int((got[1] != want[1]).sum())} labels differ"
    assert same_bits(got[0], want[0]), f"{what}: centroid bits differ in rows {np.unique(np.nonzero(got[0].view(np.uint32) != want[0].view(np.uint32))[0])[:8]}"
    assert (got[2], got[3]) == (want[2], want[3]), f"{what}: (iterations, converged) {got[2:]} != {want[2:]}"


@pytest.mark.parametrize("name,sizes", [("small", kc.SMALL_SIZES), ("stage", kc.STAGE_SIZES)])
def test_kmeans_sum_exact_cluster_sizes(gsx, name, sizes):
    """kmeans_sum_kernel at every residue of its head, 16-wide block and tail loops, on both sides of one, two and five
    stages of 1920 rows: clusters of exactly these member counts, members scattered through the index space, data whose
    float32 sum depends on the order (asserted: for every cluster of >= 16 members the sum in index order differs from the sum
    in reverse order and from the rounded float64 sum, so a kernel that adds in another order or wider cannot pass)."""
    data, members, init = kc.sized_scene(sizes, seed=0)
    assert [len(m) for m in members] == sizes and kc.order_sensitive(data, members) == []
    truth = np.empty(len(data), np.int64)
    for c, rows in enumerate(members):
        truth[rows] = c
    pts, col = kc.split(data)
    with gsx.Context(0) as c:
        for max_iter in (1, 3):
            want = kmeans_oracle.k_means_with_color(pts, len(sizes), col, init, max_iter=max_iter)
            assert np.array_equal(want[1], truth), "the scene must keep its member counts"     # CPU, before the GPU is asked
            for j, rows in enumerate(members):                                                # ... and the oracle's mean IS that sum
                assert same_bits(want[0][j], np.add.reduce(data[rows], axis=0, dtype=np.float32) / np.float32(len(rows)))
            agrees(c.kmeans(pts, col, len(sizes), init, max_iter=max_iter), want, f"{name}, max_iter {max_iter}")


EDGE_N = 50_001                 # 195 full workgroups of 256 and one of 81


@functools.lru_cache(maxsize=None)
def edge_case(k):
    """blob rows, k random initial rows, two iterations, and what the oracle makes of them (computed once per k)"""
    data = kc.blobs(EDGE_N, seed=21)
    pts, col = kc.split(data)
    init = np.random.default_rng(1000 + k).choice(EDGE_N, k, replace=False)
    return pts, col, init, kmeans_oracle.k_means_with_color(pts, k, col, init, max_iter=2)


@pytest.mark.parametrize("k", [1, 2, 3, 255, 256, 257, 1260, 1261, 2047, 2048])
def test_kmeans_k_at_its_edges(gsx, k):
    """k = 1..3; 255..257: the label sort goes from 8 bits in one radix pass to 9 bits in two, and the order lands in the other
    buffer; 1260 / 1261: the assign kernel's 52 k bytes of dynamic LDS cross 64 KB and need the raised limit; 2047 / 2048: the
    maximum, 104 KB, eight LDS counters per thread."""
    pts, col, init, want = edge_case(k)
    with gsx.Context(0) as c:
        agrees(c.kmeans(pts, col, k, init, max_iter=2), want, f"k {k}")


@pytest.mark.parametrize("n", [5, 2048])
def test_kmeans_every_row_a_centroid(gsx, n):
    """n == k: distinct rows, every row an initial centroid (in shuffled order), so every cluster has exactly one member."""
    rng = np.random.default_rng(n)
    data = rng.normal(size=(n, 6)).astype(np.float32)
    assert len(np.unique(data, axis=0)) == n
    init = rng.permutation(n)
    pts, col = kc.split(data)
    want = kmeans_oracle.k_means_with_color(pts, n, col, init, max_iter=2)
    assert np.array_equal(want[1][init], np.arange(n)) and want[2:] == (1, True)
    with gsx.Context(0) as c:
        agrees(c.kmeans(pts, col, n, init, max_iter=2), want, f"n == k == {n}")


def test_kmeans_same_context_changing_k(gsx):
    """k = 2048, 3, 2048, 1261 on one Context: a stale LDS limit or a stale buffer of the larger k would show."""
    with gsx.Context(0) as c:
        got = []
        for k in (2048, 3, 2048, 1261):
            pts, col, init, want = edge_case(k)
            got.append(c.kmeans(pts, col, k, init, max_iter=2))
            agrees(got[-1], want, f"k {k} (call {len(got)})")
        assert same_bits(got[0][0], got[2][0]) and np.array_equal(got[0][1], got[2][1]) and got[0][2:] == got[2][2:]


def test_kmeans_rejects_and_stays_usable(gsx):
    pts, col, init, want = edge_case(3)
    with gsx.Context(0) as c:
        with pytest.raises(ValueError):
            c.kmeans(pts, col, 2049, np.arange(2049))               # k > 2048, the LDS capacity of the assign kernel
        agrees(c.kmeans(pts, col, 3, init, max_iter=2), want, "after the rejected k")
        with pytest.raises(ValueError):
            c.kmeans(pts, col, 3, init, max_iter=-1)
        with pytest.raises(ValueError):
            c.kmeans(pts, col, 3, np.arange(4))                     # init of the wrong length
        with pytest.raises(ValueError):
            c.kmeans(pts, col, 3, init[:2])
        agrees(c.kmeans(pts, col, 3, init, max_iter=2), want, "after the rejected arguments")


@pytest.mark.parametrize("where", ["first", "last", "run"])
def test_kmeans_empty_clusters_where_offsets_degenerate(gsx, where):
    """Empty clusters at index 0 (offsets[0] == offsets[1] == 0), at k - 1 (offsets[k - 1] == offsets[k] == n) and in three
    consecutive indices: they keep their centroid bit for bit, no label names them, all else as the oracle over 3 iterations.
    Index 0 can only be empty from the second pass on (kmeans_cases.empty_scene says why and how)."""
    data, init, empty = kc.empty_scene(where)
    pts, col = kc.split(data)
    k = len(init)
    want = kmeans_oracle.k_means_with_color(pts, k, col, init, max_iter=3)
    assert want[2] == 3 and not np.isin(want[1], empty).any() and len(np.unique(want[1])) == k - len(empty)
    if where == "first":
        one = kmeans_oracle.k_means_with_color(pts, k, col, init, max_iter=1)
        assert (one[1] == 0).sum() == 0 and (kmeans_oracle.assign(data, data[init]) == 0).sum() == 2    # {A, D}, then nobody
        kept = one[0][empty]
        assert not same_bits(kept, data[init][empty])
    else:
        kept = data[init][empty]
    with gsx.Context(0) as c:
        got = c.kmeans(pts, col, k, init, max_iter=3)
    agrees(got, want, where)
    assert same_bits(got[0][empty], kept) and not np.isin(got[1], empty).any()


def test_kmeans_distance_expression_decides(gsx):
    """20 000 rows on the diagonal against a centroid and three coordinate permutations of it: equally far in exact arithmetic,
    so the float64 rounding of ((d0^2 + d1^2) + d2^2) + d3^2, + d4^2, + d5^2 decides, and the first-minimum rule the ties that
    remain.  Asserted on the CPU first: at least 10 % of the rows get another label under the pairwise association, under the
    reversed one, and when d5^2 is folded in by a fused multiply-add (32.4 %, 49.5 % and 10.8 % measured) - a
    contracted, re-associated or narrowed kernel cannot pass.  max_iter = 0: labels straight from the initial rows."""
    data, init = kc.diagonal_scene()
    rows, cent = data[:kc.DIAG_ROWS], data[init]
    want = kmeans_oracle.assign(data, cent)
    assert (np.bincount(want[:kc.DIAG_ROWS], minlength=4) > 0).all()
    for other in (kc.labels_pairwise, kc.labels_reversed, kc.labels_fma_tail):
        share = float((other(rows, cent) != want[:kc.DIAG_ROWS]).mean())
        print(f"{other.__name__}: {share:.4f} of the diagonal rows change label")
        assert share >= 0.10, other.__name__
    pts, col = kc.split(data)
    with gsx.Context(0) as c:
        cent_out, labels, iters, conv = c.kmeans(pts, col, 4, init, max_iter=0)
    assert np.array_equal(labels, want), f"{int((labels != want).sum())} labels differ"
    assert same_bits(cent_out, cent) and (iters, conv) == (0, False)


def test_kmeans_loop_semantics(gsx):
    """The convergence test comes BEFORE the new centroids are adopted (k_means.py:132-138)."""
    data = kc.blobs(20_011, seed=8)
    pts, col = kc.split(data)
    init = np.random.default_rng(9).choice(len(data), 7, replace=False)
    with gsx.Context(0) as c:
        # tol = 1e30: converged in the first iteration, so the centroids in hand are still the initial rows
        got = c.kmeans(pts, col, 7, init, max_iter=10, tol=1e30)
        agrees(got, kmeans_oracle.k_means_with_color(pts, 7, col, init, max_iter=10, tol=1e30), "tol 1e30")
        assert got[2:] == (1, True) and same_bits(got[0], data[init]) and np.array_equal(got[1], kmeans_oracle.assign(data, data[init]))
        # tol = 0.0: no norm is < 0
        got = c.kmeans(pts, col, 7, init, max_iter=4, tol=0.0)
        agrees(got, kmeans_oracle.k_means_with_color(pts, 7, col, init, max_iter=4, tol=0.0), "tol 0")
        assert got[2:] == (4, False)
        got = c.kmeans(pts, col, 7, init, max_iter=1)
        agrees(got, kmeans_oracle.k_means_with_color(pts, 7, col, init, max_iter=1), "max_iter 1")
        assert got[2:] == (1, False)
        # seven tight blobs 100 apart, one initial row in each: the first update is final, the second finds a change of 0
        rng = np.random.default_rng(10)
        which = rng.integers(0, 7, size=20_011)
        which[:7] = np.arange(7)
        tight = (100.0 * np.eye(7, 6)[which] + rng.normal(size=(20_011, 6))).astype(np.float32)
        tp, tc = kc.split(tight)
        want = kmeans_oracle.k_means_with_color(tp, 7, tc, np.arange(7), max_iter=10)
        assert want[2:] == (2, True) and np.array_equal(want[1], which)
        agrees(c.kmeans(tp, tc, 7, np.arange(7), max_iter=10), want, "clean separation")


def test_kmeans_sign_of_a_zero_mean(gsx):
    """numpy's axis-0 reduction starts from +0.0, so the reference's mean of members that are all -0.0 is +0.0 - for a
    single member too (tests/test_oracle_kmeans.py pins that).  A sum kernel that starts its chain FROM the first member
    returns -0.0 for clusters 0 and 2 of this scene (== cannot tell; the bit patterns can); the mixed column of cluster 1 is
    +0.0 either way."""
    data, init, members = kc.zero_sign_scene()
    pts, col = kc.split(data)
    assert np.signbit(data[members[0], 4]).all() and np.signbit(data[members[2], 4]).all() and np.signbit(data[members[1][0], 4])
    assert not np.signbit(data[members[1], 4]).all()
    with gsx.Context(0) as c:
        for max_iter in (1, 2):
            want = kmeans_oracle.k_means_with_color(pts, 4, col, init, max_iter=max_iter)
            assert all(np.array_equal(np.nonzero(want[1] == j)[0], members[j]) for j in range(4))
            assert (want[0][:3, 4].view(np.uint32) == 0).all()                                 # +0.0, three times
            agrees(c.kmeans(pts, col, 4, init, max_iter=max_iter), want, f"max_iter {max_iter}")
