"""The k-means oracle (oracle/kmeans_oracle.py) against the vectors the reference itself produced
(tests/golden/kmeans.npz, tools/make_golden_kmeans.py): labels and float32 centroids bit-exact."""
import os

import numpy as np
import pytest

from oracle import kmeans_oracle

GOLD = os.path.join(os.path.dirname(__file__), "golden", "kmeans.npz")


def golden_cases():
    z = np.load(GOLD)
    names = sorted({k.split("/")[0] for k in z.files})
    return [(n, {k.split("/")[1]: z[k] for k in z.files if k.startswith(n + "/")}) for n in names]


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c[0])
def test_oracle_equals_reference(case):
    name, g = case
    cent, labels, iters, converged = kmeans_oracle.k_means_with_color(g["points"], int(g["k"]), g["colors"], g["init"],
                                                                       max_iter=int(g["max_iter"]))
    assert np.array_equal(labels, g["labels"]), name
    assert cent.dtype == np.float32 and np.array_equal(cent, g["centroids"]), name
    assert converged == bool(g["converged"])


def test_mean_is_sequential_float32_and_distance_order():
    """The two numerical facts the restatement (and the GPU kernels) rely on."""
    rng = np.random.default_rng(0)
    a = (rng.normal(size=(20_001, 6)) * np.array([1e-3, 1, 1e3, 1, 1, 1])).astype(np.float32)
    acc = np.zeros(6, np.float32)
    for row in a:
        acc = (acc + row).astype(np.float32)
    assert np.array_equal(a.mean(axis=0), acc / np.float32(len(a)))
    from scipy.spatial import KDTree
    cent = rng.normal(size=(13, 6)).astype(np.float32)
    pts = rng.normal(size=(3000, 6)).astype(np.float32)
    tree = KDTree(cent)
    assert np.array_equal(np.array([tree.query(p)[1] for p in pts]), kmeans_oracle.assign(pts, cent))


def test_assign_does_not_depend_on_the_chunk_size():
    """assign() bounds its temporaries by k (k = 2048 would otherwise need tens of GB); the arithmetic is elementwise"""
    g = dict(golden_cases())["uniform_k13"]
    data = np.concatenate((g["points"], g["colors"]), axis=1)
    for cent in (data[g["init"]], g["centroids"]):
        want = kmeans_oracle.assign(data, cent)
        for chunk in (1, 7, 200_000):
            assert np.array_equal(kmeans_oracle.assign(data, cent, chunk=chunk), want), chunk
    assert np.array_equal(kmeans_oracle.assign(data, g["centroids"]), g["labels"])
    big = kmeans_oracle.assign(data[:300], np.tile(data[:1024], (2, 1)))          # k = 2048, duplicates: the first copy wins
    assert big.max() < 1024 and np.array_equal(big[:300], np.arange(300))


def test_kd_tree_agrees_on_the_diagonal_rows():
    """tests/kmeans_cases.py::diagonal_scene: every diagonal row is equally far, in exact arithmetic, from the four centroids,
    so the reference's KD-tree query and the oracle's arg-min agree only if they round the squared distance alike.  Rows whose
    smallest float64 distance occurs more than once are left out - the tree's traversal order breaks such ties in the
    reference (oracle/kmeans_oracle.py: unpinned): 17 718 of the 20 004 rows; the other 2 286 must agree, and they do not
    agree with the pairwise or the reversed summation."""
    import kmeans_cases as kc
    from scipy.spatial import KDTree
    data, init = kc.diagonal_scene()
    cent = data[init]
    d = kmeans_oracle.sq_distances(data, cent)
    tied = (d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1
    print(f"{int(tied.sum())} of {len(data)} rows left out (exactly tied in float64)")
    assert int(tied.sum()) == 17_718 and not tied[init].any()
    want = kmeans_oracle.assign(data, cent)
    got = KDTree(cent).query(data)[1]
    assert np.array_equal(got[~tied], want[~tied])
    assert len(np.unique(want[~tied])) == 4
    for other in (kc.labels_pairwise, kc.labels_reversed):
        assert (other(data, cent)[~tied] != want[~tied]).mean() > 0.10, other.__name__


@pytest.mark.parametrize("m", [1, 2, 1921])
def test_mean_of_negative_zeros_is_positive_zero(m):
    """The reference takes members.mean(axis=0) (k_means.py:126); numpy's reduction over axis 0 starts from +0.0, and
    (+0.0) + (-0.0) = +0.0 - also for a single member.  == cannot tell, so the bit patterns are compared."""
    import kmeans_cases as kc
    members = np.full((m, 6), -0.0, np.float32)
    assert np.signbit(members).all()
    assert kc.same_bits(members.mean(axis=0), np.zeros(6, np.float32))
    mixed = members.copy()
    mixed[1::2] = 0.0                                                   # first member -0.0
    assert kc.same_bits(mixed.mean(axis=0), np.zeros(6, np.float32))
    new = kmeans_oracle.update(members, np.zeros(m, np.int64), np.full((2, 6), -0.0, np.float32))
    assert kc.same_bits(new[0], np.zeros(6, np.float32))
    assert np.signbit(new[1]).all()                                     # the empty cluster keeps its centroid, sign and all
