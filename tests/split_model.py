"""The specification of gsx_split_labels / gsx_split_labels_lists (include/gsx.h) as plain numpy and Python: the edge rule over
given neighbour lists, a union-find over the edges, and the ranking of the components.  No GPU, no tolerance: the kernels
(csrc/split.hip) are held to this exactly."""
import numpy as np


def edges(nbr, labels, points=None, max_dist=None, ignore_label=None):
    """-> (i, j) int64 arrays: the list entries that are edges.  Row i names j, i != j, the labels agree and are not ignored,
    and d2(i, j) <= max_dist * max_dist with d2 = (dx*dx + dy*dy) + dz*dz in fp64 of the widened float32 coordinates."""
    nbr = np.asarray(nbr, np.int64)
    labels = np.asarray(labels, np.int32)
    n, k = nbr.shape
    i = np.repeat(np.arange(n, dtype=np.int64), k)
    j = nbr.reshape(-1)
    assert ((j >= 0) & (j < n)).all()
    keep = (i != j) & (labels[i] == labels[j])
    if ignore_label is not None:
        keep &= labels[i] != np.int32(ignore_label)
    if max_dist is not None and np.isfinite(max_dist):
        p = np.asarray(points, np.float32).reshape(n, 3).astype(np.float64)
        d = p[j] - p[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        keep &= d2 <= float(max_dist) * float(max_dist)       # one fp64 product; +inf for a huge max_dist, without a warning
    return i[keep], j[keep]


def components(n, i, j):
    """rep int64 (n,): the smallest index of every point's connected component under the undirected edges (i, j)"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    pairs = np.unique(np.stack((np.minimum(i, j), np.maximum(i, j)), axis=1), axis=0) if len(i) else np.zeros((0, 2), np.int64)
    for a, b in pairs.tolist():
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)        # the root is always the smallest index of its tree
    return np.array([find(x) for x in range(n)], np.int64)


def rank(reps, sizes, min_size=1, max_instances=0):
    """positions (into reps / sizes) of the instances in id order: size >= min_size, by size descending, then rep ascending,
    cut at max_instances when that is > 0"""
    reps, sizes = np.asarray(reps, np.int64), np.asarray(sizes, np.int64)
    at = np.flatnonzero(sizes >= min_size)
    at = at[np.lexsort((reps[at], -sizes[at]))]
    return at[:max_instances] if max_instances > 0 else at


def run(nbr, labels, points=None, max_dist=None, min_size=1, max_instances=0, ignore_label=None):
    """Everything the C call returns: dict(labels int32 (n,), component int32 (n,), label int32 (M,), size int64 (M,),
    rep int32 (M,), n_instances, n_components)."""
    labels = np.asarray(labels, np.int32).reshape(-1)
    n = len(labels)
    rep = components(n, *edges(nbr, labels, points, max_dist, ignore_label))
    ignored = labels == np.int32(ignore_label) if ignore_label is not None else np.zeros(n, bool)
    roots, sizes = np.unique(rep[~ignored], return_counts=True)
    at = rank(roots, sizes, min_size, max_instances)
    id_of = np.full(n, -1, np.int64)
    id_of[roots[at]] = np.arange(len(at))
    out = np.where(ignored, -1, id_of[rep])
    return {"labels": out.astype(np.int32), "component": np.where(ignored, -1, rep).astype(np.int32),
            "label": labels[roots[at]].astype(np.int32), "size": sizes[at].astype(np.int64), "rep": roots[at].astype(np.int32),
            "n_instances": len(at), "n_components": len(roots)}
