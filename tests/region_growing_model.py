"""numpy-only fp64 restatement of 3D_clustering/region_growing.py (compute_normals :78-129, compute_residuals
:132-163, segmentation_3D :166-226): brute-force exact k-NN, fp64 moments, numpy.linalg.eigh, the same sequential
growth.  It is the model the HIP kernels (csrc/normals.hip) and the host growth (csrc/region_grow.cpp) are tested
against at sizes the fixture cannot hold; tools/make_golden_region_growing.py pins it to the reference itself.

Distances are fp64 of the widened float32 coordinates, (dx*dx + dy*dy) + dz*dz - the expression the kernels evaluate,
so the neighbour ORDER agrees bit for bit.  Ties: nearer first, then lower index."""
import numpy as np


def knn(points, k, queries=None, chunk=None, with_next=False):
    """Exact k nearest points of every query row (default: every point), ascending (d2, index).
    Returns (index int32 (m, k), d2 float64 (m, k)); with_next: d2 has k + 1 columns (inf if n == k)."""
    P = np.ascontiguousarray(points, np.float32).astype(np.float64)
    n = len(P)
    q = np.arange(n) if queries is None else np.asarray(queries)
    m = len(q)
    kk = k + 1 if with_next and n > k else k
    idx = np.empty((m, k), np.int32)
    d2o = np.full((m, k + 1 if with_next else k), np.inf)
    chunk = chunk or max(1, min(m, (1 << 24) // max(n, 1)))
    for s in range(0, m, chunk):
        Q = P[q[s:s + chunk]]
        dx = P[None, :, 0] - Q[:, None, 0]
        d2 = dx * dx
        dx = P[None, :, 1] - Q[:, None, 1]
        d2 += dx * dx
        dx = P[None, :, 2] - Q[:, None, 2]
        d2 += dx * dx
        if kk < n:
            kth = np.partition(d2, kk - 1, axis=1)[:, kk - 1]
        else:
            kth = np.full(len(Q), np.inf)
        for r in range(len(Q)):
            cand = np.flatnonzero(d2[r] <= kth[r])
            o = cand[np.lexsort((cand, d2[r, cand]))][:kk]
            idx[s + r] = o[:k]
            d2o[s + r, :len(o)] = d2[r, o]
    return idx, d2o


def normals_from_neighbours(points, nbr, queries=None):
    """PCA normal and residual of every query from its neighbour rows.  Returns (normals (m, 3), residuals (m,),
    flip dot (m,) = dot(normal, p - centroid) after orientation, eigen-gap (l1 - l0) / l2)."""
    P = np.ascontiguousarray(points, np.float32).astype(np.float64)
    q = np.arange(len(P)) if queries is None else np.asarray(queries)
    m = len(q)
    nrm = np.empty((m, 3))
    dot = np.empty(m)
    gap = np.empty(m)
    step = max(1, (1 << 22) // nbr.shape[1])
    for s in range(0, m, step):
        N = P[nbr[s:s + step]]                                  # (b, k, 3)
        cen = N.mean(axis=1)
        D = N - cen[:, None, :]
        cov = np.einsum("bki,bkj->bij", D, D)
        w, v = np.linalg.eigh(cov)
        nv = v[:, :, 0]
        d = np.einsum("bi,bi->b", nv, P[q[s:s + step]] - cen)
        flip = d > 0
        nv = np.where(flip[:, None], -nv, nv)
        d = np.where(flip, -d, d)
        nv = nv / np.linalg.norm(nv, axis=1, keepdims=True)
        nrm[s:s + step] = nv
        dot[s:s + step] = d
        with np.errstate(divide="ignore", invalid="ignore"):
            gap[s:s + step] = np.where(w[:, 2] > 0, (w[:, 1] - w[:, 0]) / w[:, 2], 0.0)
    return nrm, np.abs(dot), dot, gap


def moments(points, nbr, queries=None):
    """(centroid (m, 3), centered^T centered (m, 3, 3), largest squared distance between the query and a neighbour (m,))
    of every neighbour row"""
    P = np.ascontiguousarray(points, np.float32).astype(np.float64)
    q = np.arange(len(P)) if queries is None else np.asarray(queries)
    m = len(nbr)
    cen = np.empty((m, 3))
    cov = np.empty((m, 3, 3))
    r2 = np.empty(m)
    step = max(1, (1 << 22) // nbr.shape[1])
    for s in range(0, m, step):
        N = P[nbr[s:s + step]]
        cen[s:s + step] = N.mean(axis=1)
        D = N - cen[s:s + step, None, :]
        cov[s:s + step] = np.einsum("bki,bkj->bij", D, D)
        Dq = N - P[q[s:s + step], None, :]
        r2[s:s + step] = (Dq * Dq).sum(axis=2).max(axis=1)
    return cen, cov, r2


def normals(points, k, queries=None):
    nbr, _ = knn(points, k, queries)
    return normals_from_neighbours(points, nbr, queries)


def grow(normals_, residuals, nbr, residual_threshold, angle_threshold, with_margin=False):
    """segmentation_3D.  Returns (labels int32: rank of the region by size, largest first, creation order among equals;
    n_regions[, smallest |margin| of any accept / reject decision])."""
    n = len(residuals)
    nrm = np.asarray(normals_, np.float64)
    res = np.asarray(residuals, np.float64)
    order = np.argsort(res, kind="stable")
    cos_thr = np.cos(angle_threshold)
    region = np.full(n, -1, np.int64)
    sizes = []
    margin = np.inf
    nxt = 0
    nb_list = np.asarray(nbr).tolist()
    resl = res.tolist()
    while True:
        while nxt < n and region[order[nxt]] >= 0:
            nxt += 1
        if nxt == n:
            break
        rid = len(sizes)
        seed0 = int(order[nxt])
        region[seed0] = rid
        queue = [seed0]
        head = 0
        while head < len(queue):
            seed = queue[head]
            head += 1
            ns = nrm[seed]
            for v in nb_list[seed]:
                if region[v] >= 0:
                    continue
                c = abs(float(ns[0] * nrm[v, 0] + ns[1] * nrm[v, 1] + ns[2] * nrm[v, 2]))
                margin = min(margin, abs(c - cos_thr))
                if c > cos_thr:
                    region[v] = rid
                    margin = min(margin, abs(resl[v] - residual_threshold))
                    if resl[v] < residual_threshold:
                        queue.append(v)
        sizes.append(rid)
    sizes = np.bincount(region, minlength=len(sizes))
    by_size = np.argsort(-sizes, kind="stable")
    rank = np.empty(len(sizes), np.int64)
    rank[by_size] = np.arange(len(sizes))
    labels = rank[region].astype(np.int32)
    if with_margin:
        return labels, len(sizes), float(margin)
    return labels, len(sizes)


def same_regions(a, b):
    """True iff the two labellings are the same regions (as sets) with the same sizes in label order; regions of equal
    size may be numbered differently (their mutual order depends on the order the seeds were met)."""
    a = np.asarray(a).astype(np.int64)
    b = np.asarray(b).astype(np.int64)
    if a.shape != b.shape or a.min() < 0 or b.min() < 0:
        return False
    na, nb = np.bincount(a), np.bincount(b)
    if not np.array_equal(na, nb):
        return False
    pairs = np.unique(a * len(nb) + b)
    return len(pairs) == len(na)


def labels_from_regions(regions, n):
    """The reference returns a size-sorted list of index lists (:221-226): label = position in that list."""
    lab = np.full(n, -1, np.int32)
    for r, members in enumerate(regions):
        lab[np.asarray(members, np.int64)] = r
    assert (lab >= 0).all()
    return lab
