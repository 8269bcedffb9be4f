"""numpy restatement of the label filter's contract (include/gsx.h, gsx_smooth_labels) from neighbour index rows - where the
rows come from (region_growing_model.knn, nn_cases.model_lists, or lists made up by a test) is the caller's business.

One round, L = the labels at its start (Jacobi: every point reads L):
  count[c] = number of j in N(i) with L[j] == c; neighbours whose label is `ignore_label` cast no vote (ignore_label None:
  every neighbour votes).  No neighbour votes: new[i] = L[i].  Otherwise m = max count, W = the labels that reach m; the
  winner is L[i] if L[i] is in W, else min(W).  new[i] = winner unless m < min_votes.  fill_only: new[i] = L[i] whenever
  L[i] != fill_label.  support[i] = count[new[i]] (0 when that label cast no vote).
A row may name a point twice: it votes twice.

round_rows is vectorised; round_slow says the same with a dict per row and is what test_smooth_frontend.py holds it to."""
import numpy as np

I64_MAX = np.iinfo(np.int64).max


def round_rows(nbr, L, rows=None, min_votes=1, ignore_label=None, fill_only=False, fill_label=None):
    """One round for the points `rows` (default: all, then len(nbr) == len(L)), nbr[r] = the neighbours of rows[r].
    fill_label: the label fill_only spares everything but (default: ignore_label).  Returns (new int32 (m,), support int32 (m,))."""
    L = np.asarray(L).astype(np.int64)
    nbr = np.asarray(nbr)
    rows = np.arange(len(L)) if rows is None else np.asarray(rows)
    assert len(nbr) == len(rows)
    fill_label = ignore_label if fill_label is None else fill_label
    m_rows, k = nbr.shape
    new = np.empty(m_rows, np.int64)
    sup = np.empty(m_rows, np.int64)
    step = max(1, (1 << 24) // (k * k))
    for s in range(0, m_rows, step):
        V = L[nbr[s:s + step]]                                            # (b, k)
        own = L[rows[s:s + step]]
        votes = np.ones(V.shape, bool) if ignore_label is None else V != ignore_label
        cnt = ((V[:, :, None] == V[:, None, :]) & votes[:, None, :]).sum(axis=2)   # voters that share column j's label
        cnt = np.where(votes, cnt, 0)
        m = cnt.max(axis=1)
        cand = votes & (cnt == m[:, None])
        wmin = np.where(cand, V, I64_MAX).min(axis=1)
        own_in = (cand & (V == own[:, None])).any(axis=1)
        out = np.where((m >= 1) & (m >= min_votes), np.where(own_in, own, wmin), own)
        if fill_only:
            out = np.where(own != fill_label, own, out)
        new[s:s + step] = out
        sup[s:s + step] = (votes & (V == out[:, None])).sum(axis=1)
    return new.astype(np.int32), sup.astype(np.int32)


def round_slow(nbr, L, min_votes=1, ignore_label=None, fill_only=False, fill_label=None):
    """round_rows for every point, one row at a time with a dict: the contract read aloud"""
    fill_label = ignore_label if fill_label is None else fill_label
    new, sup = [], []
    for i, row in enumerate(np.asarray(nbr).tolist()):
        count = {}
        for j in row:
            c = int(L[j])
            if ignore_label is None or c != ignore_label:
                count[c] = count.get(c, 0) + 1
        own = int(L[i])
        w = own
        if count:
            m = max(count.values())
            W = [c for c, v in count.items() if v == m]
            if m >= min_votes:
                w = own if own in W else min(W)
        if fill_only and own != fill_label:
            w = own
        new.append(w)
        sup.append(count.get(w, 0))
    return np.array(new, np.int32), np.array(sup, np.int32)


def run(nbr, L, rounds=1, min_votes=1, ignore_label=None, fill_only=False, fill_label=None):
    """The whole call on every point.  Returns (labels, changed list of `rounds` counts, rounds executed, support of the last
    executed round)."""
    L = np.asarray(L, np.int32)
    changed = [0] * rounds
    done = 0
    sup = None
    for r in range(rounds):
        new, sup = round_rows(nbr, L, None, min_votes, ignore_label, fill_only, fill_label)
        changed[r] = int((new != L).sum())
        L = new
        done = r + 1
        if not changed[r]:
            break
    return L, changed, done, sup
