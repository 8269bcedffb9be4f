"""numpy model of the Mask2Former query post-processing (csrc/queries.hip, Context.segmap_from_queries): transformers'
post_process_instance_segmentation as the reference calls it (deep_learning_segmentation.py:156-158), op for op, from the K
slots its softmax / top-k selected to the map of segment ids (or class ids) at the image size.

This file is the specification.  Every product and sum of the bilinear step is one float32 operation (numpy rounds each), so
the device, built without contraction, gives the same `v` bit for bit; torch's CPU kernel contracts some of them to FMAs,
which is why the reference-made fixture (tools/make_golden_queries.py -> tests/golden/segmap_queries.npz) is compared up to
knife-edge pixels (knife_pixels) and must hold no knife-edge slot (knife_slots)."""
import numpy as np

F = np.float32
KNIFE_V = 2.0 ** -20        # |v| <= KNIFE_V * max|mask logits|: two evaluation orders of the four-tap sum may disagree in sign
KNIFE_SCORE = 1e-4          # |pred - threshold| <= KNIFE_SCORE: two summation orders may disagree on acceptance


# ---- the two index rules -------------------------------------------------------------------------------------------------------
def bilinear_axis(S, D):
    """torch's align_corners=False rule in float32, S source -> D destination: (i0, i1 int64 (D,), l0, l1 float32 (D,))"""
    scale = F(S) / F(D)
    src = np.maximum(scale * (np.arange(D, dtype=F) + F(0.5)) - F(0.5), F(0))
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < S - 1)
    l1 = src - i0.astype(F)
    return i0, i1, F(1) - l1, l1


def nearest_torch(S, D):
    """torch's 'nearest': min((int)floorf(d * scale), S - 1) with scale = (float)S / D in float32; int64 (D,)"""
    scale = F(S) / F(D)
    return np.minimum(np.floor(np.arange(D, dtype=F) * scale).astype(np.int64), S - 1)


def nearest_exact(S, D):
    return np.minimum(np.arange(D, dtype=np.int64) * S // D, S - 1)


def nearest_opencv(S, D):
    inv = 1.0 / (float(D) / float(S))
    return np.minimum(np.floor(np.arange(D, dtype=np.float64) * inv).astype(np.int64), S - 1)


def torch_rule_differs(S, D):
    """torch's float32 rule differs from floor(d * S / D) AND from OpenCV's rule somewhere"""
    t = nearest_torch(S, D)
    return bool((t != nearest_exact(S, D)).any() and (t != nearest_opencv(S, D)).any())


def differing_pairs(s_max=12, d_max=200):
    return [(S, D) for S in range(1, s_max + 1) for D in range(1, d_max + 1) if torch_rule_differs(S, D)]


# ---- step 1: bilinear to the mid grid ------------------------------------------------------------------------------------------------
def upsample(mask, mid_w, mid_h):
    """float32 (h, w) -> (mid_h, mid_w): v = ly0 * (lx0 * a00 + lx1 * a01) + ly1 * (lx0 * a10 + lx1 * a11), each op in float32"""
    a = np.asarray(mask, F)
    h, w = a.shape
    y0, y1, ly0, ly1 = bilinear_axis(h, mid_h)
    x0, x1, lx0, lx1 = bilinear_axis(w, mid_w)
    with np.errstate(invalid="ignore", over="ignore"):
        top = lx0[None, :] * a[y0][:, x0] + lx1[None, :] * a[y0][:, x1]
        bot = lx0[None, :] * a[y1][:, x0] + lx1[None, :] * a[y1][:, x1]
        v = ly0[:, None] * top + ly1[:, None] * bot
    assert v.dtype == F
    return v


def sigmoid(v):
    with np.errstate(over="ignore", invalid="ignore"):
        return F(1) / (F(1) + np.exp(-v.astype(F)))


# ---- the whole op ---------------------------------------------------------------------------------------------------------------------
def segmap_from_queries(masks, slot_query, slot_score, size, slot_label=None, mid=(384, 384), threshold=0.5, labels=False):
    """masks float32 (Q, h, w); slot_* (K,); size and mid = (width, height).  Returns a dict:
    map int32 (height, width), slot_segment int32 (K,), slot_pred float32 (K,), low int32 (mid_h, mid_w), and `v`, the
    upsampled mask of every query some slot read ({query: float32 (mid_h, mid_w)})."""
    masks = np.asarray(masks, F)
    Q = masks.shape[0]
    W, H = int(size[0]), int(size[1])
    mid_w, mid_h = int(mid[0]), int(mid[1])
    slot_query = np.asarray(slot_query, np.int64).reshape(-1)
    slot_score = np.asarray(slot_score, F).reshape(-1)
    K = len(slot_query)
    rows, cols = nearest_torch(mid_h, H), nearest_torch(mid_w, W)
    vs, sets = {}, {}
    seg = np.full(K, -1, np.int32)
    pred = np.zeros(K, F)
    low = np.full((mid_h, mid_w), -1, np.int32)
    n_acc = 0
    for k in range(K):
        q = int(slot_query[k])
        if not 0 <= q < Q:
            continue
        if q not in vs:
            vs[q] = upsample(masks[q], mid_w, mid_h)
            with np.errstate(invalid="ignore"):
                sets[q] = vs[q] > 0
        v, on = vs[q], sets[q]
        count = int(on.sum())
        total = F(np.nan) if np.isnan(v).any() else F(np.sum(sigmoid(v)[on].astype(np.float64)))
        with np.errstate(invalid="ignore"):
            pred[k] = slot_score[k] * (total / (F(count) + F(1e-6)))
        if on[rows][:, cols].any() and float(pred[k]) >= threshold:
            seg[k] = n_acc
            low[on] = int(slot_label[k]) if labels else n_acc
            n_acc += 1
    return {"map": low[rows][:, cols].astype(np.int32), "slot_segment": seg, "slot_pred": pred, "low": low, "v": vs}


# ---- where two correct implementations may differ ------------------------------------------------------------------------------------
def knife_slots(res, slot_query, Q, threshold=0.5):
    """bool (K,): slots whose score is within KNIFE_SCORE of the threshold (slots that read nothing are never knife-edge)"""
    slot_query = np.asarray(slot_query, np.int64).reshape(-1)
    valid = (slot_query >= 0) & (slot_query < Q)
    with np.errstate(invalid="ignore"):
        return valid & (np.abs(res["slot_pred"].astype(np.float64) - threshold) <= KNIFE_SCORE)


def knife_pixels(res, masks, slot_query, size):
    """bool (height, width): target pixels whose mid-grid source pixel has |v| <= KNIFE_V * max|mask logits| for some accepted slot"""
    masks = np.asarray(masks, F)
    W, H = int(size[0]), int(size[1])
    finite = np.abs(masks[np.isfinite(masks)])
    bound = KNIFE_V * float(finite.max()) if finite.size else 0.0
    slot_query = np.asarray(slot_query, np.int64).reshape(-1)
    mid_h, mid_w = res["low"].shape
    knife = np.zeros((mid_h, mid_w), bool)
    for k in np.nonzero(res["slot_segment"] >= 0)[0]:
        with np.errstate(invalid="ignore"):
            knife |= np.abs(res["v"][int(slot_query[k])]) <= bound
    return knife[nearest_torch(mid_h, H)][:, nearest_torch(mid_w, W)]


def select_slots(class_logits):
    """numpy restatement of the selection (softmax over the classes, the no-object column dropped, the Q largest of Q * C):
    (set of flat indices, scores float64 (Q * C,)).  The ORDER of the selection is torch's own and is not modelled."""
    x = np.asarray(class_logits, np.float64)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    p = (e / e.sum(axis=-1, keepdims=True))[:, :-1].reshape(-1)
    order = np.argsort(-p, kind="stable")[:x.shape[0]]
    return set(int(i) for i in order), p
