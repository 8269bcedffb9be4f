"""Case builders for the Mask2Former query post-processing (csrc/queries.hip): the reference-made fixture
(tests/golden/segmap_queries.npz, tools/make_golden_queries.py) and constructed inputs that sit on the kernels' structural edges
(gsx_debug_queries_constants) and on the edges of the semantics (tests/queries_model.py).

A case is a dict: name, masks float32 (Q, h, w), slot_query / slot_score / slot_label (K,), size and mid = (width, height),
threshold; fixture cases also hold map, label_ids, scores and class_logits.  `exact`: the case places a slot ON the threshold by
construction (its score is exact); every other case must hold no knife-edge slot, which the tests assert on the model."""
import os

import numpy as np

import queries_model as QM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segmap_queries.npz")
_FIX = None
F = np.float32


def fixture_cases():
    global _FIX
    if _FIX is None:
        z = np.load(GOLDEN)
        mid = tuple(int(v) for v in z["mid"])
        _FIX = [dict(name=str(n), masks=z[f"{n}/masks"], class_logits=z[f"{n}/class_logits"], slot_query=z[f"{n}/slot_query"],
                     slot_score=z[f"{n}/slot_score"], slot_label=z[f"{n}/slot_label"], size=tuple(int(v) for v in z[f"{n}/size"]), mid=mid,
                     threshold=0.5, map=z[f"{n}/map"], label_ids=z[f"{n}/label_ids"], scores=z[f"{n}/scores"]) for n in z["cases"]]
    return _FIX


def case(name, masks, slot_query, slot_score, size, mid, slot_label=None, threshold=0.5, exact=False):
    slot_query = np.asarray(slot_query, np.int32).reshape(-1)
    if slot_label is None:
        slot_label = (np.arange(len(slot_query)) * 7 + 3) % 150
    return dict(name=name, masks=np.ascontiguousarray(masks, F), slot_query=slot_query, slot_score=np.asarray(slot_score, F).reshape(-1),
                slot_label=np.asarray(slot_label, np.int32).reshape(-1), size=tuple(size), mid=tuple(mid), threshold=threshold, exact=exact)


def model(c, labels=False):
    return QM.segmap_from_queries(c["masks"], c["slot_query"], c["slot_score"], c["size"], c["slot_label"], c["mid"], c["threshold"], labels)


def seeded(name, seed, Q, h, w, K, size, mid, quarter=True):
    """Mask logits in quarters (exact in fp16 and bf16) of mixed sign, K slots drawn over Q queries (queries repeat), scores on both
    sides of what the threshold needs.  The seed is advanced until the model sees no knife-edge slot:
    that is a property of the inputs, decided by the model alone."""
    for s in range(seed, seed + 50):
        rng = np.random.default_rng(s)
        coarse = rng.integers(-24, 17, (Q, (h + 1) // 2, (w + 1) // 2))
        masks = (np.repeat(np.repeat(coarse, 2, 1), 2, 2)[:, :h, :w] + rng.integers(-4, 5, (Q, h, w))).astype(F) / (4 if quarter else 3)
        c = case(name, masks, rng.integers(0, Q, K), rng.choice(np.array([0.3, 0.62, 0.8, 0.95, 0.999], F), K), size, mid)
        r = model(c)
        acc = r["slot_segment"] >= 0
        if not QM.knife_slots(r, c["slot_query"], Q).any() and (K < 4 or (acc.any() and not acc.all())):    # both kinds of slot
            return c
    raise AssertionError(f"{name}: no seed without a knife-edge slot")


def constructed_cases(U):
    """U: gsx.queries_constants()"""
    cols, rows_wg, rows_wave, word, waves = U["cols"], U["rows_wg"], U["rows_wave"], U["scan_word"], U["accept_waves"]
    out = []
    # ragged ballot words and row groups: mid widths around one and two words, heights around a wave's and a workgroup's rows
    for mw in (1, cols - 1, cols, cols + 1, 2 * cols + 1):
        for mh in (1, 5):
            out.append(seeded(f"mid_{mw}x{mh}", 1000 + mw * 7 + mh, 5, 4, 6, 7, (mw + 3, 7), (mw, mh)))
    for mh in (rows_wave, rows_wave + 1, rows_wg - 1, rows_wg, rows_wg + 1, 2 * rows_wg + 3):
        out.append(seeded(f"mid_70x{mh}", 1200 + mh, 4, 5, 5, 6, (9, mh + 2), (70, mh)))
    # source sizes: one row, one column, one pixel, as large as the mid grid, larger
    out.append(seeded("src_h1", 1300, 4, 1, 9, 6, (31, 17), (40, 12)))
    out.append(seeded("src_w1", 1301, 4, 9, 1, 6, (31, 17), (40, 12)))
    out.append(seeded("src_1x1", 1302, 4, 1, 1, 6, (5, 4), (9, 3)))
    out.append(seeded("src_eq_mid", 1303, 4, 12, 40, 6, (31, 17), (40, 12)))
    out.append(seeded("src_gt_mid", 1304, 4, 30, 90, 6, (31, 17), (40, 12)))
    out.append(seeded("src_thirds", 1305, 6, 7, 11, 9, (50, 33), (70, 21), quarter=False))
    # v == 0 exactly: taps -3 and 1 at weights .25 / .75 (w = 2 -> mid_w = 4, destination 2); 0 is not set
    out.append(case("v_zero", [[[-3.0, 1.0]]], [0], [0.9], (4, 1), (4, 1)))
    # slot counts: K = 1, around the scan's ballot word, around the accept kernel's waves, 129; K > Q: queries repeat
    for K in sorted({1, 2, waves - 1, waves, waves + 1, word - 1, word, word + 1, 2 * word + 1}):
        out.append(seeded(f"k{K}", 1400 + K, 9, 6, 6, K, (21, 13), (70, 9)))
    # every slot rejected by its score
    c = seeded("all_rejected", 1500, 5, 6, 6, 8, (21, 13), (30, 9))
    out.append(dict(c, slot_score=np.full(8, 0.05, F)))
    # a whole-mask +30 slot: sigmoid(30) == 1 in fp32, so pred is exactly the score - 0.5 is accepted, the float below is not
    full = np.full((1, 3, 3), 30.0, F)
    out.append(case("on_threshold", full, [0, 0, 0], [np.nextafter(F(0.5), F(0)), 0.5, np.nextafter(F(0.5), F(0))], (5, 4), (8, 8), exact=True))
    # set pixels only on rows / columns the 8 x 8 -> 3 x 5 target never reads (it reads columns 0, 2, 5 and rows 0, 1, 3, 4, 6)
    m = np.full((4, 8, 8), -2.0, F)
    m[0, 2, :] = 2.0
    m[0, 7, :] = 2.0                 # query 0: rows 2 and 7 only
    m[1, :, 1] = 2.0
    m[1, :, 3] = 2.0                 # query 1: columns 1 and 3 only
    m[2, 2, 2] = 2.0                 # query 2: one pixel on a read column but an unread row
    m[3, 3:6, 4:7] = 2.0             # query 3: a block that is read
    out.append(case("unsampled", m, [0, 3, 1, 2, 3], [0.9] * 5, (3, 5), (8, 8)))
    # a NaN logit, and an inf logit under a zero weight (h == mid: the second tap's weight is 0, 0 * inf = NaN): both reject the slot
    m = np.full((3, 4, 4), 1.5, F)
    m[0, 1, 2] = np.nan
    m[1, 3, 3] = np.inf
    out.append(case("nan_inf", m, [2, 0, 2, 1, 2], [0.9] * 5, (9, 6), (4, 4)))
    m = np.full((2, 4, 4), 1.5, F)
    m[0, 1, 1] = -np.inf             # -inf: its own pixel is not set, the pixels whose zero-weight tap it is become NaN
    out.append(case("neg_inf", m, [0, 1], [0.9, 0.9], (9, 6), (4, 4)))
    # slot_query outside [0, Q)
    c = seeded("bad_query", 1600, 3, 5, 5, 7, (17, 11), (20, 10))
    q = c["slot_query"].copy()
    q[1], q[4] = -1, 3
    out.append(dict(c, slot_query=q, slot_score=np.full(7, 0.95, F)))
    # a rejected slot after an accepted one does not overwrite it
    m = np.full((2, 3, 3), 4.0, F)
    out.append(case("rejected_after", m, [0, 1, 1], [0.9, 0.1, np.nan], (7, 5), (6, 6)))
    # torch's fp32 nearest rule where it differs from floor(d * S / D) and from OpenCV's rule, on both axes
    pairs = QM.differing_pairs()
    assert len(pairs) >= 4
    for (S1, D1), (S2, D2) in zip(pairs[:6:2], pairs[1:6:2]):
        out.append(seeded(f"nearest_{S1}to{D1}_{S2}to{D2}", 1700 + S1 + D1, 6, 3, 3, 6, (D1, D2), (S1, S2)))
        out.append(seeded(f"nearest_{S2}to{D2}_{S1}to{D1}", 1800 + S1 + D1, 6, 3, 3, 6, (D2, D1), (S2, S1)))
    return out


def reference_shape_case():
    """Q = K = 100, 96 x 96 -> 384 x 384 -> 270 x 480: smooth mask logits, several slots per query"""
    for s in range(1900, 1950):
        rng = np.random.default_rng(s)
        coarse = rng.standard_normal((100, 13, 13)).astype(F)
        masks = np.repeat(np.repeat(coarse, 8, 1), 8, 2)[:, :96, :96] * 6 + rng.standard_normal((100, 96, 96)).astype(F) - 2
        c = case("reference_shape", masks, rng.integers(0, 100, 100), rng.uniform(0.3, 1.0, 100), (480, 270), (384, 384))
        if not QM.knife_slots(model(c), c["slot_query"], 100).any():
            return c
    raise AssertionError("reference_shape: no seed without a knife-edge slot")
