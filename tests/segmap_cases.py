"""Case builders for the class-map producer (csrc/segmap.hip): the reference-made fixture (tests/golden/segmap.npz,
tools/make_golden_segmap.py) and constructed volumes that put ties, NaNs and signed zeros on the kernels' structural edges."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segmap.npz")
_FIX = None


def fixture():
    global _FIX
    if _FIX is None:
        _FIX = dict(np.load(GOLDEN))
    return _FIX


def logits_cases():
    """[(name, logits float32 (C, h, w), (width, height), map int32 (height, width))]"""
    z = fixture()
    return [(str(n), z[f"logits/{n}/logits"], tuple(int(v) for v in z[f"logits/{n}/size"]), z[f"logits/{n}/map"]) for n in z["cases_logits"]]


def masks_cases():
    """[(name, masks float32 (K, mh, mw), cls (K,), conf (K,), (width, height), map int32 (height, width))]"""
    z = fixture()
    return [(str(n), z[f"masks/{n}/masks"], z[f"masks/{n}/cls"], z[f"masks/{n}/conf"], tuple(int(v) for v in z[f"masks/{n}/size"]),
             z[f"masks/{n}/map"]) for n in z["cases_masks"]]


def channel_counts(K):
    """C = 1, one step and one round of the slices +-1, 255, 256, 1000"""
    step, rnd = K["step"], K["step"] * K["slices"]
    return sorted({1, 2, step - 1, step, step + 1, rnd - 1, rnd, rnd + 1, 2 * rnd + 1, 255, 256, 1000})


def boundary_volume(C, K):
    """float32 (C, 1, P): one pixel per pattern.  For every channel boundary b (every multiple of the step size: a boundary
    between two steps, between two slices, and - every slices * step channels - between two rounds of one slice) and the two
    channels a = b - 1, b on either side of it:
      tie           a and b hold the maximum: a wins          tie_far      0 and b hold it: 0 wins
      nan_first     NaN at a, +inf at b: a wins               inf_first    +inf at a, NaN at b: b wins (a NaN is the maximum)
      two_nans      NaN at a and b: a wins                    zeros        -0.0 at a, +0.0 at b, the rest negative: a wins
      zeros_rev     +0.0 at a, -0.0 at b: a wins              late         the maximum only at b"""
    step = K["step"]
    bounds = [b for b in range(step, C, step)] or ([1] if C > 1 else [])
    cols = []
    for b in bounds:
        a = b - 1
        base = -1.0 - (np.arange(C, dtype=np.float32) % 5)

        def col(**kv):
            v = base.copy()
            for k, x in kv.items():
                v[int(k[1:])] = x
            cols.append(v)

        col(**{f"c{a}": 3.0, f"c{b}": 3.0})
        col(**{"c0": 3.0, f"c{b}": 3.0})
        col(**{f"c{a}": np.nan, f"c{b}": np.inf})
        col(**{f"c{a}": np.inf, f"c{b}": np.nan})
        col(**{f"c{a}": np.nan, f"c{b}": np.nan})
        col(**{f"c{a}": -0.0, f"c{b}": 0.0})
        col(**{f"c{a}": 0.0, f"c{b}": -0.0})
        col(**{f"c{b}": 7.0})
    cols.append(np.full(C, -np.inf, np.float32))                 # all -inf -> 0
    cols.append(np.where(np.arange(C) % 2 == 0, -0.0, 0.0).astype(np.float32))   # only zeros of both signs -> 0
    cols.append(np.full(C, np.nan, np.float32))                  # all NaN -> 0
    last = np.full(C, -np.inf, np.float32)
    last[C - 1] = -3.0e38
    cols.append(last)                                            # the maximum in the very last channel
    return np.stack(cols, axis=1).reshape(C, 1, len(cols)).astype(np.float32)


def seeded_logits(rng, shape, ties=True):
    """small integers (ties everywhere) or normals, float32"""
    if ties:
        return rng.integers(-3, 4, shape).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


def seeded_masks(rng, K, mh, mw, density=0.3):
    """float32 (K, mh, mw): values in {0, 0.25, 0.5, 0.75, 1} - exact in fp16 and bf16 too -, cls in 0..79, conf on both sides of 0.5"""
    m = (rng.random((K, mh, mw)) < density) * rng.choice(np.array([0.25, 0.5, 0.75, 1.0], np.float32), (K, mh, mw))
    cls = rng.integers(0, 80, K).astype(np.float32)
    conf = rng.choice(np.array([0.25, 0.5, 0.5000001, 0.75, 0.9375], np.float32), K)
    return m.astype(np.float32), cls, conf
