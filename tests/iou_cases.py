"""Shared by the IoU tests: the reference-made fixture (tests/golden/iou.npz, tools/make_golden_iou.py) and exact compares."""
import functools
import os

import numpy as np

from conftest import GOLDEN

LABELME = ("0001_2", "0001_3", "DSCF4667", "street")


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(GOLDEN, "iou.npz"))
    return {k: z[k] for k in z.files}


def mask_cases():
    """[(name, masks, gts, iou (M, G), best_iou (M,), best_gt (M,))] as the reference computed them"""
    z = fixture()
    out = []
    for name in (str(n) for n in z["cases"]):
        masks = [z[f"{name}/mask{i}"] for i in range(int(z[f"{name}/n_masks"]))]
        gts = [z[f"{name}/gt{i}"] for i in range(int(z[f"{name}/n_gt"]))]
        out.append((name, masks, gts, z[f"{name}/iou"], z[f"{name}/best_iou"], z[f"{name}/best_gt"]))
    return out


def same_doubles(a, b):
    """equal bit patterns, NaNs in the same places"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.int64), b[ok].view(np.int64))


def copies(arrs):
    return [np.array(a) for a in arrs]
