"""GPU: every form a class map can arrive in gives lift_view, assoc_view and label_map_tables the result of its int32 host form,
integer for integer.  The vote has this in test_vote_gpu.py::test_seg_dtypes_and_device_maps.

One 5 x 7 map with values in [-1, 2] as int32, int64, int16, uint8 labels (a copy without -1: they cannot say it), packed uint8
(label + 1) and in Fortran order, on the host and as a tensor on the GPU; and as a tensor that starts one element into a larger
buffer, whose pointer is aligned to its element only.  35 pixels are no multiple of the four a lane of the relabel and table
kernels reads at once: seg_bins4 (csrc/seg_dtype.hpp) takes its scalar tail, and on the shifted tensor only the scalar path."""
import numpy as np
import pytest

import assoc_cases as ac
import blend_cases

pytestmark = pytest.mark.gpu

H, W, C = 5, 7, 3
MAP = np.random.default_rng(57).integers(-1, C, (H, W)).astype(np.int32)
MAP_B = np.random.default_rng(75).integers(-1, C, (H, W)).astype(np.int32)
FORMS = {  # name -> (the map in that form, packed_u8, it is fed the copy without -1)
    "int32": (lambda m: m.astype(np.int32), False, False),
    "int64": (lambda m: m.astype(np.int64), False, False),
    "int16": (lambda m: m.astype(np.int16), False, False),
    "uint8": (lambda m: m.astype(np.uint8), False, True),
    "packed_u8": (lambda m: (m + 1).astype(np.uint8), True, False),
    "fortran": (lambda m: np.asfortranarray(m.astype(np.int32)), False, False),
}
CASES = [(f, s) for f in FORMS for s in ("host", "device")] + [(f, "shifted") for f in ("int32", "int64", "uint8", "packed_u8")]


def form_of(m, form, side):
    """-> (the map m as the case feeds it, packed_u8, the int32 host map it must agree with)"""
    import torch
    conv, packed, no_minus = FORMS[form]
    base = np.maximum(m, 0) if no_minus else m
    x = conv(base)
    if side == "device":
        x = torch.from_numpy(x).cuda()
        assert x.is_contiguous() == (form != "fortran")
    elif side == "shifted":
        buf = torch.from_numpy(np.concatenate([np.zeros(1, x.dtype), x.reshape(-1), np.zeros(4, x.dtype)])).cuda()
        x = buf.flatten()[1:1 + H * W].view(H, W)
        assert x.data_ptr() % (4 if x.element_size() == 1 else 16) == x.element_size() and x.is_contiguous()
    return x, packed, base.astype(np.int32)


def test_the_maps_hold_every_value():
    assert set(MAP.ravel().tolist()) == set(MAP_B.ravel().tolist()) == {-1, 0, 1, 2} and not np.array_equal(MAP, MAP_B)


# ---- lift: a handful of splats in front of the identity camera of a 7 x 5 frame ----------------------------------------------------
@pytest.fixture(scope="module")
def lift_ctx(gsx):
    rng = np.random.default_rng(5)
    sc = blend_cases.Scene("seg_forms", W, H)
    for _ in range(9):
        sc.add(rng.uniform(0, W), rng.uniform(0, H), rng.uniform(3.0, 5.0), rng.uniform(0.8, 2.0, 3), blend_cases.unit_quat(rng),
               int(rng.integers(40, 101)), rng.integers(0, 256, 3))
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays())
        yield c, sc.cam, {}


def lift_table(c, cam, seg, packed=False):
    c.lift_begin(C)
    c.lift_view(cam, seg, packed_u8=packed)
    return c.lift_table()


@pytest.mark.parametrize("form, side", CASES)
def test_lift_table(lift_ctx, form, side):
    c, cam, want = lift_ctx
    seg, packed, ref = form_of(MAP, form, side)
    key = ref.tobytes()
    if key not in want:
        want[key] = lift_table(c, cam, ref)
        assert (want[key].sum(0) > 0).sum() >= 3                       # the splats cover pixels of several classes
    assert np.array_equal(lift_table(c, cam, seg, packed), want[key])


# ---- assoc: 128 Gaussians, one per pixel of a 16 x 8 grid of the 40 x 24 image the 7 x 5 map is scaled to ---------------------------
_ASSOC = {}


def assoc_once(c, seg, packed=False):
    c.upload_positions(ac.grid_positions())
    c.assoc_begin(C, 16)
    remap, out = c.assoc_view(ac.small_cam(), seg, (ac.MW, ac.MH), packed_u8=packed)
    return remap, out.cpu().numpy(), c.assoc_table()


@pytest.mark.parametrize("form, side", CASES)
def test_assoc_remap_and_relabelled_map(ctx, form, side):
    seg, packed, ref = form_of(MAP, form, side)
    key = ref.tobytes()
    if key not in _ASSOC:
        _ASSOC[key] = assoc_once(ctx, ref)
        remap, out, _ = _ASSOC[key]
        assert sorted(remap.tolist()) == [0, 1, 2] and np.array_equal(out, np.where(ref >= 0, remap[np.maximum(ref, 0)], -1))
    for got, want in zip(assoc_once(ctx, seg, packed), _ASSOC[key]):
        assert got.dtype == want.dtype and np.array_equal(got, want)


# ---- label_map_tables: the form on both sides of the pair ----------------------------------------------------------------------------
_TABLES = {}


@pytest.mark.parametrize("form, side", CASES)
def test_label_map_tables(ctx, form, side):
    (a, packed, ref_a), (b, _, ref_b) = form_of(MAP, form, side), form_of(MAP_B, form, side)
    key = ref_a.tobytes() + ref_b.tobytes()
    if key not in _TABLES:
        _TABLES[key] = ctx.label_map_tables([ref_a], [ref_b], C, C)
        assert _TABLES[key].sum() == H * W and (_TABLES[key] > 0).sum() > C + 1
    for lds in (1, 0):
        ctx.set_option("iou_table_lds", lds)
        got = ctx.label_map_tables([a], [b], C, C, packed_u8=packed)
        ctx.set_option("iou_table_lds", 1)
        assert got.dtype == np.int64 and np.array_equal(got, _TABLES[key])
