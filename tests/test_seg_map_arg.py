"""labeler._seg_map_arg on numpy inputs: the one place where a class map given to vote_view, lift_view, assoc_view or
label_map_tables becomes (C-contiguous 2-D array, GSX_SEG_* code, h, w, device).  No GPU and no library call."""
import numpy as np
import pytest

from conftest import load_pkg

L, lib = load_pkg().labeler, load_pkg()._lib

H, W = 5, 7
MAP = (np.arange(H * W).reshape(H, W) * 5 % 4 - 1).astype(np.int32)          # every value of [-1, 2]


def arg(x, packed_u8=False):
    seg, dt, h, w, device = L._seg_map_arg(x, packed_u8)
    assert type(seg) is np.ndarray and seg.flags.c_contiguous and seg.ndim == 2 and (h, w) == seg.shape and device is False
    return seg, dt


def test_the_map_holds_every_value():
    assert MAP.shape == (H, W) and set(MAP.ravel().tolist()) == {-1, 0, 1, 2}


@pytest.mark.parametrize("dtype, code", [(np.int32, lib.GSX_SEG_I32), (np.int64, lib.GSX_SEG_I64), (np.uint8, lib.GSX_SEG_U8_LABELS)])
def test_supported_dtypes_pass_through_as_they_are(dtype, code):
    x = (MAP + 1).astype(dtype)
    seg, dt = arg(x)
    assert seg is x and dt == code


def test_packed_u8_concerns_uint8_only():
    x8, x32 = (MAP + 1).astype(np.uint8), MAP.copy()
    seg, dt = arg(x8, packed_u8=True)
    assert seg is x8 and dt == lib.GSX_SEG_U8
    seg, dt = arg(x32, packed_u8=True)
    assert seg is x32 and dt == lib.GSX_SEG_I32


@pytest.mark.parametrize("form", ["int16", "bool", "uint16", "float list"])
def test_other_dtypes_are_widened_to_int32(form):
    x = {"int16": lambda: MAP.astype(np.int16), "bool": lambda: MAP > 0, "uint16": lambda: (MAP + 1).astype(np.uint16),
         "float list": lambda: MAP.astype(np.float64).tolist()}[form]()
    seg, dt = arg(x)
    assert dt == lib.GSX_SEG_I32 and seg.dtype == np.int32 and np.array_equal(seg, np.asarray(x))
    assert arg(x, packed_u8=True)[1] == lib.GSX_SEG_I32


def test_nested_list_of_ints():
    """A nested list goes through np.asarray like every non-array: equal values, and the code of the dtype numpy gives it.
    That is numpy's default integer - int64 here, a supported dtype that is handed over as it is, as every entry point did
    before _seg_map_arg existed; int32 only where numpy's default integer is 32 bits wide."""
    x = MAP.tolist()
    seg, dt = arg(x)
    assert np.array_equal(seg, MAP) and seg.dtype == np.asarray(x).dtype
    assert dt == {4: lib.GSX_SEG_I32, 8: lib.GSX_SEG_I64}[seg.dtype.itemsize]


@pytest.mark.parametrize("dtype", [np.int32, np.int64, np.uint8, np.int16])
def test_fortran_order_and_slices_come_back_c_contiguous(dtype):
    f = np.asfortranarray((MAP + 1).astype(dtype))
    big = np.zeros((2 * H, 2 * W), dtype)
    big[::2, ::2] = MAP + 1
    for x in (f, big[::2, ::2]):
        assert x.shape == (H, W) and not x.flags.c_contiguous
        seg, dt = arg(x)
        assert seg is not x and np.array_equal(seg, MAP + 1) and dt == L._SEG_NP_DT.get(np.dtype(dtype), lib.GSX_SEG_I32)


def test_read_only_array_is_accepted():
    x = MAP.copy()
    x.flags.writeable = False
    seg, dt = arg(x)
    assert seg is x and dt == lib.GSX_SEG_I32


@pytest.mark.parametrize("shape", [(H * W,), (1, H, W)])
def test_not_two_dimensional(shape):
    for x in (MAP.reshape(shape), MAP.reshape(shape).astype(np.int16), MAP.reshape(shape).tolist()):
        with pytest.raises(ValueError, match="seg_map must be 2-D"):
            L._seg_map_arg(x, False)


def test_empty_map_passes_through():
    x = np.zeros((0, 0), np.int32)
    seg, dt, h, w, device = L._seg_map_arg(x, False)
    assert seg is x and dt == lib.GSX_SEG_I32 and (h, w) == (0, 0) and device is False
