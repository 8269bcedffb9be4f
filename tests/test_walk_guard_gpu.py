"""The one front of the walked frames (csrc/render.hip: frame_walk_guard) through its three entries - lift_view after lift_begin,
label_view, depth_view - on the edges_17x17 scene of tests/blend_cases.py (two tiles per side, both cut by the frame): an edit
state, a frame over 4096 pixels per side and an empty frame are refused by each with the same code and the same words, nothing
is left behind by a refused call, and the next good view returns the bits of the first."""
import numpy as np
import pytest

import blend_cases
import lift_model

pytestmark = pytest.mark.gpu

C = 4


def lift(c, sc, W, H):
    seg = lift_model.maps(sc.W, sc.H)["blocks"][0] if (W, H) == (sc.W, sc.H) else np.zeros((H, W), np.int32)
    c.lift_begin(C)
    c.lift_view(sc.cam, seg, image_size=(sc.W, sc.H))
    return (c.lift_table(),)


def label(c, sc, W, H):
    return c.label_view(sc.cam, W, H, C, return_weights=True)


def depth(c, sc, W, H):
    f = c.depth_view(sc.cam, W, H, 0.5)
    return f.total, f.moment, f.surface_key, f.surface_index


@pytest.mark.parametrize("entry", (lift, label, depth))
def test_guard(gsx, entry):
    lib = gsx._lib
    sc = blend_cases.all_cases()["edges_17x17"]()
    assert (sc.W, sc.H) == (17, 17) and lift_model.maps(sc.W, sc.H)["blocks"][1] <= C
    view = lambda W=sc.W, H=sc.H: entry(c, sc, W, H)
    same = lambda got: all(np.array_equal(g, w) for g, w in zip(got, good))
    with gsx.Context(0) as c:
        c.upload_splats(*sc.arrays(), labels=np.arange(len(sc.xyz), dtype=np.int32) % C)
        good = view()
        assert len(good) >= 1 and any(g.any() for g in good)
        c.set_render_edits(hidden=[0])                                   # an edit state
        with pytest.raises(lib.GsxError, match="edit state") as e:
            view()
        assert e.value.code == lib.GSX_E_STATE
        c.clear_render_edits()
        assert same(view())
        for W, H in ((4097, 16), (16, 4097)):                            # over 4096 pixels per side: before anything is allocated
            with pytest.raises(lib.GsxError, match=f"{W}x{H}") as e:
                view(W, H)
            assert e.value.code == lib.GSX_E_UNSUPPORTED
        assert same(view())
        for W, H in ((0, sc.H), (sc.W, 0)):                              # an empty frame
            with pytest.raises(ValueError, match=f"libgsx error {lib.GSX_E_INVALID}:"):
                view(W, H)
        assert same(view())
