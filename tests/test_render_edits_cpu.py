"""CPU: the viewer's label edits (gsx_render_set_edits) - the fixture of the reference's own shaders under edit states is
consistent with the semantics include/gsx.h states, and the library and the Python front end carry the entry points."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import render_edits_ref as ref
from conftest import GOLDEN, check_against_gl_frame, load_pkg

CALLS = ref.fixture_calls(os.path.join(GOLDEN, "render_gl_edits.npz"))


def test_fixture_covers_the_edit_states():
    notes = " | ".join(c["note"] for c in CALLS)
    for what in ("highlight only", "table colours for several labels", "u_customColor + highlight", "one displacement",
                 "across the 1.2 w cull", "behind the camera", "packed row 0", "farthest splat", "all at once", "label -1 selected",
                 "-999999 selected", "selection_mode off", "hidden and coloured at once", "non-finite attributes", "2^24 + 1"):
        assert what in notes, what
    assert sum(not c["applies"] for c in CALLS) >= 2          # frames with colour-edited splats at fade < 1: GPU tests only
    assert all(np.isfinite(c["frame"]).all() for c in CALLS)
    assert os.path.getsize(os.path.join(GOLDEN, "render_gl_edits.npz")) < (1 << 20)


@pytest.mark.parametrize("call", [c for c in CALLS if c["applies"]], ids=lambda c: c["id"])
def test_composition_of_oracle_pieces_matches_the_reference_shaders(call):
    """(a) texture words edited as the worker / vertex shader do, depth order of the UNEDITED buffer, colours as the fragment
    shader: the unchanged oracle reproduces the GL frame wherever override_color's fade does not matter."""
    img, applies = ref.compose(*call["attrs"], call["labels"], call["cam"], call["W"], call["H"], call["state"])
    assert applies
    worst, over = check_against_gl_frame(img, call["frame"], f"{call['id']} ({call['note']})")
    print(f"{call['id']}: max |composition - GL| {worst:.3e}, {over} threshold pixel(s)")


def test_selection_mode_off_changes_nothing():
    """uSelectedLabel without uSelectionMode or u_enableCustomColor: the frame of the unedited scene."""
    call = next(c for c in CALLS if "selection_mode off" in c["note"])
    import oracle
    plain = oracle.render_scene(*call["attrs"], call["cam"], call["W"], call["H"], labels=call["labels"])
    check_against_gl_frame(plain, call["frame"], call["id"])


def test_library_and_front_end_carry_the_entry_points():
    """(b) libgsx.so exports gsx_render_set_edits, Context.set_render_edits has the documented signature."""
    g = load_pkg()
    g.build()
    lib = ctypes.CDLL(g._lib.SO_PATH)
    assert hasattr(lib, "gsx_render_set_edits") and hasattr(lib, "gsx_render_num_hidden")
    sig = inspect.signature(g.Context.set_render_edits)
    assert list(sig.parameters) == ["self", "selected", "selection_mode", "colours", "custom_colour", "displacements", "hidden"]
    assert sig.parameters["selected"].default is None and sig.parameters["selection_mode"].default is False
    assert sig.parameters["hidden"].default == ()
    assert callable(g.Context.clear_render_edits)
    # the ctypes mirror of gsx_render_edits: 4-byte fields, the tables of 100, then the i64 count and the pointer
    e = g._lib.RenderEdits
    assert e.num_colors.offset == 24 and e.color_labels.offset == 28 and e.colors.offset == 428
    assert e.enable_displacement.offset == 1628 and e.displacements.offset == 2036
    assert e.num_hidden.offset == 3240 and e.hidden_labels.offset == 3248 and ctypes.sizeof(e) == 3256


def test_null_context_is_an_error_not_a_crash():
    g = load_pkg()
    lib = g.lib()
    assert lib.gsx_render_set_edits(None, None) != 0
    assert lib.gsx_render_num_hidden(None) == 0
