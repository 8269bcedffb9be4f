"""GPU: the viewer's label edits (gsx_render_set_edits / Context.set_render_edits) against the frames the reference's own
shaders and worker produce under the same edit states (tests/golden/render_gl_edits.npz), and their invariants."""
import os

import numpy as np
import pytest

import oracle
import render_edits_ref as ref
from conftest import GOLDEN, check_against_gl_frame, gl_golden_calls

pytestmark = pytest.mark.gpu

CALLS = ref.fixture_calls(os.path.join(GOLDEN, "render_gl_edits.npz"))


@pytest.fixture(autouse=True)
def no_edits_left_behind(ctx):
    yield
    ctx.clear_render_edits()
    ctx.set_option("render_frames", 4)


def upload(ctx, call):
    ctx.upload_splats(*call["attrs"], labels=call["labels"])


def labelled_scene(gsx, n, seed, n_labels=6):
    scene = gsx.scene
    xyz = scene.make_positions(n, seed)
    a = scene.make_splat_attributes(n, seed, sh_degree=0)
    a["scale"] += np.float32(0.5)
    labels = (np.arange(n) % n_labels).astype(np.int32)
    return [xyz, a["scale"], a["rot"], a["opacity"], a["f_dc"]], labels


@pytest.mark.parametrize("call", CALLS, ids=lambda c: c["id"])
def test_every_fixture_frame_render_view(ctx, call):
    upload(ctx, call)
    ctx.set_render_edits(**call["state"])
    img = ctx.render_view(call["cam"], call["W"], call["H"])
    worst, over = check_against_gl_frame(img, call["frame"], f"{call['id']} ({call['note']})")
    print(f"{call['id']}: max |HIP - GL| {worst:.3e}, {over} threshold pixel(s); composition applies: {call['applies']}")


@pytest.mark.parametrize("call", CALLS, ids=lambda c: c["id"])
def test_every_fixture_frame_render_views_four_in_flight(ctx, call):
    """the multi-frame pre pass (pre_multi_kernel's edit instantiation) and the twin contexts see the state"""
    others = [c["cam"] for c in CALLS if c["scene"] == call["scene"] and c["W"] == call["W"]][:3]
    cams = [call["cam"]] + others + [call["cam"]] * 2          # six views, four in flight: two groups
    upload(ctx, call)
    ctx.set_render_edits(**call["state"])
    ctx.set_option("render_frames", 4)
    imgs = ctx.render_views(cams, call["W"], call["H"])
    for k in (0, len(cams) - 2, len(cams) - 1):
        check_against_gl_frame(imgs[k], call["frame"], f"{call['id']} view {k} of render_views")
    one = [ctx.render_view(c, call["W"], call["H"]) for c in cams[:4]]
    for k in range(4):
        assert np.array_equal(imgs[k], one[k]), f"render_views differs from render_view under edits (view {k})"


def test_cleared_and_never_set_are_bit_identical(gsx, ctx):
    calls = [c for c in gl_golden_calls() if c[0].startswith("render_gl_scenes")]
    _, xyz, scale, rot, opacity, f_dc, cam, W, H, frame = calls[0]
    labels = (np.arange(len(xyz)) % 7).astype(np.int32)
    with gsx.Context(0) as fresh:                              # a context that never had an edit state
        fresh.upload_splats(xyz, scale, rot, opacity, f_dc, labels=labels)
        never = fresh.render_view(cam, W, H)
        never4 = fresh.render_views([cam] * 4, W, H)
    ctx.upload_splats(xyz, scale, rot, opacity, f_dc, labels=labels)
    ctx.set_render_edits(selected=3, selection_mode=True, colours={1: (0, 1, 0)}, displacements={2: (1, 0, 0)}, hidden=(4,))
    assert ctx.render_num_hidden() == int((labels == 4).sum())
    edited = ctx.render_view(cam, W, H)
    assert not np.array_equal(edited, never)
    ctx.clear_render_edits()
    assert ctx.render_num_hidden() == 0
    assert np.array_equal(ctx.render_view(cam, W, H), never)
    assert np.array_equal(ctx.render_views([cam] * 4, W, H), never4)
    check_against_gl_frame(never, frame, "unedited frame")
    # a state that edits nothing runs the edit instantiation and still gives the same pixels
    ctx.set_render_edits(selected=3, selection_mode=False, colours={1234: (0, 1, 0)}, hidden=(99,))
    assert np.array_equal(ctx.render_view(cam, W, H), never)


def test_zero_displacement_is_bit_identical_to_none(gsx, ctx):
    attrs, labels = labelled_scene(gsx, 5000, 0xED17A1)
    W, H = 320, 180
    cams = gsx.scene.make_cameras(4, W, H, convention="c2w")
    ctx.upload_splats(*attrs, labels=labels)
    plain = ctx.render_views(cams, W, H)
    ctx.set_render_edits(displacements={2: (0.0, 0.0, 0.0), 3: (0.0, -0.0, 0.0)})
    assert np.array_equal(ctx.render_views(cams, W, H), plain)
    assert np.array_equal(ctx.render_view(cams[1], W, H), plain[1])


def test_hiding(gsx, ctx):
    attrs, labels = labelled_scene(gsx, 5000, 0xED17A2)
    W, H = 320, 180
    cam = gsx.scene.make_cameras(3, W, H, convention="c2w")[1]
    ctx.upload_splats(*attrs, labels=labels)
    plain = ctx.render_view(cam, W, H)
    pairs_plain = ctx.render_num_pairs()
    assert plain[..., 3].max() > 0.5
    ctx.set_render_edits(hidden=(1, 4))
    assert ctx.render_num_hidden() == int(np.isin(labels, (1, 4)).sum())
    some = ctx.render_view(cam, W, H)
    # hidden splats keep their rectangle (alpha 0): no pair more than without the edit - as long as no tile of
    # the unedited frame turns opaque before the last depth phase, as here; at 3 M splats the tiles behind hidden splats turn
    # opaque later and the later phase bins 0.4 % MORE pairs (profiles/render_edits_cost.json)
    assert ctx.render_num_pairs() <= pairs_plain
    want, applies = ref.compose(*attrs, labels, cam, W, H, ref.state(hidden=(1, 4)))
    assert applies
    check_against_gl_frame(some, want, "two labels hidden, against the composition of oracle pieces")
    ctx.set_render_edits(hidden=range(6))                      # every label: nothing is left to see
    assert ctx.render_num_hidden() == len(labels)
    assert (ctx.render_view(cam, W, H) == 0).all()
    assert (ctx.render_views([cam] * 4, W, H) == 0).all()
    ctx.set_render_edits(hidden=(ref.NO_SELECTION,))           # the worker ignores NO_SELECTION (gs.js:619)
    ctx.upload_splats(*attrs)                                  # no labels: every splat carries NO_SELECTION
    ctx.set_render_edits(hidden=(ref.NO_SELECTION,))
    assert ctx.render_num_hidden() == 0
    assert np.array_equal(ctx.render_view(cam, W, H), plain)


def test_highlight_closed_form(gsx, ctx):
    """every splat selected: rgb' = 0.5 rgb + 0.5 (1, 0, 0) alpha per pixel (the under-operator sum is linear in the colours)"""
    attrs, _ = labelled_scene(gsx, 5000, 0xED17A3)
    labels = np.full(5000, 17, np.int32)
    W, H = 320, 180
    cam = gsx.scene.make_cameras(3, W, H, convention="c2w")[0]
    ctx.upload_splats(*attrs, labels=labels)
    plain = ctx.render_view(cam, W, H).astype(np.float64)
    ctx.set_render_edits(selected=17, selection_mode=True)
    lit = ctx.render_view(cam, W, H).astype(np.float64)
    want = 0.5 * plain
    want[..., 0] += 0.5 * plain[..., 3]
    want[..., 3] = plain[..., 3]
    d = np.abs(lit - want).max()
    print(f"highlight closed form: max deviation {d:.3e}")
    assert d <= 1e-5


def test_hit_test_ignores_every_edit(gsx, ctx):
    call = CALLS[7]                                            # "all at once"
    upload(ctx, call)
    rng = np.random.default_rng(5)
    clicks = [(float(x), float(y)) for x, y in zip(rng.uniform(0, call["W"], 40), rng.uniform(0, call["H"], 40))]
    before = [ctx.hit_test(call["cam"], call["W"], call["H"], x, y) for x, y in clicks]
    assert len({b[0] for b in before}) > 2
    ctx.set_render_edits(**call["state"])
    assert [ctx.hit_test(call["cam"], call["W"], call["H"], x, y) for x, y in clicks] == before


def test_error_paths_and_state_lifetime(gsx, ctx):
    attrs, labels = labelled_scene(gsx, 2000, 0xED17A4)
    W, H = 160, 96
    cam = gsx.scene.make_cameras(3, W, H, convention="c2w")[2]
    with gsx.Context(0) as fresh:
        with pytest.raises(gsx.GsxError) as e:
            fresh.set_render_edits(selected=1, selection_mode=True)
        assert e.value.code == gsx._lib.GSX_E_STATE
        fresh.clear_render_edits()                             # clearing nothing is not an error
    ctx.upload_splats(*attrs, labels=labels)
    plain = ctx.render_view(cam, W, H)
    ctx.set_render_edits(colours={k: (1, 0, 0) for k in range(100)}, displacements={k: (0, 1, 0) for k in range(100)})
    with pytest.raises(ValueError):
        ctx.set_render_edits(colours={k: (1, 0, 0) for k in range(101)})
    with pytest.raises(ValueError):
        ctx.set_render_edits(displacements={k: (1, 0, 0) for k in range(101)})
    with pytest.raises(ValueError):
        ctx.set_render_edits(colours={1: (float("nan"), 0, 0)})
    with pytest.raises(ValueError):
        ctx.set_render_edits(displacements={1: (0, float("inf"), 0)})
    with pytest.raises(ValueError):
        ctx.set_render_edits(selected=1, custom_colour=(0, 0, float("nan")))
    e = gsx._lib.RenderEdits()
    e.num_hidden = 3                                           # a count without an array
    assert gsx.lib().gsx_render_set_edits(ctx.h, __import__("ctypes").byref(e)) == gsx._lib.GSX_E_INVALID
    # a rejected call leaves the previous state (100 + 100 entries) in force
    ctx.set_render_edits(hidden=(2,))
    hidden = ctx.render_view(cam, W, H)
    assert not np.array_equal(hidden, plain)
    with pytest.raises(ValueError):
        ctx.set_render_edits(colours={1: (float("nan"), 0, 0)})
    assert np.array_equal(ctx.render_view(cam, W, H), hidden)
    # ... and the next upload_splats clears it: the codes belonged to the old labels
    ctx.upload_splats(*attrs, labels=labels)
    assert ctx.render_num_hidden() == 0
    assert np.array_equal(ctx.render_view(cam, W, H), plain)


def test_sh_colour_is_edited_on_top(gsx, ctx):
    """unpinned by the reference (it has no SH colour): vColor.rgb = fade * clamp(0.5 + SH), edited in the same order"""
    n, W, H = 3000, 160, 96
    xyz = gsx.scene.make_positions(n, 0xED17A5)
    a = gsx.scene.make_splat_attributes(n, 0xED17A5, sh_degree=2)
    a["scale"] += np.float32(0.5)
    labels = (np.arange(n) % 4).astype(np.int32)
    cam = gsx.scene.make_cameras(3, W, H, convention="c2w")[1]
    st = ref.state(selected=2, selection_mode=True, colours={1: (0.1, 0.9, 0.3), 2: (0.5, 0.5, 1.0)}, hidden=(3,))
    ctx.upload_splats(xyz, a["scale"], a["rot"], a["opacity"], a["f_dc"], labels=labels)
    ctx.upload_sh(a["f_rest"], 2)
    ctx.set_render_edits(**st)
    img = ctx.render_view(cam, W, H)
    buf, order = oracle.pack_splats(xyz, a["scale"], a["rot"], a["opacity"], a["f_dc"])
    lab = labels[order]
    tex = oracle.texture(buf, lab).reshape(n, 8).copy()
    tex[lab == 3, 7] &= np.uint32(0x00ffffff)
    di, _ = oracle.depth_order(buf, oracle.multiply4(oracle.proj_matrix(cam["fx"], cam["fy"], W, H), oracle.view_matrix(cam)))
    col = oracle.sh_colors(xyz[order], a["f_dc"][order], a["f_rest"][order], 2, cam["position"])
    col[:, :3], _ = ref.edited_colours(col[:, :3], ref.shader_labels(lab), st)
    want = oracle.render_view(tex.reshape(-1), di, cam, W, H, override_color=col)   # (outside camera: every fade is 1)
    check_against_gl_frame(img, want, "SH colour + edits against the oracle's SH path")


def test_mid_size_scene_four_streams_busy(gsx, ctx):
    """200 k splats at 1080p, labels from the vote; three classes hidden, two recoloured, one moved; against the composition of
    oracle pieces on cameras where every fade is 1, under the rule of check_against_gl_frame."""
    n, V, W, H = 200_000, 6, 1920, 1080
    pos, vcams, segs = gsx.scene.make_scene(n, V, 320, 180, config_id=1, convention="w2c")
    labels = gsx.assign_labels_from_maps(pos, vcams, segs, [(320, 180)] * V, n_classes=150, ctx=ctx)
    top = [int(l) for l in np.argsort(-np.bincount(labels[labels >= 0], minlength=150))[:6]]
    a = gsx.scene.make_splat_attributes(n, 0xED17A6, sh_degree=0)
    attrs = [pos, a["scale"], a["rot"], a["opacity"], a["f_dc"]]
    st = ref.state(colours={top[3]: (0.0, 1.0, 0.0), top[4]: (1.0, 0.0, 1.0)}, displacements={top[5]: (0.5, 0.25, -0.5)},
                   hidden=top[:3])
    cams = gsx.scene.make_cameras(4, W, H, radius=14.0, convention="c2w")
    ctx.upload_splats(*attrs, labels=labels)
    ctx.set_render_edits(**st)
    assert ctx.render_num_hidden() == int(np.isin(labels, top[:3]).sum()) > 0
    imgs = ctx.render_views(cams, W, H)
    for k in (0, 3):
        want, applies = ref.compose(*attrs, labels, cams[k], W, H, st)
        assert applies
        worst, over = check_against_gl_frame(imgs[k], want, f"mid-size scene, view {k}")
        print(f"mid-size view {k}: max |HIP - composition| {worst:.3e}, {over} threshold pixel(s)")
    for k in range(4):
        assert np.array_equal(ctx.render_view(cams[k], W, H), imgs[k])
