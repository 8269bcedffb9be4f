"""The blend kernels (csrc/blend.hip: blend_kernel, blend2_kernel, blend4_kernel with and without BIN32) against the fp64 model
of tests/blend_model.py on the scenes of tests/blend_cases.py: list lengths on the vote distance, the chunks of 64 and 256 and
the 256-entry BIN32 fetch; bounding-box lists a third of whose pairs make no fragment; opaque walls in front of loud records;
frames whose border cuts the rows a lane owns; the dropped-splat epilogue.  test_blend_model.py shows on the CPU that the
scenes are what they claim and that removing ANY single record moves a pixel by at least ten tolerances.

Tolerance: tol = min(8 * ref_dist, 1e-5) per scene, ref_dist = max |oracle - model| outside the threshold mask (6.1e-8 .. 1.6e-6
over the scenes, recomputed here); scenes with opaque tiles get the kernels' documented cut of 1e-5 on top.  Every test prints
the distance per scene and option set, and the records evaluated against the derived count.

Measured on an MI355X, worst max |HIP - model| outside the mask over the nine option sets (0 threshold pixels flipped anywhere):
    lengths             4.11e-07 = 1.00 x ref_dist          edges (ten frames)   1.24e-07, at most 1.08 x ref_dist (47x47)
    needles             8.06e-08 = 0.79 x ref_dist          epilogue_1, _3       1.82e-07 = 0.99 x ref_dist
    walls_80x48         9.96e-07 = 0.95 x ref_dist (P, K1; 0.44 x with a vote every 16)
    walls_65x53         1.35e-06 = 0.85 x ref_dist (P, K1; 0.25 x with a vote every 16)
    epilogue_3_opaque   6.06e-06 = 11.9 x ref_dist (K2, B, X, D, D2: the cut of the closed tiles; 4.72e-07 = 0.93 x under P, K1, D3)
Where no tile turns opaque __expf costs nothing one can see: the kernels lie 0.79 .. 1.08 x ref_dist from the model, as far as the
oracle itself, and the factor 8 leaves a margin of 7.  The wall scenes stay within 0.07 x their tolerance, the cut costs 6e-6.
Kernel against kernel the frames are compared bit for bit wherever no tile reaches the opacity cut."""
import math

import numpy as np
import pytest

import blend_cases
from blend_model import E4

pytestmark = pytest.mark.gpu

P = {"blend_pk2": 0, "exact_cull": 0, "render_bin32": 0, "render_phases": 1, "tile_lpt": 0}
K2 = dict(P, blend_pk2=2)
OPTION_SETS = {
    "P": P,
    "K1": dict(P, blend_pk2=1),
    "K2": K2,
    "B0": dict(K2, render_bin32=1, render_wide_sort=0),
    "B1": dict(K2, render_bin32=1, render_wide_sort=1),
    "X": dict(K2, exact_cull=1),
    "D": {},
    "D2": {"render_phases": 2},
    "D3": {"render_phases": 3},
}
VOTE_EVERY = {"P": 256, "K1": 256, "K2": 16, "B0": 16, "B1": 16, "X": 16}     # records between two opacity votes, one depth phase
NAMES = list(blend_cases.all_cases())
N_BLIND = 50        # records per cut tile, at the least, that only a vote waiting for out-of-frame pixels would evaluate
_RENDERED = {}


def rendered(gsx, key):
    """every case under one option set, in a fresh context: name -> (frame, pairs binned, records evaluated)"""
    if key not in _RENDERED:
        out = {}
        with gsx.Context(0) as c:
            for k, v in OPTION_SETS[key].items():
                c.set_option(k, v)
            for name in NAMES:
                sc = blend_cases.prepared(name).scene
                c.upload_splats(*sc.arrays())
                frame = c.render_view(sc.cam, sc.W, sc.H)
                out[name] = (frame, c.render_num_pairs(), c.render_num_pairs_consumed())
        _RENDERED[key] = out
    return _RENDERED[key]


def has_opaque_tiles(name):
    return not blend_cases.bitwise(name)


@pytest.mark.parametrize("name", NAMES)
def test_every_kernel_and_option_against_the_model(gsx, name):
    p = blend_cases.prepared(name)
    m = p.model
    # The kernels' cut of 1e-5 comes on top wherever a tile turns opaque.  In epilogue_3_opaque that is under EVERY option set,
    # not only with two or three depth phases: the stacks close their tiles within one phase as well, and what the kernel then
    # leaves out (the faint records behind the stack, the epilogue's draws of splat 0) the model blends.  Measured: with one
    # phase and a vote every 16 records the scene lies 5.9e-6 from the model, above its plain tol of 4.1e-6.
    tol = p.tol + (1.0e-5 if has_opaque_tiles(name) else 0.0)
    masked = int(m.mask.sum())
    dist = {}
    for key in OPTION_SETS:
        frame = rendered(gsx, key)[name][0]
        assert frame.shape == m.frame.shape and np.isfinite(frame).all()
        dist[key] = d = np.abs(frame.astype(np.float64) - m.frame).max(axis=2)
        worst = float(d[~m.mask].max())
        print(f"{name} {key}: max |HIP - model| {worst:.2e} = {worst / p.ref_dist:.2f} x ref_dist (tol {tol:.2e}), "
              f"{int((d[m.mask] > tol).sum())} of {masked} threshold pixels flipped")
    for key, d in dist.items():
        assert d[~m.mask].max() <= tol, (key, float(d[~m.mask].max()), tol)
        if masked:                                                         # one fragment on the discard threshold, on any
            assert d[m.mask].max() <= p.alpha_max * E4 + tol, key          # number of the masked pixels


@pytest.mark.parametrize("name", [n for n in NAMES if blend_cases.bitwise(n)])
def test_kernels_and_options_agree_bit_for_bit(gsx, name):
    """blend.hip: "Per component the operation order is unchanged ... so `discard` decides exactly as before" - and the staging,
    the BIN32 fetch, exact culling, the launch defaults and the depth phases change which records a tile walks when, never a
    pixel, as long as no tile turns opaque."""
    p = blend_cases.prepared(name)
    assert p.model.frame[..., 3].max() < 1 - 1e-3
    base = rendered(gsx, "P")[name][0]
    for key in OPTION_SETS:
        frame = rendered(gsx, key)[name][0]
        if not np.array_equal(base, frame):
            r, x, ch = (int(v[0]) for v in np.nonzero(base != frame))
            t = (r // 16) * p.model.tiles_x + x // 16
            raise AssertionError(f"{name}: {key} differs from P on {int((base != frame).any(2).sum())} pixels, first at row {r} x {x} "
                                 f"channel {ch} (tile {t}, list of {len(p.model.lists[t])}): {frame[r, x]} against {base[r, x]}")


@pytest.mark.parametrize("name", ["walls_80x48", "walls_65x53"])
def test_walls_hide_what_is_behind_them_and_stop_the_walk(gsx, name):
    p = blend_cases.prepared(name)
    m, meta = p.model, p.scene.meta
    base = rendered(gsx, "P")[name][0].astype(np.float64)
    ys, xs, _ = m.tile_pixels(meta["hole"])
    cy, cx = ys[[0, 0, 15, 15], [0, 15, 0, 15]], xs[[0, 0, 15, 15], [0, 15, 0, 15]]
    assert m.frame[cy, cx, :3].max(axis=1).min() > 0.5                   # the hole's corners show the loud records
    for key in OPTION_SETS:
        frame, _, consumed = rendered(gsx, key)[name]
        assert np.abs(frame - base).max() <= 1e-5 + 1e-6, key
        assert np.abs(frame[cy, cx] - base[cy, cx]).max() <= p.tol and np.abs(frame[cy, cx] - m.frame[cy, cx]).max() <= p.tol, key
        if key in VOTE_EVERY:
            g = VOTE_EVERY[key]
            want = blind = 0
            for t, ids in enumerate(m.lists):
                if t == meta["hole"]:
                    count, decided = m.consumed(t, g)                    # walks on until the shared walls close its corners
                    assert decided
                    want += count
                else:
                    # also in the column of tiles the right border cuts to one pixel: three needles close that pixel column
                    # and touch no other, the loud records follow - a vote that waits for the fifteen columns outside the
                    # frame walks all of them, to the shared walls at the end of the list
                    want += min(len(ids), g * math.ceil((meta["m"][t] + 3) / g))
                    if t in meta["cut"]:
                        blind += len(ids) - m.consumed(t, g)[0]
            print(f"{name} {key}: {consumed} records evaluated, {want} derived, {sum(len(l) for l in m.lists)} in the lists"
                  + (f", {want + blind} for a vote that forgot the frame's border" if meta["cut"] else ""))
            assert blind >= N_BLIND * len(meta["cut"])
            assert consumed == want, key


def test_pairs_binned_are_the_models_lists(gsx):
    m = blend_cases.prepared("lengths").model
    assert rendered(gsx, "P")["lengths"][1] == sum(len(l) for l in m.lists) == sum(blend_cases.LENGTHS)
    # exact culling: a pair is kept iff q <= 4.04 somewhere on the rectangle of the tile's pixel centres (tile_test.hpp)
    m = blend_cases.prepared("needles").model
    got = rendered(gsx, "X")["needles"][1]
    lo = hi = exact = unsure = 0
    for t, ids in enumerate(m.lists):
        frag = m.has_fragment(t)
        for k, i in enumerate(ids):
            x0, x1, r0, r1 = m.rec.box[i]
            one_tile = x0 // 16 == x1 // 16 and r0 // 16 == r1 // 16      # a one-tile rectangle is not tested
            q = 0.0 if one_tile else m.rect_min_q(t, i)
            lo += bool(frag[k])
            hi += q <= 4.1
            exact += q <= 4.04
            unsure += abs(q - 4.04) < 1e-3
    print(f"needles, exact culling: {got} pairs binned; model: {exact} with q <= 4.04 ({unsure} within 1e-3 of it), {lo} with a fragment, "
          f"{hi} with q <= 4.1, {sum(len(l) for l in m.lists)} in the bounding boxes")
    assert lo <= got <= hi
    if unsure == 0:
        assert got == exact
