"""The blend cases are what they claim (CPU, reference side only): the fp64 model of tests/blend_model.py against
oracle.render_scene, and the realised per-tile lists of every family of tests/blend_cases.py against its intent, before
test_blend_gpu.py holds the HIP kernels to the same model on the same scenes.

Sensitivity is asserted for every list position that puts a fragment on an in-frame pixel of its tile: a position of a
bounding-box list without one (a third of the needles' pairs, by design; at most a tenth in `edges`, asserted) changes nothing when it is removed - what such a pair
can break is the order and the slots of the others, and those are all sensitive."""
import math

import numpy as np
import pytest

import blend_cases
from blend_model import E4

NAMES = list(blend_cases.all_cases())


@pytest.mark.parametrize("name", NAMES)
def test_model_matches_oracle_outside_the_threshold_mask(name):
    p = blend_cases.prepared(name)
    m = p.model
    share = m.mask.mean()
    longest = max(len(m.sequence(t)) for t in range(len(m.lists)))
    print(f"{name}: ref_dist {p.ref_dist:.2e}, tol {p.tol:.2e}, masked share {share:.4%}, longest sequence {longest}")
    assert p.ref.shape == m.frame.shape and np.isfinite(m.frame).all()
    # fp32 against fp64: every blended record rounds four times to 2^-24 of a value <= 1
    assert 0.0 < p.ref_dist <= 4 * (longest + 8) * 2.0 ** -24
    assert share < 0.01
    if m.mask.any():                                   # there the two may decide `discard` differently: by one fragment at most
        assert p.diff[m.mask].max() <= p.alpha_max * E4 + p.ref_dist
    if blend_cases.bitwise(name):
        assert m.frame[..., 3].max() < 1 - 1e-3        # no tile comes near the opacity cut


@pytest.mark.parametrize("name", [n for n in NAMES if blend_cases.family(n) in ("lengths", "needles", "edges")])
def test_every_record_moves_a_pixel_by_ten_tolerances(name):
    p = blend_cases.prepared(name)
    m = p.model
    least, pairs, bare = np.inf, 0, 0
    for t in range(len(m.lists)):
        if len(m.lists[t]) == 0:
            continue
        effect, frag = m.leave_one_out(t), m.has_fragment(t)
        assert (effect[~frag] == 0).all()
        pairs += len(frag)
        bare += int((~frag).sum())
        if frag.any():
            least = min(least, float(effect[frag].min()))
    print(f"{name}: smallest leave-one-out effect {least:.2e} = {least / p.tol:.0f} x tol, {bare} of {pairs} pairs without a fragment")
    assert least >= 10 * p.tol
    if name == "lengths":
        assert bare == 0
    if name == "needles":
        assert bare >= 0.25 * pairs
    if blend_cases.family(name) == "edges":
        # axis ratios stay under 3: an ellipse fills pi/4 of its box, and a tile met by a corner of the box alone is the exception
        assert bare <= 0.1 * pairs


def test_lengths_lists_have_the_lengths_of_the_table():
    m = blend_cases.prepared("lengths").model
    assert tuple(len(l) for l in m.lists) == blend_cases.LENGTHS
    assert sorted(blend_cases.LENGTHS) == [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 319, 320, 321, 513]
    bin0 = sorted(blend_cases.LENGTHS[k] for k in (0, 1, 6, 7))          # the four tiles of one 32x32 bin
    assert bin0 == [0, 1, 257, 513]
    assert m.n_epilogue == 1


def test_needles_graze_corner_pixels():
    """some (tile, needle) pairs touch their tile only with fragments near the threshold (3 < q <= 4)"""
    m = blend_cases.prepared("needles").model
    grazing = 0
    for t in range(len(m.lists)):
        q, _, _ = m.tile_terms(t)
        inside = m.tile_pixels(t)[2]
        qmin = np.where(inside[None], q, np.inf).reshape(len(q), -1).min(1)[:len(m.lists[t])]
        grazing += int(((qmin > 3.0) & (qmin <= 4.0)).sum())
    assert grazing >= 5


@pytest.mark.parametrize("name", ["walls_80x48", "walls_65x53"])
def test_walls_lists_saturation_and_walk(name):
    p = blend_cases.prepared(name)
    m, meta = p.model, p.scene.meta
    walls = [int(p.packed[i]) for i in meta["walls"]]
    assert set(meta["m"].values()) >= set(blend_cases.WALL_M) and all(v % 16 <= 13 for v in meta["m"].values())
    if name == "walls_65x53":
        assert m.W % 16 == 1 and m.H % 16 == 5 and m.tiles_x * 16 > m.W and m.tiles_y * 16 > m.H
        assert meta["cut"] == [4, 9, 14, 19]
    else:
        assert meta["cut"] == []
    for t, (faint, discs, loud) in meta["tags"].items():
        ids = m.lists[t]
        mj = meta["m"][t]
        ids_of = lambda group: sorted(int(p.packed[i]) for i in group)
        inside = m.tile_pixels(t)[2]
        a = m.alpha_after(t)
        assert len(faint) == mj and sorted(ids[:mj]) == ids_of(faint)
        if t in meta["cut"]:
            # one pixel column in the frame: three needles close it, the loud records follow, the shared walls come last
            assert inside.sum() in (16, m.H % 16) and not inside[:, 1:].any()
            assert list(ids[mj:mj + 3]) == [int(p.packed[i]) for i in discs]
            assert sorted(ids[mj + 3:-3]) == ids_of(loud) and len(loud) == blend_cases.N_LOUD and list(ids[-3:]) == walls
            assert a[mj + 3][inside].min() > 1 - 1e-6 and a[mj][inside].max() < 1 - 1e-3
            assert a[len(ids) - 3][:, 4:].max() == 0.0                    # nothing before the walls reaches the tile's far columns:
            everywhere = np.ones_like(inside)                             # a vote that waits for them walks the whole list
            for group in (16, 256):
                assert m.consumed(t, group) == (min(len(ids), group * math.ceil((mj + 3) / group)), True)
                assert m.consumed(t, group, inside=everywhere) == (len(ids), True)
        elif t != meta["hole"]:
            assert list(ids[mj:mj + 3]) == walls
            assert sorted(ids[mj + 3:]) == ids_of(loud) and len(loud) == blend_cases.N_LOUD
            assert a[mj + 3][inside].min() > 1 - 1e-6                     # after the third wall
            assert a[mj][inside].max() < 1 - 1e-3                         # and far from it before the first
            for group in (16, 256):                                       # the kernels' distance between two votes
                assert m.consumed(t, group) == (min(len(ids), group * math.ceil((mj + 3) / group)), True)
        else:
            assert sorted(ids[mj:mj + 3]) == ids_of(discs)
            assert sorted(ids[mj + 3:mj + 3 + len(loud)]) == ids_of(loud) and list(ids[mj + 3 + len(loud):]) == walls
            corners = a[:, [0, 0, 15, 15], [0, 15, 0, 15]]
            assert corners[mj + 3].max() == 0.0                           # the discs miss the corner pixels,
            assert 0.5 < corners[mj + 3 + len(loud)].min() < 1 - 1e-4     # the loud records show there and do not close them
            for group in (16, 256):
                count, decided = m.consumed(t, group)
                assert decided and count == len(ids)                      # so the tile walks on to the shared walls


@pytest.mark.parametrize("name", ["epilogue_1", "epilogue_3", "epilogue_3_opaque"])
def test_epilogue_layout(name):
    p = blend_cases.prepared(name)
    m, meta = p.model, p.scene.meta
    assert p.packed[meta["zero"]] == 0 and m.rec.drawn[0] and m.n_epilogue == meta["k"]
    assert m.rec.color[0, 3] < 0.5                                        # splat 0 is not opaque
    tx0, tx1, ty0, ty1 = meta["rect"]
    x0, x1, r0, r1 = m.rec.box[0]
    assert (x0 // 16, x1 // 16, r0 // 16, r1 // 16) == (tx0, tx1, ty0, ty1)
    for t in range(len(m.lists)):
        ty, tx = divmod(t, m.tiles_x)
        assert (0 in m.lists[t]) == (tx0 <= tx <= tx1 and ty0 <= ty <= ty1)
    for t in meta["bare"]:
        assert list(m.lists[t]) == [0]                                    # inside the rectangle, no other record
    nvis = sum(1 for b in m.rec.box[m.walk[:m.rec.n - m.n_epilogue]] if b[1] >= b[0])
    front = set(int(i) for i in m.walk[:nvis // 6])                       # what precedes the last of two or three depth phases
    assert 0 in front
    for t in meta["closed"]:                                              # opaque before the last phase
        ids = m.lists[t]
        k = int(np.isin(ids, list(front)).sum())
        assert np.isin(ids[:k], list(front)).all()
        assert m.alpha_after(t)[k][m.tile_pixels(t)[2]].min() > 1 - 5e-6
    if not meta["opaque"]:
        assert meta["closed"] == ()
