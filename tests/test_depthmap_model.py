"""The depth frames' fp64 model (tests/depthmap_model.py) and the host-only part of the interface, CPU only, before
test_depthmap_gpu.py holds the HIP kernel against them.

gsx_depth_key_to_z: for random cameras and float32 points, key * scale + offset lies within one key unit (= scale) of the fp64
view-space z the viewer's getViewMatrix gives; the key is stated as gs.js:437 states it, in numpy.

The model's own transpose identity: sum over the pixels of moment == sum over the records of key * (the record's row of
lift_model's table), to 1e-12 relative - the two models scatter the same weights, one by pixel, one by record.

The margins the GPU tests lean on, asserted here so that a changed scene cannot hollow them out:
- surfaces against the model are compared at DECIDED pixels only; on walls_80x48, walls_65x53 and epilogue_3_opaque at quantile
  0.5 the undecided ones are at most 5 % of the pixels with a surface;
- the chunk-border scenes: the list has exactly L records, what stands in front of the opaque splat sums to <= 0.2 per pixel,
  the opaque splat's own B is >= 0.9 on every pixel, and the model's surface is that splat;
- walls_80x48 under the tags' labels: no decided pixel of an ordinary tile has a loud surface, each corner of the hole tile has
  a decided pixel whose surface is loud, and at least five ordinary tiles have a loud record whose centre lies on a decided
  pixel that shows a wall."""
import numpy as np
import pytest

import blend_cases
import depthmap_model
import lift_model
from lift_model import ONE

NAMES = list(blend_cases.all_cases())
DECIDED_CASES = ("walls_80x48", "walls_65x53", "epilogue_3_opaque")


def random_camera(rng, W, H):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    a, b, c, d = q
    R = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                  [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                  [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])
    return {"fx": float(rng.uniform(0.5, 2.0) * W), "fy": float(rng.uniform(0.5, 2.0) * H), "width": W, "height": H,
            "rotation": R.tolist(), "position": rng.uniform(-5, 5, 3).tolist()}


def test_key_to_z_against_the_viewers_view_matrix(gsx):
    import oracle
    rng = np.random.default_rng(20291)
    for W, H in ((96, 48), (1920, 1080), (1, 1), (4096, 7)):
        cam = random_camera(rng, W, H)
        scale, offset = gsx.depth_key_to_z(cam, W, H)
        view = oracle.view_matrix(cam)
        vp = oracle.multiply4(oracle.proj_matrix(cam["fx"], cam["fy"], W, H), view)
        pts = rng.uniform(-40, 40, (4000, 3)).astype(np.float32).astype(np.float64)
        key = np.trunc((vp[2] * pts[:, 0] + vp[6] * pts[:, 1] + vp[10] * pts[:, 2]) * 4096.0)          # gs.js:437, `| 0`
        assert np.abs(key).max() < 2.0 ** 31
        z = view[2] * pts[:, 0] + view[6] * pts[:, 1] + view[10] * pts[:, 2] + view[14]               # getViewMatrix, row 2
        err = np.abs(key * scale + offset - z)
        assert scale > 0 and (err <= scale).all(), (W, H, float(err.max() / scale))
        assert (err > 0.25 * scale).any()                                 # ... and the unit is the key's, not a coarser one
    GsxError = gsx._lib.GsxError
    for bad in ((0, 5), (5, 0), (-1, -1)):
        with pytest.raises((ValueError, GsxError)):
            gsx.depth_key_to_z(cam, *bad)


def test_constants(gsx):
    k, l = gsx.depth_constants(), gsx.lift_constants()
    assert k == {"one": ONE, "shift": 20, "tile": 16, "chunk": 256} and all(k[n] == l[n] for n in k)
    assert [depthmap_model.cut_of(q) for q in (2.0 ** -21, 2.0 ** -20, 0.5, 0.5 + 2.0 ** -21, 1.0)] == [1, 1, ONE // 2, ONE // 2 + 1, ONE]


def test_keys_are_affine_in_depth(gsx):
    p = blend_cases.prepared("needles")
    key = depthmap_model.keys(p.scene, p.model)
    scale, offset = gsx.depth_key_to_z(p.scene.cam, p.scene.W, p.scene.H)
    z = p.scene.arrays()[0][np.asarray(p.model.rec.order), 2].astype(np.float64)                      # the identity camera: z_view = z
    assert (np.abs(key * scale + offset - z) <= scale).all() and key.min() > 0 and len(np.unique(key)) > 200


@pytest.mark.parametrize("name", NAMES)
def test_transpose_identity_of_the_two_models(name):
    p = blend_cases.prepared(name)
    m = p.model
    key = depthmap_model.keys(p.scene, m)
    d = depthmap_model.case_frame(name)
    seg, C = lift_model.maps(m.W, m.H)["uniform"]
    rows = lift_model.lift(m, seg, C).table.sum(1)
    left, right = float(d.moment.sum()), float((key * rows).sum())
    assert right > 0 and abs(left - right) <= 1e-12 * abs(right), (left, right)
    assert abs(d.total.sum() - rows.sum()) <= 1e-12 * rows.sum()
    assert ((d.total == 0) == (d.P == 0)).all() and (d.index[d.total < 0.5] == -1).all() and (d.index[d.total > 0.5 + 1e-9] >= 0).all()


@pytest.mark.parametrize("name", DECIDED_CASES)
def test_undecided_pixels_are_few(name):
    d = depthmap_model.case_frame(name)
    surf = d.index >= 0
    undecided = int((surf & ~d.decided).sum())
    print(f"{name}: {undecided} undecided of {int(surf.sum())} pixels with a surface ({undecided / surf.sum():.1%})")
    assert surf.sum() > 1000 and undecided <= 0.05 * surf.sum()
    assert (d.decided & surf).sum() > 1000


@pytest.mark.parametrize("L", depthmap_model.BORDER_L)
def test_chunk_border_scenes(L):
    b, m = depthmap_model.border(L), depthmap_model.border_model(L)
    assert len(m.lists) == 1 and len(m.lists[0]) == L and m.n_epilogue == 1
    opaque = int(np.argsort(m.rec.order)[b.opaque])                       # its importance row
    assert m.lists[0][-1] == opaque
    _, B, _ = m.tile_terms(0)
    assert (B[L - 1] >= 0.9).all()
    d = depthmap_model.frame(m, depthmap_model.keys(b.scene, m), 0.5, 1e-5, 1.0, False)
    assert d.faint.max() <= 0.2 and (L == 1 or d.faint.max() > 0.0)
    assert (d.index == opaque).all() and d.decided.all()


def test_walls_the_surface_is_the_wall_not_what_stands_behind_it():
    p = blend_cases.prepared("walls_80x48")
    sc, m = p.scene, p.model
    labels = depthmap_model.wall_labels(sc)
    assert sorted(np.unique(labels)) == [-1, 0, 1, 2, 3] and (labels == -1).sum() == 1
    d = depthmap_model.case_frame("walls_80x48")
    lab = np.where(d.index >= 0, labels[np.asarray(m.rec.order)[np.maximum(d.index, 0)]], -999999)
    hole = sc.meta["hole"]
    ys, xs, _ = m.tile_pixels(hole)
    in_hole = np.zeros((m.H, m.W), bool)
    in_hole[ys, xs] = True
    assert not ((lab == 2) & d.decided & ~in_hole).any()
    assert ((lab == 3) & d.decided & ~in_hole).sum() > 3000
    loud = (lab == 2) & d.decided & in_hole
    y0, x0 = ys.min(), xs.min()
    for cy in (slice(y0, y0 + 3), slice(y0 + 13, y0 + 16)):
        for cx in (slice(x0, x0 + 3), slice(x0 + 13, x0 + 16)):
            assert loud[cy, cx].any()
    # loud records behind the walls whose centre lies on a decided pixel: in at least five ordinary tiles (where many faint
    # records share the tile's centre with them, their sum comes near the cut and the centre pixels are undecided)
    assert len(depthmap_model.behind_the_walls(sc, d, np.asarray(m.rec.order))) >= 5


def test_the_integer_rule():
    q = np.array([[0, 3], [5, 0], [0, 0], [7, 2]])
    key, row = [10, -20, 30, 40], [4, 9, 1, 6]
    for cut, want_key, want_row in ((1, (-20, 10), (9, 4)), (5, (-20, 40), (9, 6)), (6, (40, 0), (6, -1)), (12, (40, 0), (6, -1)),
                                    (13, (0, 0), (-1, -1))):
        total, moment, skey, srow = depthmap_model.rule(q, key, row, cut / ONE)
        assert depthmap_model.cut_of(cut / ONE) == cut
        assert list(total) == [12, 5] and list(moment) == [180, 110] and tuple(skey) == want_key and tuple(srow) == want_row, cut
