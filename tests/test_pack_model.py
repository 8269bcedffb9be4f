"""CPU: the scenes and hit cases of tests/pack_cases.py against the oracle.  The builders' rules hold (no NaN importance, at
most 0.1 % of the random values redrawn under the +-8-ulp rule, every placed row robust, the oracle's order == the stable
descending argsort); the value-edge scene reaches the edges it names; floatToHalf written with Python ints from gs.js:248-275
equals the oracle's; the oracle's hit test gives the answers written by hand in the cases.  tests/test_pack_gpu.py then holds
the kernels to the same expectations."""
import numpy as np
import pytest

import oracle
import pack_cases as pc

PACK = pc.all_pack_scenes()


def halves_of(tex):
    """(n, 6) the six half-floats of each texture row"""
    w = np.asarray(tex).reshape(-1, 8)[:, 4:7]
    return np.stack([w[:, 0] & 0xFFFF, w[:, 0] >> 16, w[:, 1] & 0xFFFF, w[:, 1] >> 16, w[:, 2] & 0xFFFF, w[:, 2] >> 16], axis=1)


@pytest.mark.parametrize("name", list(PACK))
def test_builder_rules_hold(name):
    s = PACK[name]()
    s.check_rules()
    buf, order, tex, lab = s.expect()            # asserts order == argsort(-importance, stable) for the oracle
    assert buf.shape == (s.n, 32) and tex.shape == (8 * s.n,) and sorted(order.tolist()) == list(range(s.n))
    print(f"{name}: {s.redrawn} of {s.random_values} random exp arguments redrawn (cap {pc.REDRAW_CAP * s.random_values:.1f})")


@pytest.mark.parametrize("degree,n", pc.SH_CASES)
def test_sh_scene_rules_and_planes(degree, n):
    s = pc.sh_scene(degree, n)
    _, order, _, _ = s.expect()
    K = (degree + 1) ** 2
    planes = pc.sh_planes(s.f_dc, s.f_rest, order, degree)
    assert planes.shape == (K, 3, n) and planes.dtype == np.float32
    k, c, j = np.meshgrid(np.arange(K), np.arange(3), np.arange(n), indexing="ij")
    assert np.array_equal(planes, (64 * order[j].astype(np.int64) + 4 * k + c).astype(np.float32))     # every float names its (r, k, c)
    if n > 1:
        assert not np.array_equal(order, np.arange(n))


def test_size_scenes_have_ties_across_blocks_and_tiles():
    for n in pc.SIZES:
        s = pc.size_scene(n)
        _, order, _, _ = s.expect()
        imp = pc.importance(s.scale, s.opacity)[order]
        run = np.nonzero(imp[1:] == imp[:-1])[0]
        if n >= 2:
            assert len(run) + 1 >= n // 4 >= 0 and len(run) >= 1, n
        if n >= 64:
            assert np.isinf(imp[:5]).all() and (imp[-5:] == 0).all()           # +Infinity first, +0 last, five of each
            assert (np.diff(order[:5].astype(np.int64)) > 0).all() and (np.diff(order[-5:].astype(np.int64)) > 0).all()
        if n > 4097:
            src = np.sort(order[run].astype(np.int64))
            assert src[0] < 4096 and src[-1] >= n - 4096                       # tie rows in the first and the last sort tile


def test_value_edge_scene_reaches_its_edges():
    s = pc.value_edge_scene()
    buf, order, tex, lab = s.expect()
    where = np.empty(s.n, np.int64)
    where[order] = np.arange(s.n)                                              # source row -> packed row
    row = lambda name: int(where[s.rows[name]])
    scales = buf[:, 12:24].copy().view(np.float32)
    imp = pc.importance(s.scale, s.opacity)
    tiny = pc.F32_MIN_NORMAL
    # ties: both runs are contiguous in packed order and keep their source order; the long one crosses a 256 boundary
    for rows in (s.run, s.ones):
        j = where[rows]
        assert np.array_equal(j, np.arange(j[0], j[0] + len(rows)))
    j = where[s.run]
    assert j[0] // 256 != j[-1] // 256 and len(s.run) == 300
    assert (imp[s.ones] == 1.0).all() and len(s.ones) == 20
    # importance extremes
    zeros = [s.rows[f"imp_zero_{i}"] for i in range(4)] + [s.rows["opacity_-800"]]
    nz = int((imp == 0).sum())
    assert (imp[zeros] == 0).all() and nz >= 5
    assert np.array_equal(order[s.n - nz:], np.nonzero(imp == 0)[0])            # the +0 tie at the far end, in source order
    assert 0 < imp[s.rows["opacity_-104"]] < tiny or imp[s.rows["opacity_-104"]] == 0
    assert imp[s.rows["imp_e-105"]] == 0 and imp[s.rows["imp_e-120"]] == 0      # e^-105 lies below half the smallest subnormal
    assert np.isinf(imp[s.rows["imp_inf_0"]]) and np.isinf(imp[s.rows["imp_inf_1"]])
    assert row("imp_inf_0") == 0 and row("imp_inf_1") == 1                     # +Infinity sorts first, source order kept
    assert 0 < imp[s.rows["imp_-91"]] < tiny
    # scale stores
    assert 0 < scales[row("scale_-88"), 0] < tiny and 0 < scales[row("scale_-100"), 1] < tiny
    assert scales[row("scale_-104"), 2] == 0
    assert np.isfinite(scales[row("scale_88.7"), 0]) and scales[row("scale_88.7"), 0] > 3e38
    assert np.isinf(scales[row("scale_89"), 0])
    bits = pc.four_sigma(buf)
    e = (bits >> 23) & 0xFF
    h = halves_of(tex)
    j = row("sigma_subnormal")
    assert e[j, 0] == 0 and bits[j, 0] & 0x7FFFFF                             # floatToHalf's exp == 0 branch with a non-zero fraction
    j = row("sigma_shift_51")
    assert (113 - e[j, [0, 3, 5]] >= 32).all()
    j = row("sigma_shift_36")
    assert (113 - e[j, [0, 3, 5]] >= 32).all() and (h[j, [0, 3, 5]] != 0).all()   # the count taken mod 32 leaves garbage behind
    assert set(range(22)) | {31} <= set(((h >> 10) & 31).reshape(-1).tolist())  # half exponents 0-21 and 31
    # quaternions
    quat = lambda name: buf[row(name), 28:32].tolist()
    assert quat("quat_zero") == [0, 0, 0, 0] and quat("quat_nan") == [0, 0, 0, 0]
    assert quat("quat_w") == [255, 128, 128, 128] and quat("quat_-w") == [0, 128, 128, 128]
    assert quat("quat_tiny") == [128, 128, 128, 255]
    assert quat("quat_huge") == [219, 219, 128, 128]
    assert quat("quat_ones") == [192, 192, 192, 192]
    assert quat("quat_inf") == [0, 128, 128, 128]
    # colour and alpha
    assert buf[row("dc_nonfinite"), 24:27].tolist() == [255, 0, 0]
    assert buf[row("half_way"), 24:28].tolist() == [128, 128, 128, 128]
    assert buf[row("opacity_inf"), 27] == 255 and buf[row("imp_zero_0"), 27] == 0
    # labels: exact in `lab`, rounded in the texture word
    word = lambda name: float(tex.reshape(-1, 8)[row(name), 3:4].copy().view(np.float32)[0])
    for v, rounded in ((2 ** 24 + 1, 2 ** 24), (2 ** 24 + 3, 2 ** 24 + 4), (-2 ** 24 - 1, -2 ** 24), (pc.INT32_MAX, 2 ** 31),
                       (pc.INT32_MIN, -2 ** 31), (pc.NO_SELECTION, pc.NO_SELECTION)):
        assert lab[row(f"label_{v}")] == v and word(f"label_{v}") == float(rounded)


def py_halves(bits):
    return np.array([pc.js_float_to_half(int(b)) for b in np.asarray(bits).reshape(-1)], np.uint32).reshape(np.shape(bits))


def test_float_to_half_python_equals_oracle_on_every_exponent():
    """every f32 exponent x mantissas at the truncation and shift edges x both signs, straight into the oracle's floatToHalf
    (most of these patterns - negative zero, NaN payloads, single bits - are not the 4 * sigma of any splat)"""
    pats = np.array([(s << 31) | (e << 23) | m for e in range(256) for m in (0, 1, 0x1FFF, 0x2000, 0x400000, 0x7FFFFF) for s in (0, 1)],
                    np.uint32)
    with np.errstate(invalid="ignore"):
        got = oracle.float_to_half(pats.view(np.float32).astype(np.float64))
    assert np.array_equal(got, py_halves(pats))
    assert len(set(got.tolist())) > 256


def test_float_to_half_python_equals_oracle_texture_on_the_value_edge_scene():
    s = pc.value_edge_scene()
    buf, _, tex, _ = s.expect()
    bits = pc.four_sigma(buf)
    want = halves_of(tex)
    got = py_halves(bits)
    bad = np.nonzero((got != want).any(1))[0]
    assert len(bad) == 0, f"packed rows {bad[:8]}: {got[bad[0]]} != {want[bad[0]]} for 4 * sigma bits {bits[bad[0]]}"
    shifts = 113 - ((bits >> 23) & 0xFF).astype(np.int64)
    assert (shifts >= 32).sum() > 50 and ((bits >> 23) & 0xFF == 0).any() and ((bits >> 23) & 0xFF == 255).any()


def hit_buffer(case):
    xyz, f_dc, labels = case.arrays()
    buf, order = oracle.pack_splats(xyz, None, None, None, f_dc)
    assert np.array_equal(order, np.arange(case.n))
    return buf, labels


@pytest.mark.parametrize("case", pc.HIT_CASES, ids=lambda c: c.name)
def test_oracle_hit_test_gives_the_answers_written_in_the_cases(case):
    buf, labels = hit_buffer(case)
    assert oracle.hit_test(buf, labels, pc.HIT_CAM, pc.HIT_W, pc.HIT_H, *case.click) == case.want


def test_hit_cases_cover_what_they_name():
    names = [c.name for c in pc.HIT_CASES]
    assert len(set(names)) == len(names)
    # (0, 0, z) projects exactly onto the centre: a click 10 px away is exactly on the threshold
    buf, labels = hit_buffer(pc.HitCase("centre", 1, {0: pc.P}, None))
    assert oracle.hit_test(buf, labels, pc.HIT_CAM, pc.HIT_W, pc.HIT_H, 330.0, 240.0) == (pc.NO_SELECTION, -1)
    assert oracle.hit_test(buf, labels, pc.HIT_CAM, pc.HIT_W, pc.HIT_H, 329.999, 240.0) == (1000, 0)
    # the mirrored splat of the clip case would be hit if w <= 0 were not skipped: the same splat in front is
    buf, labels = hit_buffer(pc.HitCase("front", 2, {1: (0.0, 0.0, 2.0)}, None))
    assert oracle.hit_test(buf, labels, pc.HIT_CAM, pc.HIT_W, pc.HIT_H, *pc.CENTRE) == (1001, 1)
    big = [c for c in pc.HIT_CASES if c.n > pc.TRIP]
    assert big and all(max(c.rows) >= pc.TRIP for c in big)


def test_hit_order_scene_aims_at_coincident_pairs_of_the_tie_run():
    s = pc.hit_order_scene()
    buf, order, _, lab = s.expect()
    where = np.empty(s.n, np.int64)
    where[order] = np.arange(s.n)
    assert not np.array_equal(order, np.arange(s.n))
    hits = [oracle.hit_test(buf, lab, pc.HIT_CAM, pc.HIT_W, pc.HIT_H, x, y) for x, y in s.clicks]
    assert hits[-1] == (pc.NO_SELECTION, -1)
    on_run = [(label, j) for label, j in hits[:-1] if order[j] in s.placed]
    assert len(on_run) >= 40
    for label, j in on_run:
        twin = int(order[j]) + 1                                               # the source row that shares the position
        assert label == s.labels[order[j]] and int(np.float32(label)) != label
        assert np.array_equal(s.xyz[twin], s.xyz[order[j]]) and where[twin] == j + 1      # ... packed right behind: the lower row won
