"""CPU: the numpy models of the per-splat pre pass (tests/vertex_model.py) against the oracle, and the scenes of
tests/vertex_cases.py against what they claim to hold.

The vertex model equals oracle.vertex BIT FOR BIT on every splat of every scene (drawn flag and, where drawn, every output
field); its buckets, stably sorted, give oracle.depth_order's depth_index and dropped count.  Every scene asserts, from the model
alone, that each branch it was built for is taken by at least the stated number of splats."""
import numpy as np
import pytest

import oracle
import vertex_cases as vc
import vertex_model as vm

NAMES = list(vc.all_cases())
FIELDS = ("cx", "cy", "g0", "g1", "major", "minor", "color", "fade")


def oracle_vertex(ev, idx):
    """oracle.vertex on the packed splats idx -> (drawn (m,), fields (m, 15) float32)"""
    cam, tex = ev.cam, ev.tex.reshape(-1, 8)
    view, proj = ev.view.astype(np.float32), ev.proj.astype(np.float32)
    drawn, out = np.zeros(len(idx), bool), np.zeros((len(idx), 15), np.float32)
    for j, i in enumerate(idx):
        o = oracle.vertex(tex[i], view, proj, cam["fx"], cam["fy"], ev.W, ev.H)
        drawn[j] = bool(o.drawn)
        out[j] = (o.cx, o.cy, *o.g0, *o.g1, *o.major, *o.minor, *o.color, o.fade)
    return drawn, out


def model_fields(ev, idx):
    v = ev.v
    return np.concatenate([v["cx"][idx, None], v["cy"][idx, None], v["g0"][idx], v["g1"][idx], v["major"][idx], v["minor"][idx],
                           v["color"][idx], v["fade"][idx, None]], 1).astype(np.float32)


def assert_model_is_oracle(ev, idx, what):
    drawn, want = oracle_vertex(ev, idx)
    assert np.array_equal(drawn, ev.drawn[idx]), f"{what}: drawn flag differs at packed splats {idx[drawn != ev.drawn[idx]][:8]}"
    got = model_fields(ev, idx)
    same = (got.view(np.uint32) == want.view(np.uint32)).all(1) | ~drawn
    assert same.all(), f"{what}: {int((~same).sum())} drawn splats differ in their bits, first {idx[~same][:8]}"
    return int(drawn.sum())


def assert_depth_order(ev, what):
    for compact in (0, 1):
        b = vm.buckets(ev.depth, compact, ev.rect)
        di, dropped = oracle.depth_order(ev.buf, ev.vp)
        assert b["dropped"] == dropped, f"{what}: dropped {b['dropped']} != {dropped}"
        assert np.array_equal(vm.depth_index(b["bucket"]), di), f"{what}: depth_index differs"


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_oracle_bit_for_bit(name):
    case = vc.all_cases()[name]
    for k in range(len(case.cams)):
        ev = case.ev(k)
        assert_model_is_oracle(ev, np.arange(case.n), f"{name} view {k}")
        assert_depth_order(ev, f"{name} view {k}")


@pytest.mark.parametrize("name", NAMES)
def test_scene_holds_what_it_was_built_for(name):
    case = vc.all_cases()[name]
    counts = case.counts(case.ev(0))
    print(name, case.n, "splats:", counts)
    for key, least in case.need.items():
        if key in ("n", "dropped", "kept", "one_key", "bucket_0", "first_is_packed_0", "first_dropped", "first_drawn", "first_has_rect",
                   "first_culled", "pairs_split", "pairs_kept_side_has_rect"):
            assert counts[key] == least, f"{name}: {key} = {counts[key]}, built for exactly {least}"
        else:
            assert counts[key] >= least, f"{name}: {key} = {counts[key]}, built for at least {least}"
    for a, b, k, axis in case.meta.get("pairs", ()):
        pa, pb = case.attrs[0][a], case.attrs[0][b]
        assert np.nextafter(pa[axis], pb[axis]) == pb[axis] and np.array_equal(np.delete(pa, axis), np.delete(pb, axis))
        c = case.ev(0).src(case.ev(0).cls)
        assert c[a] >= vc.CULLED and c[b] == k, f"{name}: the pair around comparison {k} is not split"


def test_edit_state_reaches_every_kind_of_edit():
    import render_edits_ref as ref
    case = vc.all_cases()["views"]
    ev = case.ev(0)
    vlabel = ref.shader_labels(ev.labels)
    st = ref.state(**case.edits)
    assert (ref.first_match(vlabel, st["colours"].keys()) >= 0).sum() >= 100
    assert (ref.first_match(vlabel, st["displacements"].keys()) >= 0).sum() >= 100
    assert (vlabel == st["selected"]).sum() >= 50 and np.isin(ev.labels, st["hidden"]).sum() >= 100
    assert ((vlabel != ev.labels) & (ref.first_match(vlabel, st["colours"].keys()) >= 0)).sum() >= 8      # fp32-rounded label, coloured
    assert (ev.labels == 2 ** 24 + 3).sum() >= 8                                                          # .. and hidden by its exact value


@pytest.mark.parametrize("n", vc.LARGE_SIZES)
def test_large_sizes_sample(n):
    """20 000 random splats and the last 4 096 against oracle.vertex (the oracle's per-splat loop costs 20 us a splat); the depth
    order of the whole scene"""
    case = vc.size_case(n)
    ev = case.ev(0)
    idx = np.unique(np.concatenate([np.random.default_rng(n).integers(0, n, 20000), np.arange(n - 4096, n)]))
    drawn = assert_model_is_oracle(ev, idx, case.name)
    assert_depth_order(ev, case.name)
    cls = np.bincount(ev.cls, minlength=len(vm.CLASSES))
    print(case.name, "sample drawn", drawn, "classes", dict(zip(vm.CLASSES, cls.tolist())))
    assert all(cls[vm.CLS[k]] >= 8 for k in vm.CLASSES), "every class occurs in the random scene"
