"""The rasterizer's per-splat pre pass on the GPU (csrc/render_pre.hip: pre_geom, pre_one, pre_kernel<EDIT>, the twelve
pre_multi_kernel<NV, EDIT> and bucket_kernel) through gsx_debug_render_pre, which issues the product's own launches, against the
numpy models of tests/vertex_model.py on the scenes of tests/vertex_cases.py.  test_vertex_model.py shows on the CPU that the
models equal the oracle bit for bit and that every scene enters the branches it names.

Everything is compared EXACTLY: depth keys, tile rectangles, pre[0..2], buckets, sort keys (both `compact` forms), the cleared
rectangles and the dropped count as integers; the 12 floats of a record through their uint32 view wherever the model gives the
splat a rectangle and at splat 0; every other record must still hold the 0xFF bytes it was filled with.  The vertex stage is
fp32 in the oracle's operation order, compiled without contraction, with correctly rounded division and square root: no
tolerance anywhere in this file.  On an MI355X every field of every splat is identical (39 tests, 1 048 581 splats at the most).

Mutants of the unit (then part of render.hip), each built once and run once (tests of this file that failed / older rasterizer tests that noticed):
    p2[0] > clip -> >=                       the 3 frustum scenes / none       1/64 slack taken off ex       18 / none
    floorf for x0                            31 / 3 (blend lists)              grid stride doubled           the 2 large sizes / none
    depth_range_to without slo[3]            wave3, size_256, 524289 / 10      .. without shi[3]             13 / 8
    record store of pre_multi without i == 0 23 / 20                           b <= 65536                    30 / 43
    tx1 << 7                                 32 / 87
    acc + b * p at k == 0 in pre_multi_kernel: survives everything, and must - acc starts at 0.0f, 0.0f + x is x for every x but
    -0.0, and the + 0.5f of the clamp erases the sign of a zero sum: no output bit can differ."""
import numpy as np
import pytest

import vertex_cases as vc
import vertex_model as vm

pytestmark = pytest.mark.gpu
NAMES = [n for n in vc.all_cases() if n != "views"]
INT_FIELDS = ("depth", "rect", "bucket", "key", "rect_bucket")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_view(out, geo, depth, records, compact, what):
    """one view's outputs of the hook against the models: geo = the Eval of the geometry the shader sees, depth = the keys"""
    assert np.array_equal(out["depth"], depth), f"{what}: depth keys differ at {np.nonzero(out['depth'] != depth)[0][:8]}"
    bad = np.nonzero(out["rect"] != geo.rect)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} rectangles differ, first {bad[:8]}: {out['rect'][bad[:8]]} != {geo.rect[bad[:8]]} " \
                          f"(classes {geo.cls[bad[:8]]})"
    assert out["pre"][0] == depth.min() and out["pre"][1] == depth.max(), f"{what}: depth range {out['pre'][:2]}"
    assert np.uint32(out["pre"][2]) == geo.rect[0], f"{what}: pre[2] = {out['pre'][2]:#x}, splat 0's rectangle is {geo.rect[0]:#x}"
    b = vm.buckets(depth, compact, geo.rect)
    for k, want in (("bucket", b["bucket"]), ("key", b["key"]), ("rect_bucket", b["rect"])):
        bad = np.nonzero(out[k] != want)[0]
        assert len(bad) == 0, f"{what} compact={compact}: {k} differs at {bad[:8]}: {out[k][bad[:8]]} != {want[bad[:8]]}"
    assert out["dropped"] == b["dropped"], f"{what}: dropped {out['dropped']} != {b['dropped']}"
    got, want = bits(out["rec"]), bits(records)
    written = geo.rect != vm.EMPTY_RECT
    written[0] = True
    bad = np.nonzero(written & (got != want).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} records differ in their bits, first {bad[:4]}: fields {np.nonzero(got[bad[0]] != want[bad[0]])[0]}, " \
                          f"{out['rec'][bad[0]]} != {records[bad[0]]}"
    stale = np.nonzero(~written & (got != 0xFFFFFFFF).any(1))[0]
    assert len(stale) == 0, f"{what}: {len(stale)} splats without a rectangle wrote a record, first {stale[:8]}"
    return int(written.sum()), b["dropped"]


def assert_same_outputs(a, b, what):
    for k in INT_FIELDS:
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs at {np.nonzero(a[k] != b[k])[0][:8]}"
    assert np.array_equal(a["pre"][:3], b["pre"][:3]) and a["dropped"] == b["dropped"], f"{what}: pre / dropped"
    bad = np.nonzero((bits(a["rec"]) != bits(b["rec"])).any(1))[0]
    assert len(bad) == 0, f"{what}: records (unwritten slots included) differ at {bad[:8]}"


@pytest.mark.parametrize("name", NAMES)
def test_single_view_against_the_models(ctx, name):
    """every scene and frame, one view: pre_kernel and pre_multi_kernel<1>, both `compact` forms"""
    case = vc.all_cases()[name]
    ev = case.ev(0)
    ctx.upload_splats(*case.attrs)
    buf, order, tex = ctx.render_debug()
    assert np.array_equal(order, ev.order) and np.array_equal(buf, ev.buf) and np.array_equal(tex, ev.tex), \
        f"{name}: the packed scene is not the oracle's (the branch counts of test_vertex_model.py would not hold)"
    _, records = vc.edited(case, ev, 0)
    for multi in (False, True):
        for compact in (0, 1):
            out = ctx.debug_render_pre([case.cam], case.W, case.H, multi=multi, compact=compact)[0]
            written, dropped = check_view(out, ev, ev.depth, records, compact, f"{name} multi={multi}")
    print(f"{name}: {case.n} splats, {written} records, {dropped} dropped: exact")


@pytest.mark.parametrize("edits", (False, True), ids=("plain", "edits"))
@pytest.mark.parametrize("sh", (None, 0, 1, 2, 3), ids=lambda d: "rgba8" if d is None else f"sh{d}")
def test_multi_view_kernel_equals_single_view_kernel_and_the_models(ctx, sh, edits):
    """six cameras that draw different subsets of the scene: ONE pre_multi_kernel<nv> launch, nv = 1..6, gives every view what
    its own pre_kernel launch gives, bit for bit, unwritten records included - and both are the models' (SH colour: fade *
    oracle.sh_colors; edits: render_edits_ref on the displaced scene, depth keys of the undisplaced one)"""
    case = vc.all_cases()["views"]
    ctx.upload_splats(*case.attrs, labels=case.labels)
    if sh is not None:
        ctx.upload_sh(vc.f_rest_for(case, sh), sh)
    if edits:
        ctx.set_render_edits(**case.edits)
    try:
        buf, order, tex = ctx.render_debug()
        assert np.array_equal(order, case.ev(0).order) and np.array_equal(tex, case.ev(0).tex)
        single = ctx.debug_render_pre(case.cams, case.W, case.H, multi=False)
        want = np.zeros((case.n, len(case.cams)), bool)
        for k in range(len(case.cams)):
            geo, records = vc.edited(case, case.ev(k), k, sh, edits)
            check_view(single[k], geo, case.ev(k).depth, records, 1, f"views sh={sh} edits={edits} view {k}")
            want[:, k] = geo.rect != vm.EMPTY_RECT
        mixed, none = int((want.any(1) & ~want.all(1)).sum()), int((~want.any(1)).sum())
        assert mixed >= case.n // 10 and none >= case.n // 100
        for nv in range(1, len(case.cams) + 1):
            multi = ctx.debug_render_pre(case.cams[:nv], case.W, case.H, multi=True)
            for k in range(nv):
                assert_same_outputs(multi[k], single[k], f"views sh={sh} edits={edits} nv={nv} view {k}")
        print(f"views sh={sh} edits={edits}: {mixed} splats drawn in some views only, {none} in none: exact")
    finally:
        ctx.clear_render_edits()


@pytest.mark.parametrize("n", vc.LARGE_SIZES)
def test_grid_stride_sizes(ctx, n):
    """2048 * 256 + 1 and 2 * 2048 * 256 + 5 splats: the second and third trip of the capped grid's stride loop, both kernels,
    the whole of every output against the models; the depth range against numpy's min and max"""
    case = vc.size_case(n)
    ctx.upload_splats(*case.attrs)
    packed = ctx.render_debug()
    ev = vc.Eval(None, case.cam, case.W, case.H, packed=packed)
    _, records = vc.edited(case, ev, 0)
    for multi in (False, True):
        out = ctx.debug_render_pre([case.cam], case.W, case.H, multi=multi, compact=int(multi))[0]
        assert out["pre"][0] == out["depth"].min() and out["pre"][1] == out["depth"].max()
        written, dropped = check_view(out, ev, ev.depth, records, int(multi), f"{case.name} multi={multi}")
    print(f"{case.name}: {written} records, {dropped} dropped, classes {np.bincount(ev.cls, minlength=len(vm.CLASSES)).tolist()}: exact")


def test_hook_leaves_the_context_as_it_was(ctx):
    """frames before and after the hook are the same bits: gsx_render_view, and gsx_render_views with the same cameras"""
    case = vc.all_cases()["views"]
    ctx.upload_splats(*case.attrs, labels=case.labels)
    ctx.upload_sh(case.f_rest, 3)
    before = ctx.render_view(case.cams[2], case.W, case.H)
    many_before = ctx.render_views(case.cams, case.W, case.H)
    assert before[..., 3].max() > 0.1
    ctx.debug_render_pre(case.cams, case.W, case.H, multi=True)
    ctx.debug_render_pre(case.cams[:2], case.W, case.H, multi=False, compact=False)
    after = ctx.render_view(case.cams[2], case.W, case.H)
    assert np.array_equal(bits(after), bits(before))
    ctx.debug_render_pre(case.cams[3:], case.W, case.H, multi=True)
    many_after = ctx.render_views(case.cams, case.W, case.H)
    assert np.array_equal(bits(many_after), bits(many_before))
    assert np.array_equal(bits(ctx.render_view(case.cams[2], case.W, case.H)), bits(before))
