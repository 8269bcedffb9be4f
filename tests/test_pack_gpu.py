"""The scene upload and the hit test on the GPU (csrc/render_scene.hip: splat_importance_kernel + the radix sort, splat_pack_kernel,
labels_pack_kernel, sh_pack_kernel; hit_partial_kernel, hit_final_kernel) against the expectations of tests/pack_cases.py,
which tests/test_pack_model.py checks against the oracle on the CPU.

Everything is compared EXACTLY: the 32-byte rows, the importance permutation, the eight texture words, the int32 labels and the
SH planes through their uint32 view; (label, row) of every pick.  No tolerance anywhere in this file: the scenes are built so
that no stored value depends on the last bits of the device's fp64 exp (pack_cases rule 2).

On an MI355X all 65 tests pass, 2.4 s in all.  Mutants of the unit (then part of render.hip), each built once and run once against this file (tests that
failed, of 65):
    hit_final_kernel's label through fp32, (int)(float)labels[idx], the value the texture word holds      3: label_2^24+1 gives
        (16777216, 299) for (16777217, 299), label_-2^24-1, and the scene in importance order
    hit_better: a.idx > b.idx                12: every tie case with two rows on the click, the scene in importance order
    sh_pack_kernel: plane (c * K + k)        10: degrees 1-3 at every n, the replaced scene (degree 0 has one k: identical)
    dist <= 10.0                             2: threshold_10, threshold_10_y"""
import ctypes as C

import numpy as np
import pytest

import oracle
import pack_cases as pc

pytestmark = pytest.mark.gpu
PACK = pc.all_pack_scenes()


def upload(ctx, s):
    ctx.upload_splats(*s.attrs(), labels=s.labels)


def read_back(ctx):
    buf, order, tex = ctx.render_debug()
    labels, sh, degree = ctx.debug_render_scene()
    return (buf, order, tex, labels), sh, degree


def check_pack(ctx, s):
    got, sh, degree = read_back(ctx)
    assert ctx._lib.gsx_num_splats(ctx.h) == s.n
    diff = pc.first_difference(got, s.expect())
    assert diff is None, f"{s.name}: {diff}"
    return sh, degree


def check_planes(sh, want, order, what):
    assert sh is not None and sh.shape == want.shape, f"{what}: planes {None if sh is None else sh.shape}, expected {want.shape}"
    bad = np.argwhere(sh.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} coefficients differ, first (k, c, packed row) = {tuple(bad[0])} (source row " \
                          f"{order[bad[0][2]]}): {sh[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("name", list(PACK))
def test_upload_matches_the_oracle_byte_for_byte(ctx, name):
    s = PACK[name]()
    upload(ctx, s)
    sh, degree = check_pack(ctx, s)
    assert sh is None and degree == -1


@pytest.mark.parametrize("degree,n", pc.SH_CASES)
def test_sh_planes_are_laid_out_by_coefficient_channel_row(ctx, degree, n):
    s = pc.sh_scene(degree, n)
    upload(ctx, s)
    ctx.upload_sh(s.f_rest if degree else None, degree)
    sh, got_degree = check_pack(ctx, s)
    assert got_degree == degree
    order = s.expect()[1]
    check_planes(sh, pc.sh_planes(s.f_dc, s.f_rest, order, degree), order, s.name)


def test_a_new_upload_replaces_every_part_of_the_scene(ctx, gsx):
    lib = gsx.lib()
    first, second = pc.sh_scene(3, 4097), pc.sh_scene(2, 257)
    upload(ctx, first)
    ctx.upload_sh(first.f_rest, 3)
    ctx.set_render_edits(hidden=(int(first.labels[0]),))
    assert ctx.render_num_hidden() == int((first.labels == first.labels[0]).sum()) > 0
    assert ctx.debug_render_scene()[2] == 3
    # 257 splats without SH on top of 4097 with degree 3
    upload(ctx, second)
    assert lib.gsx_num_splats(ctx.h) == 257
    sh, degree = check_pack(ctx, second)
    assert sh is None and degree == -1
    assert ctx.render_num_hidden() == 0
    sentinel = np.full(3 * 16 * 4097, -7.5, np.float32)                        # sh_out is left alone while the SH colour is off
    labels = np.empty(257, np.int32)
    deg = C.c_int32(99)
    assert lib.gsx_debug_render_scene(ctx.h, labels.ctypes.data, sentinel.ctypes.data, C.byref(deg)) == 0
    assert (sentinel == -7.5).all() and deg.value == -1 and np.array_equal(labels, second.expect()[3])
    assert lib.gsx_debug_render_scene(ctx.h, None, None, None) == 0            # any pointer may be NULL
    # SH of degree 2 now lays out the SECOND scene's f_dc in the second scene's order
    ctx.upload_sh(second.f_rest, 2)
    sh, degree = check_pack(ctx, second)
    assert degree == 2
    order = second.expect()[1]
    check_planes(sh, pc.sh_planes(second.f_dc, second.f_rest, order, 2), order, "degree 2 after the second upload")
    # an empty scene after a scene
    ctx.upload_splats(np.zeros((0, 3), np.float32), None, None, None, np.zeros((0, 3), np.float32))
    assert lib.gsx_num_splats(ctx.h) == 0
    assert ctx.hit_test(pc.HIT_CAM, pc.HIT_W, pc.HIT_H, *pc.CENTRE) == (pc.NO_SELECTION, -1)
    labels, sh, degree = ctx.debug_render_scene()
    assert len(labels) == 0 and sh is None and degree == -1


@pytest.mark.parametrize("case", pc.HIT_CASES, ids=lambda c: c.name)
def test_hit_test_constructed_cases(ctx, case):
    xyz, f_dc, labels = case.arrays()
    ctx.upload_splats(xyz, None, None, None, f_dc, labels=labels)
    got = ctx.hit_test(pc.HIT_CAM, pc.HIT_W, pc.HIT_H, *case.click)
    assert got == case.want, f"{case.name}: (label, row) {got}, the reference's loop gives {case.want}"


def test_hit_test_in_importance_order_returns_exact_labels(ctx):
    s = pc.hit_order_scene()
    upload(ctx, s)
    check_pack(ctx, s)
    buf, order, _, lab = s.expect()
    for x, y in s.clicks:
        want = oracle.hit_test(buf, lab, pc.HIT_CAM, pc.HIT_W, pc.HIT_H, x, y)
        got = ctx.hit_test(pc.HIT_CAM, pc.HIT_W, pc.HIT_H, x, y)
        assert got == want, f"click ({x}, {y}): (label, row) {got} != {want} (source row {order[want[1]] if want[1] >= 0 else None})"
