"""GPU: the instance association (gsx_assoc_*) against tests/assoc_model.py fed with Context.project_all - every comparison
exact: the table, the remap, gid after every view, the relabelled map, the instance and dropped counts."""
import numpy as np
import pytest

import assoc_cases as ac
import assoc_model as am

pytestmark = pytest.mark.gpu


def run_both(c, pos, cams, maps, S, M, min_overlap=0.3, min_size=1, sizes=None, convert=None, packed_u8=False):
    """the same run on the GPU and in the model, compared after every view -> (model run, remaps, relabelled maps)"""
    c.upload_positions(pos)
    c.assoc_begin(S, M, min_overlap, min_size)
    run = am.Run(len(pos), S, M, min_overlap, min_size)
    remaps, outs = [], []
    for v, (cam, seg) in enumerate(zip(cams, maps)):
        size = None if sizes is None else sizes[v]
        x, y = c.project_all(cam)
        want_remap, want_out = run.view(x, y, seg.astype(np.int64) - 1 if packed_u8 else seg, size)
        remap, out = c.assoc_view(cam, seg if convert is None else convert(seg), size, packed_u8=packed_u8)
        out = out.cpu().numpy()
        assert remap.dtype == np.int32 and np.array_equal(remap, want_remap), f"view {v}: remap"
        assert np.array_equal(c.assoc_table(), run.table), f"view {v}: table"
        assert np.array_equal(c.assoc_ids(), run.gid), f"view {v}: gid"
        assert out.dtype == np.int32 and np.array_equal(out, want_out), f"view {v}: relabelled map"
        assert (c.assoc_num_views(), c.assoc_num_instances(), c.assoc_num_dropped()) == (run.views, run.G, run.dropped), f"view {v}"
        remaps.append(remap)
        outs.append(out)
    return run, remaps, outs


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_sizes(ctx, n):
    cams, maps = ac.small_views(3, 8, 100 + n)
    pos = ac.small_positions(n, n)
    if n == 1:
        pos[0] = (0.1, 0.1, 4.0)
    run, _, _ = run_both(ctx, pos, cams, maps, 8, 16)
    if n >= 63:
        assert run.G >= 2 and (run.gid >= 0).sum() > n // 4 and (run.gid < 0).any()


def test_view_nobody_is_seen_in_and_background_only_map(ctx):
    cams, maps = ac.small_views(2, 8, 7)
    pos = ac.small_positions(300, 8)
    cams = [cams[0], ac.AWAY, ac.small_cam(), cams[1]]
    maps = [maps[0], maps[1], np.full((ac.MH, ac.MW), -1, np.int32), maps[1]]
    run, remaps, outs = run_both(ctx, pos, cams, maps, 8, 16)
    assert (ctx.project_all(ac.AWAY)[0] < 0).all()
    assert (remaps[1] == -1).all() and (outs[1] == -1).all()           # nobody seen: every row is empty
    assert (remaps[2] == -1).all() and (outs[2] == -1).all() and ctx.assoc_num_views() == 4
    assert run.G >= 2


def test_extreme_segment_ids(ctx):
    S = 254
    assert am.MAX_SEGMENTS == S
    seg = np.zeros((ac.MH, ac.MW), np.int32)
    seg[:, ac.MW // 2:] = S - 1
    seg2 = np.where(seg == 0, S - 1, 0).astype(np.int32)
    run, remaps, _ = run_both(ctx, ac.small_positions(500, 9), [ac.small_cam(), ac.small_cam((0.2, 0.0, 0.0))], [seg, seg2], S, 255)
    assert run.G == 2 and sorted(remaps[0][[0, S - 1]].tolist()) == [0, 1] and remaps[1][0] == remaps[0][S - 1]


@pytest.mark.parametrize("M", [1, 255])
def test_instance_limits(ctx, M):
    cams, maps = ac.small_views(3, 12, 31)
    run, _, _ = run_both(ctx, ac.small_positions(1000, 32), cams, maps, 12, M)
    if M == 1:
        assert run.G == 1 and run.dropped > 0
    else:
        assert run.G > 4 and run.dropped == 0


@pytest.mark.parametrize("kind", ["one", "distinct", "interleaved"])
def test_wave_keys(ctx, kind):
    """a wave whose 64 lanes hold one key, 64 distinct keys, two keys interleaved: 128 Gaussians, each alone on its pixel, and
    maps painted along the upload's Morton order; the second view brings the same through the gid column of the key"""
    pos, cam, S, M = ac.grid_positions(), ac.small_cam(), 200, 255
    ctx.upload_positions(pos)
    order = ctx.spatial_order().astype(np.int64)
    assert not np.array_equal(order, np.arange(128))
    x, y = ctx.project_all(cam)
    assert (x >= 0).all() and len(set(zip(x.tolist(), y.tolist()))) == 128
    slot = np.arange(128)
    first = {"one": slot // 64 + 3, "distinct": slot, "interleaved": slot % 2}[kind]
    second = {"one": np.full(128, 7), "distinct": np.full(128, 7), "interleaved": slot // 64}[kind]
    maps = [ac.paint(x, y, order, first), ac.paint(x, y, order, second)]
    run, _, _ = run_both(ctx, pos, [cam, cam], maps, S, M)
    expect = {"one": 1, "distinct": 64, "interleaved": 2}[kind]
    probe = am.Run(128, S, M)
    for seg in maps:                                      # the keys each wave held in each view, from the model's own quantities
        keys = (seg[y[order], x[order]] + 1) * (M + 1) + probe.gid[order] + 1
        for wave in (keys[:64], keys[64:]):
            assert len(np.unique(wave)) == expect
            if kind == "interleaved":
                assert (wave[::2] == wave[0]).all() and (wave[1::2] == wave[1]).all()
        probe.view(x, y, seg)
    assert np.array_equal(probe.gid, run.gid)


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2500])
def test_workgroup_edges(ctx, n):
    """the table kernel's workgroups take 1024 Gaussians a step: sizes around one and past two of them"""
    cams, maps = ac.small_views(3, 8, 200 + n)
    run_both(ctx, ac.small_positions(n, 300 + n), cams, maps, 8, 16)


def test_several_steps_per_workgroup_and_the_largest_table(gsx, ctx):
    """600 000 Gaussians are 586 steps: two per workgroup while two copies of the table fit a CU (512 workgroups), three once
    240 instances are open and S = 254 leaves room for one copy (256 workgroups) of 255 x 241 16-bit counters; entries of the
    global table pass 2^16, which no workgroup's counter may"""
    k = gsx.assoc_constants()
    n = 600_000
    assert -(-n // k["block"]) > 512 and k["lds_entries"] == 255 * 256
    r, c = np.mgrid[0:ac.MH, 0:ac.MW]
    many = ((r // 2) * (ac.MW // 2) + c // 2).astype(np.int32)            # 240 segments of 2 x 2 pixels
    one = np.zeros((ac.MH, ac.MW), np.int32)
    cams, maps = ac.small_views(2, 12, 91)
    tables = []
    ctx.upload_positions(ac.small_positions(n, 92))
    run = am.Run(n, 254, 255)
    ctx.assoc_begin(254, 255)
    for cam, seg in zip([ac.small_cam(), ac.small_cam()] + cams, [one, many] + maps):
        want_remap, want_out = run.view(*ctx.project_all(cam), seg)
        remap, out = ctx.assoc_view(cam, seg)
        assert np.array_equal(remap, want_remap) and np.array_equal(out.cpu().numpy(), want_out)
        assert np.array_equal(ctx.assoc_table(), run.table)
        tables.append((run.G, int(run.table.max())))
    assert np.array_equal(ctx.assoc_ids(), run.gid) and (ctx.assoc_num_instances(), ctx.assoc_num_dropped()) == (run.G, run.dropped)
    assert tables[0] == (1, tables[0][1]) and tables[0][1] > 65535 and tables[1][0] == 240 and tables[2][1] > 65535
    assert 255 * (240 + 1) * 2 * 2 > 160 * 1024 and run.dropped > 0


def test_map_half_the_image_size(ctx):
    cams, maps = ac.small_views(3, 6, 41, ac.MW // 2, ac.MH // 2)
    run, _, outs = run_both(ctx, ac.small_positions(600, 42), cams, maps, 6, 32, sizes=[(ac.MW, ac.MH)] * 3)
    assert outs[0].shape == (ac.MH // 2, ac.MW // 2) and run.G >= 2


@pytest.mark.parametrize("dtype", ["int32", "int64", "uint8", "packed_u8"])
def test_dtypes_host_and_device(ctx, dtype):
    import torch
    cams, maps = ac.small_views(3, 8, 51)
    pos = ac.small_positions(700, 52)
    if dtype == "uint8":
        maps = [np.maximum(m, 0) for m in maps]         # a uint8 label map has no -1
    packed = dtype == "packed_u8"
    np_dt = {"int32": np.int32, "int64": np.int64, "uint8": np.uint8, "packed_u8": np.uint8}[dtype]
    maps = [(m + 1 if packed else m).astype(np_dt) for m in maps]
    ref = run_both(ctx, pos, cams, [m.astype(np.int32) for m in maps], 8, 16, packed_u8=False) if not packed else None
    host = run_both(ctx, pos, cams, maps, 8, 16, packed_u8=packed)
    dev = run_both(ctx, pos, cams, maps, 8, 16, packed_u8=packed, convert=lambda m: torch.from_numpy(m).cuda())
    for a, b in zip(host[1] + host[2], dev[1] + dev[2]):
        assert np.array_equal(a, b)
    if ref is not None:
        for a, b in zip(ref[1] + ref[2], host[1] + host[2]):
            assert np.array_equal(a, b)
    # a map at an address that is aligned to its element only takes the scalar loads
    big = torch.zeros(ac.MH * ac.MW + 1, dtype=torch.from_numpy(maps[0]).dtype, device="cuda")
    odd = big[1:].view(ac.MH, ac.MW)
    odd.copy_(torch.from_numpy(maps[0]))
    ctx.assoc_begin(8, 16)
    remap, out = ctx.assoc_view(cams[0], odd, packed_u8=packed)
    assert np.array_equal(remap, host[1][0]) and np.array_equal(out.cpu().numpy(), host[2][0])


def test_ids_come_back_in_upload_order(ctx):
    pos = ac.small_positions(1000, 61)
    cams, maps = ac.small_views(2, 8, 62)
    run, _, _ = run_both(ctx, pos, cams, maps, 8, 16)
    assert not np.array_equal(ctx.spatial_order(), np.arange(1000))
    assert np.array_equal(ctx.assoc_ids(), run.gid) and len(np.unique(run.gid)) > 3


def test_same_run_twice(ctx):
    pos = ac.small_positions(1000, 71)
    cams, maps = ac.small_views(4, 10, 72)
    a = run_both(ctx, pos, cams, maps, 10, 8, 0.5, 3)
    gid_a = ctx.assoc_ids()
    b = run_both(ctx, pos, cams, maps, 10, 8, 0.5, 3)
    assert np.array_equal(gid_a, ctx.assoc_ids())
    for u, w in zip(a[1] + a[2], b[1] + b[2]):
        assert np.array_equal(u, w)


@pytest.mark.parametrize("device", [False, True])
def test_range_error_changes_nothing(ctx, device):
    import torch
    pos = ac.small_positions(500, 81)
    cams, maps = ac.small_views(3, 8, 82)
    up = (lambda m: torch.from_numpy(m).cuda()) if device else (lambda m: m)
    ctx.upload_positions(pos)
    ctx.assoc_begin(8, 16)
    run = am.Run(500, 8, 16)
    run.view(*ctx.project_all(cams[0]), maps[0])
    ctx.assoc_view(cams[0], up(maps[0]))
    state = (ctx.assoc_ids(), ctx.assoc_num_instances(), ctx.assoc_num_views(), ctx.assoc_num_dropped(), ctx.assoc_table())
    for value, where in ((8, (ac.MH - 1, ac.MW - 1)), (-2, (0, 0)), (2 ** 31 - 1, (5, 7))):
        bad = maps[1].copy()
        bad[where] = value                     # a corner no Gaussian need project to: the whole map is checked
        with pytest.raises(ValueError, match=f"row {where[0]}, column {where[1]}"):
            ctx.assoc_view(cams[1], up(bad))
        now = (ctx.assoc_ids(), ctx.assoc_num_instances(), ctx.assoc_num_views(), ctx.assoc_num_dropped(), ctx.assoc_table())
        assert all(np.array_equal(a, b) for a, b in zip(state, now))
    for cam, seg in zip(cams[1:], maps[1:]):   # and the next views proceed
        want_remap, want_out = run.view(*ctx.project_all(cam), seg)
        remap, out = ctx.assoc_view(cam, up(seg))
        assert np.array_equal(remap, want_remap) and np.array_equal(out.cpu().numpy(), want_out)
    assert np.array_equal(ctx.assoc_ids(), run.gid) and ctx.assoc_num_views() == 3


def test_error_codes(gsx):
    E = gsx._lib
    seg = np.zeros((ac.MH, ac.MW), np.int32)
    with gsx.Context(0) as c:
        lib, cam = c._lib, gsx.Camera.from_dict(ac.small_cam())
        view = lambda: lib.gsx_assoc_view(c.h, cam, seg.ctypes.data, E.GSX_SEG_I32, ac.MW, ac.MH, ac.MW, ac.MH, None, None)
        assert lib.gsx_assoc_begin(c.h, 8, 16, 0.3, 1) == E.GSX_E_STATE          # before gsx_upload_positions
        c.upload_positions(ac.small_positions(10, 1))
        ids = np.empty(10, np.int32)
        table = np.empty((9, 17), np.uint32)
        assert view() == E.GSX_E_STATE and lib.gsx_assoc_ids(c.h, ids.ctypes.data) == E.GSX_E_STATE  # before gsx_assoc_begin
        assert lib.gsx_assoc_table(c.h, table.ctypes.data) == E.GSX_E_STATE
        assert (lib.gsx_assoc_num_views(c.h), lib.gsx_assoc_num_instances(c.h), lib.gsx_assoc_num_dropped(c.h)) == (0, 0, 0)
        for args in ((0, 16, 0.3, 1), (255, 16, 0.3, 1), (8, 0, 0.3, 1), (8, 256, 0.3, 1), (8, 16, -0.1, 1), (8, 16, 1.5, 1),
                     (8, 16, float("nan"), 1), (8, 16, float("inf"), 1), (8, 16, 0.3, 0)):
            assert lib.gsx_assoc_begin(c.h, *args) == E.GSX_E_INVALID, args
        assert lib.gsx_assoc_begin(c.h, 254, 255, 1.0, 1) == E.GSX_OK
        assert lib.gsx_assoc_begin(c.h, 8, 16, 0.0, 1) == E.GSX_OK
        assert view() == E.GSX_OK and lib.gsx_assoc_num_views(c.h) == 1
        assert lib.gsx_assoc_view(c.h, None, seg.ctypes.data, E.GSX_SEG_I32, ac.MW, ac.MH, ac.MW, ac.MH, None, None) == E.GSX_E_INVALID
        assert lib.gsx_assoc_view(c.h, cam, None, E.GSX_SEG_I32, ac.MW, ac.MH, ac.MW, ac.MH, None, None) == E.GSX_E_INVALID
        assert lib.gsx_assoc_view_device(c.h, cam, None, E.GSX_SEG_I32, ac.MW, ac.MH, ac.MW, ac.MH, None, None) == E.GSX_E_INVALID
        assert lib.gsx_assoc_view(c.h, cam, seg.ctypes.data, 99, ac.MW, ac.MH, ac.MW, ac.MH, None, None) == E.GSX_E_INVALID
        assert lib.gsx_assoc_view(c.h, cam, seg.ctypes.data, E.GSX_SEG_I32, 0, ac.MH, ac.MW, ac.MH, None, None) == E.GSX_E_INVALID
        assert lib.gsx_assoc_view(c.h, cam, seg.ctypes.data, E.GSX_SEG_I32, ac.MW, ac.MH, 0, ac.MH, None, None) == E.GSX_E_INVALID
        assert lib.gsx_assoc_ids(c.h, None) == E.GSX_E_INVALID and lib.gsx_assoc_table(c.h, None) == E.GSX_E_INVALID
        assert lib.gsx_assoc_num_views(c.h) == 1
        c.upload_positions(ac.small_positions(10, 2))                             # a new upload ends the run
        assert view() == E.GSX_E_STATE and lib.gsx_assoc_num_views(c.h) == 0
    assert gsx.lib().gsx_assoc_begin(None, 8, 16, 0.3, 1) == E.GSX_E_INVALID
    assert gsx.lib().gsx_debug_assoc_constants(None) == E.GSX_E_INVALID
    k = gsx.assoc_constants()
    assert (k["one"], k["shift"], k["block"], k["max_segments"], k["max_instances"]) == (1 << 20, 20, 1024, 254, 255)
    assert k["one"] == 1 << am.ONE_SHIFT and (k["lds_entries"], k["max_chunks"]) == (255 * 256, 63) and k["block"] * k["max_chunks"] < 65536


def test_value_scene(gsx, ctx):
    import oracle
    pos, blob, cams, maps, sizes = ac.value_scene()
    run = am.Run(len(pos), 254, 255, 0.3, 1)
    ctx.upload_positions(pos)
    relabelled = [run.view(*ctx.project_all(cam), seg, size)[1] for cam, seg, size in zip(cams, maps, sizes)]
    want = oracle.assign_labels(pos, cams, relabelled, sizes)
    labels, n_instances = gsx.assign_instances_from_maps(pos, cams, maps, sizes, ctx=ctx)
    assert labels.dtype == np.int32 and np.array_equal(labels, want) and n_instances == run.G == ac.K
    assert np.array_equal(ctx.assoc_ids(), run.gid) and ctx.assoc_num_dropped() == 0
    assert (labels >= 0).all() and am.same_partition(labels, blob)
    assert not am.same_partition(gsx.assign_labels_from_maps(pos, cams, maps, sizes, n_classes=254, ctx=ctx), blob)
