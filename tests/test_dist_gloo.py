"""CPU, world_size 2 (gloo): the multi-GPU vote exchange protocol of dist.py — all-reduce SUM of the
int32-packed histogram, tie-break keys, all-reduce MAX — on numpy-backed shards.  The per-rank planes
have exactly the layout the HIP kernels produce (tests/test_vote_gpu.py checks that on the GPU).

Time limits of the GatherPipeline scenarios with locally derived views (_worker_local): the slowest case of this module without
them takes 4.3 s on the build machine (spawning the ranks and importing torch in each is most of it; the whole module ran at
the same time as a compiler).  A collective gets COLLECTIVE_TIMEOUT_S = 45 s, ten times that, so a rank that meets a protocol
mismatch fails instead of sitting there; the parent waits PARENT_TIMEOUT_S = 75 s for a result (one collective's limit plus the
start-up and the vote) and then terminates every child it started."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle
from conftest import ROOT, golden_assign_cases


def _worker(rank, world, port, case_idx, wide, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pkg = importlib.import_module("3d_gaussian_splatting_project_amd")
        name, pos, cams, segs, sizes, labels = golden_assign_cases()[case_idx]
        V = len(cams)
        lo, hi = pkg.dist.view_range(V, rank, world)
        total = 300 if wide else V                     # > 255 announces 16-bit counters
        shard = oracle.NumpyVoteShard(pos, cams[lo:hi], segs[lo:hi], sizes[lo:hi], 150, lo, total)
        got = pkg.dist.exchange_labels(pkg.dist.HostVoteShard(shard))
        q.put((rank, bool(np.array_equal(got, labels)), int((got != labels).sum())))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case_idx,wide", [(2, False), (3, False), (4, False), (2, True)])
def test_two_rank_exchange_equals_reference_labels(case_idx, wide):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() + case_idx * 7 + (3 if wide else 0)) % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, case_idx, wide, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok, _ in res), res


def _worker_sparse(rank, world, port, case_idx, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pkg = importlib.import_module("3d_gaussian_splatting_project_amd")
        name, pos, cams, segs, sizes, labels = golden_assign_cases()[case_idx]
        lo, hi = pkg.dist.view_range(len(cams), rank, world)
        shard = oracle.NumpySparseShard(pos, cams[lo:hi], segs[lo:hi], sizes[lo:hi], 150, world)
        got = pkg.dist.exchange_labels_sparse(pkg.dist.HostSparseShard(shard))
        q.put((rank, bool(np.array_equal(got, labels)), int((got != labels).sum())))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case_idx,world", [(2, 2), (3, 2), (4, 2), (3, 3)])
def test_sparse_tie_exchange_equals_reference_labels(case_idx, world):
    """Protocol v3 (counts-only all-to-all + sparse tie pass), incl. the ties fixture and 3 ranks."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + (os.getpid() + case_idx * 13 + world) % 2000
    procs = [ctx.Process(target=_worker_sparse, args=(r, world, port, case_idx, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok, _ in res), res


def _worker_a2a(rank, world, port, case_idx, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pkg = importlib.import_module("3d_gaussian_splatting_project_amd")
        name, pos, cams, segs, sizes, labels = golden_assign_cases()[case_idx]
        lo, hi = pkg.dist.view_range(len(cams), rank, world)
        shard = oracle.NumpySlabShard(pos, cams[lo:hi], segs[lo:hi], sizes[lo:hi], 150, world)
        got = pkg.dist.exchange_labels_a2a(pkg.dist.HostSlabShard(shard))
        q.put((rank, bool(np.array_equal(got, labels)), int((got != labels).sum())))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case_idx,world", [(2, 2), (3, 2), (4, 2), (3, 3)])
def test_all_to_all_exchange_equals_reference_labels(case_idx, world):
    """Protocol v2 (all-to-all -> slab arg-max -> all-gather of labels), incl. the ties fixture and 3 ranks."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() + case_idx * 11 + world) % 2000
    procs = [ctx.Process(target=_worker_a2a, args=(r, world, port, case_idx, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok, _ in res), res


def _worker_gather(rank, world, port, case_idx, product_packer, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pkg = importlib.import_module("3d_gaussian_splatting_project_amd")
        name, pos, cams, segs, sizes, labels = golden_assign_cases()[case_idx]
        lo, hi = pkg.dist.view_range(len(cams), rank, world)
        # product_packer: the maps are packed by libgsx's own host packer (gsx_debug_host_pack, no GPU needed), i.e. the
        # bytes that really cross the fabric; otherwise by the oracle's numpy restatement of the layout
        labeler = importlib.import_module("3d_gaussian_splatting_project_amd.labeler")
        pack = (lambda seg: labeler.host_pack(seg, 150, threads=2)[0]) if product_packer else None
        shard = oracle.NumpyGatherShard(pos, cams[lo:hi], segs[lo:hi], sizes[lo:hi], 150, pack=pack)
        got = pkg.dist.exchange_labels_gather(pkg.dist.HostGatherShard(shard), cap_views=len(cams))
        out = np.empty(len(pos), np.int32)
        same = pkg.dist.exchange_labels_gather(pkg.dist.HostGatherShard(shard), out=out, cap_views=len(cams))
        q.put((rank, bool(np.array_equal(got, labels)) and same is out and bool(np.array_equal(out, labels)), int((got != labels).sum())))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case_idx,world,product_packer", [(2, 2, True), (3, 2, False), (4, 2, True), (3, 3, True), (0, 3, False)])
def test_gather_exchange_equals_reference_labels(case_idx, world, product_packer):
    """Protocol v4 (all-gather of the packed maps, Gaussian slabs, all-gather of labels), incl. the ties fixture, the
    mixed-geometry fixture (maps smaller than the image, camera size != image size), 3 ranks, and a rank WITHOUT any
    view (case 0 has one view: ranks 1 and 2 stage nothing)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35500 + (os.getpid() + case_idx * 17 + world) % 2000
    procs = [ctx.Process(target=_worker_gather, args=(r, world, port, case_idx, product_packer, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok, _ in res), res


def _worker_pipeline(rank, world, port, case_idx, chunks, q, uniform=False, local=False, spoil=-1):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pkg = importlib.import_module("3d_gaussian_splatting_project_amd")
        name, pos, cams, segs, sizes, labels = golden_assign_cases()[case_idx]
        lo, hi = pkg.dist.view_range(len(cams), rank, world)
        mine = slice(lo, hi - 1) if rank == spoil else slice(lo, hi)       # spoil: this rank stages one view less than its share
        shard = oracle.NumpyGatherShard(pos, cams[mine], segs[mine], sizes[mine], 150)
        kw = dict(cameras=cams, map_size=segs[0].shape[::-1], image_size=sizes[0]) if local else dict(assume_uniform=uniform)
        pipe = pkg.dist.GatherPipeline(pkg.dist.HostGatherShard(shard), len(cams), chunks=chunks, **kw)
        for _ in range(hi - lo):
            pipe.after_view()
        if rank == spoil:
            # the other ranks fall back to the plain gather; so does this one - whose labels then lack the view it dropped
            got = pipe.finish()
            q.put((rank, True, (0, pipe.stride, pipe.C, pipe.bounds)))
            return
        got = pipe.finish()
        want = labels if spoil < 0 else None
        q.put((rank, want is None or bool(np.array_equal(got, want)), (int((got != labels).sum()), pipe.stride, pipe.C, pipe.bounds)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case_idx,world,chunks", [(2, 2, 4), (2, 3, 2), (3, 2, 3), (3, 3, 8), (4, 2, 2), (0, 3, 4), (1, 2, 1)])
def test_pipelined_gather_equals_reference_labels(case_idx, world, chunks):
    """GatherPipeline: the chunked all-gathers overlapped with the hand-over.  Uneven blocks (8 views over 3 ranks, 6 over
    ... ), more chunks than views, a rank without views (case 0: one view, three ranks), the ties fixture, and the
    mixed-geometry fixture (case 4), where the strides disagree and every rank must fall back to the plain gather together."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 37500 + (os.getpid() + case_idx * 19 + world * 3 + chunks) % 2000
    procs = [ctx.Process(target=_worker_pipeline, args=(r, world, port, case_idx, chunks, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok, _ in res), res
    strides = {info[1] for _, _, info in res}
    assert len(strides) == 1                      # every rank took the same decision
    if case_idx == 4:
        assert strides == {0}                     # mixed geometries: the fallback
    elif case_idx != 0:
        assert strides != {0}                     # uniform maps: really pipelined


@pytest.mark.parametrize("case_idx,world", [(2, 2), (3, 3), (0, 3)])
def test_pipelined_gather_without_the_agreement_collective(case_idx, world):
    """assume_uniform=True: every rank derives the stride from its own first map and the agreement all_gather is skipped -
    unless some rank owns no view (case 0: one view, three ranks), which every rank can tell from (total, world) alone,
    so all of them run the agreement after all and the collective sequences still match."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 39500 + (os.getpid() + case_idx * 23 + world) % 2000
    procs = [ctx.Process(target=_worker_pipeline, args=(r, world, port, case_idx, 3, q, True)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok, _ in res), res
    assert len({info[1] for _, _, info in res}) == 1


def test_view_range_is_contiguous_and_ordered():
    pkg = importlib.import_module("3d_gaussian_splatting_project_amd")
    for total in (1, 7, 8, 200, 1601):
        for world in (1, 2, 3, 8):
            spans = [pkg.dist.view_range(total, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == total
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            assert max(h - l for l, h in spans) - min(h - l for l, h in spans) <= 1


def test_single_process_exchange_is_identity():
    """world == 1: the protocol degenerates to a local arg-max and still equals the reference."""
    pkg = importlib.import_module("3d_gaussian_splatting_project_amd")
    name, pos, cams, segs, sizes, labels = golden_assign_cases()[3]
    shard = oracle.NumpyVoteShard(pos, cams, segs, sizes, 150, 0, len(cams))
    assert np.array_equal(pkg.dist.exchange_labels(pkg.dist.HostVoteShard(shard)), labels)
    g = oracle.NumpyGatherShard(pos, cams, segs, sizes, 150)
    assert np.array_equal(pkg.dist.exchange_labels_gather(pkg.dist.HostGatherShard(g)), labels)


@pytest.mark.parametrize("case_idx,world,chunks", [(2, 2, 4), (2, 3, 2), (3, 2, 3), (3, 3, 8), (1, 2, 1), (1, 3, 4)])
def test_pipelined_gather_with_locally_derived_views(case_idx, world, chunks):
    """GatherPipeline(cameras=..., map_size=...): no header exchange - every rank derives all descriptors from the shared camera
    list (gsx_vote_import_uniform; here its numpy stand-in) and the chunk schedule has a short last chunk."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 41500 + (os.getpid() + case_idx * 29 + world * 5 + chunks) % 2000
    procs = [ctx.Process(target=_worker_pipeline, args=(r, world, port, case_idx, chunks, q, False, True)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok, _ in res), res
    assert {info[1] for _, _, info in res} != {0} and len({info[1] for _, _, info in res}) == 1


def test_locally_derived_views_fall_back_together_when_a_rank_is_short():
    """A rank that staged fewer views than its share raises its flag in the 4-byte flag gather; every rank reads the flags next
    to the labels and all of them run the plain gather - nobody hangs, nobody returns labels built on a wrong schedule."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    world, port = 2, 43500 + os.getpid() % 2000
    procs = [ctx.Process(target=_worker_pipeline, args=(r, world, port, 2, 3, q, False, True, 1)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok, _ in res), res


# ---- GatherPipeline with locally derived views (cameras + map_size): what a rank staged must never shape a collective ----------
# Every worker below passes COLLECTIVE_TIMEOUT_S to init_process_group, so a rank that meets a protocol mismatch fails instead of
# sitting in a collective; the parent waits PARENT_TIMEOUT_S for each result and then terminates every child it started.
def _resample(seg, w, h):
    """nearest-neighbour copy of a class map at another size (w, h)"""
    H, W = seg.shape
    return np.ascontiguousarray(seg[(np.arange(h) * H // h)[:, None], (np.arange(w) * W // w)[None, :]])


def _sizes_with_average_stride(W, H):
    """two map sizes, one smaller and one larger than (W, H), whose pool strides average to the stride of a (W, H) map: a rank
    that stages them in place of two (W, H) maps has an irregular pool whose bytes still are views x a multiple of 256"""
    S = oracle.map_stride_numpy
    for w1 in range(16, 2 * W, 16):
        for h1 in range(8, 2 * H, 8):
            if S(w1, h1) >= S(W, H):
                continue
            for w2 in range(W, 2 * W, 16):
                for h2 in range(H - H % 8, 2 * H, 8):
                    if S(w1, h1) + S(w2, h2) == 2 * S(W, H):
                        return (w1, h1), (w2, h2)
    return None


def _scenario_inputs(spec, world):
    """-> pos, cameras (the list every rank holds), per-view maps, per-view image sizes (what the ranks really stage), the
    map_size and image_size handed to every GatherPipeline, the labels every rank must return.
    The labels are the reference's own (tests/golden/vote_assign.npz) wherever the staged views are a golden case's.  Where a
    scenario changes the maps or the image sizes there is no reference-made golden for that input (the fixtures were written
    once, by the reference, for five inputs): there the arbiter is oracle.assign_labels on the very maps the ranks stage, which
    test_oracle_vote.py pins to the reference's labels bit for bit on all golden cases."""
    pkg = importlib.import_module("3d_gaussian_splatting_project_amd")
    name, pos, cams, segs, sizes, labels = golden_assign_cases()[spec["case"]]
    cams, segs, sizes = [dict(c) for c in cams], list(segs), [tuple(int(v) for v in sz) for sz in sizes]
    H, W = segs[0].shape
    map_size, image_size, kind, changed = (W, H), sizes[0], spec["kind"], False
    odd = spec.get("odd", -1)
    lo, hi = pkg.dist.view_range(len(cams), odd, world) if odd >= 0 else (0, 0)
    if kind == "half":                                  # b: one rank's maps at half resolution, its image size kept
        for v in range(lo, hi):
            segs[v] = np.ascontiguousarray(segs[v][::2, ::2])
        changed = True
    elif kind == "average":                             # c: irregular own pool, bytes still views x (a multiple of 256)
        pair = _sizes_with_average_stride(W, H)
        assert pair is not None and hi - lo >= 2
        segs[lo], segs[lo + 1] = _resample(segs[lo], *pair[0]), _resample(segs[lo + 1], *pair[1])
        own = [oracle.map_stride_numpy(*s.shape[::-1]) for s in segs[lo:hi]]
        assert sum(own) == (hi - lo) * oracle.map_stride_numpy(W, H) and len(set(own)) > 1
        changed = True
    elif kind == "swapped":                             # d: (H, W) for (W, H) on a non-square map
        assert W != H
        map_size, image_size = (H, W), None
    elif kind == "other_resolution":                    # d: a map_size of another resolution
        map_size, image_size = (W // 2, H // 2), sizes[0]
    elif kind in ("images_twice_the_maps", "wrong_image_size"):
        # images (and the cameras' frames) of twice the maps' size, uniformly; d: ... and the map size handed in as image size
        for c in cams:
            c["fx"], c["fy"], c["width"], c["height"] = 2 * c["fx"], 2 * c["fy"], 2 * c["width"], 2 * c["height"]
        sizes = [(2 * a, 2 * b) for a, b in sizes]
        image_size = sizes[0] if kind == "images_twice_the_maps" else (W, H)
        changed = True
    elif kind == "extra_view":                          # f: one rank stages a view more than the whole run has
        pass
    else:
        assert kind == "plain"
    want = oracle.assign_labels(pos, cams, segs, sizes, threads=1) if changed else labels
    return pos, cams, segs, sizes, map_size, image_size, want


def _expected_collectives(spec, world, n_gaussians, total):
    """the (numel, dtype) of every collective of a locally-derived-views run up to the labels, from (total_views, world, chunks,
    map_size) alone - the class docstring's promise - and whether an agreement gather precedes them"""
    pkg = importlib.import_module("3d_gaussian_splatting_project_amd")
    n = [b - a for a, b in (pkg.dist.view_range(total, r, world) for r in range(world))]
    bounds = pkg.dist.chunk_bounds(max(n), spec["chunks"])
    stride = oracle.map_stride_numpy(*spec["map_size"])
    seq = [((b - a) * stride, "torch.uint8") for a, b in zip(bounds, bounds[1:])]
    sn = ((n_gaussians + world - 1) // world + 255) // 256 * 256 or 256
    return seq + [(1, "torch.int32"), (sn, "torch.int32")], min(n) < 1


def _worker_local(rank, world, port, spec, q):
    import datetime
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=COLLECTIVE_TIMEOUT_S))
    try:
        pkg = importlib.import_module("3d_gaussian_splatting_project_amd")
        pos, cams, segs, sizes, map_size, image_size, want = _scenario_inputs(spec, world)
        lo, hi = pkg.dist.view_range(len(cams), rank, world)
        mine = list(range(lo, hi))
        if spec["kind"] == "extra_view" and rank == spec["odd"]:
            mine = list(range(len(cams))) + [0]                  # more views than the run announces: the plain gather's cap
        shard = oracle.NumpyGatherShard(pos, [cams[v] for v in mine], [segs[v] for v in mine], [sizes[v] for v in mine], 150)
        seen, inner = [], pkg.dist._all_gather_into

        def recording(full, part, group, async_op=False):        # every collective of the pipeline and of its fallback goes through here
            seen.append((int(part.numel()), str(part.dtype)))
            return inner(full, part, group, async_op=async_op)
        pkg.dist._all_gather_into = recording
        kw = {} if image_size is None else {"image_size": image_size}
        pipe = pkg.dist.GatherPipeline(pkg.dist.HostGatherShard(shard), len(cams), chunks=spec["chunks"], cameras=cams, map_size=map_size, **kw)
        for _ in range(hi - lo):
            pipe.after_view()
        out = np.full(len(pos), SENTINEL, np.int32)
        try:
            got = pipe.finish(out=out)
            res = ("labels", got is out, int((out != want).sum()))
        except ValueError as e:
            res = ("ValueError", bool((out == SENTINEL).all()), str(e)[:200])
        q.put((rank, res, seen))
    finally:
        dist.destroy_process_group()


SENTINEL = -77                  # no label: labels are -1 .. n_classes - 1
COLLECTIVE_TIMEOUT_S = 45      # see the module docstring
PARENT_TIMEOUT_S = 75


def _run_local(spec, world, port):
    """-> [(result, collectives)] by rank.  No child outlives the call, whatever happens."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_local, args=(r, world, port, spec, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted(q.get(timeout=PARENT_TIMEOUT_S) for _ in procs)
        for p in procs:
            p.join(timeout=30)
            assert p.exitcode == 0, p.exitcode
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(timeout=10)
            if p.is_alive():
                p.kill()
                p.join()
    assert [r for r, _, _ in res] == list(range(world))
    return [(r, seen) for _, r, seen in res]


PIPELINED, FALLBACK, FALLBACK_RAISES = 0, 3, 1        # collectives behind the labels gather: none; header, pools, labels; header


def _check_local(spec, world, port, after_labels):
    """One run of `spec` on `world` ranks.  Every rank: the reference's labels in `out`, bit for bit; the same sequence of
    collectives (test e); that sequence = what (total_views, world, chunks, map_size) alone give, up to the labels gather, where
    the flags are known, whether the run ends there (PIPELINED) or goes on into the plain gather (FALLBACK: its header, pool
    and labels gathers; FALLBACK_RAISES: the header gather, whose check raises)."""
    pos, cams, segs, sizes, map_size, image_size, want = _scenario_inputs(spec, world)
    res = _run_local(spec, world, port)
    seqs = [seen for _, seen in res]
    assert all(s == seqs[0] for s in seqs), seqs                                # every rank joined the same collectives
    head, agreement = _expected_collectives(dict(spec, map_size=map_size), world, len(pos), len(cams))
    if agreement:                                                               # some rank owns no view: the strides' gather comes first
        assert seqs[0][:1] == [(1, "torch.int64")], seqs[0]
    rest = seqs[0][1:] if agreement else seqs[0]
    assert rest[:len(head)] == head, (rest, head)
    assert len(rest) == len(head) + after_labels, (after_labels, rest)          # every rank took the decision expected here
    return res


def _labels_ok(res):
    for rank, (r, _) in enumerate(res):
        assert r[0] == "labels" and r[1] and r[2] == 0, (rank, r)


@pytest.mark.parametrize("case_idx,world,chunks", [(2, 2, 4), (2, 3, 2), (3, 2, 3), (3, 3, 8), (1, 2, 1), (0, 3, 4)])
def test_local_views_collective_sequence_is_pinned(case_idx, world, chunks):
    """e, from the uniform side: a run that stays pipelined issues the C chunk gathers, the flag gather and the labels gather with
    the sizes (total_views, world, chunks, map_size) give, nothing else (case 0, one view on three ranks: the agreement gather of
    the strides in front, as before), the same on every rank."""
    _labels_ok(_check_local({"case": case_idx, "chunks": chunks, "kind": "plain"}, world,
                            45500 + (os.getpid() + case_idx * 31 + world * 7 + chunks) % 2000, PIPELINED))


def test_local_views_with_images_larger_than_the_maps():
    """image_size != map_size, handed in correctly: stays pipelined (the own-view check compares the scales too)."""
    _labels_ok(_check_local({"case": 2, "chunks": 2, "kind": "images_twice_the_maps"}, 2, 47400 + os.getpid() % 90, PIPELINED))


@pytest.mark.parametrize("world,chunks", [(2, 1), (2, 3), (3, 1), (3, 3)])
def test_local_views_mixed_geometry_falls_back_together(world, chunks):
    """a: the mixed-geometry fixture (case 4) with locally derived views: the ranks whose maps are not of map_size lower their
    flags, every rank joins every collective and all take the plain gather: the reference's labels, nobody hangs."""
    _labels_ok(_check_local({"case": 4, "chunks": chunks, "kind": "plain"}, world, 47500 + (os.getpid() + world * 5 + chunks) % 400,
                            FALLBACK))


@pytest.mark.parametrize("case_idx,world,odd,chunks", [(2, 3, 0, 2), (2, 3, 1, 4), (3, 3, 2, 2), (2, 2, 0, 4), (3, 2, 1, 2)])
def test_local_views_one_rank_at_half_resolution(case_idx, world, odd, chunks):
    """b: one rank's maps at half resolution (seg[::2, ::2], image size kept), first, middle and last rank in turn.  The labels
    are the oracle's on the very maps staged (see _scenario_inputs for why no reference-made golden exists for this input)."""
    _labels_ok(_check_local({"case": case_idx, "chunks": chunks, "kind": "half", "odd": odd}, world,
                            47900 + (os.getpid() + case_idx * 3 + world * 11 + odd * 5 + chunks) % 400, FALLBACK))


@pytest.mark.parametrize("world,odd,chunks", [(2, 1, 2), (3, 0, 3)])
def test_local_views_irregular_pool_with_a_regular_average(world, odd, chunks):
    """c: two of one rank's maps have other sizes whose strides average to the common one (320x180: 16x24 and 416x280), so
    its pool bytes are views x stride although no view lies where the schedule puts it: bytes / views is not a uniformity test."""
    _labels_ok(_check_local({"case": 2, "chunks": chunks, "kind": "average", "odd": odd}, world,
                            48300 + (os.getpid() + world * 11 + odd * 5 + chunks) % 400, FALLBACK))


@pytest.mark.parametrize("kind,case_idx,world,chunks", [("swapped", 2, 2, 2), ("swapped", 3, 3, 3), ("other_resolution", 2, 3, 2),
                                                         ("other_resolution", 3, 2, 4), ("wrong_image_size", 2, 2, 3),
                                                         ("wrong_image_size", 3, 3, 2)])
def test_local_views_wrong_sizes_on_every_rank(kind, case_idx, world, chunks):
    """d: every rank is handed the same wrong map_size ((H, W) for (W, H); half the resolution) or image_size (the map size, for
    images twice as large): no rank's own views match what it would derive, all fall back and return the right labels -
    the collectives up to the flags are those the WRONG map_size gives, on every rank alike."""
    _labels_ok(_check_local({"case": case_idx, "chunks": chunks, "kind": kind}, world,
                            48700 + (os.getpid() + len(kind) * 13 + case_idx * 3 + world * 11 + chunks) % 400, FALLBACK))


@pytest.mark.parametrize("world,odd", [(2, 1), (3, 0)])
def test_local_views_out_is_untouched_when_the_fallback_raises(world, odd):
    """f: one rank staged more views than the run announces, so the run falls back and the plain gather's header check raises
    the same ValueError on every rank.  The caller's `out` still holds what it held: the pipelined attempt's labels, voted before
    the flags were known, never reached it."""
    res = _check_local({"case": 2, "chunks": 3, "kind": "extra_view", "odd": odd}, world, 49100 + (os.getpid() + world * 11 + odd) % 400,
                       FALLBACK_RAISES)
    for rank, (r, _) in enumerate(res):
        assert r[0] == "ValueError" and "cap_views" in r[2], (rank, r)
        assert r[1], f"rank {rank}: out was written before the flags were known"


def test_chunk_bounds():
    pkg = importlib.import_module("3d_gaussian_splatting_project_amd")
    cb = pkg.dist.chunk_bounds
    assert cb(25, 4) == [0, 7, 14, 22, 25] and cb(0, 4) == [0] and cb(1, 4) == [0, 1] and cb(3, 8) == [0, 1, 2, 3]
    for n in range(1, 300):
        for c in (1, 2, 3, 4, 8):
            b = cb(n, c)
            assert b[0] == 0 and b[-1] == n and all(x < y for x, y in zip(b, b[1:])) and len(b) - 1 <= max(c, 1) + (n < 2 * c) * n
