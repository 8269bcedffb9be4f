"""GPU: the four multi-rank vote exchanges (dist.py, include/gsx.h: v1 all-reduce of the planes, v2 all-to-all of both planes, v3
counts + sparse tie pass, v4 gather of the maps) against the rank-split model of tests/exchange_model.py, on constructed votes that
meet the kernels' constants: candidate words of 32 bins, slabs of ceil(ceil(n / W) / 256) * 256 Gaussians, ranks without views, rank
counters at 255, totals above 255, 16-bit planes from 256 views on, a rank's own second batch, the tie order across ranks.
tests/test_exchange_model.py has shown on the CPU that the oracle's stand-ins compute the same arrays from the same scenes.

One process; `world` contexts on device 0 play the ranks and the collectives are torch slices and torch.cat, as in the
*_exchange_on_one_gpu tests of test_vote_gpu.py.  With spatial_sort 0 every intermediate (count words, planes, candidate masks,
tie codes, slab labels with their -2) is compared with np.array_equal; with the Morton sort on, whose permutation the library does
not expose, the final labels and the slab size.  Pad entries (positions >= n of a slab) are compared where the library documents
them: count planes and tie codes are zero there.  Integer work: no tolerance anywhere."""
import contextlib

import numpy as np
import pytest

import exchange_model as xm
import vote_cases as vc

pytestmark = pytest.mark.gpu

BASE_SETS = [{}, {"spatial_sort": 0}]
KERNEL_SETS = [{"flat_project": 0}, {"vote_unroll": 2}, {"seg_coarse": 0}, {"wave_cull": 0}]    # other count and plane kernels


def _id(opts):
    return "-".join(f"{k}{v}" for k, v in opts.items()) or "defaults"


def _sync(*ctxs):
    """The hand-made collectives run on torch's stream, the library on its contexts' streams: fence both."""
    import torch
    for c in ctxs:
        c.synchronize()
    torch.cuda.synchronize()


@contextlib.contextmanager
def _ranks(gsx, opts):
    """get(world) -> that many contexts with the options set; made when first asked for, closed at the end of the test."""
    made = []

    def get(world):
        while len(made) < world:
            c = gsx.Context(0)
            made.append(c)
            for k, v in opts.items():
                c.set_option(k, v)
        return made[:world]
    try:
        yield get
    finally:
        for c in made:
            c.close()


def _launches(c, name):
    return c.profile_get(name)[0] if name in c.profile_names() else 0


def _same(got, want, *what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shapes {got.shape} and {want.shape}"
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} differ, first at {np.flatnonzero(got.reshape(-1) != want.reshape(-1))[:8].tolist()}"


def _stage(ctxs, case, world, phase, slabs, local, mixed=False):
    """Every rank's block of views into its context.  mixed: host and device hand-over alternate by view."""
    import torch
    pos, cams, segs, sizes = case.scene(phase)
    V = len(cams)
    m = xm.xmodel(case, world)
    for r, c in enumerate(ctxs):
        c.set_option("exchange_slabs", slabs)
        c.set_option("exchange_local", local)
        c.set_option("early_vote", 0)                  # a rank of a multi-rank run never votes early (dist._GpuShard.hold)
        c.profile(True)
        c.upload_positions(pos)
        c.vote_begin(case["n_classes"], m["ranks"][r]["first_view"], V)
        lo, hi = m["spans"][r]
        for v in range(lo, hi):
            seg = torch.from_numpy(segs[v]).cuda() if mixed and (v + r) % 2 else segs[v]
            c.vote_view(cams[v], seg, sizes[v])
        assert c.vote_num_views() == hi - lo


def _a2a(parts, r, world):
    """What rank r holds after all_to_all_single over flat tensors of `world` equal chunks."""
    import torch
    ch = parts[0].numel() // world
    return torch.cat([parts[s][r * ch:(r + 1) * ch] for s in range(world)])


def run_v1(gsx, ctxs, case, world, phase, plain):
    import torch
    m = xm.xmodel(case, world)
    n, what = m["n"], (case["name"], world, phase, "v1")
    _stage(ctxs, case, world, phase, 1, 0)
    shards = [gsx.dist.GpuVoteShard(c) for c in ctxs]
    counts = [sh.counts_tensor() for sh in shards]
    _sync(*ctxs)
    if plain:
        for r in range(world):
            _same(counts[r].cpu().numpy(), m["v1"]["words"][r], *what, "count words", r)
            cnt, fv = ctxs[r].debug_planes(case["bins"])
            _same(fv, m["v1"]["fv"][r], *what, "first views", r)
    total = counts[0].clone()
    for t in counts[1:]:
        total += t                                     # == all_reduce(SUM) over the int32-packed counters
    if plain:
        _same(total.cpu().numpy(), m["v1"]["sum"], *what, "sum")
    for t in counts:
        t.copy_(total)
    _sync()
    keys = [sh.compute_keys() for sh in shards]
    _sync(*ctxs)
    if plain:
        for r in range(world):
            _same(keys[r].cpu().numpy()[:n], m["v1"]["keys"][r][:n], *what, "keys", r)
    kmax = keys[0].clone()
    for k in keys[1:]:
        kmax = torch.maximum(kmax, k)                  # == all_reduce(MAX)
    if plain:
        _same(kmax.cpu().numpy()[:n], m["v1"]["max"][:n], *what, "max")
    for k in keys:
        k.copy_(kmax)
    _sync()
    for r, c in enumerate(ctxs):
        _same(shards[r].labels(), m["labels"], *what, "labels", r)
        lo, hi = m["spans"][r]
        assert _launches(c, "vote_fused_planes") == (-(-(hi - lo) // vc.MAX_BATCH) if n else 0) and _launches(c, "vote_keys") == (1 if n else 0)


def run_v2(gsx, ctxs, case, world, phase, plain):
    import torch
    m = xm.xmodel(case, world)
    what = (case["name"], world, phase, "v2")
    _stage(ctxs, case, world, phase, world, 1)
    shards = [gsx.dist.GpuSlabShard(c) for c in ctxs]
    planes = [sh.planes() for sh in shards]
    _sync(*ctxs)
    for r, c in enumerate(ctxs):
        assert c.slab_size() == m["sn"]
        cnt = planes[r][0].cpu().numpy().view(np.uint8).reshape(world, case["bins"], -1)
        ins = np.broadcast_to(m["inside"][:, None, :], cnt.shape)
        assert not cnt[~ins].any(), (*what, "pad Gaussians hold counts", r)     # in any order of the Gaussians
        if plain:
            _same(cnt, m["v2"]["cnt"][r], *what, "counts", r)
            _same(planes[r][1].cpu().numpy().view(np.uint8).reshape(cnt.shape)[ins], m["v2"]["fv"][r][ins], *what, "first views", r)
    slabs = []
    for r, c in enumerate(ctxs):
        rc, rf = _a2a([p[0] for p in planes], r, world), _a2a([p[1] for p in planes], r, world)
        _sync()
        t = shards[r].reduce(rc, rf)
        _sync(c)
        slabs.append(t.clone())
        assert t.numel() == m["sn"] and _launches(c, "vote_slab_reduce") == 1
        if plain:
            ins = m["inside"][r]
            _same(slabs[r].cpu().numpy()[ins], m["v2"]["slabs"][r][ins], *what, "slab labels", r)
    full = torch.cat(slabs)                            # == all_gather
    _sync()
    for r in range(world):
        _same(shards[r].finish(full), m["labels"], *what, "labels", r)


def run_v3(gsx, ctxs, case, world, phase, plain):
    import torch
    m = xm.xmodel(case, world)
    n, sn, what = m["n"], m["sn"], (case["name"], world, phase, "v3")
    _stage(ctxs, case, world, phase, world, 1)
    shards = [gsx.dist.GpuSparseShard(c) for c in ctxs]
    cnts = [sh.counts() for sh in shards]
    _sync(*ctxs)
    cands = []
    for r, c in enumerate(ctxs):
        assert c.slab_size() == sn
        if plain:
            _same(cnts[r].cpu().numpy().view(np.uint8), m["v3"]["cnt"][r].reshape(-1), *what, "counts", r)
        rc = _a2a(cnts, r, world)
        _sync()
        t = shards[r].totals(rc)
        _sync(c)
        cands.append(t.clone())
        if plain:
            ins = m["inside"][r]
            _same(cands[r].cpu().numpy().view(np.uint32).reshape(xm.CAND_WORDS, sn)[:, ins], m["v3"]["masks"][r][:, ins], *what, "masks", r)
            kp, _ = c.keys_device()
            tied = gsx.dist.device_words_tensor(kp, sn, 0).cpu().numpy()
            _same(tied[ins], m["v3"]["tied"][r][ins], *what, "labels with ties", r)
    cand_all = torch.cat(cands)                        # == all_gather
    _sync()
    codes = []
    for r, c in enumerate(ctxs):
        t = shards[r].tie_codes(cand_all)
        _sync(c)
        codes.append(t.clone())
        if plain:
            _same(codes[r].cpu().numpy().view(np.uint16), m["v3"]["codes"][r], *what, "tie codes", r)
    slabs = []
    for r, c in enumerate(ctxs):
        rcodes = _a2a(codes, r, world)
        _sync()
        t = shards[r].resolve(rcodes)
        _sync(c)
        slabs.append(t.clone())
        got = slabs[r].cpu().numpy()
        assert not (got == -2).any(), (*what, r)
        if plain:
            ins = m["inside"][r]
            _same(got[ins], m["v3"]["slabs"][r][ins], *what, "slab labels", r)
        assert _launches(c, "vote_fused_counts") == (1 if n else 0) and _launches(c, "vote_slab_totals") == 1
        assert _launches(c, "vote_tie") == (1 if n else 0) and _launches(c, "vote_tie_resolve") == 1
    full = torch.cat(slabs)
    _sync()
    for r in range(world):
        _same(shards[r].finish(full), m["labels"], *what, "labels", r)


def one_geometry(case):
    v0 = case["views"][0]
    return all(vw["map_shape"] == v0["map_shape"] and vw["img_size"] == v0["img_size"] for vw in case["views"])


def run_v4(gsx, ctxs, case, world, phase, plain, uniform=False):
    import torch
    m = xm.xmodel(case, world)
    n, sn, what = m["n"], m["sn"], (case["name"], world, phase, "v4")
    _, cams, segs, sizes = case.scene(phase)
    V = len(cams)
    _stage(ctxs, case, world, phase, 1, 0, mixed=True)
    shards = [gsx.dist.GpuGatherShard(c) for c in ctxs]
    heads = [sh.header(max(1, V)).cpu().numpy() for sh in shards]
    counts = np.stack([h[:16].copy().view(np.int64) for h in heads])
    assert counts[:, 0].tolist() == [hi - lo for lo, hi in m["spans"]]
    chunk = max(256, int(counts[:, 1].max()))
    blobs = np.concatenate([heads[r][16:16 + 256 * counts[r, 0]] for r in range(world)])
    pools = [sh.pool(chunk) for sh in shards]
    _sync(*ctxs)
    pool_all = torch.cat([p.clone() for p in pools])   # == all_gather of the pools
    _sync()
    part_views, offs = counts[:, 0].astype(np.int32), np.arange(world, dtype=np.int64) * chunk
    S = -(-V // vc.MAX_BATCH)
    for how in ("blobs", "uniform") if uniform else ("blobs",):
        slabs = []
        for r, c in enumerate(ctxs):
            c.profile(True)
            if how == "uniform":
                shards[r].undo_import()
                assert c.vote_num_views() == counts[r, 0]
                shards[r].import_uniform(part_views, offs, cams, (segs[0].shape[1], segs[0].shape[0]), sizes[0], pool_all)
            else:
                shards[r].import_all(part_views, offs, blobs, pool_all)
            assert c.vote_num_views() == V
            t = shards[r].slab_labels(r, world)
            _sync(c)
            slabs.append(t.clone())
            a, b = m["v4"]["slices"][r]
            assert t.numel() == sn
            if plain:
                _same(slabs[r].cpu().numpy()[:b - a], m["v4"]["slabs"][r], *what, how, "slab labels", r)
            if V <= vc.MAX_BATCH:
                assert _launches(c, "vote_fused_labels") == (1 if b > a else 0) and _launches(c, "vote_slab_totals") == 0
            else:
                assert _launches(c, "vote_fused_counts") == (S if b > a else 0) and _launches(c, "vote_tie") == (S if b > a else 0)
                assert _launches(c, "vote_slab_totals") == _launches(c, "vote_tie_resolve") == (1 if b > a else 0)
        full = torch.cat(slabs)                        # == all_gather of the labels
        _sync()
        for r in range(world):
            _same(shards[r].finish(full), m["labels"], *what, how, "labels", r)
    # an imported context holds every view: a plain finalize on it is the single-GPU result
    _same(ctxs[world - 1].vote_finalize(), m["labels"], *what, "finalize after the import")


RUN = {"v1": run_v1, "v2": run_v2, "v3": run_v3, "v4": run_v4}


def run_case(gsx, get, opts, case, protocols=None, worlds=None):
    plain = opts.get("spatial_sort", 1) == 0
    for world in (case["worlds"] if worlds is None else worlds):
        ctxs = get(world)
        m = xm.xmodel(case, world)
        for phase in vc.PHASES:
            for p in (case["protocols"] if protocols is None else protocols):
                if p not in m:
                    continue
                if p == "v4":
                    run_v4(gsx, ctxs, case, world, phase, plain, uniform=case["family"] in ("x1", "x2") and one_geometry(case))
                else:
                    RUN[p](gsx, ctxs, case, world, phase, plain)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("opts", BASE_SETS + KERNEL_SETS, ids=_id)
def test_ranks_and_views(gsx, opts, world):
    """X1: 1, 2, 3 and 8 ranks over 1 .. 17 views: ranks without a view (first_view = min(lo, total - 1)), a rank with one; tied
    maxima and abstentions."""
    with _ranks(gsx, opts) as get:
        for case in xm.cases_of("x1"):
            assert world in case["worlds"]
            run_case(gsx, get, opts, case, worlds=(world,))


@pytest.mark.parametrize("opts", BASE_SETS, ids=_id)
def test_slab_geometry(gsx, opts):
    """X2: n at 1, 255 .. 257 and 256 W - 1 .. 256 W + 1 for 2, 3 and 8 ranks: empty slabs, a slab of one Gaussian under the
    four-a-thread totals kernel, a slab boundary on n; every Gaussian an answer of its own."""
    with _ranks(gsx, opts) as get:
        for case in xm.cases_of("x2"):
            run_case(gsx, get, opts, case)


@pytest.mark.parametrize("opts", BASE_SETS, ids=_id)
def test_candidate_words(gsx, opts):
    """X3: maximal bins in every word of the candidate mask alone, across the words (0, 7) and (3, 4), on bits 0 and 31; decoys one
    vote below in the words before and after; early words that a later word overtakes."""
    with _ranks(gsx, opts) as get:
        for case in xm.cases_of("x3"):
            run_case(gsx, get, opts, case)


@pytest.mark.parametrize("opts", BASE_SETS, ids=_id)
def test_tie_order_across_ranks(gsx, opts):
    """X4: 3 and 8 ranks, 5 and 255 classes; the winner first voted by rank 0, 1 or the last one, in the first or the last local
    view, the larger or the smaller bin, bin 0 and bin 255; rank 0 with votes for non-candidates only, and with none."""
    with _ranks(gsx, opts) as get:
        for case in xm.cases_of("x4"):
            run_case(gsx, get, opts, case)


@pytest.mark.parametrize("opts", BASE_SETS + KERNEL_SETS, ids=_id)
def test_counters(gsx, opts):
    """X5: a rank counter of 255 and a candidate first voted in local view 254; totals of 256 and 264 out of u8 rank counters; v1's
    packed SUM at 255 a byte, 16-bit planes with first_view > 0 at 256 views, a rank whose own second batch merges into them."""
    with _ranks(gsx, opts) as get:
        for case in xm.cases_of("x5"):
            run_case(gsx, get, opts, case)


@pytest.mark.parametrize("opts", BASE_SETS, ids=_id)
def test_workgroup_order(gsx, opts):
    """X6: grids of 7 .. 33 workgroups under every xcd_swizzle, for the kernels that go through logical_block in v3 and v4."""
    with _ranks(gsx, opts) as get:
        for swizzle in (0, 1, 2, 3):
            for c in get(2):
                c.set_option("xcd_swizzle", swizzle)
            for case in xm.cases_of("x6"):
                run_case(gsx, get, opts, case)


def test_pad_entries_after_a_larger_scene(gsx):
    """Contexts that come back with a smaller scene, and with another slab count for the same one: the count plane and the tie
    codes of v3 are zero at the pad entries again, whatever the earlier runs left in the buffers."""
    big, small = (next(c for c in xm.cases_of("x6") if c["name"] == nm) for nm in ("x6-g14", "x6-g6"))
    x1 = next(c for c in xm.cases_of("x1") if c["name"] == "x1-V9")
    with _ranks(gsx, {"spatial_sort": 0}) as get:
        for case, world in ((big, 2), (small, 2), (x1, 2), (x1, 1), (x1, 3)):
            run_v3(gsx, get(3)[:world], case, world, 0.5, True)


def test_rank_counter_limit(gsx):
    """X5 (a): under exchange_local a rank's 256th view is refused (GSX_E_RANGE) and stages nothing; the context goes on to the
    next run."""
    case = next(c for c in xm.cases_of("x5") if c["name"] == "x5a-255+1")
    _, cams, segs, sizes = case.scene(0.5)
    with _ranks(gsx, {"spatial_sort": 0}) as get:
        ctxs = get(2)
        _stage(ctxs, case, 2, 0.5, 2, 1)
        c = ctxs[0]
        before = (c.vote_num_views(), c.vote_pool_bytes())
        assert before[0] == 255
        with pytest.raises(ValueError, match="at most 255 views per rank"):
            c.vote_view(cams[255], segs[255], sizes[255])
        assert (c.vote_num_views(), c.vote_pool_bytes()) == before
        run_v3(gsx, ctxs, case, 2, 0.5, True)
