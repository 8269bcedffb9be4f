"""GPU: the compact hand-over of host maps (csrc/handover.hip: hand_over_compact, vote_flush_pending, seg_expand_kernel - the default
path of gsx_vote_view with a host pointer, and the one the benchmark times) and the pool-form ring beside it (hand_over_pool_form)
pinned byte for byte to the numpy model of the pool form (tests/segpool_model.py), padding, gaps and unread coarse cells included.

Every run starts on a pool filled with 0xA5 (tests/segpool_rig.py) and every comparison is M.check_map over the whole stride of every
map: nothing has a tolerance.  The inputs go through the host chain on the CPU in tests/test_segpool_model.py (host packer ->
oracle.expand_compact_numpy == the model), so a mismatch here is the expansion kernel's or the driver's.  Where a case relies on a
unit of the source (threads per workgroup, slots and records per group of the pinned ring) it takes it from segpack_constants() and
asserts the relation it relies on.

Measured on an MI355X: the file's 33 tests take 2.6 s of wall time, pytest's start included; the slowest test 0.24 s.

Mutants of seg_expand_kernel, each built in a scratch copy, run once against this file and never committed; all of them read a lower
or clamped block index or skip a store, so they stay inside the allocations.  What failed:
  - `before` starts at 0 instead of `running` (the second round of a cell row ranks from 0): the rank cases 5, 6 and 8 - not 1 to 4,
    whose second round has no mixed cell, and not 7, whose first round has none -, 1040 x 9, every width above 1024 (1028 x 8 and x 9,
    2044 x 5, 2048 x 8, 2052 x 5, 4100 x 4), 65535 x 1, the four dtype tests (1028 x 9) and the first run of the two-run test.
  - the wave prefix taken as k <= wv, the clamp kept: 30 of 33 - all but 1 x 65535 (one cell to a row: the clamp sets the index right) and the
    two pool-form tests.
  - the coarse copy without its stride loop: 2052 x 5, 4100 x 4 and 65535 x 1, the three maps with more than 256 pieces per band.
  - the two gap loops removed: 23 of 33 - every test with a map whose levels do not end on a 256-byte boundary (all rank cases, 1040 x 9,
    1028 x 8 and x 9, 2052 x 5, 4100 x 4, the edge shapes, the dtype, group, flush, two-geometry and two-run tests).
  - the two cell rows of a band swapped in the output offset: 31 of 33 - everything but the two pool-form tests.
"""
import numpy as np
import pytest

import segpool_model as M
from segpool_rig import CAM, N_CLASSES, Rig, compact_layout, dev

pytestmark = pytest.mark.gpu

THREADS = (1, 3, 16)                 # packer threads: the order of the blocks in a record's stream differs, the pool must not


@pytest.fixture(scope="module")
def K(gsx):
    """the units the expansion and its driver are built on, exported from the source (gsx_debug_segpack_constants)"""
    k = gsx.segpack_constants()
    assert (k["strip_cols"], k["band_rows"], k["cstrip_cells"], k["cband_rows"]) == (M.STRIP_COLS, M.BAND_ROWS, M.CSTRIP_CELLS, M.CBAND_ROWS)
    assert 1 < k["dma_batch"] < k["compact_batch"]
    return k


def cells_per_row(w):
    """cells of a cell row as the expansion walks it: padded to whole strips of 16 pixel columns"""
    return (w + M.STRIP_COLS - 1) // M.STRIP_COLS * (M.STRIP_COLS // M.CELL)


def noise_maps(w, h, dtype="i32", n_classes=N_CLASSES, seed=0, count=len(M.NOISE)):
    """[(map, packed_u8)]: M.NOISE content - uniform blocks, lightly and heavily mixed -, cycling when more maps are asked for; with
    the defaults the maps tests/test_segpool_model.py sends through the host chain"""
    rng = np.random.default_rng(w * 100_003 + h + 7 * seed)
    return [M.as_dtype(M.blocky_labels(rng, w, h, n_classes, M.NOISE[v % len(M.NOISE)], 0 if dtype == "u8" else -1), dtype) for v in range(count)]


def host_stage(maps, after=None):
    """every map handed over as a host array; after(c, v) runs behind map v"""
    def stage(c):
        for v, (arr, packed) in enumerate(maps):
            c.vote_view(CAM, arr, packed_u8=packed)
            if after is not None:
                after(c, v)
    return stage


def record_sum(maps, n_classes=N_CLASSES):
    return sum(M.record_bytes(a, compact_layout(a.shape[1], a.shape[0], n_classes)[2], p) for a, p in maps)


def handed(r, K, maps, stage=None, tail=False, n_classes=N_CLASSES, device_maps=0, what=""):
    """one run of host maps on the dirtied pool, announced with room behind the maps (no run tail: groups fill) or exactly (tail: the last
    dma_batch - 1 maps go up one by one) -> (pool, seg_expand launches, link bytes); every stride has been checked against the model"""
    before = r.launches("seg_expand")
    pool = r.run(stage or host_stage(maps), maps, n_classes, total=len(maps) + (0 if tail else K["dma_batch"]), launches=device_maps, finalize=False,
                 what=what)
    link = r.c.vote_link_bytes()
    r.c.vote_finalize()
    return pool, r.launches("seg_expand") - before, link


def compact(r, K, maps, **kw):
    """handed() for a run whose host maps all take the compact form: records crossed the link, and exactly their bytes"""
    pool, launches, link = handed(r, K, maps, **kw)
    assert launches >= 1 and link == record_sum(maps), (kw.get("what"), launches, link, record_sum(maps))
    return pool, launches


# ---- a. ranks in a cell row -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(M.RANK_CASES)), ids=lambda i: f"case{i + 1}")
def test_ranks_in_a_cell_row(gsx, K, case):
    """1040 x 8: 260 cells per cell row, so a second round of the cell-row loop with four cells in it, in one band.  The mixed cells sit
    at the last lane of a wave and the first of the next (63 | 64), at the last thread of a round and the first of the next (255 | 256),
    fill a round and go one beyond, or start in the second round only; every block has a (label, place) of its own, so a block taken
    from another rank shows.  The pool is the model's and the same whatever the number of packer threads."""
    w, h = M.RANK_SHAPE
    assert K["block"] < cells_per_row(w) == w // M.CELL < 2 * K["block"] and h == M.BAND_ROWS and K["block"] == 4 * 64
    lab = M.mixed_cells_map(w, h, M.rank_case_cells(M.RANK_CASES[case]), 7)
    maps = [(lab.astype(np.int32), False)]
    assert record_sum(maps) == compact_layout(w, h)[2] + 16 * M.RANK_BLOCKS[case]
    pools = []
    for t in THREADS:
        with Rig(gsx, host_threads=t) as r:
            pools.append(compact(r, K, maps, what=f"case {case + 1}, {t} threads")[0])
    assert np.array_equal(pools[0], pools[1]) and np.array_equal(pools[0], pools[2])


def test_second_band_sticks_out(gsx, K):
    """1040 x 9: a second band whose first cell row holds one pixel row and whose second lies past the map, lightly and heavily mixed"""
    w, h = M.RANK_SHAPE[0], M.RANK_SHAPE[1] + 1
    maps = noise_maps(w, h)[1:]
    pools = []
    for t in THREADS:
        with Rig(gsx, host_threads=t) as r:
            pools.append(compact(r, K, maps, what=f"{t} threads")[0])
    assert np.array_equal(pools[0], pools[1]) and np.array_equal(pools[0], pools[2])


# ---- b. widths and heights at the kernel's own units ------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", M.UNIT_SHAPES, ids=lambda v: str(v))
def test_widths_round_the_workgroup_and_the_coarse_copy(gsx, K, w, h):
    """255, 256 and 257 cells in a cell row (walked as 256, 256 and 260: whole strips), in one band and with a band that sticks out;
    2044 x 5, 2048 x 8 and 2052 x 5: the coarse level of one band is 256, 256 and 264 pieces of 16 bytes dealt over 256 threads, so
    the last one strides; 4100 x 4 strides three times"""
    g = M.geometry(w, h, N_CLASSES)
    pieces, bands = (g["map_bytes"] - g["coarse_off"]) // 16, (h + M.BAND_ROWS - 1) // M.BAND_ROWS
    cells = {1020: 255, 1024: 256, 1028: 257}
    assert K["block"] == 256 and cells.get(w, (w + 3) // 4) == (w + 3) // 4 and (cells_per_row(w) > K["block"]) == (w > 1024)
    assert {2044: 256, 2048: 256, 2052: 264, 4100: 520}.get(w, pieces) == pieces and (pieces > bands * K["block"]) == (w > 2048)
    maps = noise_maps(w, h)
    with Rig(gsx) as r:
        compact(r, K, maps, what=f"{w}x{h}")


@pytest.mark.parametrize("w,h", M.LONG_SHAPES, ids=lambda v: str(v))
def test_largest_sides(gsx, K, w, h):
    """65535 x 1: 4096 strips and 64 rounds of the cell-row loop in one band; 1 x 65535: 8192 bands of one strip - the largest strip and
    band offsets the library accepts"""
    maps = noise_maps(w, h)[1:]
    with Rig(gsx) as r:
        compact(r, K, maps, what=f"{w}x{h}")


def test_cell_strip_and_band_edges(gsx, K):
    """every width x height round the cell, the strip, the band, the coarse strip and the coarse band, as the device pack has them
    (tests/test_segpack_gpu.py): three maps per shape in one run, the ring re-laid from shape to shape"""
    maps = [m for w in M.EDGE_WIDTHS for h in M.EDGE_HEIGHTS for m in noise_maps(w, h)]
    with Rig(gsx) as r:
        compact(r, K, maps, what="edges")


# ---- c. dtypes through the compact form -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_dtypes_through_the_compact_form(gsx, K, dtype):
    maps = [m for (w, h) in M.DTYPE_SHAPES for m in noise_maps(w, h, dtype)]
    with Rig(gsx) as r:
        compact(r, K, maps, what=dtype)


# ---- d. groups --------------------------------------------------------------------------------------------------------------------
def all_mixed(w, h, base):
    return M.mixed_cells_map(w, h, [(cy, cx) for cy in range(h // M.CELL) for cx in range(w // M.CELL)], base)


def test_groups_of_records(gsx, K):
    """64 x 32, more than eight full groups of either kind.  Records lie back to back at 256-byte steps in a group of dma_batch slots
    (a slot = a worst-case record); a group closes at compact_batch records or when a worst-case record no longer fits: uniform maps
    (512 bytes) close it by count, all-mixed ones (a slot each) by room, and a ring of fewer groups than that is lapped.  One expansion
    launch per group.  Announced exactly, the last maps go up one by one: the same bytes."""
    w, h = 64, 32
    cap, _, so = compact_layout(w, h)
    assert (cap, so) == (2560, 512) and cap % 256 == 0                                  # slot = capacity, a uniform record = so
    assert K["compact_batch"] * so <= K["dma_batch"] * cap - cap + so                   # compact_batch uniform records fit: the count closes the group
    n = 8 * K["compact_batch"] + 3
    ceil = lambda a, b: (a + b - 1) // b
    uniform = [(np.full((h, w), v % N_CLASSES - 1, np.int32), False) for v in range(n)]
    mixed = [(all_mixed(w, h, v % N_CLASSES).astype(np.int32), False) for v in range(n)]
    noisy = noise_maps(w, h, count=n)
    assert record_sum(uniform) == n * so and record_sum(mixed) == n * cap
    with Rig(gsx) as r:
        assert compact(r, K, uniform, what="uniform")[1] == ceil(n, K["compact_batch"])
        assert compact(r, K, mixed, what="all mixed")[1] == ceil(n, K["dma_batch"])
        pool, launches = compact(r, K, noisy, what="noise")
        assert ceil(n, K["compact_batch"]) <= launches <= ceil(n, K["dma_batch"]), launches
        exact, launches_exact = compact(r, K, noisy, tail=True, what="noise, announced exactly")
        assert launches_exact >= launches + K["dma_batch"] - 2 and np.array_equal(exact, pool)


# ---- e. a flush inside a group ----------------------------------------------------------------------------------------------------
def test_flush_inside_a_group(gsx, K):
    """vote_export after the 2nd and after the 7th of 20 maps sends the pending records up; the group goes on filling behind them.  With
    uniform 64 x 32 maps (compact_batch to a group) that is two launches more than the groups alone; with 61 x 35 maps of every content
    the whole pool is the model's.  A device map in those places is packed by its own kernel between the records' maps."""
    assert 7 < K["compact_batch"] < 20 <= 2 * K["compact_batch"]
    flush = lambda c, v: c.vote_export() if v in (1, 6) else None
    with Rig(gsx) as r:
        uniform = [(np.full((32, 64), v, np.int32), False) for v in range(20)]
        assert compact(r, K, uniform, what="uniform, no flush")[1] == 2
        assert compact(r, K, uniform, stage=host_stage(uniform, flush), what="uniform, two flushes")[1] == 4
        maps = noise_maps(61, 35, count=20)
        plain, _ = compact(r, K, maps, what="no flush")
        flushed, _ = compact(r, K, maps, stage=host_stage(maps, flush), what="two flushes")
        assert np.array_equal(plain, flushed)

        between = noise_maps(61, 35, seed=5, count=2)
        order = maps[:2] + between[:1] + maps[2:7] + between[1:] + maps[7:]

        def stage(c):
            for v, (arr, packed) in enumerate(order):
                c.vote_view(CAM, dev(arr) if v in (2, 8) else arr, packed_u8=packed)

        pool, launches, link = handed(r, K, order, stage=stage, device_maps=2, what="device maps between")
        assert launches >= 1 and link == record_sum(maps)
        stride = M.geometry(61, 35, N_CLASSES)["stride"]
        host_part = np.concatenate([pool[:2 * stride], pool[3 * stride:8 * stride], pool[9 * stride:]])
        assert np.array_equal(host_part, plain)


# ---- f. two geometries ------------------------------------------------------------------------------------------------------------
def test_two_geometries_of_one_slot_size(gsx, K):
    """64 x 32 and 32 x 64 alternate: the same slot, so the ring stays as it lies, and every change of geometry sends the pending
    record up on its own (one expansion launch = one geometry)"""
    assert compact_layout(64, 32)[0] == compact_layout(32, 64)[0]
    a, b = noise_maps(64, 32, count=12), noise_maps(32, 64, count=12)
    maps = [m for pair in zip(a, b) for m in pair]
    with Rig(gsx) as r:
        assert compact(r, K, maps, what="64x32 / 32x64")[1] == len(maps)


def test_two_geometries_of_different_slot_sizes(gsx, K):
    """17 x 9, 322 x 181 and 17 x 9 again in one run: the ring is re-laid at each change, with records pending"""
    assert compact_layout(17, 9)[0] != compact_layout(322, 181)[0]
    maps = noise_maps(17, 9, count=5) + noise_maps(322, 181, count=5) + noise_maps(17, 9, seed=1, count=5)
    with Rig(gsx) as r:
        assert compact(r, K, maps, what="17x9, 322x181, 17x9")[1] >= 3


# ---- g. the pool-form ring --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_classes,options", [(N_CLASSES, {"host_compact": 0}), (255, {})], ids=["host_compact=0", "255 classes"])
def test_pool_form_ring(gsx, K, n_classes, options):
    """30 maps through the ring of pool-form slots (the compact form switched off, or 255 classes, where no coarse level exists and so
    no compact form): groups of dma_batch slots, lapped more than once; no expansion, and the link carries every stride whole"""
    n, (w, h) = 30, (61, 35)
    g = M.geometry(w, h, n_classes)
    assert (g["coarse_off"] is None) == (n_classes == 255) and n > 7 * K["dma_batch"]
    maps = noise_maps(w, h, n_classes=n_classes, count=n)
    flush = lambda c, v: c.vote_export() if v == 1 else None
    with Rig(gsx, **options) as r:
        pools = [handed(r, K, maps, n_classes=n_classes, what="no tail"),
                 handed(r, K, maps, n_classes=n_classes, tail=True, what="announced exactly"),
                 handed(r, K, maps, n_classes=n_classes, stage=host_stage(maps, flush), what="flush after the 2nd map")]
    for pool, launches, link in pools:
        assert launches == 0 and link == n * g["stride"] and np.array_equal(pool, pools[0][0])


# ---- h. two runs on one context ---------------------------------------------------------------------------------------------------
def test_second_run_holds_nothing_of_the_first(gsx, K):
    """six all-mixed 1028 x 9 maps (every record fills its slot), then six uniform 17 x 9 maps on the same context, ring and staging:
    the second run's pool is the model's over every stride, and the pool the same run leaves on a fresh context"""
    rng = np.random.default_rng(1028)
    first = [(rng.integers(-1, N_CLASSES, size=(9, 1028)).astype(np.int32), False) for _ in range(6)]
    assert record_sum(first) == 6 * compact_layout(1028, 9)[0]
    second = [(np.full((9, 17), 11 * v, np.int32), False) for v in range(6)]
    with Rig(gsx) as r:
        compact(r, K, first, what="first run")
        after = compact(r, K, second, what="second run")[0]
    with Rig(gsx) as r:
        fresh = compact(r, K, second, what="fresh context")[0]
    assert np.array_equal(after, fresh)
