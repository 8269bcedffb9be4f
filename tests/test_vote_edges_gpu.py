"""GPU: the vote kernels of csrc/vote.hip against the matrix model of tests/vote_cases.py, at the sizes where their own constants
bite (views per chunk, per culling word, per batch; bytes of the record in flight; rows of four bins; lanes per Gaussian group;
threads per workgroup; workgroups per XCD round; strips, lines and cells of the packed maps).  The votes are authored, the expected
labels and planes come from integer numpy, and tests/test_vote_model.py has shown on the CPU that the oracle reads the same out of
the same scenes.  Integer work: every comparison is np.array_equal.

Routes:  R1 one piece (early_vote 0, vote_finalize) - R2 planes (vote_rewind, vote_flush, debug_planes == the model's counts and
first-view codes, then the keys) - R3 early planes + fold (vote_fused_final) - R4 early record + replay (vote_fused_replay), both
with the split point E chosen through early_vote_at and read back - R5 more than 255 views: batched counts on and off, and the early
count batches.  The early vote needs the branchless projection (vote.hip: early_common), so option sets with flat_project = 0 run
R1 and R2 only; that the others really split where asked is asserted on every run."""
import numpy as np
import pytest

import vote_cases as vc

pytestmark = pytest.mark.gpu

OPTION_SETS = [{}, {"vote_unroll": 2}, {"vote_unroll": 4}, {"filter_project": 0}, {"seg_coarse": 0}, {"seg_tiled": 0},
               {"flat_project": 0}, {"wave_cull": 0}, {"spatial_sort": 0},
               {"labels_u8": 0}]
MAP_OPTION_SETS = [{"seg_tiled": t, "seg_coarse": c, "host_pack": h} for t in (0, 1) for c in (0, 1) for h in (0, 1)]


def _id(opts):
    return "-".join(f"{k}{v}" for k, v in opts.items()) or "defaults"


@pytest.fixture(scope="module")
def contexts(gsx):
    """One context per option set, made when first asked for."""
    made = {}

    def get(opts):
        key = tuple(sorted(opts.items()))
        if key not in made:
            c = gsx.Context(0)
            for k, v in opts.items():
                c.set_option(k, v)
            made[key] = c
        return made[key]
    yield get
    for c in made.values():
        c.close()


def _launches(c, name):
    return c.profile_get(name)[0] if name in c.profile_names() else 0


def _stage(c, case, phase):
    pos, cams, segs, sizes = case.scene(phase)
    c.upload_positions(pos)
    c.vote_begin(case["n_classes"], 0, len(cams))
    for cam, seg, sz in zip(cams, segs, sizes):
        c.vote_view(cam, seg, sz)


def _same(got, want, what):
    assert np.array_equal(got, want), (*what, int((got != want).sum()), np.flatnonzero(got != want)[:8].tolist())


def r1_one_piece(c, case, phase):
    c.set_option("early_vote", 0)
    _stage(c, case, phase)
    got = c.vote_finalize()
    _same(got, case.model()["labels"], (case["name"], phase, "R1"))
    return got


def r2_planes(c, case, phase):
    """On the views R1 staged."""
    m = case.model()
    c.vote_rewind()
    c.vote_flush()
    cnt, fv = c.debug_planes(case["bins"])
    _same(cnt, m["cnt"], (case["name"], phase, "R2 counts"))
    _same(fv, m["fv"], (case["name"], phase, "R2 first views"))
    c.vote_tiebreak_keys()
    _same(c.vote_labels_from_keys(), m["labels"], (case["name"], phase, "R2 labels"))


def r34_early(c, case, phase, E, replay):
    V = case["B"].shape[1]
    c.set_option("early_vote", 2)
    c.set_option("early_replay", replay)
    c.set_option("early_vote_at", vc.early_permille(V, E))
    c.profile(True)
    try:
        _stage(c, case, phase)
        assert c.vote_early_views() == E, (case["name"], E, c.vote_early_views())
        _same(c.vote_finalize(), case.model()["labels"], (case["name"], phase, "R4" if replay else "R3", E))
        last, first = ("vote_fused_replay", "vote_early_record") if replay else ("vote_fused_final", "vote_early_planes")
        assert _launches(c, last) == 1 and _launches(c, first) == 1 and _launches(c, "vote_fused_labels") == 0
    finally:
        c.profile(False)
        c.set_option("early_vote", 0)
        c.set_option("early_vote_at", 0)


def _early_ok(opts):
    return opts.get("flat_project", 1) != 0


def run_case(c, opts, case, routes, splits=None):
    """-> the number of early runs made."""
    early = 0
    for phase in vc.PHASES:
        if "R1" in routes:
            r1_one_piece(c, case, phase)
            if "R2" in routes:
                r2_planes(c, case, phase)
        if _early_ok(opts) and case["n_classes"] <= 254:
            for E in (case["E"] if splits is None else splits):
                for replay in (0, 1):
                    if ("R4" if replay else "R3") in routes:
                        r34_early(c, case, phase, E, replay)
                        early += 1
    return early


@pytest.mark.parametrize("opts", OPTION_SETS, ids=_id)
def test_view_counts(contexts, opts):
    """Family 1: V at the edges of the chunk of 8, the culling word of 64 and the batch of 255; from 63 views on also split at
    E = V - 1 and E = 64; two cases abstain through the sheet a view looks at."""
    c = contexts(opts)
    early = sum(run_case(c, opts, case, ("R1", "R2", "R3", "R4")) for case in vc.cases_of(1))
    assert early == (2 * 2 * 15 if _early_ok(opts) else 0)


@pytest.mark.parametrize("opts", OPTION_SETS, ids=_id)
def test_ragged_waves_and_blocks(contexts, opts):
    """Family 2: n at the edges of the wave of 64 and the workgroup of 256, every Gaussian with an answer of its own."""
    c = contexts(opts)
    for case in vc.cases_of(2):
        run_case(c, opts, case, ("R1", "R2"))


@pytest.mark.parametrize("opts", OPTION_SETS, ids=_id)
def test_workgroup_order(contexts, opts):
    """Family 3: grids of 7, 8, 9, 15, 16, 17, 18 and 33 workgroups under every xcd_swizzle."""
    c = contexts(opts)
    try:
        for swizzle in (0, 1, 2, 3):
            c.set_option("xcd_swizzle", swizzle)
            for case in vc.cases_of(3):
                run_case(c, opts, case, ("R1", "R4"))
    finally:
        c.set_option("xcd_swizzle", 1)


@pytest.mark.parametrize("opts", OPTION_SETS, ids=_id)
def test_bin_counts(contexts, opts):
    """Family 4: bins mod 4, the register rows (bins <= 152) and the rounds of 13 rows of the last stage, 255 classes."""
    c = contexts(opts)
    early = sum(run_case(c, opts, case, ("R1", "R2", "R3", "R4")) for case in vc.cases_of(4))
    assert early == (2 * 2 * 13 if _early_ok(opts) else 0)


@pytest.mark.parametrize("opts", OPTION_SETS, ids=_id)
def test_last_stage_orderings(contexts, opts):
    """Family 5: early-only, late-only and both-stage bins at equal and unequal totals, 64 patterns per wave."""
    c = contexts(opts)
    early = sum(run_case(c, opts, case, ("R1", "R2", "R3", "R4")) for case in vc.cases_of(5))
    assert early == (2 * 2 * 4 if _early_ok(opts) else 0)


@pytest.mark.parametrize("opts", OPTION_SETS, ids=_id)
def test_record_split_points(contexts, opts):
    """Family 6: E round the 16 record bytes in flight."""
    c = contexts(opts)
    early = sum(run_case(c, opts, case, ("R1", "R2", "R3", "R4")) for case in vc.cases_of(6))
    assert early == (2 * 2 * 8 if _early_ok(opts) else 0)


@pytest.mark.parametrize("opts", OPTION_SETS, ids=_id)
def test_saturated_counters(contexts, opts):
    """Family 7: counts of 255, 254 and 128 : 127 in 255 views."""
    c = contexts(opts)
    early = sum(run_case(c, opts, case, ("R1", "R2", "R3", "R4")) for case in vc.cases_of(7))
    assert early == (2 * 2 * 3 if _early_ok(opts) else 0)


@pytest.mark.parametrize("opts", OPTION_SETS, ids=_id)
def test_more_than_255_views(contexts, opts):
    """Family 8: R1 (the batched kernels), R2 (16-bit planes) and R5."""
    c = contexts(opts)
    try:
        for case in vc.cases_of(8):
            V = case["B"].shape[1]
            want = case.model()["labels"]
            for phase in vc.PHASES:
                r1_one_piece(c, case, phase)
                c.set_option("batched_counts", 0)
                c.vote_rewind()
                _same(c.vote_finalize(), want, (case["name"], phase, "batched_counts 0"))
                c.set_option("batched_counts", 1)
                r2_planes(c, case, phase)
                # the early count batches: every batch of the early cut but the last starts as soon as its views are staged
                c.set_option("early_vote", 2)
                c.profile(True)
                _stage(c, case, phase)
                ends = vc.early_bounds(V)[1:-1]
                started = len(ends) if _early_ok(opts) else 0
                assert c.vote_early_views() == (ends[-1] if started else 0)
                _same(c.vote_finalize(), want, (case["name"], phase, "R5 early counts"))
                assert _launches(c, "vote_early_counts") == started
                assert _launches(c, "vote_fused_counts") == (1 if started else -(-V // vc.MAX_BATCH))
                c.profile(False)
                c.set_option("early_vote", 0)
    finally:
        c.set_option("batched_counts", 1)
        c.set_option("early_vote", 0)
        c.profile(False)


@pytest.mark.parametrize("opts", MAP_OPTION_SETS, ids=_id)
def test_map_geometry(contexts, opts):
    """Family 9: map sides round the strip of 16 columns, the line of 8 rows and the cell of 4 x 4; uniform, mixed, top-label,
    unlabelled and ragged cells; maps of half and 1.5 times the image with the clamp at the last column and row; 255 classes,
    whose top label packs to the byte that marks a mixed cell."""
    c = contexts(opts)
    for case in vc.cases_of(9):
        run_case(c, opts, case, ("R1", "R2"))


def test_wave_culling_of_constructed_windows(contexts):
    """Family 1 at V = 63, 64, 65, 129 with alternate views that see the first row only: whole waves are culled, bits of more than
    one mask word are set, and no vote changes."""
    for case in vc.cases_of(1, cull=True):
        got = {}
        for cull in (1, 0):
            c = contexts({"wave_cull": cull})
            c.vote_culled(reset=True)
            got[cull] = r1_one_piece(c, case, 0.5)
            skipped = c.vote_culled(reset=True)
            assert (skipped > 0) if cull else skipped == 0, (case["name"], cull, skipped)
            r2_planes(c, case, 0.5)
            r1_one_piece(c, case, 0.0)
        assert np.array_equal(got[1], got[0])
