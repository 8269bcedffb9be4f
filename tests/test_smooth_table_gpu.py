"""GPU: the search form of the label filter (csrc/smooth.hip: smooth_search_kernel) at the edges of its class table and of its
16-bit counters, on the clump scenes of tests/smooth_cases.py, whose neighbour sets are the clumps and whose votes are
therefore constructed: ties and near-ties between classes on one dword, on neighbouring dwords, on lane 63 against lane 0 of
the next trip of the winner scan (the larger class in the lower lane), on one lane's two trips and at the ends of a
4096-class table; C = 1 .. 4096 around the scan's second trip; counts of 255, 256, 257 in either half of a dword with the
other half at m - 1 and at 0; 32767, 32768, 32769 in a hi half (k = n); the ignored label at rank 0, at the last rank of an odd
C, in the hi half beside the winner, and absent from the data; min_votes at m, m + 1, 65536 and 2^31 - 1; int32 extremes as
labels; four rounds with the live labels at classes 127, 128, 129 and C - 1; a 3-class call behind a 4096-class call on one
context; n = 1 modulo the queries of a workgroup.  tests/test_smooth_cases_model.py holds every scene and its closed-form
result to the models on the CPU.

Everything is integers: labels, support, the changed list and smooth_rounds_done are compared with np.array_equal, no
tolerance.  For k <= 64 the default (lists), "smooth_search", "nn_brute" and both together must all give the expected result;
for k > 64 the default and "nn_brute".  Once a GPU call of this module has raised, nothing more is started.

Mutants of smooth.hip, each built once outside the tree and run once over this file and the two older smooth GPU files (tests of
this file that failed / older tests that failed; "ties" = test_clumps[tie-*], "classes" = test_clumps[classes-*], both k):
  1 the butterfly without `oi < bi`      ties 126-128, 127-128, 5-128-4095, ignore-hi-beside-winner, both rounds tests: 10 /
                                         51 (test_smooth_search_gpu: scenes 10, forms 28, rounds 13 - ties between lanes 0 .. 2)
  2 `hi > bc` -> `>=`                    ties 0-1 and 130-131, ignore-last-odd, the 3 ignore-absent, rounds[8]: 13 /
                                         54 (test_smooth_search_gpu: scenes 10, forms 30, rounds 14)
  3 the scan limited to its first trip   every tie with a class >= 128 (16), classes 129, 130, 4095, 4096 (8), count-255/256/257,
                                         both rounds tests, the small table behind the large one: 30 / 1 (test_class_limit)
  4 no "own among the winners" clause    every tie (20), classes 127 .. 4096 (12), every ignore case (12), values (2), both
                                         rounds tests, small behind large: 49 /
                                         79 (test_smooth_search_gpu: scenes 10, forms 43, rounds 25, test_class_limit)
  5 the scan reads counters `& 0xff`     count-255, count-256, count-257, top bit 32768 and 32769: 5 / none
  6 host `words = C / 2`                 tie 129-130 (C odd), classes 1, 3, 127, 129, 4095, ignore-last-odd, min-votes-2-k65,
                                         values-k65 (C odd), the 3 top-bit cases (C = 3), small behind large: 20 /
                                         18 (test_smooth_search_gpu: forms 8, rounds 10 - the scenes of 3 .. 7 points)
None of the six moves an address.  The older files notice 1, 2, 4 and 6 on the low lanes of their six classes; what they cannot
see is the second trip of the scan (3) and a counter above 255 (5), and they never place a tie across lane 63 / lane 0.

Times on the MI355X (pytest --durations=0): the whole file about 2 s; the slowest are test_rounds_at_high_class_ids[65] 0.19 s,
test_a_small_table_behind_a_large_one 0.12 s and test_rounds_at_high_class_ids[8] 0.11 s.  A k = n = 33000 case takes 0.09 s for
its two calls, so the three of them stay."""
import numpy as np
import pytest

import region_growing_model as model
import smooth_cases as sc
import smooth_model as sm
from test_smooth_search_gpu import blobs

pytestmark = pytest.mark.gpu

CASES = sc.all_cases()
_BROKEN = []


def forms(k):
    """(smooth_search, nn_brute) settings a k runs with"""
    return ((0, 0), (1, 0), (0, 1), (1, 1)) if k <= sc.constants()["list_max_k"] else ((0, 0), (0, 1))


def gpu(ctx, pts, L, k, search, brute, **kw):
    """one call: (labels, changed, support, rounds done).  The options are reset whatever happens; once a call has raised, no
    test of this module goes to the GPU again."""
    if _BROKEN:
        pytest.fail(f"an earlier GPU call of this module failed ({_BROKEN[0]}): nothing more is started")
    try:
        try:
            ctx.set_option("nn_brute", int(brute))
            ctx.set_option("smooth_search", int(search))
            got, changed, sup = ctx.smooth_labels(pts, L, k=k, return_support=True, **kw)
            return got, changed, sup, ctx.smooth_rounds_done
        finally:
            ctx.set_option("nn_brute", 0)
            ctx.set_option("smooth_search", 0)
    except BaseException as e:
        _BROKEN.append(f"n = {len(L)}, k = {k}, search {search}, brute {brute}, {kw}: {type(e).__name__}: {e}")
        raise


def check(got, want, what):
    """got, want: (labels, changed, support, rounds done) / (labels, support, changed, rounds done)"""
    labels, changed, sup, done = got
    w_labels, w_sup, w_changed, w_done = want
    bad = np.flatnonzero(labels != w_labels)
    assert np.array_equal(labels, w_labels), (what, len(bad), bad[:5].tolist(), labels[bad[:5]].tolist(), w_labels[bad[:5]].tolist())
    bad = np.flatnonzero(sup != w_sup)
    assert np.array_equal(sup, w_sup), (what, len(bad), bad[:5].tolist(), sup[bad[:5]].tolist(), w_sup[bad[:5]].tolist())
    assert changed == w_changed and done == w_done, (what, changed, w_changed, done, w_done)


def run_case(ctx, case):
    pts, L, _ = sc.scene(case)
    for kw in case.kws:
        want = sc.expected(case, kw)
        for search, brute in forms(case.k):
            check(gpu(ctx, pts, L, case.k, search, brute, **kw), want, (case.name, kw, search, brute))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_clumps(ctx, case):
    run_case(ctx, case)


@pytest.mark.parametrize("h", sc.TOP_COUNTS)
def test_top_bit_of_a_hi_half(ctx, h):
    """k = n: the hi half of dword 0 counts to 32767, 32768 and 32769; with min_votes above it every point keeps its label and
    reports the count of its own class, the lo half of the same dword and of the next one included"""
    case = sc.top_bit_case(h)
    pts, L, _ = sc.scene(case)
    for kw in case.kws:
        check(gpu(ctx, pts, L, case.k, 0, 0, **kw), sc.expected(case, kw), (case.name, kw))


@pytest.mark.parametrize("k", [8, 65])
def test_rounds_at_high_class_ids(ctx, k):
    """the blobs of test_smooth_search_gpu.py - real overlap, not clumps - with their four labels at
    classes 127, 128, 129 and C - 1 = 139"""
    pts, L = sc.high_id_blobs(*blobs())
    nbr = model.knn(pts, k)[0]
    for kw in sc.ROUND_KWS:
        want, w_changed, w_done, w_sup = sm.run(nbr, L, rounds=4, **kw)
        if not kw:
            assert w_changed[0] > 0                                       # the first round does change something
        for search, brute in forms(k):
            check(gpu(ctx, pts, L, k, search, brute, rounds=4, **kw), (want, w_sup, w_changed, w_done), (k, kw, search, brute))


def test_a_small_table_behind_a_large_one(ctx):
    """one context: 3 classes, 4096 classes, 3 classes again - a call clears and scans the dwords of its own classes only"""
    big, small = sc.reuse_cases()
    for case in (small, big, small, big):
        pts, L, _ = sc.scene(case)
        for search, brute in forms(case.k):
            check(gpu(ctx, pts, L, case.k, search, brute), sc.expected(case, {}), (case.name, search, brute))
