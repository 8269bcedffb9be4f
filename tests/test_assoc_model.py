"""CPU: the association rule (tests/assoc_model.py) on constructed tables, and the value scene: blobs whose segment ids are
permuted from view to view come out as the blob partition after association + the oracle's vote, and do not without it."""
import numpy as np
import pytest

import assoc_cases as ac
import assoc_model as am
import oracle

ONE = 1 << am.ONE_SHIFT


def table(S, M, rows):
    """rows: {b: {column: count}} -> (S + 1, M + 1) table"""
    t = np.zeros((S + 1, M + 1), np.int64)
    for b, cols in rows.items():
        for k, v in cols.items():
            t[b, k] = v
    return t


def q_of(min_overlap):
    return am.Run(1, 1, 1, min_overlap).q


def test_threshold_met_exactly_and_missed_by_one():
    q = q_of(0.25)                                   # q = 2^18: count * 2^20 == q * size  <=>  4 * count == size
    assert q == ONE // 4
    hit = table(2, 4, {1: {0: 6, 1: 2}})             # size 8, count 2: equality
    remap, G, d = am.decide(hit, 1, 4, q, 1)
    assert remap.tolist() == [0, -1] and (G, d) == (1, 0)
    miss = table(2, 4, {1: {0: 7, 1: 2}})            # size 9, count 2: 2 * 2^20 < 2^18 * 9
    remap, G, d = am.decide(miss, 1, 4, q, 1)
    assert remap.tolist() == [1, -1] and (G, d) == (2, 0)
    # the same one step on the count's side, with a q that is no power of two
    q3 = q_of(0.3)
    assert q3 == int(np.ceil(0.3 * ONE)) and q3 * 10 > 3 * ONE    # ceil: 3 of 10 is NOT enough, 0.3 is not a binary fraction
    assert am.decide(table(1, 2, {1: {0: 7, 1: 3}}), 1, 2, q3, 1)[0].tolist() == [1]
    assert am.decide(table(1, 2, {1: {0: 6, 1: 4}}), 1, 2, q3, 1)[0].tolist() == [0]


def test_equal_counts_take_the_lowest_instance():
    t = table(1, 4, {1: {2: 5, 3: 5, 4: 1}})
    assert am.decide(t, 4, 4, q_of(0.3), 1)[0].tolist() == [1]


def test_two_segments_want_the_same_instance():
    q = q_of(0.3)
    big_second = table(2, 4, {1: {1: 4}, 2: {1: 6}})              # row 2 is larger: it takes instance 0, row 1 opens instance 1
    remap, G, d = am.decide(big_second, 1, 4, q, 1)
    assert remap.tolist() == [1, 0] and (G, d) == (2, 0)
    equal = table(2, 4, {1: {1: 5}, 2: {1: 5}})                   # equal sizes: the lower b goes first
    remap, G, d = am.decide(equal, 1, 4, q, 1)
    assert remap.tolist() == [0, 1] and (G, d) == (2, 0)
    # the loser falls back on its second choice when that still meets the threshold
    second = table(2, 4, {1: {1: 5, 2: 4}, 2: {1: 9, 2: 1}})
    assert am.decide(second, 2, 4, q, 1)[0].tolist() == [1, 0]


def test_min_size_edge():
    t = table(2, 4, {1: {0: 5}, 2: {0: 4}})
    remap, G, d = am.decide(t, 0, 4, q_of(0.3), 5)                # size == min_size is kept, min_size - 1 is not - and not counted
    assert remap.tolist() == [0, -1] and (G, d) == (1, 0)


def test_full_bank_drops_and_counts():
    t = table(3, 2, {1: {0: 9}, 2: {0: 8}, 3: {0: 7}})
    remap, G, d = am.decide(t, 0, 2, q_of(0.3), 1)
    assert remap.tolist() == [0, 1, -1] and (G, d) == (2, 1)
    # a full bank still matches
    t = table(2, 2, {1: {0: 3, 2: 6}, 2: {0: 4}})
    remap, G, d = am.decide(t, 2, 2, q_of(0.3), 1)
    assert remap.tolist() == [1, -1] and (G, d) == (2, 1)


def test_first_view_numbers_by_descending_size():
    t = table(4, 8, {1: {0: 3}, 2: {0: 9}, 3: {0: 0}, 4: {0: 9}})
    remap, G, d = am.decide(t, 0, 8, q_of(0.3), 1)
    assert remap.tolist() == [2, 0, -1, 1] and (G, d) == (3, 0)    # sizes 9 (b = 2), 9 (b = 4), 3 (b = 1); the empty row gets -1


def test_min_overlap_zero_and_one():
    assert q_of(0.0) == 0 and q_of(1.0) == ONE
    t = table(2, 4, {1: {0: 99, 1: 1}, 2: {0: 5}})
    assert am.decide(t, 1, 4, 0, 1)[0].tolist() == [0, 1]          # any overlap is enough; none at all still opens an instance
    assert am.decide(t, 1, 4, ONE, 1)[0].tolist() == [1, 2]        # every Gaussian has to carry it
    full = table(1, 4, {1: {1: 7}})
    assert am.decide(full, 1, 4, ONE, 1)[0].tolist() == [0]


def test_run_remembers_the_first_assignment_and_fails_clean():
    run = am.Run(4, 3, 4, 0.5, 1)
    x, y = np.array([0, 1, 2, -1], np.int32), np.array([0, 0, 0, -1], np.int32)
    remap, out = run.view(x, y, np.array([[0, 0, 1]], np.int32))
    assert remap.tolist() == [0, 1, -1] and out.tolist() == [[0, 0, 1]] and run.gid.tolist() == [0, 0, 1, -1]
    assert run.table[1, 0] == 2 and run.table[2, 0] == 1 and run.table.sum() == 3
    state = (run.gid.copy(), run.G, run.dropped, run.views)
    with pytest.raises(am.RangeError):
        run.view(x, y, np.array([[0, 3, 1]], np.int32))
    with pytest.raises(am.RangeError):
        run.view(x, y, np.array([[0, -2, 1]], np.int32))
    assert np.array_equal(run.gid, state[0]) and (run.G, run.dropped, run.views) == state[1:]
    # one segment over Gaussians of instances 0, 0 and 1: it takes 0, and the Gaussian that carried 1 keeps it
    remap, out = run.view(x, y, np.array([[2, 2, 2]], np.int32))
    assert remap.tolist() == [-1, -1, 0] and run.gid.tolist() == [0, 0, 1, -1] and run.views == 2


@pytest.fixture(scope="module")
def value():
    pos, blob, cams, maps, sizes = ac.value_scene()
    run = am.Run(len(pos), 254, 255, 0.3, 1)
    seen = np.zeros(len(pos), bool)
    relabelled, per_view = [], []
    for cam, seg, size in zip(cams, maps, sizes):
        x, y = oracle.project_many(pos, cam)
        seen |= x >= 0
        per_view.append(np.unique(blob[x >= 0]))
        relabelled.append(run.view(x, y, seg, size)[1])
    labels = oracle.assign_labels(pos, cams, relabelled, sizes)
    raw = oracle.assign_labels(pos, cams, maps, sizes)
    return dict(blob=blob, seen=seen, per_view=per_view, labels=labels, raw=raw, run=run)


def test_value_scene_recovers_the_blobs(value):
    assert [len(v) for v in value["per_view"]] == [6, 6, 4, 6, 6]          # one view sees only four of the blobs
    seen = value["seen"]
    assert seen.all()
    assert value["run"].G == ac.K and value["run"].dropped == 0
    assert (value["labels"][seen] >= 0).all()
    assert am.same_partition(value["labels"][seen], value["blob"][seen])
    assert am.same_partition(value["run"].gid[seen], value["blob"][seen])


def test_value_scene_needs_the_association(value):
    seen = value["seen"]
    assert not am.same_partition(value["raw"][seen], value["blob"][seen])
