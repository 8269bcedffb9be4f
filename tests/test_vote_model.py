"""CPU: the constructed-vote cases of tests/vote_cases.py are what they claim to be.  For every case and both phases the oracle
on the realised scene gives exactly the labels of the matrix model, its per-view votes are the matrix's columns, and every
family's guard finds the edge the family is there for.  The model itself is checked against the reference's ties fixture."""
import numpy as np
import pytest

import oracle
import vote_cases as vc
from conftest import golden_assign_cases


@pytest.mark.parametrize("case", vc.all_cases(), ids=repr)
def test_oracle_equals_model(case):
    case.check_guard()
    want = case.model()["labels"]
    B = case["B"]
    V = B.shape[1]
    for phase in vc.PHASES:
        pos, cams, segs, sizes = case.scene(phase)
        assert pos.dtype == np.float32 and len(cams) == V
        got = oracle.assign_labels(pos, cams, segs, sizes, threads=0)
        assert np.array_equal(got, want), (case["name"], phase, int((got != want).sum()))
        for v in sorted({0, V // 2, V - 1}):
            assert np.array_equal(oracle.view_bins(pos, cams[v], segs[v], sizes[v]), B[:, v]), (case["name"], phase, v)


def test_every_listed_edge_has_a_case():
    names = {c["name"] for c in vc.all_cases()}
    assert len(names) == len(vc.all_cases())
    assert {f"f1-V{V}" for V in (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 254, 255)} <= names
    assert {f"f1-V{V}-cull" for V in (63, 64, 65, 129)} <= names
    assert {f"f2-n{n}" for n in (1, 63, 64, 65, 255, 256, 257, 1025)} <= names
    assert {f"f3-g{g}" for g in (6, 7, 8, 15, 16, 17, 32)} <= names
    assert {f"f4-C{C}" for C in (1, 2, 3, 4, 150, 151, 152, 153, 155, 156, 207, 208, 254, 255)} <= names
    assert {f"f5-E{E}" for E in (1, 8, 12, 23)} <= names
    assert {f"f8-V{V}" for V in (256, 257, 510, 511)} <= names
    assert {f"f9-{w}x{h}-{k}" for (w, h) in ((15, 7), (16, 8), (17, 9), (33, 5), (64, 32), (65, 33)) for k in ("same", "half", "x1.5")} <= names
    assert vc.cases_of(6)[0]["E"] == (1, 15, 16, 17, 31, 32, 33, 39) and vc.cases_of(7)[0]["E"] == (1, 128, 254)
    # the last stage's row counts: nq = (bins + 3) / 4 at 38 | 39 (three full rounds of 13) | 40, 52 | 53, 64
    assert {(c["bins"] + 3) // 4 for c in vc.cases_of(4)} >= {1, 2, 38, 39, 40, 52, 53, 64}
    assert {c["bins"] % 4 for c in vc.cases_of(4)} == {0, 1, 2, 3}
    # every pattern of the last stage's orderings is feasible, and guarded, at some split point
    assert set().union(*(vc.f5_feasible(24, E) for E in (1, 8, 12, 23))) == set(vc.F5_PATTERNS)
    assert vc.f5_feasible(24, 8) == vc.f5_feasible(24, 12) == set(vc.F5_PATTERNS)


def test_model_handles_hand_made_matrices():
    m = vc.vote_model(np.array([[2, 1, 1, 2], [-1, -1, -1, -1], [0, 3, -1, 3], [0, 3, 0, 3], [1, -1, 2, -1]]), 4)
    assert m["labels"].tolist() == [1, -1, 2, -1, 0]
    assert m["cnt"][:, 0].tolist() == [0, 2, 2, 0] and m["fv"][:, 0].tolist() == [0, 254, 255, 0]
    assert vc.vote_model(np.zeros((1, 300), np.int64), 2)["fv"][0, 0] == 65535


def test_permille_reaches_every_split_point():
    for V in (24, 40, 63, 64, 65, 127, 128, 129, 254, 255, 12, 3):
        for E in range(1, V):
            p = vc.early_permille(V, E)
            assert max(1, (V * p + 999) // 1000) == E
    assert vc.balanced_bounds(510) == [0, 255, 510] and vc.balanced_bounds(511) == [0, 170, 340, 511] and vc.early_bounds(511) == [0, 240, 480, 511]
    assert vc.balanced_bounds(256) == [0, 128, 256] and vc.early_bounds(256) == [0, 240, 256]


def test_model_on_the_ties_fixture():
    """The reference's own labels on its ties fixture, from the matrix of its per-view votes."""
    name, pos, cams, segs, sizes, labels = next(c for c in golden_assign_cases() if c[0].startswith("ties"))
    B = np.stack([oracle.view_bins(pos, cam, seg, sz) for cam, seg, sz in zip(cams, segs, sizes)], axis=1)
    m = vc.vote_model(B, int(B.max()) + 1)
    assert np.array_equal(m["labels"], labels)
    assert (((m["cnt"] == m["top"][None]) & (m["cnt"] > 0)).sum(0) >= 2).mean() > 0.05     # the fixture does hold ties
