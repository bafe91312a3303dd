"""The seams of thr_posq (thrifty_amd/csrc/posq.hip, csrc/pos_lm.hpp): group sizes around the register rows and
the re-read loop with and without an excluded receiver, group counts around a workgroup's 32 teams, candidates
that cross a workgroup, a candidate that pairs missing leave underdetermined, a zero weight sum, a flagged group
with no eligible candidate, max_iter = 0, and a repeated call.  Everything is exact: `thr_pos` on the same or
on rebuilt groups, and the rule of the choice on the device's own rms values (tests/posq_golden.py)."""
import itertools

import numpy as np
import pytest

import posq_golden
from thrifty_amd import _native

pytestmark = pytest.mark.gpu

TINY_GATE = 1e-9        # metres: every group that may be flagged is


def cols_of(s):
    return s["group_ptr"], s["rx0"], s["rx1"], s["tdoa"], s["snr"], s["table"]


def check(s, gate_m=TINY_GATE, weights=None, max_iter=100, ratio=0.5, min_rx=5):
    """Ungated output against thr_pos, gated candidates against thr_pos on rebuilt groups, the choice against the
    rule -> (counts, gated output)."""
    cols = cols_of(s)
    want = _native.pos(*cols, max_iter=max_iter)
    _, plain = _native.posq(*cols, row_weight=weights, max_iter=max_iter)
    counts, out = _native.posq(*cols, row_weight=weights, gate_m=gate_m, ratio=ratio, min_rx=min_rx, max_iter=max_iter)
    for key in ("pos", "dop", "snr", "status", "iters"):
        assert plain[key].tobytes() == want[key].tobytes(), key
    assert out["full_pos"].tobytes() == want["pos"].tobytes() and out["snr"].tobytes() == want["snr"].tobytes()
    assert posq_golden.assert_candidates_equal_thr_pos(out, *cols, max_iter=max_iter) == counts["tasks"]
    posq_golden.assert_choice_follows_the_rule(out, cols[0], cols[1], cols[2], gate_m, ratio, min_rx)
    return counts, out


@pytest.mark.parametrize("rows", [1, 3, 8, 9, 32, 33, 40])
def test_group_sizes_around_the_register_rows(rows):
    # ten receivers; the first `rows` pairs in order: receiver 9 sits in rows 8, 16, 23, 29 and 34, so leaving it
    # out switches off register rows and re-read rows; its arrival is 150 m late in every group
    pairs = list(itertools.combinations(range(10), 2))[:rows]
    s = posq_golden.scene(seed=rows, n_rx=10, n_groups=3, every=1, late_rx=9, pairs=pairs)
    n_rx = len({i for pr in pairs for i in pr})
    counts, out = check(s, gate_m=3.0 if rows >= 32 else TINY_GATE)
    assert counts["flagged"] == (3 if n_rx >= 5 else 0) and counts["tasks"] == counts["flagged"] * n_rx
    if rows >= 32:
        np.testing.assert_array_equal(out["counts"][:, 2], 9)
        np.testing.assert_array_equal(out["flags"], _native.POSQ_INCONSISTENT | _native.POSQ_EXCLUDED)
        assert out["rms"][:, 1].max() < 1.0 < 3.0 < out["rms"][:, 0].min()
        assert np.all(out["counts"][:, 1] == rows - int(sum(9 in pr for pr in pairs)))


@pytest.mark.parametrize("n_groups", [0, 1, 32, 33])
def test_group_counts_around_a_workgroup(n_groups):
    s = posq_golden.scene(seed=40 + n_groups, n_rx=5, n_groups=n_groups, every=2)
    counts, out = check(s, gate_m=3.0)
    assert counts == {"groups": n_groups, "rows": 10 * n_groups, "flagged": n_groups // 2, "tasks": 5 * (n_groups // 2)}
    assert out["task_ptr"].shape == (n_groups + 1,) and out["pos"].shape == (n_groups, 2) and out["used"].shape == (10 * n_groups,)
    np.testing.assert_array_equal(out["counts"][:, 2], s["planted"])


def test_thirty_five_candidates_cross_a_workgroup():
    s = posq_golden.scene(seed=7, n_rx=5, n_groups=7, every=1)
    counts, out = check(s, gate_m=3.0)
    assert (counts["flagged"], counts["tasks"]) == (7, 35)
    np.testing.assert_array_equal(out["task_ptr"], 5 * np.arange(8))
    np.testing.assert_array_equal(out["counts"][:, 2], s["planted"])


def test_a_candidate_that_missing_pairs_leave_underdetermined():
    # without receiver 0 only the row (1, 2) is left: two receivers
    s = posq_golden.scene(seed=11, n_rx=5, n_groups=4, every=0, pairs=[(0, 1), (0, 2), (0, 3), (0, 4), (1, 2)])
    counts, out = check(s)
    assert (counts["flagged"], counts["tasks"]) == (4, 20)
    first = out["task_ptr"][:-1]
    np.testing.assert_array_equal(out["task_rx"][first], 0)
    np.testing.assert_array_equal(out["task_status"][first], _native.POS_UNDERDETERMINED)
    np.testing.assert_array_equal(out["task_nrx"][first], 2)
    assert np.all(out["counts"][:, 2] != 0)


def test_a_zero_weight_sum_is_nonfinite():
    s = posq_golden.scene(seed=12, n_rx=6, n_groups=5, every=0)
    weights = np.ones(len(s["tdoa"]))
    weights[s["group_ptr"][2]:s["group_ptr"][3]] = 0.0
    _, plain = _native.posq(*cols_of(s))
    _, out = _native.posq(*cols_of(s), row_weight=weights, gate_m=TINY_GATE)
    others = np.arange(5) != 2
    assert out["status"][2] == _native.POS_NONFINITE and out["flags"][2] == 0 and out["iters"][2] == 0
    assert out["full_pos"][others].tobytes() == plain["pos"][others].tobytes() and np.all(out["full_status"][others] == _native.POS_OK)
    # a candidate whose rows all weigh nothing: group 3 keeps weight on the rows of receiver 0 only
    weights[:] = 1.0
    rows = np.arange(s["group_ptr"][3], s["group_ptr"][4])
    weights[rows[(s["rx0"][rows] != 0) & (s["rx1"][rows] != 0)]] = 0.0
    _, out = _native.posq(*cols_of(s), row_weight=weights, gate_m=TINY_GATE)
    t = out["task_ptr"][3]
    assert out["task_rx"][t] == 0 and out["task_status"][t] == _native.POS_NONFINITE
    assert np.all(out["task_status"][t + 1:out["task_ptr"][4]] != _native.POS_NONFINITE)


def test_a_flagged_group_with_no_eligible_candidate():
    # one iteration leaves every solve THR_POS_UNCONVERGED: flagged (not dropped), but no candidate is eligible
    s = posq_golden.scene(seed=13, n_rx=6, n_groups=4, every=1)
    counts, out = check(s, gate_m=3.0, max_iter=1)
    assert counts["flagged"] == 4 and np.all(out["task_status"] == _native.POS_UNCONVERGED)
    np.testing.assert_array_equal(out["flags"], _native.POSQ_INCONSISTENT | _native.POSQ_NO_CANDIDATE)
    np.testing.assert_array_equal(out["counts"][:, 2], -1)
    # and one where candidates are eligible but the ratio is not met: clean groups under a tiny gate
    s = posq_golden.scene(seed=14, n_rx=6, n_groups=4, every=0)
    counts, out = check(s, ratio=1e-6)
    assert counts["flagged"] == 4 and np.all(out["task_status"] == _native.POS_OK)
    np.testing.assert_array_equal(out["flags"], _native.POSQ_INCONSISTENT | _native.POSQ_NO_CANDIDATE)


def test_no_iteration_evaluates_at_the_start():
    s = posq_golden.scene(seed=15, n_rx=6, n_groups=3, every=0)
    counts, out = check(s, max_iter=0)
    np.testing.assert_array_equal(out["pos"], np.full((3, 2), 0.1))
    assert not out["iters"].any() and not out["task_iters"].any() and np.all(out["status"] == _native.POS_UNCONVERGED)
    assert np.all(out["rms"][:, 0] > 1.0) and counts["flagged"] == 3


def test_a_repeated_call_returns_the_same_bytes():
    s = posq_golden.scene(seed=16, n_rx=8, n_groups=40, every=3, keep=0.8)
    weights = s["snr"]
    first = _native.posq(*cols_of(s), row_weight=weights, gate_m=3.0)
    again = _native.posq(*cols_of(s), row_weight=weights, gate_m=3.0)
    assert first[0] == again[0] and first[0]["tasks"] > 32
    for key in first[1]:
        assert first[1][key].tobytes() == again[1][key].tobytes(), key
