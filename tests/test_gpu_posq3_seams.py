"""The seams of thr_posq3 (thrifty_amd/csrc/posq3.hip, csrc/pos3_lm.hpp) in both modes, with and without a z_range:
group sizes around the register rows and the re-read loop with and without an excluded receiver, group counts around
a workgroup's 32 teams, candidates that cross a workgroup, the floors of min_rx, a candidate that pairs missing leave
underdetermined, a zero weight sum, a flagged group with no eligible candidate, a height per group, max_iter = 0,
no group at all, and a repeated call.  Everything is exact: `thr_pos3` on the same or on rebuilt groups, and the rule
of the choice on the device's own rms values (tests/posq3_golden.py)."""
import itertools

import numpy as np
import pytest

import posq3_golden
from thrifty_amd import _native

pytestmark = pytest.mark.gpu

TINY_GATE = 1e-9        # metres: every group that may be flagged is
MODES = ("h", "z", "z_open")        # known height; free z inside z_range -20 .. 100 m; free z in thr_pos3's own box
FLOOR = {"h": 5, "z": 6, "z_open": 6}


def scene(mode, seed, n_rx, n_groups, **kw):
    """posq3_golden.scene with the antennas at 3 .. 80 m; with the height known every group has a height of its own."""
    tag_z = np.linspace(0.5, 2.5, n_groups) if mode == "h" else 1.0
    return posq3_golden.scene(seed, n_rx, n_groups, z_span=(3.0, 80.0), tag_z=tag_z, **kw)


def call_of(s, mode):
    """(the columns and the mode, the keyword arguments thr_pos3 and thr_posq3 share)."""
    free_z = mode != "h"
    cols = (s["group_ptr"], s["rx0"], s["rx1"], s["tdoa"], s["snr"], s["table"], _native.POS3_FREE_Z if free_z else _native.POS3_KNOWN_HEIGHT)
    if mode == "h":
        return cols, dict(group_h=s["mobile"][:, 2].copy(), x0=(0.1, 0.1, 0.0), z_range=None)
    if mode == "z":
        return cols, dict(group_h=None, x0=(0.1, 0.1, 40.0), z_range=(-20.0, 100.0))
    return cols, dict(group_h=None, x0=(0.1, 0.1, float(s["table"][:, 2].min()) - 1.0), z_range=None)


def check(s, mode, gate_m=TINY_GATE, max_iter=100, ratio=0.5):
    """Ungated output against thr_pos3, gated candidates against thr_pos3 on rebuilt groups, the choice against the
    rule -> (counts, gated output)."""
    cols, shared = call_of(s, mode)
    want = _native.pos3(*cols, max_iter=max_iter, **shared)
    _, plain = _native.posq3(*cols, max_iter=max_iter, **shared)
    counts, out = _native.posq3(*cols, gate_m=gate_m, ratio=ratio, max_iter=max_iter, **shared)
    for key in ("pos", "dop", "hdop", "vdop", "snr", "status", "iters"):
        assert plain[key].tobytes() == want[key].tobytes(), key
    assert np.ascontiguousarray(plain["rms"][:, 0]).tobytes() == want["rms"].tobytes()
    assert out["full_pos"].tobytes() == want["pos"].tobytes() and out["snr"].tobytes() == want["snr"].tobytes()
    assert posq3_golden.assert_candidates_equal_thr_pos3(out, *cols, max_iter=max_iter, **shared) == counts["tasks"]
    posq3_golden.assert_choice_follows_the_rule(out, cols[0], cols[1], cols[2], gate_m, ratio, FLOOR[mode])
    if mode == "h":
        np.testing.assert_array_equal(out["pos"][:, 2], shared["group_h"])
        assert np.all(out["q"][:, 3:] == 0.0) and np.all(out["vdop"] == 0.0)
    return counts, out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rows", [1, 3, 8, 9, 32, 33, 40])
def test_group_sizes_around_the_register_rows(rows, mode):
    # ten receivers; the first `rows` pairs in order: receiver 9 sits in rows 8, 16, 23, 29 and 34, so leaving it
    # out switches off register rows and re-read rows; its arrival is 150 m late in every group
    pairs = list(itertools.combinations(range(10), 2))[:rows]
    s = scene(mode, rows, 10, 3, every=1, late_rx=9, pairs=pairs)
    n_rx = len({i for pr in pairs for i in pr})
    counts, out = check(s, mode, gate_m=3.0 if rows >= 32 else TINY_GATE)
    assert counts["flagged"] == (3 if n_rx >= FLOOR[mode] else 0) and counts["tasks"] == counts["flagged"] * n_rx
    if rows >= 32 and mode == "h":
        np.testing.assert_array_equal(out["counts"][:, 2], 9)
        np.testing.assert_array_equal(out["flags"], _native.POSQ3_INCONSISTENT | _native.POSQ3_EXCLUDED)
        assert np.all(out["counts"][:, 1] == rows - int(sum(9 in pr for pr in pairs)))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_groups", [0, 1, 31, 32, 33])
def test_group_counts_around_a_workgroup(n_groups, mode):
    s = scene(mode, 40 + n_groups, 6, n_groups, every=2)
    counts, out = check(s, mode, gate_m=3.0)
    assert counts == {"groups": n_groups, "rows": 15 * n_groups, "flagged": n_groups // 2, "tasks": 6 * (n_groups // 2)}
    assert out["task_ptr"].shape == (n_groups + 1,) and out["pos"].shape == (n_groups, 3) and out["used"].shape == (15 * n_groups,)
    assert out["q"].shape == (n_groups, 6) and out["task_pos"].shape == (counts["tasks"], 3)
    if mode == "h":
        np.testing.assert_array_equal(out["counts"][:, 2], s["planted"])


@pytest.mark.parametrize("mode", MODES)
def test_a_flagged_groups_candidates_straddle_a_workgroup(mode):
    s = scene(mode, 7, 6, 7, every=1)
    counts, out = check(s, mode, gate_m=3.0)
    assert (counts["flagged"], counts["tasks"]) == (7, 42)
    np.testing.assert_array_equal(out["task_ptr"], 6 * np.arange(8))
    assert out["task_ptr"][5] < 32 < out["task_ptr"][6]       # group 5: teams 30, 31 of one workgroup and 0 .. 3 of the next


@pytest.mark.parametrize("mode,named,flagged", [("h", 4, False), ("h", 5, True), ("z", 5, False), ("z", 6, True), ("z_open", 5, False),
                                                ("z_open", 6, True)])
def test_the_floor_of_min_rx_per_mode(mode, named, flagged):
    pairs = list(itertools.combinations(range(named), 2))
    s = scene(mode, 20 + named, 10, 4, every=1, late_rx=1, pairs=pairs)
    counts, out = check(s, mode)
    assert (counts["flagged"], counts["tasks"]) == ((4, 4 * named) if flagged else (0, 0))
    assert np.all(out["counts"][:, 0] >= named - 1)
    cols, shared = call_of(s, mode)
    with pytest.raises(ValueError, match="min_rx must lie in %d" % FLOOR[mode]):
        _native.posq3(*cols, min_rx=FLOOR[mode] - 1, **shared)
    raised, _ = _native.posq3(*cols, gate_m=TINY_GATE, min_rx=named + 1, **shared)
    assert raised["flagged"] == 0


@pytest.mark.parametrize("mode", MODES)
def test_a_candidate_that_missing_pairs_leave_underdetermined(mode):
    # without receiver 0 only the row (1, 2) is left: two receivers
    s = scene(mode, 11, 6, 4, every=0, pairs=[(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (1, 2)])
    counts, out = check(s, mode)
    assert (counts["flagged"], counts["tasks"]) == (4, 24)
    first = out["task_ptr"][:-1]
    np.testing.assert_array_equal(out["task_rx"][first], 0)
    np.testing.assert_array_equal(out["task_status"][first], _native.POS_UNDERDETERMINED)
    np.testing.assert_array_equal(out["task_nrx"][first], 2)
    assert np.all(out["counts"][:, 2] != 0)


@pytest.mark.parametrize("mode", MODES)
def test_a_zero_weight_sum_is_nonfinite(mode):
    s = scene(mode, 12, 7, 5, every=0)
    cols, shared = call_of(s, mode)
    weights = np.ones(len(s["tdoa"]))
    weights[s["group_ptr"][2]:s["group_ptr"][3]] = 0.0
    _, plain = _native.posq3(*cols, **shared)
    _, out = _native.posq3(*cols, row_weight=weights, gate_m=TINY_GATE, **shared)
    others = np.arange(5) != 2
    assert out["status"][2] == _native.POS_NONFINITE and out["flags"][2] == 0 and out["iters"][2] == 0
    assert out["full_pos"][others].tobytes() == plain["pos"][others].tobytes()
    assert out["full_status"][others].tobytes() == plain["status"][others].tobytes()
    # a candidate whose rows all weigh nothing: group 3 keeps weight on the rows of receiver 0 only
    weights[:] = 1.0
    rows = np.arange(s["group_ptr"][3], s["group_ptr"][4])
    weights[rows[(s["rx0"][rows] != 0) & (s["rx1"][rows] != 0)]] = 0.0
    _, out = _native.posq3(*cols, row_weight=weights, gate_m=TINY_GATE, **shared)
    t = out["task_ptr"][3]
    assert out["task_rx"][t] == 0 and out["task_status"][t] == _native.POS_NONFINITE
    assert np.all(out["task_status"][t + 1:out["task_ptr"][4]] != _native.POS_NONFINITE)


@pytest.mark.parametrize("mode", MODES)
def test_a_flagged_group_with_no_eligible_candidate(mode):
    # one iteration leaves every solve THR_POS_UNCONVERGED: flagged (not dropped), but no candidate is eligible
    s = scene(mode, 13, 7, 4, every=1)
    counts, out = check(s, mode, gate_m=3.0, max_iter=1)
    assert counts["flagged"] == 4 and np.all(out["task_status"] == _native.POS_UNCONVERGED)
    np.testing.assert_array_equal(out["flags"], _native.POSQ3_INCONSISTENT | _native.POSQ3_NO_CANDIDATE)
    np.testing.assert_array_equal(out["counts"][:, 2], -1)
    assert out["pos"].tobytes() == out["full_pos"].tobytes()      # the full solve is kept
    # and one where the ratio cannot be met: clean groups under a tiny gate
    s = scene(mode, 14, 7, 4, every=0)
    counts, out = check(s, mode, ratio=1e-6)
    assert counts["flagged"] == 4
    np.testing.assert_array_equal(out["flags"], _native.POSQ3_INCONSISTENT | _native.POSQ3_NO_CANDIDATE)
    assert out["pos"].tobytes() == out["full_pos"].tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_no_iteration_evaluates_at_the_start(mode):
    s = scene(mode, 15, 7, 3, every=0)
    counts, out = check(s, mode, max_iter=0)
    _, shared = call_of(s, mode)
    start = np.tile(np.array(shared["x0"]), (3, 1))
    if mode == "h":
        start[:, 2] = shared["group_h"]
    np.testing.assert_array_equal(out["pos"], start)
    assert not out["iters"].any() and not out["task_iters"].any() and np.all(out["status"] == _native.POS_UNCONVERGED)
    assert np.all(out["rms"][:, 0] > 1.0) and counts["flagged"] == 3


@pytest.mark.parametrize("mode", MODES)
def test_a_repeated_call_returns_the_same_bytes(mode):
    s = scene(mode, 16, 8, 40, every=3, keep=0.8)
    cols, shared = call_of(s, mode)
    first = _native.posq3(*cols, row_weight=s["snr"], gate_m=3.0, **shared)
    again = _native.posq3(*cols, row_weight=s["snr"], gate_m=3.0, **shared)
    assert first[0] == again[0] and first[0]["tasks"] > 32
    for key in first[1]:
        assert first[1][key].tobytes() == again[1][key].tobytes(), key
