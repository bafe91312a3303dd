"""`thr_posg` at its seams: group lengths around the 8-lane team, the register rows and the row-staging chunk; the
three grids; 1, 4 and 8 starts; fewer local minima than starts; a minimum on the edge of the search area; a constant
surface; NaN, underdetermined and empty groups; group counts around the wave and the workgroup of the task kernel; the
map range; max_iter = 0; the margin's limit.  Every case is held to the NumPy statement (tests/posg_ref.py) for the
discrete outputs, to `thr_pos` for every task's bits and to the choice rule on the device's own task outputs."""
import numpy as np
import pytest

import posg_golden
import posg_ref
from thrifty_amd import _native, pos_global

pytestmark = pytest.mark.gpu
CHUNK = _native.POSG_ROW_CHUNK


def device(s, margin_m=None, **kw):
    margin_m = posg_golden.margin_of(s["table"]) if margin_m is None else margin_m
    counts, out = _native.posg(s["group_ptr"], s["rx0"], s["rx1"], s["tdoa"], s["snr"], s["table"], margin_m, **kw)
    return counts, out, margin_m


def check(s, margin_m=None, maps=True, **kw):
    """One call with the map of every group -> (out, ref), held to the statement, to thr_pos and to the choice rule."""
    n = len(s["group_ptr"]) - 1
    if maps:
        kw.update(map_first=0, map_count=n)
    counts, out, margin_m = device(s, margin_m, **kw)
    opts = {k: v for k, v in kw.items() if k not in ("map_first", "map_count")}
    ref = posg_ref.posg_ref(s["group_ptr"], s["rx0"], s["rx1"], s["tdoa"], s["snr"], s["table"], margin_m, **opts)
    assert counts["groups"] == n and counts["tasks"] == out["task_status"].shape[1] == opts.get("starts", 4) + 1
    posg_golden.assert_same_discrete_outputs(out, ref)
    posg_golden.assert_tasks_equal_thr_pos(out, s["group_ptr"], s["rx0"], s["rx1"], s["tdoa"], s["snr"], s["table"], ref["cx"], ref["cy"],
                                           max_iter=opts.get("max_iter", 100))
    posg_golden.assert_choice_follows_the_rule(out, opts.get("merge_m", 1.0), opts.get("ratio", 2.0), opts.get("floor_m", 0.0))
    if maps:
        for k in range(n):
            a, b = int(s["group_ptr"][k]), int(s["group_ptr"][k + 1])
            if np.all(np.isnan(ref["map"][k])):
                assert np.all(np.isnan(out["map"][k]))
                continue
            bound = posg_golden.surface_bound(s["rx0"][a:b], s["rx1"][a:b], s["tdoa"][a:b], s["table"], ref["cx"], ref["cy"])
            assert np.all(np.abs(out["map"][k] - ref["map"][k]) <= bound), k
    return out, ref


def test_group_lengths_around_the_team_the_registers_and_the_row_chunk():
    lengths = [1, 3, 8, 9, 32, 33, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1, 5]
    s = posg_golden.scene(3, 5, len(lengths), 0.3, offset=posg_golden.OFFSET, rows=lengths)
    assert np.diff(s["group_ptr"]).tolist() == lengths
    out, ref = check(s)
    assert out["task_status"][0, 0] == _native.POS_UNDERDETERMINED and np.all(out["start_cell"][0] == -1)      # one row: two receivers
    assert np.all(out["n_local"][1:] >= 1) and np.all(out["task_status"][1:, 1] != _native.POSG_NO_TASK)


@pytest.mark.parametrize("starts", [1, 4, 8])
def test_starts_and_fewer_local_minima_than_starts(starts):
    s = posg_golden.scene(5, 4, 12, 0.3, offset=posg_golden.OFFSET)
    out, _ = check(s, starts=starts)
    assert out["start_cell"].shape == (12, starts) and np.all(out["start_cell"][:, 0] >= 0)
    if starts == 8:
        short = out["n_local"] < starts
        assert short.any()
        for g in np.flatnonzero(short).tolist():
            k = int(out["n_local"][g])
            assert np.all(out["start_cell"][g, :k] >= 0) and np.all(out["start_cell"][g, k:] == -1)
            assert np.all(out["task_status"][g, 1 + k:] == _native.POSG_NO_TASK)
    f = np.where(out["start_cell"] >= 0, out["start_f"], np.finfo(np.float64).max)
    assert np.all(np.diff(f, axis=1) >= 0)


def test_the_three_grids_reach_the_same_best_minimum():
    s = posg_golden.scene(7, 5, 6, 0.3, offset=posg_golden.OFFSET)
    best = {}
    for grid in _native.POSG_GRIDS:
        out, _ = check(s, grid=grid)
        assert out["map"].shape == (6, grid, grid) and not np.any(out["flags"] & _native.POSG_NO_MINIMUM)
        best[grid] = out["pos"]
    assert np.max(np.abs(best[16] - best[32])) <= 1e-9 and np.max(np.abs(best[64] - best[32])) <= 1e-9


def test_a_planted_position_outside_the_search_area_gives_an_edge_minimum():
    s = posg_golden.scene(2, 4, 8, 0.3, outside=True)
    out, ref = check(s, margin_m=5.0)
    cells = out["start_cell"][out["start_cell"] >= 0]
    i, j = cells % 32, cells // 32
    assert np.any((i == 0) | (i == 31) | (j == 0) | (j == 31))
    lo, hi = s["table"].min(axis=0) - 5.0, s["table"].max(axis=0) + 5.0
    ok = out["task_status"] == _native.POS_OK
    outside = np.any((out["task_pos"] < lo) | (out["task_pos"] > hi), axis=2)
    assert np.any(ok & outside)                                         # the iteration walked out of the area


def test_a_constant_surface_has_one_local_minimum_in_cell_0():
    table = np.array([[0.0, 0.0], [100.0, 0.0], [0.0, 100.0]])
    s = {"table": table, "group_ptr": np.array([0, 3], dtype=np.int64), "rx0": np.array([0, 1, 2], dtype=np.int32),
         "rx1": np.array([0, 1, 2], dtype=np.int32), "tdoa": np.full(3, 1e-8), "snr": np.ones(3)}
    out, ref = check(s)
    tc = 1e-8 * posg_golden.C
    assert np.all(out["map"] == (tc * tc + tc * tc) + tc * tc) and out["n_local"].tolist() == [1] and out["map_min"][0, 0, 0] == 1
    assert out["start_cell"].tolist() == [[0, -1, -1, -1]] and out["start_f"][0, 0] == out["map"][0, 0, 0]
    assert out["task_status"].tolist() == [[0, 0, -1, -1, -1]] and out["task_iters"].tolist() == [[1, 1, 0, 0, 0]]
    assert out["task_pos"][0, 1].tolist() == [ref["cx"][0], ref["cy"][0]] and out["task_pos"][0, 0].tolist() == [0.1, 0.1]
    # equal rms: the lower task is the best, the other a second minimum that fits as well
    assert (int(out["task"][0]), int(out["n_minima"][0]), int(out["flags"][0])) == (0, 2, _native.POSG_AMBIGUOUS)
    assert out["rms"][0] == out["rms2"][0] == np.sqrt((tc * tc + tc * tc + tc * tc) / 3.0) and out["dop"][0] == -1.0


def test_nan_underdetermined_and_empty_groups_get_no_grid():
    s = posg_golden.scene(4, 4, 5, 0.3, offset=posg_golden.OFFSET, rows=[6, 6, 1, 0, 6])
    s["tdoa"][7] = np.nan                                               # group 1
    out, _ = check(s)
    assert out["task_status"][1:4, 0].tolist() == [_native.POS_NONFINITE, _native.POS_UNDERDETERMINED, _native.POS_UNDERDETERMINED]
    assert np.all(np.isin(out["task_status"][[0, 4], 0], (_native.POS_OK, _native.POS_AT_BOUND))) and np.all(out["n_local"][[0, 4]] >= 1)
    for g in (1, 2, 3):
        assert int(out["flags"][g]) == _native.POSG_NO_MINIMUM | _native.POSG_MOVED and int(out["task"][g]) == 0
        assert int(out["status"][g]) == int(out["task_status"][g, 0]) and int(out["n_minima"][g]) == 0
        assert np.all(out["start_cell"][g] == -1) and int(out["n_local"][g]) == 0 and np.all(np.isnan(out["map"][g]))
        assert np.all(out["task_status"][g, 1:] == _native.POSG_NO_TASK) and not out["map_min"][g].any()
        assert out["pos"][g].tolist() == [0.1, 0.1]
    assert np.isnan(out["snr"][3]) and not np.any(out["flags"][[0, 4]] & _native.POSG_NO_MINIMUM)


def test_group_counts_around_the_wave_and_the_task_workgroup():
    s = posg_golden.scene(6, 4, 65, 0.3, offset=posg_golden.OFFSET)
    whole, _ = check(s, starts=1, maps=False)
    per_group = [k for k in _native.POSG_OUTPUTS if k not in ("map", "map_min")]
    for n in (0, 1, 32, 33, 63, 64):                                    # 32 teams fill one workgroup of the task kernel
        rows = int(s["group_ptr"][n])
        part = dict(s, group_ptr=s["group_ptr"][:n + 1], rx0=s["rx0"][:rows], rx1=s["rx1"][:rows], tdoa=s["tdoa"][:rows], snr=s["snr"][:rows])
        counts, out, _ = device(part, starts=1)
        assert counts["groups"] == n and counts["rows"] == rows
        for key in per_group:
            assert out[key].tobytes() == whole[key][:n].tobytes(), (n, key)
    more, _ = check(posg_golden.scene(6, 4, 9, 0.3, offset=posg_golden.OFFSET), starts=4, maps=False)     # 8 groups x 4 starts fill one, plus one
    assert more["task_status"].shape == (9, 5)


def test_both_surface_paths_give_the_same_bytes_at_the_receiver_threshold():
    """Up to POSG_DIST_RECEIVERS receivers a cell's distances are taken once per receiver, above it twice per row."""
    limit = _native.POSG_DIST_RECEIVERS
    s = posg_golden.scene(11, 5, 6, 0.3, offset=posg_golden.OFFSET, rows=[10, 10, 33, 7, 64, 10])
    margin = posg_golden.margin_of(s["table"])
    _, plain, _ = device(s, margin, map_first=0, map_count=6)
    for n_rx in (limit - 1, limit, limit + 1, 64):              # further receivers on top of receiver 0: the same area
        padded = dict(s, table=np.concatenate([s["table"], np.repeat(s["table"][:1], n_rx - 5, axis=0)]))
        _, out, _ = device(padded, margin, map_first=0, map_count=6)
        for key in _native.POSG_OUTPUTS:
            assert out[key].tobytes() == plain[key].tobytes(), (n_rx, key)
    for n_rx in (limit, limit + 1):                             # and every receiver named, on either side of the threshold
        out, _ = check(posg_golden.scene(12, n_rx, 3, 0.3, offset=posg_golden.OFFSET, rows=[40, n_rx, 70],
                                         pairs=[(k % n_rx, (k + 1 + k // n_rx) % n_rx) for k in range(2 * n_rx)]))
        assert np.all(out["n_local"] >= 1)


def test_the_map_range():
    s = posg_golden.scene(8, 4, 7, 0.3, offset=posg_golden.OFFSET)
    _, whole, _ = device(s, map_first=0, map_count=7)
    for first, count in ((0, 1), (6, 1), (2, 3), (0, 0), (7, 0)):
        counts, out, _ = device(s, map_first=first, map_count=count)
        assert counts["map_groups"] == count and out["map"].shape == (count, 32, 32)
        assert out["map"].tobytes() == whole["map"][first:first + count].tobytes()
        assert out["map_min"].tobytes() == whole["map_min"][first:first + count].tobytes()
        assert out["start_cell"].tobytes() == whole["start_cell"].tobytes()
    for first, count in ((7, 1), (5, 3), (0, 8), (-1, 1), (0, 257)):
        with pytest.raises(ValueError, match="thr_posg"):
            device(s, map_first=first, map_count=count)


def test_max_iter_zero_leaves_every_task_at_its_start():
    s = posg_golden.scene(9, 4, 4, 0.3, offset=posg_golden.OFFSET)
    out, ref = check(s, max_iter=0)
    there = out["start_cell"] >= 0
    assert np.all(out["task_iters"] == 0) and np.all(out["task_status"][:, 0] == _native.POS_UNCONVERGED)
    assert np.all(out["flags"] == _native.POSG_NO_MINIMUM | _native.POSG_MOVED) and np.all(out["pos"] == [0.1, 0.1])
    assert out["task_pos"][:, 1:, 0][there].tolist() == ref["cx"][out["start_cell"][there] % 32].tolist()
    # the rms of a task at its start cell is the surface there, summed in the team's order instead of the rows'
    np.testing.assert_allclose(out["task_rms"][:, 1:][there], np.sqrt(out["start_f"][there] / 6.0), rtol=1e-13)


def test_the_margin_may_reach_thr_pos_box_and_no_farther():
    s = posg_golden.scene(10, 4, 3, 0.3)
    out, _ = check(s, margin_m=10e3, maps=False)
    assert np.all(out["n_local"] >= 1)
    for margin in (10e3 + 1e-6, 0.0, -5.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="thr_posg: margin_m"):
            device(s, margin_m=margin)
    for bad in (dict(grid=48), dict(starts=0), dict(starts=9), dict(merge_m=0.0), dict(ratio=0.99), dict(floor_m=-1.0), dict(max_iter=-1)):
        with pytest.raises(ValueError, match="thr_posg"):
            device(s, **bad)
    with pytest.raises(ValueError, match="receivers"):
        _native.posg(s["group_ptr"], s["rx0"] + 4, s["rx1"], s["tdoa"], s["snr"], s["table"], 50.0)
    with pytest.raises(ValueError, match="2 dimensions"):
        _native.posg(s["group_ptr"], s["rx0"], s["rx1"], s["tdoa"], s["snr"], s["table"][:, :1].copy(), 50.0)
