"""`thr_posg3` at its seams: the plane counts around the rolling window of three planes, both grids, 1, 4 and 8 starts, the
lowest minimum in the first and in the last plane, fewer minima than starts, a later plane displacing an earlier pick;
group lengths around the team and the row chunk (a longer group stages its chunks again for every plane); group counts
around the task workgroup; the receiver threshold of the distance table; the map range; max_iter 0 and 3; NaN,
underdetermined and empty groups; a z_grid that touches the z box; a constant volume.

Every case is held, exactly, to the minimum rule and the start order applied in NumPy to the device's OWN volume, to
`thr_pos3` for every task's bits and to the choice rule on the device's own task outputs; the volume itself is held to
the NumPy statement (tests/posg3_ref.py) within the derived bound."""
import numpy as np
import pytest

import posg3_golden
import posg3_ref
from thrifty_amd import _native

pytestmark = pytest.mark.gpu
CHUNK = _native.POSG3_ROW_CHUNK
FREE_Z, KNOWN_HEIGHT = _native.POS3_FREE_Z, _native.POS3_KNOWN_HEIGHT


def margin_of(table):
    return float(np.max(table[:, :2].max(axis=0) - table[:, :2].min(axis=0)))


def device(s, mode=FREE_Z, **kw):
    kw.setdefault("margin_m", margin_of(s["table"]))
    if mode == FREE_Z:
        kw.setdefault("z_grid", posg3_golden.default_z_grid(s["table"]))
        kw.setdefault("x0", (0.1, 0.1, float(s["table"][:, 2].min()) - 1.0))
    else:
        kw.setdefault("grid_z", 1)
    counts, out = _native.posg3(s["group_ptr"], s["rx0"], s["rx1"], s["tdoa"], s["snr"], s["table"], mode, **kw)
    return counts, out, kw


def check(s, mode=FREE_Z, maps=True, **kw):
    """One call with the map of every group -> out, held to the rules (the module docstring)."""
    n = len(s["group_ptr"]) - 1
    if maps:
        kw.update(map_first=0, map_count=n)
    counts, out, kw = device(s, mode, **kw)
    free_z = mode == FREE_Z
    grid, grid_z, starts = kw.get("grid", 32), kw.get("grid_z", 8), kw.get("starts", 4)
    assert counts["groups"] == n and counts["tasks"] == out["task_status"].shape[1] == starts + 1 and counts["grid_z"] == grid_z
    out["cx"], out["cy"], out["cz"] = posg3_ref.centres(s["table"], kw["margin_m"], grid, kw.get("z_grid"), grid_z)
    posg3_golden.assert_tasks_equal_thr_pos3(out, s["group_ptr"], s["rx0"], s["rx1"], s["tdoa"], s["snr"], s["table"], mode,
                                             kw.get("group_h"), kw.get("x0", (0.1, 0.1, 0.0)), kw.get("z_range"), kw.get("max_iter", 100))
    posg3_golden.assert_choice_follows_the_rule(out, kw.get("merge_m", 1.0), kw.get("ratio", 2.0), kw.get("floor_m", 0.0), free_z)
    gridded = ~np.isin(out["task_status"][:, 0], (_native.POS_UNDERDETERMINED, _native.POS_NONFINITE))
    assert np.all(out["n_local"][~gridded] == 0) and np.all(out["start_cell"][~gridded] == -1)
    assert np.all(out["task_status"][~gridded, 1:] == _native.POSG3_NO_TASK)
    np.testing.assert_array_equal(out["start_cell"] < 0, np.isnan(out["start_f"]))
    if maps:
        assert out["map"].shape == (n, grid_z, grid, grid)
        for k in range(n):
            a, b = int(s["group_ptr"][k]), int(s["group_ptr"][k + 1])
            if not gridded[k]:
                assert np.all(np.isnan(out["map"][k])) and not out["map_min"][k].any()
                continue
            cz = out["cz"] if free_z else [float(kw["group_h"][k])]
            want = posg3_ref.volume(s["rx0"][a:b], s["rx1"][a:b], s["tdoa"][a:b], s["table"], out["cx"], out["cy"], cz)
            bound = posg3_golden.volume_bound(s["rx0"][a:b], s["rx1"][a:b], s["tdoa"][a:b], s["table"], out["cx"], out["cy"], cz)
            assert np.all(np.abs(out["map"][k] - want) <= bound), k
            minima = posg3_ref.local_minima(out["map"][k])
            np.testing.assert_array_equal(out["map_min"][k].astype(bool), minima)
            assert int(out["n_local"][k]) == int(minima.sum())
            cells, f = posg3_ref.lowest(out["map"][k], minima, starts)
            assert out["start_cell"][k].tolist() == cells.tolist() and out["start_f"][k].tobytes() == f.tobytes(), k
    return out


def ring(seed, n_groups, n_rx=6, rows=None, z_span=(2.0, 42.0), radius=300.0, noise=3e-9):
    return posg3_golden.ring_scene(seed, n_rx, radius, z_span, noise, n_groups, rows=rows)


@pytest.mark.parametrize("grid_z", [2, 3, 8, 16, 32])
def test_plane_counts_around_the_window_of_three(grid_z):
    out = check(ring(21, 6), grid_z=grid_z)
    assert np.all(out["n_local"] >= 1) and np.all(out["start_cell"][:, 0] >= 0)


@pytest.mark.parametrize("grid, starts", [(16, 1), (16, 8), (32, 1), (32, 8)])
def test_both_grids_and_the_number_of_starts(grid, starts):
    out = check(ring(22, 6), grid=grid, starts=starts, grid_z=5)
    assert out["start_cell"].shape == (6, starts)
    if starts == 8:          # fewer minima than starts: the slots after them are empty and their tasks do not exist
        short = out["n_local"] < starts
        assert short.any()
        for g in np.flatnonzero(short).tolist():
            k = int(out["n_local"][g])
            assert np.all(out["start_cell"][g, :k] >= 0) and np.all(out["start_cell"][g, k:] == -1)
            assert np.all(out["task_status"][g, 1 + k:] == _native.POSG3_NO_TASK)


def mirror_scene():
    g = posg3_golden.load("z_mirror6")
    ptr, rx0, rx1, tdoa, snr, table = posg3_golden.columns(g)
    return dict(group_ptr=ptr, rx0=rx0, rx1=rx1, tdoa=tdoa, snr=snr, table=table)


@pytest.mark.parametrize("z_grid", [(-5.0, 75.0), (-45.0, 5.0)])
def test_the_lowest_minimum_in_the_first_and_in_the_last_plane(z_grid):
    """z_mirror6 with a shifted z_grid: coplanar antennas hardly determine the height, and either grid has groups whose
    lowest minimum lies in plane 0 and groups where it lies in plane 7 (the statement says so on the CPU), where half of
    the neighbours are outside."""
    out = check(mirror_scene(), z_grid=z_grid, x0=(0.1, 0.1, 1.0))
    first = out["start_cell"][:, 0] // 1024
    assert np.any(first == 0) and np.any(first == 7)


@pytest.mark.parametrize("starts", [1, 8])
def test_a_later_plane_displaces_an_earlier_pick(starts):
    """With the grid below, the mirror minimum near 58 m (plane 6) is lower on the raster than the one near 2 m (plane 1)
    in a share of z_mirror6's groups: the running list must give way."""
    out = check(mirror_scene(), z_grid=(-8.0, 70.0), starts=starts, x0=(0.1, 0.1, 1.0))
    first = out["start_cell"][:, 0] // 1024
    lowest_plane = np.array([int(np.flatnonzero(m.reshape(8, -1).any(axis=1))[0]) for m in out["map_min"]])
    assert np.any(first > lowest_plane), "no group's lowest minimum lies above its first plane with a minimum"


def test_group_lengths_around_the_team_the_registers_and_the_row_chunk():
    lengths = [0, 1, 3, 8, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
    s = ring(23, len(lengths), rows=lengths)
    assert np.diff(s["group_ptr"]).tolist() == lengths
    out = check(s, grid_z=4)
    assert out["task_status"][:2, 0].tolist() == [_native.POS_UNDERDETERMINED] * 2       # 0 rows and 1 row; 3 rows name four receivers
    assert np.all(out["n_local"][2:] >= 1) and np.all(out["task_status"][2:, 1] != _native.POSG3_NO_TASK)
    known = check(s, KNOWN_HEIGHT, group_h=s["planted"][:, 2].copy())
    assert known["task_status"][:2, 0].tolist() == [_native.POS_UNDERDETERMINED] * 2 and np.all(known["n_local"][2:] >= 1)


def test_group_counts_around_the_task_workgroup():
    s = ring(24, 65)
    _, whole, _ = device(s, starts=1, grid=16, grid_z=2)
    per_group = [k for k in _native.POSG3_OUTPUTS if k not in ("map", "map_min")]
    for n in (0, 1, 63, 64):
        rows = int(s["group_ptr"][n])
        part = dict(s, group_ptr=s["group_ptr"][:n + 1], rx0=s["rx0"][:rows], rx1=s["rx1"][:rows], tdoa=s["tdoa"][:rows], snr=s["snr"][:rows])
        counts, out, _ = device(part, starts=1, grid=16, grid_z=2)
        assert counts["groups"] == n and counts["rows"] == rows
        for key in per_group:
            assert out[key].tobytes() == whole[key][:n].tobytes(), (n, key)
    check(dict(s, group_ptr=s["group_ptr"][:10], **{k: s[k][:int(s["group_ptr"][9])] for k in ("rx0", "rx1", "tdoa", "snr")}),
          grid=16, grid_z=2, maps=False)                                # 8 groups x 4 starts fill one workgroup, plus one


def test_both_volume_paths_give_the_same_bytes_at_the_receiver_threshold():
    """Up to POSG3_DIST_RECEIVERS receivers a cell's distances are taken once per receiver, above it twice per row."""
    limit = _native.POSG3_DIST_RECEIVERS
    s = ring(25, 4, rows=[10, 33, 7, 64])
    kw = dict(grid_z=3, map_first=0, map_count=4, margin_m=margin_of(s["table"]), z_grid=posg3_golden.default_z_grid(s["table"]))
    _, plain, _ = device(s, **kw)
    for n_rx in (limit - 1, limit, limit + 1, 64):              # further receivers on top of receiver 0: the same volume
        padded = dict(s, table=np.concatenate([s["table"], np.repeat(s["table"][:1], n_rx - 6, axis=0)]))
        _, out, _ = device(padded, **kw)
        for key in _native.POSG3_OUTPUTS:
            assert out[key].tobytes() == plain[key].tobytes(), (n_rx, key)
    for n_rx in (limit, limit + 1):                             # and every receiver named, on either side of the threshold
        out = check(ring(26, 2, n_rx=n_rx, rows=[2 * n_rx, 40]), grid_z=2)
        assert np.all(out["n_local"] >= 1)


def test_the_map_range():
    s = ring(27, 7)
    _, whole, _ = device(s, grid=16, grid_z=3, map_first=0, map_count=7)
    for first, count in ((0, 1), (6, 1), (2, 3), (0, 0), (7, 0)):
        counts, out, _ = device(s, grid=16, grid_z=3, map_first=first, map_count=count)
        assert counts["map_groups"] == count and out["map"].shape == (count, 3, 16, 16)
        assert out["map"].tobytes() == whole["map"][first:first + count].tobytes()
        assert out["map_min"].tobytes() == whole["map_min"][first:first + count].tobytes()
        assert out["start_cell"].tobytes() == whole["start_cell"].tobytes()
    for first, count in ((7, 1), (5, 3), (0, 8), (-1, 1), (0, 257)):
        with pytest.raises(ValueError, match="thr_posg3"):
            device(s, map_first=first, map_count=count)


def test_max_iter_zero_and_three():
    s = ring(28, 4)
    out = check(s, max_iter=0)
    assert np.all(out["task_iters"] == 0) and np.all(out["task_status"][:, 0] == _native.POS_UNCONVERGED)
    assert np.all(out["flags"] == _native.POSG3_NO_MINIMUM | _native.POSG3_MOVED) and np.all(out["pos"] == [0.1, 0.1, 1.0])
    there = out["start_cell"] >= 0
    assert out["task_pos"][:, 1:, 2][there].tolist() == out["cz"][out["start_cell"][there] // 1024].tolist()
    out = check(s, max_iter=3)            # nothing converges in three steps from 300 m away: thr_pos3's answer, flagged
    assert np.all(out["task_status"][:, 0] == _native.POS_UNCONVERGED) and np.all(out["task_iters"][:, 0] == 3)
    none = (out["task_status"] != _native.POS_OK).all(axis=1)
    assert none.any() and np.all(out["flags"][none] == _native.POSG3_NO_MINIMUM | _native.POSG3_MOVED)
    assert np.all(out["task"][none] == 0) and out["pos"][none].tobytes() == out["task_pos"][none, 0].tobytes()


def test_nan_underdetermined_and_empty_groups_get_no_grid():
    s = ring(29, 5, rows=[8, 8, 1, 0, 8])
    s["tdoa"][9] = np.nan                                               # group 1
    out = check(s, grid_z=4)
    assert out["task_status"][1:4, 0].tolist() == [_native.POS_NONFINITE, _native.POS_UNDERDETERMINED, _native.POS_UNDERDETERMINED]
    assert np.all(out["n_local"][[0, 4]] >= 1) and not np.any(np.isnan(out["map"][[0, 4]]))
    for g in (1, 2, 3):
        assert int(out["flags"][g]) == _native.POSG3_NO_MINIMUM | _native.POSG3_MOVED and int(out["task"][g]) == 0
        assert int(out["status"][g]) == int(out["task_status"][g, 0]) and int(out["n_minima"][g]) == 0
        assert out["pos"][g].tolist() == [0.1, 0.1, 1.0]
    assert np.isnan(out["snr"][3])
    clean = ring(29, 5, rows=[8, 8, 1, 0, 8])
    _, alone, _ = device(clean, grid_z=4, map_first=0, map_count=5)
    for key in _native.POSG3_OUTPUTS:                                   # the NaN moved its own group only
        assert out[key][[0, 2, 3, 4]].tobytes() == alone[key][[0, 2, 3, 4]].tobytes(), key


def test_a_z_grid_may_touch_the_z_box_and_no_farther():
    s = ring(30, 3)
    out = check(s, z_range=(-20.0, 90.0), z_grid=(-20.0, 90.0), x0=(0.1, 0.1, 1.0), grid_z=4)
    assert np.all(out["n_local"] >= 1)
    box = (2.0 - 10e3, 42.0 + 10e3)
    check(s, z_grid=box, grid_z=2, maps=False)
    bad = [dict(z_range=(-20.0, 90.0), z_grid=(-20.000001, 90.0), x0=(0.1, 0.1, 1.0)), dict(z_grid=(box[0] - 1.0, 50.0)),
           dict(z_grid=(5.0, 5.0)), dict(z_grid=(9.0, 5.0)), dict(z_grid=(float("nan"), 5.0)), dict(z_grid=(0.0, float("inf"))),
           dict(grid_z=1), dict(grid_z=33), dict(grid=64), dict(starts=0), dict(starts=9), dict(merge_m=0.0), dict(ratio=0.5),
           dict(floor_m=-1.0), dict(margin_m=10e3 + 1e-6), dict(max_iter=-1)]
    for kw in bad:
        with pytest.raises(ValueError, match="thr_posg3"):
            device(s, **kw)
    with pytest.raises(ValueError, match="needs z_grid"):
        _native.posg3(s["group_ptr"], s["rx0"], s["rx1"], s["tdoa"], s["snr"], s["table"], FREE_Z, 100.0, x0=(0.1, 0.1, 1.0))
    with pytest.raises(ValueError, match="grid_z must be 1"):
        device(s, KNOWN_HEIGHT, group_h=np.zeros(3), grid_z=2)


def test_a_constant_volume_has_one_local_minimum_in_cell_0():
    table = np.array([[0.0, 0.0, 5.0], [100.0, 0.0, 9.0], [0.0, 100.0, 2.0], [80.0, 90.0, 20.0]])
    s = {"table": table, "group_ptr": np.array([0, 4], dtype=np.int64), "rx0": np.arange(4, dtype=np.int32),
         "rx1": np.arange(4, dtype=np.int32), "tdoa": np.full(4, 1e-8), "snr": np.ones(4)}
    out = check(s, grid_z=5)
    tc = 1e-8 * posg3_golden.C
    assert np.all(out["map"] == ((tc * tc + tc * tc) + tc * tc) + tc * tc) and out["n_local"].tolist() == [1]
    assert out["map_min"][0, 0, 0, 0] == 1 and out["start_cell"].tolist() == [[0, -1, -1, -1]]
    assert out["start_f"][0, 0] == out["map"][0, 0, 0, 0] and out["task_status"][0, 2:].tolist() == [-1, -1, -1]
