"""`thr_posg3` on the device against the fixtures (tests/golden/make_golden_posg3.py) and the NumPy statement
(tests/posg3_ref.py): the volume within its derived bound, the discrete outputs exactly, every task byte for byte
`thr_pos3` from that task's start, the choice and the MIRROR flag against the rule on the device's own task outputs,
repeatability, the end-to-end claim on `z_lost6`, and the known-height mode on a flat table byte for byte `thr_posg`."""
import numpy as np
import pytest

import posg3_golden
import posg3_ref
import posg_golden
from thrifty_amd import _native, pos_3d, pos_3d_global, tdoa_est

pytestmark = pytest.mark.gpu
_runs = {}


def run(name):
    """(fixture, the device's outputs with the map of every group and the cell centres) -- computed once per fixture."""
    if name not in _runs:
        g = posg3_golden.load(name)
        n = len(g["group_id"])
        opts = posg3_golden.options(g)
        counts, out = _native.posg3(*posg3_golden.columns(g), posg3_golden.mode_of(g), map_first=0, map_count=n, **opts)
        out["counts"] = counts
        out["cx"], out["cy"], out["cz"] = posg3_ref.centres(g["rx_xyz"], opts["margin_m"], opts["grid"], opts["z_grid"], opts["grid_z"])
        _runs[name] = (g, out)
    return _runs[name]


@pytest.mark.parametrize("name", posg3_golden.SETS)
def test_cells_starts_counts_and_flags_equal_the_statements(name):
    g, out = run(name)
    n, free_z = len(g["group_id"]), bool(g["free_z"])
    assert out["counts"] == dict(groups=n, rows=len(g["rx0"]), tasks=5, starts=4, grid=32, grid_z=8 if free_z else 1, map_groups=n)
    recorded = {key: g["ref_" + key] for key in posg3_golden.RECORDED}
    posg3_golden.assert_same_discrete_outputs(out, recorded, g["ref_order_safe"])
    opts = posg3_golden.options(g)
    mine = pos_3d_global.cell_centres(g["rx_xyz"], opts["margin_m"], opts["grid"], opts["z_grid"], opts["grid_z"])
    for ours, theirs in zip(mine, (out["cx"], out["cy"], out["cz"])):
        assert (ours is None and theirs is None) or ours.tobytes() == theirs.tobytes()
    if name == "z_mirror6":
        both = _native.POSG3_AMBIGUOUS | _native.POSG3_MIRROR
        marked = (out["flags"] & both) == both
        mirrored = out["pos"] * np.array([1.0, 1.0, -1.0]) + np.array([0.0, 0.0, 60.0])
        assert marked.sum() >= 16 and np.all(np.sqrt(np.sum((out["pos2"] - mirrored)[marked] ** 2, axis=1)) <= 1e-6)
    if name == "z_tall6g":
        assert not np.any(out["flags"] & (_native.POSG3_MOVED | _native.POSG3_AMBIGUOUS))
    if not free_z:
        assert not np.any(out["flags"] & _native.POSG3_MIRROR)


@pytest.mark.parametrize("name", posg3_golden.SETS)
def test_the_volume_is_within_its_derived_bound(name):
    g, out = run(name)
    ptr, rx0, rx1, tdoa, _, table = posg3_golden.columns(g)
    gridded = ~np.isin(out["task_status"][:, 0], (_native.POS_UNDERDETERMINED, _native.POS_NONFINITE))
    np.testing.assert_array_equal(np.all(np.isnan(out["map"]), axis=(1, 2, 3)), ~gridded)
    worst, equal = 0.0, True
    for k in np.flatnonzero(gridded).tolist():
        a, b = int(ptr[k]), int(ptr[k + 1])
        cz = out["cz"] if bool(g["free_z"]) else [float(g["group_h"][k])]
        want = posg3_ref.volume(rx0[a:b], rx1[a:b], tdoa[a:b], table, out["cx"], out["cy"], cz)
        bound = posg3_golden.volume_bound(rx0[a:b], rx1[a:b], tdoa[a:b], table, out["cx"], out["cy"], cz)
        diff = np.abs(out["map"][k] - want)
        worst, equal = max(worst, float(np.max(diff / bound))), equal and out["map"][k].tobytes() == want.tobytes()
        assert np.all(diff <= bound), k
        # the minimum rule and the starts on the device's OWN volume: exact whatever the rounding
        minima = posg3_ref.local_minima(out["map"][k])
        np.testing.assert_array_equal(out["map_min"][k].astype(bool), minima)
        cells, f = posg3_ref.lowest(out["map"][k], minima, out["start_cell"].shape[1])
        assert out["start_cell"][k].tolist() == cells.tolist() and out["start_f"][k].tobytes() == f.tobytes()
    print("%s: the maps are %s (largest difference / bound: %.3g)" % (name, "EQUAL to the bit" if equal else "not equal to the bit", worst))


@pytest.mark.parametrize("name", posg3_golden.SETS)
def test_every_task_is_thr_pos3_from_its_start_to_the_bit(name):
    g, out = run(name)
    opts = posg3_golden.options(g)
    n = posg3_golden.assert_tasks_equal_thr_pos3(out, *posg3_golden.columns(g), posg3_golden.mode_of(g), opts["group_h"], opts["x0"])
    assert n == np.count_nonzero(out["task_status"] != _native.POSG3_NO_TASK) >= len(g["group_id"])


@pytest.mark.parametrize("name", posg3_golden.SETS)
def test_the_choice_follows_the_rule_on_the_devices_own_tasks(name):
    g, out = run(name)
    posg3_golden.assert_choice_follows_the_rule(out, float(g["merge_m"]), float(g["ratio"]), float(g["floor_m"]), bool(g["free_z"]))
    with np.errstate(invalid="ignore"):
        ok = out["task_status"] == _native.POS_OK
        assert np.all(out["rms"][ok.any(axis=1)] == np.min(np.where(ok, out["task_rms"], np.inf), axis=1)[ok.any(axis=1)])


def test_a_repeated_call_returns_the_same_bytes():
    g, out = run("z_mirror6")
    _, again = _native.posg3(*posg3_golden.columns(g), posg3_golden.mode_of(g), map_first=0, map_count=len(g["group_id"]),
                             **posg3_golden.options(g))
    for key in _native.POSG3_OUTPUTS:
        assert again[key].tobytes() == out[key].tobytes(), key
    assert len(_native.posg3_times()) == 6 and all(t >= 0.0 for t in _native.posg3_times())


def tdoa_groups(g):
    groups = []
    for k in range(len(g["group_id"])):
        a, b = int(g["group_ptr"][k]), int(g["group_ptr"][k + 1])
        rows = np.zeros(b - a, dtype=tdoa_est.TDOA_DTYPE)
        for name in ("rx0", "rx1", "tdoa", "snr"):
            rows[name] = g[name][a:b]
        groups.append(tdoa_est.TdoaGroup(int(g["group_id"][k]), float(g["timestamp"][k]), int(g["group_tx"][k]), rows))
    return groups


def test_the_global_solve_finds_what_the_fixed_start_loses():
    """`lost` as the generator defines it.  The fixed start: not OK, or more than 10 m from the solve started at the
    planted position.  The global solve: no eligible task, or a cost above that solve's x (1 + 1e-9) plus the rounding
    term of the residuals."""
    g = posg3_golden.load("z_lost6")
    groups, uncut = tdoa_groups(g), g["uncut"]
    fixed, found = {}, {}
    pos_3d.solve(groups, posg3_golden.rx_pos(g), free_z=True, details=fixed)
    records = pos_3d_global.solve(groups, posg3_golden.rx_pos(g), free_z=True, details=found)
    assert records["group_id"].tolist() == g["group_id"][uncut].tolist()
    assert found["z_grid"] == tuple(g["z_grid"].tolist()) and found["margin_m"] == float(g["margin_m"])
    far = np.sqrt(np.sum((fixed["pos"] - g["planted_pos"]) ** 2, axis=1)) > 10.0
    lost_fixed = uncut & ((fixed["status"] != _native.POS_OK) | far)
    ptr, table = g["group_ptr"], g["rx_xyz"]
    lost_found = np.zeros(len(uncut), dtype=bool)
    for k in np.flatnonzero(uncut).tolist():
        a, b = int(ptr[k]), int(ptr[k + 1])
        da = np.sqrt(np.sum((table[posg3_golden.dense(g, g["rx0"][a:b])] - g["planted"][k]) ** 2, axis=1))
        db = np.sqrt(np.sum((table[posg3_golden.dense(g, g["rx1"][a:b])] - g["planted"][k]) ** 2, axis=1))
        floor = float(np.sum((4.0 * 2.0 ** -53 * (np.abs(g["tdoa"][a:b] * posg3_golden.C) + da + db)) ** 2))
        eligible = found["task_status"][k, found["task"][k]] == _native.POS_OK
        lost_found[k] = not (eligible and found["rms"][k] ** 2 * (b - a) <= g["planted_rms"][k] ** 2 * (b - a) * (1 + 1e-9) + floor)
    err = np.sqrt(np.sum((found["pos"] - g["planted_pos"]) ** 2, axis=1))[uncut]
    print("z_lost6: thr_pos3 loses %d of %d groups, the global solve %d (at most %.3g m from the planted-start solve)" % (
        lost_fixed.sum(), uncut.sum(), lost_found.sum(), err.max()))
    assert lost_fixed.sum() >= 5 and lost_found.sum() == 0
    assert np.all((found["flags"][lost_fixed] & pos_3d_global.MOVED) != 0)


@pytest.mark.parametrize("name", ["far4", "three_out"])
def test_a_flat_table_at_the_known_height_gives_thr_posgs_bytes(name):
    """posg's fixtures lifted to z = 12.5 m with group_h = 12.5 m: vz is 0 everywhere, and every output thr_posg3
    shares with thr_posg -- the map and the flags included -- equals thr_posg's on the flat table byte for byte."""
    g = posg_golden.load(name)
    n = len(g["group_id"])
    ptr, rx0, rx1, tdoa, snr, flat = posg_golden.columns(g)
    opts = posg_golden.options(g)
    _, want = _native.posg(ptr, rx0, rx1, tdoa, snr, flat, map_first=0, map_count=n, **opts)
    lifted = np.c_[flat, np.full(len(flat), 12.5)]
    counts, out = _native.posg3(ptr, rx0, rx1, tdoa, snr, lifted, _native.POS3_KNOWN_HEIGHT, group_h=np.full(n, 12.5), grid_z=1,
                                map_first=0, map_count=n, **opts)
    assert counts["grid_z"] == 1 and set(_native.POSG_OUTPUTS) <= set(_native.POSG3_OUTPUTS)
    for key in _native.POSG_OUTPUTS:
        ours = out[key]
        if key in ("pos", "pos2", "task_pos"):
            there = ~np.isnan(ours[..., 0])
            assert np.all(ours[..., 2][there] == 12.5) and np.all(np.isnan(ours[..., 2][~there])), key
            ours = np.ascontiguousarray(ours[..., :2])
        if key in ("map", "map_min"):
            ours = ours[:, 0]
        assert ours.tobytes() == want[key].tobytes(), key
    exists = out["task_status"] != _native.POSG3_NO_TASK
    assert out["task_hdop"].tobytes() == out["task_dop"].tobytes() and np.all(out["task_vdop"][exists] == 0.0)
    assert out["hdop"].tobytes() == out["dop"].tobytes() and np.all(out["vdop"] == 0.0)
