"""`thr_posg` on the device against the fixtures (tests/golden/make_golden_posg.py) and the NumPy statement
(tests/posg_ref.py): the surface within its derived bound, the discrete outputs exactly, every task byte for byte
`thr_pos` from that task's start, the choice against the rule on the device's own task outputs, repeatability, and
the end-to-end claim on `far4`."""
import numpy as np
import pytest

import posg_golden
import posg_ref
from thrifty_amd import _native, pos_est, pos_global, tdoa_est

pytestmark = pytest.mark.gpu
_runs = {}


def run(name):
    """(fixture, the device's outputs with the map of every group, the statement) -- computed once per fixture."""
    if name not in _runs:
        g = posg_golden.load(name)
        n = len(g["group_id"])
        out = pos_global.global_columns(g["group_ptr"], g["rx0"], g["rx1"], g["tdoa"], g["snr"], posg_golden.rx_pos(g),
                                        map_first=0, map_count=n, **posg_golden.options(g))
        ref = posg_ref.posg_ref(*posg_golden.columns(g), **posg_golden.options(g))
        _runs[name] = (g, out, ref)
    return _runs[name]


@pytest.mark.parametrize("name", posg_golden.SETS)
def test_cells_starts_counts_and_flags_equal_the_statements(name):
    g, out, ref = run(name)
    assert out["counts"] == dict(groups=len(g["group_id"]), rows=len(g["rx0"]), tasks=5, starts=4, grid=32, map_groups=len(g["group_id"]))
    posg_golden.assert_same_discrete_outputs(out, ref, g["ref_order_safe"])
    recorded = {key: g["ref_" + key] for key in posg_golden.RECORDED}
    posg_golden.assert_same_discrete_outputs(out, recorded, g["ref_order_safe"])
    assert out["cx"].tobytes() == ref["cx"].tobytes() and out["cy"].tobytes() == ref["cy"].tobytes()


@pytest.mark.parametrize("name", posg_golden.SETS)
def test_the_surface_is_within_its_derived_bound(name):
    g, out, ref = run(name)
    ptr, rx0, rx1, tdoa, _, table = posg_golden.columns(g)
    gridded = ~np.all(np.isnan(ref["map"]), axis=(1, 2))
    np.testing.assert_array_equal(np.all(np.isnan(out["map"]), axis=(1, 2)), ~gridded)
    worst = 0.0
    for k in np.flatnonzero(gridded).tolist():
        a, b = int(ptr[k]), int(ptr[k + 1])
        bound = posg_golden.surface_bound(rx0[a:b], rx1[a:b], tdoa[a:b], table, ref["cx"], ref["cy"])
        diff = np.abs(out["map"][k] - ref["map"][k])
        worst = max(worst, float(np.max(diff / bound)))
        assert np.all(diff <= bound), k
    print("%s: the maps are %s (largest difference / bound: %.3g)" % (
        name, "EQUAL to the bit" if out["map"].tobytes() == ref["map"].tobytes() else "not equal to the bit", worst))
    picked = out["start_cell"] >= 0
    flat = out["map"].reshape(len(out["map"]), -1)
    assert out["start_f"][picked].tobytes() == flat[np.nonzero(picked)[0], out["start_cell"][picked]].tobytes()


@pytest.mark.parametrize("name", posg_golden.SETS)
def test_every_task_is_thr_pos_from_its_start_to_the_bit(name):
    g, out, _ = run(name)
    n = posg_golden.assert_tasks_equal_thr_pos(out, *posg_golden.columns(g), out["cx"], out["cy"])
    assert n == np.count_nonzero(out["task_status"] != _native.POSG_NO_TASK) >= len(g["group_id"])


@pytest.mark.parametrize("name", posg_golden.SETS)
def test_the_choice_follows_the_rule_on_the_devices_own_tasks(name):
    g, out, _ = run(name)
    posg_golden.assert_choice_follows_the_rule(out, float(g["merge_m"]), float(g["ratio"]), float(g["floor_m"]))
    with np.errstate(invalid="ignore"):
        ok = out["task_status"] == _native.POS_OK
        assert np.all(out["rms"][ok.any(axis=1)] == np.min(np.where(ok, out["task_rms"], np.inf), axis=1)[ok.any(axis=1)])


def test_a_repeated_call_returns_the_same_bytes():
    g, out, _ = run("three_out")
    again = pos_global.global_columns(g["group_ptr"], g["rx0"], g["rx1"], g["tdoa"], g["snr"], posg_golden.rx_pos(g),
                                      map_first=0, map_count=len(g["group_id"]), **posg_golden.options(g))
    for key in _native.POSG_OUTPUTS:
        assert again[key].tobytes() == out[key].tobytes(), key
    assert len(_native.posg_times()) == 6 and all(t >= 0.0 for t in _native.posg_times())


def test_the_global_solve_finds_what_the_fixed_start_loses():
    g = posg_golden.load("far4")
    groups = []
    for k in range(len(g["group_id"])):
        a, b = int(g["group_ptr"][k]), int(g["group_ptr"][k + 1])
        rows = np.zeros(b - a, dtype=tdoa_est.TDOA_DTYPE)
        for name in ("rx0", "rx1", "tdoa", "snr"):
            rows[name] = g[name][a:b]
        groups.append(tdoa_est.TdoaGroup(int(g["group_id"][k]), float(g["timestamp"][k]), 7, rows))
    fixed = pos_est.solve(groups, posg_golden.rx_pos(g))
    found = pos_global.solve(groups, posg_golden.rx_pos(g))
    assert fixed["group_id"].tolist() == found["group_id"].tolist() == g["group_id"].tolist()
    err_fixed = np.hypot(fixed["x"] - g["planted"][:, 0], fixed["y"] - g["planted"][:, 1])
    err_found = np.hypot(found["x"] - g["planted"][:, 0], found["y"] - g["planted"][:, 1])
    print("far4: thr_pos leaves %d of %d groups more than 10 m from the planted position, the global solve %d (worst %.2f m)" % (
        np.count_nonzero(err_fixed > 10.0), len(fixed), np.count_nonzero(err_found > 10.0), err_found.max()))
    assert np.count_nonzero(err_fixed > 10.0) >= 4 and np.count_nonzero(err_found > 10.0) == 0
    np.testing.assert_array_equal((found["flags"] & pos_global.MOVED) != 0, err_fixed > 10.0)
