"""`tdoa` on the device against the fixtures the reference's `estimate_tdoas` produced
(tests/golden/make_golden_tdoa.py).  Exact: groups, receivers, detection indices, the row order, the
failures, and per detection pair the window length and the number of pairs the outlier mask kept.
`tdoa` must be as close to the EXACT least-squares answer (stored in the fixture) as the reference is
(ref_err_max, 1x) and within 2 ref_err_max of the reference; snr relative 1e-14, model_quality 1e-12.

Measured on an MI355X (max |tdoa - exact|, device / reference): see DESIGN.md 3.8."""
import sys

import numpy as np
import pytest

import tdoa_golden
from thrifty_amd import _native, matchmaker, tdoa_est

pytestmark = pytest.mark.gpu


def cols_of(g):
    return {key: g[key] for key in ("rxid", "txid", "timestamp", "soa", "energy", "noise")}


@pytest.mark.parametrize("name", tdoa_golden.SETS)
def test_columns_equal_the_reference(name):
    g = tdoa_golden.load(name)
    rx_pos, beacon_pos = tdoa_golden.positions(g)
    res = tdoa_est.tdoa_columns(cols_of(g), g["match_ptr"], g["match_idx"], float(g["window"]), beacon_pos, rx_pos,
                                float(g["sample_rate"]), int(g["deg"]))
    rows = res["tdoas"]
    assert rows.dtype == np.dtype(tdoa_est.TDOA_DTYPE)
    tdoa_golden.check_against_fixture(
        g, res["group_id"], res["timestamp"], res["tx"], res["group_ptr"],
        {"rx0": rows["rx0"], "rx1": rows["rx1"], "tdoa": rows["tdoa"], "snr": rows["snr"],
         "model_quality": rows["model_quality"], "det0": rows["det0_idx"], "det1": rows["det1_idx"]},
        res["failures"], res["n_window"], res["n_kept"])


@pytest.mark.parametrize("name", tdoa_golden.SETS)
def test_estimate_tdoas_equals_the_reference(name):
    g = tdoa_golden.load(name)
    rx_pos, beacon_pos = tdoa_golden.positions(g)
    groups, failures = tdoa_est.estimate_tdoas(tdoa_golden.detections(g), tdoa_golden.matches(g), float(g["window"]),
                                               beacon_pos, rx_pos, float(g["sample_rate"]))
    assert all(isinstance(grp, tdoa_est.TdoaGroup) and isinstance(grp.group_id, int) for grp in groups)
    assert all(isinstance(pair, tuple) for pair in failures)
    table = tdoa_est.groups_to_matrix(groups)
    tdoa_golden.check_against_fixture(
        g, [grp.group_id for grp in groups], [grp.timestamp for grp in groups], [grp.tx for grp in groups],
        np.cumsum([0] + [len(grp.tdoas) for grp in groups]),
        {"rx0": table["rx0"], "rx1": table["rx1"], "tdoa": table["tdoa"], "snr": table["snr"],
         "model_quality": table["model_quality"], "det0": table["det0_idx"], "det1": table["det1_idx"]}, failures)


def test_command_line_writes_the_tdoa_file(tmp_path, capsys):
    g = tdoa_golden.load("tdoa_failures")
    rx_pos, beacon_pos = tdoa_golden.positions(g)
    toads, match, out = tmp_path / "data.toads", tmp_path / "data.match", tmp_path / "data.tdoa"
    rx_cfg, beacon_cfg = tmp_path / "pos-rx.cfg", tmp_path / "pos-beacon.cfg"
    # a .toads line keeps eight decimals of the SoA and six of the timestamp: the fixture's timestamps
    # have no more, its SoAs do, so the expectation is computed from what the file holds
    dets = tdoa_golden.detections(g)
    toads.write_text("".join(d.serialize() + "\n" for d in dets))
    with open(str(match), "w") as handle:
        matchmaker.save_matches(tdoa_golden.matches(g), handle)
    rx_cfg.write_text("".join("%d: %r %r\n" % (r, float(p[0]), float(p[1])) for r, p in rx_pos.items()))
    beacon_cfg.write_text("".join("%d: %r %r\n" % (b, float(p[0]), float(p[1])) for b, p in beacon_pos.items()))
    tdoa_est._main([str(toads), str(match), "-o", str(out), "-r", str(rx_cfg), "-b", str(beacon_cfg)])
    printed = capsys.readouterr().out.splitlines()
    back = tdoa_est.load_tdoa_groups(str(out))
    assert printed == ["Number of TDOA estimations: %d" % len(back),
                       "Number of TDOA estimation failures: %d" % len(g["failures"])]
    assert [grp.group_id for grp in back] == g["group_id"].tolist()
    table = tdoa_est.groups_to_matrix(back)
    for ours, theirs in (("rx0", "rx0"), ("rx1", "rx1"), ("det0_idx", "det0"), ("det1_idx", "det1")):
        np.testing.assert_array_equal(table[ours], g[theirs])
    assert np.all(np.abs(table["tdoa"] - g["tdoa"]) <= 2 * float(g["ref_err_max"]) + 1e-8 / 2.4e6)   # + the SoAs' 8 decimals
    assert not sys.stdout.closed


def test_times_are_reported():
    g = tdoa_golden.load("tdoa_realistic")
    rx_pos, beacon_pos = tdoa_golden.positions(g)
    tdoa_est.tdoa_columns(cols_of(g), g["match_ptr"], g["match_idx"], 8.0, beacon_pos, rx_pos, 2.4e6)
    times = _native.tdoa_times()
    assert len(times) == 3 and all(t > 0 for t in times)
