"""Host side of `tdoa` (no GPU): the sequential statement tests/tdoa_ref.py against the fixtures the
reference's own `estimate_tdoas` produced (tests/golden/make_golden_tdoa.py), the .tdoa text format,
the command line's defaults, `load_pos_config`, the three deviations from the reference, and the wiring
of `thr_tdoa` into the header, the symbol list and the build."""
import io
import os
import re

import numpy as np
import pytest

import tdoa_golden
from tdoa_ref import bisect_left, bisect_right, outlier_mask, tdoa_ref
from thrifty_amd import _native, build, tdoa_est

ROOT = tdoa_golden.ROOT
_ref = {}


def ref_of(name):
    """tdoa_ref's answer for a fixture, computed once."""
    if name not in _ref:
        g = tdoa_golden.load(name)
        rx_pos, beacon_pos = tdoa_golden.positions(g)
        _ref[name] = tdoa_ref(g["rxid"], g["txid"], g["timestamp"], g["soa"], g["energy"], g["noise"],
                              tdoa_golden.matches(g), float(g["window"]), beacon_pos, rx_pos,
                              float(g["sample_rate"]), int(g["deg"]))
    return _ref[name]


def test_fixtures_are_what_the_issue_asks_for():
    for name in tdoa_golden.SETS:
        assert os.path.getsize(os.path.join(tdoa_golden.GOLDEN, name + ".npz")) < 100 * 1024
        g = tdoa_golden.load(name)
        assert 0 < float(g["ref_err_max"]) < 1e-9 and len(g["exact_tdoa"]) == len(g["tdoa"]) > 0
        assert len(g["n_window"]) == len(g["n_kept"]) == len(g["tdoa"]) + len(g["failures"])
    real = tdoa_golden.load("tdoa_realistic")
    assert len(real["tdoa"]) >= 200 and real["n_window"].min() >= 10 and len(real["rx_ids"]) == 3
    fail = tdoa_golden.load("tdoa_failures")
    assert {0, 1, 2, 3} <= set(fail["n_window"].tolist()) and len(fail["uncovered_matches"]) > 0
    assert np.any((fail["n_window"] >= 3) & (fail["n_kept"] < 3))
    wide = tdoa_golden.load("tdoa_wide")
    assert {63, 64, 65} <= set(wide["n_window"].tolist()) and 125 <= wide["n_window"].max() <= 140
    ties = tdoa_golden.load("tdoa_ties")
    assert np.all(ties["soa"] == np.round(ties["soa"])) and np.all(2 * ties["timestamp"] == np.round(2 * ties["timestamp"]))
    assert {0, 1} <= set((ties["n_window"][ties["n_window"] > 1] % 2).tolist())
    # recomputed from the columns: the receiver pairs' lists in match order, every task's window and its MAD
    rx, tx, ts, soa, window = ties["rxid"], ties["txid"], ties["timestamp"], ties["soa"], float(ties["window"])
    ordered = lambda match: [(a, b) if rx[a] < rx[b] else (b, a) for i, a in enumerate(match) for b in match[i + 1:]]  # noqa: E731
    lists, mad_zero, on_left, on_right = {}, [], 0, 0
    for match in tdoa_golden.matches(ties):
        if tx[match[0]] in ties["beacon_ids"]:
            for d0, d1 in ordered(match):
                lists.setdefault((rx[d0], rx[d1]), []).append((d0, d1))
    for match in tdoa_golden.matches(ties):
        if tx[match[0]] not in ties["beacon_ids"]:
            for d0, d1 in ordered(match):
                pairs = lists[(rx[d0], rx[d1])]
                stamps = [ts[p[0]] for p in pairs]
                inside = pairs[bisect_left(stamps, ts[d0] - window):bisect_right(stamps, ts[d0] + window)]
                on_left += any(ts[p[0]] == ts[d0] - window for p in inside)
                on_right += any(ts[p[0]] == ts[d0] + window for p in inside)
                sdoa = np.array([soa[p[0]] - soa[p[1]] for p in inside])
                diff = np.abs(sdoa - np.median(sdoa))
                mad_zero.append(0 if len(inside) < 2 or np.median(diff) != 0 else 2 if np.any(diff != 0) else 1)
    assert mad_zero == ties["mad_zero"].tolist()
    # mad == 0 where every difference is the median (0 / 0: all kept), mad == 0 where some are not (x / 0:
    # dropped), and ordinary windows; timestamps exactly on t0 - window and on t0 + window
    zero, kept_all = ties["mad_zero"], ties["n_kept"] == ties["n_window"]
    assert np.any((zero == 1) & kept_all) and not np.any((zero == 1) & ~kept_all)
    assert np.any((zero == 2) & ~kept_all & (ties["n_kept"] >= 3)) and not np.any((zero == 2) & kept_all)
    assert np.any((zero == 0) & (ties["n_window"] > 1))
    assert on_left > 0 and on_right > 0
    # at least one receiver pair's list of det0 timestamps is not monotone
    assert any(np.any(np.diff([ts[p[0]] for p in pairs]) < 0) for pairs in lists.values())


@pytest.mark.parametrize("name", tdoa_golden.SETS)
def test_tdoa_ref_equals_the_reference(name):
    g, out = tdoa_golden.load(name), ref_of(name)
    rows = [row for group in out["groups"] for row in group[3]]
    cols = {key: np.array([row[k] for row in rows]) for k, key in
            enumerate(("rx0", "rx1", "tdoa", "snr", "model_quality", "det0", "det1"))}
    tdoa_golden.check_against_fixture(
        g, [grp[0] for grp in out["groups"]], [grp[1] for grp in out["groups"]], [grp[2] for grp in out["groups"]],
        np.cumsum([0] + [len(grp[3]) for grp in out["groups"]]), cols, out["failures"], out["n_window"], out["n_kept"])


def test_bisection_on_an_unsorted_list_is_pythons():
    import bisect
    rng = np.random.default_rng(3)
    for _ in range(200):
        a = rng.integers(0, 6, int(rng.integers(0, 12))).astype(float).tolist()
        x = float(rng.integers(-1, 7))
        assert bisect_left(a, x) == bisect.bisect_left(a, x) and bisect_right(a, x) == bisect.bisect_right(a, x)


def test_mask_follows_ieee_when_mad_is_zero():
    assert outlier_mask(np.array([5.0, 5.0, 5.0, 7.0])).tolist() == [False, False, False, True]     # 0/0 stays, x/0 goes
    assert outlier_mask(np.array([1.0, 1.0])).tolist() == [False, False]
    assert outlier_mask(np.array([0.0, 1.0, 2.0, 3.0, 100.0])).tolist() == [False, False, False, False, True]


def small_case(n_beacon=6, uncovered=False, repeat_x=False, twice=False):
    """Receivers 0, 1 (and 2): n_beacon beacon matches a second apart, then one mobile match."""
    rx, tx, ts, soa = [], [], [], []
    for k in range(n_beacon):
        for r in (0, 1):
            rx.append(r), tx.append(0), ts.append(100.0 + k)
            soa.append((7e9 if r else 3e9) + 2.4e6 * (0 if repeat_x and k > 1 else k) + (0.25 * k * k if r == 0 else 0))
    matches = [[2 * k, 2 * k + 1] for k in range(n_beacon)]
    mobile_rx = (0, 2) if uncovered else (0, 0) if twice else (0, 1)
    for r in mobile_rx:
        rx.append(r), tx.append(5), ts.append(100.0 + n_beacon / 2)
        soa.append((7e9 if r else 3e9) + 2.4e6 * n_beacon / 2 + 3.0)
    matches.append([len(rx) - 2, len(rx) - 1])
    n = len(rx)
    rx_pos = {0: np.array([0.0, 0.0]), 1: np.array([900.0, 0.0]), 2: np.array([0.0, 700.0])}
    return (rx, tx, ts, soa, [100.0] * n, [2.0] * n, matches, 8.0, {0: np.array([300.0, 400.0])}, rx_pos, 2.4e6)


def test_deviations_in_the_sequential_statement():
    out = tdoa_ref(*small_case())
    assert len(out["groups"]) == 1 and out["failures"] == [] and out["n_window"] == [6] and out["n_kept"] == [6]
    out = tdoa_ref(*small_case(uncovered=True))          # no beacon list for (0, 2): an empty window
    assert out["groups"] == [] and out["failures"] == [(12, 13)] and out["n_window"] == [0]
    out = tdoa_ref(*small_case(repeat_x=True))           # six kept pairs, two distinct abscissae: no parabola
    assert out["groups"] == [] and out["failures"] == [(12, 13)] and out["n_kept"] == [6]
    with pytest.raises(ValueError, match="two detections of receiver 0"):
        tdoa_ref(*small_case(twice=True))
    args = list(small_case())
    args[9] = {0: args[9][0]}
    with pytest.raises(KeyError):
        tdoa_ref(*args)


def test_two_detections_of_one_receiver_and_unknown_receivers_are_refused_on_the_host():
    """estimate_tdoas raises before anything is launched: no device is needed to get here."""
    rx, tx, ts, soa, en, no, matches, window, beacon_pos, rx_pos, fs = small_case(twice=True)
    cols = {"rxid": np.array(rx), "txid": np.array(tx), "timestamp": np.array(ts), "soa": np.array(soa),
            "energy": np.array(en), "noise": np.array(no)}
    ptr, idx = np.cumsum([0] + [len(m) for m in matches]), np.concatenate(matches)
    with pytest.raises(ValueError, match="two detections of one receiver"):
        tdoa_est.tdoa_columns(cols, ptr, idx, window, beacon_pos, rx_pos, fs)
    with pytest.raises(KeyError):
        tdoa_est.tdoa_columns(cols, ptr, idx, window, beacon_pos, {0: rx_pos[0]}, fs)
    with pytest.raises(ValueError, match="deg must be"):
        cols["rxid"] = np.array(small_case()[0])
        tdoa_est.tdoa_columns(cols, ptr, idx, window, beacon_pos, rx_pos, fs, deg=4)
    with pytest.raises(ValueError, match="at least one detection"):
        tdoa_est.tdoa_columns(cols, [0, 2, 2], idx[:2], window, beacon_pos, rx_pos, fs)


def fixture_groups(g):
    rows = np.zeros(len(g["tdoa"]), dtype=tdoa_est.TDOA_DTYPE)
    for ours, theirs in (("rx0", "rx0"), ("rx1", "rx1"), ("tdoa", "tdoa"), ("snr", "snr"),
                         ("model_quality", "model_quality"), ("det0_idx", "det0"), ("det1_idx", "det1")):
        rows[ours] = g[theirs]
    ptr = g["group_ptr"].tolist()
    return [tdoa_est.TdoaGroup(int(i), float(t), int(tx), rows[a:b]) for i, t, tx, a, b in
            zip(g["group_id"], g["group_timestamp"], g["group_tx"], ptr[:-1], ptr[1:])]


@pytest.mark.parametrize("name", ["tdoa_realistic", "tdoa_failures"])
def test_tdoa_file_round_trip(name, tmp_path):
    g = tdoa_golden.load(name)
    groups = fixture_groups(g)
    text = io.StringIO()
    tdoa_est.save_tdoa_groups(text, groups)
    lines = text.getvalue().splitlines()
    first, row = groups[0], groups[0].tdoas[0]
    assert lines[0] == "%d %.06f %d %d %d %r %r %r %d %d" % (
        first.group_id, first.timestamp, first.tx, row["rx0"], row["rx1"], float(row["tdoa"] * 1e9), float(row["snr"]),
        float(row["model_quality"]), row["det0_idx"], row["det1_idx"])
    assert len(lines) == len(g["tdoa"])
    path = tmp_path / "data.tdoa"
    tdoa_est.save_tdoa_groups(str(path), groups)
    assert path.read_text() == text.getvalue()
    back = tdoa_est.load_tdoa_groups(str(path))
    assert len(back) == len(groups)
    for ours, theirs in zip(back, groups):
        # timestamps are written with six decimals (the fixtures' have no more); tdoa goes through
        # nanoseconds as in the reference: t * 1e9 is written exactly, the loader divides by 1e9
        assert (ours.group_id, ours.timestamp, ours.tx) == (theirs.group_id, theirs.timestamp, theirs.tx)
        for key in ("rx0", "rx1", "snr", "model_quality", "det0_idx", "det1_idx"):
            np.testing.assert_array_equal(ours.tdoas[key], theirs.tdoas[key])
        np.testing.assert_array_equal(ours.tdoas["tdoa"], theirs.tdoas["tdoa"] * 1e9 / 1e9)
        assert ours.tdoas.dtype == np.dtype(tdoa_est.TDOA_DTYPE)
    matrix = tdoa_est.load_tdoa_matrix(io.StringIO(text.getvalue()))
    np.testing.assert_array_equal(matrix["group_id"], tdoa_est.groups_to_matrix(groups)["group_id"])
    assert matrix.dtype == np.dtype(tdoa_est.MATRIX_DTYPE) and len(matrix) == len(g["tdoa"])


def test_loader_reads_the_twelve_digit_form_too():
    text = "7 1700000012.250000 3 0 1 -123.456789012 5432.10987654 4321.0 41 40\n# a comment\n\n"
    (group,) = tdoa_est.load_tdoa_groups(io.StringIO(text))
    assert (group.group_id, group.timestamp, group.tx) == (7, 1700000012.25, 3)
    assert group.tdoas.tolist() == [(0, 1, -123.456789012 / 1e9, 5432.10987654, 4321.0, 41, 40)]
    assert len(tdoa_est.load_tdoa_matrix(io.StringIO(""))) == 0 and tdoa_est.load_tdoa_groups(io.StringIO("")) == []


def test_cli_defaults_are_the_references():
    parser = tdoa_est._parser()
    assert parser.get_default("toads") == "data.toads" and parser.get_default("matches") == "data.match"
    assert parser.get_default("output") == "data.tdoa"
    assert parser.get_default("rx_pos") == "pos-rx.cfg" and parser.get_default("beacon_pos") == "pos-beacon.cfg"
    assert parser.get_default("window_size") == 8 and parser.get_default("sample_rate") == 2.4e6
    flags = {s for a in parser._actions for s in a.option_strings}
    assert {"-o", "--output", "-r", "--rx-coordinates", "-b", "--beacon-coordinates", "-w", "--window-size",
            "-s", "--sample-rate"} <= flags
    assert tdoa_est.SPEED_OF_LIGHT == 2.997e8 and tdoa_est.MAX_TDOA == 30e3 / 2.997e8


def test_load_pos_config(tmp_path):
    text = "# receivers\n0: 10.5 -3\n12: 1e3 2 3.5   # with a height\n\n"
    pos = tdoa_est.load_pos_config(io.StringIO(text))
    assert sorted(pos) == [0, 12] and pos[0].tolist() == [10.5, -3.0] and pos[12].tolist() == [1000.0, 2.0, 3.5]
    path = tmp_path / "pos-rx.cfg"
    path.write_text(text)
    assert {k: v.tolist() for k, v in tdoa_est.load_pos_config(str(path)).items()} == {k: v.tolist() for k, v in pos.items()}


def test_thr_tdoa_is_declared_listed_and_built():
    header = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
    assert re.search(r"\bint thr_tdoa\(int device_id, size_t n_det,", header)
    assert re.search(r"\bint thr_debug_tdoa_times\(double\* ms_out", header)
    assert "#define THR_ABI_VERSION 11" in header and _native.ABI_VERSION == 11
    assert re.search(r"\+ thr_tdoa / thr_debug_tdoa_times", header)
    assert {"thr_tdoa", "thr_debug_tdoa_times"} <= set(_native.EXPORTS) and callable(_native.tdoa)
    assert "tdoa.hip" in build.SOURCES and set(build.UNPROFILED_TDOA) == {"tdoa.hip"}
    assert "-ffp-contract=off" in build.PER_FILE_FLAGS["tdoa.hip"]
    source = open(os.path.join(build.CSRC, "tdoa.hip")).read()
    assert "#pragma clang fp contract(off)" in source
    assert (int(re.search(r"constexpr int kBlock = (\d+);", source).group(1)) // 64 == _native.TDOA_TASKS_PER_WORKGROUP)
    assert int(re.search(r"constexpr int kLdsWindow = (\d+);", source).group(1)) == _native.TDOA_LDS_WINDOW
    if os.path.exists(_native.LIB_PATH):
        lib = _native.load_library()
        assert lib.thr_tdoa and lib.thr_debug_tdoa_times
