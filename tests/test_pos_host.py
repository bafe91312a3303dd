"""Host side of `pos` (no GPU): the NumPy restatement tests/pos_ref.py against the fixtures the
reference's own `solve` produced (tests/golden/make_golden_pos.py) under the rules the device is held
to, the .pos text format, the command line's defaults, `dop` / `dop_matrix`, the inputs refused before
the library is loaded, and the wiring of `thr_pos` into the header, the symbol list and the build."""
import io
import os
import re

import numpy as np
import pytest

import pos_golden
from pos_ref import pos_ref_groups, team_sum
from thrifty_amd import _native, build, pos_est, tdoa_est

ROOT = pos_golden.ROOT


def test_fixtures_are_what_the_issue_asks_for():
    for name in pos_golden.SETS:
        assert os.path.getsize(os.path.join(pos_golden.GOLDEN, name + ".npz")) <= 64 * 1024
        g = pos_golden.load(name)
        assert 0 < len(g["group_id"]) <= 64 and len(g["x_star"]) == len(g["x_ref"]) == len(g["solved"])
    for name, n_rx in (("pos_ring4", 4), ("pos_ring6", 6), ("pos_ring8", 8), ("pos_three", 3), ("pos_outside", 5)):
        g = pos_golden.load(name)
        assert len(g["rx_ids"]) == n_rx and float(g["ref_err_max"]) >= 1e-9
        assert (len(g["omitted"]) > 0) <= (name == "pos_outside") and len(g["omitted"]) <= 3
        inner = np.flatnonzero(~g["solved"])
        if name.startswith("pos_ring"):      # failures sit between solved groups
            assert len(inner) >= 2 and inner.min() > 0 and inner.max() < len(g["solved"]) - 1
        else:
            assert len(inner) == 0
    assert set(np.diff(pos_golden.load("pos_three")["group_ptr"]).tolist()) == {2, 3}
    for name in pos_golden.SETS_1D:
        g = pos_golden.load(name)
        assert g["rx_xyz"].shape == (2, 1) and np.any(g["dop_ref"] == -1) and np.any(g["dop_ref"] == 0.5)
        assert np.any(g["tdoa"] > 0) and np.any(g["tdoa"] < 0)
    falling, rising = (pos_golden.load(name)["rx_xyz"][:, 0] for name in pos_golden.SETS_1D)
    assert falling[0] > falling[1] and rising[0] < rising[1]


@pytest.mark.parametrize("name", pos_golden.SETS)
def test_pos_ref_meets_the_devices_rules(name):
    g = pos_golden.load(name)
    out = pos_ref_groups(g["group_ptr"], pos_golden.dense(g, g["rx0"]), pos_golden.dense(g, g["rx1"]), g["tdoa"],
                         g["snr"], g["rx_xyz"])
    keep = ~np.isin(out["status"], (_native.POS_UNDERDETERMINED, _native.POS_NONFINITE))
    np.testing.assert_array_equal(keep, g["solved"])
    assert set(out["status"][keep].tolist()) == {_native.POS_OK} and out["iters"].max() < 50
    pos_golden.check_positions(g, g["group_id"][keep], g["group_timestamp"][keep], g["group_tx"][keep],
                               out["pos"][keep], out["dop"][keep], out["snr"][keep])


def test_team_sum_is_the_eight_lane_tree():
    v = [1.0, 0.0, 2.0 ** -53, 2.0 ** -53]
    assert sum(v) == 1.0 and team_sum(v) == 1.0 + 2.0 ** -52          # (1 + 0) + (u + u), not ((1 + 0) + u) + u
    assert team_sum([0.0, 1.0] + [0.0] * 6 + [2.0 ** -53, 2.0 ** -53]) == 1.0 and team_sum([]) == 0.0     # rows 8, 9: lanes 0, 1


def records(g):
    ok = g["solved"]
    dims = g["rx_xyz"].shape[1]
    res = np.zeros(int(ok.sum()), dtype={"names": pos_est.POSITION_INFO_DTYPE["names"][:5 + dims],
                                         "formats": pos_est.POSITION_INFO_DTYPE["formats"][:5 + dims]})
    res["group_id"], res["timestamp"], res["tx"] = g["group_id"][ok], g["group_timestamp"][ok], g["group_tx"][ok]
    res["dop"], res["snr"] = g["dop_ref"][ok], g["snr_ref"][ok]
    for axis, key in enumerate(("x", "y")[:dims]):
        res[key] = g["x_ref"][ok][:, axis]
    return res


@pytest.mark.parametrize("name", ["pos_ring4", "pos_line"])
def test_pos_file_round_trip(name, tmp_path):
    res = records(pos_golden.load(name))
    text = io.StringIO()
    pos_est.save_positions(text, res)
    lines = text.getvalue().splitlines()
    first = res[0]
    assert lines[0] == " ".join(["%d %.6f %d" % (first["group_id"], first["timestamp"], first["tx"])] +
                                [repr(float(first[key])) for key in res.dtype.names[3:]])
    assert len(lines) == len(res)
    path = tmp_path / "data.pos"
    pos_est.save_positions(str(path), res)
    assert path.read_text() == text.getvalue()
    back = pos_est.load_positions(str(path))
    assert back.dtype == res.dtype and back.tolist() == res.tolist()     # six decimals hold the fixtures' timestamps


def test_loader_reads_the_twelve_digit_form_too():
    text = "7 1700000012.250000 3 1.23456789012 5432.10987654 -12.5 1e-05\n# a comment\n\n8 1.5 3 -1 2.0 3.0 4.0\n"
    got = pos_est.load_positions(io.StringIO(text))
    assert got.dtype.names == ("group_id", "timestamp", "tx", "dop", "snr", "x", "y")
    assert got.tolist() == [(7, 1700000012.25, 3, 1.23456789012, 5432.10987654, -12.5, 1e-05), (8, 1.5, 3, -1.0, 2.0, 3.0, 4.0)]
    one = pos_est.load_positions(io.StringIO("7 1.0 3 0.5 20.0 17.25\n"))
    assert one.dtype.names[-1] == "x" and one.tolist() == [(7, 1.0, 3, 0.5, 20.0, 17.25)]
    assert len(pos_est.load_positions(io.StringIO(""))) == 0


def test_cli_defaults_and_names_are_the_references():
    parser = pos_est._parser()
    assert parser.get_default("tdoa") == "data.tdoa" and parser.get_default("output") == "data.pos"
    assert parser.get_default("rx_pos") == "pos-rx.cfg"
    assert {s for a in parser._actions for s in a.option_strings} >= {"-o", "--output", "-r", "--rx-coordinates"}
    assert len([a for a in parser._actions if a.dest != "help"]) == 3
    assert pos_est.MAX_DIST == 10e3 and pos_est.SPEED_OF_LIGHT == 2.997e8 and issubclass(pos_est.EstimationError, Exception)
    assert pos_est.POSITION_INFO_DTYPE == {"names": ("group_id", "timestamp", "tx", "dop", "snr", "x", "y", "z"),
                                           "formats": ("i4", "f8", "i4", "f8", "f8", "f8", "f8", "f8")}
    assert all(callable(getattr(pos_est, f)) for f in ("solve_1d", "solve_numerically", "solve", "save_positions",
                                                        "load_positions", "pos_columns", "dop", "dop_matrix", "_main"))


@pytest.mark.parametrize("name", ["pos_ring6", "pos_outside", "pos_line"])
def test_dop_against_the_stored_values(name):
    g = pos_golden.load(name)
    rx_pos, ptr = pos_golden.rx_pos(g), g["group_ptr"].tolist()
    for k in np.flatnonzero(g["solved"])[:12].tolist():
        pairs = list(zip(g["rx0"][ptr[k]:ptr[k + 1]].tolist(), g["rx1"][ptr[k]:ptr[k + 1]].tolist()))
        got = pos_est.dop(g["x_ref"][k], rx_pos, pairs)
        if g["dop_ref"][k] == -1:
            assert got == -1 and pos_est.dop_matrix(g["x_ref"][k], rx_pos, pairs) is None
        else:
            assert abs(got - g["dop_ref"][k]) <= 1e-12 * g["dop_ref"][k]
            matrix = pos_est.dop_matrix(g["x_ref"][k], rx_pos, iter(pairs))
            assert matrix.shape == (g["rx_xyz"].shape[1],) * 2 and np.sqrt(np.trace(matrix)) == got


def test_bad_inputs_are_refused_before_the_library_is_loaded(monkeypatch):
    def no_library():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_native, "load_library", no_library)
    flat = {0: np.array([0.0, 0.0]), 1: np.array([100.0, 0.0]), 2: np.array([0.0, 100.0])}
    args = ([0, 3], [0, 0, 1], [1, 2, 2], [1e-9, 2e-9, 3e-9], [1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="3-D"):
        pos_est.pos_columns(*args, {k: np.append(v, 1.0) for k, v in flat.items()})
    with pytest.raises(KeyError):
        pos_est.pos_columns(*args, {0: flat[0], 1: flat[1], 7: flat[2]})
    line = {4: np.array([0.0]), 9: np.array([50.0])}
    with pytest.raises(ValueError, match="exactly one TDOA"):
        pos_est.pos_columns([0, 2], [4, 4], [9, 9], [1e-9, 2e-9], [1.0, 1.0], line)
    with pytest.raises(ValueError, match="exactly two receivers"):
        pos_est.pos_columns([0, 1], [4], [9], [1e-9], [1.0], {4: line[4], 9: line[9], 11: np.array([70.0])})
    with pytest.raises(ValueError, match="differ in length"):
        pos_est.pos_columns(*args, {0: flat[0], 1: flat[1], 2: np.array([1.0])})
    with pytest.raises(ValueError, match="group_ptr"):
        pos_est.pos_columns([0, 2], *args[1:], flat)
    rows = np.zeros(3, dtype=tdoa_est.TDOA_DTYPE)
    rows["rx0"], rows["rx1"] = args[1], args[2]
    with pytest.raises(ValueError, match="3-D"):
        pos_est.solve([tdoa_est.TdoaGroup(1, 2.0, 3, rows)], {k: np.append(v, 1.0) for k, v in flat.items()})
    with pytest.raises(KeyError):
        pos_est.solve([tdoa_est.TdoaGroup(1, 2.0, 3, rows)], {0: flat[0], 1: flat[1]})
    with pytest.raises(ValueError, match="one coordinate"):
        pos_est.solve_1d(rows[:1], flat)
    with pytest.raises(ValueError, match="2-D"):
        pos_est.solve_numerically(rows, line)


def test_thr_pos_is_declared_listed_and_built():
    header = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
    assert re.search(r"\bint thr_pos\(int device_id, size_t n_groups, const int64_t\* group_ptr,", header)
    assert re.search(r"\bint thr_debug_pos_times\(double\* ms_out", header)
    assert "#define THR_ABI_VERSION 11" in header and _native.ABI_VERSION == 11
    assert re.search(r"\+ thr_pos / thr_debug_pos_times", header)
    for k, status in enumerate(pos_est.STATUS_NAMES):
        assert "#define THR_POS_%s %d" % (status, k) in header and getattr(_native, "POS_" + status) == k
    assert {"thr_pos", "thr_debug_pos_times"} <= set(_native.EXPORTS) and callable(_native.pos)
    assert "pos.hip" in build.SOURCES and set(build.UNPROFILED_POS) == {"pos.hip"}
    assert "-ffp-contract=off" in build.PER_FILE_FLAGS["pos.hip"]
    source = open(os.path.join(build.CSRC, "pos.hip")).read()
    assert "#pragma clang fp contract(off)" in source and '#include "lmdif8.hpp"' in source
    assert int(re.search(r"constexpr int kBlock = (\d+);", source).group(1)) // 8 == _native.POS_GROUPS_PER_WORKGROUP
    assert int(re.search(r"constexpr int kRegRows = (\d+);", source).group(1)) == _native.POS_REGISTER_ROWS
    assert int(re.search(r"constexpr int kMaxReceivers = (\d+);", source).group(1)) == _native.POS_MAX_RECEIVERS


def test_the_built_library_exports_thr_pos():
    assert os.path.exists(_native.LIB_PATH), "the library is not built: python -m thrifty_amd.build"
    lib = _native.load_library()
    assert lib.thr_pos and lib.thr_debug_pos_times


def test_csrc_hash_does_not_see_pos_hip(monkeypatch):
    with_pos = build.csrc_hash()
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "pos.hip"])
    assert build.csrc_hash() == with_pos
    monkeypatch.undo()
    monkeypatch.setattr(build, "UNPROFILED_POS", ())
    assert build.csrc_hash() != with_pos
