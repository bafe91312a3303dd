"""Host side of `thr_posq` (no GPU): the wiring into the header, the symbol list and the build; what is refused
before the library is loaded; the NumPy statement (tests/posq_ref.py) on the fixtures
(tests/golden/make_golden_posq.py); the .posq text format; the command line's options."""
import io
import os
import re

import numpy as np
import pytest

import pos_golden
import posq_golden
import posq_ref
from pos_ref import pos_ref_groups
from thrifty_amd import _native, build, pos_quality, tdoa_est

ROOT = posq_golden.ROOT


def test_thr_posq_is_declared_listed_and_built():
    header = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
    assert re.search(r"\bint thr_posq\(int device_id, size_t n_groups, const int64_t\* group_ptr,", header)
    assert re.search(r"\bint thr_posq_fetch\(thr_posq_result\* result, int which, void\* dst, size_t dst_bytes\);", header)
    assert "void thr_posq_free(thr_posq_result* result);" in header and "int thr_debug_posq_times(double* ms_out" in header
    assert "#define THR_ABI_VERSION 11" in header and _native.ABI_VERSION == 11
    assert re.search(r"\+ thr_posq / thr_posq_fetch / thr_posq_free / thr_debug_posq_times", header)
    for name, (index, _, _) in _native.POSQ_OUTPUTS.items():
        assert re.search(r"#define THR_POSQ_%s %d\b" % (name.upper(), index), header), name
    assert "#define THR_POSQ_N_OUTPUTS %d" % len(_native.POSQ_OUTPUTS) in header
    for name in ("INCONSISTENT", "EXCLUDED", "NO_CANDIDATE"):
        assert "#define THR_POSQ_%s %d" % (name, getattr(_native, "POSQ_" + name)) in header
        assert getattr(pos_quality, name) == getattr(_native, "POSQ_" + name)
    assert {"thr_posq", "thr_posq_fetch", "thr_posq_free", "thr_debug_posq_times"} <= set(_native.EXPORTS)
    assert [f[0] for f in _native.ThrPosqOpts._fields_] == ["max_iter", "min_rx", "x0", "gate_m", "ratio"]
    assert [f[0] for f in _native.ThrPosqCounts._fields_] == ["groups", "rows", "flagged", "tasks"]
    assert "posq.hip" in build.SOURCES and "pos_lm.hpp" in build.HEADERS
    assert build.UNPROFILED_POSQ == ("posq.hip", "pos_lm.hpp") and build.UNPROFILED_POS == ("pos.hip",)
    assert build.PER_FILE_FLAGS["posq.hip"] == ["-ffp-contract=off"]
    pos, posq, lm = (open(os.path.join(build.CSRC, name)).read() for name in ("pos.hip", "posq.hip", "pos_lm.hpp"))
    for source in (pos, posq):
        assert '#include "pos_lm.hpp"' in source and "#pragma clang fp contract(off)" in source
        assert "solve_team<" in source
    assert "#pragma clang fp contract(off)" in lm and lm.count("for (int it = 0; it < max_iter; ++it)") == 1
    assert "atomicAdd" not in posq and "hipMalloc(" not in posq
    assert int(re.search(r"constexpr int kRegRows = (\d+);", posq).group(1)) == _native.POS_REGISTER_ROWS


def test_the_built_library_exports_thr_posq():
    assert os.path.exists(_native.LIB_PATH), "the library is not built: python -m thrifty_amd.build"
    lib = _native.load_library()
    assert lib.thr_posq and lib.thr_posq_fetch and lib.thr_posq_free and lib.thr_debug_posq_times


def test_csrc_hash_does_not_see_the_two_new_files(monkeypatch):
    with_posq = build.csrc_hash()
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "posq.hip"])
    monkeypatch.setattr(build, "HEADERS", [h for h in build.HEADERS if h != "pos_lm.hpp"])
    assert build.csrc_hash() == with_posq
    monkeypatch.undo()
    monkeypatch.setattr(build, "UNPROFILED_POSQ", ())
    assert build.csrc_hash() != with_posq


def test_the_parents_digests_are_stored():
    digests = posq_golden.parent_digests()
    assert set(digests) == set(pos_golden.SETS_2D)
    for entry in digests.values():
        assert set(entry) == {"pos", "dop", "snr", "status", "iters"} and all(re.fullmatch(r"[0-9a-f]{64}", v) for v in entry.values())


def test_bad_inputs_are_refused_before_the_library_is_loaded(monkeypatch):
    def no_library():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_native, "load_library", no_library)
    flat = {k: np.array(xy) for k, xy in enumerate([(0.0, 0.0), (100.0, 0.0), (0.0, 100.0)])}
    args = ([0, 3], [0, 0, 1], [1, 2, 2], [1e-9, 2e-9, 3e-9], [1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="3-D"):
        pos_quality.quality_columns(*args, {k: np.append(v, 1.0) for k, v in flat.items()})
    with pytest.raises(ValueError, match="1-D"):
        pos_quality.quality_columns([0, 1], [0], [1], [1e-9], [1.0], {0: np.array([0.0]), 1: np.array([50.0])})
    with pytest.raises(KeyError):
        pos_quality.quality_columns(*args, {0: flat[0], 1: flat[1], 7: flat[2]})
    with pytest.raises(ValueError, match="group_ptr"):
        pos_quality.quality_columns([0, 2], *args[1:], flat)
    for weights in ([1.0, -1.0, 1.0], [1.0, np.nan, 1.0], [1.0, np.inf, 1.0]):
        with pytest.raises(ValueError, match="negative or not finite"):
            pos_quality.quality_columns(*args, flat, weights=weights)
    with pytest.raises(ValueError, match="one weight per row"):
        pos_quality.quality_columns(*args, flat, weights=[1.0, 1.0])
    with pytest.raises(ValueError, match="weights must be"):
        pos_quality.quality_columns(*args, flat, weights="energy")
    for ratio in (0.0, -0.5, 1.5, np.nan):
        with pytest.raises(ValueError, match="ratio"):
            pos_quality.quality_columns(*args, flat, ratio=ratio)
    for min_rx in (4, 65, 5.5):
        with pytest.raises(ValueError, match="min_rx"):
            pos_quality.quality_columns(*args, flat, min_rx=min_rx)
    for gate in (0.0, -3.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="exclude_gate_m"):
            pos_quality.quality_columns(*args, flat, exclude_gate_m=gate)
    rows = np.zeros(3, dtype=tdoa_est.TDOA_DTYPE)
    rows["rx0"], rows["rx1"] = args[1], args[2]
    with pytest.raises(ValueError, match="ratio"):
        pos_quality.solve([tdoa_est.TdoaGroup(1, 2.0, 3, rows)], flat, ratio=2.0)
    with pytest.raises(ValueError, match="3-D"):
        pos_quality.solve([tdoa_est.TdoaGroup(1, 2.0, 3, rows)], {k: np.append(v, 1.0) for k, v in flat.items()})


def _ref(g, weighted=True, **kw):
    weights = posq_golden.weights_of(g) if weighted else None
    return posq_ref.posq_ref(g["group_ptr"], posq_golden.dense(g, g["rx0"]), posq_golden.dense(g, g["rx1"]), g["tdoa"], g["snr"],
                             g["rx_xy"], weights, float(g["gate_m"]), float(g["ratio"]), int(g["min_rx"]), **kw)


def test_fixtures_are_small_and_hold_the_scene_of_the_issue():
    for name in posq_golden.SETS:
        assert os.path.getsize(os.path.join(posq_golden.GOLDEN, name + ".npz")) <= 64 * 1024
        g = posq_golden.load(name)
        assert 0 < len(g["group_id"]) <= 64 and 1e-14 < float(g["ref_err_max"]) < 1e-9
        assert len(g["full_x_star"]) == len(g["group_id"]) and len(g["task_x_star"]) == g["ref_task_ptr"][-1]
    g = posq_golden.load("posq_fault6")
    assert len(g["rx_ids"]) == 6 and set(np.diff(g["group_ptr"]).tolist()) == {15} and len(g["weights"]) == 0
    assert (float(g["gate_m"]), float(g["ratio"]), int(g["min_rx"])) == (3.0, 0.5, 5)
    affected = g["planted"] >= 0
    assert affected.sum() == 16 and np.all(affected == (np.arange(48) % 3 == 2)) and set(g["planted"][affected]) == set(g["rx_ids"])
    radius = np.hypot(*g["rx_xy"].T)
    assert np.all(np.abs(radius - 100.0) < 20.0)
    g = posq_golden.load("posq_weighted7")
    assert len(g["rx_ids"]) == 7 and np.any(g["weights"] == 0.0) and np.all(g["weights"] >= 0.0) and len(set(np.diff(g["group_ptr"]))) > 1


def test_the_statement_excludes_the_planted_receiver_and_no_other():
    g = posq_golden.load("posq_fault6")
    ref = _ref(g)
    affected = g["planted"] >= 0
    np.testing.assert_array_equal(ref["counts"][:, 2], np.where(affected, posq_golden.dense(g, np.maximum(g["planted"], g["rx_ids"][0])), -1))
    np.testing.assert_array_equal(ref["flags"], np.where(affected, 3, 0))
    np.testing.assert_array_equal(ref["flags"], g["ref_flags"])
    # the numbers of the issue: clean groups below 0.7 m, the best candidate at most 0.010 of the full rms, and the
    # repaired positions as good as the clean ones
    assert ref["rms"][~affected, 0].max() < 0.7 and ref["rms"][:, 1].max() < 0.9
    assert np.all(ref["rms"][affected, 1] <= 0.010 * ref["rms"][affected, 0])
    np.testing.assert_array_equal(ref["used"].reshape(48, 15).sum(axis=1), np.where(affected, 10, 15))


@pytest.mark.parametrize("name", posq_golden.SETS)
def test_the_statement_sits_on_the_exact_minimisers(name):
    g = posq_golden.load(name)
    ref = _ref(g)
    np.testing.assert_array_equal(ref["task_ptr"], g["ref_task_ptr"])
    assert np.max(np.abs(ref["pos"] - g["ref_pos"])) <= float(g["ref_err_max"])      # NumPy's sums may differ between builds
    for pos, status, star in ((ref["full_pos"], ref["full_status"], g["full_x_star"]), (ref["task_pos"], ref["task_status"], g["task_x_star"])):
        ok = np.all(np.isfinite(star), axis=1)
        assert np.all(status[ok] == 0) and ok.sum() >= len(ok) // 2
        assert np.max(np.abs(pos[ok] - star[ok])) <= float(g["ref_err_max"])


def test_the_statement_without_weights_is_pos_ref():
    g = pos_golden.load("pos_ring6")
    cols = (g["group_ptr"], pos_golden.dense(g, g["rx0"]), pos_golden.dense(g, g["rx1"]), g["tdoa"], g["snr"], g["rx_xyz"])
    want, got = pos_ref_groups(*cols), posq_ref.posq_ref(*cols)
    for key in ("pos", "dop", "snr", "status", "iters"):
        assert got[key].tobytes() == want[key].tobytes(), key
    ones = posq_ref.posq_ref(*cols, weights=np.ones(len(cols[1])))
    assert ones["pos"].tobytes() == got["pos"].tobytes() and ones["rms"].tobytes() == got["rms"].tobytes()
    assert np.all(np.isnan(got["q"][got["dop"] == -1])) and not got["flags"].any() and not got["task_ptr"].any()


def test_weights_are_normalised_per_task_in_team_order():
    w = np.array([3.0, 0.0, 1.0, 2.0, 5.0])
    use = np.array([True, True, False, True, True])
    got = posq_ref.task_weights(w, use)
    assert got[2] == 0.0 and np.isclose(got[use].sum(), 4.0) and got[0] == 3.0 * (4.0 / 10.0)
    assert np.all(posq_ref.task_weights(np.ones(5), use)[use] == 1.0) and posq_ref.task_weights(None, use) is None
    assert np.all(np.isnan(posq_ref.task_weights(np.zeros(5), use)[use]))
    none = posq_ref.solve_task([0, 0, 1], [1, 2, 2], [1e-9, 2e-9, 3e-9], [[0.0, 0.0], [100.0, 0.0], [0.0, 100.0]], weights=np.zeros(3))
    assert none["status"] == 4 and none["iters"] == 0


def test_the_ellipse_of_q():
    xdop, ydop, major, minor, angle = pos_quality.ellipse([[4.0, 0.0, 1.0], [1.0, 0.0, 4.0], [2.5, 1.5, 2.5], [np.nan] * 3])
    np.testing.assert_allclose(xdop[:3], [2.0, 1.0, np.sqrt(2.5)])
    np.testing.assert_allclose(ydop[:3], [1.0, 2.0, np.sqrt(2.5)])
    np.testing.assert_allclose(major[:3], [2.0, 2.0, 2.0])
    np.testing.assert_allclose(minor[:3], [1.0, 1.0, 1.0])
    np.testing.assert_allclose(angle[:3], [0.0, 90.0, 45.0])
    assert all(np.isnan(v[3]) for v in (xdop, ydop, major, minor, angle))
    for q in ([4.0, 0.0, 1.0], [2.5, 1.5, 2.5], [1.0, -0.3, 0.7]):
        np.testing.assert_allclose([v[0] for v in pos_quality.ellipse([q])], posq_ref.ellipse(q), rtol=1e-14, atol=1e-14)


def _records():
    res = np.zeros(3, dtype=pos_quality.QUALITY_DTYPE)
    res["group_id"], res["timestamp"], res["tx"] = [7, 8, 11], [1700000012.25, 1.5, 2.75], 3
    for k, name in enumerate(pos_quality.QUALITY_DTYPE["names"][3:13]):
        res[name] = [0.1 * (k + 1), 1e-5 / (k + 1), -12.5 * (k + 1)]
    res["n_rx"], res["n_rows"], res["excluded"], res["flags"] = [6, 5, 6], [15, 10, 15], [-1, 21, -1], [0, 3, 5]
    return res


def test_posq_file_round_trip(tmp_path):
    res = _records()
    text = io.StringIO()
    pos_quality.save_quality(text, res)
    lines = text.getvalue().splitlines()
    assert len(lines) == 3 and len(lines[1].split()) == 17
    assert lines[1].split()[:3] == ["8", "1.500000", "3"] and lines[1].split()[-4:] == ["5", "10", "21", "3"]
    assert lines[0].split()[3] == repr(0.1)
    path = tmp_path / "data.posq"
    pos_quality.save_quality(str(path), res)
    assert path.read_text() == text.getvalue()
    back = pos_quality.load_quality(str(path))
    assert back.dtype == res.dtype and back.tolist() == res.tolist()
    assert len(pos_quality.load_quality(io.StringIO("# nothing\n\n"))) == 0
    with pytest.raises(ValueError, match="17"):
        pos_quality.load_quality(io.StringIO("7 1.0 3 0.5 20.0 17.25 1.0\n"))


def test_the_summary_counts_exclusions_per_receiver():
    res = np.concatenate([_records(), _records()])
    res["excluded"][4], res["flags"][5] = 34, 3
    res["excluded"][5] = 21
    assert pos_quality.format_summary(res) == ("6 positions, 4 inconsistent, 3 with a receiver excluded\n"
                                               "  RX 21: excluded 2 times\n  RX 34: excluded 1 times\n")
    assert pos_quality.format_summary(res[:1]) == "1 positions, 0 inconsistent, 0 with a receiver excluded\n"


def test_command_line_options():
    parser = pos_quality._parser()
    assert parser.get_default("tdoa") == "data.tdoa" and parser.get_default("output") == "data.posq"
    assert parser.get_default("rx_pos") == "pos-rx.cfg" and parser.get_default("gate_m") is None
    assert (parser.get_default("ratio"), parser.get_default("min_rx"), parser.get_default("weights")) == (0.5, 5, None)
    assert {s for a in parser._actions for s in a.option_strings} >= {
        "-o", "--output", "-r", "--rx-coordinates", "--weights", "--exclude", "--ratio", "--min-rx", "--pos"}
    with pytest.raises(SystemExit):
        parser.parse_args(["--weights", "energy"])
    assert pos_quality.QUALITY_DTYPE["names"] == ("group_id", "timestamp", "tx", "dop", "snr", "x", "y", "rms", "xdop", "ydop",
                                                   "major", "minor", "angle", "n_rx", "n_rows", "excluded", "flags")


def test_the_command_line_refuses_a_bad_ratio_before_the_library_is_loaded(tmp_path, monkeypatch, capsys):
    def no_library():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_native, "load_library", no_library)
    g = posq_golden.load("posq_fault6")
    rows = np.zeros(15, dtype=tdoa_est.TDOA_DTYPE)
    for name in ("rx0", "rx1", "tdoa", "snr"):
        rows[name] = g[name][:15]
    tdoa, cfg, out = tmp_path / "data.tdoa", tmp_path / "pos-rx.cfg", tmp_path / "data.posq"
    tdoa_est.save_tdoa_groups(str(tdoa), [tdoa_est.TdoaGroup(100, 1.0, 7, rows)])
    cfg.write_text("".join("%d: %r %r\n" % (r, float(x), float(y)) for r, (x, y) in zip(g["rx_ids"], g["rx_xy"])))
    assert pos_quality._main([str(tdoa), "-r", str(cfg), "-o", str(out), "--ratio", "1.5"]) == 1
    assert "ratio" in capsys.readouterr().err and out.read_text() == ""
