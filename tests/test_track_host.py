"""Host side of `thr_track` (no GPU): the wiring into the header, the symbol list and the build; the three CPU
statements of tests/track_ref.py against the recorded tolerances (tests/golden/make_golden_track.py); the gate's
rounds; what is refused before the library is loaded; the .track text format; the command line on a mocked device."""
import hashlib
import importlib.util
import io
import json
import os
import re

import numpy as np
import pytest

import track_check
import track_ref
import track_scenes
from thrifty_amd import _native, build, pos_est, pos_quality, track

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLERANCES = json.load(open(os.path.join(ROOT, "tests", "golden", "track_tolerances.json")))
OUTPUTS = ("filt", "filt_var", "smooth", "smooth_var", "nis")
OLD_SCENES = {"gating_0", "gating_1", "gating_2", "gating_1_no_gate", "gating_0_one_round"} | set(track_scenes.seams())
CLAUSES = sorted(track_scenes.clauses())


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_track", os.path.join(ROOT, "tests", "golden", "make_golden_track.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def _ref(s, **kw):
    kw.setdefault("q", s["q"])
    kw.setdefault("v0", s["v0"])
    return track_ref.run(*track_scenes.columns(s), **kw)


def test_thr_track_is_declared_listed_and_built():
    header = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
    assert re.search(r"\bint thr_track\(int device_id, size_t n, const int32_t\* tx, const double\* timestamp,", header)
    assert re.search(r"\bint thr_track_fetch\(thr_track_result\* result, int which, void\* dst, size_t dst_bytes\);", header)
    assert "void thr_track_free(thr_track_result* result);" in header and "int thr_debug_track_times(double* ms_out" in header
    assert "int thr_debug_track_geometry(int* tile_len, int* workgroup, int* element_doubles);" in header
    assert "#define THR_ABI_VERSION 11" in header and _native.ABI_VERSION == 11
    within = header[header.index("within 11, a pure addition"):header.index("#define THR_ABI_VERSION")]
    assert re.search(r"\+ thr_track / thr_track_fetch / thr_track_free / thr_debug_track_times", within)
    for name, (index, _, _) in _native.TRACK_OUTPUTS.items():
        assert re.search(r"#define THR_TRACK_%s %d\b" % (name.upper(), index), header), name
    assert "#define THR_TRACK_N_OUTPUTS %d" % len(_native.TRACK_OUTPUTS) in header
    assert "#define THR_TRACK_LOST %d" % _native.TRACK_LOST in header and track.LOST == _native.TRACK_LOST == track_ref.LOST
    assert {"thr_track", "thr_track_fetch", "thr_track_free", "thr_debug_track_times", "thr_debug_track_geometry"} <= set(_native.EXPORTS)
    assert [f[0] for f in _native.ThrTrackOpts._fields_] == ["q", "v0", "gate", "max_rounds", "reserved"]
    assert [f[0] for f in _native.ThrTrackCounts._fields_] == ["rows", "tracks", "used", "rejected", "rounds", "converged"]
    assert track.GATE_999 == track_ref.GATE_999 == -2.0 * np.log(0.001)
    assert "track.hip" in build.SOURCES and "track_scan.hpp" in build.HEADERS
    assert build.UNPROFILED_TRACK == ("track.hip", "track_scan.hpp")
    assert build.PER_FILE_FLAGS["track.hip"] == ["-ffp-contract=off"]
    source, scan = (open(os.path.join(build.CSRC, name)).read() for name in ("track.hip", "track_scan.hpp"))
    assert "#pragma clang fp contract(off)" in source and "#pragma clang fp contract(off)" in scan
    assert "sort_cells(" in source and "build_layout(" in source and "seg::reduce<" in source
    # the only atomic counts changed mask bits in an integer
    assert source.count("atomicAdd") == 1 and "int* __restrict__ changed" in source and "hipMalloc(" not in source


def test_the_built_library_exports_thr_track():
    assert os.path.exists(_native.LIB_PATH), "the library is not built: python -m thrifty_amd.build"
    lib = _native.load_library()
    assert lib.thr_track and lib.thr_track_fetch and lib.thr_track_free and lib.thr_debug_track_times and lib.thr_debug_track_geometry


def test_csrc_hash_does_not_see_the_two_new_files(monkeypatch):
    with_track = build.csrc_hash()
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "track.hip"])
    monkeypatch.setattr(build, "HEADERS", [h for h in build.HEADERS if h != "track_scan.hpp"])
    assert build.csrc_hash() == with_track
    monkeypatch.undo()
    monkeypatch.setattr(build, "UNPROFILED_TRACK", ())
    assert build.csrc_hash() != with_track


def test_the_recorded_tolerances_cover_every_scene():
    scenes = TOLERANCES["scenes"]
    assert TOLERANCES["factor"] == 16 and TOLERANCES["longdouble_bits"] >= 64
    assert set(scenes) == OLD_SCENES | set(CLAUSES) and not OLD_SCENES & set(CLAUSES)
    for name in OLD_SCENES:
        for key in OUTPUTS:
            # metres (m^2, 1) on positions of 2e4 m: an error in an element or a combination is ten orders above this
            assert 0.0 <= scenes[name][key] < 1e-6, (name, key)
    assert TOLERANCES["factor"] == track_check.FACTOR
    not_compared = {}
    for name in CLAUSES:      # their own condition, column by column: a bound below 1e-3 of what the column is measured against
        assert isinstance(scenes[name]["gated"], bool)
        assert ("with_gate" in scenes[name]) == (scenes[name]["gated"] and name in track_scenes.REGIMES)
        for tag, record in (("", scenes[name]), (" with the gate", scenes[name].get("with_gate"))):
            if record is None:
                continue
            assert [len(record["columns"][key]) for key in OUTPUTS] == [4, 6, 4, 6, 1]
            assert all(0.0 <= max(record["columns"][key]) == record[key] for key in OUTPUTS)
            assert 16 * max(record["columns"][key][col] for key in ("filt", "smooth") for col in (0, 2)) <= record["position_bound"]
            assert record["position_bound"] < 1e-3 * record["smallest_sigma"]
            for column, numbers in record["not_compared"].items():
                assert numbers["bound"] >= 1e-3 * numbers["scale"] > 0.0 and column[:column.index("[")] in OUTPUTS[1:]
            if record["not_compared"]:
                not_compared[name + tag] = sorted(record["not_compared"])
    # every regime is compared with the gate as well, and the columns whose bound says nothing are these and no others
    # ("Range of the definition"): one that joins them does not do so unseen
    assert all(scenes[name]["gated"] for name in CLAUSES) and len(track_scenes.REGIMES) == 11
    velocity, position = ["smooth_var[2]", "smooth_var[5]"], ["filt_var[0]", "filt_var[3]", "smooth_var[0]", "smooth_var[3]"]
    assert not_compared == {"v0_1e5": velocity, "v0_1e5 with the gate": velocity, "gap_400_v0_1e5": velocity,
                            "gap_400_v0_1e5 with the gate": velocity, "steps_1e4": position, "steps_1e4 with the gate": position}
    assert set(TOLERANCES["out_of_range"]) == set(track_scenes.OUT_OF_RANGE) and not set(track_scenes.OUT_OF_RANGE) & set(CLAUSES)
    generator = _generator()
    for name, record in TOLERANCES["out_of_range"].items():      # measured, documented, in no test
        assert record["position_bound"] >= 1e-3 * record["smallest_sigma"], name
        assert generator.measure_out_of_range(name, track_scenes.OUT_OF_RANGE[name]) == record, name


def test_the_old_scenes_keep_their_bytes_and_their_records():
    """The knobs that the clauses added draw no random number unless used; no recorded tolerance of an old scene moved.
    The digests were taken before the knobs and the new scenes were added."""
    h = hashlib.sha256()
    for name, s in [("gating_%d" % k, track_scenes.gating(k)) for k in range(3)] + sorted(track_scenes.seams().items()):
        h.update(name.encode())
        for key in track_scenes.COLUMNS + ("outlier",):
            h.update(np.ascontiguousarray(s[key]).tobytes())
        h.update(repr((s["q"], s["v0"])).encode())
    assert h.hexdigest() == "5bed668bfd8b4986d29a59691beaa559d54b8cb93d54c58b02901ef58042f3bf"
    old = {name: TOLERANCES["scenes"][name] for name in OLD_SCENES}
    assert hashlib.sha256(json.dumps(old, sort_keys=True).encode()).hexdigest() == \
        "3816d1656859c196075e75d7680fa14ac5ad9c9e71eaab88c19861b33bcc2ec9"
    generator = _generator()      # and the generator still writes them: a few of them measured again
    assert generator.measure(track_scenes.gating(1), gate=0.0) == old["gating_1_no_gate"]
    for name in ("single_257", "meet_at_last", "reject_256", "invalid_tile", "epoch_ms"):
        assert generator.measure(track_scenes.seams()[name]) == old[name], name


@pytest.mark.parametrize("name", CLAUSES)
def test_a_clause_scene_holds_what_it_is_named_after_and_its_record_is_the_generators(name):
    track_check.assert_clause_holds(name)
    s, options = track_scenes.clauses()[name]      # measure_clause stops where the positions miss the usefulness condition
    assert _generator().measure_clause(name, s, options) == TOLERANCES["scenes"][name]


def test_the_tiles_form_is_the_scan_inside_one_fragment_and_the_recursion_across_fragments():
    s = track_scenes.seams()["single_255"]
    scan, tiles = _ref(s, form="scan"), _ref(s, form="tiles")
    assert scan["counts"] == tiles["counts"]
    for key in OUTPUTS + ("track_stats", "used"):
        assert scan[key].tobytes() == tiles[key].tobytes(), key
    assert track_ref.fragments(0, 255) == [(0, 255)] and track_ref.fragments(0, 769) == [(0, 256), (256, 512), (512, 768), (768, 769)]
    assert track_ref.fragments(100, 600) == [(0, 156), (156, 412), (412, 600)] and track_ref.fragments(256, 3) == [(0, 3)]
    assert track_ref.fragments(255, 2) == [(0, 1), (1, 2)] and track_ref.fragments(7, 0) == []
    for name in ("invalid_tile", "single_769"):
        s = track_scenes.seams()[name]
        truth, tiles, scan = _ref(s, kind=np.longdouble), _ref(s, form="tiles"), _ref(s, form="scan")
        assert tiles["counts"] == truth["counts"] and np.array_equal(tiles["used"], truth["used"])
        assert any(tiles[out].tobytes() != scan[out].tobytes() for out in OUTPUTS)      # another tree
        # the tolerance a device gets on this scene (the record of the OTHER two forms times 16), against longdouble
        for out in OUTPUTS:
            a, b = tiles[out].astype(np.longdouble), truth[out]
            assert np.array_equal(np.isnan(a), np.isnan(b))
            assert float(np.nanmax(np.abs(a - b))) <= track_check.bound(TOLERANCES["scenes"][name][out], tiles[out]), (name, out)


@pytest.mark.parametrize("name", ["gating_1", "single_513", "invalid_tile", "equal_times", "epoch_ms", "no_valid_row"])
def test_the_three_cpu_statements_agree(name):
    s = track_scenes.gating(int(name[-1])) if name.startswith("gating") else track_scenes.seams()[name]
    runs = {(kind, form): _ref(s, kind=kind, form=form)
            for kind, form in ((np.longdouble, "sequential"), (np.float64, "sequential"), (np.float64, "scan"))}
    truth = runs[np.longdouble, "sequential"]
    record = TOLERANCES["scenes"][name]
    assert truth["counts"]["rounds"] == record["rounds"] and truth["counts"]["converged"] == record["converged"]
    for key, run in runs.items():
        assert run["counts"] == truth["counts"] and np.array_equal(run["used"], truth["used"])
        assert np.array_equal(run["order"], truth["order"]) and np.array_equal(run["track_ptr"], truth["track_ptr"])
        if key[0] is np.longdouble:
            continue
        for out in OUTPUTS:
            a, b = run[out].astype(np.longdouble), truth[out]
            assert np.array_equal(np.isnan(a), np.isnan(b))
            if np.any(~np.isnan(a)):
                # re-measured here: the record is this number (the larger of the two forms')
                assert float(np.nanmax(np.abs(a - b))) <= record[out], (key, out)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_the_gate_reaches_a_fixed_point_and_rejects_every_planted_outlier(k):
    s = track_scenes.gating(k)
    ref = _ref(s, smoother=False)
    assert ref["counts"]["converged"] == 1 and ref["counts"]["rounds"] <= 4
    assert int(s["outlier"].sum()) > 40 and not np.any(ref["used"].astype(bool) & s["outlier"])
    good = (s["valid"] == 1) & ~s["outlier"]
    assert np.count_nonzero(good & (ref["used"] == 0)) <= 0.005 * np.count_nonzero(good)      # the 99.9 % gate, in three rounds
    assert ref["counts"]["used"] + ref["counts"]["rejected"] == int(s["valid"].sum())
    assert not np.any(ref["track_flags"])
    # a filter run with a converged mask changes nothing: one more round gives the same result
    again = _ref(s, smoother=False, max_rounds=8)
    assert again["counts"] == ref["counts"] and np.array_equal(again["used"], ref["used"])


def test_an_outlier_as_start_row_costs_the_track_its_rows_and_invalidating_it_is_the_remedy():
    s = track_scenes.scene(77, rows=200)
    first = np.argmin(s["timestamp"])
    s["x"][first] += 1e5
    # the first run takes every row, so the state jumps to the truth at once and only the rows right behind the start
    # contradict it; every further round predicts from the start row through the rows it has lost, and loses more
    lost = [_ref(s, smoother=False, max_rounds=rounds)["counts"] for rounds in (1, 4, 16)]
    assert [c["converged"] for c in lost[:2]] == [0, 0]
    assert 25 <= lost[0]["rejected"] < lost[1]["rejected"] <= lost[2]["rejected"] and lost[1]["rejected"] > 60
    s["valid"][first] = 0      # the remedy
    ref = _ref(s, smoother=False)
    assert ref["counts"]["converged"] == 1 and ref["counts"]["rejected"] <= 3 and ref["track_flags"][0] == 0
    assert np.isnan(ref["filt"][first]).all() and ref["used"][first] == 0


def test_bad_inputs_are_refused_before_the_library_is_loaded(monkeypatch):
    def no_library():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_native, "load_library", no_library)
    tx, t, x, y, r = [1, 1, 1], [0.0, 1.0, 2.0], [0.0, 1.0, 2.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
    with pytest.raises(ValueError, match="one-dimensional"):
        track.track_columns([tx], [t], [x], [y], [r], [r], accel=1.0)
    with pytest.raises(ValueError, match="one-dimensional"):
        track.track_columns(tx, t[:2], x, y, r, r, accel=1.0)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="timestamp"):
            track.track_columns(tx, [0.0, bad, 2.0], x, y, r, r, accel=1.0)
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="variance"):
            track.track_columns(tx, t, x, y, [1.0, bad, 1.0], r, accel=1.0)
        with pytest.raises(ValueError, match="variance"):
            track.track_columns(tx, t, x, y, r, [1.0, 1.0, bad], accel=1.0)
    with pytest.raises(ValueError, match="position"):
        track.track_columns(tx, t, [0.0, np.nan, 2.0], y, r, r, accel=1.0)
    for rounds in (0, 17, 2.5):
        with pytest.raises(ValueError, match="max_rounds"):
            track.track_columns(tx, t, x, y, r, r, accel=1.0, max_rounds=rounds)
    with pytest.raises(ValueError, match="accel"):
        track.track_columns(tx, t, x, y, r, r)
    for kw in (dict(accel=-1.0), dict(accel=np.nan)):
        with pytest.raises(ValueError, match="accel"):
            track.track_columns(tx, t, x, y, r, r, **kw)
    for bad in (0.0, -1.0, np.inf):
        with pytest.raises(ValueError, match="speed_prior"):
            track.track_columns(tx, t, x, y, r, r, accel=1.0, speed_prior=bad)
    for bad in (-1.0, np.nan):
        with pytest.raises(ValueError, match="gate"):
            track.track_columns(tx, t, x, y, r, r, accel=1.0, gate=bad)
    one_d = np.zeros(2, dtype=pos_est._result_dtype(1))
    with pytest.raises(ValueError, match="1-D"):
        track.track(one_d, 1.0, 1.0)
    with pytest.raises(ValueError, match="3-D"):
        track.track(np.zeros(2, dtype=pos_est._result_dtype(3)), 1.0, 1.0)
    with pytest.raises(ValueError, match="sigma_m"):
        track.track(np.zeros(2, dtype=pos_est._result_dtype(2)), 0.0, 1.0)


def test_a_bad_row_that_is_invalid_is_not_refused(monkeypatch):
    seen = {}

    def fake(tx, *cols, **kw):
        seen["valid"] = kw["valid"]
        raise RuntimeError("reached the device call")
    monkeypatch.setattr(_native, "track", fake)
    with pytest.raises(RuntimeError, match="reached"):
        track.track_columns([1, 1], [0.0, 1.0], [0.0, np.nan], [0.0, 0.0], [1.0, -1.0], [1.0, 0.0], valid=[1, 0], accel=1.0)
    assert seen["valid"].tolist() == [1, 0]


def _positions():
    pos = np.zeros(6, dtype=pos_est._result_dtype(2))
    pos["group_id"], pos["tx"], pos["timestamp"] = np.arange(6), [4, 4, 9, 4, 9, 4], [0.0, 1.0, 0.5, 2.0, 1.5, 3.0]
    pos["dop"], pos["x"], pos["y"] = [1.0, 2.0, 1.5, np.nan, 0.0, 1.0], [0.0, 1.0, np.nan, 3.0, 4.0, 5.0], [0.0] * 6
    posq = np.zeros(6, dtype=pos_quality.QUALITY_DTYPE)
    for name in pos.dtype.names:
        posq[name] = pos[name]
    posq["xdop"], posq["ydop"] = [0.5, 1.0, 1.0, 1.0, 1.0, -1.0], [2.0, 1.0, 1.0, np.inf, 1.0, 1.0]
    posq["flags"] = [0, pos_quality.INCONSISTENT | pos_quality.NO_CANDIDATE, 0, 0, pos_quality.EXCLUDED | pos_quality.INCONSISTENT, 0]
    return pos, posq


def test_positions_map_to_the_stated_variances():
    pos, posq = _positions()
    rx, ry, valid = track.measurement_columns(pos, 3.0)
    assert valid.tolist() == [True, True, False, False, False, True]
    assert np.array_equal(rx[valid], (3.0 * pos["dop"][valid]) ** 2 / 2.0) and np.array_equal(rx[valid], ry[valid])
    rx, ry, valid = track.measurement_columns(posq, 3.0)
    assert valid.tolist() == [True, False, False, False, True, False]
    assert np.array_equal(rx[valid], (3.0 * posq["xdop"][valid]) ** 2) and np.array_equal(ry[valid], (3.0 * posq["ydop"][valid]) ** 2)
    assert rx[0] == 2.25 and ry[0] == 36.0


def _fake_native(calls):
    """_native.track answered by the NumPy statement."""
    def fake(tx, timestamp, x, y, rx, ry, valid=None, q=None, v0=10.0, gate=track_ref.GATE_999, max_rounds=4, outputs=None, device_id=0):
        calls.append(dict(tx=np.array(tx), valid=None if valid is None else np.array(valid), rx=np.array(rx), ry=np.array(ry), q=q, v0=v0,
                          gate=gate, max_rounds=max_rounds))
        ref = track_ref.run(tx, timestamp, x, y, rx, ry, valid, q=q, v0=v0, gate=gate, max_rounds=max_rounds)
        return ref["counts"], {name: ref[name] for name in _native.TRACK_OUTPUTS}
    return fake


def test_track_round_trip_and_summary(monkeypatch, tmp_path):
    calls = []
    monkeypatch.setattr(_native, "track", _fake_native(calls))
    pos, _ = _positions()
    pos["dop"], pos["x"] = 1.0, [0.0, 1.0, 7.0, 2.0, 8.0, np.nan]
    records, out = track.track(pos, 2.0, 0.5)
    assert calls[0]["q"] == 0.25 and calls[0]["v0"] == 10.0 and calls[0]["gate"] == track.GATE_999 and calls[0]["max_rounds"] == 4
    assert np.array_equal(calls[0]["rx"], np.full(6, 2.0)) and calls[0]["valid"].tolist() == [1, 1, 1, 1, 1, 0]
    # (tx, timestamp) order; the invalid last row of tx 4 is tracked (predicted), so it has a line
    assert records["group_id"].tolist() == [0, 1, 3, 5, 2, 4] and records["used"].tolist() == [1, 1, 1, 0, 1, 1]
    assert np.array_equal(records["x"], out["smooth"][out["order"], 0]) and np.isnan(records["nis"][3])
    assert np.array_equal(records["speed"], np.hypot(records["vx"], records["vy"])) or np.allclose(
        records["speed"], np.hypot(records["vx"], records["vy"]), rtol=1e-15, atol=0)
    path = str(tmp_path / "data.track")
    track.save_tracks(path, records)
    lines = open(path).read().splitlines()
    assert len(lines) == 6 and lines[0].split()[1] == "0.000000" and len(lines[0].split()) == len(track.TRACK_DTYPE["names"])
    back = track.load_tracks(path)
    for name in track.TRACK_DTYPE["names"]:
        assert np.array_equal(back[name], records[name], equal_nan=name == "nis"), name
    with pytest.raises(ValueError, match="fields"):
        track.load_tracks(io.StringIO("1 2.0 3 4.0\n"))
    filtered, _ = track.track(pos, 2.0, 0.5, filter_only=True)
    assert np.array_equal(filtered["x"], out["filt"][out["order"], 0]) and not np.array_equal(filtered["x"], records["x"])
    only, sub = track.track(pos, 2.0, 0.5, tx=[9])
    assert only["group_id"].tolist() == [2, 4] and sub["rows"].tolist() == [2, 4] and calls[-1]["tx"].tolist() == [9, 9]
    summary = track.format_summary(out).splitlines()
    assert len(summary) == 2 and summary[0].startswith("TX 4: 4 rows, 3 used, 0 rejected, mean nis ") and "km/h" in summary[0]
    out["track_flags"][1] = track.LOST
    assert track.format_summary(out).splitlines()[1].endswith(", LOST")


def test_the_command_line(monkeypatch, tmp_path, capsys):
    monkeypatch.chdir(tmp_path)
    open("in.posq", "w").close()
    args = track._parser().parse_args(["in.posq", "--sigma", "2", "--accel", "0.5", "--tx", "4", "9"])
    assert (args.sigma_m, args.accel, args.speed_prior, args.gate, args.max_rounds) == (2.0, 0.5, 10.0, track.GATE_999, 4)
    assert args.tx == [4, 9] and not args.filter_only and args.npz is None and args.output.name == "data.track"
    args.positions.close() if hasattr(args.positions, "close") else None
    args.output.close()
    with pytest.raises(SystemExit):
        track._parser().parse_args(["--accel", "1"])          # --sigma has no default
    with pytest.raises(SystemExit):
        track._parser().parse_args(["--sigma", "1"])          # nor has --accel
    calls = []
    monkeypatch.setattr(_native, "track", _fake_native(calls))
    pos, posq = _positions()
    posq["xdop"], posq["ydop"], posq["flags"], posq["x"] = 1.0, 2.0, 0, np.arange(6.0)
    pos_path, posq_path, out_path, npz_path = (str(tmp_path / name) for name in ("data.pos", "data.posq", "data.track", "all.npz"))
    pos["dop"], pos["x"] = 1.0, np.arange(6.0)
    pos_est.save_positions(pos_path, pos)
    pos_quality.save_quality(posq_path, posq)
    assert track._main([posq_path, "-o", out_path, "--sigma", "2", "--accel", "0.5", "--speed-prior", "3", "--gate", "9", "--rounds", "2",
                        "--npz", npz_path]) == 0
    assert (calls[-1]["q"], calls[-1]["v0"], calls[-1]["gate"], calls[-1]["max_rounds"]) == (0.25, 3.0, 9.0, 2)
    assert np.array_equal(calls[-1]["rx"], np.full(6, 4.0)) and np.array_equal(calls[-1]["ry"], np.full(6, 16.0))
    records, _ = track.track(pos_quality.load_quality(posq_path), 2.0, 0.5, speed_prior=3.0, gate=9.0, max_rounds=2)
    back = track.load_tracks(out_path)
    assert all(np.array_equal(back[name], records[name], equal_nan=True) for name in track.TRACK_DTYPE["names"])
    assert capsys.readouterr().out.startswith("TX 4: 4 rows")
    saved = np.load(npz_path)
    assert set(_native.TRACK_OUTPUTS) <= set(saved.files) and int(saved["count_rounds"]) >= 1
    assert track._main([pos_path, "-o", out_path, "--sigma", "2", "--accel", "0.5", "--tx", "9", "--filter-only"]) == 0
    assert np.array_equal(calls[-1]["rx"], np.full(2, 2.0)) and calls[-1]["tx"].tolist() == [9, 9]
    records, _ = track.track(pos_est.load_positions(pos_path), 2.0, 0.5, tx=[9], filter_only=True)
    assert np.array_equal(track.load_tracks(out_path)["vx"], records["vx"])
    one_d = np.zeros(2, dtype=pos_est._result_dtype(1))
    pos_est.save_positions(pos_path, one_d)
    assert track._main([pos_path, "-o", out_path, "--sigma", "2", "--accel", "0.5"]) == 1
    assert "1-D" in capsys.readouterr().err
