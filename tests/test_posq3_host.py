"""Host side of `thr_posq3` (no GPU): the wiring into the header, the symbol list and the build; what is refused
before the library is loaded; the NumPy statement (tests/posq3_ref.py) on the fixtures
(tests/golden/make_golden_posq3.py); the .posq3 text format and its .posq companion; the command line's options."""
import io
import json
import os
import re

import numpy as np
import pytest

import pos3_golden
import pos3_ref
import posg3_golden
import posq3_golden
import posq3_ref
import posq_ref
from thrifty_amd import _native, build, pos_3d_quality, pos_quality, tdoa_est, track

ROOT = posq3_golden.ROOT


def test_thr_posq3_is_declared_listed_and_built():
    header = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
    assert re.search(r"\bint thr_posq3\(int device_id, size_t n_groups, const int64_t\* group_ptr,", header)
    assert re.search(r"\bint thr_posq3_fetch\(thr_posq3_result\* result, int which, void\* dst, size_t dst_bytes\);", header)
    assert "void thr_posq3_free(thr_posq3_result* result);" in header and "int thr_debug_posq3_times(double* ms_out" in header
    assert "#define THR_ABI_VERSION 11" in header and _native.ABI_VERSION == 11
    block = header[header.index("within 11, a pure addition"):header.index("#define THR_ABI_VERSION")]
    assert re.search(r"\+ thr_posq3 / thr_posq3_fetch / thr_posq3_free / thr_debug_posq3_times", block)
    for name, (index, _, _) in _native.POSQ3_OUTPUTS.items():
        assert re.search(r"#define THR_POSQ3_%s %d\b" % (name.upper(), index), header), name
    assert "#define THR_POSQ3_N_OUTPUTS %d" % len(_native.POSQ3_OUTPUTS) in header and len(_native.POSQ3_OUTPUTS) == 22
    for name in ("INCONSISTENT", "EXCLUDED", "NO_CANDIDATE"):
        assert "#define THR_POSQ3_%s %d" % (name, getattr(_native, "POSQ3_" + name)) in header
        assert getattr(pos_3d_quality, name) == getattr(_native, "POSQ3_" + name) == getattr(_native, "POSQ_" + name)
    # thr_posq's names keep their indices and element types; the two dops are appended
    for name, (index, kind, _) in _native.POSQ_OUTPUTS.items():
        assert _native.POSQ3_OUTPUTS[name][:2] == (index, kind), name
    assert list(_native.POSQ3_OUTPUTS)[20:] == ["hdop", "vdop"]
    counts = {"groups": 3, "rows": 11, "flagged": 1, "tasks": 5}
    shapes = {name: entry[2](counts) for name, entry in _native.POSQ3_OUTPUTS.items()}
    assert shapes["pos"] == shapes["full_pos"] == (3, 3) and shapes["task_pos"] == (5, 3) and shapes["q"] == (3, 6)
    assert shapes["hdop"] == shapes["vdop"] == (3,) and shapes["residual"] == (11,)
    assert {"thr_posq3", "thr_posq3_fetch", "thr_posq3_free", "thr_debug_posq3_times"} <= set(_native.EXPORTS)
    assert [f[0] for f in _native.ThrPosq3Opts._fields_] == ["max_iter", "min_rx", "has_z_range", "x0", "z_range", "gate_m", "ratio"]
    assert re.search(r"typedef struct thr_posq3_opts \{\s*int32_t max_iter, min_rx, has_z_range;\s*double x0\[3\];\s*double z_range\[2\];"
                     r"[^}]*double gate_m, ratio;\s*\} thr_posq3_opts;", header)
    assert [f[0] for f in _native.ThrPosq3Counts._fields_] == [f[0] for f in _native.ThrPosqCounts._fields_]
    assert _native.POSQ3_MIN_RX == (5, 6) and pos_3d_quality.MIN_RX_FLOOR == (5, 6) and posq3_ref.MIN_RX == (5, 6)
    assert callable(_native.posq3) and callable(_native.posq3_times)
    assert "posq3.hip" in build.SOURCES and build.UNPROFILED_POSQ3 == ("posq3.hip",)
    assert build.PER_FILE_FLAGS["posq3.hip"] == ["-ffp-contract=off"]
    source = open(os.path.join(build.CSRC, "posq3.hip")).read()
    assert '#include "pos3_lm.hpp"' in source and "#pragma clang fp contract(off)" in source
    assert "solve_team<FREE_Z, kRegRows, WEIGHTED, AllRows>" in source and "solve_team<FREE_Z, kRegRows, WEIGHTED, NotReceiver>" in source
    assert not re.search(r"atomic[A-Z_(]", source) and "hipMalloc(" not in source
    assert int(re.search(r"constexpr int kRegRows = (\d+);", source).group(1)) == _native.POS3_REGISTER_ROWS
    assert int(re.search(r"constexpr int kMinRxKnownHeight = (\d+);", source).group(1)) == _native.POSQ3_MIN_RX[0]
    assert int(re.search(r"constexpr int kMinRxFreeZ = (\d+);", source).group(1)) == _native.POSQ3_MIN_RX[1]


def test_the_iteration_header_keeps_the_unweighted_solve_as_its_default():
    shared = open(os.path.join(build.CSRC, "pos3_lm.hpp")).read()
    assert "template <bool FREE_Z, int REG_ROWS, bool WEIGHTED = false, class Used = poslm::AllRows>" in shared
    assert "const double* __restrict__ weight = nullptr, Used used = Used{})" in shared
    assert "sqrt((ax * ax + ay * ay) + az * az)" in shared and shared.count("for (int it = 0; it < max_iter; ++it)") == 1
    assert "w_scale = double(n_used) / group8_sum(w_sum);" in shared and "int m_used;" in shared
    # the known-height weighted terms are pos_lm.hpp's, operand for operand
    flat = open(os.path.join(build.CSRC, "pos_lm.hpp")).read()
    for term in ("w * (res * res)", "w * (gx * gx)", "w * (gx * gy)", "w * (gy * gy)", "w * (gx * res)", "w * (gy * res)",
                 "wreg[k] = wreg[k] * w_scale;", "weight[i] * w_scale"):
        assert term in shared and term in flat, term
    for name in ("pos3.hip", "posg3.hip"):      # the existing calls stand as they were
        text = open(os.path.join(build.CSRC, name)).read()
        assert re.search(r"solve_team<(false|true|FREE_Z), kRegRows>\(", text) and "WEIGHTED" not in text, name


def test_the_built_library_exports_thr_posq3():
    assert os.path.exists(_native.LIB_PATH), "the library is not built: python -m thrifty_amd.build"
    lib = _native.load_library()
    assert lib.thr_posq3 and lib.thr_posq3_fetch and lib.thr_posq3_free and lib.thr_debug_posq3_times


def test_csrc_hash_does_not_see_the_new_file(monkeypatch):
    with_posq3 = build.csrc_hash()
    with open(os.path.join(ROOT, "profiles", "hbm_traffic.json")) as f:
        recorded = json.load(f)
    hashes = {w["_source"]["csrc_sha16"] for w in recorded.values() if isinstance(w, dict) and "_source" in w}
    assert hashes == {with_posq3}                    # the recorded hash still holds
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "posq3.hip"])
    assert build.csrc_hash() == with_posq3
    monkeypatch.undo()
    monkeypatch.setattr(build, "UNPROFILED_POSQ3", ())
    assert build.csrc_hash() != with_posq3


def test_the_parents_digests_are_stored():
    digests = posq3_golden.parent_digests()
    assert set(digests) == {"thr_pos3", "thr_posg3"}
    assert set(digests["thr_pos3"]) == set(pos3_golden.SETS) and set(digests["thr_posg3"]) == set(posg3_golden.SETS)
    for stage, names in (("thr_pos3", _native.POS3_OUTPUTS), ("thr_posg3", _native.POSG3_OUTPUTS)):
        for entry in digests[stage].values():
            assert set(entry) == set(names) and all(re.fullmatch(r"[0-9a-f]{64}", v) for v in entry.values())
    assert len(_native.POS3_OUTPUTS) == 8


def test_bad_inputs_are_refused_before_the_library_is_loaded(monkeypatch):
    def no_library():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_native, "load_library", no_library)
    table = {k: np.array(xyz) for k, xyz in enumerate([(0.0, 0.0, 5.0), (100.0, 0.0, 9.0), (0.0, 100.0, 7.0)])}
    args = ([0, 3], [0, 0, 1], [1, 2, 2], [1e-9, 2e-9, 3e-9], [1.0, 1.0, 1.0])
    call = pos_3d_quality.quality3_columns
    with pytest.raises(ValueError, match="three coordinates"):
        call(*args, {k: v[:2] for k, v in table.items()}, height=1.0)
    with pytest.raises(ValueError, match="no default mode"):
        call(*args, table)
    with pytest.raises(ValueError, match="no default mode"):
        call(*args, table, height=1.0, free_z=True)
    with pytest.raises(KeyError):
        call(*args, {0: table[0], 1: table[1], 7: table[2]}, height=1.0)
    with pytest.raises(ValueError, match="group_ptr"):
        call([0, 2], *args[1:], table, height=1.0)
    for weights in ([1.0, -1.0, 1.0], [1.0, np.nan, 1.0], [1.0, np.inf, 1.0]):
        with pytest.raises(ValueError, match="negative or not finite"):
            call(*args, table, free_z=True, weights=weights)
    with pytest.raises(ValueError, match="one weight per row"):
        call(*args, table, height=1.0, weights=[1.0, 1.0])
    with pytest.raises(ValueError, match="weights must be"):
        call(*args, table, height=1.0, weights="energy")
    for ratio in (0.0, -0.5, 1.5, np.nan):
        with pytest.raises(ValueError, match="ratio"):
            call(*args, table, height=1.0, ratio=ratio)
    for kwargs, min_rx in ((dict(height=1.0), 4), (dict(free_z=True), 5), (dict(free_z=True), 4), (dict(height=1.0), 65), (dict(height=1.0), 5.5)):
        with pytest.raises(ValueError, match="min_rx"):
            call(*args, table, min_rx=min_rx, **kwargs)
    for gate in (0.0, -3.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="exclude_gate_m"):
            call(*args, table, height=1.0, exclude_gate_m=gate)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="finite"):
            call(*args, table, height=bad)
    with pytest.raises(ValueError, match="belong to free_z"):
        call(*args, table, height=1.0, z0=2.0)
    with pytest.raises(ValueError, match="z_range"):
        call(*args, table, free_z=True, z_range=(5.0, 5.0))
    with pytest.raises(ValueError, match="outside the z range"):
        call(*args, table, free_z=True, z0=50.0, z_range=(-20.0, 40.0))
    level = {k: np.array([v[0], v[1], 6.0]) for k, v in table.items()}
    with pytest.raises(ValueError, match="mirror plane"):       # a start on the antennas' common plane
        call(*args, level, free_z=True, z0=6.0)
    rows = np.zeros(3, dtype=tdoa_est.TDOA_DTYPE)
    rows["rx0"], rows["rx1"] = args[1], args[2]
    group = [tdoa_est.TdoaGroup(1, 2.0, 3, rows)]
    with pytest.raises(ValueError, match="ratio"):
        pos_3d_quality.solve(group, table, height=1.0, ratio=2.0)
    with pytest.raises(ValueError, match="min_rx"):
        pos_3d_quality.solve(group, table, free_z=True, min_rx=5)
    with pytest.raises(ValueError, match="three coordinates"):
        pos_3d_quality.solve(group, {k: v[:2] for k, v in table.items()}, height=1.0)
    with pytest.raises(ValueError, match="no height for tx 3"):
        pos_3d_quality.solve(group, table, height={4: 1.0})


def _ref(g, weighted=True, **kw):
    opts = posq3_golden.options(g, weighted, weights_key="weights")
    opts.update(kw)
    return posq3_ref.posq3_ref(*posq3_golden.columns(g), **opts)


_refs = {}


def ref_of(name):
    if name not in _refs:
        _refs[name] = _ref(posq3_golden.load(name))
    return _refs[name]


def test_fixtures_are_small_and_hold_the_scenes_of_the_issue():
    for name in posq3_golden.SETS:
        assert os.path.getsize(os.path.join(posq3_golden.GOLDEN, name + ".npz")) <= 64 * 1024
        g = posq3_golden.load(name)
        assert 24 <= len(g["group_id"]) <= 36 and 1e-14 < float(g["ref_err_max"]) < 1e-9
        assert len(g["full_x_star"]) == len(g["group_id"]) and len(g["task_x_star"]) == g["ref_task_ptr"][-1]
        assert (float(g["gate_m"]), float(g["ratio"])) == (3.0, 0.5)
        assert bool(g["free_z"]) == (name in posq3_golden.SETS_Z) and int(g["min_rx"]) == (6 if bool(g["free_z"]) else 5)
        assert np.all(np.abs(np.hypot(*g["rx_xyz"][:, :2].T) - 100.0) < 20.0)
    g = posq3_golden.load("h_fault6")
    assert len(g["rx_ids"]) == 6 and set(np.diff(g["group_ptr"]).tolist()) == {15} and len(g["weights"]) == 0
    assert (g["rx_xyz"][:, 2].min(), g["rx_xyz"][:, 2].max()) == (3.0, 40.0) and np.all(g["group_h"] == 1.0) and np.all(g["mobile"][:, 2] == 1.0)
    affected = g["planted"] >= 0
    assert affected.sum() == 10 and np.all(affected == (np.arange(30) % 3 == 2)) and set(g["planted"][affected]) == set(g["rx_ids"])
    for name in posq3_golden.SETS_Z:
        g = posq3_golden.load(name)
        assert len(g["rx_ids"]) == 7 and (g["rx_xyz"][:, 2].min(), g["rx_xyz"][:, 2].max()) == (3.0, 80.0)
        assert g["z_range"].tolist() == [-20.0, 100.0]
    g = posq3_golden.load("z_weighted7")
    assert np.array_equal(g["weights"], g["snr"]) and len(set(np.diff(g["group_ptr"]))) > 1
    g = posq3_golden.load("h_five")
    assert len(g["rx_ids"]) == 5 and len(set(g["group_h"].tolist())) == 24 and np.array_equal(g["group_h"], g["mobile"][:, 2])


@pytest.mark.parametrize("name", posq3_golden.SETS)
def test_the_statement_excludes_the_planted_receiver_and_no_other(name):
    g = posq3_golden.load(name)
    ref = ref_of(name)
    affected = g["planted"] >= 0
    assert affected.sum() >= 6
    np.testing.assert_array_equal(ref["counts"][:, 2], np.where(affected, posq3_golden.dense(g, np.maximum(g["planted"], g["rx_ids"][0])), -1))
    np.testing.assert_array_equal(ref["flags"], np.where(affected, 3, 0))
    np.testing.assert_array_equal(ref["flags"], g["ref_flags"])
    assert np.all(ref["rms"][affected, 1] <= 0.5 * ref["rms"][affected, 0]) and ref["rms"][~affected, 0].max() < 3.0
    n_rx = len(g["rx_ids"])
    np.testing.assert_array_equal(ref["counts"][:, 0], np.where(affected, n_rx - 1, n_rx))


@pytest.mark.parametrize("name", posq3_golden.SETS)
def test_the_statement_sits_on_the_exact_minimisers(name):
    g = posq3_golden.load(name)
    ref = ref_of(name)
    np.testing.assert_array_equal(ref["task_ptr"], g["ref_task_ptr"])
    assert np.max(np.abs(ref["pos"] - g["ref_pos"])) <= float(g["ref_err_max"])      # NumPy's sums may differ between builds
    for pos, status, star in ((ref["full_pos"], ref["full_status"], g["full_x_star"]), (ref["task_pos"], ref["task_status"], g["task_x_star"])):
        ok = np.all(np.isfinite(star), axis=1)
        # with z free most candidates still hold the late receiver and do not end OK: the excluded ones do
        assert np.all(status[ok] == 0) and ok.sum() >= np.count_nonzero(ref["flags"] & 2) > 0
        assert np.max(np.abs(pos[ok] - star[ok])) <= float(g["ref_err_max"])
    # the chosen task's position: within ref_err_max of the mpmath minimiser
    chosen = np.where(((ref["flags"] & 2) != 0)[:, None], np.nan, g["full_x_star"])
    for k in np.flatnonzero(ref["flags"] & 2).tolist():
        t = int(ref["task_ptr"][k]) + ref["task_rx"][ref["task_ptr"][k]:ref["task_ptr"][k + 1]].tolist().index(int(ref["counts"][k, 2]))
        chosen[k] = g["task_x_star"][t]
    assert np.all(np.isfinite(chosen)) and np.max(np.abs(ref["pos"] - chosen)) <= float(g["ref_err_max"])


@pytest.mark.parametrize("name", ["h_ring6", "z_tall6"])
def test_the_statement_without_weights_is_pos3_ref(name):
    g = pos3_golden.load(name)
    free_z = pos3_golden.free_z(g)
    cols = (g["group_ptr"], pos3_golden.dense(g, g["rx0"]), pos3_golden.dense(g, g["rx1"]), g["tdoa"], g["snr"], g["rx_xyz"],
            pos3_ref.FREE_Z if free_z else pos3_ref.KNOWN_HEIGHT)
    shared = dict(group_h=None if free_z else g["group_h"], x0=(0.1, 0.1, float(g["z0"]) if free_z else 0.0),
                  z_range=tuple(g["z_range"].tolist()) if free_z and len(g["z_range"]) else None)
    want, got = pos3_ref.pos3_ref_groups(*cols, **shared), posq3_ref.posq3_ref(*cols, **shared)
    for key in ("pos", "dop", "hdop", "vdop", "snr", "status", "iters"):
        assert got[key].tobytes() == want[key].tobytes(), key
    assert np.ascontiguousarray(got["rms"][:, 0]).tobytes() == want["rms"].tobytes()
    ones = posq3_ref.posq3_ref(*cols, weights=np.ones(len(cols[1])), **shared)
    assert np.allclose(ones["pos"], got["pos"], rtol=0, atol=1e-9) and not got["flags"].any() and not got["task_ptr"].any()
    ok = (got["dop"] != -1) & (got["status"] == 0)       # (an underdetermined group's A is singular to rounding)
    assert ok.sum() >= len(ok) // 2
    if free_z:      # q's diagonal is what the dops are made of
        assert np.allclose(np.sqrt(got["q"][ok, 0] + got["q"][ok, 2] + got["q"][ok, 5]), got["dop"][ok], rtol=1e-9)
    else:
        assert np.all(got["q"][:, 3:] == 0.0) and np.allclose(np.sqrt(got["q"][ok, 0] + got["q"][ok, 2]), got["dop"][ok], rtol=1e-9)


def test_q_is_the_inverse_and_a_zero_weight_sum_is_nonfinite():
    rng = np.random.default_rng(1)
    for n in (2, 3):
        b = rng.normal(size=(6, n))
        a = b.T @ b
        q, inv = posq3_ref.q_of(a), np.linalg.inv(a)
        want = [inv[0, 0], inv[0, 1], inv[1, 1]] + ([inv[0, 2], inv[1, 2], inv[2, 2]] if n == 3 else [0.0] * 3)
        np.testing.assert_allclose(q, want, rtol=1e-10)
    assert np.all(np.isnan(posq3_ref.q_of(np.zeros((3, 3))))) and np.isnan(posq3_ref.q_of(np.zeros((2, 2)))[:3]).all()
    table = [[0.0, 0.0, 5.0], [100.0, 0.0, 9.0], [0.0, 100.0, 7.0], [90.0, 90.0, 30.0]]
    none = posq3_ref.solve_task([0, 0, 1, 2], [1, 2, 3, 3], [1e-9, 2e-9, 3e-9, 1e-9], table, posq3_ref.FREE_Z, weights=np.zeros(4),
                                x0=(0.1, 0.1, 1.0))
    assert none["status"] == 4 and none["iters"] == 0
    assert pos3_ref.evaluate is posq3_ref.pos3_ref.evaluate and pos3_ref.evaluate.__module__ == "pos3_ref"      # put back


def _records():
    res = np.zeros(3, dtype=pos_3d_quality.QUALITY3_DTYPE)
    res["group_id"], res["timestamp"], res["tx"] = [7, 8, 11], [1700000012.25, 1.5, 2.75], 3
    for k, name in enumerate(pos_3d_quality.QUALITY3_DTYPE["names"][3:17]):
        res[name] = [0.1 * (k + 1), 1e-5 / (k + 1), 12.5 * (k + 1)]
    res["n_rx"], res["n_rows"], res["excluded"], res["flags"] = [6, 5, 6], [15, 10, 15], [-1, 21, -1], [0, 3, 5]
    return res


def test_posq3_file_round_trip_and_its_posq_companion(tmp_path):
    res = _records()
    text = io.StringIO()
    pos_3d_quality.save_quality3(text, res)
    lines = text.getvalue().splitlines()
    assert len(lines) == 3 and len(lines[1].split()) == 21 == len(pos_3d_quality.QUALITY3_DTYPE["names"])
    assert lines[1].split()[:3] == ["8", "1.500000", "3"] and lines[1].split()[-4:] == ["5", "10", "21", "3"]
    assert lines[0].split()[3] == repr(0.1)
    path = tmp_path / "data.posq3"
    pos_3d_quality.save_quality3(str(path), res)
    assert path.read_text() == text.getvalue()
    back = pos_3d_quality.load_quality3(str(path))
    assert back.dtype == res.dtype and back.tolist() == res.tolist()
    assert len(pos_3d_quality.load_quality3(io.StringIO("# nothing\n\n"))) == 0
    with pytest.raises(ValueError, match="21"):
        pos_3d_quality.load_quality3(io.StringIO("7 1.0 3 0.5 20.0 17.25 1.0\n"))
    # the horizontal part as a .posq file: pos_quality reads it, dop is hdop, and track takes its variances from it
    flat = tmp_path / "data.posq"
    pos_quality.save_quality(str(flat), pos_3d_quality.horizontal(res))
    held = pos_quality.load_quality(str(flat))
    assert held.dtype.names == pos_quality.QUALITY_DTYPE["names"] and len(flat.read_text().splitlines()[0].split()) == 17
    np.testing.assert_array_equal(held["dop"], res["hdop"])
    for name in ("group_id", "timestamp", "tx", "snr", "x", "y", "rms", "xdop", "ydop", "major", "minor", "angle", "n_rx", "n_rows",
                 "excluded", "flags"):
        np.testing.assert_array_equal(held[name], res[name], err_msg=name)
    rx, ry, valid = track.measurement_columns(held, 2.0)
    assert valid.tolist() == [True, True, False]        # the third carries NO_CANDIDATE
    np.testing.assert_array_equal(rx, (2.0 * res["xdop"]) ** 2)
    np.testing.assert_array_equal(ry, (2.0 * res["ydop"]) ** 2)


def test_records_take_zdop_and_the_horizontal_ellipse_from_q():
    q = np.array([[4.0, 0.0, 1.0, 0.3, -0.2, 9.0], [2.5, 1.5, 2.5, 0.0, 0.0, 0.0], [np.nan] * 6])
    out = {"status": np.array([0, 3, 2], np.int32), "q": q, "pos": np.arange(9.0).reshape(3, 3)}
    for k, name in enumerate(("dop", "hdop", "vdop", "snr", "rms")):
        out[name] = np.array([1.0, 2.0, 3.0]) + k
    for name in ("n_rx", "n_rows", "excluded", "flags"):
        out[name] = np.array([6, 5, 6], np.int32)
    rows = np.zeros(1, dtype=tdoa_est.TDOA_DTYPE)
    groups = [tdoa_est.TdoaGroup(10 + k, 1.5 * k, 7, rows) for k in range(3)]
    res = pos_3d_quality.records(groups, out)
    assert res["group_id"].tolist() == [10, 11, 12] and res["z"].tolist() == [2.0, 5.0, 8.0]
    np.testing.assert_allclose(res["zdop"][:2], [3.0, 0.0])
    np.testing.assert_allclose([res[n][0] for n in ("xdop", "ydop", "major", "minor", "angle")], posq_ref.ellipse(q[0, :3]))
    np.testing.assert_allclose([res[n][1] for n in ("xdop", "ydop", "major", "minor", "angle")], [np.sqrt(2.5), np.sqrt(2.5), 2.0, 1.0, 45.0])
    assert all(np.isnan(res[n][2]) for n in ("xdop", "ydop", "zdop", "major", "minor", "angle"))
    assert pos_3d_quality.format_summary is pos_quality.format_summary


def test_dropped_groups_print_pos_3ds_sentence(capsys):
    out = {"status": np.array([1, 0, 4], np.int32), "q": np.ones((3, 6)), "pos": np.zeros((3, 3))}
    for name in ("dop", "hdop", "vdop", "snr", "rms", "n_rx", "n_rows", "excluded", "flags"):
        out[name] = np.zeros(3)
    rows = np.zeros(1, dtype=tdoa_est.TDOA_DTYPE)
    res = pos_3d_quality.records([tdoa_est.TdoaGroup(10 + k, 0.0, 7, rows) for k in range(3)], out)
    assert res["group_id"].tolist() == [11]
    assert capsys.readouterr().out.splitlines() == ["Failed to estimate group #10: Underdetermined", "Failed to estimate group #12: Nonfinite"]


def test_command_line_options(tmp_path):
    parser = pos_3d_quality._parser()
    (tmp_path / "data.tdoa").write_text("")
    (tmp_path / "pos-rx.cfg").write_text("")
    files = [str(tmp_path / "data.tdoa"), "-r", str(tmp_path / "pos-rx.cfg"), "-o", "-"]
    assert parser.get_default("tdoa") == "data.tdoa" and parser.get_default("output") == "data.posq3"
    assert parser.get_default("rx_pos") == "pos-rx.cfg" and parser.get_default("gate_m") is None
    assert (parser.get_default("ratio"), parser.get_default("min_rx"), parser.get_default("weights")) == (0.5, None, None)
    assert {s for a in parser._actions for s in a.option_strings} >= {
        "-o", "--output", "-r", "--rx-coordinates", "--height", "--height-tx", "--free-z", "--z0", "--z-range", "--weights", "--exclude",
        "--ratio", "--min-rx", "--pos", "--posq"}
    args = parser.parse_args(files + ["--height", "1.5", "--height-tx", "7=2.5", "8=3", "--exclude", "3", "--min-rx", "6", "--ratio", "0.4",
                                      "--weights", "snr"])
    assert (args.height, args.height_tx, args.gate_m, args.min_rx, args.ratio, args.weights) == (1.5, [[(7, 2.5), (8, 3.0)]], 3.0, 6, 0.4, "snr")
    args = parser.parse_args(files + ["--free-z", "--z0", "-2", "--z-range", "-20", "100"])
    assert args.free_z and args.z0 == -2.0 and args.z_range == [-20.0, 100.0] and args.height is None
    for bad in (["--weights", "energy", "--free-z"], [], ["--height", "1", "--free-z"], ["--height", "1", "--height-tx", "7"]):
        with pytest.raises(SystemExit):
            parser.parse_args(files + bad)
    assert pos_3d_quality.QUALITY3_DTYPE["names"] == (
        "group_id", "timestamp", "tx", "dop", "hdop", "vdop", "snr", "x", "y", "z", "rms", "xdop", "ydop", "zdop", "major", "minor",
        "angle", "n_rx", "n_rows", "excluded", "flags")


def test_the_command_line_refuses_bad_options_before_the_library_is_loaded(tmp_path, monkeypatch, capsys):
    def no_library():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_native, "load_library", no_library)
    g = posq3_golden.load("h_fault6")
    rows = np.zeros(15, dtype=tdoa_est.TDOA_DTYPE)
    for name in ("rx0", "rx1", "tdoa", "snr"):
        rows[name] = g[name][:15]
    tdoa, cfg, out = tmp_path / "data.tdoa", tmp_path / "pos-rx.cfg", tmp_path / "data.posq3"
    tdoa_est.save_tdoa_groups(str(tdoa), [tdoa_est.TdoaGroup(100, 1.0, 7, rows)])
    cfg.write_text("".join("%d: %r %r %r\n" % (r, float(x), float(y), float(z)) for r, (x, y, z) in zip(g["rx_ids"], g["rx_xyz"])))
    base = [str(tdoa), "-r", str(cfg), "-o", str(out)]
    assert pos_3d_quality._main(base + ["--height", "1.0", "--ratio", "1.5"]) == 1
    assert "ratio" in capsys.readouterr().err and out.read_text() == ""
    assert pos_3d_quality._main(base + ["--free-z", "--min-rx", "5"]) == 1
    assert "min_rx must lie in 6" in capsys.readouterr().err
    assert pos_3d_quality._main(base + ["--height", "1.0", "--min-rx", "4"]) == 1
    assert "min_rx must lie in 5" in capsys.readouterr().err
    for bad in (["--free-z", "--height-tx", "7=1.0"], ["--height", "1.0", "--z0", "2.0"]):
        with pytest.raises(SystemExit):
            pos_3d_quality._main(base + bad)
    capsys.readouterr()
