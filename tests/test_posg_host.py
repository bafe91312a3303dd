"""Host side of `thr_posg` (no GPU): the wiring into the header, the symbol list and the build; the NumPy statement
(tests/posg_ref.py) against the fixtures (tests/golden/make_golden_posg.py); what is refused before the library is
loaded; the receiver-id mapping; the .posg text format and `--pos`; the command line on a mocked `_native.posg`; the
tie rule on a constant surface."""
import io
import os
import re

import numpy as np
import pytest

import pos_ref
import posg_golden
import posg_ref
from thrifty_amd import _native, build, pos_est, pos_global, tdoa_est

ROOT = posg_golden.ROOT


def test_thr_posg_is_declared_listed_and_built():
    header = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
    assert re.search(r"\bint thr_posg\(int device_id, size_t n_groups, const int64_t\* group_ptr,", header)
    assert re.search(r"\bint thr_posg_fetch\(thr_posg_result\* result, int which, void\* dst, size_t dst_bytes\);", header)
    assert "void thr_posg_free(thr_posg_result* result);" in header and "int thr_debug_posg_times(double* ms_out" in header
    assert "#define THR_ABI_VERSION 11" in header and _native.ABI_VERSION == 11
    within = header[header.index("within 11, a pure addition"):header.index("#define THR_ABI_VERSION")]
    assert re.search(r"\+ thr_posg / thr_posg_fetch / thr_posg_free / thr_debug_posg_times", within)
    for name, (index, _, _) in _native.POSG_OUTPUTS.items():
        assert re.search(r"#define THR_POSG_%s %d\b" % (name.upper(), index), header), name
    assert "#define THR_POSG_N_OUTPUTS %d" % len(_native.POSG_OUTPUTS) in header
    for name in ("MOVED", "AMBIGUOUS", "NO_MINIMUM"):
        assert "#define THR_POSG_%s %d" % (name, getattr(_native, "POSG_" + name)) in header
        assert getattr(pos_global, name) == getattr(_native, "POSG_" + name) == getattr(posg_ref, name)
    assert "#define THR_POSG_NO_TASK (%d)" % _native.POSG_NO_TASK in header and posg_ref.NO_TASK == _native.POSG_NO_TASK
    assert "#define THR_POSG_ROW_CHUNK %d " % _native.POSG_ROW_CHUNK in header
    assert {"thr_posg", "thr_posg_fetch", "thr_posg_free", "thr_debug_posg_times"} <= set(_native.EXPORTS)
    assert [f[0] for f in _native.ThrPosgOpts._fields_] == ["max_iter", "grid", "starts", "x0", "margin_m", "merge_m", "ratio",
                                                           "floor_m", "map_first", "map_count"]
    assert [f[0] for f in _native.ThrPosgCounts._fields_] == ["groups", "rows", "tasks", "starts", "grid", "map_groups"]
    assert "posg.hip" in build.SOURCES and build.UNPROFILED_POSG == ("posg.hip",)
    assert build.PER_FILE_FLAGS["posg.hip"] == ["-ffp-contract=off"]
    source = open(os.path.join(build.CSRC, "posg.hip")).read()
    assert '#include "pos_lm.hpp"' in source and "#pragma clang fp contract(off)" in source
    assert "solve_team<false, kRegRows>" in source and "AllRows{}" in source
    assert "atomicAdd" not in source and "atomicCAS" not in source and "hipMalloc(" not in source
    assert int(re.search(r"constexpr int kRegRows = (\d+);", source).group(1)) == _native.POS_REGISTER_ROWS
    assert int(re.search(r"constexpr int kDistRx = (\d+);", source).group(1)) == _native.POSG_DIST_RECEIVERS


def test_the_built_library_exports_thr_posg():
    assert os.path.exists(_native.LIB_PATH), "the library is not built: python -m thrifty_amd.build"
    lib = _native.load_library()
    assert lib.thr_posg and lib.thr_posg_fetch and lib.thr_posg_free and lib.thr_debug_posg_times


def test_csrc_hash_does_not_see_the_new_file(monkeypatch):
    with_posg = build.csrc_hash()
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "posg.hip"])
    assert build.csrc_hash() == with_posg
    monkeypatch.undo()
    monkeypatch.setattr(build, "UNPROFILED_POSG", ())
    assert build.csrc_hash() != with_posg


def _ref(g, **kw):
    return posg_ref.posg_ref(*posg_golden.columns(g), **dict(posg_golden.options(g), **kw))


@pytest.fixture(scope="module")
def statements():
    return {name: _ref(posg_golden.load(name)) for name in posg_golden.SETS}


def test_fixtures_are_small_and_hold_the_scenes_of_the_issue():
    for name in posg_golden.SETS:
        assert os.path.getsize(os.path.join(posg_golden.GOLDEN, name + ".npz")) <= 64 * 1024
        g = posg_golden.load(name)
        seed, n_rx, n_groups, noise, outside, offset, floor_m = posg_golden.SCENES[name]
        assert 24 <= len(g["group_id"]) == n_groups <= 40 and len(g["rx_ids"]) == n_rx and float(g["floor_m"]) == floor_m
        assert set(np.diff(g["group_ptr"]).tolist()) == {n_rx * (n_rx - 1) // 2}
        centre = g["rx_xy"].mean(axis=0) - offset
        assert np.hypot(*centre) < 10.0 and np.all(np.abs(np.hypot(*(g["rx_xy"] - offset).T) - 100.0) < 20.0)
        radius = np.hypot(*(g["planted"] - offset).T)
        assert np.all(radius >= 120.0) and np.all(radius <= 300.0) if outside else np.all(radius <= 60.0)
        assert float(g["margin_m"]) == posg_golden.margin_of(g["rx_xy"])
        assert (int(g["grid"]), int(g["starts"]), float(g["merge_m"]), float(g["ratio"])) == (32, 4, 1.0, 2.0)


@pytest.mark.parametrize("name", posg_golden.SETS)
def test_the_statement_gives_what_the_fixture_records(name, statements):
    g, ref = posg_golden.load(name), statements[name]
    recorded = {key: g["ref_" + key] for key in posg_golden.RECORDED}
    posg_golden.assert_same_discrete_outputs(ref, recorded, g["ref_order_safe"])
    safe = g["ref_order_safe"]
    assert ref["start_f"].tobytes() == g["ref_start_f"].tobytes()       # the surface is elementwise float64: the same bits
    ok = ref["task_status"] == pos_ref.OK
    assert np.max(np.abs(ref["task_pos"][ok] - g["ref_task_pos"][ok])) < 1e-6      # NumPy's sums may differ between builds
    assert np.all(safe) or name == "three_out"


def test_the_claims_of_the_issue_hold_on_the_statement(statements):
    for name in ("far4", "far8"):
        g, ref = posg_golden.load(name), statements[name]
        fixed = np.hypot(*(ref["task_pos"][:, 0] - g["planted"]).T)
        assert np.count_nonzero(fixed > 10.0) == int(g["lost_by_the_fixed_start"]) >= 4
        assert np.all(np.hypot(*(ref["pos"] - g["planted"]).T) < (2.0 if name == "far4" else 20.0))
        np.testing.assert_array_equal((ref["flags"] & posg_ref.MOVED) != 0, fixed > 10.0)
    three = statements["three_out"]
    assert np.count_nonzero(three["flags"] & posg_ref.AMBIGUOUS) >= 5
    both = (three["flags"] & posg_ref.AMBIGUOUS) != 0
    assert np.all(three["n_minima"][both] >= 2) and np.all(np.hypot(*(three["pos"][both] - three["pos2"][both]).T) > 1.0)
    clean = statements["clean6"]
    assert not np.any(clean["flags"]) and np.all(clean["n_minima"] == 1)
    assert np.all(np.isnan(clean["rms2"])) and np.all(np.isnan(clean["pos2"]))


def test_the_cell_centres_are_the_header_expression():
    table = np.array([[5000.0, -3000.0], [5100.0, -2950.0], [4990.0, -3100.0]])
    cx, cy = posg_ref.centres(table, 37.5, 16)
    lo0, hi0 = 4990.0 - 37.5, 5100.0 + 37.5
    assert cx.tolist() == [lo0 + (i + 0.5) * ((hi0 - lo0) / 16) for i in range(16)]
    assert cy[0] == (-3100.0 - 37.5) + 0.5 * ((-2950.0 + 37.5 - (-3100.0 - 37.5)) / 16)
    mine = pos_global.cell_centres(table, 37.5, 16)
    assert mine[0].tobytes() == cx.tobytes() and mine[1].tobytes() == cy.tobytes()


def test_the_surface_is_a_sequential_sum_and_finite_on_a_receiver():
    table = np.array([[0.0, 0.0], [100.0, 0.0], [0.0, 100.0]])
    rx0, rx1, tdoa = [0, 0, 1], [1, 2, 2], [1e-7, -2e-7, 3e-8]
    cx, cy = np.array([0.0, 50.0]), np.array([0.0, 25.0])          # cell (0, 0) sits on receiver 0
    F = posg_ref.surface(rx0, rx1, tdoa, table, cx, cy)
    assert np.all(np.isfinite(F)) and F.shape == (2, 2)
    acc = 0.0
    for a, b, t in zip(rx0, rx1, tdoa):
        da = np.sqrt((table[a, 0] - 50.0) * (table[a, 0] - 50.0) + (table[a, 1] - 25.0) * (table[a, 1] - 25.0))
        db = np.sqrt((table[b, 0] - 50.0) * (table[b, 0] - 50.0) + (table[b, 1] - 25.0) * (table[b, 1] - 25.0))
        res = t * pos_ref.C - (da - db)
        acc += res * res
    assert F[1, 1] == acc


def test_the_tie_rule_on_a_constant_surface_and_with_nans():
    flat = np.full((16, 16), 3.0)
    minima = posg_ref.local_minima(flat)
    assert minima.sum() == 1 and minima[0, 0]                       # only cell 0 has no equal neighbour below it
    cells, f = posg_ref.lowest(flat, minima, 4)
    assert cells.tolist() == [0, -1, -1, -1] and f[0] == 3.0 and np.all(np.isnan(f[1:]))
    two = flat.copy()
    two[5, 7] = two[9, 2] = 1.0                                     # equal F: the lower cell first
    cells, _ = posg_ref.lowest(two, posg_ref.local_minima(two), 2)
    assert cells.tolist() == [5 * 16 + 7, 9 * 16 + 2]
    plateau = flat.copy()
    plateau[4, 4] = plateau[4, 5] = 1.0                             # two equal neighbours: the lower cell alone
    assert np.flatnonzero(posg_ref.local_minima(plateau).ravel()).tolist() == [0, 4 * 16 + 4]
    corner = flat.copy()
    corner[15, 15], corner[0, 9] = 0.5, 0.25                        # corner and edge cells can be minima
    assert np.flatnonzero(posg_ref.local_minima(corner).ravel()).tolist() == [0, 9, 255]
    nan = flat.copy()
    nan[3, 3], nan[2, 2] = np.nan, 1.0                              # a NaN is no minimum and keeps its neighbours from being one
    assert np.flatnonzero(posg_ref.local_minima(nan).ravel()).tolist() == [0]
    assert not posg_ref.local_minima(np.full((16, 16), np.inf)).any()


def test_the_choice_rule():
    pos = np.array([[0.0, 0.0], [10.0, 0.0], [10.0, 0.5], [50.0, 0.0], [np.nan, np.nan]])
    rms = np.array([3.0, 1.0, 1.0, 1.5, np.nan])
    status = np.array([0, 0, 0, 0, posg_ref.NO_TASK])
    got = posg_ref.pick(pos, rms, status, 1.0, 2.0, 0.0)
    assert got["task"] == 1 and got["n_minima"] == 3 and got["duplicate"].tolist() == [False, False, True, False, False]
    assert got["pos2"].tolist() == [50.0, 0.0] and got["rms2"] == 1.5 and got["flags"] == posg_ref.MOVED | posg_ref.AMBIGUOUS
    assert posg_ref.pick(pos, rms, status, 1.0, 1.2, 0.0)["flags"] == posg_ref.MOVED                 # 1.5 > 1.2 x 1.0
    assert posg_ref.pick(pos, rms, status, 1.0, 1.2, 1.5)["flags"] == posg_ref.MOVED | posg_ref.AMBIGUOUS   # ... but within the floor
    assert posg_ref.pick(pos, rms, status, 0.4, 2.0, 0.0)["n_minima"] == 4                           # 0.5 m apart > merge_m
    none = posg_ref.pick(pos, rms, np.array([3, 2, 2, 4, posg_ref.NO_TASK]), 1.0, 2.0, 0.0)
    assert none["flags"] == posg_ref.NO_MINIMUM | posg_ref.MOVED and none["task"] == 0 and none["n_minima"] == 0
    assert none["pos"].tolist() == [0.0, 0.0] and np.isnan(none["rms2"])
    only0 = posg_ref.pick(pos, rms, np.array([0, 2, 2, 2, posg_ref.NO_TASK]), 1.0, 2.0, 0.0)
    assert only0["flags"] == 0 and only0["task"] == 0 and only0["n_minima"] == 1
    lost0 = posg_ref.pick(pos, rms, np.array([3, 0, 0, 0, posg_ref.NO_TASK]), 1.0, 2.0, 0.0)
    assert lost0["flags"] & posg_ref.MOVED and lost0["task"] == 1


def _no_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_native, "load_library", no_library)


def test_bad_inputs_are_refused_before_the_library_is_loaded(monkeypatch):
    _no_library(monkeypatch)
    flat = {k: np.array(xy) for k, xy in enumerate([(0.0, 0.0), (100.0, 0.0), (0.0, 100.0)])}
    args = ([0, 3], [0, 0, 1], [1, 2, 2], [1e-9, 2e-9, 3e-9], [1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="3-D"):
        pos_global.global_columns(*args, {k: np.append(v, 1.0) for k, v in flat.items()})
    with pytest.raises(ValueError, match="1-D"):
        pos_global.global_columns([0, 1], [0], [1], [1e-9], [1.0], {0: np.array([0.0]), 1: np.array([50.0])})
    with pytest.raises(ValueError, match="empty"):
        pos_global.global_columns(*args, {})
    with pytest.raises(KeyError):
        pos_global.global_columns(*args, {0: flat[0], 1: flat[1], 7: flat[2]})
    with pytest.raises(ValueError, match="group_ptr"):
        pos_global.global_columns([0, 2], *args[1:], flat)
    for grid in (0, 8, 33, 128):
        with pytest.raises(ValueError, match="grid"):
            pos_global.global_columns(*args, flat, grid=grid)
    for starts in (0, 9, 2.5):
        with pytest.raises(ValueError, match="starts"):
            pos_global.global_columns(*args, flat, starts=starts)
    for margin in (0.0, -1.0, 10000.5, np.inf, np.nan):
        with pytest.raises(ValueError, match="margin_m"):
            pos_global.global_columns(*args, flat, margin_m=margin)
    with pytest.raises(ValueError, match="margin_m"):                # the default: a bounding box without extent
        pos_global.global_columns(*args, {k: np.array([1.0, 2.0]) for k in range(3)})
    for merge in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="merge_m"):
            pos_global.global_columns(*args, flat, merge_m=merge)
    for ratio in (0.5, 0.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="ratio"):
            pos_global.global_columns(*args, flat, ratio=ratio)
    for floor in (-0.1, np.inf, np.nan):
        with pytest.raises(ValueError, match="floor_m"):
            pos_global.global_columns(*args, flat, floor_m=floor)
    with pytest.raises(ValueError, match="max_iter"):
        pos_global.global_columns(*args, flat, max_iter=-1)
    for first, count in ((0, 2), (1, 1), (-1, 1), (0, 257), (0, -1)):
        with pytest.raises(ValueError, match="map"):
            pos_global.global_columns(*args, flat, map_first=first, map_count=count)
    with pytest.raises(ValueError, match="x0"):
        pos_global.global_columns(*args, flat, x0=(0.0, np.nan))
    rows = np.zeros(3, dtype=tdoa_est.TDOA_DTYPE)
    rows["rx0"], rows["rx1"] = args[1], args[2]
    with pytest.raises(ValueError, match="ratio"):
        pos_global.solve([tdoa_est.TdoaGroup(1, 2.0, 3, rows)], flat, ratio=0.9)
    with pytest.raises(ValueError, match="no group"):
        pos_global.surface([tdoa_est.TdoaGroup(1, 2.0, 3, rows)], flat, 2)


def _mock_posg(monkeypatch, g, seen):
    """`_native.posg` answered by the statement; the call's arguments are kept in `seen`."""
    def posg(ptr, rx0, rx1, tdoa, snr, table, margin_m, grid=32, starts=4, merge_m=1.0, ratio=2.0, floor_m=0.0, map_first=0,
             map_count=0, x0=(0.1, 0.1), max_iter=100, outputs=None, device_id=0):
        seen.append(dict(rx0=np.array(rx0), rx1=np.array(rx1), table=np.array(table), margin_m=margin_m, grid=grid, starts=starts,
                         merge_m=merge_m, ratio=ratio, floor_m=floor_m, map_first=map_first, map_count=map_count))
        ref = posg_ref.posg_ref(ptr, rx0, rx1, tdoa, snr, table, margin_m, grid, starts, merge_m, ratio, floor_m, x0, max_iter)
        out = {name: ref[name] for name in _native.POSG_OUTPUTS}
        out["map"], out["map_min"] = ref["map"][map_first:map_first + map_count], ref["map_min"][map_first:map_first + map_count]
        counts = dict(groups=len(ptr) - 1, rows=len(rx0), tasks=starts + 1, starts=starts, grid=grid, map_groups=map_count)
        return counts, out
    monkeypatch.setattr(_native, "posg", posg)


def test_receiver_ids_are_mapped_to_dense_indices_and_defaults_are_the_conventions(monkeypatch):
    g, seen = posg_golden.load("clean6"), []
    _mock_posg(monkeypatch, g, seen)
    shuffled = {int(r): np.array(g["rx_xy"][k]) for k, r in reversed(list(enumerate(g["rx_ids"])))}     # another insertion order
    n = int(g["group_ptr"][3])
    out = pos_global.global_columns(g["group_ptr"][:4], g["rx0"][:n], g["rx1"][:n], g["tdoa"][:n], g["snr"][:n], shuffled)
    call = seen[0]
    ids = list(shuffled)
    assert [ids[k] for k in call["rx0"]] == g["rx0"][:n].tolist() and [ids[k] for k in call["rx1"]] == g["rx1"][:n].tolist()
    assert call["rx0"].dtype == np.int32 and call["table"].tolist() == [shuffled[i].tolist() for i in ids]
    assert (call["grid"], call["starts"], call["merge_m"], call["ratio"], call["floor_m"], call["map_count"]) == (32, 4, 1.0, 2.0, 0.0, 0)
    assert call["margin_m"] == posg_golden.margin_of(g["rx_xy"]) == out["margin_m"]
    assert out["pos"].shape == (3, 2) and len(out["cx"]) == 32 and out["counts"]["groups"] == 3
    np.testing.assert_array_equal(out["start_cell"], g["ref_start_cell"][:3])


def _records():
    res = np.zeros(3, dtype=pos_global.GLOBAL_DTYPE)
    res["group_id"], res["timestamp"], res["tx"] = [7, 8, 11], [1700000012.25, 1.5, 2.75], 3
    for k, name in enumerate(pos_global.GLOBAL_DTYPE["names"][3:11]):
        res[name] = [0.1 * (k + 1), 1e-5 / (k + 1), -12.5 * (k + 1)]
    res["x2"][0] = res["y2"][0] = res["rms2"][0] = np.nan
    res["n_minima"], res["task"], res["flags"] = [1, 2, 0], [0, 3, 0], [0, 3, 5]
    return res


def test_posg_file_round_trip(tmp_path):
    res = _records()
    text = io.StringIO()
    pos_global.save_global(text, res)
    lines = text.getvalue().splitlines()
    assert len(lines) == 3 and len(lines[1].split()) == 14
    assert lines[1].split()[:3] == ["8", "1.500000", "3"] and lines[1].split()[-3:] == ["2", "3", "3"]
    assert lines[0].split()[0:2] == ["7", "1700000012.250000"] and lines[0].split()[3] == repr(0.1) and lines[0].split()[8] == "nan"
    path = tmp_path / "data.posg"
    pos_global.save_global(str(path), res)
    assert path.read_text() == text.getvalue()
    back = pos_global.load_global(str(path))
    assert back.dtype == res.dtype and back.tobytes() == res.tobytes()
    assert len(pos_global.load_global(io.StringIO("# nothing\n\n"))) == 0
    with pytest.raises(ValueError, match="14"):
        pos_global.load_global(io.StringIO("7 1.0 3 0.5 20.0 17.25 1.0\n"))
    assert pos_global.format_summary(res) == "3 positions, 2 moved, 1 ambiguous, 1 without a minimum, 1.00 minima per position\n"
    assert pos_global.format_summary(res[:0]).startswith("0 positions, 0 moved")


def _write_inputs(tmp_path, g, n_groups):
    groups = []
    for k in range(n_groups):
        a, b = int(g["group_ptr"][k]), int(g["group_ptr"][k + 1])
        rows = np.zeros(b - a, dtype=tdoa_est.TDOA_DTYPE)
        for name in ("rx0", "rx1", "tdoa", "snr"):
            rows[name] = g[name][a:b]
        groups.append(tdoa_est.TdoaGroup(int(g["group_id"][k]), float(g["timestamp"][k]), 7, rows))
    tdoa, cfg = tmp_path / "data.tdoa", tmp_path / "pos-rx.cfg"
    tdoa_est.save_tdoa_groups(str(tdoa), groups)
    cfg.write_text("".join("%d: %r %r\n" % (r, float(x), float(y)) for r, (x, y) in zip(g["rx_ids"], g["rx_xy"])))
    return str(tdoa), str(cfg)


def test_the_command_line_on_a_mocked_device(tmp_path, monkeypatch, capsys):
    g, seen = posg_golden.load("far4"), []
    _mock_posg(monkeypatch, g, seen)
    tdoa, cfg = _write_inputs(tmp_path, g, 8)
    out, pos, npz = tmp_path / "data.posg", tmp_path / "data.pos", tmp_path / "map.npz"
    rc = pos_global._main([tdoa, "-r", cfg, "-o", str(out), "--noise", "0.5", "--ratio", "3", "--pos", str(pos), "--map", "103",
                           "--npz", str(npz)])
    assert rc == 0
    assert (seen[0]["ratio"], seen[0]["floor_m"], seen[0]["grid"], seen[0]["starts"], seen[0]["map_count"]) == (3.0, 0.5, 32, 4, 0)
    assert (seen[1]["map_first"], seen[1]["map_count"]) == (3, 1)
    records = pos_global.load_global(str(out))
    assert records["group_id"].tolist() == g["group_id"][:8].tolist() and np.all(records["tx"] == 7)
    np.testing.assert_array_equal(records["task"], g["ref_task"][:8])
    np.testing.assert_array_equal(records["flags"] & pos_global.MOVED, g["ref_flags"][:8] & pos_global.MOVED)
    np.testing.assert_allclose(np.c_[records["x"], records["y"]], g["ref_pos"][:8], atol=1e-6)
    moved = int(np.count_nonzero(records["flags"] & pos_global.MOVED))
    assert capsys.readouterr().out == "8 positions, %d moved, 0 ambiguous, 0 without a minimum, %.2f minima per position\n" % (
        moved, g["ref_n_minima"][:8].mean())
    positions = pos_est.load_positions(str(pos))                    # `thrifty pos`' format
    assert positions.dtype.names == ("group_id", "timestamp", "tx", "dop", "snr", "x", "y")
    for name in positions.dtype.names:
        assert positions[name].tolist() == records[name].tolist(), name
    with np.load(str(npz)) as saved:
        assert saved["map"].shape == (32, 32) and saved["map_min"].sum() == g["ref_n_local"][3] and len(saved["cx"]) == 32
        np.testing.assert_array_equal(saved["start_cell"], g["ref_start_cell"][3])


def test_the_command_line_options_and_refusals(tmp_path, monkeypatch, capsys):
    parser = pos_global._parser()
    assert parser.get_default("tdoa") == "data.tdoa" and parser.get_default("output") == "data.posg"
    assert parser.get_default("rx_pos") == "pos-rx.cfg" and parser.get_default("margin_m") is None
    assert (parser.get_default("grid"), parser.get_default("starts"), parser.get_default("merge_m"), parser.get_default("ratio"),
            parser.get_default("floor_m")) == (32, 4, 1.0, 2.0, 0.0)
    assert {s for a in parser._actions for s in a.option_strings} >= {
        "-o", "--output", "-r", "--rx-coordinates", "--grid", "--starts", "--margin", "--merge", "--ratio", "--noise", "--pos",
        "--map", "--npz"}
    with pytest.raises(SystemExit):
        parser.parse_args(["--grid", "48"])
    assert pos_global.GLOBAL_DTYPE["names"] == ("group_id", "timestamp", "tx", "dop", "snr", "x", "y", "rms", "x2", "y2", "rms2",
                                                "n_minima", "task", "flags")
    _no_library(monkeypatch)
    tdoa, cfg = _write_inputs(tmp_path, posg_golden.load("far4"), 2)
    out = tmp_path / "data.posg"
    assert pos_global._main([tdoa, "-r", cfg, "-o", str(out), "--ratio", "0.5"]) == 1
    assert "ratio" in capsys.readouterr().err and out.read_text() == ""
    assert pos_global._main([tdoa, "-r", cfg, "-o", str(out), "--map", "100"]) == 1
    assert "--npz" in capsys.readouterr().err
    assert pos_global._main([tdoa, "-r", cfg, "-o", str(out), "--margin", "20000"]) == 1
    assert "margin_m" in capsys.readouterr().err


def test_dropped_groups_print_the_sentence_of_pos_est(monkeypatch, capsys):
    g, seen = posg_golden.load("clean6"), []
    _mock_posg(monkeypatch, g, seen)
    a, b = int(g["group_ptr"][0]), int(g["group_ptr"][1])
    rows = np.zeros(b - a, dtype=tdoa_est.TDOA_DTYPE)
    for name in ("rx0", "rx1", "tdoa", "snr"):
        rows[name] = g[name][a:b]
    bad = rows.copy()
    bad["tdoa"][1] = np.nan
    two = rows[:1].copy()                                           # one pair: two receivers
    res = pos_global.solve([tdoa_est.TdoaGroup(5, 1.0, 7, rows), tdoa_est.TdoaGroup(6, 2.0, 7, bad), tdoa_est.TdoaGroup(9, 3.0, 7, two)],
                           posg_golden.rx_pos(g))
    assert capsys.readouterr().out == "Failed to estimate group #6: Nonfinite\nFailed to estimate group #9: Underdetermined\n"
    assert res["group_id"].tolist() == [5] and res["flags"].tolist() == [0]
