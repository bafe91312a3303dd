"""Host side of `thr_posg3` (no GPU): the wiring into the header, the symbol list and the build; the NumPy statement
(tests/posg3_ref.py) against the fixtures (tests/golden/make_golden_posg3.py) and the claims they were drawn for; the
rules in three coordinates; what is refused before the library is loaded; the default z_grid; the .posg3 text format
and `--pos`; the command line on a mocked `_native.posg3`."""
import io
import json
import os
import re

import numpy as np
import pytest

import pos3_ref
import pos_ref
import posg3_golden
import posg3_ref
import posg_ref
from thrifty_amd import _native, build, pos_3d_global, pos_est, tdoa_est

ROOT = posg3_golden.ROOT


def test_thr_posg3_is_declared_listed_and_built():
    header = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
    assert re.search(r"\bint thr_posg3\(int device_id, size_t n_groups, const int64_t\* group_ptr,", header)
    assert re.search(r"\bint thr_posg3_fetch\(thr_posg3_result\* result, int which, void\* dst, size_t dst_bytes\);", header)
    assert "void thr_posg3_free(thr_posg3_result* result);" in header and "int thr_debug_posg3_times(double* ms_out" in header
    assert "#define THR_ABI_VERSION 11" in header and _native.ABI_VERSION == 11
    within = header[header.index("within 11, a pure addition"):header.index("#define THR_ABI_VERSION")]
    assert re.search(r"\+ thr_posg3 / thr_posg3_fetch / thr_posg3_free / thr_debug_posg3_times", within)
    for name, (index, _, _) in _native.POSG3_OUTPUTS.items():
        assert re.search(r"#define THR_POSG3_%s %d\b" % (name.upper(), index), header), name
    assert "#define THR_POSG3_N_OUTPUTS %d" % len(_native.POSG3_OUTPUTS) in header
    for name, (index, kind, _) in _native.POSG_OUTPUTS.items():         # thr_posg's outputs keep their indices and types
        assert _native.POSG3_OUTPUTS[name][:2] == (index, kind), name
    for name in ("MOVED", "AMBIGUOUS", "NO_MINIMUM", "MIRROR"):
        assert "#define THR_POSG3_%s %d" % (name, getattr(_native, "POSG3_" + name)) in header
        assert getattr(pos_3d_global, name) == getattr(_native, "POSG3_" + name) == getattr(posg3_ref, name)
    assert (_native.POSG3_MOVED, _native.POSG3_AMBIGUOUS, _native.POSG3_NO_MINIMUM) == (posg_ref.MOVED, posg_ref.AMBIGUOUS, posg_ref.NO_MINIMUM)
    assert "#define THR_POSG3_NO_TASK (%d)" % _native.POSG3_NO_TASK in header and posg3_ref.NO_TASK == _native.POSG3_NO_TASK
    assert {"thr_posg3", "thr_posg3_fetch", "thr_posg3_free", "thr_debug_posg3_times"} <= set(_native.EXPORTS)
    assert [f[0] for f in _native.ThrPosg3Opts._fields_] == ["max_iter", "grid", "grid_z", "starts", "x0", "margin_m", "merge_m", "ratio",
                                                            "floor_m", "map_first", "map_count"]
    struct = header[header.index("typedef struct thr_posg3_opts {"):header.index("} thr_posg3_opts;")]
    assert re.sub(r"\s+", " ", struct).endswith("int32_t max_iter, grid, grid_z, starts; double x0[3]; double margin_m, merge_m, ratio, "
                                                 "floor_m; int64_t map_first; int32_t map_count; ")
    assert [f[0] for f in _native.ThrPosg3Counts._fields_] == ["groups", "rows", "tasks", "starts", "grid", "grid_z", "map_groups"]
    assert "posg3.hip" in build.SOURCES and build.UNPROFILED_POSG3 == ("posg3.hip",)
    assert build.PER_FILE_FLAGS["posg3.hip"] == ["-ffp-contract=off"]
    source = open(os.path.join(build.CSRC, "posg3.hip")).read()
    assert '#include "pos3_lm.hpp"' in source and "#pragma clang fp contract(off)" in source
    assert "solve_team<FREE_Z, kRegRows>" in source and "atomic" not in source.lower() and "hipMalloc(" not in source
    assert int(re.search(r"constexpr int kRegRows = (\d+);", source).group(1)) == _native.POS3_REGISTER_ROWS
    assert int(re.search(r"constexpr int kDistRx = (\d+);", source).group(1)) == _native.POSG3_DIST_RECEIVERS
    assert int(re.search(r"constexpr int kRowChunk = (\d+);", source).group(1)) == _native.POSG3_ROW_CHUNK
    assert int(re.search(r"constexpr int kMaxGridZ = (\d+);", source).group(1)) == _native.POSG3_MAX_GRID_Z
    assert "(gz < 3 ? gz : 3) * kCells" in source                          # three planes at most, never the volume


def test_the_built_library_exports_thr_posg3():
    assert os.path.exists(_native.LIB_PATH), "the library is not built: python -m thrifty_amd.build"
    lib = _native.load_library()
    assert lib.thr_posg3 and lib.thr_posg3_fetch and lib.thr_posg3_free and lib.thr_debug_posg3_times


def test_csrc_hash_is_the_recorded_one_and_does_not_see_the_new_file(monkeypatch):
    with_posg3 = build.csrc_hash()
    recorded = json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json")))
    assert {workload["_source"]["csrc_sha16"] for workload in recorded.values()} == {with_posg3}
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "posg3.hip"])
    assert build.csrc_hash() == with_posg3
    monkeypatch.undo()
    monkeypatch.setattr(build, "UNPROFILED_POSG3", ())
    assert build.csrc_hash() != with_posg3


def _ref(g, **kw):
    return posg3_ref.posg3_ref(*posg3_golden.columns(g), posg3_golden.mode_of(g), **dict(posg3_golden.options(g), **kw))


@pytest.fixture(scope="module")
def statements():
    return {name: _ref(posg3_golden.load(name)) for name in posg3_golden.SETS}


def test_fixtures_are_small_and_hold_the_scenes_of_the_issue():
    shapes = {"z_lost6": (48, 6, True), "z_mirror6": (32, 6, True), "h_far4": (32, 4, False), "z_tall6g": (24, 6, True)}
    for name in posg3_golden.SETS:
        assert os.path.getsize(os.path.join(posg3_golden.GOLDEN, name + ".npz")) <= 64 * 1024
        g = posg3_golden.load(name)
        n_groups, n_rx, free_z = shapes[name]
        assert len(g["group_id"]) == n_groups <= 64 and len(g["rx_ids"]) == n_rx and bool(g["free_z"]) == free_z
        assert float(g["margin_m"]) == float(np.max(g["rx_xyz"][:, :2].max(axis=0) - g["rx_xyz"][:, :2].min(axis=0)))
        assert (int(g["grid"]), int(g["starts"]), float(g["merge_m"]), float(g["ratio"]), float(g["floor_m"])) == (32, 4, 1.0, 2.0, 0.0)
        assert int(g["grid_z"]) == (8 if free_z else 1) and np.all(g["planted"][:, 2] >= 0.0) and np.all(g["planted"][:, 2] <= 3.0)
        if free_z:
            assert float(g["z0"]) == g["rx_xyz"][:, 2].min() - 1.0
            want = (-10.0, 70.0) if name == "z_mirror6" else pos_3d_global.default_z_grid(g["rx_xyz"])
            assert tuple(g["z_grid"].tolist()) == want == (want if name == "z_mirror6" else posg3_golden.default_z_grid(g["rx_xyz"]))
    lost = posg3_golden.load("z_lost6")
    assert int(lost["uncut"].sum()) == 44 and np.flatnonzero(~lost["uncut"]).tolist() == [5, 6, 20, 33]
    assert sorted(lost["rx_xyz"][:, 2].tolist()) == np.linspace(2.0, 42.0, 6).tolist()
    assert np.all(posg3_golden.load("z_mirror6")["rx_xyz"][:, 2] == 30.0)
    assert sorted(posg3_golden.load("h_far4")["rx_xyz"][:, 2].tolist()) == np.linspace(2.0, 32.0, 4).tolist()
    with np.load(os.path.join(ROOT, "tests", "golden", "pos3", "z_tall6.npz")) as tall:
        assert posg3_golden.load("z_tall6g")["rx_xyz"].tobytes() == tall["rx_xyz"].tobytes()


@pytest.mark.parametrize("name", posg3_golden.SETS)
def test_the_statement_gives_what_the_fixture_records(name, statements):
    g, ref = posg3_golden.load(name), statements[name]
    recorded = {key: g["ref_" + key] for key in posg3_golden.RECORDED}
    posg3_golden.assert_same_discrete_outputs(ref, recorded, g["ref_order_safe"])
    assert ref["start_f"].tobytes() == g["ref_start_f"].tobytes()       # the volume is elementwise float64: the same bits
    ok = ref["task_status"] == pos_ref.OK
    assert np.max(np.abs(ref["task_pos"][ok] - g["ref_task_pos"][ok])) < 1e-6      # NumPy's sums may differ between builds
    assert np.all(g["ref_order_safe"]) or name == "z_mirror6"


def test_the_claims_of_the_issue_hold_on_the_records():
    lost = posg3_golden.load("z_lost6")
    uncut = lost["uncut"]
    far = np.sqrt(np.sum((lost["ref_task_pos"][:, 0] - lost["planted_pos"]) ** 2, axis=1)) > 10.0
    fixed = uncut & ((lost["ref_task_status"][:, 0] != pos_ref.OK) | far)
    assert fixed.sum() == int(lost["lost_by_the_fixed_start"]) >= 5
    rows = np.arange(len(uncut))
    assert np.all(lost["ref_task_status"][rows, lost["ref_task"]][uncut] == pos_ref.OK)
    assert np.all(lost["ref_rms"][uncut] <= lost["planted_rms"][uncut] * (1 + 1e-9))
    assert np.all((lost["ref_flags"][fixed] & posg3_ref.MOVED) != 0)
    assert np.all(lost["ref_flags"][~uncut] == posg3_ref.NO_MINIMUM | posg3_ref.MOVED)
    mirror = posg3_golden.load("z_mirror6")
    both = posg3_ref.AMBIGUOUS | posg3_ref.MIRROR
    marked = (mirror["ref_flags"] & both) == both
    assert marked.sum() >= 16 and not mirror["ref_order_safe"][marked].any()
    mirrored = mirror["ref_pos"] * np.array([1.0, 1.0, -1.0]) + np.array([0.0, 0.0, 60.0])
    assert np.all(np.sqrt(np.sum((mirror["ref_pos2"] - mirrored)[marked] ** 2, axis=1)) <= 1e-6)
    assert np.all(np.abs(mirror["ref_rms2"][marked] - mirror["ref_rms"][marked]) <= 1e-9 * mirror["ref_rms"][marked])
    far4 = posg3_golden.load("h_far4")
    assert int(far4["lost_by_the_fixed_start"]) >= 5 and not np.any(far4["ref_flags"] & (posg3_ref.NO_MINIMUM | posg3_ref.MIRROR))
    assert np.all(far4["ref_rms"] <= far4["planted_rms"] * (1 + 1e-9)) and np.all(far4["ref_pos"][:, 2] == far4["group_h"])
    tall = posg3_golden.load("z_tall6g")
    assert not np.any(tall["ref_flags"]) and np.all(tall["ref_n_minima"] == 1)


def test_the_cell_centres_are_the_header_expression():
    table = np.array([[5000.0, -3000.0, 4.0], [5100.0, -2950.0, 9.0], [4990.0, -3100.0, 30.0]])
    cx, cy, cz = posg3_ref.centres(table, 37.5, 16, (-7.0, 55.0), 5)
    lo0, hi0 = 4990.0 - 37.5, 5100.0 + 37.5
    assert cx.tolist() == [lo0 + (i + 0.5) * ((hi0 - lo0) / 16) for i in range(16)]
    assert cy[0] == (-3100.0 - 37.5) + 0.5 * ((-2950.0 + 37.5 - (-3100.0 - 37.5)) / 16)
    assert cz.tolist() == [-7.0 + (k + 0.5) * ((55.0 - -7.0) / 5) for k in range(5)]
    mine = pos_3d_global.cell_centres(table, 37.5, 16, (-7.0, 55.0), 5)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(mine, (cx, cy, cz)))
    assert posg3_ref.centres(table, 37.5, 16)[2] is None and pos_3d_global.cell_centres(table, 37.5, 16)[2] is None


def test_the_volume_is_a_sequential_sum_and_posgs_surface_on_a_flat_table():
    table = np.array([[0.0, 0.0, 3.0], [100.0, 0.0, 17.0], [0.0, 100.0, 8.0]])
    rx0, rx1, tdoa = [0, 0, 1], [1, 2, 2], [1e-7, -2e-7, 3e-8]
    cx, cy, cz = np.array([0.0, 50.0]), np.array([0.0, 25.0]), np.array([3.0, 11.0])      # cell (0, 0, 0) sits on receiver 0
    F = posg3_ref.volume(rx0, rx1, tdoa, table, cx, cy, cz)
    assert np.all(np.isfinite(F)) and F.shape == (2, 2, 2)
    acc = 0.0
    for a, b, t in zip(rx0, rx1, tdoa):
        va, vb = table[a] - [50.0, 25.0, 11.0], table[b] - [50.0, 25.0, 11.0]
        da = np.sqrt((va[0] * va[0] + va[1] * va[1]) + va[2] * va[2])
        db = np.sqrt((vb[0] * vb[0] + vb[1] * vb[1]) + vb[2] * vb[2])
        res = t * pos_ref.C - (da - db)
        acc += res * res
    assert F[1, 1, 1] == acc
    flat = table.copy()
    flat[:, 2] = 12.5
    lifted = posg3_ref.volume(rx0, rx1, tdoa, flat, cx, cy, [12.5])
    assert lifted[0].tobytes() == posg_ref.surface(rx0, rx1, tdoa, flat[:, :2], cx, cy).tobytes()


def test_the_minimum_rule_in_three_dimensions():
    const = np.full((4, 16, 16), 3.0)
    minima = posg3_ref.local_minima(const)
    assert minima.sum() == 1 and minima[0, 0, 0]                    # only cell 0 has no equal neighbour below it
    cells, f = posg3_ref.lowest(const, minima, 4)
    assert cells.tolist() == [0, -1, -1, -1] and f[0] == 3.0 and np.all(np.isnan(f[1:]))
    two = const.copy()
    two[3, 5, 7] = two[0, 9, 2] = 1.0                               # equal F: the lower cell first; the outer planes can hold minima
    cells, _ = posg3_ref.lowest(two, posg3_ref.local_minima(two), 2)
    assert cells.tolist() == [9 * 16 + 2, 3 * 256 + 5 * 16 + 7]
    column = const.copy()
    column[1, 4, 4] = column[2, 4, 4] = 1.0                         # equal neighbours in two planes: the lower cell alone
    assert np.flatnonzero(posg3_ref.local_minima(column).ravel()).tolist() == [0, 256 + 4 * 16 + 4]
    diagonal = const.copy()
    diagonal[1, 4, 4], diagonal[2, 5, 5] = 1.0, 0.5                 # a lower cell across a corner: 26 neighbours, not 6
    assert np.flatnonzero(posg3_ref.local_minima(diagonal).ravel()).tolist() == [0, 2 * 256 + 5 * 16 + 5]
    nan = const.copy()
    nan[2, 3, 3], nan[1, 2, 2] = np.nan, 1.0                        # a NaN is no minimum and keeps its neighbours from being one
    assert np.flatnonzero(posg3_ref.local_minima(nan).ravel()).tolist() == [0]
    assert not posg3_ref.local_minima(np.full((2, 16, 16), np.inf)).any()
    one = np.full((16, 16), 3.0)
    one[4, 4] = one[4, 5] = 1.0                                     # one plane: posg's rule over 8 neighbours
    np.testing.assert_array_equal(posg3_ref.local_minima(one[None])[0], posg_ref.local_minima(one))


def test_the_choice_rule_and_the_mirror_flag():
    pos = np.array([[0.0, 0.0, 1.0], [10.0, 0.0, 2.0], [10.0, 0.5, 2.0], [10.2, 0.1, 58.0], [np.nan] * 3])
    rms = np.array([3.0, 1.0, 1.0, 1.5, np.nan])
    status = np.array([0, 0, 0, 0, posg3_ref.NO_TASK])
    got = posg3_ref.pick(pos, rms, status, 1.0, 2.0, 0.0, True)
    assert got["task"] == 1 and got["n_minima"] == 3 and got["duplicate"].tolist() == [False, False, True, False, False]
    assert got["pos2"].tolist() == [10.2, 0.1, 58.0] and got["rms2"] == 1.5
    assert got["flags"] == posg3_ref.MOVED | posg3_ref.AMBIGUOUS | posg3_ref.MIRROR      # 0.22 m apart horizontally, 56 m in height
    assert posg3_ref.pick(pos, rms, status, 1.0, 1.2, 0.0, True)["flags"] == posg3_ref.MOVED          # not ambiguous: no mirror either
    assert posg3_ref.pick(pos, rms, status, 0.2, 2.0, 0.0, True)["flags"] == posg3_ref.MOVED | posg3_ref.AMBIGUOUS   # 0.22 m > merge_m
    known = posg3_ref.pick(pos, rms, status, 1.0, 2.0, 0.0, False)      # the height known: the horizontal distance merges, no mirror
    assert known["n_minima"] == 2 and known["duplicate"].tolist() == [False, False, True, True, False]
    assert known["flags"] == posg3_ref.MOVED and known["pos2"].tolist() == [0.0, 0.0, 1.0] and known["rms2"] == 3.0
    flat = posg_ref.pick(pos[:, :2], rms, status, 1.0, 2.0, 0.0)         # ... which is posg's rule word for word
    assert (flat["task"], flat["n_minima"], flat["flags"]) == (known["task"], known["n_minima"], known["flags"])
    none = posg3_ref.pick(pos, rms, np.array([3, 2, 2, 4, posg3_ref.NO_TASK]), 1.0, 2.0, 0.0, True)      # AT_BOUND is not eligible
    assert none["flags"] == posg3_ref.NO_MINIMUM | posg3_ref.MOVED and none["task"] == 0 and none["n_minima"] == 0
    assert none["pos"].tolist() == [0.0, 0.0, 1.0] and np.isnan(none["rms2"])


def _no_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_native, "load_library", no_library)


RX = {k: np.array(xyz) for k, xyz in enumerate([(0.0, 0.0, 2.0), (100.0, 0.0, 12.0), (0.0, 100.0, 7.0), (90.0, 80.0, 22.0)])}
ARGS = ([0, 4], [0, 0, 1, 2], [1, 2, 2, 3], [1e-9, 2e-9, 3e-9, 4e-9], [1.0, 1.0, 1.0, 1.0])


def test_bad_inputs_are_refused_before_the_library_is_loaded(monkeypatch):
    _no_library(monkeypatch)
    columns = pos_3d_global.global3_columns
    for kw in (dict(), dict(height=1.0, free_z=True)):
        with pytest.raises(ValueError, match="no default mode"):
            columns(*ARGS, RX, **kw)
    with pytest.raises(ValueError, match="three coordinates"):
        columns(*ARGS, {k: v[:2] for k, v in RX.items()}, height=1.0)
    with pytest.raises(ValueError, match="empty"):
        columns(*ARGS, {}, height=1.0)
    with pytest.raises(ValueError, match="not finite"):
        columns(*ARGS, {**RX, 3: np.array([1.0, np.nan, 2.0])}, height=1.0)
    with pytest.raises(KeyError):
        columns(*ARGS, {0: RX[0], 1: RX[1], 2: RX[2], 7: RX[3]}, height=1.0)
    with pytest.raises(ValueError, match="group_ptr"):
        columns([0, 2], *ARGS[1:], RX, height=1.0)
    for mode in (dict(height=1.0), dict(free_z=True)):
        for grid in (0, 8, 33, 64):
            with pytest.raises(ValueError, match="grid"):
                columns(*ARGS, RX, grid=grid, **mode)
        for starts in (0, 9, 2.5):
            with pytest.raises(ValueError, match="starts"):
                columns(*ARGS, RX, starts=starts, **mode)
        for margin in (0.0, -1.0, 10000.5, np.inf, np.nan):
            with pytest.raises(ValueError, match="margin_m"):
                columns(*ARGS, RX, margin_m=margin, **mode)
        for merge in (0.0, -1.0, np.inf, np.nan):
            with pytest.raises(ValueError, match="merge_m"):
                columns(*ARGS, RX, merge_m=merge, **mode)
        for ratio in (0.5, 0.0, np.inf, np.nan):
            with pytest.raises(ValueError, match="ratio"):
                columns(*ARGS, RX, ratio=ratio, **mode)
        for floor in (-0.1, np.inf, np.nan):
            with pytest.raises(ValueError, match="floor_m"):
                columns(*ARGS, RX, floor_m=floor, **mode)
        with pytest.raises(ValueError, match="max_iter"):
            columns(*ARGS, RX, max_iter=-1, **mode)
        for first, count in ((0, 2), (1, 1), (-1, 1), (0, 257), (0, -1)):
            with pytest.raises(ValueError, match="map"):
                columns(*ARGS, RX, map_first=first, map_count=count, **mode)
        with pytest.raises(ValueError, match="x0"):
            columns(*ARGS, RX, x0=(0.0, np.nan), **mode)
    with pytest.raises(ValueError, match="margin_m"):                    # the default: a bounding box without horizontal extent
        columns(*ARGS, {k: np.array([1.0, 2.0, float(k)]) for k in range(4)}, height=1.0)
    # the free-z volume
    for grid_z in (0, 1, 33, 2.5):
        with pytest.raises(ValueError, match="grid_z"):
            columns(*ARGS, RX, free_z=True, grid_z=grid_z)
    for z_grid in ((5.0, 5.0), (9.0, 5.0), (np.nan, 5.0), (0.0, np.inf), (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError, match="z_grid must be"):
            columns(*ARGS, RX, free_z=True, z_grid=z_grid)
    for z_grid in ((2.0 - 10e3 - 1.0, 5.0), (0.0, 22.0 + 10e3 + 1.0)):
        with pytest.raises(ValueError, match="leaves the z box"):
            columns(*ARGS, RX, free_z=True, z_grid=z_grid)
    with pytest.raises(ValueError, match="leaves the z box"):
        columns(*ARGS, RX, free_z=True, z_range=(0.0, 40.0), z_grid=(-1.0, 40.0))
    # what pos_3d refuses
    with pytest.raises(ValueError, match="z_range must be"):
        columns(*ARGS, RX, free_z=True, z_range=(5.0, 5.0))
    with pytest.raises(ValueError, match="z0 = "):
        columns(*ARGS, RX, free_z=True, z_range=(0.0, 40.0), z0=50.0)
    with pytest.raises(ValueError, match="z0 must be finite"):
        columns(*ARGS, RX, free_z=True, z0=np.nan)
    with pytest.raises(ValueError, match="mirror plane"):
        columns(*ARGS, {k: np.array([v[0], v[1], 5.0]) for k, v in RX.items()}, free_z=True, z0=5.0)
    for kw in (dict(z0=1.0), dict(z_range=(0.0, 9.0))):
        with pytest.raises(ValueError, match="belong to free_z"):
            columns(*ARGS, RX, height=1.0, **kw)
    for kw in (dict(z_grid=(0.0, 9.0)), dict(grid_z=8)):
        with pytest.raises(ValueError, match="one plane"):
            columns(*ARGS, RX, height=1.0, **kw)
    with pytest.raises(ValueError, match="height must be finite"):
        columns(*ARGS, RX, height=np.inf)
    with pytest.raises(ValueError, match="no height for tx 9"):
        columns(*ARGS, RX, height={3: 1.0}, group_tx=[9])
    rows = np.zeros(4, dtype=tdoa_est.TDOA_DTYPE)
    rows["rx0"], rows["rx1"] = ARGS[1], ARGS[2]
    with pytest.raises(ValueError, match="ratio"):
        pos_3d_global.solve([tdoa_est.TdoaGroup(1, 2.0, 3, rows)], RX, free_z=True, ratio=0.9)
    with pytest.raises(ValueError, match="no group"):
        pos_3d_global.volume([tdoa_est.TdoaGroup(1, 2.0, 3, rows)], RX, 2, height=1.0)


def test_the_default_z_grid_is_the_stated_convention():
    table = np.array([[0.0, 0.0, 2.0], [1.0, 0.0, 42.0], [0.0, 1.0, 10.0]])
    assert pos_3d_global.default_z_grid(table) == (2.0 - 40.0, 42.0 + 40.0)                 # s = the spread
    table[:, 2] = [30.0, 33.0, 31.0]
    assert pos_3d_global.default_z_grid(table) == (30.0 - 10.0, 33.0 + 10.0)                # s = 10 m at least
    table[:, 2] = 30.0
    assert pos_3d_global.default_z_grid(table) == (20.0, 40.0)
    assert pos_3d_global.default_z_grid(table, (1.5, 60.0)) == (1.5, 60.0)                  # z_range where one is given
    assert pos_3d_global.MIN_Z_MARGIN == 10.0


def _mock_posg3(monkeypatch, seen):
    """`_native.posg3` answered by the statement; the call's arguments are kept in `seen`."""
    def posg3(ptr, rx0, rx1, tdoa, snr, table, mode, margin_m, group_h=None, x0=(0.1, 0.1, 0.0), z_range=None, z_grid=None, grid=32,
              grid_z=8, starts=4, merge_m=1.0, ratio=2.0, floor_m=0.0, map_first=0, map_count=0, max_iter=100, outputs=None,
              device_id=0):
        seen.append(dict(rx0=np.array(rx0), rx1=np.array(rx1), table=np.array(table), mode=mode, margin_m=margin_m, group_h=group_h,
                         x0=tuple(x0), z_range=z_range, z_grid=z_grid, grid=grid, grid_z=grid_z, starts=starts, merge_m=merge_m,
                         ratio=ratio, floor_m=floor_m, map_first=map_first, map_count=map_count))
        ref = posg3_ref.posg3_ref(ptr, rx0, rx1, tdoa, snr, table, mode, margin_m, group_h, x0, z_range, z_grid, grid, grid_z, starts,
                                  merge_m, ratio, floor_m, max_iter)
        out = {name: ref[name] for name in _native.POSG3_OUTPUTS}
        out["map"], out["map_min"] = ref["map"][map_first:map_first + map_count], ref["map_min"][map_first:map_first + map_count]
        counts = dict(groups=len(ptr) - 1, rows=len(rx0), tasks=starts + 1, starts=starts, grid=grid, grid_z=grid_z, map_groups=map_count)
        return counts, out
    monkeypatch.setattr(_native, "posg3", posg3)


def test_receiver_ids_are_mapped_to_dense_indices_and_defaults_are_the_conventions(monkeypatch):
    g, seen = posg3_golden.load("z_tall6g"), []
    _mock_posg3(monkeypatch, seen)
    shuffled = {int(r): np.array(g["rx_xyz"][k]) for k, r in reversed(list(enumerate(g["rx_ids"])))}     # another insertion order
    n = int(g["group_ptr"][2])
    out = pos_3d_global.global3_columns(g["group_ptr"][:3], g["rx0"][:n], g["rx1"][:n], g["tdoa"][:n], g["snr"][:n], shuffled, free_z=True)
    call, ids = seen[0], list(shuffled)
    assert [ids[k] for k in call["rx0"]] == g["rx0"][:n].tolist() and [ids[k] for k in call["rx1"]] == g["rx1"][:n].tolist()
    assert call["rx0"].dtype == np.int32 and call["table"].tolist() == [shuffled[i].tolist() for i in ids]
    assert (call["grid"], call["grid_z"], call["starts"], call["merge_m"], call["ratio"], call["floor_m"], call["map_count"]) == (
        32, 8, 4, 1.0, 2.0, 0.0, 0)
    assert call["mode"] == _native.POS3_FREE_Z and call["group_h"] is None and call["z_range"] is None
    assert call["margin_m"] == float(g["margin_m"]) == out["margin_m"] and call["z_grid"] == tuple(g["z_grid"].tolist()) == out["z_grid"]
    assert call["x0"] == (0.1, 0.1, float(g["z0"]))
    assert out["pos"].shape == (2, 3) and len(out["cx"]) == 32 and len(out["cz"]) == 8 and out["counts"]["groups"] == 2
    np.testing.assert_array_equal(out["start_cell"], g["ref_start_cell"][:2])
    pos_3d_global.global3_columns(g["group_ptr"][:3], g["rx0"][:n], g["rx1"][:n], g["tdoa"][:n], g["snr"][:n], shuffled, height={7: 1.5},
                                  group_tx=[7, 7])
    call = seen[1]
    assert call["mode"] == _native.POS3_KNOWN_HEIGHT and call["group_h"].tolist() == [1.5, 1.5]
    assert (call["grid_z"], call["z_grid"], call["z_range"]) == (1, None, None)


def _records():
    res = np.zeros(3, dtype=pos_3d_global.GLOBAL3_DTYPE)
    res["group_id"], res["timestamp"], res["tx"] = [7, 8, 11], [1700000012.25, 1.5, 2.75], 3
    for k, name in enumerate(pos_3d_global.GLOBAL3_DTYPE["names"][3:15]):
        res[name] = [0.1 * (k + 1), 1e-5 / (k + 1), -12.5 * (k + 1)]
    res["x2"][0] = res["y2"][0] = res["z2"][0] = res["rms2"][0] = np.nan
    res["n_minima"], res["task"], res["flags"] = [1, 2, 0], [0, 3, 0], [0, 11, 5]
    return res


def test_posg3_file_round_trip(tmp_path):
    res = _records()
    text = io.StringIO()
    pos_3d_global.save_global3(text, res)
    lines = text.getvalue().splitlines()
    assert len(lines) == 3 and len(lines[1].split()) == 18
    assert lines[1].split()[:3] == ["8", "1.500000", "3"] and lines[1].split()[-3:] == ["2", "3", "11"]
    assert lines[0].split()[0:2] == ["7", "1700000012.250000"] and lines[0].split()[3] == repr(0.1) and lines[0].split()[11] == "nan"
    path = tmp_path / "data.posg3"
    pos_3d_global.save_global3(str(path), res)
    assert path.read_text() == text.getvalue()
    back = pos_3d_global.load_global3(str(path))
    assert back.dtype == res.dtype and back.tobytes() == res.tobytes()
    assert len(pos_3d_global.load_global3(io.StringIO("# nothing\n\n"))) == 0
    with pytest.raises(ValueError, match="18"):
        pos_3d_global.load_global3(io.StringIO("7 1.0 3 0.5 20.0 17.25 1.0\n"))
    assert pos_3d_global.format_summary(res) == ("3 positions, 2 moved, 1 ambiguous (1 of them in height only), 1 without a minimum, "
                                                 "1.00 minima per position\n")
    assert pos_3d_global.format_summary(res[:0]).startswith("0 positions, 0 moved")
    assert pos_3d_global.positions(res, True).dtype.names == ("group_id", "timestamp", "tx", "dop", "snr", "x", "y", "z")
    assert pos_3d_global.positions(res, False).dtype.names == ("group_id", "timestamp", "tx", "dop", "snr", "x", "y")


def _write_inputs(tmp_path, g, n_groups):
    groups = []
    for k in range(n_groups):
        a, b = int(g["group_ptr"][k]), int(g["group_ptr"][k + 1])
        rows = np.zeros(b - a, dtype=tdoa_est.TDOA_DTYPE)
        for name in ("rx0", "rx1", "tdoa", "snr"):
            rows[name] = g[name][a:b]
        groups.append(tdoa_est.TdoaGroup(int(g["group_id"][k]), float(g["timestamp"][k]), int(g["group_tx"][k]), rows))
    tdoa, cfg = tmp_path / "data.tdoa", tmp_path / "pos-rx.cfg"
    tdoa_est.save_tdoa_groups(str(tdoa), groups)
    cfg.write_text("".join("%d: %r %r %r\n" % (r, float(x), float(y), float(z)) for r, (x, y, z) in zip(g["rx_ids"], g["rx_xyz"])))
    return str(tdoa), str(cfg)


def test_the_command_line_on_a_mocked_device(tmp_path, monkeypatch, capsys):
    g, seen = posg3_golden.load("z_mirror6"), []
    _mock_posg3(monkeypatch, seen)
    tdoa, cfg = _write_inputs(tmp_path, g, 4)
    out, pos, npz = tmp_path / "data.posg3", tmp_path / "data.pos", tmp_path / "map.npz"
    rc = pos_3d_global._main([tdoa, "-r", cfg, "-o", str(out), "--free-z", "--z-grid", "-10", "70", "--noise", "0.5", "--pos", str(pos),
                              "--map", "102", "--npz", str(npz)])
    assert rc == 0
    assert (seen[0]["floor_m"], seen[0]["grid"], seen[0]["grid_z"], seen[0]["starts"], seen[0]["map_count"]) == (0.5, 32, 8, 4, 0)
    assert seen[0]["z_grid"] == (-10.0, 70.0) and seen[0]["x0"] == (0.1, 0.1, 29.0) and seen[0]["z_range"] is None
    assert (seen[1]["map_first"], seen[1]["map_count"]) == (2, 1)
    records = pos_3d_global.load_global3(str(out))
    assert records["group_id"].tolist() == g["group_id"][:4].tolist() and np.all(records["tx"] == 7)
    np.testing.assert_array_equal(records["flags"] & ~1, g["ref_flags"][:4] & ~1)
    np.testing.assert_array_equal(records["n_minima"], g["ref_n_minima"][:4])
    mirror = int(np.count_nonzero(records["flags"] & pos_3d_global.MIRROR))
    assert mirror >= 1 and capsys.readouterr().out == "4 positions, %d moved, %d ambiguous (%d of them in height only), 0 without a minimum, %.2f minima per position\n" % (
        np.count_nonzero(records["flags"] & 1), np.count_nonzero(records["flags"] & 2), mirror, records["n_minima"].mean())
    positions = pos_est.load_positions(str(pos))                    # pos_3d's record with z free: 8 columns
    assert positions.dtype.names == ("group_id", "timestamp", "tx", "dop", "snr", "x", "y", "z")
    for name in positions.dtype.names:
        assert positions[name].tolist() == records[name].tolist(), name
    with np.load(str(npz)) as saved:
        assert saved["map"].shape == (8, 32, 32) and saved["map_min"].sum() == g["ref_n_local"][2] and len(saved["cz"]) == 8
        np.testing.assert_array_equal(saved["start_cell"], g["ref_start_cell"][2])
    # the height known: 7 columns, one plane
    far = posg3_golden.load("h_far4")
    tdoa, cfg = _write_inputs(tmp_path, far, 3)
    rc = pos_3d_global._main([tdoa, "-r", cfg, "-o", str(out), "--height", "1.25", "--height-tx", "7=%r" % float(far["group_h"][0]),
                              "--pos", str(pos), "--map", "100", "--npz", str(npz)])
    assert rc == 0 and seen[2]["mode"] == _native.POS3_KNOWN_HEIGHT and seen[2]["group_h"].tolist() == [float(far["group_h"][0])] * 3
    positions = pos_est.load_positions(str(pos))
    assert positions.dtype.names == ("group_id", "timestamp", "tx", "dop", "snr", "x", "y") and len(positions) == 3
    records = pos_3d_global.load_global3(str(out))
    assert np.all(records["z"] == float(far["group_h"][0])) and np.all(records["vdop"] == 0.0)
    np.testing.assert_allclose(np.c_[records["x"], records["y"]][0], far["ref_pos"][0, :2], atol=1e-6)
    with np.load(str(npz)) as saved:
        assert saved["map"].shape == (1, 32, 32) and saved["cz"].tolist() == [float(far["group_h"][0])]


def test_the_command_line_options_and_refusals(tmp_path, monkeypatch, capsys):
    parser = pos_3d_global._parser()
    assert parser.get_default("tdoa") == "data.tdoa" and parser.get_default("output") == "data.posg3"
    assert parser.get_default("rx_pos") == "pos-rx.cfg" and parser.get_default("margin_m") is None
    assert (parser.get_default("grid"), parser.get_default("grid_z"), parser.get_default("starts"), parser.get_default("merge_m"),
            parser.get_default("ratio"), parser.get_default("floor_m")) == (32, None, 4, 1.0, 2.0, 0.0)
    assert {s for a in parser._actions for s in a.option_strings} >= {
        "-o", "--output", "-r", "--rx-coordinates", "--height", "--height-tx", "--free-z", "--z0", "--z-range", "--z-grid", "--grid-z",
        "--grid", "--starts", "--margin", "--merge", "--ratio", "--noise", "--pos", "--map", "--npz"}
    for argv in (["--grid", "64", "--free-z"], [], ["--height", "1", "--free-z"]):
        with pytest.raises(SystemExit):
            parser.parse_args(argv)
    assert pos_3d_global.GLOBAL3_DTYPE["names"] == ("group_id", "timestamp", "tx", "dop", "hdop", "vdop", "snr", "x", "y", "z", "rms", "x2",
                                                   "y2", "z2", "rms2", "n_minima", "task", "flags")
    _no_library(monkeypatch)
    tdoa, cfg = _write_inputs(tmp_path, posg3_golden.load("z_tall6g"), 2)
    out = tmp_path / "data.posg3"
    assert pos_3d_global._main([tdoa, "-r", cfg, "-o", str(out), "--free-z", "--ratio", "0.5"]) == 1
    assert "ratio" in capsys.readouterr().err and out.read_text() == ""
    assert pos_3d_global._main([tdoa, "-r", cfg, "-o", str(out), "--free-z", "--map", "100"]) == 1
    assert "--npz" in capsys.readouterr().err
    assert pos_3d_global._main([tdoa, "-r", cfg, "-o", str(out), "--free-z", "--z-grid", "5", "1"]) == 1
    assert "z_grid" in capsys.readouterr().err
    assert pos_3d_global._main([tdoa, "-r", cfg, "-o", str(out), "--free-z", "--grid-z", "40"]) == 1
    assert "grid_z" in capsys.readouterr().err
    for argv in (["--height", "1", "--grid-z", "4"], ["--height", "1", "--z-grid", "0", "9"], ["--free-z", "--height-tx", "3=1"]):
        with pytest.raises(SystemExit):
            pos_3d_global._main([tdoa, "-r", cfg, "-o", str(out)] + argv)


def test_dropped_groups_print_the_sentence_of_pos_3d(monkeypatch, capsys):
    g, seen = posg3_golden.load("z_tall6g"), []
    _mock_posg3(monkeypatch, seen)
    a, b = int(g["group_ptr"][0]), int(g["group_ptr"][1])
    rows = np.zeros(b - a, dtype=tdoa_est.TDOA_DTYPE)
    for name in ("rx0", "rx1", "tdoa", "snr"):
        rows[name] = g[name][a:b]
    bad = rows.copy()
    bad["tdoa"][1] = np.nan
    two = rows[:1].copy()                                           # one pair: two receivers
    details = {}
    res = pos_3d_global.solve([tdoa_est.TdoaGroup(5, 1.0, 7, rows), tdoa_est.TdoaGroup(6, 2.0, 7, bad), tdoa_est.TdoaGroup(9, 3.0, 7, two)],
                              posg3_golden.rx_pos(g), free_z=True, details=details)
    assert capsys.readouterr().out == "Failed to estimate group #6: Nonfinite\nFailed to estimate group #9: Underdetermined\n"
    assert res["group_id"].tolist() == [5] and res["flags"].tolist() == [0]
    assert details["group_id"].tolist() == [5, 6, 9] and details["status"].tolist()[1:] == [pos3_ref.NONFINITE, pos3_ref.UNDERDETERMINED]
