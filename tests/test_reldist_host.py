"""Host side of the relative-distance stage (no GPU): the wiring of thr_reldist into the header, the symbol list and
the build; the NumPy statement (tests/reldist_ref.py) against the reference's recorded runs
(tests/golden/reldist) bit for bit; np.searchsorted's ties; the geometry from positions against the script's three
constants; the argument errors that need no device; the smoother's recorded tolerance; the command line's parser."""
import os
import re

import numpy as np
import pytest

import reldist_ref as R
import reldist_scenes as SC
from thrifty_amd import _native, build, cli, reldist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["thr_reldist", "thr_reldist_fetch", "thr_reldist_free", "thr_debug_reldist_times", "thr_debug_reldist_geometry"]


def test_entry_points_are_declared_listed_and_built():
    header = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
    assert "#define THR_ABI_VERSION 11" in header and _native.ABI_VERSION == 11
    assert "+ thr_reldist / thr_reldist_fetch" in header.split("#define THR_ABI_VERSION")[0]      # the "within 11" list
    for sym in SYMBOLS:
        assert re.search(r"\b%s\(" % sym, header) and sym in _native.EXPORTS, sym
    for name, (which, _, _) in _native.RELDIST_OUTPUTS.items():
        assert re.search(r"#define THR_RELDIST_%s %d\b" % (name.upper(), which), header), name
    assert "#define THR_RELDIST_N_OUTPUTS %d" % len(_native.RELDIST_OUTPUTS) in header
    assert re.search(r"size_t rows, cells, speeds, speed_points, dop_points;\s*\} thr_reldist_counts;", header)
    assert _native.RELDIST_COUNTS == ("rows", "cells", "speeds", "speed_points", "dop_points")
    assert [n for n, _ in _native.RELDIST_COLUMNS] == [n for n, _ in R.RELDIST_COLUMNS]
    for name, value in (("NEAREST", _native.RELDIST_METHODS["nearest"]), ("LINPOL", _native.RELDIST_METHODS["linpol"]),
                        ("ROW_HELD", R.ROW_HELD), ("CELL_UNSORTED", R.CELL_UNSORTED), ("CELL_NO_BEACON", R.CELL_NO_BEACON)):
        assert "#define THR_RELDIST_%s %d\n" % (name, value) in header
    assert (_native.RELDIST_ROW_HELD, _native.RELDIST_CELL_UNSORTED, _native.RELDIST_CELL_NO_BEACON) == \
        (R.ROW_HELD, R.CELL_UNSORTED, R.CELL_NO_BEACON)
    assert "reldist.hip" in build.SOURCES and "seg_cells.hpp" in build.HEADERS
    assert build.UNPROFILED_RELDIST == ("reldist.hip", "seg_cells.hpp")
    assert build.PER_FILE_FLAGS["reldist.hip"] == ["-ffp-contract=off"]
    source = open(os.path.join(build.CSRC, "reldist.hip")).read()
    assert "#pragma clang fp contract(off)" in source and '#include "seg_reduce.hpp"' in source
    assert "atomic" not in source.split("#include", 1)[1] and "hipMalloc(" not in source     # every sum has one order
    assert "constexpr double kLight = 2.997e8;" in source and R.LIGHT == reldist.LIGHT == 2.997e8
    assert "constexpr double kSingular = 1e-12;" in source and R.SINGULAR == 1e-12
    shared = open(os.path.join(build.CSRC, "seg_cells.hpp")).read()
    assert "atomic" not in shared.split("#include", 1)[1] and "hipMalloc(" not in shared
    assert "THR_RELDIST_N_OUTPUTS" in open(os.path.join(build.CSRC, "seg_reduce.hpp")).read()      # kMaxOutputs counts it


def test_the_built_library_exports_them():
    assert os.path.exists(_native.LIB_PATH), "the library is not built: python -m thrifty_amd.build"
    lib = _native.load_library()
    assert all(getattr(lib, sym) for sym in SYMBOLS)
    tile, workgroup, lanes = _native.reldist_geometry()
    assert tile >= 64 and workgroup % 64 == 0 and lanes == 64


def test_csrc_hash_does_not_see_the_stage(monkeypatch):
    with_stage = build.csrc_hash()
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "reldist.hip"])
    monkeypatch.setattr(build, "HEADERS", [s for s in build.HEADERS if s != "seg_cells.hpp"])
    assert build.csrc_hash() == with_stage
    monkeypatch.undo()
    monkeypatch.setattr(build, "UNPROFILED_RELDIST", ())
    assert build.csrc_hash() != with_stage


def test_cli_has_no_such_command():
    assert "reldist" not in cli.COMMANDS and "reldist_nearest" not in cli.COMMANDS


# ------------------------------------------------------------------ the statement against the reference
@pytest.fixture(scope="module")
def golden():
    return {name: SC.load(name) for name in SC.NAMES}


@pytest.fixture(scope="module")
def restated(golden):
    out = {}
    for name, g in golden.items():
        for method in ("nearest", "linpol"):
            args, kwargs = SC.golden_input(g, method)
            out[name, method] = R.reldist_ref(*args, **kwargs)
    return out


check_against_fixture = SC.check_against_fixture


def test_the_fixtures_are_the_scenes_of_the_issue(golden, restated):
    for name in ("a", "b", "c", "e", "f"):
        g = golden[name]
        assert sorted(set(g["rxid"].tolist())) == [0, 1] and "m1_b0_0_1_raw_linpol" in g
    out = restated["a", "linpol"][1]
    assert not out["row_flags"].any() and np.all((out["hi"] >= 1) & (out["hi"] < out["cell_counts"][0, 1]))      # the interior
    out = restated["b", "linpol"][1]
    assert out["row_flags"].tolist() == [0] * (len(out["raw"]) - 1) + [R.ROW_HELD] and out["hi"][-1] == out["cell_counts"][0, 1]
    c = golden["c"]
    rows = c["soa"][restated["c", "nearest"][1]["row_det"][:, 0]] % 1000.0
    assert np.count_nonzero(rows == 500.0) > 20 and np.count_nonzero(rows == 0.0) > 5        # midway, and ON a beacon row
    d = golden["d"]
    assert sorted(set(d["rxid"].tolist())) == [0, 1, 2, 5] and len(restated["d", "linpol"][1]["cell_key"]) == 24
    assert set(np.diff(d["match_ptr"]).tolist()) == {2, 3, 4}
    for method in ("nearest", "linpol"):
        out = restated["e", method][1]
        assert all(out[m].any() for m in ("mask1", "mask2", "mask3")), method
    out = restated["f", "linpol"][1]
    assert out["medians"][0, 1] == 0.0 and out["medians"][0, 5] == 0.0 and out["mask1"].any()        # MAD = 0
    assert sum(os.path.getsize(os.path.join(SC.GOLDEN, f)) for f in os.listdir(SC.GOLDEN)) < 256 << 10


@pytest.mark.parametrize("name", SC.NAMES)
@pytest.mark.parametrize("method", ["nearest", "linpol"])
def test_statement_equals_the_reference_bit_for_bit(golden, restated, name, method):
    counts, out = restated[name, method]
    seen = check_against_fixture(out, golden[name], method, name)
    assert seen >= 1 and counts["rows"] == len(out["raw"]) == out["cell_ptr"][-1]


def test_pairs_of_a_four_receiver_match_are_the_two_detection_matches(golden, restated):
    """Scene d, pair (1, 5): the rows are exactly the matches that hold both, whatever else they hold."""
    g = golden["d"]
    out = restated["d", "nearest"][1]
    ci = out["cell_key"].tolist().index([1, 0, 1, 5])
    a, b = out["cell_ptr"][ci:ci + 2]
    want = []
    for i, (s, e) in enumerate(zip(g["match_ptr"][:-1], g["match_ptr"][1:])):
        dets = g["match_idx"][s:e]
        if g["txid"][dets[0]] == 1 and {1, 5} <= set(g["rxid"][dets].tolist()):
            want.append(i)
    assert out["row_match"][a:b].tolist() == want and len(want) > 20


def test_searchsorted_ties_and_nan():
    b0 = np.array([5.0, 10.0, 10.0, 15.0])
    t0 = np.array([4.0, 5.0, 7.5, 10.0, 12.5, 15.0, 16.0, np.nan])
    hi, near = R.nearest_rows(b0, t0)
    assert hi.tolist() == [0, 0, 1, 1, 3, 3, 4, 4]              # side='left': ON a row is that row; a NaN is last
    assert near.tolist() == [0, 0, 1, 1, 3, 3, 3, 3]            # a tie (7.5, 12.5) keeps hi: the comparison is strict
    raw, held = R.raw_linpol(t0[:7], t0[:7] + 1.0, b0, b0 + 100.0, hi[:7])
    assert held.tolist() == [True, True, False, False, False, False, True]
    assert raw.tolist() == [4.0 + 1 - 105, 5.0 + 1 - 105, 7.5 + 1 - 107.5, 10.0 + 1 - 110, 12.5 + 1 - 112.5, 16 - 115.0, 17 - 115.0]


# ------------------------------------------------------------------ geometry, smoother, errors, command line
def test_geometry_from_positions_gives_the_scripts_constants():
    d_beacon, dist_rx, dist_beacon = SC.SCRIPT_METRES
    to_rx0 = dist_beacon - d_beacon
    bx = (to_rx0 ** 2 - dist_beacon ** 2 + dist_rx ** 2) / (2 * dist_rx)
    beacon = (bx, np.sqrt(to_rx0 ** 2 - bx ** 2))
    s2m = 2.997e8 / 2.4e6
    row = reldist.geometry_row(0, 0, 1, beacon, (0.0, 0.0), (dist_rx, 0.0), 2.4e6)
    assert row[:3] == (0, 0, 1)
    assert np.allclose(row[3:], [d_beacon / s2m, dist_rx / s2m, dist_beacon / s2m], rtol=1e-12, atol=0)
    table = reldist.geometry_table({0: (0.0, 0.0), 1: (dist_rx, 0.0), 4: (0.0, 100.0)}, {0: beacon, 9: (1.0, 1.0)}, 2.4e6)
    assert [r[:3] for r in table] == [(0, 0, 1), (0, 0, 4), (0, 1, 4), (9, 0, 1), (9, 0, 4), (9, 1, 4)] and table[0] == row
    assert reldist.geometry_table(None, {0: beacon}, 2.4e6) == []
    # a mobile on the baseline at p metres from rx1, ideal clocks: x is p minus the beacon's distance from rx1
    p = 2500.0
    raw = ((p - (dist_rx - p)) - (dist_beacon - to_rx0)) / s2m       # TDOA(mobile) - TDOA(beacon) = (2 p - D) - d_beacon
    x = (raw + row[3] + row[4]) / 2.0 - row[5]
    assert abs(x * s2m - (p - dist_beacon)) < 1e-6


def test_smoother_definition_on_small_cases():
    x = np.arange(7.0)
    y = 3.0 + 0.5 * x
    assert R.window_len(7, 0.025) == 2 and R.window_len(7, 0.5) == 3 and R.window_len(7, 1.0) == 7 and R.window_len(200, 0.025) == 5
    assert [R.window_start(x, i, 3) for i in range(7)] == [0, 0, 1, 2, 3, 4, 4]         # pinned at both ends
    assert [R.window_start(x, i, 4) for i in range(7)] == [0, 0, 0, 1, 2, 3, 3]         # ties: the lowest window
    assert [R.window_start(np.full(5, 2.0), i, 2) for i in range(5)] == [0] * 5
    assert np.allclose(R.smooth(x, y, 1.0), y, rtol=1e-14)                              # a line is its own local line
    assert R.smooth(x, y, 0.025).tolist() == y.tolist()                                 # k = 2: the far point weighs 0
    flat = R.smooth(np.full(5, 2.0), np.array([1.0, 2.0, 3.0, 4.0, 10.0]), 0.6)
    assert flat.tolist() == [2.0] * 5                                                   # h = 0: the mean of the window
    assert R.smooth(x[:1], y[:1], 0.5).tolist() == y[:1].tolist() and R.smooth(x, y, 0.0).tolist() == y.tolist()


def test_recorded_smoother_tolerance_is_the_measured_one():
    """The measurement of tests/reldist_ref.py's docstring, taken again: the gap of every input is below 1e-9, and the
    largest is the recorded one (to the digits that were printed)."""
    worst = 0.0
    for name, (args, kwargs) in SC.every_input().items():
        narrow = R.reldist_ref(*args, **kwargs)[1]
        wide = R.reldist_ref(*args, dtype=np.longdouble, **kwargs)[1]
        gap = R.smooth_gap(wide, narrow)[0]
        assert gap < 1e-9, name
        worst = max(worst, gap)
    if np.finfo(np.longdouble).eps < 2e-19:        # 80-bit long double, as where it was measured
        assert float("%.3g" % worst) == R.SMOOTH_GAP
    assert R.SMOOTH_RTOL == 16 * R.SMOOTH_GAP


def _scene(n=12):
    txs = SC.synth(SC.interleaved(2 * n, 2), {0: 0.0, 1: 9000.0}, 3, {0: 4000.0})
    return SC.assemble(txs)


@pytest.mark.parametrize("change,words", [
    (dict(smooth_frac=1.5), r"smooth_frac must lie in \[0, 1\]"), (dict(smooth_frac=-0.1), "smooth_frac must lie"),
    (dict(smooth_frac=float("nan")), "smooth_frac must lie"),
    (dict(sample_rate=0.0), "must be positive"), (dict(carrier_hz=-1.0), "must be positive"),
    (dict(ptr=np.array([1, 2, 48])), r"match_ptr\[0\] must be 0"),
    (dict(ptr=np.array([0, 2, 1, 48])), "match_ptr decreases at match 1"),
    (dict(idx=np.r_[np.arange(47), 48]), "holds detection 48 of 48"),
    (dict(idx=np.r_[0, 2, np.arange(2, 48)]), "match 0 holds two detections of one receiver"),
    (dict(ptr=np.array([0]), idx=np.zeros(0, np.int64)), "selection is empty"),
])
def test_what_thr_reldist_refuses_on_the_host(change, words):
    cols, ptr, idx = _scene()
    assert len(idx) == 48
    ptr, idx = change.pop("ptr", ptr), change.pop("idx", idx)
    with pytest.raises(ValueError, match=words):
        _native.reldist(cols, ptr, idx, [0], **change)


def test_what_the_wrapper_and_the_statement_refuse():
    cols, ptr, idx = _scene()
    with pytest.raises(ValueError, match="two detections of one receiver"):
        R.reldist_ref(cols, ptr, np.r_[0, 2, np.arange(2, 48)], [0])
    with pytest.raises(ValueError, match="selection is empty"):
        R.reldist_ref(cols, ptr, idx, [0], mobiles=[9])
    with pytest.raises(ValueError, match="differ in length"):
        _native.reldist(dict(cols, soa=np.zeros(3)), ptr, idx, [0])
    with pytest.raises(ValueError, match="CSR pair"):
        _native.reldist(cols, ptr, idx[:-1], [0])
    with pytest.raises(ValueError, match="'nearest' or 'linpol'"):
        _native.reldist(cols, ptr, idx, [0], method="cubic")
    with pytest.raises(ValueError, match="list of beacons"):
        _native.reldist(cols, ptr, idx, None)


def test_parser_takes_the_scripts_defaults_and_the_new_arguments(tmp_path):
    parser = reldist._parser()
    actions = {a.dest: a for a in parser._actions}
    assert (actions["toads"].default, actions["matches"].default) == ("rx.toads", "rx.match")
    assert [actions[k].default for k in ("tx", "rx0", "rx1", "method", "sample_rate", "block_size", "carrier_hz", "frac")] == \
        [1, 0, 1, "linpol", 2.4e6, 16384, 433e6, 0.025]
    toads = tmp_path / "x.toads"
    toads.write_text("")
    args = parser.parse_args([str(toads), str(toads), "--beacon", "0", "--beacon", "7", "--tx", "3", "--rx0", "2", "--rx1", "5",
                              "--method", "nearest", "-r", "rx.cfg", "-b", "b.cfg", "-s", "2e6", "--block-size", "8192",
                              "--carrier-hz", "868e6", "--frac", "0.1", "--all", "-o", "r.npz"])
    assert (args.beacon, args.tx, args.rx0, args.rx1, args.method, args.rx_pos, args.beacon_pos) == ([0, 7], 3, 2, 5, "nearest", "rx.cfg", "b.cfg")
    assert (args.sample_rate, args.block_size, args.carrier_hz, args.frac, args.all, args.output) == (2e6, 8192, 868e6, 0.1, True, "r.npz")
    args.toads.close()
    args.matches.close()
    with pytest.raises(SystemExit):
        parser.parse_args([str(toads), str(toads)])         # --beacon is required
    with pytest.raises(SystemExit):
        parser.parse_args([str(toads), str(toads), "--beacon", "0", "--method", "cubic"])
    assert "matplotlib" not in open(reldist.__file__).read() and "statsmodels.lowess" in reldist.__doc__


def test_report_text_from_the_restated_arrays(restated):
    counts, out = restated["e", "linpol"]
    result = reldist.RelDist(counts, out, "linpol", 2.4e6)
    text = reldist.format_report(result, 0).splitlines()
    kept = int(out["cell_counts"][0, 2])
    assert text[0] == "Number of outliers: %d / %d" % (counts["rows"] - kept, counts["rows"]) and kept < counts["rows"]
    assert text[1] == "mean = %s" % float(out["cell_stats"][0, 1]) and text[2] == "std = %s" % float(out["cell_stats"][0, 2])
    assert re.fullmatch(r"within one std = \d+%; median smoothed speed = -?\d+\.\d km/h; median smoothed Doppler = -?\d+\.\d km/h", text[3])
    cell = result.cell(1, 0, 0, 1)
    assert len(cell["x"]) == counts["rows"] and len(cell["speed"]) == kept - 1 and cell["count"] == kept
    assert len(cell["speed_smooth"]) == len(cell["speed_smooth_x"]) == int(out["cell_counts"][0, 3])
    assert len(cell["doppler_smooth"]) == int(out["cell_counts"][0, 4]) and result.cells == [(1, 0, 0, 1)]
    with pytest.raises(KeyError):
        result.index(2, 0, 0, 1)
