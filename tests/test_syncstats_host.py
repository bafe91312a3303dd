"""Host side of the clock-sync and TDOA statistics (no GPU): the wiring of thr_beaconsync and thr_tdoastats into
the header, the symbol list and the build; the NumPy restatement (tests/syncstats_ref.py) against the
reference's recorded runs (tests/golden/syncstats); the argument errors that need no device; the exact
expansion of centred to raw coefficients; the report text from fixture arrays; both command lines' parsers."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import syncstats_golden as G
import syncstats_ref as R
from thrifty_amd import _native, beacon_analysis, build, cli, tdoa_analysis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["thr_beaconsync", "thr_bsync_fetch", "thr_bsync_free", "thr_debug_beaconsync_times",
           "thr_debug_beaconsync_geometry", "thr_tdoastats", "thr_tdstats_fetch", "thr_tdstats_free",
           "thr_debug_tdoastats_times", "thr_debug_tdoastats_geometry"]


def test_both_entry_points_are_declared_listed_and_built():
    header = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
    assert "#define THR_ABI_VERSION 11" in header and _native.ABI_VERSION == 11
    for sym in SYMBOLS:
        assert re.search(r"\b%s\(" % sym, header) and sym in _native.EXPORTS, sym
    for prefix, table in (("BSYNC", _native.BSYNC_OUTPUTS), ("TDSTATS", _native.TDSTATS_OUTPUTS)):
        for name, (which, _, _) in table.items():
            assert re.search(r"#define THR_%s_%s %d\b" % (prefix, name.upper(), which), header), name
        assert "#define THR_%s_N_OUTPUTS %d" % (prefix, len(table)) in header
    assert re.search(r"size_t rows, cells, discontinuities, cuts;\s*\} thr_bsync_counts;", header)
    assert re.search(r"size_t rows, cells, robust;\s*\} thr_tdstats_counts;", header)
    assert [n for n, _ in _native.BSYNC_COLUMNS] == [n for n, _ in R.BSYNC_COLUMNS]
    assert [n for n, _ in _native.TDSTATS_COLUMNS] == [n for n, _ in R.TDSTATS_COLUMNS]
    assert (_native.BSYNC_CUT_FITTED, _native.BSYNC_CUT_DEGENERATE, _native.BSYNC_CELL_NO_FIT) == \
        (R.CUT_FITTED, R.CUT_DEGENERATE, R.CELL_NO_FIT)
    assert "syncstats.hip" in build.SOURCES and build.UNPROFILED_SYNCSTATS == ("syncstats.hip",)
    assert build.PER_FILE_FLAGS["syncstats.hip"] == ["-ffp-contract=off"]
    source = open(os.path.join(build.CSRC, "syncstats.hip")).read()
    assert "#pragma clang fp contract(off)" in source and '#include "post_stages.hpp"' in source
    assert "atomic" not in source.split("#include", 1)[1] and "hipMalloc(" not in source     # partials in a fixed order
    assert '#include "seg_reduce.hpp"' in source        # the reduction: the same properties hold of its text
    shared = open(os.path.join(build.CSRC, "seg_reduce.hpp")).read()
    assert "#pragma clang fp contract(off)" in shared and "atomic" not in shared.split("#include", 1)[1]
    assert "hipMalloc(" not in shared and not re.search(r"\blog10\(", shared)
    assert "constexpr double kLight = 2.997e8;" in source and R.LIGHT == 2.997e8
    # what this file shares with reldist.hip stands once, in seg_cells.hpp: neither defines those kernels itself,
    # one inclusive sum of flags serves both, and every launch of the statistics stages is seg_reduce.hpp's
    cells = open(os.path.join(build.CSRC, "seg_cells.hpp")).read()
    other = open(os.path.join(build.CSRC, "reldist.hip")).read()
    assert "atomic" not in cells.split("#include", 1)[1] and "hipMalloc(" not in cells
    for kernel in ("k_pairs", "k_median", "k_td_median", "k_dev", "k_td_dev", "k_mask", "k_td_mask"):
        assert not re.search(r"\bvoid %s\(" % kernel, source + other), kernel
        assert kernel.startswith("k_td_") or len(re.findall(r"\bvoid %s\(" % kernel, cells)) == 1, kernel
    assert (source + other + cells + shared).count("hipcub::DeviceScan::InclusiveSum") == 1
    five = source + other + cells + shared + open(os.path.join(build.CSRC, "toadstats.hip")).read()
    assert five.count("hipLaunchKernelGGL") == 1 and "<<<" not in five
    assert "hipLaunchKernelGGL(k, grid, dim3(kBlock), 0, s, static_cast<P>(a)...);" in shared


def test_the_built_library_exports_both():
    assert os.path.exists(_native.LIB_PATH), "the library is not built: python -m thrifty_amd.build"
    lib = _native.load_library()
    assert all(getattr(lib, sym) for sym in SYMBOLS)
    for which in ("beaconsync", "tdoastats"):
        tile, workgroup = _native.syncstats_geometry(which)
        assert tile >= 64 and workgroup % 64 == 0


def test_csrc_hash_is_the_recorded_one_and_does_not_see_syncstats(monkeypatch):
    recorded = set(re.findall(r'"csrc_sha16": "([0-9a-f]{16})"', open(os.path.join(ROOT, "profiles", "hbm_traffic.json")).read()))
    assert recorded == {build.csrc_hash()}
    with_sync = build.csrc_hash()
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "syncstats.hip"])
    assert build.csrc_hash() == with_sync
    monkeypatch.undo()
    monkeypatch.setattr(build, "UNPROFILED_SYNCSTATS", ())
    assert build.csrc_hash() != with_sync


def test_cli_still_refuses_both_commands(capsys):
    for command in ("analyze_beacon", "analyze_tdoa"):
        assert command not in cli.COMMANDS
        assert cli.main([command]) != 0
    assert "not part of this port" in capsys.readouterr().err


# ------------------------------------------------------------------ the restatement against the reference
@pytest.fixture(scope="module")
def golden():
    return {name: G.load(name) for name in G.NAMES}


def test_the_fixtures_are_the_scenes_of_the_issue(golden):
    g = golden["realistic"]
    assert sorted(set(g["rxid"].tolist())) == [0, 1, 2] and sorted(set(g["txid"].tolist())) == [0, 1, 2, 3]
    counts, out = G.restated("realistic", 2)
    assert counts["cells"] == 6 and np.all(out["cell_stats"][:, 0] > 0)             # rx1 faster than rx0
    jumped = out["cell_counts"][:, 1] == 3
    assert jumped.sum() == 4 and np.all(out["cell_counts"][jumped, 2] == 3)         # one of four cuts is too short
    short = (out["cut_right"] - out["cut_left"] > 0) & (out["cut_flags"] == 0)
    assert short.any() and np.all((out["cut_right"] - out["cut_left"])[short] <= 8)
    rate = [g["b0_0_%d_deg1_coefs" % r][0, 0] - 1 for r in (1, 2)]      # the reference's own slope: tens of ppm
    assert all(5e-6 < v < 150e-6 for v in rate)
    counts, out = G.restated("slow_rx1", 2)
    assert np.all(out["cell_stats"][:, 0] < 0) and np.all(out["cell_flags"] == R.CELL_NO_FIT)
    assert np.all(out["cell_counts"][:, 1] >= out["cell_counts"][:, 0] - 3)         # (nearly) every row
    t = golden["tdoa"]
    assert t["is_outlier"].sum() >= 6 and len(t["cell_key"]) == 11
    assert sum(os.path.getsize(os.path.join(G.GOLDEN, f)) for f in os.listdir(G.GOLDEN)) < 200 << 10


@pytest.mark.parametrize("name,deg", [(n, d) for n in ("realistic", "slow_rx1") for d in (1, 2, 3)])
def test_restatement_equals_the_reference(golden, name, deg):
    counts, out = G.restated(name, deg)
    exact = G.exact(name, deg)
    G.check_beacon(counts, out, exact, golden[name], deg, name)


@pytest.mark.parametrize("robust", [False, True])
def test_tdoa_restatement_equals_the_reference(golden, robust):
    g = golden["tdoa"]
    counts, out = R.tdoa_stats_ref(G.tdoa_columns(g), robust=robust)
    G.check_tdoa(counts, out, g, "restatement")


# ------------------------------------------------------------------ argument errors before anything is launched
def _scene(n=12):
    rng = np.random.default_rng(3)
    cols = {"rxid": np.tile(np.array([0, 1], np.int32), n), "txid": np.zeros(2 * n, np.int32),
            "soa": np.repeat(np.arange(n) * 2.4e6, 2) + rng.normal(0, 1, 2 * n), "energy": np.full(2 * n, 500.0),
            "noise": np.full(2 * n, 10.0), "idx": np.arange(2 * n, dtype=np.int64)}
    return cols, 2 * np.arange(n + 1, dtype=np.int64), np.arange(2 * n, dtype=np.int64)


@pytest.mark.parametrize("change,words", [
    (dict(deg=0), "deg must be 1, 2 or 3"), (dict(deg=4), "deg must be 1, 2 or 3"),
    (dict(id_range=(5, 4)), "id range 5-4 is empty"),
    (dict(ptr=np.array([1, 2, 24])), r"match_ptr\[0\] must be 0"),
    (dict(ptr=np.array([0, 2, 1, 24])), "match_ptr decreases at match 1"),
    (dict(idx=np.r_[np.arange(23), 24]), "holds detection 24 of 24"),
    (dict(idx=np.r_[0, 2, np.arange(2, 24)]), "match 0 holds two detections of one receiver"),
    (dict(ptr=np.array([0]), idx=np.zeros(0, np.int64)), "selection is empty"),
])
def test_what_thr_beaconsync_refuses_on_the_host(change, words):
    cols, ptr, idx = _scene()
    ptr, idx = change.pop("ptr", ptr), change.pop("idx", idx)
    with pytest.raises(ValueError, match=words):
        _native.beaconsync(cols, ptr, idx, **change)


def test_duplicate_receiver_is_refused_by_the_restatement_too():
    cols, ptr, idx = _scene()
    with pytest.raises(ValueError, match="two detections of one receiver"):
        R.beacon_sync_ref(cols, ptr, np.r_[0, 2, np.arange(2, 24)])
    with pytest.raises(ValueError, match="differ in length"):
        _native.beaconsync(dict(cols, soa=np.zeros(3)), ptr, idx)
    with pytest.raises(ValueError, match="CSR pair"):
        _native.beaconsync(cols, ptr, idx[:-1])


@pytest.mark.parametrize("kwargs,words", [
    (dict(timestamp=(2.0, 1.0)), "timestamp range is empty"), (dict(detidx=(9, 3)), "detection id range is empty"),
    (dict(timestamp=(1.0, np.nan)), "timestamp range is empty"),
])
def test_what_thr_tdoastats_refuses_on_the_host(golden, kwargs, words):
    with pytest.raises(ValueError, match=words):
        _native.tdoastats(G.tdoa_columns(golden["tdoa"]), **kwargs)
    empty = {name: np.zeros(0, kind) for name, kind in R.TDSTATS_COLUMNS}
    with pytest.raises(ValueError, match="selection is empty"):
        _native.tdoastats(empty)
    with pytest.raises(ValueError, match="selection is empty"):
        R.tdoa_stats_ref(empty)


# ------------------------------------------------------------------ coefficients, reports, command lines
def test_expansion_of_centred_to_raw_coefficients_is_exact():
    rng = np.random.default_rng(11)
    for deg in (1, 2, 3):
        fit = np.r_[2.1e9 + rng.uniform(0, 1), 3.3e8 * rng.uniform(0.5, 1), 2.1e9 + rng.uniform(0, 1e4),
                    rng.normal(0, 1.0), 3.3e8 + rng.normal(0, 1e3), rng.normal(0, 50.0), rng.normal(0, 5.0)]
        fit[4 + deg:] = 0.0
        coef = beacon_analysis.raw_coefficients(fit, deg)
        assert coef.shape == (deg + 1,)
        xm, sc, ym = (Fraction(float(v)) for v in fit[:3])
        want = [Fraction(0)] * (deg + 1)        # by the binomial theorem, independently of the module's recurrence
        for k in range(deg + 1):
            for i in range(k + 1):
                want[i] += Fraction(float(fit[3 + k])) / sc ** k * math_comb(k, i) * (-xm) ** (k - i)
        want[0] += ym
        assert [float(v) for v in reversed(want)] == coef.tolist()
        for x in (fit[0] - fit[1], fit[0] + 0.37 * fit[1]):      # and the expansion IS the centred polynomial
            u = (Fraction(float(x)) - xm) / sc
            assert sum(w * Fraction(float(x)) ** i for i, w in enumerate(want)) == ym + sum(
                Fraction(float(fit[3 + k])) * u ** k for k in range(deg + 1))


def math_comb(n, k):
    import math
    return math.comb(n, k)


def test_fit_poly_model_is_the_exact_fit(golden):
    g = golden["realistic"]
    tag = "b0_0_2_deg2_"
    matrix, left = g[tag + "matrix"], int(g[tag + "cut_left"][0])
    soa = g["soa"][matrix][left:left + 20]
    coef, residuals = beacon_analysis.fit_poly_model(soa, 2)
    want_coef, mean, want_res = R.exact_polyfit(soa[:, 0], soa[:, 1], 2)
    assert residuals.tolist() == [float(v) for v in want_res]
    assert coef.tolist() == [float(v) for v in reversed(R.expand(want_coef, mean))]
    with pytest.raises(ValueError, match="distinct soa"):
        beacon_analysis.fit_poly_model(np.ones((12, 2)), 1)


@pytest.mark.parametrize("name,deg", [("realistic", 1), ("realistic", 2), ("realistic", 3), ("slow_rx1", 2)])
def test_report_text_from_the_restated_arrays_is_the_references(golden, name, deg):
    g = golden[name]
    counts, out = G.restated(name, deg)
    sync = beacon_analysis.BeaconSync(counts, out, g["idx"], deg, 2.4e6)
    for c, (b, r0, r1) in enumerate(sync.cell_key):
        tag = "b%d_%d_%d_deg%d_" % (b, r0, r1, deg)
        text = beacon_analysis.format_report(sync, c)
        if str(g[tag + "error"]):
            assert text == str(g[tag + "text"]) + beacon_analysis.NO_FIT_TEXT + "\n"
        else:
            assert text == str(g[tag + "text"])
        assert sync.cell(b, r0, r1)["discontinuities"].tolist() == out["disc_idx"][out["disc_ptr"][c]:out["disc_ptr"][c + 1]].tolist()
    with pytest.raises(KeyError):
        sync.index(9, 0, 1)


def test_tdoa_report_and_tables_from_the_restated_arrays(golden, tmp_path):
    g = golden["tdoa"]
    stats = tdoa_analysis.TdoaStats(*R.tdoa_stats_ref(G.tdoa_columns(g), robust=True))
    for c in range(len(stats)):
        assert tdoa_analysis.format_report(stats, c) == str(g["text"][c])
    tx, std = tdoa_analysis.variance_table(stats, 0, 1)
    assert tx.tolist() == [2, 3, 5, 7] and std.tolist() == np.around(g["np_stats"][:4, 1], 1).tolist()
    tx, mean = tdoa_analysis.mean_table(stats, 1, 2)
    assert tx.tolist() == [2, 3, 5, 7] and mean.tolist() == np.around(g["np_stats"][7:, 0], 1).tolist()
    assert tdoa_analysis.count_table(stats, 0, 2)[1].tolist() == np.diff(stats.cell_ptr)[4:7].tolist()
    assert tdoa_analysis.count_table(stats, 0, 1, robust=True)[1].tolist() == stats.robust_count[:4].tolist()
    cell = stats.cell(0, 1, 7)
    assert cell["count"] == 6 and cell["std"] == 0.0 and cell["mad"] == 0.0 and not cell["outlier"].any()
    stats.save(tmp_path / "s.npz")
    assert np.array_equal(np.load(tmp_path / "s.npz")["stats"], stats.stats)


def test_beacon_parser_takes_the_references_arguments(tmp_path, capsys):
    parser = beacon_analysis._parser()
    actions = {a.dest: a for a in parser._actions}
    assert (actions["toads"].default, actions["matches"].default) == ("data.toads", "data.match")
    assert [actions[k].default for k in ("beacon", "rx0", "rx1", "deg", "range")] == [0, 0, 1, 2, None]
    toads = tmp_path / "x.toads"
    toads.write_text("")
    args = parser.parse_args([str(toads), str(toads), "--beacon", "3", "--rx0", "2", "--rx1", "5", "--range", "10-250",
                              "--deg", "3", "--all", "-o", "sync.npz"])
    assert (args.beacon, args.rx0, args.rx1, args.range, args.deg, args.all, args.output) == (3, 2, 5, (10, 250), 3, True, "sync.npz")
    args.toads.close()
    args.matches.close()
    assert beacon_analysis.parse_range(None) is None and beacon_analysis.parse_range("4-9") == (4, 9)
    for export in (["--export"], ["--export", "figure"]):
        assert beacon_analysis._main([str(toads), str(toads)] + export) == 1
        assert "plots are not part of this port" in capsys.readouterr().err
    assert "matplotlib" not in open(beacon_analysis.__file__).read()


def test_tdoa_parser_takes_the_references_arguments(tmp_path):
    parser = tdoa_analysis._parser()
    actions = {a.dest: a for a in parser._actions}
    assert actions["tdoa"].default == "data.tdoa"
    assert [actions[k].default for k in ("rx0", "rx1", "tx", "timestamp", "detidx")] == [0, 1, 0, None, None]
    path = tmp_path / "x.tdoa"
    path.write_text("")
    args = parser.parse_args([str(path), "--rx0", "2", "--rx1", "1", "--tx", "4", "--timestamp", "100-200", "--detidx", "5-9",
                              "--robust", "--all", "-o", "s.npz"])
    assert (args.rx0, args.rx1, args.tx, args.timestamp, args.detidx, args.robust, args.all) == (2, 1, 4, (100, 200), (5, 9), True, True)
    args.tdoa.close()
    assert tdoa_analysis._main([str(path)]) == 1        # an empty file: an empty selection, said so, status 1
    assert "matplotlib" not in open(tdoa_analysis.__file__).read()


def test_module_docstrings_name_the_deviations():
    for words in ("sign-sensitive", "row 0", "nine rows", "0 outliers", "rational arithmetic", "without a fitted cut",
                  "3e8 / sample_rate"):
        assert words in beacon_analysis.__doc__, words
    for words in ("2.997e8", "is_outlier", "3.5", "one row", "re-estimation"):
        assert words in tdoa_analysis.__doc__, words


def test_a_tuple_of_two_match_lists_is_not_taken_for_csr():
    ptr, idx = beacon_analysis._as_csr(([0, 1], [2, 3]))
    assert ptr.tolist() == [0, 2, 4] and idx.tolist() == [0, 1, 2, 3]
    ptr, idx = beacon_analysis._as_csr([[0, 1], [2, 3, 4]])
    assert ptr.tolist() == [0, 2, 5] and idx.tolist() == [0, 1, 2, 3, 4]
    pair = (np.array([0, 2, 5]), np.array([7, 8, 9, 10, 11]))
    assert beacon_analysis._as_csr(pair) is pair
    ptr, idx = beacon_analysis._as_csr((np.array([1, 2]), np.array([3, 4])))      # ptr[0] != 0: two matches
    assert ptr.tolist() == [0, 2, 4] and idx.tolist() == [1, 2, 3, 4]
