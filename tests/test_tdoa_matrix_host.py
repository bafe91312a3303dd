"""Per-beacon TDOA matrices, the part that needs no GPU: the NumPy statement (tests/tdoa_matrix_ref.py) against every
fixture the reference made, the table functions and the report text on a fixture's arrays, command-line parsing, and
the plumbing (header, export list, build lists, the hash)."""
import os
import re

import numpy as np
import pytest

import tdoa_matrix_golden as G
from tdoa_matrix_ref import tdoa_matrix_ref
from thrifty_amd import _native, build, tdoa_matrix

ROOT = G.ROOT
_ref = {}


def ref_of(name):
    if name not in _ref:
        g = G.load(name)
        _ref[name] = tdoa_matrix_ref(G.columns(g), g["match_ptr"], g["match_idx"], **G.arguments(g))
    return _ref[name]


@pytest.mark.parametrize("name", G.SETS)
def test_the_statement_equals_the_reference(name):
    g = G.load(name)
    counts, out = ref_of(name)
    assert counts["cells"] == len(g["cell_key"]) and counts["tasks"] == len(g["status"])
    G.check_structure(out, g, name)
    G.check_rows(out, g, name)
    G.check_own_mask_and_stats(out, name)
    G.check_reference_stats(out, g, name)


def test_the_fixtures_hold_what_they_are_for():
    g = G.load("tdmat_realistic")
    assert len(g["receivers"]) == 4 and sorted(g["beacons"].tolist()) == [0, 1] and 150 <= len(g["match_ptr"]) - 1 <= 400
    assert np.mean(np.r_[g["firm_std"], g["firm_mean"]]) >= 0.9
    keys = [tuple(k) for k in g["cell_key"][:, 2:].tolist()]
    assert (0, 1) in keys and (1, 0) in keys                       # one beacon measured against the other
    assert np.any(np.diff(g["match_ptr"]) < 4)                      # some matches miss a receiver
    e = G.load("tdmat_edges")
    assert e["beacons"].tolist() == [5, 1]                          # an unsorted beacon list
    assert {0, 1, 2, 3} <= set(e["n_window"].tolist()) and {0, 1, 2, 3} <= set(e["status"].tolist())
    assert {1, 2} <= set(e["cell_counts"][:, 2].tolist()) and {2, 3} <= set(e["cell_counts"][:, 0].tolist())
    assert {64, 65, 256, 257} <= set(G.load("tdmat_wide")["n_window"].tolist())
    n = G.load("tdmat_nearest")
    assert float(n["ref_err_max"]) == 0.0 and str(n["model"]) == "nearest" and n["outlier"].any()
    for name in G.SETS:
        assert os.path.getsize(os.path.join(G.GOLDEN, name + ".npz")) < 128 * 1024


def result_of(name):
    g = G.load(name)
    counts, out = ref_of(name)
    return g, tdoa_matrix.TdoaMatrices(counts, out, g["beacons"].tolist(), str(g["model"]), int(g["deg"]))


@pytest.mark.parametrize("name", G.SETS)
def test_tables_are_the_scripts_numbers(name):
    g, result = result_of(name)
    G.check_tables(result, g, name)


def test_tables_cells_and_report_text():
    g, result = result_of("tdmat_edges")
    beacons, txids, std = result.variance_table(0, 1)
    assert beacons.tolist() == [1, 5] and txids.tolist() == sorted(set(g["cell_key"][:, 3].tolist()) | {1, 5})
    _, _, count = result.count_table(0, 1)
    _, _, mean = result.mean_table(0, 1)
    assert count.dtype == np.int64 and std.shape == mean.shape == count.shape == (2, len(txids))
    at = {t: i for i, t in enumerate(txids.tolist())}
    assert count[0, at[1]] == 0 and std[0, at[1]] == 0.0 and mean[1, at[5]] == 0.0           # the diagonal: no cell
    assert count[0, at[9]] == 1 and std[0, at[9]] == 0.0 and count[0, at[10]] == 2          # one TDOA, two TDOAs
    assert count[0, at[8]] == 0 and mean[0, at[8]] == 0.0                                   # every task failed
    assert count[1, at[1]] == 0                                                              # beacon 5: a list of 2 rows
    cell = result.cell(0, 1, 1, 9)
    assert cell["tdoas"] == 1 and cell["kept"] == 1 and cell["tx_rows"] == 3 and not cell["too_few"]
    assert len(cell["timestamp"]) == len(cell["tdoa"]) == len(cell["outlier"]) == 3 and cell["std"] == 0.0
    assert result.cell(0, 1, 5, 1)["too_few"] and np.isnan(result.cell(0, 1, 5, 1)["mean"])
    with pytest.raises(KeyError):
        result.cell(0, 1, 1, 1)
    text = result.format_report(0, 1)
    lines = text.splitlines()
    assert lines[0] == "# TDOA matrices for RX 0 and RX 1" and lines[1] == "# TDOA variance matrix for 0 and 1:"
    assert lines[2].split() == ["v", "beacon/tx", ">"] + [str(t) for t in txids.tolist()]
    assert set(lines[3]) == {"-", " "} and lines[4].split()[0] == "1" and lines[5].split()[0] == "5"
    assert "# TDOA mean matrix for 0 and 1:" in lines and "# TDOA count matrix for 0 and 1:" in lines
    assert lines[4].split()[1:] == [str(v) for v in std[0].tolist()] and text.endswith("\n\n\n")
    assert "tabulate" not in open(tdoa_matrix.__file__).read().replace("`tabulate`", "")
    assert result.pairs == [(0, 1), (0, 2), (1, 2)]


def test_save_round_trips(tmp_path):
    g, result = result_of("tdmat_wide")
    result.save(str(tmp_path / "m.npz"))
    with np.load(tmp_path / "m.npz") as f:
        assert f["beacons"].tolist() == [0] and str(f["model"]) == "poly" and float(f["window"]) == 4.0
        for name in result.names:
            assert f[name].tobytes() == getattr(result, name).tobytes(), name


@pytest.fixture
def default_files(tmp_path, monkeypatch):
    """argparse opens the positional defaults: empty files of those names in the working directory"""
    for name in ("data.toads", "data.match", "a.toads", "a.match"):
        (tmp_path / name).write_text("")
    monkeypatch.chdir(tmp_path)


def test_command_line_parsing(default_files):
    p = tdoa_matrix._parser()
    a = p.parse_args(["--beacons", "0", "1"])
    assert a.beacons == [0, 1] and a.tx is None and a.rx is None and a.window_size == 4.0 and a.sample_rate == 2.4e6
    assert a.model == "poly" and a.deg == 2 and a.rx_pos is None and a.output is None and not a.all
    assert tdoa_matrix._selection(p, a) is None
    a = p.parse_args(["a.toads", "a.match", "--beacons", "3", "--tx", "4", "5", "--rx", "0", "2", "--all", "-w", "8", "-s", "1e6",
                      "--model", "nearest", "--deg", "1", "-o", "x.npz"])
    assert a.toads.name == "a.toads" and a.matches.name == "a.match"
    assert a.tx == [4, 5] and tdoa_matrix._selection(p, a) == [0, 2] and a.window_size == 8.0 and a.model == "nearest"
    a = p.parse_args(["--beacons", "3", "--rx0", "2", "--rx1", "1"])
    assert tdoa_matrix._selection(p, a) == [1, 2]
    for bad in (["--beacons", "3", "--rx0", "2"], ["--beacons", "3", "--rx0", "2", "--rx1", "2"],
                ["--beacons", "3", "--rx0", "2", "--rx1", "1", "--all"], [], ["--beacons", "1", "--model", "spline"]):
        with pytest.raises(SystemExit):
            tdoa_matrix._selection(p, p.parse_args(bad))


def test_argument_errors_that_need_no_device():
    g = G.load("tdmat_wide")
    with pytest.raises(ValueError, match="model must be one of"):
        tdoa_matrix.tdoa_matrices(G.columns(g), G.matches(g), [0], model="spline")
    with pytest.raises(ValueError, match="come together"):
        tdoa_matrix.tdoa_matrices(G.columns(g), G.matches(g), [0], rx_pos={0: (0, 0), 1: (1, 1)})


def test_thr_tdoamatrix_is_declared_listed_and_built():
    header = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
    assert "#define THR_ABI_VERSION 11" in header and _native.ABI_VERSION == 11
    assert re.search(r"\+ thr_tdoamatrix / thr_tdmat_fetch / thr_tdmat_free / thr_debug_tdoamatrix_times / _geometry", header)
    assert header.index("within 11, a pure addition") < header.index("+ thr_tdoamatrix /") < header.index("#define THR_ABI_VERSION")
    assert re.search(r"\bint thr_tdoamatrix\(int device_id, size_t n_det,", header)
    for name in ("thr_tdoamatrix", "thr_tdmat_fetch", "thr_tdmat_free", "thr_debug_tdoamatrix_times", "thr_debug_tdoamatrix_geometry"):
        assert name in _native.EXPORTS and re.search(r"\b%s\(" % name, header), name
    for name, (which, _, _) in _native.TDMAT_OUTPUTS.items():
        macro = {"medians": "MEDIANS", "tdoa": "TDOA", "timestamp": "TIMESTAMP", "status": "STATUS", "snr": "SNR",
                 "outlier": "OUTLIER"}.get(name, name.upper())
        assert re.search(r"#define THR_TDMAT_%s %d\b" % (macro, which), header), name
    assert re.search(r"#define THR_TDMAT_N_OUTPUTS %d\b" % len(_native.TDMAT_OUTPUTS), header)
    assert re.search(r"#define THR_TDMAT_MAX_BEACONS %d\b" % _native.TDMAT_MAX_BEACONS, header)
    for name, value in (("OK", _native.TDMAT_OK), ("NO_MODEL", _native.TDMAT_NO_MODEL), ("OUT_OF_RANGE", _native.TDMAT_OUT_OF_RANGE),
                        ("SKIPPED", _native.TDMAT_SKIPPED), ("CELL_TOO_FEW", _native.TDMAT_CELL_TOO_FEW)):
        assert re.search(r"#define THR_TDMAT_%s %d\b" % (name, value), header), name
    if os.path.exists(_native.LIB_PATH):
        lib = _native.load_library()
        assert lib.thr_tdoamatrix and lib.thr_tdmat_fetch and lib.thr_debug_tdoamatrix_geometry


def test_build_lists_and_the_one_statement_of_the_task():
    assert "tdoamatrix.hip" in build.SOURCES and "tdoa_task.hpp" in build.HEADERS
    assert build.UNPROFILED_TDMAT == ("tdoamatrix.hip", "tdoa_task.hpp")
    assert build.PER_FILE_FLAGS["tdoamatrix.hip"] == ["-ffp-contract=off"] == build.PER_FILE_FLAGS["tdoa.hip"]
    sources = {name: open(os.path.join(build.CSRC, name)).read() for name in ("tdoa.hip", "tdoamatrix.hip", "tdoa_task.hpp")}
    for name in ("tdoa.hip", "tdoamatrix.hip"):
        assert '#include "tdoa_task.hpp"' in sources[name] and "#pragma clang fp contract(off)" in sources[name]
        assert "0.6745" not in sources[name] and "wave_median" not in sources[name].replace("wave_median and the task", ""), name
    assert sources["tdoa_task.hpp"].count("0.6745 * w.value(i) / mad > 3.5") == 1
    assert "atomic" not in sources["tdoamatrix.hip"].replace("No floating-point atomic", "").replace("no atomics", "")


def test_csrc_hash_does_not_see_the_new_files(monkeypatch):
    before = build.csrc_hash()
    monkeypatch.setattr(build, "UNPROFILED_TDMAT", ())
    assert build.csrc_hash() != before                  # it does see them once the list is emptied
    monkeypatch.undo()
    assert build.csrc_hash() == before
    import json
    with open(os.path.join(ROOT, "profiles", "hbm_traffic.json")) as f:
        recorded = json.load(f)
    assert before in json.dumps(recorded)               # the recorded hash still holds
