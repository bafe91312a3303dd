"""Host side of `match` (no GPU): the sequential statement tests/match_ref.py against the fixtures the
reference's own `match_toads` produced (tests/golden/make_golden_match.py), the .match text format,
the command line's defaults, `extract_match_matrix`, and the wiring of `thr_match` into the header, the
symbol list and the build."""
import io
import os
import re

import numpy as np
import pytest

from match_ref import from_csr, match_ref, to_csr
from thrifty_amd import _native, build, matchmaker, toads_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "match")
SETS = ("match_realistic", "match_ties", "match_minmatch")


def golden_cases():
    for name in SETS:
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        for c in range(len(g["window"])):
            yield name, g, c


def detections(g):
    out = []
    for i in range(len(g["rxid"])):
        car = toads_data.CarrierSyncInfo(40, 0.1, 150.0, 7.5)
        cor = toads_data.CorrDetectionInfo(4000, 0.25, float(g["energy"][i]), 1.5)
        out.append(toads_data.DetectionResult(float(g["timestamp"][i]), i, 12288.0 * i, car, cor,
                                              rxid=int(g["rxid"][i]), txid=int(g["txid"][i])))
    return out


def test_fixtures_are_what_the_issue_asks_for():
    sizes = {name: len(np.load(os.path.join(GOLDEN, name + ".npz"))["rxid"]) for name in SETS}
    assert 550 <= sizes["match_realistic"] <= 700 and 350 <= sizes["match_ties"] <= 450
    g = np.load(os.path.join(GOLDEN, "match_minmatch.npz"))
    assert g["min_match"].tolist() == [1, 3]
    ties = np.load(os.path.join(GOLDEN, "match_ties.npz"))
    assert -1 in ties["txid"] and set(ties["energy"].tolist()) == {1.0, 2.0, 3.0}
    assert np.all(np.diff(ties["timestamp"]) >= 0) and ties["window"].tolist() == [0.0, 0.25, 0.5, 1.0]
    for name in SETS:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 100 * 1024
        assert sum(len(g2["c%d_collisions" % c]) for n2, g2, c in golden_cases() if n2 == name) > 0


@pytest.mark.parametrize("name,c", [(name, c) for name, _, c in golden_cases()])
def test_match_ref_equals_the_reference(name, c):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    matches, misses, collisions = match_ref(g["rxid"], g["txid"], g["timestamp"], g["energy"],
                                            g["window"][c], int(g["min_match"][c]))
    ptr, idx = to_csr(matches)
    assert ptr == g["c%d_match_ptr" % c].tolist() and idx == g["c%d_match_idx" % c].tolist()
    assert misses == g["c%d_misses" % c].tolist()
    assert [list(p) for p in collisions] == g["c%d_collisions" % c].tolist()


def test_match_file_round_trip(tmp_path):
    matches = [[0, 3, 5], [7, 2], [11]]
    text = io.StringIO()
    matchmaker.save_matches(matches, text)
    assert text.getvalue() == "0 3 5\n7 2\n11\n"
    assert matchmaker.load_matches(io.StringIO(text.getvalue())) == matches
    path = tmp_path / "data.match"
    path.write_text("# made by a test\n0 3 5\n\n7 2\n   \n#9 9\n11\n")
    assert matchmaker.load_matches(str(path)) == matches
    with open(str(path), "rb") as handle:
        assert matchmaker.load_matches(handle) == matches
    empty = io.StringIO()
    matchmaker.save_matches([], empty)
    assert empty.getvalue() == "" and matchmaker.load_matches(io.StringIO("")) == []


def test_cli_defaults_are_the_references():
    parser = matchmaker._parser()
    assert parser.get_default("input") == "data.toads" and parser.get_default("output") == "data.match"
    assert parser.get_default("window") == 0.2 and parser.get_default("num_matches") == 2
    assert parser.get_default("verbose") is False
    flags = {s for a in parser._actions for s in a.option_strings}
    assert {"-o", "--output", "-w", "--window", "-n", "--num-matches", "-v", "--verbose"} <= flags


@pytest.mark.parametrize("name,c", [(name, c) for name, _, c in golden_cases()])
def test_extract_match_matrix_equals_the_reference(name, c):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    dets = detections(g)
    matches = from_csr(g["c%d_match_ptr" % c], g["c%d_match_idx" % c])
    rxids, txids = g["matrix_rxids"].tolist(), g["matrix_txids"].tolist()
    assert matchmaker.extract_match_matrix(dets, matches, rxids) == g["c%d_matrix" % c].tolist()
    assert matchmaker.extract_match_matrix(dets, matches, rxids, txids) == g["c%d_matrix_tx" % c].tolist()
    assert len(g["c%d_matrix_tx" % c]) < len(g["c%d_matrix" % c])
    assert matchmaker.extract_match_matrix(dets, matches, [99]) == []


def test_none_ids_become_minus_one():
    car, cor = toads_data.CarrierSyncInfo(40, 0.1, 150.0, 7.5), toads_data.CorrDetectionInfo(4000, 0.25, 9.5, 1.5)
    dets = [toads_data.DetectionResult(1.5, 0, 0.0, car, cor), toads_data.DetectionResult(2.5, 1, 0.0, car, cor, 3, 4)]
    cols = matchmaker._columns(dets)
    assert cols["rxid"].tolist() == [-1, 3] and cols["txid"].tolist() == [-1, 4]
    assert cols["timestamp"].tolist() == [1.5, 2.5] and cols["energy"].tolist() == [9.5, 9.5]
    assert cols["rxid"].dtype == np.int32 and cols["txid"].dtype == np.int32


def test_thr_match_is_declared_listed_and_built():
    header = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
    assert re.search(r"\bint thr_match\(int device_id, size_t n,", header)
    assert "#define THR_ABI_VERSION 11" in header and _native.ABI_VERSION == 11
    assert "thr_match" in _native.EXPORTS and callable(_native.match)
    assert "match.hip" in build.SOURCES and set(build.UNPROFILED_MATCH) == {"match.hip"}
    source = open(os.path.join(build.CSRC, "match.hip")).read()
    assert int(re.search(r"constexpr int kBlock = (\d+);", source).group(1)) == _native.MATCH_WORKGROUP
    if os.path.exists(_native.LIB_PATH):
        lib = _native.load_library()
        assert lib.thr_match and lib.thr_debug_match_times
