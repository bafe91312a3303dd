"""`match` on the device against the fixtures the reference's `match_toads` produced
(tests/golden/make_golden_match.py): matches, misses and collisions equal element for element, in
order -- through `_native.match` on columns, through `matchmaker.match_toads` on DetectionResult
objects and through the command line on a written .toads file."""
import os
import sys

import numpy as np
import pytest

from match_ref import from_csr
from thrifty_amd import _native, matchmaker, toads_data

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "match")
CASES = [("match_realistic", 0), ("match_ties", 0), ("match_ties", 1), ("match_ties", 2), ("match_ties", 3),
         ("match_minmatch", 0), ("match_minmatch", 1)]


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def detections(g):
    out = []
    for i in range(len(g["rxid"])):
        car = toads_data.CarrierSyncInfo(40 + int(g["txid"][i]), 0.1, 150.0, 7.5)
        cor = toads_data.CorrDetectionInfo(4000 + i % 97, 0.25, float(g["energy"][i]), 1.5)
        out.append(toads_data.DetectionResult(float(g["timestamp"][i]), i, 12288.0 * i, car, cor,
                                              rxid=int(g["rxid"][i]), txid=int(g["txid"][i])))
    return out


@pytest.mark.parametrize("name,c", CASES)
def test_columns_equal_the_reference(name, c):
    g = load(name)
    ptr, idx, misses, collisions = _native.match(g["rxid"], g["txid"], g["timestamp"], g["energy"],
                                                 g["window"][c], int(g["min_match"][c]))
    assert all(a.dtype == np.int64 for a in (ptr, idx, misses, collisions)) and collisions.ndim == 2
    np.testing.assert_array_equal(ptr, g["c%d_match_ptr" % c])
    np.testing.assert_array_equal(idx, g["c%d_match_idx" % c])
    np.testing.assert_array_equal(misses, g["c%d_misses" % c])
    np.testing.assert_array_equal(collisions, g["c%d_collisions" % c])


@pytest.mark.parametrize("name,c", CASES)
def test_match_toads_equals_the_reference(name, c):
    g = load(name)
    matches, misses, collisions = matchmaker.match_toads(detections(g), float(g["window"][c]), int(g["min_match"][c]))
    assert matches == from_csr(g["c%d_match_ptr" % c], g["c%d_match_idx" % c])
    assert misses == g["c%d_misses" % c].tolist()
    assert collisions == [tuple(p) for p in g["c%d_collisions" % c].tolist()]
    assert all(isinstance(i, int) for m in matches for i in m) and all(isinstance(p, tuple) for p in collisions)


@pytest.mark.parametrize("name,c", [("match_realistic", 0), ("match_ties", 2), ("match_minmatch", 1)])
def test_command_line_writes_the_references_lines(name, c, tmp_path, capsys):
    g = load(name)
    dets = detections(g)
    toads, out = tmp_path / "data.toads", tmp_path / "data.match"
    toads.write_text("# source_files: [a.toad b.toad]\n" + "".join(d.serialize() + "\n" for d in dets))
    matchmaker._main([str(toads), "-o", str(out), "-w", repr(float(g["window"][c])), "-n", str(g["min_match"][c]), "-v"])
    want = from_csr(g["c%d_match_ptr" % c], g["c%d_match_idx" % c])
    assert out.read_text() == "".join(" ".join(map(str, m)) + "\n" for m in want)
    assert matchmaker.load_matches(str(out)) == want
    printed = capsys.readouterr().out.splitlines()
    collisions = g["c%d_collisions" % c].tolist()
    assert printed[-3:] == ["Number of matches: %d" % len(want), "Number of misses: %d" % len(g["c%d_misses" % c]),
                            "Number of collisions: %d" % len(collisions)]
    a, b = collisions[0]
    assert printed[0] == ("Multiple detections for RX %d and TX %d: detection #%d and #%d collides."
                          % (g["rxid"][a], g["txid"][a], a, b))
    assert len(printed) == len(collisions) + 3


def test_command_line_sorts_by_timestamp_and_leaves_stdout_open(tmp_path, capsys):
    g = load("match_ties")
    dets = detections(g)
    order = np.random.default_rng(5).permutation(len(dets))
    toads = tmp_path / "shuffled.toads"
    toads.write_text("".join(dets[i].serialize() + "\n" for i in order))
    matchmaker._main([str(toads), "-o", "-", "-w", "0.5"])
    assert not sys.stdout.closed
    lines = capsys.readouterr().out.splitlines()
    # the shuffled file sorted stably by timestamp is another order of equal timestamps than the
    # fixture's: the counts need not be the fixture's, the lines must be what the sorted columns give
    rows = sorted((dets[i] for i in order), key=lambda d: d.timestamp)
    matches, misses, collisions = matchmaker.match_toads(rows, 0.5)
    assert lines[:3] == ["Number of matches: %d" % len(matches), "Number of misses: %d" % len(misses),
                         "Number of collisions: %d" % len(collisions)]
    assert [[int(w) for w in line.split()] for line in lines[3:]] == matches


def test_no_detections():
    ptr, idx, misses, collisions = _native.match([], [], [], [], 0.2)
    assert ptr.tolist() == [0] and len(idx) == 0 and len(misses) == 0 and collisions.shape == (0, 2)
    assert matchmaker.match_toads([], 0.2) == ([], [], [])


def test_unsorted_and_nan_timestamps_are_refused():
    rx, tx, en = [0, 1, 0, 1, 2], [0, 0, 0, 0, 0], [1.0] * 5
    with pytest.raises(ValueError, match="detection 3 "):
        _native.match(rx, tx, [0.0, 1.0, 2.0, 1.5, 1.75], en, 0.2)
    with pytest.raises(ValueError, match="detection 2 is NaN"):
        _native.match(rx, tx, [0.0, 1.0, float("nan"), 3.0, 2.0], en, 0.2)
    with pytest.raises(ValueError, match="detection 0 is NaN"):
        _native.match(rx, tx, [float("nan"), 1.0, 2.0, 3.0, 4.0], en, 0.2)
    ptr, _, _, _ = _native.match(rx, tx, [0.0, 1.0, 1.0, 1.0, 4.0], en, 0.2)       # equal neighbours are in order
    assert ptr.tolist() == [0, 2]
