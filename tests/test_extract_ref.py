"""tests/extract_ref.py, the reference the extraction's GPU tests lean on, against the committed
fixtures and hand-made record arrays.  No GPU needed."""
import numpy as np
import pytest

import conftest
import extract_ref
from thrifty_amd import _native as F

FIXTURES = ["extract_1024", "extract_2048", "extract_16384"]


def records(energy, offset, corr=None):
    rec = np.zeros(len(energy), dtype=F.RECORD_DTYPE)
    rec["block_idx"] = np.arange(len(energy))
    rec["corr_energy"] = energy
    rec["corr_offset"] = offset
    corr = np.ones(len(energy), bool) if corr is None else np.asarray(corr, bool)
    rec["flags"] = np.where(corr, F.FLAG_CARRIER | F.FLAG_CORR, F.FLAG_CARRIER)
    return rec


@pytest.mark.parametrize("name", FIXTURES)
def test_expected_pick_gives_the_stored_picks_of_the_fixtures(name):
    g = conftest.load_golden("template_extract/" + name)
    rec = records(g["energy"], g["soff"], g["det"])
    rec["corr_sample"] = g["sample"]
    for pick in ("", "2"):
        want = (int(g["chosen" + pick]), int(g["n_qualifying" + pick]))
        assert extract_ref.expected_pick(rec, float(g["max_offset" + pick])) == want
    assert extract_ref.expected_pick(rec, 0.0) is None
    k, w = int(g["chosen"]), len(g["template"])
    assert np.max(np.abs(extract_ref.expected_template(g["blocks"][k], g["sample"][k], w) - g["template_ref"])) <= 1e-13


def test_of_equal_energies_the_first_is_picked():
    rec = records([3.0, 7.5, 1.0, 7.5, 7.5, 2.0], np.zeros(6))
    assert extract_ref.expected_pick(rec, 0.2) == (1, 6)
    assert extract_ref.expected_pick(rec[2:], 0.2) == (1, 4)           # positions count from the run's start
    rec["corr_offset"][1] = 0.3
    assert extract_ref.expected_pick(rec, 0.2) == (3, 5)
    # energies are compared as float32: two doubles that round to one float32 tie
    rec = records([1.0, 1.0 + 2.0 ** -30], np.zeros(2))
    assert extract_ref.expected_pick(rec, 0.2) == (0, 2)


def test_the_limit_is_inclusive():
    limit = float(np.float64(np.float32(0.123)))
    for sign in (1.0, -1.0):
        rec = records([1.0, 5.0, 2.0], [0.0, sign * limit, 0.01])
        assert extract_ref.expected_pick(rec, limit) == (1, 3)
        assert extract_ref.expected_pick(rec, np.nextafter(limit, 0)) == (2, 2)
        assert extract_ref.expected_pick(rec, np.nextafter(limit, 1)) == (1, 3)
    assert extract_ref.expected_pick(records([4.0], [0.0]), 0.0) == (0, 1)
    assert extract_ref.expected_pick(records([4.0], [5e-324]), 0.0) is None


def test_a_record_without_the_corr_flag_is_never_picked():
    rec = records([1e30, 2.0, np.inf, 1.0], np.zeros(4), corr=[False, True, False, True])
    assert extract_ref.expected_pick(rec, 0.2) == (1, 2)
    rec["flags"][[0, 2]] = F.FLAG_CARRIER | F.FLAG_INDEX_ERROR | F.FLAG_INT_OFFSET | F.FLAG_FIT_UNCONVERGED
    assert extract_ref.expected_pick(rec, 0.2) == (1, 2)
    assert extract_ref.expected_pick(rec[[0, 2]], 0.2) is None
    assert extract_ref.expected_pick(rec[:0], 0.2) is None


def test_window_of_is_the_generators_arithmetic():
    assert extract_ref.window_of(1024, 512, 127) == (193, 705)          # (the window test 6 of the GPU suite uses)
    lo, hi = extract_ref.window_of(2048, 1024, 256)
    assert (lo, hi) == (384, 1408) and hi - lo == 2048 - 1024
    lo, hi = extract_ref.window_of(2048, 1024, 512)
    assert (lo, hi) == (256, 1280) and hi + 512 <= 2048
