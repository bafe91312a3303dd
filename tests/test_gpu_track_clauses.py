"""`thr_track` at the clauses of its definition that no seam reaches (tests/track_scenes.py: clauses()): tracks that
an outlier on the start row loses, so that THR_TRACK_LOST is 1 on the device, at `2 used == valid` and one below, in
a call that does not converge and in one that needs thirteen filter runs; timestamps below zero, -0.0 beside 0.0 and
transmitter ids at the ends of int32 through the sort key; q from 0 to 1e4, v0 from 1e-3 to 1e5, variances times 1e-8
and 1e8, coordinates of a UTM northing, steps of hours, duplicate timestamps without process noise and a 400-row gap,
each on a track of three fragments; the call without the `valid` column; and a track beside a neighbour that forces
many more rounds or leaves the call unconverged.  Against tests/track_ref.py within the tolerance recorded per scene
(tests/golden/make_golden_track.py: the largest CPU error over the recursion, the balanced tree and the device's own
tiles and carries, column by column, times 16), integers exact.  Eight columns of three regimes whose bound says
nothing, because float64 itself is far from longdouble there, are named in the record (`not_compared`)
and have their NaN pattern checked alone.  What each scene must hold is asserted on the reference first."""
import numpy as np
import pytest

import track_check
import track_ref
import track_scenes
from thrifty_amd import _native

pytestmark = pytest.mark.gpu

RECORDS = track_check.TOLERANCES["scenes"]
REGIMES = sorted(track_scenes.REGIMES)
GATED = [name for name in REGIMES if RECORDS[name]["gated"]]
PER_ROW = ("used", "nis", "filt", "filt_var", "smooth", "smooth_var")


def _against_the_reference(name, with_gate=False):
    track_check.assert_clause_holds(name)
    s, options, ref, record = track_check.clause(name, with_gate)
    if options.get("gate", track_ref.GATE_999) > 0.0:
        track_check.assert_margin(ref)
    counts, out = track_check.device(s, **options)
    for key in track_check.FLOATS:      # finite wherever the reference is
        assert np.array_equal(np.isfinite(out[key]), np.isfinite(ref[key])), key
    track_check.compare(name, counts, out, ref, record=record)
    return s, ref, counts, out


def test_the_geometry_the_scenes_are_cut_for():
    assert _native.track_geometry() == (track_ref.TILE, 256, 14)


@pytest.mark.parametrize("name", track_check.LOST_SCENES)
def test_a_lost_track_is_flagged_and_one_that_is_not_lost_is_not(name):
    s, ref, counts, out = _against_the_reference(name)
    assert counts == ref["counts"]
    assert out["track_flags"].tolist() == ref["track_flags"].tolist() and {0, _native.TRACK_LOST} == set(out["track_flags"].tolist())
    assert np.array_equal(out["track_stats"][:, :4], ref["track_stats"][:, :4])


def test_timestamps_below_zero_sort_in_time_order():
    s, ref, counts, out = _against_the_reference("neg_times")
    assert np.array_equal(out["order"], ref["order"]) and np.all(np.diff(s["timestamp"][out["order"]][:300]) > 0.0)
    # its timestamps are distinct: shuffled rows return the same bytes per row
    perm = np.random.default_rng(2).permutation(len(s["tx"]))
    shuffled = {key: (value[perm] if isinstance(value, np.ndarray) else value) for key, value in s.items()}
    cb, b = track_check.device(shuffled)
    assert cb == counts
    for key in PER_ROW:
        assert out[key][perm].tobytes() == b[key].tobytes(), key
    for key in ("track_tx", "track_ptr", "track_stats", "track_flags"):
        assert out[key].tobytes() == b[key].tobytes(), key
    assert np.array_equal(perm[b["order"]], out["order"])


def test_minus_zero_and_zero_are_one_key_and_keep_their_input_order():
    s, ref, counts, out = _against_the_reference("signed_zero")
    order, track_tx, track_ptr = track_ref.sort_rows(s["tx"], s["timestamp"])
    assert np.array_equal(out["order"], order) and np.array_equal(out["track_ptr"], track_ptr)
    for tx in (3, 5):
        rows = np.flatnonzero((s["tx"] == tx) & (s["timestamp"] == 0.0))
        at = [int(np.flatnonzero(out["order"] == row)[0]) for row in rows]
        assert len(rows) == 2 and at[1] == at[0] + 1


def test_transmitter_ids_at_the_ends_of_int32_ascend_across_the_sign():
    s, ref, counts, out = _against_the_reference("tx_extremes")
    assert out["track_tx"].tolist() == [-2 ** 31, -1, 0, 2 ** 31 - 1] and out["track_ptr"].tolist() == [0, 70, 140, 210, 280]
    assert np.array_equal(s["tx"][out["order"]], np.repeat(out["track_tx"], 70))


@pytest.mark.parametrize("name", REGIMES)
def test_a_regime_without_the_gate(name):
    s, ref, counts, out = _against_the_reference(name)
    assert counts["rounds"] == 1 and counts["converged"] == 1 and counts["rejected"] == 0


@pytest.mark.parametrize("name", GATED)
def test_a_regime_with_the_gate(name):
    _against_the_reference(name, with_gate=True)


def test_every_regime_says_whether_it_runs_gated():
    assert all(isinstance(RECORDS[name]["gated"], bool) for name in REGIMES) and GATED == REGIMES and len(REGIMES) == 11


def test_without_the_valid_column_every_row_is_valid():
    s, ref, counts, out = _against_the_reference("all_valid")
    track_check.same_bytes((counts, out), track_check.device(s, with_valid=False))


@pytest.mark.parametrize("name", track_check.LOAD_SCENES)
def test_a_converged_track_beside_one_that_needs_many_more_rounds_returns_its_own_bytes(name):
    s, ref, counts, out = _against_the_reference(name)      # B, and A too, against the reference
    alone, alone_ref = track_check.load_alone()
    ca, a = track_check.device(alone)
    assert ca == alone_ref["counts"] and ca["converged"] == 1
    assert (counts["rounds"] >= ca["rounds"] + 4 and counts["converged"] == 1) if name == "under_load_16" else counts["converged"] == 0
    for key in PER_ROW:
        assert a[key].tobytes() == out[key][40:].tobytes(), key
    assert a["track_stats"].tobytes() == out["track_stats"][:1].tobytes() and a["track_flags"][0] == out["track_flags"][0] == 0
    assert np.array_equal(out["order"][:700] - 40, a["order"]) and out["track_flags"][1] == _native.TRACK_LOST
