"""What the GPU test files of thr_track share: the device call on a scene, the reference (computed once per
scene and shared), the gate's margin, and the comparison against the recorded tolerances."""
import functools
import json
import os

import numpy as np

import track_ref
import track_scenes
from thrifty_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLERANCES = json.load(open(os.path.join(ROOT, "tests", "golden", "track_tolerances.json")))
FACTOR = 16      # tests/golden/make_golden_track.py writes it into the file; tests/test_track_host.py compares
EPS = np.finfo(np.float64).eps
FLOATS = ("filt", "filt_var", "smooth", "smooth_var", "nis")
EXACT = ("order", "track_tx", "track_ptr", "used", "track_flags")


def device(s, gate=track_ref.GATE_999, max_rounds=4, with_valid=True):
    """with_valid=False: the call without the column (valid = NULL), for a scene whose rows are all valid."""
    assert with_valid or s["valid"].all()
    return _native.track(*track_scenes.columns(s)[:6], valid=s["valid"] if with_valid else None, q=s["q"], v0=s["v0"], gate=gate,
                         max_rounds=max_rounds)


def reference(s, gate=track_ref.GATE_999, max_rounds=4):
    return track_ref.run(*track_scenes.columns(s), q=s["q"], v0=s["v0"], gate=gate, max_rounds=max_rounds)


@functools.lru_cache(maxsize=None)
def gating(k):
    s = track_scenes.gating(k)
    return s, reference(s)


@functools.lru_cache(maxsize=None)
def gating_0_one_round():
    """The reference of gating(0) stopped after one round: the call that does not converge."""
    return reference(track_scenes.gating(0), max_rounds=1)


@functools.lru_cache(maxsize=None)
def seams():
    return track_scenes.seams()


@functools.lru_cache(maxsize=None)
def seam(name):
    s = seams()[name]
    return s, reference(s)


@functools.lru_cache(maxsize=None)
def clauses():
    return track_scenes.clauses()


@functools.lru_cache(maxsize=None)
def clause(name, with_gate=False):
    """scene, options of its call, reference, record.  with_gate: a regime (recorded ungated) with the default gate,
    which the record allows where it says `gated`."""
    s, options = clauses()[name]
    record = TOLERANCES["scenes"][name]
    if with_gate:
        assert name in track_scenes.REGIMES and record["gated"]
        options, record = {}, record["with_gate"]
    return s, options, reference(s, **options), record


def assert_margin(ref, gate=track_ref.GATE_999, margin=1e-6):
    """In every round no reference nis lies within a relative `margin` of the gate: otherwise a mask bit may
    legitimately differ between two correct float64 computations."""
    for nis in ref["nis_rounds"]:
        finite = nis[np.isfinite(nis)]
        if len(finite):
            assert np.min(np.abs(finite / gate - 1.0)) > margin


def bound(record_value, column):
    """16 times the recorded CPU error, never below 16 ulp of the column's largest magnitude."""
    finite = column[np.isfinite(column)]
    largest = float(np.max(np.abs(finite))) if len(finite) else 0.0
    return max(FACTOR * record_value, FACTOR * EPS * largest)


def compare(name, counts, out, ref, check_stats=True, record=None):
    """Every fetched array against the reference: integers exact, floats within the scene's recorded tolerance -- one
    number per output, or per column where the record has `columns` (the clause scenes).  A column that the record
    lists as `not_compared` (its bound says nothing: make_golden_track.py, judge) has its NaN pattern checked alone."""
    record = TOLERANCES["scenes"][name] if record is None else record
    assert counts == ref["counts"]
    for key in EXACT:
        assert out[key].dtype == _native.TRACK_OUTPUTS[key][1] and np.array_equal(out[key], ref[key]), key
    worst = {}
    for key in FLOATS:
        a, b = out[key], ref[key]
        assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), key
        for col in range(a.shape[1] if a.ndim == 2 else 1):
            x, y = (a[:, col], b[:, col]) if a.ndim == 2 else (a, b)
            if not np.any(np.isfinite(y)):
                continue
            err = float(np.nanmax(np.abs(x - y)))
            limit = bound(record["columns"][key][col] if "columns" in record else record[key], y)
            if "%s[%d]" % (key, col) in record.get("not_compared", {}):
                print("%s %s[%d]: |device - reference| = %.3e, not compared (a bound of %.3e)" % (name, key, col, err, limit))
                continue
            worst[key, col] = (err, limit)
            print("%s %s[%d]: |device - reference| = %.3e, allowed %.3e" % (name, key, col, err, limit))
            assert err <= limit, (key, col, err, limit)
    if check_stats:
        compare_stats(name, out, ref, record)
    return worst


def compare_stats(name, out, ref, record=None):
    """rows, valid, used, rejected and the duration (one subtraction of two inputs) exact.  A sum of n terms in
    another order differs by at most n eps times the sum of the magnitudes, and every term carries its own bound:
    a nis the nis bound, a distance between two smoothed positions 2 sqrt(2) position bounds, a speed sqrt(2)
    velocity bounds."""
    record = TOLERANCES["scenes"][name] if record is None else record
    a, b = out["track_stats"], ref["track_stats"]
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(a[:, :4], b[:, :4]) and np.array_equal(a[:, 5], b[:, 5], equal_nan=True)
    state = bound(record["smooth"], ref["smooth"])
    nis = bound(record["nis"], ref["nis"])
    for c in range(len(a)):
        n = b[c, 0]
        if np.isnan(b[c, 6]):
            continue
        limits = (nis + n * EPS * abs(b[c, 4]) if not np.isnan(b[c, 4]) else 0.0, None, 3.0 * n * state + n * EPS * b[c, 6],
                  1.5 * state + n * EPS * b[c, 7])
        for col in (4, 6, 7):
            if np.isnan(b[c, col]):
                continue
            err = abs(a[c, col] - b[c, col])
            print("%s track_stats[%d][%d]: |device - reference| = %.3e, allowed %.3e" % (name, c, col, err, limits[col - 4]))
            assert err <= limits[col - 4], (c, col, err)


def same_bytes(a, b):
    (ca, oa), (cb, ob) = a, b
    assert ca == cb
    for key in _native.TRACK_OUTPUTS:
        assert oa[key].tobytes() == ob[key].tobytes(), key


# ------------------------------------------------------------------ what the scenes of track_scenes.clauses() must hold
LOST_SCENES = ("lost_equal", "lost_one_below", "lost_unconverged", "lost_late", "lost_remedy")
KEY_SCENES = ("neg_times", "signed_zero", "tx_extremes")
LOAD_SCENES = ("under_load_16", "under_load_4")


@functools.lru_cache(maxsize=None)
def load_alone():
    """Track A of the independence scenes on its own."""
    a = track_scenes.load_pair()[0]
    return a, reference(a)


def assert_clause_holds(name):
    """On the reference alone: the scene reaches the clause it is named after.  tests/test_track_host.py runs this
    for every name without a device; the GPU tests run it before they call the device."""
    s, options, ref, record = clause(name)
    counts, stats, flags = ref["counts"], ref["track_stats"], ref["track_flags"].tolist()
    gate = options.get("gate", track_ref.GATE_999)
    assert len(s["tx"]) <= 1000 and counts["rounds"] == record["rounds"] and counts["converged"] == record["converged"]
    if gate > 0.0:
        assert_margin(ref)
    if name in LOST_SCENES or name in LOAD_SCENES:
        assert 1 in flags and 0 in flags
    if name == "lost_equal":      # 2 used == valid is not lost; the third track is
        assert flags == [0, 0, 1] and stats[1, 1:3].tolist() == [60, 30] and 2 * stats[1, 2] == stats[1, 1]
    elif name == "lost_one_below":
        assert flags == [0, 1] and stats[1, 1:3].tolist() == [61, 30] and 2 * stats[1, 2] == stats[1, 1] - 1
    elif name == "lost_unconverged":
        assert flags == [0, 1] and options["max_rounds"] == 4 and counts["converged"] == 0 and counts["rounds"] == 5
    elif name == "lost_late":
        assert flags == [0, 1] and options["max_rounds"] == 16 and counts["converged"] == 1 and counts["rounds"] >= 7
        earlier = reference(s, max_rounds=counts["rounds"] - 2)      # it is the lost track that needs the runs
        assert earlier["counts"]["converged"] == 0 and not np.array_equal(earlier["used"], ref["used"])
    elif name == "lost_remedy":      # the same start-row outlier in both tracks; the first has that row marked invalid
        assert flags == [0, 1] and stats[0, :4].tolist() == [40, 39, 39, 0]
        start = ref["order"][0]
        assert s["tx"][start] == 3 and s["valid"][start] == 0 and not ref["tracked"][start] and np.isnan(ref["filt"][start]).all()
    elif name == "neg_times":
        t = s["timestamp"][ref["order"]]
        assert ref["track_ptr"].tolist() == [0, 300, 500] and len(set(s["timestamp"].tolist())) == 500
        crossing = int(np.searchsorted(t[:300], 0.0))
        assert t[0] < -100.0 and t[299] > 100.0 and 0 < crossing % 256 < 255 and t[crossing - 1] < 0.0 < t[crossing]
        assert np.all(t[300:] < -1.4e9) and np.allclose(np.diff(t[300:]), 1e-3, atol=1e-6)
        assert not np.array_equal(ref["order"], np.arange(500))
    elif name == "signed_zero":
        for tx, signs in ((3, [True, False]), (5, [False, True])):      # the -0.0 row first in the input | second
            rows = np.flatnonzero((s["tx"] == tx) & (s["timestamp"] == 0.0))
            assert np.signbit(s["timestamp"][rows]).tolist() == signs
            at = [int(np.flatnonzero(ref["order"] == row)[0]) for row in rows]
            assert at[1] == at[0] + 1      # equal keys in their input order
    elif name == "tx_extremes":
        assert ref["track_tx"].tolist() == [-2 ** 31, -1, 0, 2 ** 31 - 1] and ref["track_ptr"].tolist() == [0, 70, 140, 210, 280]
        assert not np.array_equal(ref["order"], np.arange(280))
    elif name == "all_valid":
        assert s["valid"].all() and counts["tracks"] == 2 and counts["used"] <= 450
    elif name in LOAD_SCENES:
        alone = load_alone()[1]["counts"]
        assert flags == [0, 1] and ref["track_ptr"].tolist() == [0, 700, 740] and alone["converged"] == 1 and alone["rounds"] <= 4
        if name == "under_load_16":
            assert counts["converged"] == 1 and counts["rounds"] >= alone["rounds"] + 4
        else:
            assert counts["converged"] == 0 and counts["rounds"] == 5
    else:
        knobs = track_scenes.REGIMES[name]
        assert gate == 0.0 and counts["rounds"] == 1 and s["q"] == knobs.get("q", 0.25) and s["v0"] == knobs.get("v0", 10.0)
        assert ref["track_ptr"].tolist() == [0, 100, 700] and track_ref.fragments(100, 600) == [(0, 156), (156, 412), (412, 600)]
        on = ref["order"][100:]
        t, rx = s["timestamp"][on], s["rx"][on]
        for key in FLOATS[:4]:
            assert np.all(np.isfinite(ref[key]))
        if "r_scale" in knobs:
            assert np.all((rx > 2.0 * knobs["r_scale"]) & (rx < 40.0 * knobs["r_scale"]))
        if "offset" in knobs:
            assert np.all(s["x"][on] > 5.9e6) and np.all(s["y"][on] < -3.9e6)
        if "step" in knobs:
            assert np.median(np.diff(t)) > 1e3
        if "duplicates" in knobs:
            assert 250 <= np.count_nonzero(np.diff(t) == 0.0) <= 350
        if "invalid_ranges" in knobs:
            assert np.flatnonzero(s["valid"][ref["order"]] == 0).tolist() == list(range(200, 600))
    if record["gated"] and name in track_scenes.REGIMES:
        assert_margin(clause(name, True)[2])
