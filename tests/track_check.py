"""What the two GPU test files of thr_track share: the device call on a scene, the reference (computed once per
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
FACTOR = TOLERANCES["factor"]
EPS = np.finfo(np.float64).eps
FLOATS = ("filt", "filt_var", "smooth", "smooth_var", "nis")
EXACT = ("order", "track_tx", "track_ptr", "used", "track_flags")


def device(s, gate=track_ref.GATE_999, max_rounds=4):
    return _native.track(*track_scenes.columns(s)[:6], valid=s["valid"], q=s["q"], v0=s["v0"], gate=gate, max_rounds=max_rounds)


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


def compare(name, counts, out, ref, check_stats=True):
    """Every fetched array against the reference: integers exact, floats within the scene's recorded tolerance."""
    record = TOLERANCES["scenes"][name]
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
            limit = bound(record[key], y)
            worst[key, col] = (err, limit)
            print("%s %s[%d]: |device - reference| = %.3e, allowed %.3e" % (name, key, col, err, limit))
            assert err <= limit, (key, col, err, limit)
    if check_stats:
        compare_stats(name, out, ref)
    return worst


def compare_stats(name, out, ref):
    """rows, valid, used, rejected and the duration (one subtraction of two inputs) exact.  A sum of n terms in
    another order differs by at most n eps times the sum of the magnitudes, and every term carries its own bound:
    a nis the nis bound, a distance between two smoothed positions 2 sqrt(2) position bounds, a speed sqrt(2)
    velocity bounds."""
    record = TOLERANCES["scenes"][name]
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
