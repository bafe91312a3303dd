#!/usr/bin/env python
"""Measure, on the CPU, how far float64 lies from the truth for every scene of tests/track_scenes.py, and write
tests/golden/track_tolerances.json.

    python tests/golden/make_golden_track.py

Per scene and per output (filt, filt_var, smooth, smooth_var, nis) the recorded value is the larger of
|sequential float64 - longdouble| and |scan-form float64 - longdouble| (tests/track_ref.py), the longdouble run being
the sequential recursion.  A test allows the device 16 times that, and never less than 16 ulp of the column's largest
magnitude: the factor covers another association order and the absence of fused multiply-adds.  The device's output
plays no part in the numbers.  The three runs must agree on the masks and the rounds (the script stops otherwise:
pick another seed), so the difference is arithmetic alone.

The scenes of track_scenes.clauses() are measured with a third float64 form beside the two, the device's own tree
(form="tiles": 256-row tiles, carries walked between fragments), and with the options of their call.  A regime is
recorded ungated (gate 0, one run) and carries `gated`: whether it is ALSO compared with the gate, which it is only if
the four runs agree on the mask of every round, no nis of any of them lies within a relative 1e-6 of the gate and the
gated record meets the condition below as well; the gated record is then `with_gate`, and otherwise `not_gated` says
why.  These scenes are recorded column by column (`columns`), and every column's bound is held against what the column
is measured by (`scales`, `judge`): below 1e-3 of it, so that no bound can hide an error of the size of the quantity.
A scene whose POSITIONS miss that stops the script: it belongs to track_scenes.OUT_OF_RANGE, whose regimes are
printed, recorded under `out_of_range` and are in no test.  Another column that misses it is recorded under the
scene's `not_compared` with its numbers, and a test compares the scene's other columns."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import track_check  # noqa: E402  (bound: what a test allows from a record)
import track_ref  # noqa: E402
import track_scenes  # noqa: E402

OUTPUTS = ("filt", "filt_var", "smooth", "smooth_var", "nis")


FORMS = (("ld", np.longdouble, "sequential"), ("seq", np.float64, "sequential"), ("scan", np.float64, "scan"))
TILES = (("tiles", np.float64, "tiles"),)
MARGIN, USEFUL = 1e-6, 1e-3


def measure(s, gate=track_ref.GATE_999, max_rounds=4, forms=FORMS, keep=None):
    runs = {}
    for name, kind, form in forms:
        runs[name] = track_ref.run(*track_scenes.columns(s), q=s["q"], v0=s["v0"], gate=gate, max_rounds=max_rounds, kind=kind,
                                   form=form)
    ld = runs["ld"]
    record = {"rows": int(len(s["tx"])), "rounds": ld["counts"]["rounds"], "converged": ld["counts"]["converged"]}
    if keep is not None:
        keep.update(runs)
    others = [name for name, _, _ in forms[1:]]
    for name in others:
        if not np.array_equal(runs[name]["used"], ld["used"]) or runs[name]["counts"] != ld["counts"]:
            raise SystemExit("the %s run disagrees with longdouble on the mask: pick another seed" % name)
    for key in OUTPUTS:
        worst = 0.0
        for name in others:
            a, b = runs[name][key].astype(np.longdouble), ld[key]
            if not np.array_equal(np.isnan(a), np.isnan(b)):
                raise SystemExit("%s: NaN pattern of %s differs" % (name, key))
            if a.size and not np.all(np.isnan(a)):
                worst = max(worst, float(np.nanmax(np.abs(a - b))))
        record[key] = worst
    return record


def measure_columns(runs, record):
    """record["columns"][key][col]: the same distance column by column, which is what a test of a clause scene allows
    16 times of; the per-form distances of the same, for the text of DESIGN.md."""
    ld, forms = runs["ld"], [name for name in runs if name != "ld"]
    per_form = {}
    for key in OUTPUTS:
        truth = ld[key].reshape(len(ld[key]), -1)
        per_form[key] = []
        for col in range(truth.shape[1]):
            if np.all(np.isnan(truth[:, col])):
                per_form[key].append({name: 0.0 for name in forms})
                continue
            per_form[key].append({name: float(np.nanmax(np.abs(runs[name][key].reshape(len(truth), -1)[:, col].astype(np.longdouble)
                                                                - truth[:, col]))) for name in forms})
    record["columns"] = {key: [max(one.values()) for one in per_form[key]] for key in OUTPUTS}
    assert all(max(record["columns"][key], default=0.0) == record[key] for key in OUTPUTS)
    return per_form


def smallest_sigma(s):
    on = s["valid"].astype(bool)
    return float(np.sqrt(min(s["rx"][on].min(), s["ry"][on].min())))


def scales(s, ld):
    """What an error in a column is to be small against, per output and column, from the scene and the longdouble run:
    a position against the smallest measurement sigma; a variance against the smallest value that variance takes, the
    covariance of position and velocity against the smallest sqrt(pp vv) (an error of a correlation coefficient); a
    velocity against the smallest velocity sigma sqrt(vv) of the same output; nis, a chi-square of two degrees, against 1."""
    out = {"nis": [1.0]}
    for key in ("filt", "smooth"):
        var = np.abs(ld[key + "_var"].astype(np.float64))
        var = var[np.all(np.isfinite(var), axis=1)]
        out[key], out[key + "_var"] = [], []
        for axis in range(2):
            pp, vv = var[:, 3 * axis], var[:, 3 * axis + 2]
            out[key] += [smallest_sigma(s), float(np.sqrt(vv.min()))]
            out[key + "_var"] += [float(pp.min()), float(np.sqrt(pp * vv).min()), float(vv.min())]
    return out


def judge(s, record, runs, per_form):
    """The usefulness condition: the bound a test allows on a column (track_check.bound: 16 times the record, never
    below 16 ulp of the column's largest magnitude) is below USEFUL = 1e-3 of the column's scale, so that it can never
    hide an error of the size of the quantity.  Fills `position_bound`, `smallest_sigma` and `not_compared`; -> whether
    the POSITIONS meet it (a scene whose positions do not is in no test).  Another column that fails it is listed in
    `not_compared` with its numbers -- bound, scale, each form's distance from longdouble and the lowest value each
    form returns in it -- and a test checks its NaN pattern alone."""
    ld, scale = runs["ld"], scales(s, runs["ld"])
    record["position_bound"], record["smallest_sigma"], record["not_compared"] = 0.0, smallest_sigma(s), {}
    for key in OUTPUTS:
        truth = ld[key].reshape(len(ld[key]), -1).astype(np.float64)
        for col in range(truth.shape[1]):
            limit = track_check.bound(record["columns"][key][col], truth[:, col])
            if key in ("filt", "smooth") and col % 2 == 0:
                record["position_bound"] = max(record["position_bound"], limit)
            elif not limit < USEFUL * scale[key][col]:
                lowest = {name: float(np.nanmin(run[key].reshape(len(truth), -1)[:, col])) for name, run in runs.items()}
                record["not_compared"]["%s[%d]" % (key, col)] = {"bound": limit, "scale": scale[key][col],
                                                                 "distance": per_form[key][col], "lowest": lowest}
    return record["position_bound"] < USEFUL * record["smallest_sigma"]


def gate_is_safe(runs):
    """Every run made the same rounds with the same masks, and no nis of any run lies at the gate."""
    first = runs["ld"]
    for run in runs.values():
        if len(run["masks"]) != len(first["masks"]) or not all(np.array_equal(a, b) for a, b in zip(run["masks"], first["masks"])):
            return False
        for nis in run["nis_rounds"]:
            finite = nis[np.isfinite(nis)].astype(np.float64)
            if len(finite) and np.min(np.abs(finite / track_ref.GATE_999 - 1.0)) <= MARGIN:
                return False
    return True


def measure_gated(s):
    """A regime with the default gate -> (record, None), or (None, why it is not compared with the gate)."""
    runs = {}
    try:
        record = measure(s, forms=FORMS + TILES, keep=runs)
    except SystemExit as stop:
        return None, str(stop)
    if not gate_is_safe(runs):
        return None, "the runs disagree on a round's mask or a nis lies at the gate"
    if not judge(s, record, runs, measure_columns(runs, record)):
        return None, "a position bound of %.3e m is not below 1e-3 of the smallest sigma" % record["position_bound"]
    return record, None


def measure_clause(name, s, options):
    """One scene of track_scenes.clauses(): the record of its call over the three float64 forms.  `gated`: whether a
    test calls it with the gate -- its own call for a scene that is no regime; for a regime, recorded without, whether
    it is compared with the default gate as well (`with_gate`), and if not, why (`not_gated`, printed too)."""
    runs = {}
    record = measure(s, forms=FORMS + TILES, keep=runs, **options)
    if name in track_scenes.REGIMES:
        assert options == dict(gate=0.0) and record["rounds"] == 1
        gated, why = measure_gated(s)
        record["gated"] = gated is not None
        if gated is not None:
            record["with_gate"] = gated
        else:
            record["not_gated"] = why
            print("%s is not compared with the gate: %s" % (name, why))
    else:
        record["gated"] = options.get("gate", track_ref.GATE_999) > 0.0
        if record["gated"] and not gate_is_safe(runs):
            raise SystemExit("%s: the runs disagree on a round's mask or a nis lies at the gate: pick another seed" % name)
    if not judge(s, record, runs, measure_columns(runs, record)):
        raise SystemExit("%s: a position bound of %.3e m is not below 1e-3 of the smallest sigma, %.3e m: the regime "
                         "belongs to track_scenes.OUT_OF_RANGE" % (name, record["position_bound"], record["smallest_sigma"]))
    return record


def measure_out_of_range(name, knobs):
    """The forms one by one (they need not agree with each other here): the distance of each from longdouble."""
    s = track_scenes.regime(knobs)
    runs = {label: track_ref.run(*track_scenes.columns(s), q=s["q"], v0=s["v0"], gate=0.0, kind=kind, form=form)
            for label, kind, form in FORMS + TILES}
    record = {"smallest_sigma": smallest_sigma(s)}
    for label in ("seq", "scan", "tiles"):
        record[label] = {key: float(np.nanmax(np.abs(runs[label][key].astype(np.longdouble) - runs["ld"][key]))) for key in OUTPUTS}
    record["position_bound"] = max(track_check.bound(max(record[label][key] for label in ("seq", "scan", "tiles")),
                                                     runs["ld"][key][:, col].astype(np.float64))
                                   for key in ("filt", "smooth") for col in (0, 2))
    if record["position_bound"] < USEFUL * record["smallest_sigma"]:
        raise SystemExit("%s meets the condition: it belongs to track_scenes.REGIMES" % name)
    return record


def main():
    table = {}
    for k in range(3):
        table["gating_%d" % k] = measure(track_scenes.gating(k))
    table["gating_1_no_gate"] = measure(track_scenes.gating(1), gate=0.0)
    table["gating_0_one_round"] = measure(track_scenes.gating(0), max_rounds=1)
    for name, s in track_scenes.seams().items():
        table[name] = measure(s)
    for name, (s, options) in track_scenes.clauses().items():
        table[name] = measure_clause(name, s, options)
    out_of_range = {name: measure_out_of_range(name, knobs) for name, knobs in track_scenes.OUT_OF_RANGE.items()}
    with open(os.path.join(HERE, "track_tolerances.json"), "w") as f:
        json.dump({"longdouble_bits": int(np.finfo(np.longdouble).nmant) + 1, "factor": track_check.FACTOR, "scenes": table,
                   "out_of_range": out_of_range}, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, record in list(table.items()) + list(out_of_range.items()):
        print(name, record)


if __name__ == "__main__":
    main()
