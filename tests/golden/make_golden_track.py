#!/usr/bin/env python
"""Measure, on the CPU, how far float64 lies from the truth for every scene of tests/track_scenes.py, and write
tests/golden/track_tolerances.json.

    python tests/golden/make_golden_track.py

Per scene and per output (filt, filt_var, smooth, smooth_var, nis) the recorded value is the larger of
|sequential float64 - longdouble| and |scan-form float64 - longdouble| (tests/track_ref.py), the longdouble run being
the sequential recursion.  A test allows the device 16 times that, and never less than 16 ulp of the column's largest
magnitude: the factor covers another association order and the absence of fused multiply-adds.  The device's output
plays no part in the numbers.  The three runs must agree on the masks and the rounds (the script stops otherwise:
pick another seed), so the difference is arithmetic alone."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import track_ref  # noqa: E402
import track_scenes  # noqa: E402

OUTPUTS = ("filt", "filt_var", "smooth", "smooth_var", "nis")


def measure(s, gate=track_ref.GATE_999, max_rounds=4):
    runs = {}
    for name, kind, form in (("ld", np.longdouble, "sequential"), ("seq", np.float64, "sequential"), ("scan", np.float64, "scan")):
        runs[name] = track_ref.run(*track_scenes.columns(s), q=s["q"], v0=s["v0"], gate=gate, max_rounds=max_rounds, kind=kind,
                                   form=form)
    ld = runs["ld"]
    record = {"rows": int(len(s["tx"])), "rounds": ld["counts"]["rounds"], "converged": ld["counts"]["converged"]}
    for name in ("seq", "scan"):
        if not np.array_equal(runs[name]["used"], ld["used"]) or runs[name]["counts"] != ld["counts"]:
            raise SystemExit("the %s run disagrees with longdouble on the mask: pick another seed" % name)
    for key in OUTPUTS:
        worst = 0.0
        for name in ("seq", "scan"):
            a, b = runs[name][key].astype(np.longdouble), ld[key]
            if not np.array_equal(np.isnan(a), np.isnan(b)):
                raise SystemExit("%s: NaN pattern of %s differs" % (name, key))
            if a.size and not np.all(np.isnan(a)):
                worst = max(worst, float(np.nanmax(np.abs(a - b))))
        record[key] = worst
    return record


def main():
    table = {}
    for k in range(3):
        table["gating_%d" % k] = measure(track_scenes.gating(k))
    table["gating_1_no_gate"] = measure(track_scenes.gating(1), gate=0.0)
    table["gating_0_one_round"] = measure(track_scenes.gating(0), max_rounds=1)
    for name, s in track_scenes.seams().items():
        table[name] = measure(s)
    with open(os.path.join(HERE, "track_tolerances.json"), "w") as f:
        json.dump({"longdouble_bits": int(np.finfo(np.longdouble).nmant) + 1, "factor": 16, "scenes": table}, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, record in table.items():
        print(name, record)


if __name__ == "__main__":
    main()
