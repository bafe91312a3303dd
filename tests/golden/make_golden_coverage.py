#!/usr/bin/env python
"""Fixtures of `thr_coverage` (tests/golden/coverage/*.npz): small scenes and what the NumPy statement
(tests/coverage_ref.py) makes of them.  Nothing of the reference is read.

    python tests/golden/make_golden_coverage.py

ring5    5 receivers on a jittered ring of 100 m at the origin, 0.05 m of noise, 6 x 5 cells inside the ring, 70 trials:
         2100 pooled trials for the chi-square test of the prediction.
range6   6 receivers, range_m = 140 m over an area that reaches far beyond the ring: cells with 0, 2, 3, 4 and 6
         hearing receivers.
far4     the receivers of the posg fixture far4, centred on (5000, -3000) m: the fixed start (0.1, 0.1) loses cells,
         a start at the array's centre loses none (the statement's flags of both are recorded).
mixed5   one sigma per receiver, one of them 0.

The generator ASSERTS on the statement alone what the tests rely on, and records per cell whether its good / gross
decisions are SAFE to compare with the device's: every trial's |e - gross_m| exceeds 1e3 x the position tolerance the
pos fixtures record (a trial without a position, e = inf, is safe).  At most 5 % of the covered cells may be unsafe."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import coverage_golden  # noqa: E402
import coverage_ref  # noqa: E402

RECORDED = ("cx", "cy", "n_heard", "heard_mask", "flags", "pred", "cond", "counts", "iters_sum", "stats", "noise", "trial_pos",
            "trial_status", "trial_iters", "trial_dx", "trial_dy", "trial_err")


def safe_cells(ref, gross_m, margin):
    err = ref["trial_err"]
    with np.errstate(invalid="ignore"):
        near = np.abs(err - gross_m) <= margin          # inf - gross = inf: safe; NaN (uncovered): False
    return ~np.any(near, axis=1)


def main():
    os.makedirs(coverage_golden.GOLDEN, exist_ok=True)
    tol = coverage_golden.pos_tolerance()
    for name, scene in coverage_golden.scenes().items():
        ref = coverage_ref.coverage_ref(**scene)
        covered = (ref["flags"] & coverage_ref.UNCOVERED) == 0
        safe = safe_cells(ref, scene["gross_m"], 1e3 * tol)
        assert np.count_nonzero(covered & ~safe) <= 0.05 * np.count_nonzero(covered), (name, "gross_m leaves too many unsafe cells")
        data = dict(scene)
        data.update({"ref_" + key: ref[key] for key in RECORDED})
        data["safe"], data["pos_tolerance"] = safe, tol
        lossy = (ref["flags"] & coverage_ref.LOSSY) != 0
        if name == "ring5":
            assert covered.all() and not lossy.any() and int(ref["counts"][:, 4].sum()) >= 2000
        if name == "range6":
            assert {0, 2, 3, 4, 6} <= set(ref["n_heard"].tolist()), sorted(set(ref["n_heard"].tolist()))
        if name == "far4":
            assert lossy.any()
            centre = tuple(np.asarray(scene["table"]).mean(axis=0).tolist())
            mid = coverage_ref.coverage_ref(**dict(scene, x0=centre))
            assert not np.any(mid["flags"] & coverage_ref.LOSSY)
            data["x0_centre"], data["ref_flags_centre"], data["ref_counts_centre"] = np.array(centre), mid["flags"], mid["counts"]
            data["safe_centre"] = safe_cells(mid, scene["gross_m"], 1e3 * tol)
        if name == "mixed5":
            assert np.all(ref["noise"][:, :, 1] == 0.0) and covered.all()
        data = {key: np.asarray(value) for key, value in data.items()}
        data["seed"] = np.array(scene["seed"], dtype=np.uint64)
        path = os.path.join(coverage_golden.GOLDEN, name + ".npz")
        np.savez_compressed(path, **data)
        print("%-7s %3d cells, %3d covered, %2d degenerate, %2d lossy, %2d unsafe, heard %s, %6d bytes" % (
            name, len(covered), covered.sum(), np.count_nonzero(ref["flags"] & 2), lossy.sum(), np.count_nonzero(covered & ~safe),
            sorted(set(ref["n_heard"].tolist())), os.path.getsize(path)))


if __name__ == "__main__":
    main()
