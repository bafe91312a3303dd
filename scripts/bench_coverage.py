"""Measurement: `thr_coverage` on the geometry of scripts/bench_pos.py (8 receivers on a jittered ring of 1000 m): --grid x
--grid cells (default 128) over the square of +-600 m inside the ring, --trials trials per cell (default 256), 1 m of
arrival noise, gross_m = 10 m.  One warm-up call, then --repeats calls: medians and ranges of the wall time with EVERY
array fetched and of the device time split (HIP events: copies in / cells / synthesis / solve / reduction and sort /
copies out), the slab count and bytes, and a summary of the map.

Beside it the route that exists without thr_coverage: the NumPy statement's synthesis (tests/coverage_ref.py's generator,
vectorised over a block of cells) plus ONE `_native.pos` call over all groups of the block.  It is timed on --subset cells
(default 256) and EXTRAPOLATED to the whole map by the task count; the record marks it so.  Its per-cell reduction is not
timed.  Writes one JSON record (default profiles/r26_coverage.json); no figure is asserted anywhere."""
import argparse
import hashlib
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import bench_pos  # noqa: E402
import coverage_ref  # noqa: E402
from bench_posq import timed  # noqa: E402
from thrifty_amd import _native, build  # noqa: E402

PARTS = ("copies_in_ms", "cells_ms", "synthesis_ms", "solve_ms", "reduction_and_sort_ms", "copies_out_ms")


def numpy_route(table, sigma, cx, cy, nx, cells, trials, seed):
    """The statement's synthesis for `cells`, then one thr_pos call -> (seconds of synthesis, seconds of the call, groups)."""
    pairs = np.array(list(itertools.combinations(range(len(table)), 2)), dtype=np.int32)
    t0 = time.perf_counter()
    n = coverage_ref.noise(cells, trials, sigma, seed)                                   # [cells, T, n_rx]
    p = np.c_[cx[cells % nx], cy[cells // nx]]
    d = table[None, :, :] - p[:, None, :]
    dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])                        # [cells, n_rx]
    tdoa = ((dist[:, None, pairs[:, 0]] - dist[:, None, pairs[:, 1]]) + (n[..., pairs[:, 0]] - n[..., pairs[:, 1]])) / coverage_ref.C
    groups = len(cells) * trials
    ptr = np.arange(groups + 1, dtype=np.int64) * len(pairs)
    rx0, rx1, snr = np.tile(pairs[:, 0], groups), np.tile(pairs[:, 1], groups), np.ones(tdoa.size)
    t1 = time.perf_counter()
    out = _native.pos(ptr, rx0, rx1, tdoa.ravel(), snr, table)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, groups, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--trials", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--subset", type=int, default=256, help="cells the NumPy route is timed on")
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "r26_coverage.json"))
    args = ap.parse_args()
    table = bench_pos.scene(1)[5]
    sigma, half, gross_m, seed = np.full(len(table), 1.0), 0.6 * bench_pos.RADIUS, 10.0, 26
    lo, hi = (-half, -half), (half, half)
    hashes = {}
    for name in ("coverage.hip", "pos.hip", "pos_lm.hpp"):                # (csrc_hash() leaves all three out)
        with open(os.path.join(build.CSRC, name), "rb") as f:
            hashes[name] = hashlib.sha256(f.read()).hexdigest()[:16]
    rec = {"csrc_hash": build.csrc_hash(), "sha256": hashes, "receivers": len(table), "rows_per_trial": 28,
           "radius_m": bench_pos.RADIUS, "area_m": [lo, hi], "grid": [args.grid, args.grid], "trials": args.trials, "sigma_m": 1.0,
           "gross_m": gross_m, "seed": seed, "repeats": args.repeats}

    run = lambda: _native.coverage(table, sigma, lo, hi, args.grid, args.grid, gross_m, trials=args.trials, seed=seed)      # noqa: E731
    (counts, out), rec["thr_coverage"] = timed(run, _native.coverage_times, PARTS, args.repeats)
    rec["thr_coverage"]["counts"] = counts
    stats, pred, flags = out["stats"], out["pred"], out["flags"]
    rec["map"] = {"lossy_cells": int(np.count_nonzero(flags & 4)), "rms_median_m": float(np.median(stats[:, 5])),
                  "rms_worst_m": float(np.max(stats[:, 5])), "pred_rms_median_m": float(np.median(pred[:, 4])),
                  "median_rms_over_pred_rms": float(np.median(stats[:, 5] / pred[:, 4])),
                  "status_counts": out["counts"][:, :4].sum(axis=0).tolist(), "gross_trials": int(out["counts"][:, 5].sum()),
                  "mean_iters": float(out["iters_sum"].sum() / counts["tasks"])}

    cells = np.linspace(0, args.grid * args.grid - 1, min(args.subset, args.grid * args.grid)).astype(np.int64)
    numpy_route(table, sigma, out["cx"], out["cy"], args.grid, cells[:8], args.trials, seed)       # warm-up
    runs = [numpy_route(table, sigma, out["cx"], out["cy"], args.grid, cells, args.trials, seed) for _ in range(args.repeats)]
    scale = counts["tasks"] / float(runs[0][2])
    synth, solve = bench_pos.spread([1e3 * r[0] for r in runs]), bench_pos.spread([1e3 * r[1] for r in runs])
    rec["numpy_synthesis_plus_one_thr_pos_call"] = {
        "measured_on_cells": len(cells), "measured_on_groups": runs[0][2], "synthesis_ms": synth, "thr_pos_call_wall_ms": solve,
        "EXTRAPOLATED_by_task_count": {"factor": scale, "synthesis_ms": synth["median"] * scale,
                                       "thr_pos_call_wall_ms": solve["median"] * scale,
                                       "total_ms": (synth["median"] + solve["median"]) * scale},
        "not_timed": "the per-cell reduction of this route"}
    # the same trials: the subset's positions are the device's (kept cells are not fetched here; statuses are compared)
    sub = runs[0][3]["status"].reshape(len(cells), args.trials)
    rec["numpy_synthesis_plus_one_thr_pos_call"]["ok_trials_equal_the_maps"] = bool(
        np.array_equal((sub == 0).sum(axis=1), out["counts"][cells, 0]))
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
