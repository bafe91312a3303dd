"""Measurement: `thr_posg` beside `thr_pos` on the scene of scripts/bench_pos.py (8 receivers on a jittered ring of
1000 m, --groups groups (default 1 Mi) of all 28 receiver pairs each, 10 ns of TDOA noise) with the receivers shifted
by (5000, -3000) m, so that the fixed start (0.1, 0.1) lies outside the array.  One warm-up call, then --repeats calls
of each: medians and ranges of the wall time and of its split (HIP events),
  thr_pos    copies in / kernels / copies out;
  thr_posg   copies in / task 0 (the fixed start) / surface, minima and starts / refinement / choice / copies out,
and the count of groups that `thr_pos` leaves more than 10 m from the planted position and the global solve does not.
Writes one JSON record (default profiles/r24_posg.json); no figure is asserted anywhere."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402

import bench_pos  # noqa: E402
from bench_posq import timed  # noqa: E402
from thrifty_amd import _native, build  # noqa: E402

SHIFT = np.array([5000.0, -3000.0])
POSG_PARTS = ("copies_in_ms", "task0_ms", "grid_and_starts_ms", "refinement_ms", "choice_ms", "copies_out_ms")
FETCHED = ("pos", "status", "task", "n_minima", "flags", "n_local")


def planted_of(n_groups, table, seed=11):
    """The mobiles of bench_pos.scene(n_groups, seed): its draws replayed (the table comes first)."""
    rng = np.random.default_rng(seed)
    ang = np.linspace(0, 2 * np.pi, bench_pos.N_RX, endpoint=False) + 0.3
    again = np.c_[np.cos(ang), np.sin(ang)] * bench_pos.RADIUS + rng.normal(0, bench_pos.RADIUS * 0.05, (bench_pos.N_RX, 2))
    if not np.array_equal(again, table):
        raise RuntimeError("bench_pos.scene no longer draws its table first")
    return rng.uniform(-1, 1, (n_groups, 2)) * bench_pos.RADIUS * 0.6


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--starts", type=int, default=4)
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "r24_posg.json"))
    args = ap.parse_args()
    ptr, rx0, rx1, tdoa, snr, table = bench_pos.scene(args.groups)
    planted = planted_of(args.groups, table) + SHIFT
    table = table + SHIFT                                            # TDOAs do not change under a translation
    margin = float(np.max(table.max(axis=0) - table.min(axis=0)))    # the Python interface's default
    hashes = {}
    for name in ("pos.hip", "posg.hip", "pos_lm.hpp"):               # (csrc_hash() leaves all three out)
        with open(os.path.join(build.CSRC, name), "rb") as f:
            hashes[name] = hashlib.sha256(f.read()).hexdigest()[:16]
    rec = {"csrc_hash": build.csrc_hash(), "sha256": hashes, "receivers": bench_pos.N_RX, "rows_per_group": 28,
           "radius_m": bench_pos.RADIUS, "noise_s": bench_pos.NOISE, "shift_m": SHIFT.tolist(), "repeats": args.repeats,
           "groups": args.groups, "grid": args.grid, "starts": args.starts, "margin_m": margin}

    pos, rec["thr_pos"] = timed(lambda: _native.pos(ptr, rx0, rx1, tdoa, snr, table), _native.pos_times,
                                ("copies_in_ms", "kernels_ms", "copies_out_ms"), args.repeats)
    (_, out), rec["thr_posg"] = timed(lambda: _native.posg(ptr, rx0, rx1, tdoa, snr, table, margin, grid=args.grid,
                                                           starts=args.starts, outputs=FETCHED), _native.posg_times,
                                      POSG_PARTS, args.repeats)
    far_fixed = np.hypot(*(pos["pos"] - planted).T) > 10.0
    far_global = np.hypot(*(out["pos"] - planted).T) > 10.0
    rec["thr_pos"]["status_counts"] = np.bincount(pos["status"], minlength=5).tolist()
    rec["thr_posg"].update({
        "status_counts": np.bincount(out["status"], minlength=5).tolist(),
        "flag_counts": {str(k): int(v) for k, v in zip(*np.unique(out["flags"], return_counts=True))},
        "chosen_task_counts": np.bincount(out["task"], minlength=args.starts + 1).tolist(),
        "mean_n_minima": float(out["n_minima"].mean()), "mean_local_minimum_cells": float(out["n_local"].mean())})
    rec["more_than_10_m_from_the_planted_position"] = {
        "thr_pos": int(far_fixed.sum()), "thr_posg": int(far_global.sum()),
        "thr_pos_but_not_thr_posg": int(np.count_nonzero(far_fixed & ~far_global)),
        "thr_posg_but_not_thr_pos": int(np.count_nonzero(far_global & ~far_fixed))}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
