"""Measurement: `thr_track` on the geometry of scripts/bench_pos.py run as tracks -- --mobiles transmitters (default 6)
that move inside 0.6 of the 1000 m ring, --rows positions in all (default 1 Mi), interleaved, exponential time steps
of --step seconds per transmitter, position noise of 3 m (the scene's 10 ns) times a dop drawn from 1 .. 2 per axis,
--outliers (default 1 %) of the positions 100 m .. 10 km off.  One warm-up call, then --repeats calls: median and range
of the wall time with every array fetched, the device time per phase (HIP events, `thr_debug_track_times`), the rounds
and the counts.  Beside it the sequential NumPy loop of tests/track_ref.py on a scene of --ref-rows rows on one host
core; its time for the full scene is EXTRAPOLATED by the number of rows and marked so in the record.
Writes one JSON record (default profiles/r23_track.json); no figure is asserted anywhere."""
import argparse
import hashlib
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
import track_ref  # noqa: E402
from thrifty_amd import _native, build, pos_est  # noqa: E402

PARTS = ("copies_in_ms", "sort_and_layout_ms", "filter_rounds_ms", "smoother_ms", "statistics_ms", "copies_out_ms")
SIGMA = bench_pos.NOISE * pos_est.SPEED_OF_LIGHT     # 3 m
ACCEL = 0.5                                          # m s^-3/2


def scene(rows, mobiles, step, outliers, seed=23):
    rng = np.random.default_rng(seed)
    tx = rng.integers(0, mobiles, rows).astype(np.int32)
    t = np.zeros(rows)
    xy = np.zeros((rows, 2))
    for c in range(mobiles):
        mine = np.flatnonzero(tx == c)
        tc = np.cumsum(rng.exponential(step, len(mine)))
        t[mine] = tc
        # a closed curve inside 0.6 of the ring, walked at some metres per second
        w = rng.uniform(0.002, 0.01, 2)
        phase = rng.uniform(0, 2 * np.pi, 2)
        xy[mine] = 0.6 * bench_pos.RADIUS * np.c_[np.cos(w[0] * tc + phase[0]), np.sin(w[1] * tc + phase[1])] * rng.uniform(0.5, 1.0)
    dop = rng.uniform(1.0, 2.0, (rows, 2))
    xy += rng.normal(0.0, 1.0, (rows, 2)) * dop * SIGMA
    off = rng.random(rows) < outliers
    ang = rng.uniform(0, 2 * np.pi, rows)
    xy[off] += (np.exp(rng.uniform(np.log(100.0), np.log(1e4), rows)) * np.stack([np.cos(ang), np.sin(ang)])).T[off]
    r = (dop * SIGMA) ** 2
    return tx + 1, t, xy[:, 0].copy(), xy[:, 1].copy(), r[:, 0].copy(), r[:, 1].copy(), off


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--mobiles", type=int, default=6)
    ap.add_argument("--step", type=float, default=0.1)
    ap.add_argument("--outliers", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ref-rows", type=int, default=20000, help="rows the loop of tests/track_ref.py is timed on")
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "r23_track.json"))
    args = ap.parse_args()
    *cols, planted = scene(args.rows, args.mobiles, args.step, args.outliers)
    q = ACCEL * ACCEL
    run = lambda: _native.track(*cols, q=q)      # noqa: E731
    counts, out = run()                          # warm-up
    wall, parts = [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        counts, out = run()
        wall.append(time.perf_counter() - t0)
        parts.append(_native.track_times())
    hashes = {}
    for name in ("track.hip", "track_scan.hpp"):      # (csrc_hash() leaves both out)
        with open(os.path.join(build.CSRC, name), "rb") as f:
            hashes[name] = hashlib.sha256(f.read()).hexdigest()[:16]
    used = out["used"].astype(bool)
    rec = {"csrc_hash": build.csrc_hash(), "sha256": hashes, "rows": args.rows, "mobiles": args.mobiles, "step_s": args.step,
           "sigma_m": SIGMA, "accel": ACCEL, "repeats": args.repeats, "counts": counts,
           "planted_outliers": int(planted.sum()), "planted_outliers_used": int(np.count_nonzero(planted & used)),
           "other_rows_rejected": int(np.count_nonzero(~planted & ~used)),
           "track_stats": {str(int(tx)): dict(zip(_native.TRACK_STATS, map(float, stats)))
                           for tx, stats in zip(out["track_tx"], out["track_stats"])},
           "track_flags": out["track_flags"].tolist(),
           "wall_ms_every_array_fetched": bench_pos.spread([1e3 * w for w in wall])}
    rec.update({name: bench_pos.spread([p[k] for p in parts]) for k, name in enumerate(PARTS)})
    rec["device_ms_without_copies"] = bench_pos.spread([sum(p[1:5]) for p in parts])

    *ref_cols, _ = scene(args.ref_rows, args.mobiles, args.step, args.outliers)
    t0 = time.perf_counter()
    ref = track_ref.run(*ref_cols, q=q)
    ref_s = time.perf_counter() - t0
    _, small = _native.track(*ref_cols, q=q)
    rec["numpy_loop"] = {"rows": args.ref_rows, "seconds": ref_s, "rounds": ref["counts"]["rounds"],
                         "microseconds_per_row_and_filter_run": 1e6 * ref_s / args.ref_rows / ref["counts"]["rounds"],
                         "same_mask_as_the_device": bool(np.array_equal(ref["used"], small["used"])),
                         "largest_smoothed_difference_m": float(np.nanmax(np.abs(ref["smooth"] - small["smooth"]))),
                         "seconds_for_all_rows": ref_s * args.rows / args.ref_rows,
                         "seconds_for_all_rows_is": "EXTRAPOLATED from %d rows by the row count, not measured" % args.ref_rows}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
