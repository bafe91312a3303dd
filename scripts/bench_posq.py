"""Measurement: `thr_posq` beside `thr_pos` on the scene of scripts/bench_pos.py (8 receivers on a jittered ring of
1000 m, all 28 pairs, 10 ns of TDOA noise), --groups groups (default 1 Mi).  Three cases, each one warm-up call and
then --repeats calls, medians and ranges, split by HIP events:
  thr_pos                 copies in / kernels / copies out;
  thr_posq without a gate copies in / full solves / flags and expansion / candidates / choice and residuals / copies out;
  thr_posq with a gate    the same, with one receiver's arrival --delay metres late in --share of the groups; the
                          flagged groups, the candidates, and how many of the planted receivers were excluded.
Writes one JSON record (default profiles/r22_posq.json); no figure is asserted anywhere."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402

import bench_pos  # noqa: E402
from thrifty_amd import _native, build, pos_est  # noqa: E402

POSQ_PARTS = ("copies_in_ms", "full_solves_ms", "flags_and_expansion_ms", "candidates_ms", "choice_and_residuals_ms", "copies_out_ms")


def timed(run, times, names, repeats):
    out = run()                                                  # warm-up
    wall, parts = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = run()
        wall.append(time.perf_counter() - t0)
        parts.append(times())
    rec = {"wall_ms": bench_pos.spread([1e3 * w for w in wall])}
    rec.update({name: bench_pos.spread([p[k] for p in parts]) for k, name in enumerate(names)})
    return out, rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--share", type=float, default=0.01, help="share of the groups with a late arrival")
    ap.add_argument("--delay", type=float, default=150.0, help="metres")
    ap.add_argument("--gate", type=float, default=10.0, help="metres; the scene's TDOA noise is 3 m")
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "r22_posq.json"))
    args = ap.parse_args()
    ptr, rx0, rx1, tdoa, snr, table = bench_pos.scene(args.groups)
    hashes = {}
    for name in ("pos.hip", "posq.hip", "pos_lm.hpp"):               # (csrc_hash() leaves all three out)
        with open(os.path.join(build.CSRC, name), "rb") as f:
            hashes[name] = hashlib.sha256(f.read()).hexdigest()[:16]
    rec = {"csrc_hash": build.csrc_hash(), "sha256": hashes, "receivers": bench_pos.N_RX, "rows_per_group": 28,
           "radius_m": bench_pos.RADIUS, "noise_s": bench_pos.NOISE, "repeats": args.repeats, "groups": args.groups}

    pos, rec["thr_pos"] = timed(lambda: _native.pos(ptr, rx0, rx1, tdoa, snr, table), _native.pos_times,
                                ("copies_in_ms", "kernels_ms", "copies_out_ms"), args.repeats)
    (_, out), rec["thr_posq_no_gate"] = timed(lambda: _native.posq(ptr, rx0, rx1, tdoa, snr, table), _native.posq_times,
                                              POSQ_PARTS, args.repeats)
    rec["thr_posq_no_gate"]["same_bytes_as_thr_pos"] = all(out[k].tobytes() == pos[k].tobytes() for k in pos)
    del pos, out

    rng = np.random.default_rng(12)
    late = rng.random(args.groups) < args.share
    which = rng.integers(0, bench_pos.N_RX, args.groups)
    row_late, row_which = np.repeat(late, 28), np.repeat(which, 28)
    shift = args.delay / pos_est.SPEED_OF_LIGHT
    planted = tdoa + shift * (row_late & (rx0 == row_which)) - shift * (row_late & (rx1 == row_which))
    (counts, out), gated = timed(lambda: _native.posq(ptr, rx0, rx1, planted, snr, table, gate_m=args.gate), _native.posq_times,
                                 POSQ_PARTS, args.repeats)
    excluded = out["counts"][:, 2]
    gated.update({"gate_m": args.gate, "delay_m": args.delay, "groups_with_a_late_arrival": int(late.sum()),
                  "flagged": counts["flagged"], "tasks": counts["tasks"],
                  "excluded_the_planted_receiver": int(np.count_nonzero(late & (excluded == which))),
                  "excluded_another_receiver": int(np.count_nonzero((excluded >= 0) & ~(late & (excluded == which)))),
                  "flag_counts": {str(k): int(v) for k, v in zip(*np.unique(out["flags"], return_counts=True))}})
    rec["thr_posq_gate"] = gated
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
