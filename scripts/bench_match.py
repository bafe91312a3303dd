"""Measurement: `thr_match` on synthetic .toads columns -- 4 receivers, 8 transmitters sending about
once a second each, receiver clock skews of tens of ms, window 0.2 s, about 5 % of the detections a
second detection of the same transmission by the same receiver (a collision) -- at n = 2^16, 2^20 and
2^24 detections.  Per size: one warm-up call, then --repeats calls; median and range of the wall time
and of its split into copies in / kernels / copies out (HIP events, `thr_debug_match_times`), and the
rate in detections/s.  Beside it the sequential statement tests/match_ref.py on the same columns on one
host core, at the sizes where it stays under a minute (the outputs are compared while at it), and
`identify`'s recorded 46-50 M detections/s for scale.  Writes one JSON record (default
profiles/r09_match.json); no figure is asserted anywhere."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from match_ref import match_ref, to_csr  # noqa: E402
from thrifty_amd import _native, build  # noqa: E402

N_RX, N_TX, WINDOW, MIN_MATCH = 4, 8, 0.2, 2
IDENTIFY_RATE = "46-50 M detections/s (DESIGN.md 3.7)"


def columns(n, seed=9):
    """n detections in timestamp order: every transmission is seen by each receiver with probability
    0.9, and 5 % of the detections are doubled a few ms later."""
    rng = np.random.default_rng(seed)
    n_events = int(n / (N_RX * 0.9 * 1.05)) + 1
    tx = np.arange(n_events) % N_TX                 # transmitter x sends at second k + x / N_TX, a little jittered
    t = 1.7e9 + np.arange(n_events) // N_TX + tx / N_TX + rng.uniform(0, 0.02, n_events)
    skew = rng.uniform(-0.03, 0.03, N_RX)
    seen = rng.random((n_events, N_RX)) < 0.9
    ev, rx = np.nonzero(seen)
    ts = t[ev] + skew[rx] + rng.normal(0, 1e-3, len(ev))
    doubled = rng.random(len(ev)) < 0.05
    ev, rx = np.concatenate([ev, ev[doubled]]), np.concatenate([rx, rx[doubled]])
    ts = np.concatenate([ts, ts[doubled] + rng.uniform(1e-3, 8e-3, int(doubled.sum()))])
    order = np.argsort(ts, kind="stable")[:n]
    return (rx[order].astype(np.int32), tx[ev[order]].astype(np.int32), ts[order],
            rng.uniform(50, 200, len(order)))


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def measure(n, repeats, ref_limit_s):
    rx, tx, ts, en = columns(n)
    n = len(rx)
    out = _native.match(rx, tx, ts, en, WINDOW, MIN_MATCH)      # warm-up
    wall, parts = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = _native.match(rx, tx, ts, en, WINDOW, MIN_MATCH)
        wall.append(time.perf_counter() - t0)
        parts.append(_native.match_times())
    ptr, idx, misses, collisions = out
    rec = {"n": n, "matches": len(ptr) - 1, "misses": len(misses), "collisions": len(collisions),
           "collision_fraction": len(collisions) / n,
           "wall_ms": spread([1e3 * w for w in wall]),
           "copies_in_ms": spread([p[0] for p in parts]), "kernels_ms": spread([p[1] for p in parts]),
           "copies_out_ms": spread([p[2] for p in parts]),
           "detections_per_s": n / statistics.median(wall),
           "detections_per_s_kernels_only": n / (1e-3 * statistics.median([p[1] for p in parts]))}
    if ref_limit_s is not None:
        t0 = time.perf_counter()
        want = match_ref(rx, tx, ts, en, WINDOW, MIN_MATCH)
        took = time.perf_counter() - t0
        want_ptr, want_idx = to_csr(want[0])
        rec["match_ref_one_core_s"] = took
        rec["match_ref_detections_per_s"] = n / took
        rec["equals_match_ref"] = bool(ptr.tolist() == want_ptr and idx.tolist() == want_idx and
                                       misses.tolist() == want[1] and
                                       [tuple(p) for p in collisions.tolist()] == want[2])
        rec["match_ref_within_limit"] = took <= ref_limit_s
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1 << 16, 1 << 20, 1 << 24])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ref-up-to", type=int, default=1 << 24, help="largest n match_ref is run at")
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "r09_match.json"))
    args = ap.parse_args()
    runs = []
    for n in args.sizes:
        runs.append(measure(n, args.repeats, 60.0 if n <= args.ref_up_to else None))
        print(json.dumps(runs[-1]), flush=True)
    rec = {"csrc_hash": build.csrc_hash(), "receivers": N_RX, "transmitters": N_TX,
           "window_s": WINDOW, "min_match": MIN_MATCH, "repeats": args.repeats,
           "identify_recorded": IDENTIFY_RATE, "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
