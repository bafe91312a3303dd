"""Measurement: `thr_pos` on synthetic groups -- 8 receivers on a jittered ring of 1000 m, --groups
groups (default 1 Mi) of all 28 receiver pairs each, the mobile inside 0.6 of the radius, 10 ns of TDOA
noise.  One warm-up call, then --repeats calls: median and range of the wall time and of its split into
copies in / kernels / copies out (HIP events, `thr_debug_pos_times`), the rate in groups per second,
and the statuses and iteration counts.  Beside it the NumPy restatement tests/pos_ref.py on the first
--ref-groups groups on one host core (its positions are compared with the device's while at it).
Writes one JSON record (default profiles/r11_pos.json); no figure is asserted anywhere."""
import argparse
import hashlib
import itertools
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from pos_ref import pos_ref_groups  # noqa: E402
from thrifty_amd import _native, build, pos_est  # noqa: E402

N_RX, RADIUS, NOISE = 8, 1000.0, 10e-9


def scene(n_groups, seed=11):
    rng = np.random.default_rng(seed)
    ang = np.linspace(0, 2 * np.pi, N_RX, endpoint=False) + 0.3
    table = np.c_[np.cos(ang), np.sin(ang)] * RADIUS + rng.normal(0, RADIUS * 0.05, (N_RX, 2))
    pairs = np.array(list(itertools.combinations(range(N_RX), 2)), dtype=np.int32)
    mobile = rng.uniform(-1, 1, (n_groups, 2)) * RADIUS * 0.6
    dist = np.linalg.norm(table[None, :, :] - mobile[:, None, :], axis=2)
    tdoa = (dist[:, pairs[:, 0]] - dist[:, pairs[:, 1]]) / pos_est.SPEED_OF_LIGHT + rng.normal(0, NOISE, (n_groups, len(pairs)))
    ptr = np.arange(n_groups + 1, dtype=np.int64) * len(pairs)
    return (ptr, np.tile(pairs[:, 0], n_groups), np.tile(pairs[:, 1], n_groups), tdoa.ravel(),
            rng.uniform(5.0, 500.0, tdoa.size), table)


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ref-groups", type=int, default=500, help="groups tests/pos_ref.py is run on")
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "r11_pos.json"))
    args = ap.parse_args()
    ptr, rx0, rx1, tdoa, snr, table = scene(args.groups)
    run = lambda: _native.pos(ptr, rx0, rx1, tdoa, snr, table)   # noqa: E731
    out = run()                                                  # warm-up
    wall, parts = [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        out = run()
        wall.append(time.perf_counter() - t0)
        parts.append(_native.pos_times())
    kernels = statistics.median([p[1] for p in parts])
    with open(os.path.join(build.CSRC, "pos.hip"), "rb") as f:       # (csrc_hash() leaves pos.hip out: UNPROFILED_POS)
        kernel_hash = hashlib.sha256(f.read()).hexdigest()[:16]
    rec = {"csrc_hash": build.csrc_hash(), "pos_hip_sha256": kernel_hash, "receivers": N_RX, "rows_per_group": 28,
           "radius_m": RADIUS, "noise_s": NOISE, "repeats": args.repeats, "groups": args.groups,
           "status_counts": dict(zip(pos_est.STATUS_NAMES, np.bincount(out["status"], minlength=5).tolist())),
           "iterations": {"median": float(np.median(out["iters"])), "max": int(out["iters"].max())},
           "wall_ms": spread([1e3 * w for w in wall]), "copies_in_ms": spread([p[0] for p in parts]),
           "kernels_ms": spread([p[1] for p in parts]), "copies_out_ms": spread([p[2] for p in parts]),
           "groups_per_s": args.groups / statistics.median(wall), "groups_per_s_kernels_only": args.groups / (1e-3 * kernels)}
    if args.ref_groups:
        m = min(args.ref_groups, args.groups)
        t0 = time.perf_counter()
        want = pos_ref_groups(ptr[:m + 1], rx0[:28 * m], rx1[:28 * m], tdoa[:28 * m], snr[:28 * m], table)
        took = time.perf_counter() - t0
        rec.update({"pos_ref_groups": m, "pos_ref_one_core_s": took, "pos_ref_groups_per_s": m / took,
                    "same_status_as_pos_ref": bool(np.array_equal(want["status"], out["status"][:m])),
                    "max_abs_position_difference_m": float(np.max(np.abs(want["pos"] - out["pos"][:m])))})
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
