"""Measurement: `thr_pos3` beside `thr_pos` on scripts/bench_pos.py's scene (8 receivers on a jittered ring of
1000 m, --groups groups of all 28 receiver pairs, 10 ns of TDOA noise), with antenna heights.  Four legs, alternated
inside every repeat so that they share the box's state, one warm-up round first:

  flat         thr_pos on the 2-D scene: the yardstick;
  level        thr_pos3, height known, every receiver lifted to the transmitters' height: thr_pos's arithmetic plus one
               add per range, and its bytes (checked here at full size);
  known        thr_pos3, height known, antennas at 5 .. 200 m, transmitters at 0 .. 3 m (each group's own height);
  free_z       thr_pos3, z free, the same rows, from 1 m below the lowest antenna.

Per leg: median and range over --repeats of the kernel time (HIP events: `thr_debug_pos_times`' and
`thr_debug_pos3_times`' middle entry; thr_pos's window also holds its five output allocations, thr_pos3 allocates
before the first event) and of the wall time, the statuses and the iteration counts.  `level_over_flat` is the ratio
of the two median kernel times; where it exceeds 1.15 the record says so (`level_over_flat_above_1_15`) and DESIGN.md
3.22 explains it from the resource listing and the iteration counts.  Writes one JSON record (default
profiles/r27_pos3.json); no figure is asserted anywhere."""
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

LEVEL, Z_LO, Z_HI, TAG_Z = 12.5, 5.0, 200.0, 3.0


def tall_scene(n_groups, table, rx0, rx1, seed=27):
    """Antenna heights on bench_pos's ring, transmitters at 0 .. TAG_Z m at bench_pos's horizontal spread, and the
    TDOAs of the same pairs with the same noise -> (table[n_rx, 3], tdoa, group_h)."""
    rng = np.random.default_rng(seed)
    xyz = np.c_[table, rng.permutation(np.linspace(Z_LO, Z_HI, len(table)))]
    mobile = np.c_[rng.uniform(-1, 1, (n_groups, 2)) * bench_pos.RADIUS * 0.6, rng.uniform(0.0, TAG_Z, n_groups)]
    dist = np.linalg.norm(xyz[None, :, :] - mobile[:, None, :], axis=2)
    pairs0, pairs1 = rx0[:28], rx1[:28]
    tdoa = (dist[:, pairs0] - dist[:, pairs1]) / pos_est.SPEED_OF_LIGHT + rng.normal(0, bench_pos.NOISE, (n_groups, 28))
    return xyz, tdoa.ravel(), mobile[:, 2].copy()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "r27_pos3.json"))
    args = ap.parse_args()
    ptr, rx0, rx1, tdoa, snr, table = bench_pos.scene(args.groups)
    xyz, tdoa3, group_h = tall_scene(args.groups, table, rx0, rx1)
    level = np.c_[table, np.full(len(table), LEVEL)]
    z0 = float(xyz[:, 2].min()) - 1.0
    legs = {
        "flat": (lambda: _native.pos(ptr, rx0, rx1, tdoa, snr, table), _native.pos_times),
        "level": (lambda: _native.pos3(ptr, rx0, rx1, tdoa, snr, level, _native.POS3_KNOWN_HEIGHT,
                                       np.full(args.groups, LEVEL)), _native.pos3_times),
        "known": (lambda: _native.pos3(ptr, rx0, rx1, tdoa3, snr, xyz, _native.POS3_KNOWN_HEIGHT, group_h), _native.pos3_times),
        "free_z": (lambda: _native.pos3(ptr, rx0, rx1, tdoa3, snr, xyz, _native.POS3_FREE_Z, None, (0.1, 0.1, z0)),
                   _native.pos3_times),
    }
    out = {name: call() for name, (call, _) in legs.items()}           # warm-up, every leg
    wall, kernel = {name: [] for name in legs}, {name: [] for name in legs}
    for _ in range(args.repeats):
        for name, (call, times) in legs.items():                       # alternated: a drift of the box reaches all four
            t0 = time.perf_counter()
            out[name] = call()
            wall[name].append(time.perf_counter() - t0)
            kernel[name].append(times()[1])
    same = all(np.array_equal(out["level"][key] if key != "pos" else out["level"]["pos"][:, :2], out["flat"][key])
               for key in ("pos", "dop", "snr", "status", "iters"))
    with open(os.path.join(build.CSRC, "pos3.hip"), "rb") as f, open(os.path.join(build.CSRC, "pos3_lm.hpp"), "rb") as h:
        kernel_hash = hashlib.sha256(f.read() + h.read()).hexdigest()[:16]
    rec = {"csrc_hash": build.csrc_hash(), "pos3_sha256": kernel_hash, "receivers": bench_pos.N_RX, "rows_per_group": 28,
           "radius_m": bench_pos.RADIUS, "noise_s": bench_pos.NOISE, "antenna_heights_m": [Z_LO, Z_HI], "tag_heights_m": [0.0, TAG_Z],
           "z0_m": z0, "repeats": args.repeats, "groups": args.groups, "level_equals_flat_bytes": bool(same), "legs": {}}
    for name in legs:
        iters = out[name]["iters"]
        rec["legs"][name] = {
            "kernel_ms": bench_pos.spread(kernel[name]), "wall_ms": bench_pos.spread([1e3 * w for w in wall[name]]),
            "groups_per_s_kernel_only": args.groups / (1e-3 * statistics.median(kernel[name])),
            "status_counts": dict(zip(pos_est.STATUS_NAMES, np.bincount(out[name]["status"], minlength=5).tolist())),
            "iterations": {"median": float(np.median(iters)), "mean": float(np.mean(iters)), "max": int(iters.max())}}
    flat = rec["legs"]["flat"]["kernel_ms"]["median"]
    for name in ("level", "known", "free_z"):
        rec[name + "_over_flat"] = rec["legs"][name]["kernel_ms"]["median"] / flat
    rec["level_over_flat_above_1_15"] = bool(rec["level_over_flat"] > 1.15)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
