"""Measurement: `thr_posg3` on scripts/bench_pos3.py's scene (8 receivers on a jittered ring of 1000 m with antennas at
5 .. 200 m, --groups groups of all 28 receiver pairs, 10 ns of TDOA noise, transmitters at 0 .. 3 m), in both modes:

  free_z   grid 32 x 32 x 8 over the default z_grid, 4 starts, from 1 m below the lowest antenna;
  known    the same rows with each group's own height: one plane of 32 x 32.

Per leg, over --repeats calls after one warm-up call (the legs alternate inside every repeat): median and range of the
six times of `thr_debug_posg3_times` (HIP events) and of the wall time; the row residuals per second of the volume
kernel (groups x rows x cells / its median time) beside `k_grid`'s figure computed the same way from
profiles/r24_posg.json; the flag counts; and the groups that end more than 10 m (3-D; horizontally with the height
known) from the planted position, for `thr_pos3` and for `thr_posg3`.

For comparison, the route that exists without `thr_posg3` is timed on --ref-groups groups: every volume in NumPy
(tests/posg3_ref.py) plus K + 1 `thr_pos3` calls.  Its figure for all groups is an EXTRAPOLATION (x groups /
ref-groups) and is marked as one.  Grid 16, grid_z other than 8 and starts other than 4 are not measured here.
Writes one JSON record (default profiles/r28_posg3.json); no figure is asserted anywhere."""
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
import bench_pos3  # noqa: E402
import posg3_ref  # noqa: E402
from thrifty_amd import _native, build, pos_3d_global  # noqa: E402

TIMES = ("copies_in_ms", "task0_ms", "volume_and_starts_ms", "refinement_ms", "choice_ms", "copies_out_ms")
GRID, GRID_Z, STARTS = 32, 8, 4


def planted(n_groups, n_rx, seed=27):
    """The transmitters of bench_pos3.tall_scene, drawn again in its order."""
    rng = np.random.default_rng(seed)
    rng.permutation(np.linspace(bench_pos3.Z_LO, bench_pos3.Z_HI, n_rx))
    return np.c_[rng.uniform(-1, 1, (n_groups, 2)) * bench_pos.RADIUS * 0.6, rng.uniform(0.0, bench_pos3.TAG_Z, n_groups)]


def numpy_route(ptr, rx0, rx1, tdoa, snr, xyz, n, margin, z_grid, x0):
    """Seconds of the volumes, minima and starts in NumPy plus K + 1 thr_pos3 calls on the first n groups."""
    rows = int(ptr[n])
    cols = (ptr[:n + 1], rx0[:rows], rx1[:rows], tdoa[:rows], snr[:rows])
    cx, cy, cz = posg3_ref.centres(xyz, margin, GRID, z_grid, GRID_Z)
    t0 = time.perf_counter()
    cells = np.zeros((n, STARTS), dtype=np.int64)
    for g in range(n):
        a, b = int(ptr[g]), int(ptr[g + 1])
        F = posg3_ref.volume(rx0[a:b], rx1[a:b], tdoa[a:b], xyz, cx, cy, cz)
        cells[g] = posg3_ref.lowest(F, posg3_ref.local_minima(F), STARTS)[0]
    t_volume = time.perf_counter() - t0
    t0 = time.perf_counter()
    _native.pos3(*cols, xyz, _native.POS3_FREE_Z, None, x0)
    calls = 1
    for k in range(STARTS):            # one call per distinct start cell of the task: what a caller without thr_posg3 does
        for cell in np.unique(cells[:, k][cells[:, k] >= 0]).tolist():
            groups = np.flatnonzero(cells[:, k] == cell)
            idx = np.concatenate([np.arange(ptr[g], ptr[g + 1]) for g in groups])
            sub = np.concatenate([[0], np.cumsum(ptr[groups + 1] - ptr[groups])])
            _native.pos3(sub, rx0[idx], rx1[idx], tdoa[idx], snr[idx], xyz, _native.POS3_FREE_Z, None,
                         (cx[cell % GRID], cy[(cell // GRID) % GRID], cz[cell // (GRID * GRID)]))
            calls += 1
    return t_volume, time.perf_counter() - t0, calls


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ref-groups", type=int, default=64, help="groups the NumPy route is timed on")
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "r28_posg3.json"))
    args = ap.parse_args()
    ptr, rx0, rx1, _, snr, table = bench_pos.scene(args.groups)
    xyz, tdoa, group_h = bench_pos3.tall_scene(args.groups, table, rx0, rx1)
    truth = planted(args.groups, len(table))
    assert np.array_equal(truth[:, 2], group_h)
    z0 = float(xyz[:, 2].min()) - 1.0
    margin = float(np.max(table.max(axis=0) - table.min(axis=0)))
    z_grid = pos_3d_global.default_z_grid(xyz)
    common = dict(grid=GRID, starts=STARTS)
    legs = {
        "free_z": lambda: _native.posg3(ptr, rx0, rx1, tdoa, snr, xyz, _native.POS3_FREE_Z, margin, x0=(0.1, 0.1, z0), z_grid=z_grid,
                                        grid_z=GRID_Z, **common)[1],
        "known": lambda: _native.posg3(ptr, rx0, rx1, tdoa, snr, xyz, _native.POS3_KNOWN_HEIGHT, margin, group_h=group_h, grid_z=1,
                                       **common)[1],
    }
    fixed = {"free_z": _native.pos3(ptr, rx0, rx1, tdoa, snr, xyz, _native.POS3_FREE_Z, None, (0.1, 0.1, z0)),
             "known": _native.pos3(ptr, rx0, rx1, tdoa, snr, xyz, _native.POS3_KNOWN_HEIGHT, group_h)}
    out = {name: call() for name, call in legs.items()}                # warm-up, both legs
    wall, parts = {name: [] for name in legs}, {name: [] for name in legs}
    for _ in range(args.repeats):
        for name, call in legs.items():
            t0 = time.perf_counter()
            out[name] = call()
            wall[name].append(time.perf_counter() - t0)
            parts[name].append(_native.posg3_times())
    with open(os.path.join(build.CSRC, "posg3.hip"), "rb") as f:
        kernel_hash = hashlib.sha256(f.read()).hexdigest()[:16]
    with open(os.path.join(ROOT, "profiles", "r24_posg.json")) as f:
        r24 = json.load(f)
    k_grid_rate = r24["groups"] * r24["rows_per_group"] * r24["grid"] ** 2 / (1e-3 * r24["thr_posg"]["grid_and_starts_ms"]["median"])
    rec = {"csrc_hash": build.csrc_hash(), "posg3_sha256": kernel_hash, "receivers": bench_pos.N_RX, "rows_per_group": 28,
           "radius_m": bench_pos.RADIUS, "noise_s": bench_pos.NOISE, "antenna_heights_m": [bench_pos3.Z_LO, bench_pos3.Z_HI],
           "tag_heights_m": [0.0, bench_pos3.TAG_Z], "z0_m": z0, "repeats": args.repeats, "groups": args.groups, "grid": GRID,
           "grid_z": GRID_Z, "starts": STARTS, "margin_m": margin, "z_grid_m": list(z_grid),
           "not_measured": "grid 16, grid_z other than 8 (free z), starts other than 4",
           "k_grid_row_residuals_per_s_from_r24_posg": k_grid_rate, "legs": {}}
    for name in legs:
        o, cells = out[name], GRID * GRID * (GRID_Z if name == "free_z" else 1)
        leg = {"wall_ms": bench_pos.spread([1e3 * w for w in wall[name]])}
        for k, key in enumerate(TIMES):
            leg[key] = bench_pos.spread([p[k] for p in parts[name]])
        leg["volume_row_residuals_per_s"] = args.groups * 28 * cells / (1e-3 * leg["volume_and_starts_ms"]["median"])
        leg["volume_rate_over_k_grid"] = leg["volume_row_residuals_per_s"] / k_grid_rate
        flags = o["flags"]
        leg["flag_counts"] = {"moved": int(np.count_nonzero(flags & 1)), "ambiguous": int(np.count_nonzero(flags & 2)),
                              "mirror": int(np.count_nonzero(flags & 8)), "no_minimum": int(np.count_nonzero(flags & 4))}
        leg["status_counts"] = np.bincount(o["status"], minlength=5).tolist()
        leg["chosen_task_counts"] = np.bincount(o["task"], minlength=STARTS + 1).tolist()
        leg["mean_n_minima"], leg["mean_local_minimum_cells"] = float(o["n_minima"].mean()), float(o["n_local"].mean())
        axes = 3 if name == "free_z" else 2
        far = lambda pos: np.sqrt(np.sum((pos[:, :axes] - truth[:, :axes]) ** 2, axis=1)) > 10.0   # noqa: E731
        far_fixed, far_found = far(fixed[name]["pos"]), far(o["pos"])
        leg["more_than_10_m_from_the_planted_position"] = {
            "thr_pos3": int(far_fixed.sum()), "thr_posg3": int(far_found.sum()),
            "thr_pos3_but_not_thr_posg3": int((far_fixed & ~far_found).sum()),
            "thr_posg3_but_not_thr_pos3": int((far_found & ~far_fixed).sum())}
        rec["legs"][name] = leg
    n = min(args.ref_groups, args.groups)
    t_volume, t_solves, calls = numpy_route(ptr, rx0, rx1, tdoa, snr, xyz, n, margin, z_grid, (0.1, 0.1, z0))
    rec["numpy_route_free_z"] = {
        "groups": n, "volumes_s": t_volume, "thr_pos3_calls": calls, "thr_pos3_calls_s": t_solves,
        "EXTRAPOLATED_volumes_s_for_all_groups": t_volume * args.groups / n,
        "note": "the volumes' figure for all groups is an extrapolation (x groups / ref groups), not a measurement; the thr_pos3 calls "
                "are not extrapolated: their number depends on how many distinct start cells the groups share"}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
