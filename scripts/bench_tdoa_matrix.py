"""Measurement: `thr_tdoamatrix` on scripts/bench_syncstats.py's scene (4 receivers, 8 transmitters of which 2 beacons;
2^18 transmissions = 2^20 detections), window 4 and the zero geometry of the reference's scripts/tdoa_matrix.py.
Three routes to the same cells, in the same run:
 - the one call: one warm-up, then --repeats calls; median and range of the wall time (every array fetched) and of
   the five event intervals (`thr_debug_tdoamatrix_times`);
 - the route that existed before it, per cell: the matches of the beacon and the transmitter that hold both receivers,
   cut down to those two detections (NumPy), through `tdoa_est.tdoa_columns` (thr_tdoa_model; `estimate_tdoas` is this
   call behind DetectionResult objects) and then `tdoa_analysis.tdoa_stats(robust=True)` (thr_tdoastats); the same
   warm-up and repeats over ALL cells; the kept counts and the means are compared with the one call's while at it;
 - the NumPy statement tests/tdoa_matrix_ref.py on the first --ref-matches matches on one host core, EXTRAPOLATED to
   the whole scene by the task count and marked so.
Writes one JSON record (default profiles/r25_tdoa_matrix.json); no figure is asserted anywhere."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402

import bench_syncstats  # noqa: E402
import bench_tdoa  # noqa: E402
from bench_syncstats import spread  # noqa: E402
from tdoa_matrix_ref import tdoa_matrix_ref  # noqa: E402
from thrifty_amd import _native, build, tdoa_analysis, tdoa_est  # noqa: E402

WINDOW = 4.0
PHASES = ("copies_in_ms", "rows_and_tasks_ms", "estimate_ms", "mask_and_statistics_ms", "copies_out_ms")


def per_cell_route(cols, ptr, idx, keys):
    """Every cell of `keys` the way it could be had before: extraction, thr_tdoa_model, thr_tdoastats.
    -> ({key: (kept, mean)}, seconds spent in the extraction)."""
    n_matches = len(ptr) - 1
    t0 = time.perf_counter()
    match_of = np.repeat(np.arange(n_matches), np.diff(ptr))
    det_at = np.full((n_matches, int(cols["rxid"].max()) + 1), -1, np.int64)
    det_at[match_of, cols["rxid"][idx]] = idx
    match_tx = cols["txid"][idx[ptr[:-1]]]
    extraction = time.perf_counter() - t0
    out = {}
    for rx0, rx1, b, t in keys:
        t0 = time.perf_counter()
        rows = np.flatnonzero(((match_tx == b) | (match_tx == t)) & (det_at[:, rx0] >= 0) & (det_at[:, rx1] >= 0))
        cell_idx = np.column_stack([det_at[rows, rx0], det_at[rows, rx1]]).ravel()
        cell_ptr = 2 * np.arange(len(rows) + 1, dtype=np.int64)
        extraction += time.perf_counter() - t0
        res = tdoa_est.tdoa_columns(cols, cell_ptr, cell_idx, WINDOW, {b: 0.0}, {rx0: 0.0, rx1: 0.0}, bench_tdoa.FS, 2)
        per_group = np.diff(res["group_ptr"])
        matrix = {"rx0": res["tdoas"]["rx0"], "rx1": res["tdoas"]["rx1"], "tx": np.repeat(res["tx"], per_group),
                  "timestamp": np.repeat(res["timestamp"], per_group), "det0_idx": res["tdoas"]["det0_idx"],
                  "det1_idx": res["tdoas"]["det1_idx"], "tdoa": res["tdoas"]["tdoa"]}
        stats = tdoa_analysis.tdoa_stats(matrix, robust=True)
        out[(rx0, rx1, b, t)] = (int(stats.robust_count[0]), float(stats.robust_stats[0, 0]))
    return out, extraction


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matches", type=int, default=1 << 18)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ref-matches", type=int, default=1 << 11, help="matches the NumPy statement runs on (0: skip it)")
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "r25_tdoa_matrix.json"))
    args = ap.parse_args()
    cols, ptr, idx, beacon_pos, rx_pos, _ = bench_syncstats.scene(args.matches)
    cols = {name: np.ascontiguousarray(cols[name], kind) for name, kind in _native.TDMAT_COLUMNS}
    beacons = sorted(beacon_pos)
    rec = {"csrc_hash": build.csrc_hash(), "receivers": bench_tdoa.N_RX, "beacons": len(beacons), "mobiles": bench_tdoa.N_MOBILE,
           "matches": args.matches, "detections": len(cols["rxid"]), "window": WINDOW, "model": "poly", "deg": 2,
           "repeats": args.repeats, "tile_workgroup_tasks_per_workgroup": _native.tdoamatrix_geometry()}

    call = lambda: _native.tdoamatrix(cols, ptr, idx, beacons, window=WINDOW, sample_rate=bench_tdoa.FS)   # noqa: E731
    call()      # warm-up
    wall, parts = [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        counts, out = call()
        wall.append(time.perf_counter() - t0)
        parts.append(_native.tdoamatrix_times())
    one = {"wall_ms": spread([1e3 * w for w in wall])}
    for k, name in enumerate(PHASES):
        one[name] = spread([p[k] for p in parts])
    one["device_ms"] = sum(one[name]["median"] for name in PHASES[1:4])
    one.update(counts, kept=int(out["cell_counts"][:, 4].sum()), masked=int(out["outlier"].sum()),
               tasks_per_s_device=counts["tasks"] / (1e-3 * one["device_ms"]))
    rec["one_call"] = one
    print(json.dumps(one), flush=True)

    keys = [tuple(k) for k in out["cell_key"].tolist()]
    per_cell_route(cols, ptr, idx, keys[:2])      # warm-up
    wall, extraction = [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        cells, took = per_cell_route(cols, ptr, idx, keys)
        wall.append(time.perf_counter() - t0)
        extraction.append(took)
    kept = np.array([cells[k][0] for k in keys])
    mean = np.array([cells[k][1] for k in keys])
    route = {"cells": len(keys), "wall_ms": spread([1e3 * w for w in wall]), "of_which_extraction_ms": spread([1e3 * e for e in extraction]),
             "kept_counts_equal_one_call": bool(np.array_equal(kept, out["cell_counts"][:, 4])),
             "largest_mean_difference_m": float(np.nanmax(np.abs(mean - out["cell_stats"][:, 0])))}
    route["over_one_call_wall"] = route["wall_ms"]["median"] / one["wall_ms"]["median"]
    rec["per_cell_route"] = route
    print(json.dumps(route), flush=True)

    if args.ref_matches:
        n = min(args.ref_matches, args.matches)
        sub_ptr, sub_idx = ptr[:n + 1], idx[:ptr[n]]
        t0 = time.perf_counter()
        ref_counts, _ = tdoa_matrix_ref(cols, sub_ptr, sub_idx, beacons, window=WINDOW, sample_rate=bench_tdoa.FS)
        took = time.perf_counter() - t0
        scaled = took * counts["tasks"] / ref_counts["tasks"]
        rec["numpy_statement"] = {"matches": n, "tasks": ref_counts["tasks"], "one_core_s": took,
                                  "EXTRAPOLATED_to_all_tasks_s": scaled, "extrapolated_by": "task count",
                                  "extrapolated_over_one_call_wall": scaled / (1e-3 * one["wall_ms"]["median"])}
        print(json.dumps(rec["numpy_statement"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
