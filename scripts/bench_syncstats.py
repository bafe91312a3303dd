"""Measurement: `thr_beaconsync` and `thr_tdoastats` on scripts/bench_tdoa.py's scene (4 receivers, 8 transmitters
of which 2 beacons; 2^18 transmissions = 2^20 detections) with receiver clocks ascending in rate and receiver 3
losing a whole block about every 500 beacon periods (about one discontinuity per thousand rows over the cells),
its matches, and the .tdoa matrix `tdoa_est.tdoa_columns` makes of them.  Per call: one warm-up, then --repeats
calls; median and range of the wall time (every array fetched) and of the five event intervals
(`thr_debug_beaconsync_times`, `thr_debug_tdoastats_times`).  Beside it, in the same run, the NumPy restatement
tests/syncstats_ref.py of the same all-cells work on one host core (discrete outputs compared while at it), and
on the fixture tests/golden/syncstats/realistic.npz the distance of three sets of residuals from the exact ones:
np.polyfit's (recorded by the fixture's maker), the restatement's centred float64 fit, the device's.  Writes one
JSON record (default profiles/r17_syncstats.json); no figure is asserted anywhere."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402

import bench_tdoa  # noqa: E402
import syncstats_golden  # noqa: E402
import syncstats_ref  # noqa: E402
from thrifty_amd import _native, build, tdoa_est  # noqa: E402

BLOCK = 8192.0
DISCRETE = ("cell_key", "cell_ptr", "row_det", "row_match", "disc_ptr", "disc_idx", "cut_ptr", "cut_left", "cut_right",
            "cut_flags", "cell_counts", "cell_flags")
BSYNC_PHASES = ("copies_in_ms", "rows_and_cells_ms", "discontinuities_and_cuts_ms", "fits_and_summary_ms", "copies_out_ms")
TDSTATS_PHASES = ("copies_in_ms", "selection_and_cells_ms", "statistics_ms", "robust_ms", "copies_out_ms")


def scene(n_matches, seed=10):
    """bench_tdoa's scene with the receivers' SOAs re-timed: rates ascending by receiver (every cell's mean dsdoa
    is positive) and whole-block losses at receiver 3."""
    cols, ptr, idx, beacon_pos, rx_pos = bench_tdoa.scene(n_matches, seed)
    rng = np.random.default_rng(seed + 1)
    t = cols["timestamp"] - 1.7e9
    ppm = np.array([-30e-6, -10e-6, 8e-6, 30e-6])
    soa = (3600.0 * (1 + cols["rxid"]) + t) * bench_tdoa.FS * (1 + ppm[cols["rxid"]]) + rng.normal(0, 0.05, len(t))
    jumps = np.sort(rng.uniform(0, t.max(), max(1, int(t.max() / 500))))
    at3 = cols["rxid"] == 3
    soa[at3] += BLOCK * np.searchsorted(jumps, t[at3])
    cols = dict(cols, soa=soa, idx=np.arange(len(t), dtype=np.int64))
    return cols, ptr, idx, beacon_pos, rx_pos, len(jumps)


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def timed(call, times, phases, repeats):
    call()      # warm-up
    wall, parts = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        counts, out = call()
        wall.append(time.perf_counter() - t0)
        parts.append(times())
    rec = {"wall_ms": spread([1e3 * w for w in wall])}
    for k, name in enumerate(phases):
        rec[name] = spread([p[k] for p in parts])
    rec["device_ms"] = sum(rec[name]["median"] for name in phases[1:4])
    return rec, counts, out


def fixture_distances():
    """On the committed fixture, deg 2: the largest distance from the exact residuals, per source."""
    g = syncstats_golden.load("realistic")
    cols = syncstats_golden.beacon_columns(g)
    exact = syncstats_golden.exact("realistic", 2)
    restated = syncstats_golden.restated("realistic", 2)[1]
    device = _native.beaconsync(cols, g["match_ptr"], g["match_idx"], 2, beacons=syncstats_golden.BEACONS)[1]
    worst = lambda out: max(d for d, _ in syncstats_ref.residual_distances(cols, out, exact).values())   # noqa: E731
    return {"np_polyfit": max(float(np.max(v)) for k, v in g.items() if k.endswith("deg2_polyfit_distance") and len(v)),
            "centred_float64_restatement": worst(restated), "device": worst(device),
            "floor_32u_max_soa1": syncstats_ref.residual_floor(cols["soa"])}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matches", type=int, default=1 << 18)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--deg", type=int, default=2)
    ap.add_argument("--no-ref", action="store_true", help="skip the NumPy restatement")
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "r17_syncstats.json"))
    args = ap.parse_args()
    cols, ptr, idx, beacon_pos, rx_pos, n_jumps = scene(args.matches)
    beacons = sorted(beacon_pos)
    rec = {"csrc_hash": build.csrc_hash(), "receivers": bench_tdoa.N_RX, "beacons": len(beacons), "mobiles": bench_tdoa.N_MOBILE,
           "matches": args.matches, "detections": len(cols["rxid"]), "block_losses_at_receiver_3": n_jumps, "deg": args.deg,
           "repeats": args.repeats, "tile_and_workgroup": _native.syncstats_geometry("beaconsync")}

    bs, counts, out = timed(lambda: _native.beaconsync(cols, ptr, idx, args.deg, beacons=beacons),
                            lambda: _native.syncstats_times("beaconsync"), BSYNC_PHASES, args.repeats)
    bs.update(counts, fitted_cuts=int(np.sum(out["cut_flags"] == 1)), rows_per_s_device=counts["rows"] / (1e-3 * bs["device_ms"]))
    print(json.dumps(bs), flush=True)

    res = tdoa_est.tdoa_columns(cols, ptr, idx, bench_tdoa.WINDOW, beacon_pos, rx_pos, bench_tdoa.FS, args.deg)
    per_group = np.diff(res["group_ptr"])
    matrix = {"rx0": res["tdoas"]["rx0"], "rx1": res["tdoas"]["rx1"], "tx": np.repeat(res["tx"], per_group),
              "timestamp": np.repeat(res["timestamp"], per_group), "det0_idx": res["tdoas"]["det0_idx"],
              "det1_idx": res["tdoas"]["det1_idx"], "tdoa": res["tdoas"]["tdoa"]}
    td = {}
    for robust in (False, True):
        r, tcounts, tout = timed(lambda: _native.tdoastats(matrix, robust=robust), lambda: _native.syncstats_times("tdoastats"),
                                 TDSTATS_PHASES, args.repeats)
        r.update(tcounts, rows_per_s_device=tcounts["rows"] / (1e-3 * r["device_ms"]))
        if robust:
            r["outliers"] = int(tout["mask"].sum())
        td["robust" if robust else "plain"] = r
        print(json.dumps(r), flush=True)

    if not args.no_ref:
        t0 = time.perf_counter()
        ref_counts, ref = syncstats_ref.beacon_sync_ref(cols, ptr, idx, args.deg, beacons=beacons)
        took = time.perf_counter() - t0
        bs.update(restatement_one_core_s=took, restatement_over_device=took / (1e-3 * bs["device_ms"]),
                  restatement_over_wall=took / (1e-3 * bs["wall_ms"]["median"]),
                  discrete_outputs_equal_restatement=bool(ref_counts == counts and all(np.array_equal(out[k], ref[k]) for k in DISCRETE)),
                  largest_residual_difference=float(np.nanmax(np.abs(out["residual"] - ref["residual"]))))
        t0 = time.perf_counter()
        ref_counts, ref = syncstats_ref.tdoa_stats_ref(matrix, robust=True)
        took = time.perf_counter() - t0
        r = td["robust"]
        r.update(restatement_one_core_s=took, restatement_over_device=took / (1e-3 * r["device_ms"]),
                 restatement_over_wall=took / (1e-3 * r["wall_ms"]["median"]),
                 discrete_outputs_equal_restatement=bool(all(np.array_equal(tout[k], ref[k], equal_nan=True) for k in
                                                             ("cell_key", "cell_ptr", "order", "mask", "robust_count", "median"))))
    rec.update(beaconsync=bs, tdoastats=td, residual_distance_on_fixture=fixture_distances())
    print(json.dumps(rec["residual_distance_on_fixture"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
