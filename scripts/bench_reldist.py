"""Measurement: `thr_reldist` on scripts/bench_syncstats.py's scene (4 receivers, 2 beacons + 6 mobiles; 2^18
transmissions = 2^20 detections; carriers drawn here) for every (mobile, beacon, rx0 < rx1) cell, both methods,
smoothing on.  Per method: one warm-up, then --repeats calls; median and range of the wall time with every array
fetched and of the five event intervals (`thr_debug_reldist_times`); the smoother's share of the device time and
the weighted terms per second it achieves (a point of a series of m points sums k = max(2, min(m, int(frac m)))
terms).  Beside it the NumPy statement tests/reldist_ref.py on one host core, EXTRAPOLATED and marked so: everything
but the smoother is timed on the first --ref-matches matches and scaled by the rows; the smoother's per-point loop
is timed on --ref-points points (each summing as many terms) and scaled by the weighted terms.
Each method's GPU step runs in a process of its own under `timeout`; a step that fails ends the run.
Writes one JSON record (default profiles/r20_reldist.json); no figure is asserted anywhere."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402

import bench_syncstats  # noqa: E402
import bench_tdoa  # noqa: E402
import reldist_ref  # noqa: E402
from thrifty_amd import _native, build, reldist  # noqa: E402

PHASES = ("copies_in_ms", "rows_and_cells_ms", "distances_masks_statistics_ms", "smoothers_ms", "copies_out_ms")


def scene(n_matches, seed=10):
    cols, ptr, idx, beacon_pos, rx_pos, _ = bench_syncstats.scene(n_matches, seed)
    rng = np.random.default_rng(seed + 2)
    carrier = 300.0 + 5.0 * cols["txid"] + rng.normal(0, 0.05, len(cols["txid"]))
    cols = dict(cols, carrier_bin=np.floor(carrier), carrier_offset=carrier - np.floor(carrier))
    return cols, ptr, idx, beacon_pos, rx_pos


def weighted_terms(out, frac):
    total = 0
    for stem in ("speed", "dop"):
        m = np.diff(out[stem + "_smooth_ptr"])
        total += sum(int(v) * reldist_ref.window_len(int(v), frac) for v in m if v >= 2)
    return total


def measure(args, method):
    """One method's record: the GPU step a child process runs under its own time limit."""
    cols, ptr, idx, beacon_pos, rx_pos = scene(args.matches)
    beacons = sorted(beacon_pos)
    geometry = reldist.geometry_table(rx_pos, beacon_pos, bench_tdoa.FS)
    call = lambda: _native.reldist(cols, ptr, idx, beacons, method=method, smooth_frac=args.frac, geometry=geometry)   # noqa: E731
    r, counts, out = bench_syncstats.timed(call, _native.reldist_times, PHASES, args.repeats)
    terms = weighted_terms(out, args.frac)
    r.update(counts, detections=len(cols["rxid"]), flagged_cells=int(np.count_nonzero(out["cell_flags"])),
             outliers=int(out["mask1"].sum()), weighted_terms=terms,
             weighted_terms_per_s=terms / (1e-3 * r["smoothers_ms"]["median"]),
             smoother_share_of_device=r["smoothers_ms"]["median"] / r["device_ms"],
             rows_per_s_device=counts["rows"] / (1e-3 * r["device_ms"]), tile_workgroup_point_lanes=_native.reldist_geometry())
    return r


def statement(args, rows, terms):
    """The NumPy statement on one core, extrapolated: the rest by rows, the smoother by weighted terms."""
    cols, ptr, idx, beacon_pos, rx_pos = scene(args.matches)
    m = min(args.ref_matches, args.matches)
    t0 = time.perf_counter()
    ref_counts, ref = reldist_ref.reldist_ref(cols, ptr[:m + 1], idx[:int(ptr[m])], sorted(beacon_pos), method="linpol", smooth_frac=0.0,
                                              geometry=reldist.geometry_table(rx_pos, beacon_pos, bench_tdoa.FS))
    rest = (time.perf_counter() - t0) * rows / ref_counts["rows"]
    n = min(args.ref_points, ref_counts["dop_points"])
    t0 = time.perf_counter()
    reldist_ref.smooth(ref["dop_smooth_x"][:n], ref["dop_smooth"][:n], 1.0)       # n points, n terms each
    smoother = (time.perf_counter() - t0) / (n * n) * terms
    return {"extrapolated": True, "rest_timed_on_matches": m, "smoother_timed_on_terms": n * n, "rest_s": rest,
            "smoother_s": smoother, "total_s": rest + smoother}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matches", type=int, default=1 << 18)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frac", type=float, default=0.025)
    ap.add_argument("--ref-matches", type=int, default=1 << 13)
    ap.add_argument("--ref-points", type=int, default=160)
    ap.add_argument("--no-ref", action="store_true", help="skip the NumPy statement")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a GPU step may take")
    ap.add_argument("--child", default=None, help="(internal) run one method's GPU step and print its record")
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "r20_reldist.json"))
    args = ap.parse_args()
    if args.child:
        print("RECORD " + json.dumps(measure(args, args.child)), flush=True)
        return 0
    rec = {"csrc_hash": build.csrc_hash(), "receivers": bench_tdoa.N_RX, "beacons": bench_tdoa.N_BEACON, "mobiles": bench_tdoa.N_MOBILE,
           "matches": args.matches, "smooth_frac": args.frac, "repeats": args.repeats}
    for method in ("nearest", "linpol"):       # each GPU step in a process of its own, under its own time limit
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", method,
               "--matches", str(args.matches), "--repeats", str(args.repeats), "--frac", str(args.frac)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [line for line in done.stdout.splitlines() if line.startswith("RECORD ")]
        if done.returncode != 0 or not lines:
            sys.stderr.write("step %s ended with status %d: nothing more is run\n" % (method, done.returncode))
            return 1
        rec[method] = json.loads(lines[-1][7:])
        print(json.dumps(rec[method]), flush=True)
    if not args.no_ref:
        r = statement(args, rec["linpol"]["rows"], rec["linpol"]["weighted_terms"])
        r.update(over_device=r["total_s"] / (1e-3 * rec["linpol"]["device_ms"]), over_wall=r["total_s"] / (1e-3 * rec["linpol"]["wall_ms"]["median"]))
        rec["statement_one_core_extrapolated"] = r
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
