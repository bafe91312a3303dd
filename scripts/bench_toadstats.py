"""Measurement: `thr_toadstats` on scripts/bench_match.py's scene (4 receivers, 8 transmitters) with the seven
further columns of a .toads line, at n = 2^16, 2^20 and 2^24 detections.  Per size: one warm-up call, then
--repeats calls; median and range of the wall time (every output fetched) and of its five event intervals
(copies in, sort and cells, reductions and histograms, fit, copies out: `thr_debug_toadstats_times`).  The
reduction kernels' achieved bytes/s -- the eleven sorted float64 columns read by pass 1 and by pass 2 and the
position tables, over the reductions' interval -- as a fraction of the HBM rate bench.py's roofline uses
beside profiles/hbm_traffic.json.  Beside it, in the same run, the NumPy restatement tests/toadstats_ref.py on
one host core (up to --ref-up-to detections; discrete outputs compared while at it), at 2^20 the reference's
own split_rxtx + print_stats where a reference checkout exists, and thr_match's recorded 4.33 ms per 2^20
detections as the yardstick for a sort-plus-scans stage.  Writes one JSON record (default
profiles/r16_toadstats.json); no figure is asserted anywhere."""
import argparse
import contextlib
import io
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

import bench_match  # noqa: E402
import toadstats_ref  # noqa: E402
from thrifty_amd import _native, build  # noqa: E402

HBM_BYTES_PER_S = 8000.0e9      # bench.py: HBM_PEAK_GBS
MATCH_YARDSTICK = "thr_match kernels 4.33 ms per 2^20 detections (DESIGN.md 3.10, profiles/r12_postdetect.json)"
REFERENCE = os.environ.get("THRIFTY_REFERENCE", "/root/reference")
DISCRETE = ("cell_rx", "cell_tx", "cell_ptr", "order", "minute_hist", "bin_first", "bin_hist", "offset_hist", "rx_count")


def columns(n, seed=9):
    rx, tx, ts, energy = bench_match.columns(n, seed)
    rng = np.random.default_rng(seed + 1)
    n = len(rx)
    return {"rxid": rx, "txid": tx, "timestamp": ts, "energy": energy, "noise": rng.uniform(2, 8, n),
            "carrier_bin": (40 + 3 * tx + rng.integers(-1, 2, n)).astype(np.int32), "carrier_offset": rng.uniform(-.5, .5, n),
            "carrier_energy": rng.uniform(80, 160, n), "carrier_noise": rng.uniform(4, 9, n),
            "offset": rng.uniform(-.5, .5, n), "soa": (ts - 1.7e9) * 2.4e6 * (1 + 20e-6 * rx) + rng.normal(0, 0.5, n)}


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def reference_seconds(cols):
    """The reference's split_rxtx + print_stats over the same detections, or None without a checkout."""
    if not os.path.isdir(os.path.join(REFERENCE, "thrifty")):
        return None
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, REFERENCE)
    from thrifty import toads_analysis
    data = np.zeros(len(cols["rxid"]), dtype=[      # the layout of the reference's toads_array
        ("idx", "i4"), ("rxid", "i4"), ("txid", "i4"), ("timestamp", "f8"), ("block", "i4"), ("soa", "f8"), ("sample", "i4"),
        ("offset", "f8"), ("energy", "f8"), ("noise", "f8"), ("carrier_bin", "i4"), ("carrier_offset", "f8"),
        ("carrier_energy", "f8"), ("carrier_noise", "f8")])
    for name in cols:
        data[name] = cols[name]
    t0 = time.perf_counter()
    data["timestamp"] -= np.min(data["timestamp"])
    with contextlib.redirect_stdout(io.StringIO()):
        for per_tx in toads_analysis.split_rxtx(data).values():
            for cell in per_tx.values():
                toads_analysis.print_stats(cell)
    return time.perf_counter() - t0


def measure(n, repeats, with_ref, with_reference):
    cols = columns(n)
    n = len(cols["rxid"])
    counts, out = _native.toadstats(cols)       # warm-up
    wall, parts = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        counts, out = _native.toadstats(cols)
        wall.append(time.perf_counter() - t0)
        parts.append(_native.toadstats_times())
    names = ("copies_in_ms", "sort_and_cells_ms", "reductions_ms", "fit_ms", "copies_out_ms")
    rec = {"n": n, "cells": counts["cells"], "receivers": counts["receivers"], "minute_bins": counts["minute_bins"],
           "wall_ms": spread([1e3 * w for w in wall])}
    for k, name in enumerate(names):
        rec[name] = spread([p[k] for p in parts])
    device_ms = sum(rec[name]["median"] for name in names[1:4])
    rec["device_ms"] = device_ms
    rec["detections_per_s_device"] = n / (1e-3 * device_ms)
    # two passes over eleven float64 columns, plus per pass the fragment and cell number of every position
    reduction_bytes = n * (2 * 11 * 8 + 4 + 8)
    rec["reduction_bytes"] = reduction_bytes
    rec["reduction_bytes_per_s"] = reduction_bytes / (1e-3 * rec["reductions_ms"]["median"])
    rec["reduction_fraction_of_hbm"] = rec["reduction_bytes_per_s"] / HBM_BYTES_PER_S
    if with_ref:
        t0 = time.perf_counter()
        ref_counts, ref = toadstats_ref.toad_stats_ref(cols)
        took = time.perf_counter() - t0
        rec["restatement_one_core_s"] = took
        rec["restatement_over_device"] = took / (1e-3 * device_ms)
        rec["restatement_over_wall"] = took / statistics.median(wall)
        rec["discrete_outputs_equal_restatement"] = bool(all(np.array_equal(out[k], ref[k]) for k in DISCRETE))
        rec["largest_mean_difference_relative"] = float(np.max(np.abs(out["stats"][:, :, 0] - ref["stats"][:, :, 0]) /
                                                               np.abs(ref["stats"][:, :, 0])))
    if with_reference:
        rec["reference_split_and_print_s"] = reference_seconds(cols)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1 << 16, 1 << 20, 1 << 24])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ref-up-to", type=int, default=1 << 20, help="largest n the NumPy restatement is run at")
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "r16_toadstats.json"))
    args = ap.parse_args()
    runs = []
    for n in args.sizes:
        runs.append(measure(n, args.repeats, n <= args.ref_up_to, n == 1 << 20))
        print(json.dumps(runs[-1]), flush=True)
    tile, workgroup = _native.toadstats_geometry()
    rec = {"csrc_hash": build.csrc_hash(), "receivers": bench_match.N_RX, "transmitters": bench_match.N_TX,
           "repeats": args.repeats, "tile": tile, "workgroup": workgroup, "hbm_bytes_per_s": HBM_BYTES_PER_S,
           "match_yardstick": MATCH_YARDSTICK, "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
