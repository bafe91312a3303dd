"""Measurement: detection dossiers (thr_dossier_*: the scan plus thr_dossier_result for every array) against
the only route before them -- the reference's loop over Detector(yield_data=True), one block per call with
two N-point dumps across the link, plus the NumPy statement tests/dossier_ref.py for the kept blocks -- on
the same input: the 2048-block prefix of the .card capture scripts/bench_extract.py builds (block 16384,
history 4096, 1023-chip template, every block carries a burst), `-i 0- -m 64`.

Both routes stop where the reference's loop stops, at the block that fills the last of the 64 slots; the
device route has by then scanned the whole batch that block came in.  The detector is built once per route,
outside the timed passes.  One untimed warm-up pass, then --repeats timed passes: median and range of the
wall time, scan and result apart.  Writes one JSON record (default profiles/r18_dossier.json); no figure is
asserted anywhere."""
import argparse
import json
import os
import socket
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402

import bench_extract  # noqa: E402  (the capture)
import dossier_ref  # noqa: E402
from thrifty_amd import build, detect_analysis  # noqa: E402
from thrifty_amd.block_data import CardStream, card_reader  # noqa: E402
from thrifty_amd.detect import Detector, DetectorSettings  # noqa: E402

N, H = bench_extract.N, bench_extract.H
RANGES = [(0, None)]


def summary(walls):
    return {"median_s": statistics.median(walls), "min_s": min(walls), "max_s": max(walls), "wall_s": walls}


def device_route(path, forcible, max_keep, repeats):
    scans, results, totals, last = [], [], [], None
    for k in range(repeats + 1):             # pass 0 is the warm-up
        with open(path, "rb") as f:
            t0 = time.perf_counter()
            dos, samples = detect_analysis.scan(forcible, CardStream(f, N), RANGES, max_keep)
            t1 = time.perf_counter()
            got = dos.result()
            t2 = time.perf_counter()
            last = (dos.n_kept, dos.n_checked, dos.n_skipped, got)
            dos.close()
        if k:
            scans.append(t1 - t0)
            results.append(t2 - t1)
            totals.append(t2 - t0)
    return {"scan": summary(scans), "result": summary(results), "total": summary(totals)}, last


def yield_data_route(path, settings, max_keep, repeats):
    loops, refs, totals, kept = [], [], [], None
    det = Detector(settings, yield_data=True)
    try:
        for k in range(repeats + 1):
            with open(path, "rb") as f:
                t0 = time.perf_counter()
                kept = []
                for timestamp, block_idx, block in card_reader(f):
                    if not detect_analysis.block_in_range(block_idx, RANGES):
                        continue
                    detected, result, shifted, corr = det.detect(timestamp, block_idx, block)
                    if detected:
                        kept.append((block_idx, block, np.fft.ifft(shifted), corr))
                        if len(kept) >= max_keep:
                            break
                t1 = time.perf_counter()
                for block_idx, block, _, _ in kept:
                    dossier_ref.numbers(np.asarray(block.raw, dtype=np.uint8), block_idx, settings)
                t2 = time.perf_counter()
            if k:
                loops.append(t1 - t0)
                refs.append(t2 - t1)
                totals.append(t2 - t0)
    finally:
        det.close()
    return {"loop": summary(loops), "statement": summary(refs), "total": summary(totals)}, kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_dossier.json"))
    args = ap.parse_args()
    record = {"what": "detection dossiers (scan + result, every array) against Detector(yield_data=True) in a loop "
                      "plus tests/dossier_ref.py for the kept blocks; 2048-block .card prefix, -i 0- -m %d" % args.max,
              "host": socket.gethostname(), "repeats": args.repeats, "max_keep": args.max,
              "csrc_sha16": build.csrc_hash()}
    with tempfile.TemporaryDirectory() as tmpd:
        _, _, prefix, tpl, _ = bench_extract.build_inputs(tmpd, 4096)
        settings = DetectorSettings(N, H, len(tpl), bench_extract.THR, bench_extract.WINDOW, tpl, bench_extract.THR)
        forcible = detect_analysis.ForcibleDetector(settings, batch_size=2048)
        try:
            record["device"], last = device_route(prefix, forcible, args.max, args.repeats)
        finally:
            forcible.close()
        record["yield_data"], kept = yield_data_route(prefix, settings, args.max, args.repeats)
    record["kept"] = {"device": [int(v) for v in last[3]["records"]["block_idx"]], "yield_data": [int(k[0]) for k in kept],
                      "n_checked": last[1], "n_skipped": last[2]}
    record["same_blocks_kept"] = record["kept"]["device"] == record["kept"]["yield_data"]
    synced = max(float(np.linalg.norm(last[3]["synced"][i] - kept[i][2]) / np.linalg.norm(kept[i][2])) for i in range(len(kept)))
    record["synced_rel_l2_against_yield_data_max"] = synced
    record["yield_data_over_device_total"] = record["yield_data"]["total"]["median_s"] / record["device"]["total"]["median_s"]
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: record[k] for k in ("same_blocks_kept", "yield_data_over_device_total",
                                             "synced_rel_l2_against_yield_data_max")}))
    print("device", record["device"]["total"], "\nyield_data", record["yield_data"]["total"])


if __name__ == "__main__":
    main()
