"""Measurement: the carrier gate (thr_run_gate_stream) over a raw capture of the kind bench.py builds for its
`raw_to_toad` leg -- the NEW samples of 64 synthetic c2 blocks (block 16384, history 4096) back to back,
tiled -- with 100 % of the blocks passing (threshold 0c0s) and with about 10 % passing (signal in 6 of the
64 seed blocks, window 7-110, threshold 0c100s).  One untimed warm-up pass, then --repeats timed passes
per case and sink: median and spread of blocks/s, input and output GB/s, and thr_gate_run_stats' split of
the median pass.  Sinks: a regular file (rewritten every pass) and /dev/null (what is left without the
file system).  Writes one JSON record (default profiles/r07_gate.json).  The yardstick is README's
raw_to_toad on the same box; no figure is asserted here."""
import argparse
import json
import mmap
import os
import socket
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from thrifty_amd import _native, synth  # noqa: E402


def build_capture(path, n, h, n_blocks, signal_blocks, seed):
    tpl = synth.gold_template(10, 2)
    rng = np.random.default_rng(seed)
    pad = h - len(tpl) + 1                                   # the unique window of lags (soa_estimator.py:20-39)
    win = (pad // 2, n - len(tpl) + 1 - (pad - pad // 2))
    seeds, _ = synth.synth_blocks(rng, 64, n, tpl, win, signal_frac=1.0)
    quiet, _ = synth.synth_blocks(rng, 64, n, tpl, win, signal_frac=0.0)
    step = 2 * (n - h)
    chunk = np.concatenate([(seeds if j in signal_blocks else quiet)[j][-step:] for j in range(64)]).tobytes()
    with open(path, "wb") as f:
        for _ in range(n_blocks // 64):
            f.write(chunk)
        f.flush()
        os.fsync(f.fileno())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=32768)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "r07_gate.json"))
    args = ap.parse_args()
    n, h = 16384, 4096
    record = {"what": "thr_run_gate_stream over a raw u8 I/Q capture (block 16384, history 4096)",
              "host": socket.gethostname(), "blocks": args.blocks, "batch_blocks": args.batch,
              "repeats": args.repeats, "csrc_sha16": None, "cases": {}}
    from thrifty_amd import build
    record["csrc_sha16"] = build.csrc_hash()
    with tempfile.TemporaryDirectory() as tmpd:
        cases = (("pass_100", set(range(64)), (0, -1), (0.0, 0.0)),
                 ("pass_10", {3, 14, 25, 36, 47, 58}, (7, 110), (0.0, 100.0)))
        for name, signal, window, threshold in cases:
            raw = os.path.join(tmpd, name + ".bin")
            build_capture(raw, n, h, args.blocks, signal, 7)
            f = open(raw, "rb")
            buf = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
            eng = _native.Engine.gate(n, h, window, threshold, max_batch=args.batch)
            case = {"window": list(window), "threshold": list(threshold), "input_bytes": len(buf), "sinks": {}}
            for sink in ("file", "devnull"):
                path = os.path.join(tmpd, name + ".card") if sink == "file" else os.devnull
                passes = []
                for k in range(args.repeats + 1):        # pass 0 is the warm-up
                    eng.input_window(buf)
                    with open(path, "wb") as out:
                        t0 = time.perf_counter()
                        st = eng.run_gate(buf, out_fd=out.fileno(), skip=1, batch_blocks=args.batch)
                        st["wall_s"] = time.perf_counter() - t0
                    eng.input_window(None)
                    if k:
                        passes.append(st)
                rate = [p["blocks"] / p["wall_s"] for p in passes]
                med = sorted(passes, key=lambda p: p["wall_s"])[len(passes) // 2]
                case["sinks"][sink] = {
                    "blocks": med["blocks"], "passed": med["passed"], "passed_frac": med["passed"] / max(1, med["blocks"]),
                    "blocks_per_s_median": statistics.median(rate), "blocks_per_s_min": min(rate),
                    "blocks_per_s_max": max(rate),
                    "input_GBps_median": statistics.median(p["bytes_in"] / p["wall_s"] / 1e9 for p in passes),
                    "output_GBps_median": statistics.median(p["text_bytes"] / p["wall_s"] / 1e9 for p in passes),
                    "wall_s": [p["wall_s"] for p in passes], "stats_of_median_pass": med}
                print("%s -> %s: %.3f M blocks/s median (%.3f .. %.3f), in %.2f GB/s, out %.2f GB/s, %.1f %% passed" % (
                    name, sink, statistics.median(rate) / 1e6, min(rate) / 1e6, max(rate) / 1e6,
                    case["sinks"][sink]["input_GBps_median"], case["sinks"][sink]["output_GBps_median"],
                    100 * case["sinks"][sink]["passed_frac"]))
                print("   split of the median pass: " + ", ".join("%s %.3f" % (k, med[k]) for k in (
                    "total_s", "frame_s", "gate_s", "wait_s", "format_s", "write_s")))
            record["cases"][name] = case
            eng.close()
            buf.close()
            f.close()
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
