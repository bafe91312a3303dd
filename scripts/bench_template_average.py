"""Measurement: what averaging costs the extraction's whole-file loop, and that the loop WITHOUT it is the
parent commit's.

Capture: scripts/bench_extract.py's (block 16384, history 4096, 1023-chip template, every block carries a
burst), as .card text and as a raw stream, built once.  Loops, each `thr_extract_reset`, the whole file
through thr_run_extract_card / thr_run_extract_stream, and the results:
  plain     this tree, averaging not armed (launches nothing new)
  average   this tree, averaging armed, one class
  parent    a checkout of the parent commit with its library built (--parent-root), same loop as `plain`
Every loop runs in a worker process of its own (one library per process); a worker does one warm-up pass and
then --repeats timed passes and reports their median.  The workers are alternated for --rounds rounds, the order
rotating by one from round to round (no variant always runs behind the same other one), so each variant has
`rounds` medians.  The margin for "plain is the parent's loop" is the
parent's own spread over its medians (max - min); nothing is asserted, the record says
whether the difference of the variants' medians lies inside it.  Writes profiles/r30_template_average.json."""
import argparse
import json
import mmap
import os
import socket
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(args):
    """One variant, one round: -> JSON on stdout."""
    sys.path.insert(0, args.package_root)
    sys.path.insert(1, os.path.join(ROOT, "scripts"))
    import numpy as np
    from thrifty_amd import _native, synth
    import bench_extract as be
    tpl = synth.gold_template(10, 2).astype(np.float64)
    eng = _native.Engine(be.N, be.H, tpl, be.THR, be.WINDOW, be.THR, carrier_len=len(tpl), max_batch=args.batch)
    x = _native.Extraction(eng)
    if args.worker == "average":
        x.average(())
    out = {}
    for name in ("card", "raw"):
        f = open(os.path.join(args.inputs, "rx.card" if name == "card" else "rx.bin"), "rb")
        buf = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
        view = memoryview(buf) if name == "card" else memoryview(buf)[be.STEP - be.CARRY:]
        walls, blocks, counted = [], 0, None
        for k in range(args.repeats + 1):           # pass 0 is the warm-up
            t0 = time.perf_counter()
            x.reset()
            eng.input_window(buf)
            try:
                st = x.run(view, card=name == "card", first_block_idx=1, timestamp=0.0, batch_blocks=args.batch)
            finally:
                eng.input_window(None)
            rec, _, _, nq = x.result(len(tpl))
            if args.worker == "average":
                counted = int(x.average_counts()[0][0])
                x.average_result(0, len(tpl))
            if k:
                walls.append(time.perf_counter() - t0)
            blocks = int(st["blocks"])
        out[name] = {"blocks": blocks, "wall_s": walls, "blocks_per_s_median": blocks / statistics.median(walls),
                     "n_qualifying": int(nq), "averaged": counted, "picked_block": int(rec["block_idx"])}
        del view
        buf.close()
        f.close()
    x.close()
    eng.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=32768)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit, library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_template_average.json"))
    ap.add_argument("--worker", default=None, choices=["plain", "average", "parent"])
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--inputs", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.join(ROOT, "scripts"))
    import bench_extract as be
    from thrifty_amd import build
    variants = ["plain", "average"] + (["parent"] if args.parent_root else [])
    record = {"what": "thr_run_extract_card / _stream over scripts/bench_extract.py's capture: averaging armed "
                      "against not armed, and not armed against the parent commit's library",
              "host": socket.gethostname(), "blocks": args.blocks, "batch_blocks": args.batch, "repeats": args.repeats,
              "rounds": args.rounds, "csrc_sha16": build.csrc_hash(), "medians_blocks_per_s": {}, "workers": []}
    with tempfile.TemporaryDirectory() as tmpd:
        be.build_inputs(tmpd, args.blocks)
        for rnd in range(args.rounds):
            for v in variants[rnd % len(variants):] + variants[:rnd % len(variants)]:
                root = os.path.abspath(args.parent_root) if v == "parent" else ROOT
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", v, "--package-root", root, "--inputs", tmpd,
                       "--repeats", str(args.repeats), "--batch", str(args.batch)]
                text = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=300).stdout.decode()
                got = json.loads([line for line in text.splitlines() if line.startswith("RESULT ")][-1][7:])
                record["workers"].append({"round": rnd, "variant": v, "result": got})
                for name, case in got.items():
                    record["medians_blocks_per_s"].setdefault(name, {}).setdefault(v, []).append(case["blocks_per_s_median"])
                print("round %d %-7s card %.3f raw %.3f M blocks/s" % (rnd, v, got["card"]["blocks_per_s_median"] / 1e6,
                                                                      got["raw"]["blocks_per_s_median"] / 1e6), flush=True)
    record["summary"] = {}
    for name, per in record["medians_blocks_per_s"].items():
        s = {v: statistics.median(per[v]) for v in per}
        s["average_over_plain"] = s["average"] / s["plain"]
        if "parent" in per:
            s["parent_spread"] = max(per["parent"]) - min(per["parent"])
            s["plain_minus_parent"] = s["plain"] - s["parent"]
            s["plain_within_parent_spread"] = abs(s["plain_minus_parent"]) <= s["parent_spread"]
        record["summary"][name] = s
        print(name, json.dumps(s))
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
