"""Measurement: template extraction's whole-file loop (thr_run_extract_card / thr_run_extract_stream) against
the plain detect loop (thr_run_card / thr_run_stream, no text: out_fd = -1, records into an array) in the
same process on the same file, and against the only route to a template before it -- Python over
Detector(yield_data=True), two N-point dumps per block across PCIe -- on a 2048-block prefix.

Input: the capture scripts/bench_gate.py builds (the new samples of 64 synthetic c2 blocks, block 16384,
history 4096, back to back, tiled; every block carries a burst) as a raw file, and its .card twin: the
same overlapping blocks behind the zero-history lead-in block, one line each.  One untimed warm-up pass,
then --repeats timed passes per loop: median and range of blocks/s.  An extraction pass includes
thr_extract_reset and thr_extract_result.  Writes one JSON record (default profiles/r08_extract.json); no
figure is asserted anywhere."""
import argparse
import base64
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

from thrifty_amd import _native, build, synth  # noqa: E402
from thrifty_amd.block_data import CardStream  # noqa: E402
from thrifty_amd.detect import Detector, DetectorSettings  # noqa: E402

N, H = 16384, 4096
STEP, CARRY = 2 * (N - H), 2 * H
THR, WINDOW = (0, 15, 0), (7, 110)


def build_inputs(tmpd, n_blocks, seed=7):
    """-> (raw path, card path, prefix card path, template, blocks behind the lead-in)."""
    tpl = synth.gold_template(10, 2).astype(np.float64)
    pad = H - len(tpl) + 1
    win = (pad // 2, N - len(tpl) + 1 - (pad - pad // 2))
    seeds, _ = synth.synth_blocks(np.random.default_rng(seed), 64, N, tpl, win)
    chunk = np.concatenate([seeds[j][-STEP:] for j in range(64)])
    raw = os.path.join(tmpd, "rx.bin")
    with open(raw, "wb") as f:
        for _ in range(n_blocks // 64):
            f.write(chunk.tobytes())
    # block j >= 1 of the stream starts STEP * j - CARRY bytes into it; the tiling makes them periodic in 64
    two = np.concatenate([chunk, chunk, chunk])
    payload = [base64.b64encode(two[STEP * j - CARRY:STEP * j - CARRY + 2 * N].tobytes()).decode()
               for j in range(1, 65)]
    n_card = (n_blocks // 64 * 64 * STEP - (STEP - CARRY) - 2 * N) // STEP + 1      # whole blocks behind the lead-in block
    paths = []
    for name, count in (("rx.card", n_card), ("prefix.card", 2048)):
        path = os.path.join(tmpd, name)
        with open(path, "w") as f:
            for j in range(1, count + 1):
                f.write("%d.%06d %d %s\n" % (1475000000 + j // 100, (j % 100) * 10000, j, payload[(j - 1) % 64]))
        paths.append(path)
    return raw, paths[0], paths[1], tpl, n_card


def timed(passes, fn):
    out = []
    for k in range(passes + 1):          # pass 0 is the warm-up
        t0 = time.perf_counter()
        st = fn()
        st["wall_s"] = time.perf_counter() - t0
        if k:
            out.append(st)
    rate = [p["blocks"] / p["wall_s"] for p in out]
    med = sorted(out, key=lambda p: p["wall_s"])[len(out) // 2]
    return {"blocks": med["blocks"], "blocks_per_s_median": statistics.median(rate), "blocks_per_s_min": min(rate),
            "blocks_per_s_max": max(rate), "wall_s": [p["wall_s"] for p in out],
            "stats_of_median_pass": {k: v for k, v in med.items() if not isinstance(v, (dict, list, tuple))}}


def yield_data_route(path, settings, max_offset=0.2):
    """What the parent commit offers: the reference's loop over Detector(yield_data=True)."""
    best = None
    with open(path, "rb") as f, Detector(settings, CardStream(f, N), yield_data=True) as det:
        n = 0
        for detected, result, spectrum, _ in det:
            n += 1
            if detected and abs(result.corr_info.offset) <= max_offset and (
                    best is None or result.corr_info.energy > best[0].corr_info.energy):
                best = (result, np.array(spectrum))
    signal = np.fft.ifft(best[1])
    at = best[0].corr_info.sample
    cut = np.abs(signal[at:at + len(settings.template)])
    cut = cut * (2 / (cut.mean() + cut.std()))
    return {"blocks": n, "block": best[0].block, "template": cut - cut.mean()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=32768)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "r08_extract.json"))
    args = ap.parse_args()
    record = {"what": "template extraction's file loop against the plain detect loop on the same file "
                      "(block 16384, history 4096, 1023-chip template, every block carries a burst)",
              "host": socket.gethostname(), "blocks": args.blocks, "batch_blocks": args.batch,
              "repeats": args.repeats, "csrc_sha16": build.csrc_hash(), "cases": {}}
    with tempfile.TemporaryDirectory() as tmpd:
        raw, card, prefix, tpl, n_card = build_inputs(tmpd, args.blocks)
        settings = DetectorSettings(N, H, len(tpl), THR, WINDOW, tpl, THR)
        eng = _native.Engine(N, H, tpl, THR, WINDOW, THR, carrier_len=len(tpl), max_batch=args.batch)
        x = _native.Extraction(eng)
        rec_out = np.zeros(args.blocks, dtype=_native.RECORD_DTYPE)
        picks = {}
        for name, path in (("card", card), ("raw", raw)):
            f = open(path, "rb")
            buf = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
            view = memoryview(buf) if name == "card" else memoryview(buf)[STEP - CARRY:]

            def windowed(call):
                eng.input_window(buf)
                try:
                    return call()
                finally:
                    eng.input_window(None)

            def extraction():
                x.reset()
                st = windowed(lambda: x.run(view, card=name == "card", first_block_idx=1, timestamp=0.0,
                                            batch_blocks=args.batch))
                picks[name] = x.result(len(tpl))
                return st

            def plain():
                if name == "card":
                    return windowed(lambda: eng.run_card(view, batch_blocks=args.batch, rec_out=rec_out))
                return windowed(lambda: eng.run_stream(view, first_block_idx=1, batch_blocks=args.batch,
                                                       rec_out=rec_out, timestamp=0.0))

            case = {"input_bytes": len(buf), "extract": timed(args.repeats, extraction),
                    "plain": timed(args.repeats, plain)}
            case["extract_over_plain"] = (case["extract"]["blocks_per_s_median"] /
                                          case["plain"]["blocks_per_s_median"])
            rec, _, _, nq = picks[name]
            case["picked_block"], case["n_qualifying"] = int(rec["block_idx"]), int(nq)
            print("%s: extraction %.3f M blocks/s median (%.3f .. %.3f), plain loop %.3f (%.3f .. %.3f): ratio %.3f"
                  % (name, case["extract"]["blocks_per_s_median"] / 1e6, case["extract"]["blocks_per_s_min"] / 1e6,
                     case["extract"]["blocks_per_s_max"] / 1e6, case["plain"]["blocks_per_s_median"] / 1e6,
                     case["plain"]["blocks_per_s_min"] / 1e6, case["plain"]["blocks_per_s_max"] / 1e6,
                     case["extract_over_plain"]))
            record["cases"][name] = case
            del view
            buf.close()
            f.close()
        # the 2048-block prefix: both routes, same file
        f = open(prefix, "rb")
        buf = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)

        def prefix_extraction():
            x.reset()
            st = x.run(buf, card=True, batch_blocks=args.batch)
            picks["prefix"] = x.result(len(tpl))
            return st

        new = timed(args.repeats, prefix_extraction)
        buf.close()
        f.close()
        x.close()
        eng.close()
        olds = {}

        def old_route():
            olds.update(yield_data_route(prefix, settings))
            return {"blocks": olds["blocks"]}

        old = timed(args.repeats, old_route)
        rec, _, template, _ = picks["prefix"]
        record["cases"]["prefix_2048"] = {
            "extract": new, "yield_data_python": old,
            "speedup": new["blocks_per_s_median"] / old["blocks_per_s_median"],
            "same_block": int(rec["block_idx"]) == int(olds["block"]),
            "max_abs_template_difference": float(np.max(np.abs(template - olds["template"])))}
        print("2048-block prefix: extraction %.0f blocks/s, yield_data route %.0f blocks/s: x%.1f; same block: %s, "
              "templates differ by %.2g" % (new["blocks_per_s_median"], old["blocks_per_s_median"],
                                            record["cases"]["prefix_2048"]["speedup"],
                                            record["cases"]["prefix_2048"]["same_block"],
                                            record["cases"]["prefix_2048"]["max_abs_template_difference"]))
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
