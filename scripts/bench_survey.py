"""Measurement: the capture survey (thrifty_amd.survey.CaptureSurvey, integrate 100) over a raw u8 capture of
16384-sample blocks, history 0 and 4920, beside the carrier gate's verdict-only file loop (CarrierGate.run
with no output, the every-bin window, a threshold nothing passes) over the same file on the same box in the
same run -- both are synchronous chunk loops and the gate's carrier kernel is the nearest existing work.
Inputs: uniform bytes and bytes 126..129 (a quiet capture: the case the histogram layout is chosen for).
One untimed warm-up pass, then --repeats timed passes per case: median and range of blocks/s and input
GB/s.  Writes one JSON record (default profiles/r14_survey.json).  --fold adds one chunk through the fold
path (a THR_PATH_MULTIPASS handle) so that a kernel trace of this script sees its two kernels.  No figure
is asserted here."""
import argparse
import hashlib
import json
import os
import socket
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from thrifty_amd import _native, build, fastcard, survey  # noqa: E402

N = 16384


def build_capture(path, kind, n_bytes, seed):
    rng = np.random.default_rng(seed)
    lo, hi = (0, 256) if kind == "uniform" else (126, 130)
    chunk = rng.integers(lo, hi, 64 * 2 * N).astype(np.uint8).tobytes()
    with open(path, "wb") as f:
        for _ in range(-(-n_bytes // len(chunk))):
            f.write(chunk)
        f.truncate(n_bytes)
        f.flush()
        os.fsync(f.fileno())


def summary(passes, n_bytes):
    rate = [b / s for b, s in passes]
    return {"blocks": passes[0][0], "blocks_per_s_median": statistics.median(rate), "blocks_per_s_min": min(rate),
            "blocks_per_s_max": max(rate), "input_GBps_median": statistics.median(n_bytes / s / 1e9 for _, s in passes),
            "wall_s": [s for _, s in passes]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16384)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--integrate", type=int, default=100)
    ap.add_argument("--kinds", default="uniform,narrow")
    ap.add_argument("--fold", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_survey.json"))
    args = ap.parse_args()
    with open(os.path.join(build.CSRC, "survey.hip"), "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()[:16]
    record = {"what": "CaptureSurvey (integrate %d) and the carrier gate verdict-only over the same raw u8 capture, "
                      "block 16384" % args.integrate,
              "host": socket.gethostname(), "blocks": args.blocks, "batch_blocks": args.batch, "repeats": args.repeats,
              "csrc_sha16": build.csrc_hash(), "survey_hip_sha16": sha, "cases": {}}
    with tempfile.TemporaryDirectory() as tmpd:
        for kind in args.kinds.split(","):
            for h in (0, 4920):
                n_bytes = 2 * (N - h) * (args.blocks - 1) + 2 * N
                path = os.path.join(tmpd, "capture.bin")
                build_capture(path, kind, n_bytes, 7)
                case = {"history": h, "input": kind, "input_bytes": n_bytes}
                with survey.CaptureSurvey(N, h, integrate=args.integrate, batch_size=args.batch) as cs:
                    passes = []
                    for k in range(args.repeats + 1):        # pass 0 is the warm-up
                        with open(path, "rb") as f:
                            t0 = time.perf_counter()
                            n_int = sum(1 for _ in cs(f))
                            dt = time.perf_counter() - t0
                        if k:
                            passes.append((n_int * args.integrate, dt))
                    case["survey"] = summary(passes, n_bytes)
                with fastcard.CarrierGate(N, h, (0, -1), (3.0e38, 0.0), skip=0, batch_size=args.batch) as gate:
                    passes = []
                    for k in range(args.repeats + 1):
                        t0 = time.perf_counter()
                        st = gate.run(path, None)
                        dt = time.perf_counter() - t0
                        assert st["passed"] == 0
                        if k:
                            passes.append((st["blocks"], dt))
                    case["gate_verdict_only"] = summary(passes, n_bytes)
                case["survey_over_gate"] = (case["survey"]["blocks_per_s_median"] /
                                            case["gate_verdict_only"]["blocks_per_s_median"])
                record["cases"]["%s_h%d" % (kind, h)] = case
                print("%s h=%d: survey %.3f M blocks/s (%.3f .. %.3f) %.2f GB/s | gate %.3f M blocks/s %.2f GB/s | ratio %.2f" % (
                    kind, h, case["survey"]["blocks_per_s_median"] / 1e6, case["survey"]["blocks_per_s_min"] / 1e6,
                    case["survey"]["blocks_per_s_max"] / 1e6, case["survey"]["input_GBps_median"],
                    case["gate_verdict_only"]["blocks_per_s_median"] / 1e6, case["gate_verdict_only"]["input_GBps_median"],
                    case["survey_over_gate"]), flush=True)
                if args.fold and h == 0:
                    eng = _native.Engine.gate(N, 0, max_batch=1024, path="multipass")
                    with _native.Survey(eng, args.integrate) as s, open(path, "rb") as f:
                        s.feed_stream(f.read(1024 * 2 * N))
                    eng.close()
                os.unlink(path)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
