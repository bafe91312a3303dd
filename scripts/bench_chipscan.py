"""Measurement: the chip-rate scan (thr_chipscan) on 64 blocks x 128 candidate lengths around 2455, block
16384.  One warm-up call, then --repeats timed calls: median wall time of the call, its device time by events
split into carrier stage / bank kernel / scan + finish kernels (thr_debug_chipscan_times), and the rate in
(block, length) pairs per second.  Beside it, from the same run on the same box:

  * the yardstick: k_correlate's time per (block, template) on an unsectioned one-template handle of the same
    geometry (template 2455 samples), from thr_profile_read (total kernel time over total blocks), over as many
    blocks per call as the scan has pairs (the 64 blocks repeated) -- a pair of the scan costs one product +
    inverse + reduction, the same work less the block's forward transform; k_carrier's time per block from the
    same profile stands for a forward transform;
  * tests/chipscan_ref.py (float64 NumPy, one host core) on the same inputs, and how the device's records
    compare with it.

This script itself never touches the device: every step is a child process under its own `timeout -k 10`, and
the first failing step ends the run.  Writes one JSON record (default profiles/r15_chipscan.json); no figure
is asserted anywhere."""
import argparse
import hashlib
import json
import os
import socket
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N = 16384
CARRIER_LEN = 2455
STEPS = (("device", 300), ("ref", 600))      # (step, its time limit in seconds)


def inputs(n_blocks, n_lengths):
    import numpy as np
    import chipscan_ref
    from thrifty_amd import synth
    rng = np.random.default_rng(15)
    chips = synth.gold_code(10, 0)
    blocks = np.stack([chipscan_ref.burst_block(rng, chips, 2461, int(rng.integers(1, N - 2461 - 1)),
                                                carrier_bin=float(rng.uniform(-500, 500))) for _ in range(n_blocks)])
    lengths = (CARRIER_LEN - n_lengths // 2 + np.arange(n_lengths)).astype(np.int32)
    return blocks, chips, lengths


def step_device(args, scratch):
    import numpy as np
    from thrifty_amd import _native, synth
    blocks, chips, lengths = inputs(args.blocks, args.lengths)
    pairs = len(blocks) * len(lengths)
    own = synth.gold_template(10, 0, CARRIER_LEN / 1023.0)
    assert len(own) == CARRIER_LEN
    out = {"pairs": pairs}
    eng = _native.Engine(N, len(own) - 1, own, (100.0, 0.0, 0.0), None, (0.0, 0.0, 0.0), carrier_len=CARRIER_LEN,
                         max_batch=len(blocks))
    scan = _native.ChipScan(eng)
    out["candidates_per_chunk"], out["paired"] = scan.geometry(len(lengths))
    wall, dev = [], []
    for k in range(args.repeats + 1):            # call 0 is the warm-up
        t0 = time.perf_counter()
        records = scan.scan(blocks, chips, lengths)
        dt = time.perf_counter() - t0
        if k:
            wall.append(dt * 1e3)
            dev.append(scan.times())
    eng.close()
    np.save(os.path.join(scratch, "records.npy"), records)
    med = [statistics.median(d[i] for d in dev) for i in range(3)]
    out["call_wall_ms"] = {"median": statistics.median(wall), "all": wall}
    out["device_ms"] = {"carrier_stage": med[0], "bank_kernel": med[1], "scan_kernels": med[2], "sum": sum(med),
                        "all": [list(d) for d in dev]}
    out["pairs_per_s_device"] = pairs / (sum(med) * 1e-3)
    out["pairs_per_s_wall"] = pairs / (statistics.median(wall) * 1e-3)
    out["us_per_pair_scan_kernels"] = med[2] * 1e3 / pairs
    out["us_per_candidate_bank_kernel"] = med[1] * 1e3 / len(lengths)
    # the yardstick: as many (block, template) items as the scan has pairs
    many = np.ascontiguousarray(np.tile(blocks, (pairs // len(blocks), 1)))
    eng = _native.Engine(N, len(own) - 1, own, (100.0, 0.0, 0.0), None, (0.0, 0.0, 0.0), carrier_len=CARRIER_LEN,
                         max_batch=len(many), path="unsectioned")
    eng.detect(many)                              # warm-up
    eng.profile_enable(1)
    for _ in range(args.repeats):
        rec = eng.detect(many)
    prof = eng.profile_read()
    eng.close()
    assert int(((rec["flags"][:, 0] & 1) != 0).sum()) == len(many)
    # (a detect call cuts its input into chunks of 64 MiB, one launch of every kernel per chunk: the totals count)
    total_blocks = args.repeats * len(many)
    out["yardstick"] = {"blocks_per_call": len(many), "calls": args.repeats, "path": "unsectioned",
                        "template_len": CARRIER_LEN, "kernels_ms_total": {k: v[0] for k, v in prof.items()},
                        "launches": {k: v[1] for k, v in prof.items()}}
    out["yardstick"]["us_per_block_template_k_correlate"] = prof["k_correlate"][0] * 1e3 / total_blocks
    out["yardstick"]["us_per_block_k_carrier"] = prof["k_carrier"][0] * 1e3 / total_blocks
    out["pair_over_yardstick"] = out["us_per_pair_scan_kernels"] / out["yardstick"]["us_per_block_template_k_correlate"]
    return out


def step_ref(args, scratch):
    import numpy as np
    import chipscan_ref
    blocks, chips, lengths = inputs(args.blocks, args.lengths)
    t0 = time.perf_counter()
    ref = chipscan_ref.scan(blocks, chips, lengths, CARRIER_LEN)
    dt = time.perf_counter() - t0
    got = np.load(os.path.join(scratch, "records.npy"))
    sure = ref["top2_gap"] >= 1e-4
    smooth = sure & (ref["curvature"] > 1e-4)
    return {"seconds": dt, "pairs_per_s": ref.size / dt, "ms_per_pair": dt * 1e3 / ref.size,
            "device_against_ref": {
                "near_ties_left_out": int((~sure).sum()),
                "sample_mismatches": int((got["sample"][sure] != ref["sample"][sure]).sum()),
                "flag_mismatches": int((got["flags"] != ref["flags"]).sum()),
                "energy_max_rel": float(np.max(np.abs(got["energy"] - ref["energy"]) / ref["energy"])),
                "noise_max_rel": float(np.max(np.abs(got["noise"] - ref["noise"]) / ref["noise"])),
                "offset_max_abs": float(np.max(np.abs(got["offset"][smooth] - ref["offset"][smooth]))),
                "best_length_device": int(lengths[np.argmax(got["energy"].astype(np.float64).mean(axis=0))]),
                "best_length_ref": int(lengths[np.argmax(ref["energy"].mean(axis=0))])}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--lengths", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_chipscan.json"))
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--scratch", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        result = {"device": step_device, "ref": step_ref}[args.step](args, args.scratch)
        with open(os.path.join(args.scratch, args.step + ".json"), "w") as f:
            json.dump(result, f)
        return 0
    from thrifty_amd import build
    sha = hashlib.sha256()
    for name in build.UNPROFILED_CHIPSCAN:
        with open(os.path.join(build.CSRC, name), "rb") as f:
            sha.update(f.read())
    record = {"what": "thr_chipscan, %d blocks x %d lengths around %d, block 16384; medians of %d calls after a warm-up"
                      % (args.blocks, args.lengths, CARRIER_LEN, args.repeats),
              "host": socket.gethostname(), "blocks": args.blocks, "lengths": args.lengths, "repeats": args.repeats,
              "csrc_sha16": build.csrc_hash(), "chipscan_sha16": sha.hexdigest()[:16]}
    with tempfile.TemporaryDirectory() as scratch:
        for step, limit in STEPS:
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step,
                   "--scratch", scratch, "--blocks", str(args.blocks), "--lengths", str(args.lengths),
                   "--repeats", str(args.repeats)]
            rc = subprocess.call(cmd)
            if rc != 0:
                print("step %s ended with status %d: stopping, nothing written" % (step, rc), flush=True)
                return rc
            with open(os.path.join(scratch, step + ".json")) as f:
                record[step] = json.load(f)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    d, r = record["device"], record["ref"]
    print("scan: %.3f ms device (carrier %.3f, bank %.3f, scan %.3f), %.3f ms wall, %.2f M pairs/s (device), "
          "%.3f us/pair | k_correlate %.3f us per (block, template), k_carrier %.3f us per block | ratio %.2f | "
          "NumPy %.2f ms/pair" % (d["device_ms"]["sum"], d["device_ms"]["carrier_stage"], d["device_ms"]["bank_kernel"],
                                  d["device_ms"]["scan_kernels"], d["call_wall_ms"]["median"],
                                  d["pairs_per_s_device"] / 1e6, d["us_per_pair_scan_kernels"],
                                  d["yardstick"]["us_per_block_template_k_correlate"],
                                  d["yardstick"]["us_per_block_k_carrier"], d["pair_over_yardstick"], r["ms_per_pair"]))
    print(json.dumps(r["device_against_ref"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
