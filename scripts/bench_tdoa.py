"""Measurement: `thr_tdoa` on synthetic columns -- 4 receivers, 2 beacons and 6 mobiles that each send
about once a second and are heard by every receiver, receiver clocks hours apart and some ppm off,
window 8 s (about 32 beacon pairs in every window), --matches matches (default 1e6: six detection
pairs per match, three quarters of the matches mobile).  One warm-up call, then --repeats calls: median
and range of the wall time and of its split into copies in / kernels / copies out (HIP events,
`thr_debug_tdoa_times`), and the rate in mobile detection pairs per second.  Beside it the sequential
statement tests/tdoa_ref.py on the first --ref-matches matches of the same columns on one host core
(its rows are compared with the device's while at it).  Writes one JSON record (default
profiles/r10_tdoa.json); no figure is asserted anywhere.

--model M [M ...] chooses the clock model(s) (default poly).  With --postdetect-scene N the columns are
instead the TDOA stage's input on scripts/bench_postdetect.py's scene of N raw detections (identify and
match run first, untimed), every model is measured on them in turn in the same process, and the record
(default profiles/r19_tdoa_models.json) holds the kernel milliseconds per model, the polynomial's as the
yardstick beside the others."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from tdoa_ref import tdoa_ref  # noqa: E402
from thrifty_amd import _native, build, tdoa_est  # noqa: E402

N_RX, N_BEACON, N_MOBILE, WINDOW, FS, DEG = 4, 2, 6, 8.0, 2.4e6, 2


def scene(n_matches, seed=10):
    """Columns in timestamp order and the matches (every transmission, every receiver) as CSR."""
    rng = np.random.default_rng(seed)
    n_tx = N_BEACON + N_MOBILE
    rx_xy, tx_xy = rng.uniform(-1500, 1500, (N_RX, 2)), rng.uniform(-1200, 1200, (n_tx, 2))
    tx = np.arange(n_matches) % n_tx
    t = np.arange(n_matches) // n_tx + tx / n_tx + rng.uniform(0, 0.02, n_matches)
    delay = np.linalg.norm(rx_xy[None, :, :] - tx_xy[tx][:, None, :], axis=2) / tdoa_est.SPEED_OF_LIGHT
    rate = FS * (1 + rng.uniform(-30e-6, 30e-6, N_RX))
    offset = np.round(rng.uniform(1, 4, N_RX) * 3600 * FS)
    soa = offset[None, :] + (t[:, None] + delay) * rate[None, :] + rng.normal(0, 0.05, (n_matches, N_RX))
    soa += 40.0 * (rng.random((n_matches, N_RX)) < 0.03) * rng.choice([-1.0, 1.0], (n_matches, N_RX))
    stamp = 1.7e9 + t[:, None] + delay + rng.uniform(-0.03, 0.03, N_RX)[None, :]
    order = np.argsort(stamp.ravel(), kind="stable")
    where = np.empty(order.size, dtype=np.int64)
    where[order] = np.arange(order.size)
    cols = {"rxid": np.tile(np.arange(N_RX), n_matches)[order].astype(np.int32),
            "txid": np.repeat(tx, N_RX)[order].astype(np.int32), "timestamp": stamp.ravel()[order],
            "soa": soa.ravel()[order], "energy": rng.uniform(50, 200, order.size), "noise": rng.uniform(1, 3, order.size)}
    idx = np.sort(where.reshape(n_matches, N_RX), axis=1)
    first = np.argsort(idx[:, 0], kind="stable")              # matches by their first detection
    idx = idx[first].ravel()
    ptr = np.arange(n_matches + 1, dtype=np.int64) * N_RX
    return (cols, ptr, idx, {b: tx_xy[b] for b in range(N_BEACON)}, {r: rx_xy[r] for r in range(N_RX)})


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def tdoa_hip_hash():
    with open(os.path.join(build.CSRC, "tdoa.hip"), "rb") as f:       # (csrc_hash() leaves tdoa.hip out: UNPROFILED_TDOA)
        return hashlib.sha256(f.read()).hexdigest()[:16]


def measure_models(args):
    """Every model of --model on the TDOA stage's input of the post-detect scene -> the record."""
    import bench_postdetect
    from thrifty_amd import identify, matchmaker
    raw, st = bench_postdetect.scene(args.postdetect_scene)
    txid, _, order = identify.integrate_columns(raw, st.tx_freqs)
    cols = {name: raw[name][order] for name in ("rxid", "timestamp", "soa", "energy", "noise")}
    cols["txid"] = txid[order]
    ptr, idx, _, _ = matchmaker.match_columns(cols, st.match_window)
    rec = {"csrc_hash": build.csrc_hash(), "tdoa_hip_sha256": tdoa_hip_hash(), "scene": "scripts/bench_postdetect.py",
           "raw_detections": args.postdetect_scene, "detections": len(order), "matches": len(ptr) - 1,
           "window_s": st.tdoa_est_window, "deg": DEG, "repeats": args.repeats, "models": {}}
    for model in args.model:
        run = lambda: tdoa_est.tdoa_columns(cols, ptr, idx, st.tdoa_est_window, st.beacon_pos, st.rx_pos,   # noqa: E731
                                            st.sample_rate, DEG, model=model)
        out = run()                                              # warm-up
        wall, parts = [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            out = run()
            wall.append(time.perf_counter() - t0)
            parts.append(_native.tdoa_times())
        rec["pairs"] = len(out["n_window"])
        rec["window_pairs"] = {"median": float(np.median(out["n_window"])), "max": int(out["n_window"].max())}
        rec["models"][model] = {"tdoas": len(out["tdoas"]), "failures": len(out["failures"]),
                                "kernels_ms": spread([p[1] for p in parts]), "wall_ms": spread([1e3 * w for w in wall])}
    if "poly" in rec["models"]:
        yardstick = rec["models"]["poly"]["kernels_ms"]["median"]
        for model in rec["models"]:
            rec["models"][model]["kernels_over_poly"] = rec["models"][model]["kernels_ms"]["median"] / yardstick
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matches", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ref-matches", type=int, default=4000, help="matches tests/tdoa_ref.py is run on")
    ap.add_argument("--model", nargs="+", choices=sorted(tdoa_est.MODELS), default=["poly"])
    ap.add_argument("--postdetect-scene", type=int, default=None, metavar="N",
                    help="measure on the TDOA input of scripts/bench_postdetect.py's scene of N raw detections")
    ap.add_argument("-o", "--output", default=None)
    args = ap.parse_args()
    if args.postdetect_scene:
        rec = measure_models(args)
        args.output = args.output or os.path.join(ROOT, "profiles", "r19_tdoa_models.json")
        print(json.dumps(rec), flush=True)
        with open(args.output, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        return
    if len(args.model) != 1:
        ap.error("several models are measured with --postdetect-scene only")
    model = args.model[0]
    args.output = args.output or os.path.join(ROOT, "profiles", "r10_tdoa.json")
    cols, ptr, idx, beacon_pos, rx_pos = scene(args.matches)
    run = lambda: tdoa_est.tdoa_columns(cols, ptr, idx, WINDOW, beacon_pos, rx_pos, FS, DEG, model=model)   # noqa: E731
    out = run()                                                  # warm-up
    wall, parts = [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        out = run()
        wall.append(time.perf_counter() - t0)
        parts.append(_native.tdoa_times())
    pairs = len(out["n_window"])
    kernels = statistics.median([p[1] for p in parts])
    rec = {"csrc_hash": build.csrc_hash(), "tdoa_hip_sha256": tdoa_hip_hash(), "model": model, "receivers": N_RX, "beacons": N_BEACON, "mobiles": N_MOBILE,
           "window_s": WINDOW, "deg": DEG, "repeats": args.repeats, "matches": args.matches,
           "detections": len(cols["rxid"]), "pairs": pairs, "tdoas": len(out["tdoas"]), "failures": len(out["failures"]),
           "window_pairs": {"median": float(np.median(out["n_window"])), "max": int(out["n_window"].max())},
           "wall_ms": spread([1e3 * w for w in wall]), "copies_in_ms": spread([p[0] for p in parts]),
           "kernels_ms": spread([p[1] for p in parts]), "copies_out_ms": spread([p[2] for p in parts]),
           "pairs_per_s": pairs / statistics.median(wall), "pairs_per_s_kernels_only": pairs / (1e-3 * kernels)}
    if args.ref_matches and model == "poly":      # (tests/tdoa_ref.py states the polynomial)
        m = min(args.ref_matches, args.matches)
        matches = idx[:m * N_RX].reshape(m, N_RX).tolist()
        t0 = time.perf_counter()
        want = tdoa_ref(cols["rxid"], cols["txid"], cols["timestamp"], cols["soa"], cols["energy"], cols["noise"],
                        matches, WINDOW, beacon_pos, rx_pos, FS, DEG)
        took = time.perf_counter() - t0
        head = tdoa_est.tdoa_columns(cols, ptr[:m + 1], idx[:m * N_RX], WINDOW, beacon_pos, rx_pos, FS, DEG)
        rows = [row for g in want["groups"] for row in g[3]]
        same = (head["n_window"].tolist() == want["n_window"] and head["n_kept"].tolist() == want["n_kept"] and
                [tuple(p) for p in head["failures"].tolist()] == want["failures"] and
                head["tdoas"]["det0_idx"].tolist() == [row[5] for row in rows])
        rec.update({"tdoa_ref_matches": m, "tdoa_ref_pairs": len(want["n_window"]), "tdoa_ref_one_core_s": took,
                    "tdoa_ref_pairs_per_s": len(want["n_window"]) / took, "equals_tdoa_ref": bool(same),
                    "max_abs_tdoa_difference_s": float(np.max(np.abs(head["tdoas"]["tdoa"] - [row[2] for row in rows])))
                    if same and rows else None})
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
