"""Measurement: the post-detect chain in one call (`kitchen_sink.postdetect_columns`, `thr_postdetect`)
against the staged column calls (`identify.integrate_columns` -> `matchmaker.match_columns` ->
`tdoa_est.tdoa_columns` -> `pos_est.pos_columns`, with the host glue between them) on the same raw
detection columns.  The scene is `scripts/bench_match.py`'s -- 4 receivers, 8 transmitters sending about
once a second each, receiver clock skews of tens of ms, about 5 % second detections by the same receiver
-- with what the later stages need: 2 of the transmitters are beacons, the receivers stand on a ring of
1 km, and every SoA is the receiver's clock (an offset and a rate error of parts in 1e7) at the time of
arrival plus 0.05 samples of noise.  n = 2^16 and 2^20 raw detections.

Per size: one warm-up of each path, then --repeats of each, alternating; the median and range of the wall
times, the fused call's six-way split (copies in, identify, match, tdoa, pos, copies out; HIP events,
`thr_debug_post_times`) and the staged calls' own splits (`thr_debug_match_times`, `_tdoa_times`,
`_pos_times`: copies in, kernels, copies out), and whether the two paths' outputs are bit-identical.
Writes one JSON record (default profiles/r12_postdetect.json).  The one figure compared: at the largest
size the fused median must not exceed the staged median x 1.05 (`fused_within_5_percent`)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from thrifty_amd import _native, build, identify, kitchen_sink, matchmaker, pos_est, tdoa_est  # noqa: E402

N_RX, N_TX, BEACONS, WINDOW, TDOA_WINDOW, FS, C, NEW_LEN = 4, 8, (0, 1), 0.2, 8.0, 2.4e6, 2.997e8, 12288
RX_XY = np.array([(1000.0, 0.0), (0.0, 1000.0), (-1000.0, 0.0), (0.0, -1000.0)])
TX_XY = np.array([(300.0, 400.0), (-200.0, -350.0), (120.0, -80.0), (-420.0, 260.0), (510.0, 330.0), (-50.0, 620.0),
                  (640.0, -210.0), (-330.0, -480.0)])


def scene(n, seed=9):
    """(raw detection columns in per-receiver order, PostdetectSettings)."""
    rng = np.random.default_rng(seed)
    n_events = int(n / (N_RX * 0.9 * 1.05)) + 1
    tx = np.arange(n_events) % N_TX
    t = np.arange(n_events) // N_TX + tx / N_TX + rng.uniform(0, 0.02, n_events)      # seconds since the start
    seen = rng.random((n_events, N_RX)) < 0.9
    ev, rx = np.nonzero(seen)
    doubled = rng.random(len(ev)) < 0.05
    ev, rx = np.concatenate([ev, ev[doubled]]), np.concatenate([rx, rx[doubled]])
    again = np.concatenate([np.zeros(len(doubled)), np.ones(int(doubled.sum()))])      # a second detection, 3 blocks on
    skew, ppm, offset = rng.uniform(-0.03, 0.03, N_RX), rng.uniform(-3e-7, 3e-7, N_RX), rng.uniform(3e9, 1.1e10, N_RX)
    arrival = t[ev] + np.sqrt(((RX_XY[rx] - TX_XY[tx[ev]]) ** 2).sum(axis=1)) / C
    soa = offset[rx] + FS * (1 + ppm[rx]) * arrival + rng.normal(0, 0.05, len(ev)) + again * 3 * NEW_LEN
    stamp = np.round(1.7e9 + t[ev] + skew[rx] + rng.normal(0, 1e-3, len(ev)) + again * rng.uniform(1e-3, 8e-3, len(ev)), 6)
    first = np.argsort(stamp, kind="stable")[:n]                                       # the first n of the scene ...
    order = first[np.lexsort((stamp[first], rx[first]))]                               # ... receiver after receiver
    cols = {"rxid": rx[order].astype(np.int32), "block": (soa[order] // NEW_LEN).astype(np.int32), "timestamp": stamp[order],
            "carrier_bin": (40 + 10 * tx[ev[order]] + 2 * rx[order] + rng.integers(-1, 2, len(order))).astype(np.int32),
            "carrier_offset": rng.uniform(-0.5, 0.5, len(order)), "soa": soa[order],
            "energy": rng.uniform(50, 200, len(order)), "noise": rng.uniform(1, 3, len(order))}
    freqmap = {r: {x: (37.0 + 10 * x + 2 * r, 43.0 + 10 * x + 2 * r) for x in range(N_TX)} for r in range(N_RX)}
    settings = kitchen_sink.PostdetectSettings(tx_freqs=freqmap, match_window=WINDOW, tdoa_est_window=TDOA_WINDOW,
                                               rx_pos={r: RX_XY[r] for r in range(N_RX)},
                                               beacon_pos={b: TX_XY[b] for b in BEACONS}, sample_rate=FS)
    return cols, settings


def staged(cols, st, times=None):
    txid, keep, order = identify.integrate_columns(cols, st.tx_freqs)
    toads = {name: cols[name][order] for name in ("rxid", "timestamp", "soa", "energy", "noise")}
    toads["txid"] = txid[order]
    ptr, idx, misses, collisions = matchmaker.match_columns(toads, st.match_window)
    if times is not None:
        times["match"].append(_native.match_times())
    td = tdoa_est.tdoa_columns(toads, ptr, idx, st.tdoa_est_window, st.beacon_pos, st.rx_pos, st.sample_rate)
    if times is not None:
        times["tdoa"].append(_native.tdoa_times())
    rows = td["tdoas"]
    ps = pos_est.pos_columns(td["group_ptr"], rows["rx0"], rows["rx1"], rows["tdoa"], rows["snr"], st.rx_pos)
    if times is not None:
        times["pos"].append(_native.pos_times())
    out = {"txid": txid, "keep": keep, "kept_order": order, "match_ptr": ptr, "match_idx": idx, "misses": misses,
           "collisions": collisions}
    out.update(td)
    out.update(ps)
    return out


def identical(a, b):
    names = [name for name in a if name != "counts"]
    return bool(set(names) == set(b) and all(
        np.asarray(a[name]).shape == np.asarray(b[name]).shape and
        np.ascontiguousarray(a[name]).tobytes() == np.ascontiguousarray(b[name]).astype(np.asarray(a[name]).dtype).tobytes()
        for name in names))


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def measure(n, repeats):
    cols, st = scene(n)
    n = len(cols["rxid"])
    want, got = staged(cols, st), kitchen_sink.postdetect_columns(cols, st)              # warm-up of both paths
    wall = {"fused": [], "staged": []}
    split, parts = [], {"match": [], "tdoa": [], "pos": []}
    for _ in range(repeats):
        t0 = time.perf_counter()
        want = staged(cols, st, parts)
        wall["staged"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        got = kitchen_sink.postdetect_columns(cols, st)
        wall["fused"].append(time.perf_counter() - t0)
        split.append(_native.post_times())
    rec = {"n": n, "counts": got["counts"], "solved": int((got["status"] == _native.POS_OK).sum()),
           "fused_equals_staged": identical(got, want),
           "fused_wall_ms": spread([1e3 * w for w in wall["fused"]]), "staged_wall_ms": spread([1e3 * w for w in wall["staged"]]),
           "fused_over_staged": statistics.median(wall["fused"]) / statistics.median(wall["staged"]),
           "fused_detections_per_s": n / statistics.median(wall["fused"]),
           "staged_detections_per_s": n / statistics.median(wall["staged"]),
           "fused_split_ms": {name: spread([s[k] for s in split]) for k, name in enumerate(
               ("copies_in", "identify", "match", "tdoa", "pos", "copies_out"))},
           "staged_stage_ms": {stage: {name: spread([p[k] for p in parts[stage]]) for k, name in enumerate(
               ("copies_in", "kernels", "copies_out"))} for stage in parts}}
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1 << 16, 1 << 20])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "r12_postdetect.json"))
    args = ap.parse_args()
    runs = []
    for n in args.sizes:
        runs.append(measure(n, args.repeats))
        print(json.dumps(runs[-1]), flush=True)
    sources = {}
    for name in ("identify.hip", "match.hip", "tdoa.hip", "pos.hip", "postdetect.hip", "post_stages.hpp"):
        import hashlib
        with open(os.path.join(build.CSRC, name), "rb") as f:
            sources[name] = hashlib.sha256(f.read()).hexdigest()[:16]
    rec = {"csrc_hash": build.csrc_hash(), "sources_sha16": sources, "receivers": N_RX, "transmitters": N_TX,
           "beacons": len(BEACONS), "match_window_s": WINDOW, "tdoa_window_s": TDOA_WINDOW, "repeats": args.repeats,
           "runs": runs, "fused_within_5_percent": runs[-1]["fused_over_staged"] <= 1.05}
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return 0 if rec["fused_within_5_percent"] else 1


if __name__ == "__main__":
    sys.exit(main())
