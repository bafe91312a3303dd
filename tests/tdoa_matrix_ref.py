"""Sequential NumPy statement of the per-beacon TDOA matrices (include/thrifty_hip.h:
thr_tdoamatrix) on columns -- test infrastructure.  Per cell (rx0 < rx1, beacon b, transmitter t != b):

1. the extraction: the matches, in match order, whose transmitter (read off the first detection) is b or t and
   that hold a detection of both receivers, each cut down to those two detections;
2. fewer than 3 such matches of b or of t: the cell is TOO_FEW and its tasks are skipped;
3. tests/tdoa_ref.py's `tdoa_ref` (tests/tdoa_models_ref.py's for the other models) on the extraction with b as
   the only beacon -- the geometry zero unless positions are given;
4. `syncstats_ref.is_outlier` over the TDOAs in seconds, and the five statistics of tdoa * 2.997e8 over the rows
   it keeps.
"""
import numpy as np

import syncstats_ref
import tdoa_models_ref
import tdoa_ref

LIGHT = 2.997e8
CELL_TOO_FEW = 1
OK, NO_MODEL, OUT_OF_RANGE, SKIPPED = 0, 1, 2, 3
MIN_ROWS = 3


def dist_table(receivers, beacons, rx_pos, beacon_pos):
    """float64[receivers][beacons]: the distances as thrifty_amd.tdoa_est computes them."""
    def distance(a, b):
        return np.sqrt(np.sum((np.asarray(a, float) - np.asarray(b, float)) ** 2))
    return np.array([[distance(rx_pos[r], beacon_pos[b]) for b in beacons] for r in receivers], float).reshape(
        len(receivers), len(beacons))


def five(v):
    if len(v) == 0:
        return (np.nan,) * 5
    mean = np.sum(v) / np.float64(len(v))
    return mean, np.sqrt(np.sum((v - mean) * (v - mean)) / len(v)), np.sqrt(np.sum(v * v) / len(v)), np.min(v), np.max(v)


def tdoa_matrix_ref(cols, match_ptr, match_idx, beacons, receivers=None, targets=None, window=4.0, sample_rate=2.4e6,
                    model="poly", deg=2, rx_pos=None, beacon_pos=None):
    """-> (counts, outputs) with the names and dtypes of _native.TDMAT_OUTPUTS, and per task `cond` and `spread` (of the
    fit, NaN where nothing was fitted: tests/tdoa_ref.py) for tolerances."""
    rxid, txid = np.asarray(cols["rxid"]).astype(int), np.asarray(cols["txid"]).astype(int)
    ts = np.asarray(cols["timestamp"], float)
    ptr, idx = np.asarray(match_ptr, np.int64).tolist(), np.asarray(match_idx, np.int64).tolist()
    matches = [idx[a:b] for a, b in zip(ptr[:-1], ptr[1:])]
    for m, match in enumerate(matches):
        if len(set(rxid[match].tolist())) != len(match):
            raise ValueError("match %d holds two detections of one receiver" % m)
    beacons = sorted(int(b) for b in beacons)
    match_tx = [int(txid[m[0]]) if m else None for m in matches]
    if targets is None or len(targets) == 0:
        targets = sorted(set(t for t in match_tx if t is not None))
    else:
        targets = sorted(int(t) for t in targets)
    if receivers is None:
        receivers = sorted(set(int(rxid[d]) for m in matches for d in m))
    else:
        receivers = sorted(int(r) for r in receivers)
    min_kept = {"poly": deg + 1, "weighted_poly": deg + 1, "nearest": 1, "linear": 2}[model]
    out = {k: [] for k in ("cell_key", "cell_flags", "cell_counts", "cell_stats", "medians", "task_det", "task_match",
                           "timestamp", "tdoa", "status", "snr", "model_quality", "n_window", "n_kept", "outlier", "cond", "spread")}
    cell_ptr = [0]
    quality = (np.asarray(cols["energy"], float) / np.asarray(cols["noise"], float)) ** 2
    for i0, rx0 in enumerate(receivers):
        for rx1 in receivers[i0 + 1:]:
            rows = {}       # tx -> [(match, det0, det1)]
            for m, match in enumerate(matches):
                at = {int(rxid[d]): d for d in match}
                if rx0 in at and rx1 in at and (match_tx[m] in beacons or match_tx[m] in targets):
                    rows.setdefault(match_tx[m], []).append((m, at[rx0], at[rx1]))
            for b in beacons:
                for t in targets:
                    if t == b or not rows.get(t):
                        continue
                    mine, theirs = rows[t], rows.get(b, [])
                    n = len(mine)
                    flag = CELL_TOO_FEW if len(theirs) < MIN_ROWS or n < MIN_ROWS else 0
                    status = np.full(n, SKIPPED, np.int32)
                    tdoa, mq, cond, spread = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
                    n_window, n_kept = np.zeros(n, np.int32), np.zeros(n, np.int32)
                    if not flag:
                        extract = sorted(mine + theirs)
                        pos_r = {rx0: 0.0, rx1: 0.0} if rx_pos is None else {rx0: rx_pos[rx0], rx1: rx_pos[rx1]}
                        pos_b = {b: 0.0} if beacon_pos is None else {b: beacon_pos[b]}
                        args = (rxid, txid, ts, cols["soa"], cols["energy"], cols["noise"], [[d0, d1] for _, d0, d1 in extract],
                                window, pos_b, pos_r, sample_rate)
                        res = (tdoa_ref.tdoa_ref(*args, deg=deg) if model == "poly" else
                               tdoa_models_ref.tdoa_models_ref(*args, model=model, deg=deg))
                        got = {(row[5], row[6]): row for group in res["groups"] for row in group[3]}
                        assert len(res["n_window"]) == n
                        for k, (_, d0, d1) in enumerate(mine):
                            n_window[k], n_kept[k] = res["n_window"][k], res["n_kept"][k]
                            cond[k], spread[k] = res["cond"][k], res["spread"][k]
                            if (d0, d1) in got:
                                status[k], tdoa[k], mq[k] = OK, got[(d0, d1)][2], got[(d0, d1)][4]
                            elif n_kept[k] < min_kept:
                                status[k] = NO_MODEL
                            elif model in ("poly", "weighted_poly"):
                                status[k] = OUT_OF_RANGE if not np.isnan(res["cond"][k]) else NO_MODEL
                            elif model == "linear":
                                status[k] = NO_MODEL if res["picks"][k][0] < 0 else OUT_OF_RANGE
                            else:
                                status[k] = OUT_OF_RANGE
                    ok = status == OK
                    mask = np.zeros(n, np.uint8)
                    median, mad = np.nan, np.nan
                    if ok.any():
                        bad, median, mad = syncstats_ref.is_outlier(tdoa[ok])
                        if ok.sum() > 1:
                            mask[ok] = bad
                    kept = ok & (mask == 0)
                    with np.errstate(all="ignore"):
                        stats = five(tdoa[kept] * LIGHT)
                    out["cell_key"].append((rx0, rx1, b, t))
                    out["cell_flags"].append(flag)
                    out["cell_counts"].append((len(theirs), n, int(ok.sum()), 0 if flag else int(n - ok.sum()), int(kept.sum())))
                    out["cell_stats"].append(stats)
                    out["medians"].append((median, mad))
                    out["task_det"] += [(d0, d1) for _, d0, d1 in mine]
                    out["task_match"] += [m for m, _, _ in mine]
                    out["timestamp"] += [ts[d0] for _, d0, _ in mine]
                    out["snr"] += [(quality[d0] + quality[d1]) / 2 for _, d0, d1 in mine]
                    for name, value in (("tdoa", tdoa), ("status", status), ("model_quality", mq), ("n_window", n_window),
                                        ("n_kept", n_kept), ("outlier", mask), ("cond", cond), ("spread", spread)):
                        out[name] += value.tolist()
                    cell_ptr.append(cell_ptr[-1] + n)
    nc, nt = len(out["cell_key"]), cell_ptr[-1]
    shapes = {"cell_key": (np.int32, (nc, 4)), "cell_flags": (np.int32, (nc,)), "cell_counts": (np.int64, (nc, 5)),
              "cell_stats": (np.float64, (nc, 5)), "medians": (np.float64, (nc, 2)), "task_det": (np.int64, (nt, 2)),
              "task_match": (np.int64, (nt,)), "timestamp": (np.float64, (nt,)), "tdoa": (np.float64, (nt,)),
              "status": (np.int32, (nt,)), "snr": (np.float64, (nt,)), "model_quality": (np.float64, (nt,)),
              "n_window": (np.int32, (nt,)), "n_kept": (np.int32, (nt,)), "outlier": (np.uint8, (nt,)),
              "cond": (np.float64, (nt,)), "spread": (np.float64, (nt,))}
    res = {name: np.array(out[name], dtype=kind).reshape(shape) for name, (kind, shape) in shapes.items()}
    res["cell_ptr"] = np.array(cell_ptr, np.int64)
    counts = {"tasks": nt, "cells": nc, "tdoas": int(np.sum(res["status"] == OK))}
    return counts, res
