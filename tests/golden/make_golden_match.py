#!/usr/bin/env python3
"""Golden fixtures for the `match` step, made by RUNNING THE REFERENCE's thrifty/matchmaker.py
functions (`match_toads`, `extract_match_matrix`) on synthetic detection sets.  Build container only
(needs the reference checkout):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_match.py

Under Python 3 `dict.values()` lists a group's entries in the order their receivers first appeared;
that order is what the fixtures record.  Each file holds the input columns (rxid, txid, timestamp,
energy), the cases (window[c], min_match[c]) and per case c the reference's matches as CSR
(c<c>_match_ptr, c<c>_match_idx; files under tests/golden/match/), misses, collisions [k, 2], and the match matrix over `matrix_rxids`
without (c<c>_matrix) and with (c<c>_matrix_tx) the filter `matrix_txids`.
"""
import os
import sys

import numpy as np

REF = os.environ.get("THRIFTY_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

from thrifty import matchmaker, toads_data  # noqa: E402


def transmissions(rng, n_rx, n_tx, n_events, miss_prob, double_prob):
    """Every transmitter sends n_events times, about once a second; every receiver has a clock skew of
    some tens of ms, misses some transmissions and reports some twice (a weaker echo a few ms later)."""
    skew = rng.uniform(-0.03, 0.03, n_rx)
    rows = []
    for tx in range(n_tx):
        t = 1.7e9 + float(rng.uniform(0, 1))
        for _ in range(n_events):
            t += float(rng.uniform(0.7, 1.3))
            for rx in range(n_rx):
                if rng.random() < miss_prob:
                    continue
                ts = round(t + float(skew[rx]) + float(rng.normal(0, 1e-3)), 6)     # what a .toads line keeps
                en = float(rng.uniform(50, 200))
                rows.append((rx, tx, ts, en))
                if rng.random() < double_prob:
                    rows.append((rx, tx, round(ts + float(rng.uniform(1e-3, 8e-3)), 6),
                                 en * float(rng.uniform(0.3, 1.4))))
    return rows


def ties(rng, n):
    """Timestamps on a 0.25 grid, energies from {1, 2, 3}, txid -1 included: many detections land
    exactly on `timestamp + window`, many energies tie."""
    return [(int(rng.integers(0, 4)), int(rng.integers(-1, 3)), 0.25 * int(rng.integers(0, n // 6)),
             float(rng.integers(1, 4))) for _ in range(n)]


def as_objects(rows):
    out = []
    for i, (rx, tx, ts, en) in enumerate(rows):
        car = toads_data.CarrierSyncInfo(40 + tx, 0.1, 150.0, 7.5)
        cor = toads_data.CorrDetectionInfo(4000 + i % 97, 0.01 * (i % 7), en, 1.5)
        det = toads_data.DetectionResult(ts, i, 12288.0 * i, car, cor, rx)
        det.txid = tx
        out.append(det)
    return out


def save(name, rows, cases, matrix_rxids, matrix_txids):
    rows = sorted(rows, key=lambda r: r[2])         # stable, by timestamp
    dets = as_objects(rows)
    out = {"rxid": np.array([r[0] for r in rows], np.int64), "txid": np.array([r[1] for r in rows], np.int64),
           "timestamp": np.array([r[2] for r in rows], float), "energy": np.array([r[3] for r in rows], float),
           "window": np.array([c[0] for c in cases], float), "min_match": np.array([c[1] for c in cases], np.int64),
           "matrix_rxids": np.array(matrix_rxids, np.int64), "matrix_txids": np.array(matrix_txids, np.int64)}
    for c, (window, min_match) in enumerate(cases):
        matches, misses, collisions = matchmaker.match_toads(dets, window, min_match)
        matches = [list(m) for m in matches]
        out["c%d_match_ptr" % c] = np.cumsum([0] + [len(m) for m in matches]).astype(np.int64)
        out["c%d_match_idx" % c] = np.array([i for m in matches for i in m], np.int64)
        out["c%d_misses" % c] = np.array(misses, np.int64)
        out["c%d_collisions" % c] = np.array(collisions, np.int64).reshape(-1, 2)
        for key, txids in (("matrix", None), ("matrix_tx", list(matrix_txids))):
            rows_ = matchmaker.extract_match_matrix(dets, matches, list(matrix_rxids), txids)
            out["c%d_%s" % (c, key)] = np.array(rows_, np.int64).reshape(-1, len(matrix_rxids))
        print("%-16s n=%d window=%g min_match=%d: %d matches, %d misses, %d collisions, matrix %d / %d rows"
              % (name, len(rows), window, min_match, len(matches), len(misses), len(collisions),
                 len(out["c%d_matrix" % c]), len(out["c%d_matrix_tx" % c])))
    np.savez_compressed(os.path.join(HERE, "match", name + ".npz"), **out)


def main():
    rng = np.random.default_rng(20261018)
    save("match_realistic", transmissions(rng, 3, 4, 58, 0.12, 0.08), [(0.2, 2)], [0, 1, 2], [1, 3])
    save("match_ties", ties(rng, 400), [(0.0, 2), (0.25, 2), (0.5, 2), (1.0, 2)], [0, 1], [-1, 0])
    save("match_minmatch", transmissions(rng, 3, 4, 30, 0.3, 0.1), [(0.2, 1), (0.2, 3)], [0, 2], [0, 1, 2])


if __name__ == "__main__":
    main()
