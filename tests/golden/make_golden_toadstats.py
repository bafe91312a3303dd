#!/usr/bin/env python3
"""Golden fixtures for the detection statistics, made by RUNNING THE REFERENCE's thrifty/toads_data.py
(`toads_array`) and thrifty/toads_analysis.py (`split_rxtx`, `print_stats`; `print_rxtx_stats` itself does
not run under Python 3 -- `iteritems` -- so the splits are walked here), NumPy's `np.polyfit(soa, timestamp, 1)`
and the arithmetic of scripts/tdoa_matrix.py's count and mean-peak tables.  Build container only (needs the
reference checkout and matplotlib):

    cd /tmp && MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_toadstats.py

Each file under tests/golden/toadstats/ holds the eleven input columns, per cell the reference's text and the
arrays behind it, the three histograms, the reference's line per receiver, the two tables, and the exact
values (tests/toadstats_ref.py: rational arithmetic).  `realistic` also holds a match list and everything
again for the matched detections (prefix m_).  A scene is drawn again from the next seed until
 - the reference's own means and stds, and np.polyfit's residuals, are inside the bounds the device is held
   to (polyfit_distance keeps the residuals' distance from the exact ones), and
 - every number the reference printed is at least 1e-7 away from a rounding tie of its format.
"""
import contextlib
import io
import os
import sys

import numpy as np

REF = os.environ.get("THRIFTY_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))

from thrifty import toads_analysis, toads_data  # noqa: E402

import toadstats_ref as R  # noqa: E402

T0 = 1.7e9


def realistic(rng):
    """3 receivers x 4 transmitters (-1 .. 2), one hour, receiver clocks some tens of ppm apart."""
    ppm = rng.uniform(-40e-6, 40e-6, 3)
    start = rng.uniform(0, 5, 3)
    rows = []
    for tx in range(-1, 3):
        t = float(rng.uniform(0, 20))
        while t < 3600:
            for rx in range(3):
                if rng.random() < 0.18:
                    continue
                ts = round(T0 + t + float(rng.normal(0, 2e-3)), 6)
                soa = round((t + start[rx]) * 2.4e6 * (1 + ppm[rx]) + float(rng.normal(0, 0.4)), 8)
                en = float(np.float32(rng.uniform(300, 900) * (1 + 0.2 * rx)))
                rows.append((rx, tx, ts, soa, 40 + 3 * tx + int(rng.integers(-1, 2)), float(rng.uniform(-0.5, 0.5)),
                             float(np.float32(rng.uniform(80, 160))), float(np.float32(rng.uniform(4, 9))), en,
                             float(np.float32(rng.uniform(10, 20))), float(rng.uniform(-0.5, 0.5))))
            t += float(rng.uniform(45, 70))
    return rows


def ties(rng):
    """Offsets on a 0.05 grid (many on histogram edges), timestamps on whole minutes, constant columns."""
    rows = []
    for i in range(240):
        minute = int(rng.integers(0, 12))
        rows.append((int(rng.integers(0, 2)), int(rng.integers(-1, 2)), T0 + 60.0 * minute, 1.44e8 * minute + 7.0 * i,
                     55, 0.25, 128.0, 4.0, float(rng.integers(1, 4)) * 100.0, 12.5, 0.05 * int(rng.integers(-10, 11))))
    return rows


def sparse(rng):
    """Cells of one and two rows; receiver 7 has a single row."""
    rows = []
    for i, (rx, tx) in enumerate([(0, 0), (0, 1), (0, 1), (3, -1), (3, 2), (3, 2), (7, 5), (0, 4), (3, 0)]):
        t = 37.0 * i + float(rng.uniform(0, 30))
        rows.append((rx, tx, round(T0 + t, 6), round(t * 2.4e6 * (1 + 1e-5 * rx), 8), 30 + 2 * i, float(rng.uniform(-0.5, 0.5)),
                     float(rng.uniform(80, 160)), float(rng.uniform(4, 9)), float(rng.uniform(300, 900)),
                     float(rng.uniform(10, 20)), float(rng.uniform(-0.5, 0.5))))
    return rows


def as_objects(rows):
    out = []
    for i, (rx, tx, ts, soa, cbin, coff, cen, cno, en, no, off) in enumerate(rows):
        det = toads_data.DetectionResult(ts, i, soa, toads_data.CarrierSyncInfo(cbin, coff, cen, cno),
                                         toads_data.CorrDetectionInfo(int(soa) % 12288, off, en, no), rx)
        det.txid = tx
        out.append(det)
    return out


def printed_numbers_safe(stats_rows, formats):
    for value, digits in zip(stats_rows, formats):
        if not np.isfinite(value):
            continue
        scaled = abs(value) * 10.0 ** digits
        if abs((scaled % 1.0) - 0.5) < 1e-7 * 10.0 ** digits:
            return False
    return True


DIGITS = ((1, 2, 1, 1), (1, 2, 1, 1), (1, 2, 1, 1), (0, 3, 0, 0), (3, 3, 3, 3), (1, 2, 1, 1), (1, 2, 1, 1), (1, 2, 1, 1),
          (3, 3, 3, 3))


def record(prefix, detections, out):
    """Run the reference on `detections` (a toads_array, already a copy) -> fills out[prefix + ...]; False when
    one of the two conditions on a fixture fails."""
    cols = {name: np.array(detections[name]) for name, _ in R.COLUMNS}
    time0 = np.min(detections["timestamp"])
    detections["timestamp"] -= time0
    splits = toads_analysis.split_rxtx(detections)
    texts, cells, np_stats, minute, bins, first, edges, hists = [], [], [], [], [], [], [], []
    for rx, per_tx in splits.items():
        for tx, data in per_tx.items():
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                toads_analysis.print_stats(data)
            texts.append(buf.getvalue())
            cells.append((rx, tx, len(data)))
            q = R.quantities({k: data[k] for k, _ in R.COLUMNS}, slice(None))
            np_stats.append([(np.mean(x), np.std(x), np.min(x), np.max(x)) for x in q])
            by_minute = np.bincount(np.floor_divide(data["timestamp"], 60).astype("int64"))
            if not np.array_equal(by_minute, np.bincount(np.floor(data["timestamp"] / 60.0).astype(np.int64))):
                return False
            minute.append(by_minute)
            first.append(np.amin(data["carrier_bin"]))
            bins.append(np.bincount(data["carrier_bin"] - first[-1]))
            h, e = np.histogram(data["offset"], 10)
            hists.append(h)
            edges.append(e)
    np_stats = np.array(np_stats)
    for c in range(len(cells)):
        for k in range(R.N_Q):
            if not printed_numbers_safe(np_stats[c, k], DIGITS[k]):
                return False
    exact = R.exact_values(cols)
    cell_ptr = np.r_[0, np.cumsum([c[2] for c in cells])]
    try:
        R.assert_stats_within_bounds(np_stats, exact["cells"], cell_ptr, "reference")
    except AssertionError:
        return False
    rx_ids = np.unique(detections["rxid"])
    poly, poly_res, distance = [], np.zeros(len(detections)), []
    for r, rx in enumerate(rx_ids):
        j = np.flatnonzero(detections["rxid"] == rx)
        data = detections[j]
        if len(np.unique(data["soa"])) < 2:
            poly.append((np.nan, np.nan))
            poly_res[j] = np.nan
            distance.append(np.nan)
            continue
        coeffs = np.polyfit(data["soa"], data["timestamp"], 1)
        poly.append(tuple(coeffs))
        poly_res[j] = np.poly1d(coeffs)(data["soa"]) - data["timestamp"]
        distance.append(np.max(np.abs(poly_res[j] - exact["residual"][j])))
        if distance[-1] > (len(j) + 8) * R.U * np.max(np.abs(data["timestamp"])):
            return False
    txids = np.sort(np.unique(detections["txid"]))
    counts = np.zeros((len(txids), len(rx_ids)), dtype=np.int64)
    peaks = [[[] for _ in rx_ids] for _ in txids]
    for row in detections:
        t, r = int(np.searchsorted(txids, row["txid"])), int(np.searchsorted(rx_ids, row["rxid"]))
        counts[t, r] += 1
        peaks[t][r].append(row["energy"])
    means = np.array([[int(np.mean(p)) if len(p) > 0 else 0 for p in per_tx] for per_tx in peaks], dtype=np.int64)
    out.update({prefix + k: v for k, v in {
        "time0": np.float64(time0), "text": np.array(texts), "cell_rx": np.array([c[0] for c in cells], np.int32),
        "cell_tx": np.array([c[1] for c in cells], np.int32), "cell_ptr": cell_ptr.astype(np.int64), "np_stats": np_stats,
        "minute_ptr": np.r_[0, np.cumsum([len(h) for h in minute])].astype(np.int64),
        "minute_hist": np.concatenate(minute).astype(np.int64), "bin_first": np.array(first, np.int32),
        "bin_ptr": np.r_[0, np.cumsum([len(h) for h in bins])].astype(np.int64),
        "bin_hist": np.concatenate(bins).astype(np.int64), "offset_hist": np.array(hists, np.int64),
        "offset_edges": np.array(edges), "rx_id": rx_ids.astype(np.int32), "polyfit": np.array(poly),
        "polyfit_residual": poly_res, "polyfit_distance": np.array(distance), "table_txids": txids.astype(np.int32),
        "count_table": counts, "mean_energy_table": means, "exact_cells": exact["cells"], "exact_rx_fit": exact["rx_fit"],
        "exact_residual": exact["residual"]}.items()})
    return True


def save(name, scene, seed, with_matches=False):
    for attempt in range(50):
        rng = np.random.default_rng(seed + attempt)
        rows = sorted(scene(rng), key=lambda r: r[2])
        detections = toads_data.toads_array(as_objects(rows), with_ids=True)
        out = {k: np.array(detections[k]) for k, _ in R.COLUMNS}
        out["seed"] = np.int64(seed + attempt)
        if not record("", detections.copy(), out):
            continue
        if with_matches:        # disjoint groups of two or three detections, in no particular order
            pool = rng.permutation(len(rows))[:2 * len(rows) // 3].tolist()
            matches = []
            while len(pool) >= 3:
                k = 2 + int(rng.integers(0, 2))
                matches.append([pool.pop() for _ in range(k)])
            out["match_ptr"] = np.r_[0, np.cumsum([len(m) for m in matches])].astype(np.int64)
            out["match_idx"] = np.concatenate(matches).astype(np.int64)
            matched = np.sort(np.concatenate(matches))
            if not record("m_", detections[matched].copy(), out):
                continue
        np.savez_compressed(os.path.join(HERE, "toadstats", name + ".npz"), **out)
        print("%-10s seed %d: %d rows, %d cells, %d receivers, polyfit off the exact residuals by %s"
              % (name, seed + attempt, len(rows), len(out["cell_rx"]), len(out["rx_id"]), out["polyfit_distance"]))
        return
    raise SystemExit("no seed gives a usable %s scene" % name)


def main():
    os.makedirs(os.path.join(HERE, "toadstats"), exist_ok=True)
    save("realistic", realistic, 20261019, with_matches=True)
    save("ties", ties, 20261119)
    save("sparse", sparse, 20261219)


if __name__ == "__main__":
    main()
