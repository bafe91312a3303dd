#!/usr/bin/env python3
"""Golden fixtures for the clock-sync and TDOA statistics, made by RUNNING THE REFERENCE's
thrifty/beacon_analysis.py (`analyze`, `fit_poly_model`), thrifty/matchmaker.py (`extract_match_matrix`),
thrifty/stat_tools.py (`is_outlier`) and the arithmetic of thrifty/tdoa_analysis.py's three lines (its `_main`
is argparse, a file and a plot; the lines are formatted here from the same NumPy calls).  Build container only
(needs the reference checkout and matplotlib):

    cd /tmp && MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_syncstats.py

tests/golden/syncstats/realistic.npz and slow_rx1.npz hold the six detection columns, the matches as CSR, and
per (beacon, rx0, rx1) cell and degree 1..3 the reference's printed text (or the exception's name where it
raises), its coefficients, fit_poly_model's residuals per fitted cut and their distance from the exact ones
(tests/syncstats_ref.py: rational arithmetic).  tdoa.npz holds a .tdoa matrix, per cell the three lines, NumPy's
numbers and is_outlier's mask.  A scene is drawn again from the next seed until
 - every dsdoa is at least 1e-9 (relative) away from 10 * mean,
 - every printed number is at least 1e-7 away from a rounding tie of its format,
 - the reference's own residuals lie within max(floor, ...) of the exact ones, its means, stds and RMS within
   the bounds the device is held to.
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

if not hasattr(np, "bool"):         # the reference spells the mask's dtype np.bool
    np.bool = bool

from thrifty import beacon_analysis, matchmaker, stat_tools, toads_data  # noqa: E402

import syncstats_ref as R  # noqa: E402

FS = 2.4e6
BLOCK = 8192


def deployment(rng, ppm, n_seconds, jumps):
    """Transmitters 0, 1 (beacons) and 2, 3 (mobiles) heard by len(ppm) receivers; `jumps`: (receiver, time,
    blocks) -- from that time on the receiver's SOAs are `blocks` whole blocks later.
    -> (detection objects in timestamp order, matches as lists of indices)."""
    start = rng.uniform(700, 1200, len(ppm))
    events = []
    for tx in range(4):
        t = float(rng.uniform(0, 1))
        while t < n_seconds:
            events.append((t, tx))
            t += float(rng.uniform(0.9, 1.1)) * (1.0 if tx < 2 else 2.5)
    events.sort()
    dets, matches = [], []
    for t, tx in events:
        group = []
        for rx in range(len(ppm)):
            if rng.random() < 0.12:
                continue
            shift = sum(blocks * BLOCK for r, when, blocks in jumps if r == rx and t >= when)
            soa = round((t + start[rx]) * FS * (1 + ppm[rx]) + shift + float(rng.normal(0, 0.05)), 8)
            det = toads_data.DetectionResult(round(1.7e9 + t + float(rng.normal(0, 1e-3)), 6), len(dets), soa,
                                             toads_data.CarrierSyncInfo(40 + tx, 0.1, 120.0, 6.0),
                                             toads_data.CorrDetectionInfo(int(soa) % BLOCK, 0.2, float(rng.uniform(300, 900)),
                                                                          float(rng.uniform(10, 20))), rx)
            det.txid = tx
            group.append(len(dets))
            dets.append(det)
        if len(group) >= 2:
            matches.append(group)
    return dets, matches


def realistic(rng):
    """rx0 < rx1 < rx2 in clock rate, some tens of ppm apart; rx2 loses whole blocks three times, the third time
    five beacon periods after the second: a cut too short to fit."""
    ppm = np.sort(rng.uniform(-40e-6, 40e-6, 3))
    ppm[1:] += (12e-6, 24e-6)
    return deployment(rng, ppm, 150, [(2, 40.3, 1), (2, 95.2, 2), (2, 100.4, 1)])


def slow_rx1(rng):
    """rx1 slower than rx0: the mean dsdoa is negative, every row is a discontinuity, nothing is fitted."""
    return deployment(rng, np.array([30e-6, -15e-6]), 60, [])


def printed_safe(value, digits):
    if not np.isfinite(value):
        return True
    scaled = abs(value) * 10.0 ** digits
    return abs((scaled % 1.0) - 0.5) >= 1e-7 * 10.0 ** digits


def record_cell(detections, dets, matches, beacon, rx0, rx1, deg, out, tag):
    """Run the reference on one cell; False when the scene has to be drawn again."""
    matrix = np.array(matchmaker.extract_match_matrix(dets, matches, [rx0, rx1], [beacon]))
    if len(matrix) == 0:
        return True
    buf = io.StringIO()
    error, coefs = "", []
    with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
        try:
            coefs = beacon_analysis.analyze(detections, matrix, deg=deg)
        except Exception as err:            # no cut fitted: np.concatenate of nothing
            error = type(err).__name__
    soa = detections["soa"][matrix]
    sdoa = soa[:, 1] - soa[:, 0]
    dsdoa = np.diff(sdoa)
    thresh = np.mean(dsdoa) * 10
    if np.any(np.abs(dsdoa - thresh) <= 1e-9 * abs(thresh)):
        return False
    found = np.where(dsdoa > thresh)[0]
    edges = np.concatenate([[0], found, [len(matrix)]])
    residuals, distance, lefts = [], [], []
    for i in range(len(edges) - 1):
        left, right = edges[i] + 1, edges[i + 1]
        if left + 8 >= right:
            continue
        _, res = beacon_analysis.fit_poly_model(soa[left:right], deg)
        _, _, exact = R.exact_polyfit(soa[left:right, 0], soa[left:right, 1], deg)
        d = float(np.max(np.abs(res - np.array([float(v) for v in exact]))))
        if d > R.residual_floor(soa[left:right, 1]):
            return False
        residuals.append(res)
        distance.append(d)
        lefts.append(left)
    if residuals:
        all_res = np.concatenate(residuals)
        s2m = 3e8 / 2.4e6
        if not (printed_safe(np.std(all_res) * s2m, 1) and printed_safe(np.max(np.abs(all_res)) * s2m, 1)):
            return False
    out.update({tag + "matrix": matrix.astype(np.int64), tag + "text": np.array(buf.getvalue()), tag + "error": np.array(error),
                tag + "coefs": np.array(coefs, np.float64).reshape(len(coefs), deg + 1), tag + "cut_left": np.array(lefts, np.int64),
                tag + "polyfit_residual": np.concatenate(residuals) if residuals else np.zeros(0),
                tag + "polyfit_distance": np.array(distance)})
    return True


def save_beacon(name, scene, seed):
    for attempt in range(50):
        rng = np.random.default_rng(seed + attempt)
        dets, matches = scene(rng)
        detections = toads_data.toads_array(dets, with_ids=True)
        out = {k: np.array(detections[k]).astype(kind) for k, kind in R.BSYNC_COLUMNS}
        out["seed"] = np.int64(seed + attempt)
        out["match_ptr"] = np.r_[0, np.cumsum([len(m) for m in matches])].astype(np.int64)
        out["match_idx"] = np.concatenate(matches).astype(np.int64)
        receivers = sorted(set(int(d.rxid) for d in dets))
        cells = [(b, r0, r1) for b in (0, 1) for i, r0 in enumerate(receivers) for r1 in receivers[i + 1:]]
        ok = all(record_cell(detections, dets, matches, b, r0, r1, deg, out, "b%d_%d_%d_deg%d_" % (b, r0, r1, deg))
                 for b, r0, r1 in cells for deg in (1, 2, 3))
        if not ok:
            continue
        out["cells"] = np.array(cells, np.int32)
        np.savez_compressed(os.path.join(HERE, "syncstats", name + ".npz"), **out)
        worst = max([float(np.max(v)) for k, v in out.items() if k.endswith("polyfit_distance") and len(v)] or [0.0])
        print("%-10s seed %d: %d detections, %d matches, %d cells; np.polyfit off the exact residuals by at most %.3g"
              % (name, seed + attempt, len(dets), len(matches), len(cells), worst))
        return
    raise SystemExit("no seed gives a usable %s scene" % name)


def save_tdoa(seed):
    """A .tdoa matrix: 3 receiver pairs x 3 transmitters, some cells with far outliers, one constant, one single."""
    for attempt in range(50):
        rng = np.random.default_rng(seed + attempt)
        rows = []
        for rx0, rx1 in ((0, 1), (0, 2), (1, 2)):
            for tx in (2, 3, 5):
                n = int(rng.integers(20, 60))
                tdoa = rng.normal(rng.uniform(-200, 200), 3.0, n) / 2.997e8
                if tx == 3:
                    tdoa[rng.integers(0, n, 3)] += rng.choice([-1, 1], 3) * rng.uniform(2e-7, 9e-7, 3)
                for v in tdoa:
                    rows.append((rx0, rx1, tx, round(1.7e9 + float(rng.uniform(0, 300)), 6), float(v)))
        rows += [(0, 1, 7, 1.7e9 + 5.0, 1.251e-7)] * 6 + [(1, 2, 7, 1.7e9 + 9.0, -3.5e-7)]
        rows.sort(key=lambda r: r[3])
        cols = {"rx0": np.array([r[0] for r in rows], np.int32), "rx1": np.array([r[1] for r in rows], np.int32),
                "tx": np.array([r[2] for r in rows], np.int32), "timestamp": np.array([r[3] for r in rows]),
                "det0_idx": np.arange(len(rows), dtype=np.int64) * 2, "det1_idx": np.arange(len(rows), dtype=np.int64) * 2 + 1,
                "tdoa": np.array([r[4] for r in rows])}
        counts, ref = R.tdoa_stats_ref(cols, robust=True)
        texts, masks, numbers, ok = [], np.zeros(len(rows), np.uint8), [], True
        for ci, (rx0, rx1, tx) in enumerate(ref["cell_key"]):
            sel = np.flatnonzero((cols["rx0"] == rx0) & (cols["rx1"] == rx1) & (cols["tx"] == tx))
            meter = cols["tdoa"][sel] * 2.997e8
            mean, std, rms = np.mean(meter), np.std(meter), np.sqrt(np.mean(meter ** 2))
            ok = ok and all(printed_safe(v, 3) for v in (mean, std, rms))
            texts.append("TDOA bias: %.3f m\nTDOA std dev: %.3f m\nTDOA RMS: %.3f m\n" % (mean, std, rms))
            numbers.append((mean, std, rms, np.min(meter), np.max(meter)))
            if len(sel) > 1:
                with np.errstate(all="ignore"):
                    masks[sel] = stat_tools.is_outlier(meter)
        try:        # the reference's own numbers inside the bounds the device is held to
            R.assert_tdoa_within_bounds(cols, dict(ref, stats=np.array(numbers), mask=np.zeros(0, np.uint8)), "reference")
        except AssertionError:
            ok = False
        if not ok:
            continue
        out = dict(cols, seed=np.int64(seed + attempt), cell_key=ref["cell_key"], text=np.array(texts), np_stats=np.array(numbers),
                   is_outlier=masks)
        np.savez_compressed(os.path.join(HERE, "syncstats", "tdoa.npz"), **out)
        print("tdoa       seed %d: %d rows, %d cells, %d outliers" % (seed + attempt, len(rows), counts["cells"], int(masks.sum())))
        return
    raise SystemExit("no seed gives a usable tdoa scene")


def main():
    os.makedirs(os.path.join(HERE, "syncstats"), exist_ok=True)
    save_beacon("realistic", realistic, 20261019)
    save_beacon("slow_rx1", slow_rx1, 20261119)
    save_tdoa(20261219)


if __name__ == "__main__":
    main()
