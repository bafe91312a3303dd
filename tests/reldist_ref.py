"""The NumPy statement of thr_reldist (include/thrifty_hip.h gives the formulas; csrc/reldist.hip the device side):
every output of the call, cell by cell, in float64, operation for operation.  Nothing here imports the reference.

The smoother is a plain loop per point.  It has a second evaluation in np.longdouble (`dtype=`): the window of a
point is chosen in float64 either way, the weights and the five sums are then taken in the wider type.  The
device sums the same terms in another order (64 lane-strided partial sums, a butterfly), so its value differs
from the float64 loop by rounding alone; how much rounding matters on the test inputs is what the wider
evaluation measures.

SMOOTH_RTOL, measured, not chosen: `python tests/reldist_ref.py` evaluates the statement in float64 and in
np.longdouble on every input of tests/test_gpu_reldist.py and tests/test_gpu_reldist_seams.py (the scenes of
tests/reldist_scenes.py) and prints the largest |float64 - longdouble| of a smoothed value relative to its
series' scale (the largest |y| of the series).  It printed

    largest relative gap 4.4e-15 (scene smooth_frac_1, dop, cell 11); 16 x = 7.05e-14

on the build machine (x86-64, 80-bit long double).  The tolerance is 16 x that gap: the device's summation tree
differs from the loop's in both directions.  Every input keeps the gap itself below 1e-9 (asserted in
tests/test_reldist_host.py): well-conditioned abscissae, no catastrophic cancellation."""
import numpy as np

import syncstats_ref as S

U = S.U
LIGHT = 2.997e8
ROW_HELD, CELL_UNSORTED, CELL_NO_BEACON = 1, 1, 2
SINGULAR = 1e-12
SMOOTH_GAP = 4.4e-15           # the measured gap (see above)
SMOOTH_RTOL = 16 * SMOOTH_GAP
RELDIST_COLUMNS = (("rxid", np.int32), ("txid", np.int32), ("soa", np.float64), ("timestamp", np.float64),
                   ("carrier_bin", np.float64), ("carrier_offset", np.float64), ("idx", np.int64))
FLOATS = ("raw", "x", "speed_x", "speed", "dop", "dop_smooth_x", "speed_smooth_x", "medians")
DISCRETE = ("cell_key", "cell_ptr", "row_det", "row_match", "nearest_idx", "hi", "row_flags", "mask1", "mask2", "mask3",
            "cell_counts", "cell_flags", "speed_ptr", "speed_smooth_ptr", "dop_smooth_ptr")


def groups_of(c, match_ptr, match_idx, receivers=None):
    """{(txid, rx0, rx1): [(detection at rx0, detection at rx1, match), ...]} in match order, rx0 < rx1."""
    groups = {}
    for i in range(len(match_ptr) - 1):
        dets = [int(d) for d in match_idx[match_ptr[i]:match_ptr[i + 1]]]
        rx = [int(c["rxid"][d]) for d in dets]
        if len(set(rx)) != len(rx):
            raise ValueError("match %d holds two detections of one receiver" % i)
        if not dets:
            continue
        tx = int(c["txid"][dets[0]])
        for a in range(len(dets)):
            for b in range(a + 1, len(dets)):
                if receivers is not None and (rx[a] not in receivers or rx[b] not in receivers):
                    continue
                d0, d1 = (dets[a], dets[b]) if rx[a] < rx[b] else (dets[b], dets[a])
                groups.setdefault((tx, min(rx[a], rx[b]), max(rx[a], rx[b])), []).append((d0, d1, i))
    return groups


def nearest_rows(b0, t0):
    """(hi, nearest): hi = searchsorted(b0, t0, 'left'); the row before it when that one is strictly nearer."""
    hi = np.searchsorted(b0, t0, side="left").astype(np.int64)
    n = hi.copy()
    nb = len(b0)
    for i, h in enumerate(hi):
        if h > 0 and (h == nb or abs(t0[i] - b0[h - 1]) < abs(t0[i] - b0[h])):
            n[i] = h - 1
    return hi, n


def raw_nearest(t0, t1, b0, b1, n):
    return (t1 - b1[n]) - (t0 - b0[n])


def raw_linpol(t0, t1, b0, b1, hi):
    """(raw, held): interpolation between the two beacon rows around t0; the end row is held outside the span."""
    nb = len(b0)
    raw, held = np.zeros(len(t0)), np.zeros(len(t0), bool)
    for i, h in enumerate(hi):
        if h == 0 or h == nb:
            raw[i], held[i] = t1[i] - b1[0 if h == 0 else nb - 1], True
        else:
            w = (t0[i] - b0[h - 1]) / (b0[h] - b0[h - 1])
            raw[i] = t1[i] - (b1[h - 1] * (1.0 - w) + b1[h] * w)
    return raw, held


def window_start(x, i, k):
    """The smallest L for which the k points from L are not farther from x[i] than the k points from L + 1."""
    L, m = 0, len(x)
    while L + k < m and x[L + k] - x[i] < x[i] - x[L]:
        L += 1
    return L


def window_len(m, frac):
    return max(2, min(m, int(frac * m + 1e-10)))


def smooth(x, y, frac, dtype=np.float64):
    """Local linear regression, tricube weights, no robustness iteration (the header's definition)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    m = len(x)
    if m < 2 or frac == 0:
        return y.astype(dtype)
    k = window_len(m, frac)
    X, Y, out = x.astype(dtype), y.astype(dtype), np.zeros(m, dtype)
    one = dtype(1.0)
    with np.errstate(all="ignore"):
        for i in range(m):
            L = window_start(x, i, k)
            d, yy = X[L:L + k] - X[i], Y[L:L + k]
            h = np.max(np.abs(d))
            if h > 0:
                u = np.abs(d) / h
                t = one - (u * u) * u
                w = (t * t) * t
            else:
                w = np.ones(k, dtype)
            wd = w * d
            sw = swd = swy = swdd = swdy = dtype(0.0)
            for j in range(k):
                sw, swd, swy = sw + w[j], swd + wd[j], swy + w[j] * yy[j]
                swdd, swdy = swdd + wd[j] * d[j], swdy + wd[j] * yy[j]
            det = sw * swdd - swd * swd
            out[i] = (swdd * swy - swd * swdy) / det if det > dtype(SINGULAR) * (sw * swdd) else swy / sw
    return out


def reldist_ref(cols, match_ptr, match_idx, beacons, mobiles=None, receivers=None, method="linpol", sample_rate=2.4e6,
                block_len=16384, carrier_hz=433e6, thresh=3.5, smooth_frac=0.025, geometry=None, dtype=np.float64):
    """(counts, {name: array}) with the names of _native.RELDIST_OUTPUTS; ValueError where thr_reldist refuses."""
    if not 0.0 <= smooth_frac <= 1.0:
        raise ValueError("smooth_frac must lie in [0, 1]")
    c = S.columns_of(cols, RELDIST_COLUMNS)
    match_ptr, match_idx = np.asarray(match_ptr, np.int64), np.asarray(match_idx, np.int64)
    beacons = sorted(set(int(b) for b in beacons))
    groups = groups_of(c, match_ptr, match_idx, None if receivers is None else set(int(r) for r in receivers))
    geo = {(int(g[0]), int(g[1]), int(g[2])): tuple(float(v) for v in g[3:]) for g in (geometry or [])}
    keys = sorted((tx, b, r0, r1) for (tx, r0, r1) in groups for b in beacons
                  if b != tx and (tx in set(mobiles) if mobiles is not None else tx not in beacons))
    if not keys:
        raise ValueError("the selection is empty")
    s2m = LIGHT / sample_rate
    f = c["carrier_bin"] + c["carrier_offset"]
    rows = {name: [] for name in ("row_det", "row_match", "nearest_idx", "hi", "row_flags", "raw", "x", "mask1", "dop", "mask3",
                                  "speed_x", "speed", "mask2", "speed_smooth_x", "speed_smooth", "dop_smooth_x", "dop_smooth")}
    nc = len(keys)
    out = {"cell_key": np.array(keys, np.int32).reshape(nc, 4), "cell_stats": np.zeros((nc, 6)),
           "cell_counts": np.zeros((nc, 5), np.int64), "medians": np.zeros((nc, 6)), "cell_flags": np.zeros(nc, np.int32)}
    with np.errstate(all="ignore"):
        for ci, (tx, b, r0, r1) in enumerate(keys):
            mine = np.array(groups[(tx, r0, r1)], np.int64).reshape(-1, 3)
            theirs = np.array(groups.get((b, r0, r1), []), np.int64).reshape(-1, 3)
            n, nb = len(mine), len(theirs)
            t0, t1 = c["soa"][mine[:, 0]], c["soa"][mine[:, 1]]
            ts0, ts1 = c["timestamp"][mine[:, 0]], c["timestamp"][mine[:, 1]]
            b0, b1 = c["soa"][theirs[:, 0]], c["soa"][theirs[:, 1]]
            flags = 0
            if nb == 0:
                flags = CELL_NO_BEACON
            elif np.any(b0[1:] < b0[:-1]) or (smooth_frac > 0 and np.any(ts0[1:] < ts0[:-1])):
                flags = CELL_UNSORTED
            hi, near = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
            raw, dop, held = np.full(n, np.nan), np.full(n, np.nan), np.zeros(n, bool)
            if flags == 0:
                hi, near = nearest_rows(b0, t0)
                if method == "nearest":
                    raw = raw_nearest(t0, t1, b0, b1, near)
                else:
                    raw, held = raw_linpol(t0, t1, b0, b1, hi)
                dop_bin = ((f[mine[:, 0]] - f[mine[:, 1]]) - (f[theirs[near, 0]] - f[theirs[near, 1]])) / 2.0
                dop = dop_bin * (sample_rate / block_len) * 3e8 / carrier_hz * 3.6
            d_beacon, dist_rx, dist_beacon = geo.get((b, r0, r1), (0.0, 0.0, 0.0))
            x = (raw + d_beacon + dist_rx) / 2.0 - dist_beacon
            mask1, med1, mad1 = S.is_outlier(x, thresh)
            kept = x[~mask1]
            count = len(kept)
            mean = np.sum(kept) / np.float64(count) if count else np.nan
            std = np.sqrt(np.sum((kept - mean) * (kept - mean)) / count) if count else np.nan
            within = np.count_nonzero((kept >= mean - std) & (kept <= mean + std))
            out["cell_stats"][ci] = (count, mean * s2m, std * s2m, (np.min(kept) if count else np.inf) * s2m,
                                     (np.max(kept) if count else -np.inf) * s2m, within)
            speed = np.diff(kept) / np.diff(t1[~mask1]) * s2m * sample_rate
            speed_x = (ts1[~mask1] - ts0[0])[1:]
            mask2, med2, mad2 = S.is_outlier(speed, thresh) if len(speed) else (np.zeros(0, bool), np.nan, np.nan)
            mask3, med3, mad3 = S.is_outlier(dop, thresh)
            dop_x = ts0 - ts0[0]
            out["medians"][ci] = (med1, mad1, med2, mad2, med3, mad3)
            out["cell_flags"][ci] = flags
            out["cell_counts"][ci] = (n, nb, count, np.count_nonzero(~mask2), np.count_nonzero(~mask3))
            for name, value in (("row_det", mine[:, :2]), ("row_match", mine[:, 2]), ("nearest_idx", near), ("hi", hi),
                                ("row_flags", held.astype(np.int32) * ROW_HELD), ("raw", raw), ("x", x), ("mask1", mask1),
                                ("dop", dop), ("mask3", mask3), ("speed_x", speed_x), ("speed", speed), ("mask2", mask2),
                                ("speed_smooth_x", speed_x[~mask2]),
                                ("speed_smooth", smooth(speed_x[~mask2], speed[~mask2], smooth_frac, dtype)),
                                ("dop_smooth_x", dop_x[~mask3]), ("dop_smooth", smooth(dop_x[~mask3], dop[~mask3], smooth_frac, dtype))):
                rows[name].append(value)
    kinds = {"row_det": np.int64, "row_match": np.int64, "nearest_idx": np.int32, "hi": np.int32, "row_flags": np.int32,
             "mask1": np.uint8, "mask2": np.uint8, "mask3": np.uint8, "speed_smooth": dtype, "dop_smooth": dtype}
    for name, parts in rows.items():
        out[name] = np.concatenate(parts).astype(kinds.get(name, np.float64))
    for name, of in (("cell_ptr", "raw"), ("speed_ptr", "speed"), ("speed_smooth_ptr", "speed_smooth"), ("dop_smooth_ptr", "dop_smooth")):
        out[name] = np.cumsum([0] + [len(part) for part in rows[of]]).astype(np.int64)
    counts = {"rows": len(out["raw"]), "cells": nc, "speeds": len(out["speed"]), "speed_points": len(out["speed_smooth"]),
              "dop_points": len(out["dop_smooth"])}
    return counts, out


def series_of(out, stem):
    """[(cell, abscissae, smoothed values)] of the "speed" or the "dop" series."""
    ptr = out[stem + "_smooth_ptr"]
    return [(ci, out[stem + "_smooth_x"][a:b], out[stem + "_smooth"][a:b]) for ci, (a, b) in enumerate(zip(ptr[:-1], ptr[1:]))]


def kept_values(out, stem, ci):
    """The values that were smoothed: the cell's speeds (dopplers) that mask 2 (3) keeps."""
    if stem == "speed":
        a, b = out["speed_ptr"][ci:ci + 2]
        return out["speed"][a:b][out["mask2"][a:b] == 0]
    a, b = out["cell_ptr"][ci:ci + 2]
    return out["dop"][a:b][out["mask3"][a:b] == 0]


def smooth_gap(wide, narrow):
    """The largest |narrow - wide| of a smoothed value relative to its series' scale -> (gap, stem, cell)."""
    worst = (0.0, "", -1)
    for stem in ("speed", "dop"):
        for (ci, _, w), (_, _, v) in zip(series_of(wide, stem), series_of(narrow, stem)):
            y = kept_values(narrow, stem, ci)
            if len(y) == 0 or not np.all(np.isfinite(y)):
                continue
            scale = float(np.max(np.abs(y)))
            gap = float(np.max(np.abs(w - v.astype(np.longdouble)))) / scale if scale > 0 else 0.0
            worst = max(worst, (gap, stem, ci))
    return worst


def assert_smooth_within(got, ref, what=""):
    """Every smoothed value of `got` within SMOOTH_RTOL x the series' scale of the statement's; a series with a value
    that is not finite is compared by its pattern of NaNs."""
    for stem in ("speed", "dop"):
        for (ci, _, g), (_, _, r) in zip(series_of(got, stem), series_of(ref, stem)):
            assert len(g) == len(r), (what, stem, ci)
            y = kept_values(ref, stem, ci)
            if len(y) and np.all(np.isfinite(y)):
                lim = SMOOTH_RTOL * float(np.max(np.abs(y)))
                assert np.all(np.abs(g - r) <= lim), (what, stem, ci, float(np.max(np.abs(g - r))), lim)
            else:
                assert np.array_equal(np.isnan(g), np.isnan(r)), (what, stem, ci)


def assert_stats_within(out, s2m, what=""):
    """mean and std of every cell's kept rows within the rounding bounds of the exact values (syncstats_ref's rule
    and margin, on metres); count, min and max exactly.  A cell with a value that is not finite is compared by the
    caller, against the statement's pattern."""
    for ci in range(len(out["cell_key"])):
        a, b = out["cell_ptr"][ci:ci + 2]
        v = out["x"][a:b][out["mask1"][a:b] == 0]
        got = out["cell_stats"][ci]
        assert got[0] == len(v), (what, ci)
        mean, std, _, mabs = S.exact_stats(v)
        if np.isnan(mean):
            continue
        assert got[3] == np.min(v) * s2m and got[4] == np.max(v) * s2m, (what, ci)
        S.assert_mean_within(got[1], mean * s2m, mabs * s2m, len(v), (what, ci, "mean"))
        S.assert_std_within(got[2], std * s2m, mabs * s2m, len(v), what=(what, ci, "std"))


def assert_same(got, want, sample_rate=2.4e6, what=""):
    """`got` (counts, arrays of the device) against `want` (of the statement), over all rows of all cells: exactly
    but for mean and std (their rounding bounds) and the smoothed values (SMOOTH_RTOL)."""
    assert got[0] == want[0], what
    out, ref = got[1], want[1]
    for name in DISCRETE:
        assert np.array_equal(out[name], ref[name]), (what, name)
    for name in FLOATS:
        assert np.array_equal(out[name], ref[name], equal_nan=True), (what, name)
    for col in (0, 3, 4, 5):       # count, min, max, rows within one std
        assert np.array_equal(out["cell_stats"][:, col], ref["cell_stats"][:, col], equal_nan=True), (what, "cell_stats", col)
    assert np.array_equal(np.isnan(out["cell_stats"]), np.isnan(ref["cell_stats"])), what
    assert_stats_within(out, LIGHT / sample_rate, what)
    assert_smooth_within(out, ref, what)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # the package, for the tile length
    import reldist_scenes
    worst = (0.0, "", "", -1)
    for name, (args, kwargs) in reldist_scenes.every_input().items():
        narrow = reldist_ref(*args, **kwargs)[1]
        wide = reldist_ref(*args, dtype=np.longdouble, **kwargs)[1]
        gap, stem, ci = smooth_gap(wide, narrow)
        print("%-28s %.3g" % (name, gap))
        worst = max(worst, (gap, name, stem, ci))
    print("largest relative gap %.3g (scene %s, %s, cell %d); 16 x = %.3g" % (worst + (16 * worst[0],)))
