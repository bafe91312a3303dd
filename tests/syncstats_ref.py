"""Sequential NumPy statement of the clock-sync and TDOA statistics (include/thrifty_hip.h:
thr_beaconsync, thr_tdoastats) over all cells, exact values in rational arithmetic on the float64 inputs, and
the bounds the device is held to.  Shared by tests/test_syncstats_host.py, tests/test_gpu_syncstats.py,
tests/test_gpu_syncstats_seams.py and tests/golden/make_golden_syncstats.py; scripts/bench_syncstats.py times
`beacon_sync_ref` and `tdoa_stats_ref` as the host side."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
LIGHT = 2.997e8
CUT_FITTED, CUT_DEGENERATE, CELL_NO_FIT = 1, 2, 1
BSYNC_COLUMNS = (("rxid", np.int32), ("txid", np.int32), ("soa", np.float64), ("energy", np.float64),
                 ("noise", np.float64), ("idx", np.int64))
TDSTATS_COLUMNS = (("rx0", np.int32), ("rx1", np.int32), ("tx", np.int32), ("timestamp", np.float64),
                   ("det0_idx", np.int64), ("det1_idx", np.int64), ("tdoa", np.float64))


def columns_of(cols, spec):
    return {name: np.ascontiguousarray(cols[name], dtype=kind) for name, kind in spec}


# ---------------------------------------------------------------- beacon sync
def rows_of(c, match_ptr, match_idx, id_range=None, beacons=None, receivers=None):
    """(keys int64[m][3], det int64[m][2], match int64[m]) grouped by (beacon, rx0, rx1), match order inside a
    cell; ValueError for a match with two detections of one receiver."""
    ptr, idx = np.asarray(match_ptr, np.int64), np.asarray(match_idx, np.int64)
    rx, tx, ids = c["rxid"], c["txid"], c["idx"]
    keys, det, match = [], [], []
    for m in range(len(ptr) - 1):
        members = idx[ptr[m]:ptr[m + 1]]
        if len(set(rx[members].tolist())) != len(members):
            raise ValueError("match %d holds two detections of one receiver" % m)
    for m in range(len(ptr) - 1):
        members = idx[ptr[m]:ptr[m + 1]].tolist()
        if not members or (beacons is not None and tx[members[0]] not in beacons):
            continue
        for i, a in enumerate(members):
            for b in members[i + 1:]:
                d0, d1 = (a, b) if rx[a] < rx[b] else (b, a)
                if receivers is not None and (rx[d0] not in receivers or rx[d1] not in receivers):
                    continue
                if id_range is not None and not all(id_range[0] <= ids[d] <= id_range[1] for d in (d0, d1)):
                    continue
                keys.append((tx[members[0]], rx[d0], rx[d1]))
                det.append((d0, d1))
                match.append(m)
    if not keys:
        raise ValueError("the selection is empty")
    keys, det, match = np.array(keys, np.int64), np.array(det, np.int64), np.array(match, np.int64)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))      # stable
    return keys[order], det[order], match[order]


def centred_fit(soa0, soa1, deg):
    """The fit of one cut as the device states it -> (fit[7], residuals), None when it cannot be fitted."""
    sdoa = soa1 - soa0
    n = len(soa0)
    if not np.min(soa0) < np.max(soa0):
        return None
    x_mean, s_mean = np.sum(soa0) / n, np.sum(sdoa) / n
    scale = max(abs(np.max(soa0) - x_mean), abs(np.min(soa0) - x_mean))
    if not (np.isfinite(scale) and np.isfinite(s_mean)):
        return None
    u, w = (soa0 - x_mean) / scale, sdoa - s_mean
    c = np.linalg.lstsq(np.vander(u, deg + 1, increasing=True), w, rcond=None)[0]
    residual = w - np.polyval(c[::-1], u)
    y_mean = x_mean + s_mean
    fit = np.zeros(7)
    fit[:3] = x_mean, scale, y_mean
    fit[3:4 + deg] = c
    fit[3] += (x_mean - (y_mean - (y_mean - x_mean))) + (s_mean - (y_mean - x_mean))
    fit[4] += scale
    return fit, residual


def beacon_sync_ref(cols, match_ptr, match_idx, deg=2, id_range=None, beacons=None, receivers=None):
    """Every output of thr_beaconsync, cell by cell and cut by cut."""
    c = columns_of(cols, BSYNC_COLUMNS)
    keys, det, match = rows_of(c, match_ptr, match_idx, id_range, beacons, receivers)
    m = len(keys)
    head = np.flatnonzero(np.r_[True, np.any(keys[1:] != keys[:-1], axis=1)])
    cell_ptr = np.r_[head, m].astype(np.int64)
    nc = len(head)
    soa0, soa1 = c["soa"][det[:, 0]], c["soa"][det[:, 1]]
    with np.errstate(all="ignore"):
        snr2 = (c["energy"][det] ** 2 / c["noise"][det] ** 2)
    sdoa = soa1 - soa0
    residual = np.full(m, np.nan)
    disc, disc_ptr, cut_ptr = [], [0], [0]
    cuts = {"left": [], "right": [], "flags": [], "fit": [], "snr": [], "disc_soa": []}
    cell_counts, cell_stats, cell_flags = np.zeros((nc, 3), np.int64), np.zeros((nc, 4)), np.zeros(nc, np.int32)
    with np.errstate(all="ignore"):
        for ci in range(nc):
            a, b = cell_ptr[ci], cell_ptr[ci + 1]
            n = b - a
            dsdoa = np.diff(sdoa[a:b])
            mean = np.sum(dsdoa) / np.float64(len(dsdoa))
            found = np.flatnonzero(dsdoa > mean * 10)
            disc.append(found)
            edges = np.r_[0, found, n]
            snrs = []
            for i in range(len(edges) - 1):
                left, right = edges[i] + 1, edges[i + 1]
                flag, fit, snr, dsoa = 0, np.full(7, np.nan), np.nan, np.nan
                if left + 8 < right:
                    got = centred_fit(soa0[a + left:a + right], soa1[a + left:a + right], deg)
                    flag = CUT_DEGENERATE
                    if got is not None and np.all(np.isfinite(got[0])):
                        flag, fit = CUT_FITTED, got[0]
                        residual[a + left:a + right] = got[1]
                        snr = np.sum(snr2[a + left:a + right]) / (2.0 * (right - left))
                        snrs.append(snr)
                        dsoa = soa0[a + right] if right != n else np.nan
                for name, value in zip(("left", "right", "flags", "fit", "snr", "disc_soa"), (left, right, flag, fit, snr, dsoa)):
                    cuts[name].append(value)
            disc_ptr.append(disc_ptr[-1] + len(found))
            cut_ptr.append(cut_ptr[-1] + len(found) + 1)
            r = residual[a:b][~np.isnan(residual[a:b])] if snrs else np.zeros(0)
            cell_counts[ci] = n, len(found), len(snrs)
            cell_flags[ci] = 0 if snrs else CELL_NO_FIT
            if snrs:
                rmean = np.sum(r) / len(r)
                cell_stats[ci] = mean, np.sqrt(np.sum((r - rmean) ** 2) / len(r)), np.max(np.abs(r)), np.sum(snrs) / len(snrs)
            else:
                cell_stats[ci] = mean, np.nan, np.nan, np.nan
    out = {"cell_key": keys[head].astype(np.int32), "cell_ptr": cell_ptr, "row_det": det, "row_match": match, "sdoa": sdoa,
           "disc_ptr": np.array(disc_ptr, np.int64), "disc_idx": np.concatenate(disc).astype(np.int64),
           "cut_ptr": np.array(cut_ptr, np.int64), "cut_left": np.array(cuts["left"], np.int64),
           "cut_right": np.array(cuts["right"], np.int64), "cut_flags": np.array(cuts["flags"], np.int32),
           "cut_fit": np.array(cuts["fit"]).reshape(-1, 7), "cut_snr": np.array(cuts["snr"], np.float64),
           "cut_disc_soa": np.array(cuts["disc_soa"], np.float64), "residual": residual, "cell_counts": cell_counts,
           "cell_stats": cell_stats, "cell_flags": cell_flags}
    counts = {"rows": m, "cells": nc, "discontinuities": len(out["disc_idx"]), "cuts": len(out["cut_left"])}
    return counts, out


def polyfit_residuals(soa0, soa1, deg):
    """The reference's fit_poly_model: np.polyfit on the raw SOAs, np.poly1d, one subtraction."""
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            coef = np.polyfit(soa0, soa1, deg)
    return coef, soa1 - np.poly1d(coef)(soa0)


# ---------------------------------------------------------------- exact values
def _sqrt_fraction(v):
    """float nearest (within an ulp) to the square root of a non-negative Fraction."""
    if v == 0:
        return 0.0
    pq = v.numerator * v.denominator            # sqrt(p / q) = sqrt(p q) / q
    k = max(0, 80 - pq.bit_length() // 2)       # the integer root carries at least 80 bits
    return float(Fraction(math.isqrt(pq << (2 * k)), v.denominator << k))


def fractions_of(x):
    return [Fraction(float(v)) for v in x]


def exact_stats(x):
    """(mean, population std, rms, mean |x|) of float64 values in rational arithmetic, each rounded once; NaN
    when a value is not finite or there is none."""
    if len(x) == 0 or not np.all(np.isfinite(x)):
        return (np.nan,) * 4
    f = fractions_of(x)
    n = len(f)
    mean = sum(f) / n
    return (float(mean), _sqrt_fraction(sum((v - mean) ** 2 for v in f) / n), _sqrt_fraction(sum(v * v for v in f) / n),
            float(sum(abs(v) for v in f) / n))


def exact_polyfit(soa0, soa1, deg):
    """The least-squares polynomial of soa1 on soa0 in rational arithmetic -> (coefficients in powers of
    (x - mean), lowest first, and mean, as Fractions; residuals soa1 - fit(soa0) as Fractions)."""
    x, y = fractions_of(soa0), fractions_of(soa1)
    mean = sum(x) / len(x)
    u = [v - mean for v in x]
    pw = [[Fraction(1)] * len(u)]
    for _ in range(2 * deg):
        pw.append([a * b for a, b in zip(pw[-1], u)])
    s = [sum(p) for p in pw]
    rows = [[s[i + j] for j in range(deg + 1)] + [sum(a * b for a, b in zip(pw[i], y))] for i in range(deg + 1)]
    for col in range(deg + 1):
        piv = next(r for r in range(col, deg + 1) if rows[r][col] != 0)
        rows[col], rows[piv] = rows[piv], rows[col]
        rows[col] = [v / rows[col][col] for v in rows[col]]
        for r in range(deg + 1):
            if r != col:
                rows[r] = [v - rows[r][col] * w for v, w in zip(rows[r], rows[col])]
    coef = [rows[k][-1] for k in range(deg + 1)]
    residual = [b - sum(c * pw[k][i] for k, c in enumerate(coef)) for i, b in enumerate(y)]
    return coef, mean, residual


def expand(coef, mean):
    """sum c_k (x - mean)^k in powers of x, lowest first (Fractions)."""
    total, power = [Fraction(0)] * len(coef), [Fraction(1)]
    for c in coef:
        for i, p in enumerate(power):
            total[i] += c * p
        power = [(power[i - 1] if i else 0) - (power[i] if i < len(power) else 0) * mean for i in range(len(power) + 1)]
    return total


def exact_beacon_values(cols, out, deg):
    """From the discrete outputs `out` (the device's or the restatement's: rows and cuts) the exact numbers:
    per fitted cut the residuals (float64[rows], NaN elsewhere), the raw coefficients (highest power first) and
    the snr; per cell (mean dsdoa, mean |dsdoa|), and (std, max, snr, mean |r|) of the exact residuals."""
    c = columns_of(cols, BSYNC_COLUMNS)
    det = out["row_det"]
    soa0, soa1 = c["soa"][det[:, 0]], c["soa"][det[:, 1]]
    with np.errstate(all="ignore"):
        snr2 = c["energy"][det] ** 2 / c["noise"][det] ** 2
    residual = np.full(len(det), np.nan)
    nc = len(out["cell_ptr"]) - 1
    coefs, cut_snr = {}, np.full(len(out["cut_left"]), np.nan)
    cells = np.full((nc, 6), np.nan)
    for ci in range(nc):
        a, b = int(out["cell_ptr"][ci]), int(out["cell_ptr"][ci + 1])
        dsdoa = np.diff(out["sdoa"][a:b])
        mean, _, _, mabs = exact_stats(dsdoa)
        cells[ci, :2] = mean, mabs
        res, snrs = [], []
        for g in range(int(out["cut_ptr"][ci]), int(out["cut_ptr"][ci + 1])):
            if out["cut_flags"][g] != CUT_FITTED:
                continue
            lo, hi = a + int(out["cut_left"][g]), a + int(out["cut_right"][g])
            coef, mean_x, r = exact_polyfit(soa0[lo:hi], soa1[lo:hi], deg)
            residual[lo:hi] = [float(v) for v in r]
            res += r
            coefs[g] = np.array([float(v) for v in reversed(expand(coef, mean_x))])
            snr = sum(fractions_of(snr2[lo:hi].reshape(-1))) / (2 * (hi - lo))
            cut_snr[g] = float(snr)
            snrs.append(snr)
        if res:
            rmean = sum(res) / len(res)
            cells[ci, 2:] = (_sqrt_fraction(sum((v - rmean) ** 2 for v in res) / len(res)), float(max(abs(v) for v in res)),
                             float(sum(snrs) / len(snrs)), float(sum(abs(v) for v in res) / len(res)))
    return {"residual": residual, "coef": coefs, "cut_snr": cut_snr, "cells": cells}


# ---------------------------------------------------------------- the bounds, as functions
def residual_floor(soa1):
    """32 roundings at the size of soa1: a four-term Horner evaluation, a subtraction, the coefficients' error."""
    return 32 * U * float(np.max(np.abs(soa1)))


def residual_distances(cols, out, exact):
    """Per fitted cut (cut number -> (distance of out's residuals from the exact ones, the floor))."""
    c = columns_of(cols, BSYNC_COLUMNS)
    soa1 = c["soa"][out["row_det"][:, 1]]
    found = {}
    for ci in range(len(out["cell_ptr"]) - 1):
        a = int(out["cell_ptr"][ci])
        for g in range(int(out["cut_ptr"][ci]), int(out["cut_ptr"][ci + 1])):
            if out["cut_flags"][g] == CUT_FITTED:
                lo, hi = a + int(out["cut_left"][g]), a + int(out["cut_right"][g])
                found[g] = (float(np.max(np.abs(out["residual"][lo:hi] - exact["residual"][lo:hi]))), residual_floor(soa1[lo:hi]))
    return found


def assert_mean_within(value, mean, mabs, n, what=""):
    """|mean - exact| <= (n + 2) u mean|x|: n - 1 additions in any order, a division, and one rounding of the exact value."""
    lim = (n + 2) * U * mabs
    assert abs(value - mean) <= lim, (what, value, mean, lim)


def assert_std_within(value, std, mabs, n, extra=0.0, what=""):
    """|std - exact| <= (n + 4) u (std + mean|x|) (+ extra, for a comparison with the std of OTHER values: the
    population std moves by no more than the largest change of a value)."""
    lim = (n + 4) * U * (std + mabs) + extra
    assert abs(value - std) <= lim, (what, value, std, lim)


def assert_beacon_within_bounds(cols, out, exact, polyfit_distance=None, what=""):
    """Two questions, kept apart.  The fit: residuals per cut within max(2 polyfit_distance, floor) of the exact
    ones.  The summary: it is held to exact values computed from the FETCHED arrays it summarises -- max |r| of
    the fitted cuts' residual rows bit for bit, their population std within (rows + 4) u (std + mean|r|), a
    cut's snr within (2 n + 2) u snr of the exact mean of its 2 n values, the cell's snr within
    (cuts + 2) u mean of the exact mean of the fetched cut values, mean dsdoa within (count + 2) u mean|dsdoa|.
    Returns the largest residual distance in units of the floor."""
    worst = 0.0
    dist = residual_distances(cols, out, exact)
    for g, (d, floor) in dist.items():
        lim = max(2 * (polyfit_distance[g] if polyfit_distance is not None else 0.0), floor)
        assert d <= lim, (what, "cut", g, d, lim)
        worst = max(worst, d / floor)
    for ci in range(len(out["cell_ptr"]) - 1):
        a = int(out["cell_ptr"][ci])
        n = int(out["cell_ptr"][ci + 1]) - a
        mean, mabs, std, biggest = exact["cells"][ci][:4]
        got = out["cell_stats"][ci]
        if n > 1 and not np.isnan(mean):
            assert_mean_within(got[0], mean, mabs, n - 1, (what, ci, "mean dsdoa"))
        cuts = [g for g in range(int(out["cut_ptr"][ci]), int(out["cut_ptr"][ci + 1])) if g in dist]
        if not cuts:
            assert out["cell_flags"][ci] == CELL_NO_FIT and np.all(np.isnan(got[1:])), (what, ci)
            continue
        assert out["cell_flags"][ci] == 0 and out["cell_counts"][ci, 2] == len(cuts), (what, ci)
        # the summary of the fetched residuals: the rows of the fitted cuts and no others
        r = np.concatenate([out["residual"][a + int(out["cut_left"][g]):a + int(out["cut_right"][g])] for g in cuts])
        _, r_std, _, r_abs = exact_stats(r)
        assert got[2] == np.max(np.abs(r)), (what, ci, "max", got[2], np.max(np.abs(r)))
        assert_std_within(got[1], r_std, r_abs, len(r), what=(what, ci, "std"))
        for g in cuts:
            rows = int(out["cut_right"][g] - out["cut_left"][g])
            want = exact["cut_snr"][g]
            if np.isfinite(want):
                assert abs(out["cut_snr"][g] - want) <= (2 * rows + 2) * U * want, (what, "cut snr", g, out["cut_snr"][g], want)
        s_mean, _, _, s_abs = exact_stats(out["cut_snr"][cuts])
        if not np.isnan(s_mean):
            assert_mean_within(got[3], s_mean, s_abs, len(cuts), (what, ci, "snr"))
        # the fit's quality again, seen through the summary: against the std and max of the EXACT residuals
        off = max(max(2 * (polyfit_distance[g] if polyfit_distance is not None else 0.0), dist[g][1]) for g in cuts)
        assert abs(got[1] - std) <= off + (len(r) + 4) * U * (std + r_abs), (what, ci, "std of the exact residuals")
        assert abs(got[2] - biggest) <= off + U * biggest, (what, ci, "max of the exact residuals")
    return worst


# ---------------------------------------------------------------- tdoa statistics
def is_outlier(points, thresh=3.5):
    """stat_tools.is_outlier for one column, operation for operation."""
    with np.errstate(all="ignore"):
        median = np.median(points)
        diff = np.sqrt((points - median) ** 2)
        mad = np.median(diff)
        return 0.6745 * diff / mad > thresh, median, mad


def tdoa_stats_ref(cols, timestamp=None, detidx=None, robust=False):
    """Every output of thr_tdoastats."""
    c = columns_of(cols, TDSTATS_COLUMNS)
    keep = np.ones(len(c["tdoa"]), bool)
    if timestamp is not None:
        keep &= (c["timestamp"] >= timestamp[0]) & (c["timestamp"] <= timestamp[1])
    if detidx is not None:
        for name in ("det0_idx", "det1_idx"):
            keep &= (c[name] >= detidx[0]) & (c[name] <= detidx[1])
    rows = np.flatnonzero(keep)
    if len(rows) == 0:
        raise ValueError("the selection is empty")
    order = rows[np.lexsort((c["tx"][rows], c["rx1"][rows], c["rx0"][rows]))]
    keys = np.column_stack([c["rx0"][order], c["rx1"][order], c["tx"][order]])
    head = np.flatnonzero(np.r_[True, np.any(keys[1:] != keys[:-1], axis=1)])
    cell_ptr = np.r_[head, len(order)].astype(np.int64)
    nc = len(head)
    x = c["tdoa"][order] * LIGHT
    out = {"cell_key": keys[head].astype(np.int32), "cell_ptr": cell_ptr, "order": order.astype(np.int64),
           "stats": np.zeros((nc, 5)), "robust_stats": np.zeros((nc if robust else 0, 5)),
           "robust_count": np.zeros(nc if robust else 0, np.int64), "mask": np.zeros(len(order) if robust else 0, np.uint8),
           "median": np.zeros((nc if robust else 0, 2))}

    def five(v):
        mean = np.sum(v) / np.float64(len(v))
        return mean, np.sqrt(np.sum((v - mean) * (v - mean)) / len(v)), np.sqrt(np.sum(v * v) / len(v)), np.min(v), np.max(v)

    with np.errstate(all="ignore"):
        for ci in range(nc):
            v = x[cell_ptr[ci]:cell_ptr[ci + 1]]
            out["stats"][ci] = five(v)
            if robust:
                mask, median, mad = is_outlier(v)
                if len(v) <= 1:
                    mask = np.zeros(len(v), bool)
                out["mask"][cell_ptr[ci]:cell_ptr[ci + 1]] = mask
                out["median"][ci] = median, mad
                out["robust_count"][ci] = np.sum(~mask)
                out["robust_stats"][ci] = five(v[~mask])
    return {"rows": len(order), "cells": nc, "robust": int(bool(robust))}, out


def assert_tdoa_within_bounds(cols, out, what=""):
    """mean, std and RMS of every cell (and of its kept rows) within the rounding bounds of the exact values;
    a cell with a non-finite value is skipped here (the caller compares it with NumPy's pattern)."""
    c = columns_of(cols, TDSTATS_COLUMNS)
    x = c["tdoa"][out["order"]] * LIGHT
    for ci in range(len(out["cell_ptr"]) - 1):
        a, b = int(out["cell_ptr"][ci]), int(out["cell_ptr"][ci + 1])
        sets = [(out["stats"][ci], x[a:b])]
        if len(out["mask"]):
            sets.append((out["robust_stats"][ci], x[a:b][out["mask"][a:b] == 0]))
        for got, v in sets:
            mean, std, rms, mabs = exact_stats(v)
            if np.isnan(mean):
                continue
            n = len(v)
            assert_mean_within(got[0], mean, mabs, n, (what, ci, "mean"))
            assert_std_within(got[1], std, mabs, n, what=(what, ci, "std"))
            assert abs(got[2] - rms) <= (n + 4) * U * rms, (what, ci, "rms", got[2], rms)
