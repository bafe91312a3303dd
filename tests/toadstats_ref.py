"""Sequential NumPy statement of the detection statistics (include/thrifty_hip.h:
thr_toadstats), and an exact one in rational arithmetic on the float64 inputs.  Shared by
tests/test_toadstats_host.py, tests/test_gpu_toadstats.py, tests/test_gpu_toadstats_seams.py and
tests/golden/make_golden_toadstats.py; scripts/bench_toadstats.py times `toad_stats_ref` as the host side."""
import math
from fractions import Fraction

import numpy as np

COLUMNS = (("rxid", np.int32), ("txid", np.int32), ("carrier_bin", np.int32), ("timestamp", np.float64),
           ("soa", np.float64), ("carrier_offset", np.float64), ("carrier_energy", np.float64),
           ("carrier_noise", np.float64), ("energy", np.float64), ("noise", np.float64), ("offset", np.float64))
N_Q = 9
MAX_BINS = 1 << 26
U = 2.0 ** -53


def columns_of(cols):
    return {name: np.ascontiguousarray(cols[name], dtype=kind) for name, kind in COLUMNS}


def quantities(c, rows, snr_db=None):
    """float64[9][len(rows)]: the nine quantities of the selected rows (snr_db: the two dB columns to use
    instead of NumPy's own)."""
    with np.errstate(all="ignore"):
        cdb = 20 * np.log10(c["carrier_energy"][rows] / c["carrier_noise"][rows]) if snr_db is None else snr_db[:, 0]
        db = 20 * np.log10(c["energy"][rows] / c["noise"][rows]) if snr_db is None else snr_db[:, 1]
    return np.array([c["carrier_energy"][rows], c["carrier_noise"][rows], cdb, c["carrier_bin"][rows].astype(np.float64),
                     c["carrier_offset"][rows], c["energy"][rows], c["noise"][rows], db, c["offset"][rows]])


def offset_histogram(x):
    """np.histogram(x, 10) restated operation by operation -> (edges float64[11], counts int64[10], flag)."""
    lo, hi = np.min(x), np.max(x)
    if not (np.isfinite(lo) and np.isfinite(hi)):
        return np.full(11, np.nan), np.zeros(10, dtype=np.int64), 1
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    delta = hi - lo
    step = delta / 10.0
    edges = np.empty(11)
    for i in range(10):
        y = (i / 10.0) * delta if step == 0 else i * step
        edges[i] = y + lo
    edges[10] = hi
    counts = np.zeros(10, dtype=np.int64)
    for v in x:
        i = int(((v - lo) / delta) * 10.0)
        if i == 10:
            i = 9
        if v < edges[i]:
            i -= 1
        if i != 9 and v >= edges[i + 1]:
            i += 1
        counts[i] += 1
    return edges, counts, 0


def line_fit(soa, ts):
    """The line ts ~ a * soa + b, fitted in u = (soa - mean) / max|soa - mean| on ts - mean ->
    (a, b, residuals a * soa + b - ts).  Fewer than two distinct soa: NaN."""
    n = len(soa)
    if not np.min(soa) < np.max(soa):
        return np.nan, np.nan, np.full(n, np.nan)
    mean_x, mean_y = np.sum(soa) / n, np.sum(ts) / n
    scale = np.max(np.abs(soa - mean_x))
    u, v = (soa - mean_x) / scale, ts - mean_y
    s1, s2, t0, t1 = np.sum(u), np.sum(u * u), np.sum(v), np.sum(u * v)
    c1 = (n * t1 - s1 * t0) / (n * s2 - s1 * s1)
    c0 = (t0 - c1 * s1) / n
    a = c1 / scale
    return a, (mean_y + c0) - a * mean_x, (c0 + c1 * u) - v


def check_selection(c, sel):
    """The selected rows (int64) or ValueError: what thr_toadstats refuses on the host."""
    n = len(c["timestamp"])
    if sel is None:
        rows = np.arange(n, dtype=np.int64)
    else:
        rows = np.asarray(sel, dtype=np.int64)
        if len(rows) and (rows.min() < 0 or rows.max() >= n):
            raise ValueError("sel is out of range")
        if np.any(np.diff(rows) <= 0):
            raise ValueError("sel must be strictly ascending")
    if len(rows) == 0:
        raise ValueError("the selection is empty")
    if not np.all(np.isfinite(c["timestamp"][rows])):
        raise ValueError("a timestamp is not finite")
    return rows


def toad_stats_ref(cols, sel=None, snr_db=None):
    """Every output of thr_toadstats, cell by cell and receiver by receiver."""
    c = columns_of(cols)
    rows = check_selection(c, sel)
    m = len(rows)
    time0 = np.min(c["timestamp"][rows])
    ts = c["timestamp"][rows] - time0
    if not math.floor((np.max(ts)) / 60.0) + 1 <= MAX_BINS:
        raise ValueError("the histograms would exceed 2^26 bins")
    rx, tx = c["rxid"][rows], c["txid"][rows]
    q = quantities(c, rows, snr_db)
    order = np.lexsort((tx, rx))        # stable: rows of one cell keep their order
    srx, stx = rx[order], tx[order]
    head = np.flatnonzero(np.r_[True, (srx[1:] != srx[:-1]) | (stx[1:] != stx[:-1])])
    cell_ptr = np.r_[head, m].astype(np.int64)
    nc = len(head)
    out = {"cell_rx": srx[head].astype(np.int32), "cell_tx": stx[head].astype(np.int32), "cell_ptr": cell_ptr,
           "order": rows[order], "snr_db": np.ascontiguousarray(q[[2, 7]].T), "stats": np.zeros((nc, N_Q, 4)),
           "bin_first": np.zeros(nc, dtype=np.int32), "offset_edges": np.zeros((nc, 11)),
           "offset_hist": np.zeros((nc, 10), dtype=np.int64), "cell_flags": np.zeros(nc, dtype=np.int32)}
    minute, bins = [], []
    with np.errstate(all="ignore"):
        for ci in range(nc):
            j = order[cell_ptr[ci]:cell_ptr[ci + 1]]
            for k in range(N_Q):
                x = q[k][j]
                mean = np.sum(x) / len(x)
                out["stats"][ci, k] = (mean, np.sqrt(np.sum((x - mean) * (x - mean)) / len(x)), np.min(x), np.max(x))
            minute.append(np.bincount(np.floor(ts[j] / 60.0).astype(np.int64)))
            b = c["carrier_bin"][rows][j].astype(np.int64)
            out["bin_first"][ci] = b.min()
            bins.append(np.bincount(b - b.min()))
            out["offset_edges"][ci], out["offset_hist"][ci], out["cell_flags"][ci] = offset_histogram(q[8][j])
    out["minute_ptr"] = np.r_[0, np.cumsum([len(h) for h in minute])].astype(np.int64)
    out["minute_hist"] = np.concatenate(minute).astype(np.int64)
    out["bin_ptr"] = np.r_[0, np.cumsum([len(h) for h in bins])].astype(np.int64)
    out["bin_hist"] = np.concatenate(bins).astype(np.int64)
    if len(out["minute_hist"]) + len(out["bin_hist"]) + 10 * nc > MAX_BINS:
        raise ValueError("the histograms would exceed 2^26 bins")
    rx_ids = np.unique(rx)
    out["rx_id"] = rx_ids.astype(np.int32)
    out["rx_count"] = np.zeros(len(rx_ids), dtype=np.int64)
    out["rx_fit"] = np.zeros((len(rx_ids), 4))
    out["residual"] = np.zeros(m)
    soa = c["soa"][rows]
    with np.errstate(all="ignore"):
        for r, rid in enumerate(rx_ids):
            j = np.flatnonzero(rx == rid)
            a, b, res = line_fit(soa[j], ts[j])
            out["residual"][j] = res
            out["rx_count"][r] = len(j)
            out["rx_fit"][r] = (a, b, np.sqrt(np.sum(res * res) / len(j)), np.max(np.abs(res)) if len(j) else np.nan)
    counts = {"rows": m, "cells": nc, "receivers": len(rx_ids), "minute_bins": len(out["minute_hist"]),
              "carrier_bins": len(out["bin_hist"]), "offset_bins": 10 * nc, "time0": float(time0)}
    return counts, out


# ---------------------------------------------------------------- exact values
def _sqrt_fraction(v):
    """float nearest (within an ulp) to the square root of a non-negative Fraction."""
    if v == 0:
        return 0.0
    pq = v.numerator * v.denominator            # sqrt(p / q) = sqrt(p q) / q
    k = max(0, 80 - pq.bit_length() // 2)       # the integer root carries at least 80 bits
    return float(Fraction(math.isqrt(pq << (2 * k)), v.denominator << k))


def exact_mean_std(x):
    """(mean, population std, mean |x|) of float64 values in rational arithmetic, rounded once; NaN when a value
    is not finite."""
    if not np.all(np.isfinite(x)):
        return np.nan, np.nan, np.nan
    f = [Fraction(float(v)) for v in x]
    n = len(f)
    mean = sum(f) / n
    var = sum((v - mean) ** 2 for v in f) / n
    return float(mean), _sqrt_fraction(var), float(sum(abs(v) for v in f) / n)


def exact_line(soa, ts):
    """Least-squares line ts ~ a * soa + b in rational arithmetic -> (a, b, residuals, their population std,
    their largest magnitude) as floats; NaN with fewer than two distinct soa."""
    n = len(soa)
    if not np.min(soa) < np.max(soa):
        return np.nan, np.nan, np.full(n, np.nan), np.nan, np.nan
    x, y = [Fraction(float(v)) for v in soa], [Fraction(float(v)) for v in ts]
    mx, my = sum(x) / n, sum(y) / n
    sxx = sum((v - mx) ** 2 for v in x)
    sxy = sum((v - mx) * (w - my) for v, w in zip(x, y))
    a = sxy / sxx
    b = my - a * mx
    res = [a * v + b - w for v, w in zip(x, y)]
    var = sum(r * r for r in res) / n - (sum(res) / n) ** 2
    return float(a), float(b), np.array([float(r) for r in res]), _sqrt_fraction(var), float(max(abs(r) for r in res))


def exact_values(cols, sel=None, snr_db=None):
    """Per cell exact mean / std / mean|x| of the nine quantities (float64[cells][9][3]; the dB quantities from
    `snr_db` when given, else from NumPy's) and per receiver the exact line (a, b, std, max) and residuals."""
    c = columns_of(cols)
    counts, ref = toad_stats_ref(c, sel, snr_db)
    rows = check_selection(c, sel)
    q = quantities(c, rows, snr_db)
    ts = c["timestamp"][rows] - counts["time0"]
    sel_pos = {int(r): i for i, r in enumerate(rows)}
    pos = np.array([sel_pos[int(r)] for r in ref["order"]])
    cells = np.zeros((counts["cells"], N_Q, 3))
    for ci in range(counts["cells"]):
        j = pos[ref["cell_ptr"][ci]:ref["cell_ptr"][ci + 1]]
        for k in range(N_Q):
            cells[ci, k] = exact_mean_std(q[k][j])
    fit = np.zeros((counts["receivers"], 4))
    residual = np.zeros(len(rows))
    rx = c["rxid"][rows]
    for r, rid in enumerate(ref["rx_id"]):
        j = np.flatnonzero(rx == rid)
        a, b, res, std, biggest = exact_line(c["soa"][rows][j], ts[j])
        fit[r] = (a, b, std, biggest)
        residual[j] = res
    return {"cells": cells, "rx_fit": fit, "residual": residual}


# ---------------------------------------------------------------- the bounds of the issue, as functions
def assert_stats_within_bounds(stats, exact_cells, cell_ptr, what=""):
    """|mean - exact| <= (m + 2) u mean|x| and |std - exact| <= (m + 4) u (std + mean|x|), per cell and quantity;
    where the exact value is NaN (a non-finite input) the value is only required not to be finite-and-wrong:
    it is compared with NumPy's by the caller."""
    worst = 0.0
    for ci in range(len(exact_cells)):
        m = int(cell_ptr[ci + 1] - cell_ptr[ci])
        for k in range(N_Q):
            mean, std, mabs = exact_cells[ci, k]
            if np.isnan(mean):
                continue
            lim_mean = (m + 2) * U * mabs
            lim_std = (m + 4) * U * (std + mabs)
            assert abs(stats[ci, k, 0] - mean) <= lim_mean, (what, ci, k, stats[ci, k, 0], mean, lim_mean)
            assert abs(stats[ci, k, 1] - std) <= lim_std, (what, ci, k, stats[ci, k, 1], std, lim_std)
            if lim_mean > 0:
                worst = max(worst, abs(stats[ci, k, 0] - mean) / lim_mean)
            if lim_std > 0:
                worst = max(worst, abs(stats[ci, k, 1] - std) / lim_std)
    return worst


def assert_fit_within_bounds(rx_fit, residual, exact, cols, sel=None, what=""):
    """|a - exact| max|soa - mean soa| <= (n + 8) u max|timestamp|; residuals, std and max within the same."""
    c = columns_of(cols)
    rows = check_selection(c, sel)
    ts = c["timestamp"][rows] - np.min(c["timestamp"][rows])
    rx = c["rxid"][rows]
    for r, rid in enumerate(np.unique(rx)):
        j = np.flatnonzero(rx == rid)
        a, b, std, biggest = exact["rx_fit"][r]
        if np.isnan(a):
            assert np.all(np.isnan(rx_fit[r])) and np.all(np.isnan(residual[j])), (what, r)
            continue
        soa = c["soa"][rows][j]
        lim = (len(j) + 8) * U * np.max(np.abs(ts[j]))
        spread = np.max(np.abs(soa - np.mean(soa)))
        assert abs(rx_fit[r, 0] - a) * spread <= lim, (what, r, rx_fit[r, 0], a, lim)
        assert np.max(np.abs(residual[j] - exact["residual"][j])) <= lim, (what, r, lim)
        assert abs(rx_fit[r, 2] - std) <= lim and abs(rx_fit[r, 3] - biggest) <= lim, (what, r, rx_fit[r], std, biggest)
