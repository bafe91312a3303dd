"""Sequential statement of `tdoa` on columns -- test infrastructure, the role tests/match_ref.py has for
`match`.  Plain numpy float64:

1. a match whose first detection's txid is a key of `beacon_pos` is a beacon match; every pair of its
   detections (itertools.combinations order, det0 = the lower rxid) is appended to the list of its
   receiver pair, in match order -- the lists are never sorted;
2. per pair of every other (mobile) match: Python's bisect_left / bisect_right on the list's det0
   timestamps at det0.timestamp -/+ window (spelled out below: they must also say what happens on an
   unsorted list); a receiver pair without a list has an empty window;
3. more than one pair in the window: np.median / MAD mask on soa0 - soa1, dropped where
   0.6745 * diff / mad > 3.5 (IEEE for mad == 0);
4. fewer than deg + 1 kept pairs, or fewer than deg + 1 distinct abscissae: a failure; otherwise a
   least-squares polynomial of y = soa0 on x = soa1 + beacon_sdoa in u = (x - mean) / max|x - mean|
   on y - mean(y) (np.linalg.lstsq on the small Vandermonde of u), evaluated at the mobile det1's soa;
   |tdoa| >= MAX_TDOA: a failure;
5. a mobile match with at least one TDOA is a group.
"""
import itertools

import numpy as np

SPEED_OF_LIGHT = 2.997e8
MAX_TDOA = 30e3 / SPEED_OF_LIGHT


def bisect_left(a, x):
    lo, hi = 0, len(a)
    while lo < hi:
        mid = (lo + hi) // 2
        if a[mid] < x:
            lo = mid + 1
        else:
            hi = mid
    return lo


def bisect_right(a, x):
    lo, hi = 0, len(a)
    while lo < hi:
        mid = (lo + hi) // 2
        if x < a[mid]:
            hi = mid
        else:
            lo = mid + 1
    return lo


def ordered_pairs(match, rxid):
    for a, b in itertools.combinations(match, 2):
        if rxid[a] == rxid[b]:
            raise ValueError("two detections of receiver %d in one match" % rxid[a])
        yield (a, b) if rxid[a] < rxid[b] else (b, a)


def outlier_mask(sdoa):
    median = np.median(sdoa)
    diff = np.sqrt((sdoa - median) ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 0.6745 * diff / np.median(diff) > 3.5


def tdoa_ref(rxid, txid, timestamp, soa, energy, noise, matches, window, beacon_pos, rx_pos, sample_rate, deg=2):
    """-> dict: groups [(group_id, timestamp, tx, [(rx0, rx1, tdoa, snr, model_quality, det0, det1)])],
    failures [(det0, det1)], n_window, n_kept per task, and per task `kept` (positions in the receiver
    pair's list), `cond` (of the scaled Vandermonde) and `spread` (max |y - mean y|) for tolerances."""
    rxid, txid = [int(v) for v in rxid], [int(v) for v in txid]
    timestamp, soa = np.asarray(timestamp, float), np.asarray(soa, float)
    quality = (np.asarray(energy, float) / np.asarray(noise, float)) ** 2
    for match in matches:
        for rx in (rxid[i] for i in match):
            if rx not in rx_pos:
                raise KeyError(rx)
    lists = {}
    for match in matches:
        if txid[match[0]] in beacon_pos:
            for d0, d1 in ordered_pairs(match, rxid):
                lists.setdefault((rxid[d0], rxid[d1]), []).append((d0, d1))
    out = {"groups": [], "failures": [], "n_window": [], "n_kept": [], "kept": [], "cond": [], "spread": []}

    def distance(a, b):
        return np.sqrt(np.sum((np.asarray(a, float) - np.asarray(b, float)) ** 2))

    for group_id, match in enumerate(matches):
        if txid[match[0]] in beacon_pos:
            continue
        rows, tx = [], None
        for d0, d1 in ordered_pairs(match, rxid):
            tx = txid[d0]
            pairs = lists.get((rxid[d0], rxid[d1]), [])
            stamps = [timestamp[p[0]] for p in pairs]
            left = bisect_left(stamps, timestamp[d0] - window)
            right = bisect_right(stamps, timestamp[d0] + window)
            positions = list(range(left, right))
            out["n_window"].append(len(positions))
            if len(positions) > 1:
                sdoa = np.array([soa[pairs[p][0]] - soa[pairs[p][1]] for p in positions])
                positions = [p for p, bad in zip(positions, outlier_mask(sdoa)) if not bad]
            out["n_kept"].append(len(positions))
            out["kept"].append(positions)
            out["cond"].append(np.nan)
            out["spread"].append(np.nan)
            b0 = np.array([pairs[p][0] for p in positions], dtype=int)
            b1 = np.array([pairs[p][1] for p in positions], dtype=int)
            beacon_tdoa = np.array([(distance(rx_pos[rxid[d0]], beacon_pos[txid[b]]) -
                                     distance(rx_pos[rxid[d1]], beacon_pos[txid[b]])) / SPEED_OF_LIGHT for b in b0])
            x = soa[b1] + beacon_tdoa * sample_rate if len(positions) else np.zeros(0)
            if len(positions) < deg + 1 or len(np.unique(x)) < deg + 1:
                out["failures"].append((d0, d1))
                continue
            y = soa[b0]
            mean_x, mean_y = np.mean(x), np.mean(y)
            scale = np.max(np.abs(x - mean_x))
            vander = np.vander((x - mean_x) / scale, deg + 1, increasing=True)
            coef = np.linalg.lstsq(vander, y - mean_y, rcond=None)[0]
            u = (soa[d1] - mean_x) / scale
            tdoa = ((soa[d0] - mean_y) - np.polyval(coef[::-1], u)) / sample_rate
            out["cond"][-1] = float(np.linalg.cond(vander))
            out["spread"][-1] = float(np.max(np.abs(y - mean_y)))
            if abs(tdoa) >= MAX_TDOA:
                out["failures"].append((d0, d1))
                continue
            rows.append((rxid[d0], rxid[d1], float(tdoa), float((quality[d0] + quality[d1]) / 2),
                         float((np.mean(quality[b0]) + np.mean(quality[b1])) / 2), d0, d1))
        if rows:
            out["groups"].append((group_id, float(timestamp[match[0]]), tx, rows))
    return out
