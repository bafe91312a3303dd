"""Sequential statement of `tdoa` with the weighted, the nearest and the linear model -- test
infrastructure beside tests/tdoa_ref.py, whose front it shares: the receiver pairs' lists in match order,
Python's two bisections for the window, the median / MAD mask.  What is left of a window after the mask, in
list order, is the KEPT LIST; a model works on it alone.  Plain numpy float64, one operation at a time:

* nearest: no kept pair is a failure.  Bisect the kept det0 timestamps (left) for the task's; step back one
  if that ran off the end, or if the pair before is STRICTLY nearer in time.  The chosen pair gives
  ((soa0 - its soa0) - (soa1 - its soa1) + its beacon_sdoa) / sample_rate.
* linear: fewer than two kept pairs is a failure.  `high` is the same bisection, clamped to the last pair;
  `low` is the nearest earlier position in the kept list whose pair came from the same beacon (none: a
  failure; equal det0 SoAs of the two: a failure).  The task's soa0 is placed between the two det0 SoAs,
  the det1 SoAs are blended in that proportion, and tdoa = ((blend - soa1) + beacon_sdoa[high]) / sample_rate.
* weighted_poly: fewer than deg + 1 kept pairs, or distinct abscissae, is a failure, and so is a kept pair at
  the task's soa0.  w = (sqrt(sqrt(1 / |soa0_i - soa0|) / max) + 2) / 3; least squares of w (y - mean y) on
  w V(u), u the centred and scaled abscissa, as tests/tdoa_ref.py fits the unweighted one.

`picks` says what was chosen, as positions in the kept list: (idx, -1), (low, high), or (-1, -1).
"""
import numpy as np

from tdoa_ref import MAX_TDOA, SPEED_OF_LIGHT, bisect_left, bisect_right, ordered_pairs, outlier_mask

MODELS = ("weighted_poly", "nearest", "linear")


def nearest_position(stamps, t0):
    at = bisect_left(stamps, t0)
    if at == 0:
        return at
    if at == len(stamps):
        return at - 1
    return at - 1 if abs(t0 - stamps[at - 1]) < abs(t0 - stamps[at]) else at


def weights_of(y, soa0):
    w = np.sqrt(1.0 / np.abs(y - soa0))
    w = np.sqrt(w / np.max(w))
    return (w + 2) / 3


def tdoa_models_ref(rxid, txid, timestamp, soa, energy, noise, matches, window, beacon_pos, rx_pos, sample_rate,
                    model, deg=2):
    """-> dict: groups [(group_id, timestamp, tx, [(rx0, rx1, tdoa, snr, model_quality, det0, det1)])],
    failures [(det0, det1)], and per task n_window, n_kept, picks [(a, b)], cond (of the weighted, scaled
    Vandermonde) and spread (max |y - mean y|) -- NaN where nothing was fitted."""
    assert model in MODELS
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
    out = {"groups": [], "failures": [], "n_window": [], "n_kept": [], "picks": [], "cond": [], "spread": []}

    def distance(a, b):
        return np.sqrt(np.sum((np.asarray(a, float) - np.asarray(b, float)) ** 2))

    def estimate(d0, d1, b0, b1, sdoa):
        """tdoa or None; notes the pick, cond and spread of the task."""
        n = len(b0)
        stamps = [timestamp[b] for b in b0]
        if model == "nearest":
            if n < 1:
                return None
            at = nearest_position(stamps, timestamp[d0])
            out["picks"][-1] = (at, -1)
            return ((soa[d0] - soa[b0[at]]) - (soa[d1] - soa[b1[at]]) + sdoa[at]) / sample_rate
        if model == "linear":
            if n < 2:
                return None
            high = min(bisect_left(stamps, timestamp[d0]), n - 1)
            same = [p for p in range(high) if txid[b0[p]] == txid[b0[high]]]
            low = same[-1] if same else -1
            out["picks"][-1] = (low, high)
            if low < 0 or soa[b0[high]] == soa[b0[low]]:
                return None
            share = (soa[d0] - soa[b0[low]]) / (soa[b0[high]] - soa[b0[low]])
            blend = soa[b1[low]] * (1 - share) + soa[b1[high]] * share
            return ((blend - soa[d1]) + sdoa[high]) / sample_rate
        x = soa[b1] + sdoa if n else np.zeros(0)
        if n < deg + 1 or len(np.unique(x)) < deg + 1:
            return None
        y = soa[b0]
        if np.any(y == soa[d0]):
            return None
        w = weights_of(y, soa[d0])
        mean_x, mean_y = np.mean(x), np.mean(y)
        scale = np.max(np.abs(x - mean_x))
        vander = w[:, None] * np.vander((x - mean_x) / scale, deg + 1, increasing=True)
        coef = np.linalg.lstsq(vander, w * (y - mean_y), rcond=None)[0]
        out["cond"][-1] = float(np.linalg.cond(vander))
        out["spread"][-1] = float(np.max(np.abs(y - mean_y)))
        return ((soa[d0] - mean_y) - np.polyval(coef[::-1], (soa[d1] - mean_x) / scale)) / sample_rate

    for group_id, match in enumerate(matches):
        if txid[match[0]] in beacon_pos:
            continue
        rows, tx = [], None
        for d0, d1 in ordered_pairs(match, rxid):
            tx = txid[d0]
            pairs = lists.get((rxid[d0], rxid[d1]), [])
            stamps = [timestamp[p[0]] for p in pairs]
            inside = pairs[bisect_left(stamps, timestamp[d0] - window):bisect_right(stamps, timestamp[d0] + window)]
            out["n_window"].append(len(inside))
            if len(inside) > 1:
                bad = outlier_mask(np.array([soa[p[0]] - soa[p[1]] for p in inside]))
                inside = [p for p, drop in zip(inside, bad) if not drop]
            out["n_kept"].append(len(inside))
            out["picks"].append((-1, -1))
            out["cond"].append(np.nan)
            out["spread"].append(np.nan)
            b0 = np.array([p[0] for p in inside], dtype=int)
            b1 = np.array([p[1] for p in inside], dtype=int)
            sdoa = np.array([(distance(rx_pos[rxid[d0]], beacon_pos[txid[b]]) -
                              distance(rx_pos[rxid[d1]], beacon_pos[txid[b]])) / SPEED_OF_LIGHT for b in b0]) * sample_rate
            tdoa = estimate(d0, d1, b0, b1, sdoa)
            if tdoa is None or abs(tdoa) >= MAX_TDOA:
                out["failures"].append((d0, d1))
                continue
            rows.append((rxid[d0], rxid[d1], float(tdoa), float((quality[d0] + quality[d1]) / 2),
                         float((np.mean(quality[b0]) + np.mean(quality[b1])) / 2), d0, d1))
        if rows:
            out["groups"].append((group_id, float(timestamp[match[0]]), tx, rows))
    return out
