#!/usr/bin/env python3
"""Golden fixtures for the `tdoa` step, made by RUNNING THE REFERENCE's thrifty/tdoa_est.py
(`estimate_tdoas`, its default model) on synthetic detections and matches.  Needs a checkout of the
reference; THRIFTY_REFERENCE names it:

    THRIFTY_REFERENCE=<checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tdoa.py

The reference's module is Python 2 (`iteritems`, `sort(cmp=...)`, `basestring`).  It is imported as it
is and three names are put into its namespace: a `collections` whose defaultdict has `iteritems`, a
`list` whose `sort` takes `cmp` through functools.cmp_to_key (the reference's comparator never returns
a negative number, so the sort leaves the list alone -- under Python 2 and here), and `basestring`.
Two more hooks only LISTEN: `stat_tools.is_outlier` is wrapped to note the window length, and the
`model_builder` argument of `estimate_tdoas` is a wrapper around the reference's `build_model_poly`
that notes the kept pairs and solves the same least-squares problem EXACTLY (fractions.Fraction normal
equations on the float64 abscissae and ordinates the reference fits).

Each file under tests/golden/tdoa/ holds the detection columns, the matches as CSR, the positions,
(window, sample_rate, deg), and the reference's answer: groups (group_id, group_timestamp, group_tx,
group_ptr), rows (rx0, rx1, tdoa, snr, model_quality, det0, det1) with `exact_tdoa` beside them,
failures, per detection pair of the mobile matches n_window, n_kept and mad_zero (0: the window's MAD
is not zero or it was not masked, 1: MAD == 0 and every difference equals the median, 2: MAD == 0 and
some do not -- those pairs divide by zero and are dropped), and
ref_err_max = max |tdoa - exact_tdoa|.  Matches listed in `uncovered_matches` hold a receiver pair no
beacon match covers: the reference dies there (KeyError), so it is run WITHOUT them and their pairs are
recorded as what this project defines for them -- empty windows, failures, in their place in the order.
"""
import collections
import fractions
import functools
import itertools
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ["THRIFTY_REFERENCE"])

from thrifty import stat_tools, tdoa_est, toads_data  # noqa: E402


class _DefaultDict(collections.defaultdict):
    def iteritems(self):
        return iter(self.items())


class _List(list):
    def sort(self, cmp=None, **kwargs):
        if cmp is not None:
            kwargs["key"] = functools.cmp_to_key(cmp)
        list.sort(self, **kwargs)


tdoa_est.collections = types.SimpleNamespace(defaultdict=_DefaultDict, OrderedDict=collections.OrderedDict,
                                             namedtuple=collections.namedtuple)
tdoa_est.list = _List
tdoa_est.basestring = str

FS = 2.4e6
C = tdoa_est.SPEED_OF_LIGHT


class Listener(object):
    """Per detection pair of the reference's run, in order: window length, kept pairs, exact answer."""

    def __init__(self, deg):
        self.deg, self.tasks, self.window, self.mad_zero = deg, [], None, 0
        self.is_outlier = stat_tools.is_outlier

    def outlier(self, points, *args, **kwargs):
        self.window = len(points)
        diff = np.abs(points - np.median(points))
        self.mad_zero = 0 if np.median(diff) != 0 else 2 if np.any(diff != 0) else 1
        return self.is_outlier(points, *args, **kwargs)

    def builder(self, detection_pairs, beacon_sdoa, sample_rate):
        task = {"n_kept": len(detection_pairs), "n_window": len(detection_pairs) if self.window is None else self.window,
                "mad_zero": self.mad_zero}
        self.window, self.mad_zero = None, 0
        self.tasks.append(task)
        model = tdoa_est.build_model_poly(detection_pairs, beacon_sdoa, sample_rate, deg=self.deg)
        if model is None:
            return None
        x = np.array([d[1].soa for d in detection_pairs]) + np.array(beacon_sdoa)     # the reference's abscissae
        y = [d[0].soa for d in detection_pairs]
        task["distinct"] = len(set(x.tolist()))
        coef = exact_fit([fractions.Fraction(v) for v in x.tolist()], [fractions.Fraction(v) for v in y], self.deg)

        def evaluate(det0, det1):
            at = fractions.Fraction(det1.soa)
            fit = sum(c * at ** k for k, c in enumerate(coef))
            task["exact"] = float((fractions.Fraction(det0.soa) - fit) / fractions.Fraction(sample_rate))
            task["ref"] = model(det0, det1)
            return task["ref"]

        return evaluate


def exact_fit(x, y, deg):
    """Coefficients (ascending) of the least-squares polynomial, in rational arithmetic."""
    m = deg + 1
    a = [[sum(v ** (r + c) for v in x) for c in range(m)] + [sum(v ** r * w for v, w in zip(x, y))] for r in range(m)]
    for c in range(m):
        pivot = next(r for r in range(c, m) if a[r][c] != 0)
        a[c], a[pivot] = a[pivot], a[c]
        for r in range(m):
            if r != c and a[r][c] != 0:
                f = a[r][c] / a[c][c]
                a[r] = [p - f * q for p, q in zip(a[r], a[c])]
    return [a[r][m] / a[r][r] for r in range(m)]


def scene(rng, rx_sets, beacon_times, mobile_times, soa_noise=0.05, outlier_prob=0.03, ppm=30.0, grid=None,
          bogus_mobile=None):
    """Detections and matches of a field of receivers.  rx_sets[tx] = the receivers that hear
    transmitter tx; beacons are the keys of beacon_times.  Receiver clocks run hours apart and some ppm
    off; every SoA carries noise and now and then a gross error of +-40 samples.  With `grid` the SoAs
    and timestamps lie on coarse grids and the clocks do not drift."""
    n_rx = 1 + max(r for s in rx_sets.values() for r in s)
    rx_pos = {r: rng.uniform(-1500, 1500, 2) for r in range(n_rx)}
    tx_pos = {tx: rng.uniform(-1200, 1200, 2) for tx in rx_sets}
    offset = {r: float(np.round(rng.uniform(1, 4) * 3600 * FS)) for r in range(n_rx)}
    rate = {r: FS * (1 + (0 if grid else rng.uniform(-ppm, ppm) * 1e-6)) for r in range(n_rx)}
    skew = {r: (0.5 * int(rng.integers(-1, 2)) if grid else float(rng.uniform(-0.03, 0.03))) for r in range(n_rx)}
    events = sorted([(t, tx) for tx, times in itertools.chain(beacon_times.items(), mobile_times.items())
                     for t in times])
    rows, members = [], []
    for e, (t, tx) in enumerate(events):
        for r in rx_sets[tx]:
            delay = float(np.linalg.norm(rx_pos[r] - tx_pos[tx])) / C
            soa = offset[r] + (t + delay) * rate[r]
            if grid:        # the same whole number of samples per receiver and transmitter: SoA differences tie;
                # no error at all in the first seconds, so some windows hold nothing but equal differences
                soa = (offset[r] + np.round(t * rate[r]) + np.round(delay * rate[r]) +
                       (grid * int(rng.choice([0] * 12 + [1, -1, 2])) if t >= 12.0 else 0.0))
                stamp = 1.7e9 + np.round(2 * t) / 2 + skew[r] + 0.5 * int(rng.choice([0, 0, 1]))
            else:
                soa += rng.normal(0, soa_noise)
                stamp = round(1.7e9 + t + delay + skew[r] + float(rng.normal(0, 1e-3)), 6)
            if rng.random() < outlier_prob:
                soa += 40.0 * (1 if rng.random() < 0.5 else -1)
            if bogus_mobile is not None and tx == bogus_mobile and r == rx_sets[tx][-1]:
                soa += 600.0        # a false peak: |tdoa| beyond MAX_TDOA
            rows.append((float(stamp), r, tx, float(soa), float(rng.uniform(50, 200)), float(rng.uniform(1, 3)), e))
    order = sorted(range(len(rows)), key=lambda i: rows[i][0])         # .toads order: by timestamp, stable
    rows = [rows[i] for i in order]
    by_event = collections.OrderedDict()
    for i, row in enumerate(rows):
        by_event.setdefault(row[6], []).append(i)
    members = sorted(by_event.values(), key=lambda m: m[0])             # matches by their first detection
    beacon_pos = {tx: tx_pos[tx] for tx in beacon_times}
    return rows, members, rx_pos, beacon_pos


def objects(rows):
    out = []
    for i, (stamp, rx, tx, soa, energy, noise, _) in enumerate(rows):
        car = toads_data.CarrierSyncInfo(40 + tx, 0.1, 150.0, 7.5)
        cor = toads_data.CorrDetectionInfo(4000 + i % 97, 0.25, energy, noise)
        det = toads_data.DetectionResult(stamp, i, soa, car, cor, rx)
        det.txid = tx
        out.append(det)
    return out


def task_pairs(dets, match):
    return [(a, b) if dets[a].rxid < dets[b].rxid else (b, a) for a, b in itertools.combinations(match, 2)]


def save(name, rows, matches, rx_pos, beacon_pos, window, deg=2, require=None):
    dets = objects(rows)
    covered = set()
    for match in matches:
        if dets[match[0]].txid in beacon_pos:
            covered.update((dets[a].rxid, dets[b].rxid) for a, b in task_pairs(dets, match))
    mobile = [m for m, match in enumerate(matches) if dets[match[0]].txid not in beacon_pos]
    uncovered = [m for m in mobile
                 if any((dets[a].rxid, dets[b].rxid) not in covered for a, b in task_pairs(dets, matches[m]))]
    for m in uncovered:     # what this project defines for them must not need the reference: every pair uncovered
        assert all((dets[a].rxid, dets[b].rxid) not in covered for a, b in task_pairs(dets, matches[m])), name
    run = [m for m in range(len(matches)) if m not in set(uncovered)]
    listener = Listener(deg)
    tdoa_est.stat_tools = types.SimpleNamespace(is_outlier=listener.outlier)
    groups, failures = tdoa_est.estimate_tdoas(dets, [matches[m] for m in run], window, beacon_pos, rx_pos, FS,
                                               model_builder=listener.builder)
    groups = [g._replace(group_id=run[g.group_id]) for g in groups]
    # the per-pair records in the order of ALL mobile matches; the uncovered ones: empty windows, failures
    heard = iter(listener.tasks)
    tasks, place = [], {}
    for m in mobile:
        for pair in task_pairs(dets, matches[m]):
            place[pair] = len(tasks)
            tasks.append({"n_window": 0, "n_kept": 0, "mad_zero": 0} if m in set(uncovered) else next(heard))
            if m in set(uncovered):
                failures.append(pair)
    assert next(heard, None) is None
    failures.sort(key=lambda pair: place[pair])
    produced = [t for t in tasks if "ref" in t and abs(t["ref"]) < tdoa_est.MAX_TDOA]
    table = tdoa_est.groups_to_matrix(groups)
    assert len(produced) == len(table) and all(t["ref"] == v for t, v in zip(produced, table["tdoa"])), name
    assert all(t["distinct"] >= deg + 1 for t in tasks if "distinct" in t), name   # (the rank-deficient fit is a deviation)
    exact = np.array([t["exact"] for t in produced], float)
    err = float(np.max(np.abs(table["tdoa"] - exact))) if len(table) else 0.0
    n_window, n_kept = [t["n_window"] for t in tasks], [t["n_kept"] for t in tasks]
    if require:
        require(dets, matches, beacon_pos, tasks, n_window, n_kept, uncovered)
    rx_ids, beacon_ids = sorted(rx_pos), sorted(beacon_pos)
    sizes = np.cumsum([0] + [len(g.tdoas) for g in groups])
    np.savez_compressed(
        os.path.join(HERE, "tdoa", name + ".npz"),
        rxid=np.array([r[1] for r in rows], np.int64), txid=np.array([r[2] for r in rows], np.int64),
        timestamp=np.array([r[0] for r in rows], float), soa=np.array([r[3] for r in rows], float),
        energy=np.array([r[4] for r in rows], float), noise=np.array([r[5] for r in rows], float),
        match_ptr=np.cumsum([0] + [len(m) for m in matches]).astype(np.int64),
        match_idx=np.array([i for m in matches for i in m], np.int64),
        rx_ids=np.array(rx_ids, np.int64), rx_xyz=np.array([rx_pos[r] for r in rx_ids], float),
        beacon_ids=np.array(beacon_ids, np.int64), beacon_xyz=np.array([beacon_pos[b] for b in beacon_ids], float),
        window=float(window), sample_rate=FS, deg=deg,
        group_id=np.array([g.group_id for g in groups], np.int64),
        group_timestamp=np.array([g.timestamp for g in groups], float),
        group_tx=np.array([g.tx for g in groups], np.int64), group_ptr=sizes.astype(np.int64),
        rx0=table["rx0"].astype(np.int64), rx1=table["rx1"].astype(np.int64), tdoa=table["tdoa"].astype(float),
        snr=table["snr"].astype(float), model_quality=table["model_quality"].astype(float),
        det0=table["det0_idx"].astype(np.int64), det1=table["det1_idx"].astype(np.int64), exact_tdoa=exact,
        failures=np.array(failures, np.int64).reshape(-1, 2), n_window=np.array(n_window, np.int64),
        n_kept=np.array(n_kept, np.int64), mad_zero=np.array([t["mad_zero"] for t in tasks], np.int64), ref_err_max=err, uncovered_matches=np.array(uncovered, np.int64))
    print("%-15s %d detections, %d matches (%d mobile, %d uncovered): %d TDOAs in %d groups, %d failures, "
          "windows %d..%d, ref_err_max %.3g s" % (name, len(rows), len(matches), len(mobile), len(uncovered),
                                                   len(table), len(groups), len(failures),
                                                   min(n_window), max(n_window), err))


def times(rng, start, stop, period, jitter=0.3):
    out, t = [], start + float(rng.uniform(0, period))
    while t < stop:
        out.append(t)
        t += period * float(rng.uniform(1 - jitter, 1 + jitter))
    return out


def nonmonotone_lists(dets, matches, beacon_pos):
    lists = {}
    for match in matches:
        if dets[match[0]].txid in beacon_pos:
            for a, b in task_pairs(dets, match):
                lists.setdefault((dets[a].rxid, dets[b].rxid), []).append(dets[a].timestamp)
    return sum(1 for stamps in lists.values() if any(q < p for p, q in zip(stamps, stamps[1:])))


def on_the_edges(dets, matches, beacon_pos, window):
    """(a beacon det0 timestamp equals some task's t0 - window, one equals t0 + window), same receiver pair."""
    stamps = {}
    for match in matches:
        if dets[match[0]].txid in beacon_pos:
            for a, b in task_pairs(dets, match):
                stamps.setdefault((dets[a].rxid, dets[b].rxid), set()).add(dets[a].timestamp)
    tasks = [(dets[a].rxid, dets[b].rxid, dets[a].timestamp) for match in matches
             if dets[match[0]].txid not in beacon_pos for a, b in task_pairs(dets, match)]
    return (any(t - window in stamps.get((r0, r1), ()) for r0, r1, t in tasks),
            any(t + window in stamps.get((r0, r1), ()) for r0, r1, t in tasks))


def main():
    rng = np.random.default_rng(20261018)
    all_rx = [0, 1, 2]

    rows, matches, rx_pos, beacon_pos = scene(
        rng, {0: all_rx, 1: all_rx, 2: all_rx, 3: all_rx},
        {0: times(rng, 0, 60, 1.0), 1: times(rng, 0, 60, 1.0)}, {2: times(rng, 0, 60, 1.0), 3: times(rng, 0, 60, 1.0)})
    save("tdoa_realistic", rows, matches, rx_pos, beacon_pos, 8.0)

    def failures_required(dets, matches, beacon_pos, tasks, n_window, n_kept, uncovered):
        assert {0, 1, 2, 3} <= set(n_window) and uncovered
        assert any("ref" in t and abs(t["ref"]) >= tdoa_est.MAX_TDOA for t in tasks)
        assert any(w >= 3 and k < 3 for w, k in zip(n_window, n_kept))

    rows, matches, rx_pos, beacon_pos = scene(
        rng, {0: all_rx, 2: all_rx, 3: all_rx, 4: [2, 3]},
        {0: times(rng, 0, 400, 9.0, 0.6)}, {2: times(rng, 0, 400, 4.0), 3: times(rng, 0, 400, 16.0), 4: times(rng, 0, 400, 40.0)},
        outlier_prob=0.12, bogus_mobile=3)
    save("tdoa_failures", rows, matches, rx_pos, beacon_pos, 8.0, require=failures_required)

    def ties_required(dets, matches, beacon_pos, tasks, n_window, n_kept, uncovered):
        assert nonmonotone_lists(dets, matches, beacon_pos) >= 1
        zero = [(t["mad_zero"], t["n_window"], t["n_kept"]) for t in tasks]
        assert any(z == 1 and w == k for z, w, k in zero) and any(z == 2 and 3 <= k < w for z, w, k in zero), zero
        assert any(z == 0 and w > 1 for z, w, k in zero)
        assert on_the_edges(dets, matches, beacon_pos, 8.0) == (True, True)
        assert any(w % 2 == 0 and w > 1 for w in n_window) and any(w % 2 == 1 and w > 1 for w in n_window)
        assert any(1 < k < w for w, k in zip(n_window, n_kept)) and any(k == w and w > 1 for w, k in zip(n_window, n_kept))

    rows, matches, rx_pos, beacon_pos = scene(
        rng, {0: all_rx, 1: all_rx, 2: all_rx, 3: all_rx},
        {0: times(rng, 0, 50, 1.0), 1: times(rng, 14, 50, 5.0)}, {2: times(rng, 0, 50, 1.0), 3: times(rng, 0, 50, 2.0)},
        outlier_prob=0.0, grid=1.0)
    save("tdoa_ties", rows, matches, rx_pos, beacon_pos, 8.0, require=ties_required)

    def wide_required(dets, matches, beacon_pos, tasks, n_window, n_kept, uncovered):
        assert {63, 64, 65} <= set(n_window) and 125 <= max(n_window) <= 140, sorted(set(n_window))

    dense = []
    t = 0.0
    while t < 60.0:                      # the beacon rate climbs from 1.5 to 9 a second
        dense.append(t)
        t += 1.0 / (1.5 + 7.5 * t / 60.0)
    rows, matches, rx_pos, beacon_pos = scene(
        rng, {0: [0, 1], 2: [0, 1]}, {0: dense}, {2: times(rng, 0, 60, 0.45)})
    save("tdoa_wide", rows, matches, rx_pos, beacon_pos, 8.0, require=wide_required)


if __name__ == "__main__":
    main()
