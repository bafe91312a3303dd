#!/usr/bin/env python3
"""Golden fixtures for the `tdoa` step under the reference's other three models, made by RUNNING THE
REFERENCE's `estimate_tdoas` with its own `build_model_weighted_poly`, `build_model_nearest` and
`build_model_linear` on the four scenes of make_golden_tdoa.py (same generator, same seed, same order):

    THRIFTY_REFERENCE=<checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tdoa_models.py

make_golden_tdoa.py's Python-2 shims are in place once it is imported; the models also call
`sorted(..., cmp=...)`, so a `sorted` that takes `cmp` through functools.cmp_to_key goes into the module's
namespace (the comparator never returns a negative number: the order stays, under Python 2 and here).
Everything else only LISTENS: `stat_tools.is_outlier` is wrapped as before, the builder passed as
`model_builder` notes the kept pairs and hands them on, `bisect_left` notes what the models' own
bisections return, and `np` in the module's namespace is a proxy whose `polyfit` notes (x, y, deg, w) of
every weighted fit before calling numpy's.  From those notes the weighted least-squares problem is solved
EXACTLY (fractions.Fraction normal equations with w_i^2 on the float64 values the reference used).

Each file tests/golden/tdoa_models/<scene>_<model>.npz (weighted_poly at deg 2; tdoa_realistic also at
deg 1, `_deg1`) holds what tests/golden/tdoa/<scene>.npz holds -- columns, matches, positions, window,
sample_rate, deg, groups, rows, failures, n_window, n_kept, uncovered_matches -- with `model`, and for the
weighted model `exact_tdoa` and ref_err_max = max |tdoa - exact_tdoa|.  Uncovered receiver pairs are
handled as make_golden_tdoa.py handles them."""
import fractions
import functools
import os
import types

import numpy as np

import make_golden_tdoa as base
from make_golden_tdoa import FS, objects, scene, task_pairs, tdoa_est, times

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "tdoa_models")


def _sorted(iterable, cmp=None, **kwargs):
    if cmp is not None:
        kwargs["key"] = functools.cmp_to_key(cmp)
    return sorted(iterable, **kwargs)


tdoa_est.sorted = _sorted


class _Numpy(object):
    """numpy, with a polyfit that notes its arguments."""

    def __init__(self):
        self.fits = []

    def __getattr__(self, name):
        return getattr(np, name)

    def polyfit(self, x, y, deg, **kwargs):
        self.fits.append((np.array(x, float), np.array(y, float), int(deg), np.array(kwargs["w"], float)))
        return np.polyfit(x, y, deg, **kwargs)


def exact_weighted_fit(x, y, w, deg):
    """Coefficients (ascending) of the polynomial minimising sum (w (y - p(x)))^2, in rational arithmetic."""
    m = deg + 1
    x, y, w2 = ([fractions.Fraction(v) for v in x.tolist()], [fractions.Fraction(v) for v in y.tolist()],
                [fractions.Fraction(v) ** 2 for v in w.tolist()])
    a = [[sum(q * v ** (r + c) for q, v in zip(w2, x)) for c in range(m)] +
         [sum(q * v ** r * t for q, v, t in zip(w2, x, y))] for r in range(m)]
    for c in range(m):
        pivot = next(r for r in range(c, m) if a[r][c] != 0)
        a[c], a[pivot] = a[pivot], a[c]
        for r in range(m):
            if r != c and a[r][c] != 0:
                f = a[r][c] / a[c][c]
                a[r] = [p - f * q for p, q in zip(a[r], a[c])]
    return [a[r][m] / a[r][r] for r in range(m)]


class Listener(base.Listener):
    """Per detection pair of the reference's run, in order: window length, kept pairs, what the model's
    bisection returned, its answer, and for the weighted model the exact answer."""

    def __init__(self, model, deg):
        base.Listener.__init__(self, deg)
        self.model, self.numpy, self.bisections, self.in_model = model, _Numpy(), [], False
        self.reference = {"weighted_poly": tdoa_est.build_model_weighted_poly, "nearest": tdoa_est.build_model_nearest,
                          "linear": tdoa_est.build_model_linear}[model]
        self.python_bisect = tdoa_est.bisect_left

    def bisect_left(self, a, x):
        at = self.python_bisect(a, x)
        if self.in_model:
            self.bisections.append(at)
        return at

    def builder(self, detection_pairs, beacon_sdoa, sample_rate, **params):
        task = {"n_kept": len(detection_pairs), "n_window": len(detection_pairs) if self.window is None else self.window,
                "mad_zero": self.mad_zero, "beacons": [d[0].txid for d in detection_pairs],
                "stamps": [d[0].timestamp for d in detection_pairs]}
        self.window, self.mad_zero = None, 0
        self.tasks.append(task)
        model = self.reference(detection_pairs, beacon_sdoa, sample_rate, **params)
        if model is None:
            return None

        def evaluate(det0, det1):
            self.in_model, self.bisections, self.numpy.fits = True, [], []
            try:
                task["ref"] = model(det0, det1)       # (a ZeroDivisionError of the linear model ends the run)
            finally:
                self.in_model = False
            task["t0"] = det0.timestamp
            if self.model == "weighted_poly":
                (x, y, deg, w), = self.numpy.fits
                assert np.all(np.isfinite(w)) and deg == self.deg
                task["distinct"] = len(set(x.tolist()))
                coef = exact_weighted_fit(x, y, w, deg)
                at = fractions.Fraction(det1.soa)
                fit = sum(c * at ** k for k, c in enumerate(coef))
                task["exact"] = float((fractions.Fraction(det0.soa) - fit) / fractions.Fraction(sample_rate))
            else:
                task["bisect"], = self.bisections
            return task["ref"]

        return evaluate


def met(model, tasks):
    """What the reference itself went through, over the tasks of one model's scenes."""
    seen = set()
    for t in tasks:
        if "ref" in t:
            seen.add("row" if t["ref"] is not None and abs(t["ref"]) < tdoa_est.MAX_TDOA else "failure")
        else:
            seen.add("failure")
        if "bisect" not in t:
            continue
        at, n, stamps = t["bisect"], t["n_kept"], t["stamps"]
        if model == "nearest":
            if n == 1:
                seen.add("n_kept == 1")
            if at == n:
                seen.add("idx == n_kept")
            elif at > 0 and abs(t["t0"] - stamps[at - 1]) < abs(t["t0"] - stamps[at]):
                seen.add("took idx - 1")
        if model == "linear":
            if at == n:
                seen.add("high == n_kept")
            high = min(at, n - 1)
            if t["ref"] is None:
                assert all(b != t["beacons"][high] for b in t["beacons"][:high])
                seen.add("low < 0")
            elif t["beacons"][high - 1] != t["beacons"][high]:
                seen.add("skipped another beacon's pair")
    return seen


REQUIRED = {"weighted_poly": {"row", "failure"},
            "nearest": {"row", "failure", "took idx - 1", "idx == n_kept", "n_kept == 1"},
            "linear": {"row", "failure", "skipped another beacon's pair", "low < 0", "high == n_kept"}}


def save(name, model, rows, matches, rx_pos, beacon_pos, window, deg=2, suffix=""):
    dets = objects(rows)
    covered = set()
    for match in matches:
        if dets[match[0]].txid in beacon_pos:
            covered.update((dets[a].rxid, dets[b].rxid) for a, b in task_pairs(dets, match))
    mobile = [m for m, match in enumerate(matches) if dets[match[0]].txid not in beacon_pos]
    uncovered = [m for m in mobile
                 if any((dets[a].rxid, dets[b].rxid) not in covered for a, b in task_pairs(dets, matches[m]))]
    for m in uncovered:
        assert all((dets[a].rxid, dets[b].rxid) not in covered for a, b in task_pairs(dets, matches[m])), name
    run = [m for m in range(len(matches)) if m not in set(uncovered)]
    listener = Listener(model, deg)
    tdoa_est.stat_tools = types.SimpleNamespace(is_outlier=listener.outlier)
    tdoa_est.bisect_left, tdoa_est.np = listener.bisect_left, listener.numpy
    try:
        groups, failures = tdoa_est.estimate_tdoas(dets, [matches[m] for m in run], window, beacon_pos, rx_pos, FS,
                                                   model_builder=listener.builder,
                                                   model_params={"deg": deg} if model == "weighted_poly" else None)
    finally:
        tdoa_est.bisect_left, tdoa_est.np = listener.python_bisect, np
    groups = [g._replace(group_id=run[g.group_id]) for g in groups]
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
    produced = [t for t in tasks if t.get("ref") is not None and abs(t["ref"]) < tdoa_est.MAX_TDOA]
    table = tdoa_est.groups_to_matrix(groups)
    assert len(produced) == len(table) and all(t["ref"] == v for t, v in zip(produced, table["tdoa"])), name
    assert len(table) + len(failures) == len(tasks) and np.all(np.isfinite(table["tdoa"]))
    extra = {}
    if model == "weighted_poly":
        assert all(t["distinct"] >= deg + 1 for t in tasks if "distinct" in t), name
        exact = np.array([t["exact"] for t in produced], float)
        extra = {"exact_tdoa": exact, "ref_err_max": float(np.max(np.abs(table["tdoa"] - exact))) if len(table) else 0.0}
    rx_ids, beacon_ids = sorted(rx_pos), sorted(beacon_pos)
    sizes = np.cumsum([0] + [len(g.tdoas) for g in groups])
    path = os.path.join(OUT, "%s_%s%s.npz" % (name, model, suffix))
    np.savez_compressed(
        path, model=model,
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
        det0=table["det0_idx"].astype(np.int64), det1=table["det1_idx"].astype(np.int64),
        failures=np.array(failures, np.int64).reshape(-1, 2), n_window=np.array([t["n_window"] for t in tasks], np.int64),
        n_kept=np.array([t["n_kept"] for t in tasks], np.int64), uncovered_matches=np.array(uncovered, np.int64), **extra)
    assert os.path.getsize(path) < 100 * 1024, path
    seen = met(model, tasks)
    print("%-15s %-13s deg %d: %d TDOAs in %d groups, %d failures%s; %s" % (
        name, model, deg, len(table), len(groups), len(failures),
        ", ref_err_max %.3g s" % extra["ref_err_max"] if extra else "", ", ".join(sorted(seen))))
    return seen


def scenes():
    """make_golden_tdoa.main()'s four scenes: the same calls on the same generator in the same order."""
    rng = np.random.default_rng(20261018)
    all_rx = [0, 1, 2]
    yield ("tdoa_realistic",) + scene(
        rng, {0: all_rx, 1: all_rx, 2: all_rx, 3: all_rx},
        {0: times(rng, 0, 60, 1.0), 1: times(rng, 0, 60, 1.0)}, {2: times(rng, 0, 60, 1.0), 3: times(rng, 0, 60, 1.0)})
    yield ("tdoa_failures",) + scene(
        rng, {0: all_rx, 2: all_rx, 3: all_rx, 4: [2, 3]},
        {0: times(rng, 0, 400, 9.0, 0.6)}, {2: times(rng, 0, 400, 4.0), 3: times(rng, 0, 400, 16.0), 4: times(rng, 0, 400, 40.0)},
        outlier_prob=0.12, bogus_mobile=3)
    yield ("tdoa_ties",) + scene(
        rng, {0: all_rx, 1: all_rx, 2: all_rx, 3: all_rx},
        {0: times(rng, 0, 50, 1.0), 1: times(rng, 14, 50, 5.0)}, {2: times(rng, 0, 50, 1.0), 3: times(rng, 0, 50, 2.0)},
        outlier_prob=0.0, grid=1.0)
    dense = []
    t = 0.0
    while t < 60.0:
        dense.append(t)
        t += 1.0 / (1.5 + 7.5 * t / 60.0)
    yield ("tdoa_wide",) + scene(rng, {0: [0, 1], 2: [0, 1]}, {0: dense}, {2: times(rng, 0, 60, 0.45)})


def main():
    os.makedirs(OUT, exist_ok=True)
    seen = {model: set() for model in REQUIRED}
    for name, rows, matches, rx_pos, beacon_pos in scenes():
        for model in REQUIRED:
            seen[model] |= save(name, model, rows, matches, rx_pos, beacon_pos, 8.0)
        if name == "tdoa_realistic":
            seen["weighted_poly"] |= save(name, "weighted_poly", rows, matches, rx_pos, beacon_pos, 8.0, deg=1, suffix="_deg1")
    for model, need in REQUIRED.items():
        assert need <= seen[model], (model, sorted(need - seen[model]))


if __name__ == "__main__":
    main()
