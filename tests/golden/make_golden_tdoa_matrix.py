#!/usr/bin/env python3
"""Golden fixtures for the per-beacon TDOA matrices, made by RUNNING THE REFERENCE's scripts/tdoa_matrix.py
(`calculate_tdoas`, cell by cell) on synthetic detections and matches.  Needs a checkout of the reference;
THRIFTY_REFERENCE names it:

    THRIFTY_REFERENCE=<checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tdoa_matrix.py

The script is imported by path as it is.  `tabulate` and `matplotlib` get empty stand-in modules where they are
missing (its tables and plots are not called).  The Python-2 shims of thrifty/tdoa_est.py are those of
make_golden_tdoa.py (and make_golden_tdoa_models.py's `sorted` for the nearest model), which are imported for them.
While the script's `calculate_tdoas` runs, `tdoa_est.estimate_tdoas` is a wrapper that hands the reference's own
function a LISTENING model builder (make_golden_tdoa.Listener: n_window and n_kept per task, and the exact
least-squares TDOA by fractions.Fraction; make_golden_tdoa_models.Listener around `build_model_nearest` for
tdmat_nearest) and notes the groups it returns, i.e. the rows before the script's own mask.

Each file under tests/golden/tdoa_matrix/ holds the detection columns, the matches as CSR, the lists (receivers,
beacons as passed, model, deg; window 4 and sample rate 2.4e6 are the script's constants) and the reference's answer
in the layout of thr_tdoamatrix's outputs: cells in ascending (rx0, rx1, beacon, tx) order with flags and counts, tasks
in match order with det, match, timestamp, status, tdoa (the reference's), exact_tdoa, snr, model_quality, n_window,
n_kept and outlier (the rows the script's mask dropped); per cell ref_std, ref_mean (np.std, np.mean of the kept
TDOAs times 2.997e8, unrounded) and the script's printed table_std, table_mean, table_count, with firm_std / firm_mean:
the unrounded value is farther than 2 * ref_err_max * 2.997e8 from a rounding boundary.  ref_err_max = max |tdoa - exact|.

For the three polynomial sets a file is only written when, for every cell of more than one TDOA and every row,
MAD > e and |z - 3.5| > (1.349 + z) e / (MAD - e) with e = 2 ref_err_max: a TDOA that moves by the permitted e cannot
change the mask.  tdmat_realistic also needs nine tenths of its table entries firm.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_tdoa as base  # noqa: E402  (puts THRIFTY_REFERENCE on the path and the shims into tdoa_est)
import make_golden_tdoa_models as models  # noqa: E402
from make_golden_tdoa import FS, objects, tdoa_est  # noqa: E402

OUT = os.path.join(HERE, "tdoa_matrix")
C = tdoa_est.SPEED_OF_LIGHT
OK, NO_MODEL, OUT_OF_RANGE, SKIPPED = 0, 1, 2, 3
WINDOW = 4.0


def load_script():
    for name in ("tabulate", "matplotlib", "matplotlib.pyplot"):
        try:
            importlib.import_module(name)
        except ImportError:
            stand_in = types.ModuleType(name)
            stand_in.tabulate = None
            sys.modules[name] = stand_in
    if not hasattr(sys.modules["matplotlib"], "pyplot"):
        sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    path = os.path.join(os.environ["THRIFTY_REFERENCE"], "scripts", "tdoa_matrix.py")
    spec = importlib.util.spec_from_file_location("reference_tdoa_matrix", path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    assert module.WINDOW_SIZE == WINDOW and module.tdoa_est is tdoa_est
    return module


SCRIPT = load_script()
from thrifty import matchmaker  # noqa: E402


def scene(rng, events, n_rx, noise=0.05, grid=False, grid_errors=None, bogus=None):
    """events: (t, tx, receivers[, copy]) -- `copy`: the event whose SoAs this one repeats.  Receiver clocks differ by
    a few thousand samples and some ppm (none on the grid); SoAs stay below 2e8 so that the reference's raw
    Vandermonde keeps its digits."""
    rx_pos = {r: rng.uniform(-1500, 1500, 2) for r in range(n_rx)}
    tx_pos = {tx: rng.uniform(-1200, 1200, 2) for tx in sorted(set(e[1] for e in events))}
    offset = {r: float(np.round(rng.uniform(1e3, 9e3))) for r in range(n_rx)}
    rate = {r: FS * (1 + (0 if grid else rng.uniform(-30, 30) * 1e-6)) for r in range(n_rx)}
    skew = {r: float(rng.uniform(-0.03, 0.03)) for r in range(n_rx)}
    t_min = min(e[0] for e in events)
    rows, soas = [], {}
    for e, event in enumerate(events):
        t, tx, heard = event[:3]
        for r in heard:
            delay = float(np.linalg.norm(rx_pos[r] - tx_pos[tx])) / C
            if grid:
                soa = offset[r] + np.round((t - t_min) * FS) + np.round(delay * FS)
                if grid_errors and tx in grid_errors and rng.random() < grid_errors[tx]:
                    soa += float(rng.choice([1, -1, 2, -2]))
            else:
                soa = offset[r] + (t - t_min + delay) * rate[r] + rng.normal(0, noise)
            if len(event) > 3:
                soa = soas[(event[3], r)]
            if bogus is not None and tx == bogus and r == max(heard):
                soa += 600.0        # a false peak: |tdoa| beyond MAX_TDOA
            soas[(e, r)] = soa
            stamp = round(1.7e9 + t + delay + skew[r], 6)
            rows.append((float(stamp), r, tx, float(soa), float(rng.uniform(50, 200)), float(rng.uniform(1, 3)), e))
    order = sorted(range(len(rows)), key=lambda i: rows[i][0])
    rows = [rows[i] for i in order]
    by_event = {}
    for i, row in enumerate(rows):
        by_event.setdefault(row[6], []).append(i)
    matches = sorted((m for m in by_event.values() if len(m) >= 2), key=lambda m: m[0])
    return rows, matches


class Heard(object):
    """estimate_tdoas while the script's function runs: the reference's, with the listening builder."""

    def __init__(self, model):
        self.model, self.real, self.groups, self.listener = model, tdoa_est.estimate_tdoas, None, None

    def __call__(self, **kwargs):
        self.listener = base.Listener(2) if self.model == "poly" else models.Listener(self.model, 2)
        tdoa_est.stat_tools = types.SimpleNamespace(is_outlier=self.listener.outlier)
        if self.model != "poly":
            tdoa_est.bisect_left, tdoa_est.np = self.listener.bisect_left, self.listener.numpy
        try:
            self.groups, failures = self.real(model_builder=self.listener.builder, **kwargs)
        finally:
            if self.model != "poly":
                tdoa_est.bisect_left, tdoa_est.np = self.listener.python_bisect, np
        return self.groups, failures


def run_cell(dets, matches, rx0, rx1, b, t, model):
    """The script's calculate_tdoas on one cell -> (matrix or None, tasks of the listener, rows before the mask)."""
    heard = Heard(model)
    tdoa_est.estimate_tdoas = heard
    try:
        matrix = SCRIPT.calculate_tdoas(dets, matches, rx0, rx1, b, t)
    finally:
        tdoa_est.estimate_tdoas = heard.real
    if matrix is None:
        return None, [], []
    before = tdoa_est.groups_to_matrix(heard.groups)
    return matrix, heard.listener.tasks, before


def firm(value, extra):
    """value is farther than extra from every boundary (k + 1/2) / 10 of np.around(value, 1)."""
    frac = (value * 10.0) % 1.0
    return bool(abs(frac - 0.5) / 10.0 > extra)


def save(name, rows, matches, beacons, model="poly", require=None, firm_share=None):
    dets = objects(rows)
    receivers = sorted(set(r[1] for r in rows))
    txids = sorted(set(dets[m[0]].txid for m in matches))
    cells, tasks_all = [], []
    for i0, rx0 in enumerate(receivers):
        for rx1 in receivers[i0 + 1:]:
            for b in sorted(beacons):
                for t in txids:
                    mine = matchmaker.extract_match_matrix(dets, matches, [rx0, rx1], [t])
                    if t == b or not mine:
                        continue
                    theirs = matchmaker.extract_match_matrix(dets, matches, [rx0, rx1], [b])
                    matrix, heard, before = run_cell(dets, matches, rx0, rx1, b, t, model)
                    assert (matrix is None) == (len(mine) < 3 or len(theirs) < 3), (name, rx0, rx1, b, t)
                    task_match = [next(m for m, match in enumerate(matches) if row[0] in match) for row in mine]
                    cell = {"key": (rx0, rx1, b, t), "flag": int(matrix is None), "nb": len(theirs), "tasks": []}
                    assert matrix is None or len(heard) == len(mine)
                    kept_dets = set() if matrix is None else set(zip(matrix["det0_idx"].tolist(), matrix["det1_idx"].tolist()))
                    rows_before = {} if matrix is None else {(int(r["det0_idx"]), int(r["det1_idx"])): r for r in before}
                    for k, (d0, d1) in enumerate(mine):
                        task = {"det": (d0, d1), "match": task_match[k], "timestamp": dets[d0].timestamp, "status": SKIPPED,
                                "tdoa": np.nan, "exact": np.nan, "mq": np.nan, "n_window": 0, "n_kept": 0, "outlier": 0,
                                "snr": ((dets[d0].corr_info.energy / dets[d0].corr_info.noise) ** 2 +
                                        (dets[d1].corr_info.energy / dets[d1].corr_info.noise) ** 2) / 2}
                        if matrix is not None:
                            h = heard[k]
                            task["n_window"], task["n_kept"] = h["n_window"], h["n_kept"]
                            if "ref" not in h or h["ref"] is None:
                                task["status"] = NO_MODEL
                            elif abs(h["ref"]) >= tdoa_est.MAX_TDOA:
                                task["status"] = OUT_OF_RANGE
                            else:
                                row = rows_before[(d0, d1)]
                                assert row["tdoa"] == h["ref"] and row["timestamp"] == dets[d0].timestamp
                                task.update(status=OK, tdoa=float(h["ref"]), exact=float(h.get("exact", h["ref"])),
                                            mq=float(row["model_quality"]), outlier=int((d0, d1) not in kept_dets))
                                assert row["snr"] == task["snr"]
                        cell["tasks"].append(task)
                    assert len(rows_before) == sum(t_["status"] == OK for t_ in cell["tasks"])
                    column = matrix["tdoa"] if matrix is not None else np.zeros(0)
                    cell["ref_std"] = float(np.std(column) * C) if len(column) else np.nan
                    cell["ref_mean"] = float(np.mean(column) * C) if len(column) else np.nan
                    # the script's printed numbers
                    cell["table"] = (float(np.around(np.std(column) * C, 1)) if len(column) > 0 else 0.0,
                                     float(np.around(np.mean(column) * C, 1)) if len(column) > 0 else 0.0, len(column))
                    cells.append(cell)
                    tasks_all += cell["tasks"]
    ok = [t for t in tasks_all if t["status"] == OK]
    err = max([abs(t["tdoa"] - t["exact"]) for t in ok] + [0.0])
    extra = 2 * err * C
    for cell in cells:
        cell["firm"] = (cell["table"][2] == 0 or firm(cell["ref_std"], extra), cell["table"][2] == 0 or firm(cell["ref_mean"], extra))
    if model == "poly":         # a TDOA that moves by e cannot change a cell's mask
        e = 2 * err
        for cell in cells:
            v = np.array([t["tdoa"] for t in cell["tasks"] if t["status"] == OK])
            if len(v) > 1:
                diff = np.abs(v - np.median(v))
                mad = np.median(diff)
                assert mad > e, (name, cell["key"], mad, e)
                z = 0.6745 * diff / mad
                assert np.all(np.abs(z - 3.5) > (1.349 + z) * e / (mad - e)), (name, cell["key"])
    else:
        assert err == 0.0
    share = np.mean([f for cell in cells for f in cell["firm"]])
    if firm_share is not None:
        assert share >= firm_share, (name, share)
    if require:
        require(cells, tasks_all)
    os.makedirs(OUT, exist_ok=True)
    task = lambda key, kind: np.array([t[key] for t in tasks_all], kind)  # noqa: E731
    np.savez_compressed(
        os.path.join(OUT, name + ".npz"),
        rxid=np.array([r[1] for r in rows], np.int32), txid=np.array([r[2] for r in rows], np.int32),
        timestamp=np.array([r[0] for r in rows], float), soa=np.array([r[3] for r in rows], float),
        energy=np.array([r[4] for r in rows], float), noise=np.array([r[5] for r in rows], float),
        match_ptr=np.cumsum([0] + [len(m) for m in matches]).astype(np.int64),
        match_idx=np.array([i for m in matches for i in m], np.int64),
        receivers=np.array(receivers, np.int32), beacons=np.array(beacons, np.int32), model=model, deg=2,
        window=WINDOW, sample_rate=FS,
        cell_key=np.array([c["key"] for c in cells], np.int32).reshape(-1, 4),
        cell_ptr=np.cumsum([0] + [len(c["tasks"]) for c in cells]).astype(np.int64),
        cell_flags=np.array([c["flag"] for c in cells], np.int32),
        cell_counts=np.array([(c["nb"], len(c["tasks"]), sum(t["status"] == OK for t in c["tasks"]),
                               0 if c["flag"] else sum(t["status"] != OK for t in c["tasks"]), c["table"][2]) for c in cells],
                             np.int64).reshape(-1, 5),
        ref_std=np.array([c["ref_std"] for c in cells]), ref_mean=np.array([c["ref_mean"] for c in cells]),
        table_std=np.array([c["table"][0] for c in cells]), table_mean=np.array([c["table"][1] for c in cells]),
        table_count=np.array([c["table"][2] for c in cells], np.int64),
        firm_std=np.array([c["firm"][0] for c in cells], bool), firm_mean=np.array([c["firm"][1] for c in cells], bool),
        task_det=task("det", np.int64).reshape(-1, 2), task_match=task("match", np.int64), task_timestamp=task("timestamp", float),
        status=task("status", np.int32), tdoa=task("tdoa", float), exact_tdoa=task("exact", float), snr=task("snr", float),
        model_quality=task("mq", float), n_window=task("n_window", np.int32), n_kept=task("n_kept", np.int32),
        outlier=task("outlier", np.uint8), ref_err_max=float(err))
    windows = [t["n_window"] for t in tasks_all if t["status"] != SKIPPED]
    print("%-16s %d detections, %d matches: %d cells, %d tasks, %d TDOAs (%d masked), windows %d..%d, ref_err_max %.3g s, "
          "firm table entries %.3f" % (name, len(rows), len(matches), len(cells), len(tasks_all), len(ok),
                                       sum(t["outlier"] for t in tasks_all), min(windows), max(windows), err, share))


def periodic(rng, start, stop, period, jitter=0.3):
    out, t = [], start + float(rng.uniform(0, period))
    while t < stop:
        out.append(t)
        t += period * float(rng.uniform(1 - jitter, 1 + jitter))
    return out


def main():
    rng = np.random.default_rng(20261020)

    # ---- realistic: 4 receivers, 2 beacons (each measured against the other), 3 mobiles, now and then a receiver missing
    events = []
    for tx in range(5):
        for t in periodic(rng, 0, 40, 1.0):
            heard = [r for r in range(4) if rng.random() > 0.1]
            events.append((t, tx, heard))
    events.sort()

    def realistic_required(cells, tasks):
        assert any(c["key"][2:] == (0, 1) for c in cells) and any(c["key"][2:] == (1, 0) for c in cells)
        assert 150 <= len(set(t["match"] for t in tasks)) and any(t["outlier"] for t in tasks)

    rows, matches = scene(rng, events, 4)
    save("tdmat_realistic", rows, matches, [0, 1], require=realistic_required, firm_share=0.9)

    # ---- edges: beacons 1 and 5 (passed unsorted); see the requirements below
    all3 = [0, 1, 2]
    events = [(float(t), 1, all3) for t in range(0, 21)]
    events.append((6.4, 1, all3, 6))                                    # the SoAs of the transmission at t = 6 again
    events += [(2.2, 5, all3), (3.2, 5, all3), (4.2, 5, [0, 2])]        # lists of 2 rows at (0, 1), (1, 2), of 3 at (0, 2)
    events += [(8.3, 7, all3), (9.3, 7, all3), (10.3, 7, [0, 2])]       # the same for a target
    events += [(40.0 + k, 8, all3) for k in range(4)]                   # every task fails: no beacon near
    events += [(10.6, 9, all3), (50.5, 9, all3), (60.5, 9, all3)]       # exactly one TDOA
    events += [(11.6, 10, all3), (12.6, 10, all3), (55.5, 10, all3)]    # exactly two
    events += [(-3.5, 11, all3), (-2.5, 11, all3), (-1.5, 11, all3), (5.5, 11, all3), (6.7, 11, all3)]  # windows of 1, 2, 3
    events += [(7.5 + k, 12, all3) for k in range(4)]                   # out of range at its last receiver
    events.sort(key=lambda e: e[0])
    fixed = {6.4: 6.0}
    events = [e[:3] + (next(i for i, o in enumerate(events) if o[0] == fixed[e[0]] and o[1] == e[1]),) if len(e) > 3 else e
              for e in events]

    def edges_required(cells, tasks):
        by_key = {c["key"]: c for c in cells}
        assert by_key[(0, 1, 5, 1)]["flag"] and by_key[(0, 1, 5, 1)]["nb"] == 2          # beacon list of 2
        assert not by_key[(0, 2, 5, 1)]["flag"] and by_key[(0, 2, 5, 1)]["nb"] == 3      # of 3
        assert by_key[(0, 1, 1, 7)]["flag"] and len(by_key[(0, 1, 1, 7)]["tasks"]) == 2  # target list of 2
        assert not by_key[(0, 2, 1, 7)]["flag"] and len(by_key[(0, 2, 1, 7)]["tasks"]) == 3
        assert all(t["status"] == NO_MODEL and t["n_window"] == 0 for t in by_key[(0, 1, 1, 8)]["tasks"])
        assert sum(t["status"] == OK for t in by_key[(0, 1, 1, 9)]["tasks"]) == 1
        assert sum(t["status"] == OK for t in by_key[(0, 1, 1, 10)]["tasks"]) == 2
        assert {1, 2, 3} <= set(t["n_window"] for t in by_key[(0, 1, 1, 11)]["tasks"])   # (0: transmitter 8)
        assert any(t["status"] == OUT_OF_RANGE for t in by_key[(0, 2, 1, 12)]["tasks"])
        assert any(t["status"] == OK and t["n_kept"] >= 4 and abs(t["timestamp"] - 1.7e9 - 6.7) < 0.5 for t in by_key[(0, 1, 1, 11)]["tasks"])

    rows, matches = scene(rng, events, 3, bogus=12)
    save("tdmat_edges", rows, matches, [5, 1], require=edges_required)

    # ---- wide: one dense beacon, windows of 64, 65, 256 and 257 pairs, six tasks
    d1, d2 = 8.0 / 64.5, 8.0 / 256.5
    events = [(k * d1, 0, [0, 1]) for k in range(int(20 / d1))] + [(30.0 + k * d2, 0, [0, 1]) for k in range(int(20 / d2))]
    for k, f in ((40, 0.25), (41, 0.75), (50, 0.25)):
        events.append(((k + f) * d1 + 4.0, 2, [0, 1]))
    for k, f in ((200, 0.25), (201, 0.75), (220, 0.25)):
        events.append((30.0 + (k + f) * d2 + 4.0, 2, [0, 1]))
    events.sort()

    def wide_required(cells, tasks):
        assert {64, 65, 256, 257} <= set(t["n_window"] for t in tasks) and len(tasks) == 6, sorted(set(t["n_window"] for t in tasks))

    rows, matches = scene(rng, events, 2)
    save("tdmat_wide", rows, matches, [0], require=wide_required)

    # ---- nearest: SoAs on a grid, so that TDOAs tie; the reference's bits
    events = []
    for tx, period in ((0, 1.0), (2, 1.0), (3, 1.0), (4, 1.0)):
        events += [(t, tx, all3) for t in periodic(rng, 0, 30, period)]
    events.sort()

    def nearest_required(cells, tasks):
        kinds = set()
        for c in cells:
            v = np.array([t["tdoa"] for t in c["tasks"] if t["status"] == OK])
            if len(v) > 1:
                diff = np.abs(v - np.median(v))
                kinds.add("mad" if np.median(diff) != 0 else "off" if np.any(diff != 0) else "flat")
                if np.median(diff) == 0 and np.any(diff != 0):
                    assert sum(t["outlier"] for t in c["tasks"]) == int(np.sum(diff != 0))
        assert kinds == {"mad", "off", "flat"}, kinds

    rows, matches = scene(rng, events, 3, grid=True, grid_errors={3: 0.08, 4: 0.6})
    save("tdmat_nearest", rows, matches, [0], model="nearest", require=nearest_required)


if __name__ == "__main__":
    main()
