#!/usr/bin/env python3
"""Golden fixtures for thr_reldist, made by RUNNING THE REFERENCE's scripts/reldist_nearest.py: its `find_nearest`,
`reldist_nearest`, `reldist_linpol` and `is_outlier`, and nothing else of it (its `reldist` is one recording's
geometry, plots and statsmodels' lowess, which the build container does not have).  Build container only:

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_reldist.py

The script is loaded by path.  Before that, an empty stand-in for statsmodels.nonparametric.smoothers_lowess is
registered (its `lowess` raises) and matplotlib's Agg backend is selected.

tests/golden/reldist/<scene>.npz holds the seven detection columns, the matches as CSR, the beacon list, the
geometry table (the script's three constants, in samples) and, per (mobile, beacon, rx0, rx1) cell with the tag
m<mobile>_b<beacon>_<rx0>_<rx1>_:
    nearest                 find_nearest(beacon soa at rx0, mobile soa at rx0)
    raw_nearest, raw_linpol reldist_nearest / reldist_linpol on the [rows][2] SOA matrices of the two-detection
                            matches of that pair (raw_linpol is absent where the script raises or wraps: a row
                            outside the beacon's span that is not the last one)
    mask1_<method>, mask2_<method>, mask3
                            is_outlier of x, of the speeds, of the doppler.  x, the speeds and the doppler are the
                            header's formulas in NumPy (tests/reldist_ref.py; its raw equals the script's wherever
                            the script defines one, which tests/test_reldist_host.py asserts); the masks are the
                            script's.
Scenes (a few hundred rows each):
    a  two receivers, a beacon every 4th transmission, the mobile strictly inside the beacon's span
    b  the same, the mobile's last row after the last beacon row (the script's one defined edge)
    c  integer SOAs: mobile rows exactly midway between two beacon rows, and exactly on a beacon row
    d  four receivers with missing detections, reduced pair by pair
    e  injected outliers in the mobile's SOAs and carriers: no mask is empty
    f  more than half of x equal: MAD = 0
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = os.environ.get("THRIFTY_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))

if not hasattr(np, "bool"):         # the reference spells a dtype np.bool
    np.bool = bool


def load_script():
    def lowess(*args, **kwargs):
        raise RuntimeError("statsmodels is not installed: the stand-in's lowess must not be called")
    for name in ("statsmodels", "statsmodels.nonparametric", "statsmodels.nonparametric.smoothers_lowess"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["statsmodels.nonparametric.smoothers_lowess"].lowess = lowess
    import matplotlib
    matplotlib.use("Agg")
    spec = importlib.util.spec_from_file_location("reldist_nearest", os.path.join(REF, "scripts", "reldist_nearest.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


SCRIPT = load_script()

import reldist_ref as R  # noqa: E402
import reldist_scenes as SC  # noqa: E402

S2M = R.LIGHT / SC.RATE
GEOMETRY = tuple(v / S2M for v in SC.SCRIPT_METRES)
TWO = {0: 0.0, 1: SC.SCRIPT_METRES[1]}


def scene_a():
    return SC.synth(SC.interleaved(397), TWO, 21, {0: SC.SCRIPT_METRES[1] - SC.SCRIPT_METRES[2]})      # ends with a beacon row


def scene_b():
    return SC.synth(SC.interleaved(398), TWO, 21, {0: SC.SCRIPT_METRES[1] - SC.SCRIPT_METRES[2]})      # one mobile row after it


def scene_c():
    txs = []
    for i in range(60):
        txs.append((0, {0: (1000.0 * i, 1000.0 + i, 300.0, 0.25), 1: (1000.0 * i + 37.0 + (i % 5), 1000.0 + i, 300.0, 0.5)}))
        if i == 59:
            break
        where = (500.0, 0.0, 250.0, 1000.0 - 500.0, 750.0)[i % 5] if i else 500.0     # midway, ON the row, off-centre
        soa0 = 1000.0 * i + where
        txs.append((1, {0: (soa0, 1000.3 + i, 310.0, 0.125 * (i % 8)), 1: (soa0 + 90.0 + (i * 7) % 11, 1000.3 + i, 310.0, 0.5)}))
    return txs


def scene_d():
    rx = {0: 0.0, 1: SC.SCRIPT_METRES[1], 2: 3000.0, 5: 12000.0}
    return SC.synth(SC.interleaved(330, 3, mobiles=(1, 2), beacons=(0, 7)), rx, 24, {0: 4000.0, 7: 7000.0}, drop=0.15)


def scene_e():
    txs = scene_a()
    rng = np.random.default_rng(25)
    mobile = [i for i, (tx, _) in enumerate(txs) if tx == 1]
    for i in rng.choice(mobile[2:-2], 14, replace=False):
        soa, ts, cbin, coff = txs[i][1][1]
        txs[i][1][1] = (soa + float(rng.choice([-1, 1])) * float(rng.uniform(40, 400)), ts, cbin + float(rng.integers(3, 9)), coff)
    return txs


def scene_f():
    txs = []
    for i in range(50):
        txs.append((0, {0: (2000.0 * i, 1000.0 + 2 * i, 300.0, 0.25), 1: (2000.0 * i + 64.0, 1000.0 + 2 * i, 300.0, 0.5)}))
        for j in range(3):
            soa0 = 2000.0 * i + 400.0 + 300.0 * j
            extra = float((i * 3 + j) % 7) if (i * 3 + j) % 3 == 0 else 0.0       # two thirds of the rows: the same x
            txs.append((1, {0: (soa0, 1000.4 + 2 * i + 0.5 * j, 310.0, 0.25),
                            1: (soa0 + 128.0 + extra, 1000.4 + 2 * i + 0.5 * j, 310.0, 0.25 if (i + j) % 4 else 0.75)}))
    return txs[:-2]


def record(name, txs, beacons):
    cols, ptr, idx = SC.assemble(txs)
    receivers = sorted(set(cols["rxid"].tolist()))
    geometry = [(b, r0, r1) + GEOMETRY for b in beacons for r0 in receivers for r1 in receivers if r0 < r1]
    out = dict(cols, match_ptr=ptr, match_idx=idx, beacons=np.array(beacons, np.int32), geometry=np.array(geometry, np.float64))
    groups = R.groups_of(cols, ptr, idx)
    refs = {method: R.reldist_ref(cols, ptr, idx, beacons, method=method, geometry=geometry)[1] for method in ("nearest", "linpol")}
    keys = [tuple(k) for k in refs["linpol"]["cell_key"].tolist()]
    for ci, (tx, b, r0, r1) in enumerate(keys):
        tag = "m%d_b%d_%d_%d_" % (tx, b, r0, r1)
        tx_soa = cols["soa"][np.array(groups[(tx, r0, r1)])[:, :2]]
        beacon_soa = cols["soa"][np.array(groups[(b, r0, r1)])[:, :2]]
        out[tag + "nearest"] = SCRIPT.find_nearest(beacon_soa[:, 0], tx_soa[:, 0]).astype(np.int64)
        out[tag + "raw_nearest"] = SCRIPT.reldist_nearest(tx_soa, beacon_soa)
        hi = np.searchsorted(beacon_soa[:, 0], tx_soa[:, 0])
        inside = (hi >= 1) & (hi <= len(beacon_soa) - 1)
        if np.all(inside[:-1]) and (inside[-1] or hi[-1] == len(beacon_soa)):
            with np.errstate(all="ignore"):
                out[tag + "raw_linpol"] = SCRIPT.reldist_linpol(tx_soa, beacon_soa)
        for method, ref in refs.items():
            a, e = ref["cell_ptr"][ci:ci + 2]
            sa, se = ref["speed_ptr"][ci:ci + 2]
            with np.errstate(all="ignore"):
                out[tag + "mask1_" + method] = SCRIPT.is_outlier(ref["x"][a:e])
                out[tag + "mask2_" + method] = SCRIPT.is_outlier(ref["speed"][sa:se])
                out[tag + "mask3"] = SCRIPT.is_outlier(ref["dop"][a:e])
    os.makedirs(SC.GOLDEN, exist_ok=True)
    np.savez_compressed(os.path.join(SC.GOLDEN, name + ".npz"), **out)
    masks = [int(np.sum(v)) for k, v in sorted(out.items()) if "_mask" in k]
    print("%s: %d detections, %d matches, %d cells, %d with linpol; outliers %s" % (
        name, len(cols["soa"]), len(ptr) - 1, len(keys), sum(k.endswith("raw_linpol") for k in out), masks[:12]))


if __name__ == "__main__":
    record("a", scene_a(), [0])
    record("b", scene_b(), [0])
    record("c", scene_c(), [0])
    record("d", scene_d(), [0, 7])
    record("e", scene_e(), [0])
    record("f", scene_f(), [0])
