"""The pos3 fixtures (tests/golden/pos3/*.npz, made by tests/golden/make_golden_pos3.py) for the host and the GPU
tests: loading, how each set is solved, and the one comparison every path is held to."""
import os

import numpy as np

import pos_golden

ROOT = pos_golden.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "pos3")
SETS_H = ("h_ring4", "h_ring6")
SETS_Z = ("z_tall6", "z_tall5", "z_ring6", "z_four", "z_box")
SETS = SETS_H + SETS_Z
_cache = {}

rx_pos, dense, groups, snr_bound = pos_golden.rx_pos, pos_golden.dense, pos_golden.groups, pos_golden.snr_bound


def load(name):
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, name + ".npz")) as g:
            _cache[name] = {key: g[key] for key in g.files}
        for value in _cache[name].values():
            value.setflags(write=False)
    return _cache[name]


def free_z(g):
    return bool(g["free_z"])


def mode_args(g, by_tx=False):
    """The keyword arguments of `pos3_columns` / `solve` that say how the set is solved; `by_tx`: the height as the
    {tx: height} dict where the set has one."""
    if free_z(g):
        return {"free_z": True, "z0": float(g["z0"]), "z_range": tuple(g["z_range"].tolist()) if len(g["z_range"]) else None}
    if by_tx and len(g["tx_height"]):
        return {"height": {int(tx): float(h) for tx, h in g["tx_height"]}}
    return {"height": g["group_h"]}


def failure_lines(g):
    return ["Failed to estimate group #%d: Underdetermined" % i for i in g["group_id"][~g["solved"]]]


def check_positions(g, group_id, timestamp, tx, pos, dop, snr, hdop=None, vdop=None, slack=0.0):
    """The records of the SOLVED groups, in order, against the fixture.  Exact: which groups, their order, group_id,
    timestamp, tx.  pos (x, y with the height known; x, y, z with z free) within ref_err_max of the EXACT minimiser
    (as close to it as SciPy is), hence within 2 ref_err_max of SciPy's; dop, and hdop / vdop where given, within
    dop_ref_err_max (relative) of the exact ones; snr within the summation bound.  `slack` [m] is added to
    ref_err_max where the caller's inputs are not the fixture's to the bit (the caller derives it).
    -> (max |x - x_star|, max relative dop error)."""
    ok = g["solved"]
    axes = 3 if free_z(g) else 2
    np.testing.assert_array_equal(group_id, g["group_id"][ok])
    np.testing.assert_array_equal(timestamp, g["group_timestamp"][ok])
    np.testing.assert_array_equal(tx, g["group_tx"][ok])
    pos = np.asarray(pos, dtype=np.float64).reshape(int(ok.sum()), -1)[:, :axes]
    bound, dop_bound = float(g["ref_err_max"]) + slack, float(g["dop_ref_err_max"])
    err = float(np.max(np.abs(pos - g["x_star"][ok][:, :axes])))
    dop_err = 0.0
    for got, key in ((dop, "dop_star"), (hdop, "hdop_star"), (vdop, "vdop_star")):
        if got is None or (key == "vdop_star" and not free_z(g)):
            continue
        star = g[key][ok]
        dop_err = max(dop_err, float(np.max(np.abs(np.asarray(got, dtype=np.float64) - star) / star)))
    print("max |x - x_star| = %.3g m (SciPy: %.3g m); max relative dop error = %.3g (SciPy: %.3g)" % (err, bound, dop_err, dop_bound))
    assert err <= bound
    assert np.all(np.abs(pos - g["x_ref"][ok][:, :axes]) <= 2 * bound)
    assert dop_err <= dop_bound
    assert np.all(np.abs(np.asarray(snr, dtype=np.float64) - g["snr_ref"][ok]) <= snr_bound(g)[ok])
    return err, dop_err
