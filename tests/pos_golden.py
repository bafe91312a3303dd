"""The pos fixtures (tests/golden/pos/*.npz, made by tests/golden/make_golden_pos.py) for the host and
the GPU tests: loading, TdoaGroup objects, and the one comparison every path is held to."""
import os

import numpy as np

from thrifty_amd import tdoa_est

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pos")
SETS_2D = ("pos_ring4", "pos_ring6", "pos_ring8", "pos_three", "pos_outside")
SETS_1D = ("pos_line", "pos_line_rising")       # the two coordinate orders of the same two receivers
SETS = SETS_2D + SETS_1D
_cache = {}


def load(name):
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, name + ".npz")) as g:
            _cache[name] = {key: g[key] for key in g.files}
        for value in _cache[name].values():
            value.setflags(write=False)
    return _cache[name]


def rx_pos(g):
    """The receivers as the dict `solve` takes, in the fixture's order."""
    return {int(r): np.array(xyz) for r, xyz in zip(g["rx_ids"], g["rx_xyz"])}


def dense(g, column):
    index = {int(r): k for k, r in enumerate(g["rx_ids"])}
    return np.array([index[int(v)] for v in column], dtype=np.int32)


def groups(g):
    rows = np.zeros(len(g["tdoa"]), dtype=tdoa_est.TDOA_DTYPE)
    for name in ("rx0", "rx1", "tdoa", "snr"):
        rows[name] = g[name]
    rows["model_quality"], rows["det1_idx"] = 1.0, 1
    ptr = g["group_ptr"].tolist()
    return [tdoa_est.TdoaGroup(int(i), float(t), int(tx), rows[a:b]) for i, t, tx, a, b in
            zip(g["group_id"], g["group_timestamp"], g["group_tx"], ptr[:-1], ptr[1:])]


def failure_lines(g):
    return ["Failed to estimate group #%d: Underdetermined" % i for i in g["group_id"][~g["solved"]]]


def snr_bound(g):
    """(m - 1) 2^-53 sum |snr_i| / m per group: the bound of a mean for any summation order."""
    ptr = g["group_ptr"]
    m = np.diff(ptr)
    total = np.array([np.sum(np.abs(g["snr"][a:b])) for a, b in zip(ptr[:-1], ptr[1:])])
    return (m - 1) * 2.0 ** -53 * total / np.maximum(m, 1)


def check_positions(g, group_id, timestamp, tx, pos, dop, snr, slack=0.0):
    """The records of the SOLVED groups, in order, against the fixture.  Exact: which groups, their
    order, group_id, timestamp, tx -- and for a 1-D set every output.  Otherwise pos within ref_err_max
    of the EXACT minimiser (as close to it as the reference is), hence within 2 ref_err_max of the
    reference's; dop within dop_ref_err_max (relative) of the exact one; snr within the summation bound.
    `slack` [m] is added to ref_err_max where the caller's inputs are not the fixture's to the bit (the
    caller derives it); a 1-D set takes none.
    -> (max |x - x_star|, max |dop - dop_star| / dop_star)."""
    ok = g["solved"]
    np.testing.assert_array_equal(group_id, g["group_id"][ok])
    np.testing.assert_array_equal(timestamp, g["group_timestamp"][ok])
    np.testing.assert_array_equal(tx, g["group_tx"][ok])
    pos = np.asarray(pos, dtype=np.float64).reshape(int(ok.sum()), -1)
    dop, snr = np.asarray(dop, dtype=np.float64), np.asarray(snr, dtype=np.float64)
    if g["rx_xyz"].shape[1] == 1:
        assert slack == 0.0
        np.testing.assert_array_equal(pos, g["x_ref"][ok])
        np.testing.assert_array_equal(dop, g["dop_ref"][ok])
        np.testing.assert_array_equal(snr, g["snr_ref"][ok])
        return 0.0, 0.0
    bound, dop_bound = float(g["ref_err_max"]) + slack, float(g["dop_ref_err_max"])
    err = float(np.max(np.abs(pos - g["x_star"][ok])))
    dop_err = float(np.max(np.abs(dop - g["dop_star"][ok]) / g["dop_star"][ok]))
    print("max |x - x_star| = %.3g m (reference: %.3g m); max |dop - dop_star| / dop_star = %.3g (reference: %.3g)"
          % (err, bound, dop_err, dop_bound))
    assert err <= bound
    assert np.all(np.abs(pos - g["x_ref"][ok]) <= 2 * bound)
    assert dop_err <= dop_bound
    assert np.all(np.abs(snr - g["snr_ref"][ok]) <= snr_bound(g)[ok])
    return err, dop_err
