"""The tdoa fixtures (tests/golden/tdoa/*.npz, made by tests/golden/make_golden_tdoa.py) for the host
and the GPU tests: loading, DetectionResult objects, and the comparison every path is held to."""
import os

import numpy as np

from thrifty_amd import toads_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tdoa")
SETS = ("tdoa_realistic", "tdoa_failures", "tdoa_ties", "tdoa_wide")
_cache = {}


def load(name):
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, name + ".npz")) as g:
            _cache[name] = {key: g[key] for key in g.files}
    return _cache[name]


def positions(g):
    return ({int(r): xyz for r, xyz in zip(g["rx_ids"], g["rx_xyz"])},
            {int(b): xyz for b, xyz in zip(g["beacon_ids"], g["beacon_xyz"])})


def matches(g):
    ptr, idx = g["match_ptr"].tolist(), g["match_idx"].tolist()
    return [idx[a:b] for a, b in zip(ptr[:-1], ptr[1:])]


def detections(g):
    out = []
    for i in range(len(g["rxid"])):
        car = toads_data.CarrierSyncInfo(40 + int(g["txid"][i]), 0.1, 150.0, 7.5)
        cor = toads_data.CorrDetectionInfo(4000 + i % 97, 0.25, float(g["energy"][i]), float(g["noise"][i]))
        out.append(toads_data.DetectionResult(float(g["timestamp"][i]), i, float(g["soa"][i]), car, cor,
                                              rxid=int(g["rxid"][i]), txid=int(g["txid"][i])))
    return out


def check_against_fixture(g, group_id, group_timestamp, group_tx, group_ptr, rows, failures, n_window=None,
                          n_kept=None):
    """`rows`: dict of columns rx0, rx1, tdoa, snr, model_quality, det0, det1 over all rows in order.
    Exact: groups, ids, indices, orders, failures, n_window, n_kept.  tdoa: within ref_err_max of the
    EXACT least-squares value (as close to it as the reference is) and within 2 ref_err_max of the
    reference's; snr relative 1e-14, model_quality relative 1e-12.  -> max |tdoa - exact|."""
    np.testing.assert_array_equal(group_id, g["group_id"])
    np.testing.assert_array_equal(group_timestamp, g["group_timestamp"])
    np.testing.assert_array_equal(group_tx, g["group_tx"])
    np.testing.assert_array_equal(group_ptr, g["group_ptr"])
    for key in ("rx0", "rx1", "det0", "det1"):
        np.testing.assert_array_equal(rows[key], g[key], err_msg=key)
    np.testing.assert_array_equal(np.asarray(failures).reshape(-1, 2), g["failures"])
    if n_window is not None:
        np.testing.assert_array_equal(n_window, g["n_window"])
        np.testing.assert_array_equal(n_kept, g["n_kept"])
    bound = float(g["ref_err_max"])
    tdoa = np.asarray(rows["tdoa"], float)
    err = float(np.max(np.abs(tdoa - g["exact_tdoa"]))) if len(tdoa) else 0.0
    print("max |tdoa - exact| = %.3g s (reference: %.3g s)" % (err, bound))
    assert err <= bound
    assert np.all(np.abs(tdoa - g["tdoa"]) <= 2 * bound)
    np.testing.assert_allclose(rows["snr"], g["snr"], rtol=1e-14, atol=0)
    np.testing.assert_allclose(rows["model_quality"], g["model_quality"], rtol=1e-12, atol=0)
    return err
