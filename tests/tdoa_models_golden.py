"""The fixtures of the weighted, nearest and linear TDOA models (tests/golden/tdoa_models/*.npz, made by
tests/golden/make_golden_tdoa_models.py from the reference's own builders) for the host and the GPU tests:
loading, and the comparison every path is held to.  Objects and positions come from tests/tdoa_golden.py."""
import os

import numpy as np

import tdoa_golden

GOLDEN = os.path.join(tdoa_golden.ROOT, "tests", "golden", "tdoa_models")
MODELS = ("weighted_poly", "nearest", "linear")
SETS = tuple("%s_%s" % (scene, model) for scene in tdoa_golden.SETS for model in MODELS) + (
    "tdoa_realistic_weighted_poly_deg1",)
_cache = {}


def load(name):
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, name + ".npz")) as g:
            _cache[name] = {key: g[key] for key in g.files}
        _cache[name]["model"] = str(_cache[name]["model"])
    return _cache[name]


def check_against_fixture(g, group_id, group_timestamp, group_tx, group_ptr, rows, failures, n_window=None,
                          n_kept=None):
    """`rows`: dict of columns rx0, rx1, tdoa, snr, model_quality, det0, det1 over all rows in order.
    Exact: groups, ids, indices, orders, failures, n_window, n_kept.  tdoa of nearest / linear: the
    reference's bits.  tdoa of weighted_poly: within ref_err_max of the EXACT weighted least-squares value
    (as close to it as the reference is) and within 2 ref_err_max of the reference's.  snr relative 1e-14,
    model_quality relative 1e-12.  -> max |tdoa - exact| (weighted) or 0."""
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
    tdoa = np.ascontiguousarray(rows["tdoa"], dtype=np.float64)
    err = 0.0
    if g["model"] == "weighted_poly":
        bound = float(g["ref_err_max"])
        err = float(np.max(np.abs(tdoa - g["exact_tdoa"]))) if len(tdoa) else 0.0
        print("max |tdoa - exact| = %.3g s (reference: %.3g s)" % (err, bound))
        assert err <= bound
        assert np.all(np.abs(tdoa - g["tdoa"]) <= 2 * bound)
    else:
        different = np.flatnonzero(tdoa.view(np.uint64) != g["tdoa"].view(np.uint64))
        print("%d of %d tdoa differ from the reference's bits" % (len(different), len(tdoa)))
        assert len(different) == 0, (different[:5], tdoa[different[:5]], g["tdoa"][different[:5]])
    np.testing.assert_allclose(rows["snr"], g["snr"], rtol=1e-14, atol=0)
    np.testing.assert_allclose(rows["model_quality"], g["model_quality"], rtol=1e-12, atol=0)
    return err
