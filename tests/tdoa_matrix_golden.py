"""The tdoa_matrix fixtures (tests/golden/tdoa_matrix/*.npz, made by tests/golden/make_golden_tdoa_matrix.py) for
the host and the GPU tests: loading, and the comparisons every path is held to."""
import os

import numpy as np

import syncstats_ref
from syncstats_ref import LIGHT, U, assert_mean_within, assert_std_within, exact_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tdoa_matrix")
SETS = ("tdmat_realistic", "tdmat_edges", "tdmat_wide", "tdmat_nearest")
EXACT = ("cell_key", "cell_ptr", "cell_flags", "cell_counts", "task_det", "task_match", "status", "n_window", "n_kept", "outlier")
OK = 0
_cache = {}


def load(name):
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, name + ".npz")) as g:
            _cache[name] = {key: g[key] for key in g.files}
    return _cache[name]


def columns(g):
    return {name: g[name] for name in ("rxid", "txid", "timestamp", "soa", "energy", "noise")}


def matches(g):
    ptr, idx = g["match_ptr"].tolist(), g["match_idx"].tolist()
    return [idx[a:b] for a, b in zip(ptr[:-1], ptr[1:])]


def arguments(g):
    """What every path is called with for this fixture."""
    return dict(beacons=g["beacons"].tolist(), receivers=g["receivers"].tolist(), window=float(g["window"]),
                sample_rate=float(g["sample_rate"]), model=str(g["model"]), deg=int(g["deg"]))


def check_structure(out, want, what=""):
    """Exact: cell keys, pointers, flags, counts, det / match / timestamp rows, statuses, n_window, n_kept, the mask."""
    for name in EXACT:
        np.testing.assert_array_equal(out[name], want[name], err_msg="%s %s" % (what, name))
    np.testing.assert_array_equal(out["timestamp"], want["task_timestamp" if "task_timestamp" in want else "timestamp"],
                                  err_msg="%s timestamp" % what)


def check_rows(out, g, what=""):
    """The rule of tdoa_golden.check_against_fixture: every TDOA within ref_err_max of the exact value and within
    2 ref_err_max of the reference's; snr relative 1e-14, model_quality relative 1e-12; the nearest model's TDOAs
    are the reference's bits.  Tasks without a TDOA hold NaN.  -> max |tdoa - exact|."""
    ok = g["status"] == OK
    bound = float(g["ref_err_max"])
    tdoa = np.asarray(out["tdoa"], float)
    assert np.all(np.isnan(tdoa[~ok])) and np.all(np.isnan(out["model_quality"][~ok])), what
    err = float(np.max(np.abs(tdoa[ok] - g["exact_tdoa"][ok]))) if ok.any() else 0.0
    print("%s: max |tdoa - exact| = %.3g s (reference: %.3g s)" % (what, err, bound))
    if str(g["model"]) == "nearest":
        assert tdoa[ok].tobytes() == g["tdoa"][ok].tobytes(), what
    assert err <= bound, (what, err, bound)
    assert np.all(np.abs(tdoa[ok] - g["tdoa"][ok]) <= 2 * bound), what
    np.testing.assert_allclose(out["snr"], g["snr"], rtol=1e-14, atol=0, err_msg=what)
    np.testing.assert_allclose(out["model_quality"][ok], g["model_quality"][ok], rtol=1e-12, atol=0, err_msg=what)
    return err


def check_own_mask_and_stats(out, what=""):
    """The mask equals is_outlier applied on the host to out's OWN TDOAs, bit for bit (median and MAD too); the
    statistics lie within the rounding bounds of the exact statistics of out's own kept rows; min and max are theirs."""
    for c in range(len(out["cell_ptr"]) - 1):
        a, b = int(out["cell_ptr"][c]), int(out["cell_ptr"][c + 1])
        ok = out["status"][a:b] == OK
        v = out["tdoa"][a:b][ok]
        mask = np.zeros(len(v), bool)
        median, mad = np.nan, np.nan
        if len(v):
            mask, median, mad = syncstats_ref.is_outlier(v)
            if len(v) == 1:
                mask = np.zeros(1, bool)
        assert np.array_equal(out["outlier"][a:b][ok] != 0, mask) and not np.any(out["outlier"][a:b][~ok]), (what, c)
        assert np.array([median, mad]).tobytes() == out["medians"][c].tobytes() or (
            np.isnan(median) and np.all(np.isnan(out["medians"][c]))), (what, c, median, mad, out["medians"][c])
        x = v[~mask] * LIGHT
        got = out["cell_stats"][c]
        assert out["cell_counts"][c, 2] == len(v) and out["cell_counts"][c, 4] == len(x), (what, c)
        if len(x) == 0:
            assert np.all(np.isnan(got)), (what, c)
            continue
        mean, std, rms, mabs = exact_stats(x)
        n = len(x)
        assert_mean_within(got[0], mean, mabs, n, (what, c, "mean"))
        assert_std_within(got[1], std, mabs, n, what=(what, c, "std"))
        assert abs(got[2] - rms) <= (n + 4) * U * rms, (what, c, "rms", got[2], rms)
        assert got[3] == np.min(x) and got[4] == np.max(x), (what, c)


def check_reference_stats(out, g, what=""):
    """std and mean against the reference's (np.std, np.mean of ITS kept TDOAs), with extra = 2 ref_err_max * 2.997e8:
    the rows are the same ones (the mask is exact) and each lies within 2 ref_err_max of the reference's."""
    extra = 2 * float(g["ref_err_max"]) * LIGHT
    for c in range(len(g["cell_ptr"]) - 1):
        n = int(g["table_count"][c])
        got = out["cell_stats"][c]
        if n == 0:
            assert np.all(np.isnan(got)), (what, c)
            continue
        a, b = int(g["cell_ptr"][c]), int(g["cell_ptr"][c + 1])
        kept = (g["status"][a:b] == OK) & (g["outlier"][a:b] == 0)
        mabs = float(np.mean(np.abs(g["tdoa"][a:b][kept] * LIGHT)))
        assert abs(got[0] - g["ref_mean"][c]) <= (n + 2) * U * mabs + extra, (what, c, "mean", got[0], g["ref_mean"][c])
        assert_std_within(got[1], float(g["ref_std"][c]), mabs, n, extra=extra, what=(what, c, "std"))


def check_tables(result, g, what=""):
    """TdoaMatrices' three tables against the script's printed numbers, wherever the unrounded reference value is
    farther than the permitted distance from a rounding boundary (firm_*); the counts everywhere."""
    key = g["cell_key"]
    for rx0, rx1 in sorted(set((int(k[0]), int(k[1])) for k in key.tolist())):
        tables = [result.variance_table(rx0, rx1), result.mean_table(rx0, rx1), result.count_table(rx0, rx1)]
        for c in np.flatnonzero((key[:, 0] == rx0) & (key[:, 1] == rx1)).tolist():
            for (beacons, txids, table), want, firm in zip(tables, ("table_std", "table_mean", "table_count"),
                                                           (g["firm_std"][c], g["firm_mean"][c], True)):
                got = table[list(beacons).index(key[c, 2]), list(txids).index(key[c, 3])]
                if firm:
                    assert got == g[want][c], (what, key[c].tolist(), want, got, g[want][c])
