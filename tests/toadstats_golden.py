"""The fixtures of tests/golden/toadstats (made by tests/golden/make_golden_toadstats.py from the reference's
own run) and the assertions both the host restatement and the device are held to against them."""
import os

import numpy as np

import toadstats_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "toadstats")
NAMES = ("realistic", "ties", "sparse")
DISCRETE = ("cell_rx", "cell_tx", "cell_ptr", "minute_ptr", "minute_hist", "bin_first", "bin_ptr", "bin_hist",
            "offset_hist", "rx_id")
NOT_DB = (0, 1, 3, 4, 5, 6, 8)      # the seven quantities without a log10


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def columns(g):
    return {name: g[name] for name, _ in R.COLUMNS}


def matches(g):
    ptr, idx = g["match_ptr"].tolist(), g["match_idx"].tolist()
    return [idx[a:b] for a, b in zip(ptr[:-1], ptr[1:])]


def selection(g, prefix):
    return None if prefix == "" else np.sort(g["match_idx"])


def db_distance_ulps(snr_db, cols, sel=None):
    """Largest distance, in ulps of NumPy's value, between `snr_db` and NumPy's 20 * log10(a / b)."""
    c = R.columns_of(cols)
    rows = R.check_selection(c, sel)
    want = R.quantities(c, rows)[[2, 7]].T
    finite = np.isfinite(want)
    assert np.array_equal(snr_db[~finite], want[~finite], equal_nan=True)
    if not finite.any():
        return 0.0
    return float(np.max(np.abs(snr_db[finite] - want[finite]) / np.spacing(np.abs(want[finite]))))


def check(counts, out, g, prefix="", what=""):
    """Every assertion of the issue against fixture `g` (prefix m_: the matched detections).  The dB statistics
    are held to exact values computed from out["snr_db"] itself.  Returns the dB columns' distance in ulps."""
    cols, sel = columns(g), selection(g, prefix)
    assert counts["time0"] == float(g[prefix + "time0"])
    for name in DISCRETE:
        assert np.array_equal(out[name], g[prefix + name]), (what, name)
    order = out["order"]
    assert counts["rows"] == len(order) == (len(cols["rxid"]) if sel is None else len(sel))
    for c in range(counts["cells"]):        # grouped by cell, input order inside
        rows = order[out["cell_ptr"][c]:out["cell_ptr"][c + 1]]
        assert np.all(np.diff(rows) > 0), (what, c)
        assert np.all(cols["rxid"][rows] == out["cell_rx"][c]) and np.all(cols["txid"][rows] == out["cell_tx"][c])
        j = rows if sel is None else np.searchsorted(sel, rows)
        for k, col in ((2, 0), (7, 1)):     # the dB extremes are those of the dB column that was fetched
            assert out["stats"][c, k, 2] == np.min(out["snr_db"][j, col]) and out["stats"][c, k, 3] == np.max(out["snr_db"][j, col])
    assert np.array_equal(out["rx_count"], [np.sum(cols["rxid"][order] == r) for r in out["rx_id"]])
    assert not out["cell_flags"].any()
    np_stats = g[prefix + "np_stats"]
    for k in NOT_DB:
        assert out["stats"][:, k, 2:].tobytes() == np_stats[:, k, 2:].tobytes(), (what, k)
    assert out["offset_edges"].tobytes() == g[prefix + "offset_edges"].tobytes(), what
    ulps = db_distance_ulps(out["snr_db"], cols, sel)
    exact = R.exact_values(cols, sel, out["snr_db"])
    for k in NOT_DB:        # the recorded exact values are the ones computed here
        assert np.array_equal(exact["cells"][:, k], g[prefix + "exact_cells"][:, k], equal_nan=True)
    assert np.array_equal(exact["rx_fit"], g[prefix + "exact_rx_fit"], equal_nan=True)
    R.assert_stats_within_bounds(out["stats"], exact["cells"], out["cell_ptr"], what)
    R.assert_fit_within_bounds(out["rx_fit"], out["residual"], exact, cols, sel, what)
    return ulps


# The dB columns against NumPy's 20 * log10(a / b), element by element.  Measured on the MI355X over the three
# fixtures and every case of tests/test_gpu_toadstats_seams.py: the device's log10 is at most
DB_ULPS_MEASURED = 2.0      # ulps of NumPy's value away (one ulp of log10, doubled by the multiplication by 20)
DB_ULPS_LIMIT = max(1.0, 2 * DB_ULPS_MEASURED)
