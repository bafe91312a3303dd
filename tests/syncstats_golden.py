"""The recorded runs of the reference under tests/golden/syncstats (made by tests/golden/make_golden_syncstats.py)
and the comparisons every holder of the numbers is put through: the NumPy restatement on the CPU
(tests/test_syncstats_host.py), the device on the GPU (tests/test_gpu_syncstats.py)."""
import functools
import os
from fractions import Fraction

import numpy as np

import syncstats_ref as R
from thrifty_amd import beacon_analysis, tdoa_analysis

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "syncstats")
NAMES = ("realistic", "slow_rx1", "tdoa")
BEACONS = [0, 1]


@functools.lru_cache(maxsize=None)
def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as f:
        return {k: f[k] for k in f.files}


def beacon_columns(g):
    return {name: g[name] for name, _ in R.BSYNC_COLUMNS}


def tdoa_columns(g):
    return {name: g[name] for name, _ in R.TDSTATS_COLUMNS}


@functools.lru_cache(maxsize=None)
def restated(name, deg):
    """The NumPy restatement on the fixture's beacons (computed once; nobody changes it)."""
    g = load(name)
    return R.beacon_sync_ref(beacon_columns(g), g["match_ptr"], g["match_idx"], deg, beacons=BEACONS)


@functools.lru_cache(maxsize=None)
def exact(name, deg):
    return R.exact_beacon_values(beacon_columns(load(name)), restated(name, deg)[1], deg)


def check_beacon(counts, out, exact_values, g, deg, what=""):
    """`out` against the reference's run: rows, discontinuities, cuts and text exactly; residuals per cut within
    max(2 polyfit_distance, floor) of the exact ones; the raw coefficients as good as the residuals; the summary
    within its rounding bounds.  Returns the largest residual distance in units of the floor."""
    cols = beacon_columns(g)
    sync = beacon_analysis.BeaconSync(counts, out, g["idx"], deg, 2.4e6)
    assert [tuple(k) for k in out["cell_key"].tolist()] == [tuple(k) for k in g["cells"].tolist()], what
    polyfit_distance = {}
    for c, (b, r0, r1) in enumerate(out["cell_key"].tolist()):
        tag = "b%d_%d_%d_deg%d_" % (b, r0, r1, deg)
        a, e = int(out["cell_ptr"][c]), int(out["cell_ptr"][c + 1])
        assert np.array_equal(out["row_det"][a:e], g[tag + "matrix"]), (what, tag)
        text = beacon_analysis.format_report(sync, c)
        failed = bool(str(g[tag + "error"]))
        assert text == str(g[tag + "text"]) + (beacon_analysis.NO_FIT_TEXT + "\n" if failed else ""), (what, tag)
        assert bool(out["cell_flags"][c] & R.CELL_NO_FIT) == failed, (what, tag)
        fitted = [k for k in range(int(out["cut_ptr"][c]), int(out["cut_ptr"][c + 1])) if out["cut_flags"][k] == R.CUT_FITTED]
        assert out["cut_left"][fitted].tolist() == g[tag + "cut_left"].tolist(), (what, tag)
        assert len(g[tag + "coefs"]) == len(fitted)
        for i, k in enumerate(fitted):
            polyfit_distance[k] = float(g[tag + "polyfit_distance"][i])
            lo, hi = a + int(out["cut_left"][k]), a + int(out["cut_right"][k])
            soa0, soa1 = cols["soa"][out["row_det"][lo:hi, 0]], cols["soa"][out["row_det"][lo:hi, 1]]
            coef = [Fraction(float(v)) for v in beacon_analysis.raw_coefficients(out["cut_fit"][k], deg)]
            for x, y, r in zip(R.fractions_of(soa0), R.fractions_of(soa1), exact_values["residual"][lo:hi]):
                terms = [cf * x ** (deg - j) for j, cf in enumerate(coef)]
                # the polynomial returned, evaluated exactly, is the exact fit up to the residuals' own limit
                # and one rounding of each coefficient
                lim = max(2 * polyfit_distance[k], R.residual_floor(soa1)) + 4 * R.U * float(sum(abs(t) for t in terms))
                assert abs(float(y - sum(terms)) - r) <= lim, (what, tag, k)
    return R.assert_beacon_within_bounds(cols, out, exact_values, polyfit_distance, what)


def check_tdoa(counts, out, g, what=""):
    """`out` against NumPy's numbers and the reference's mask: cells, order, min, max, text and mask exactly;
    mean, std and RMS within their rounding bounds."""
    cols = tdoa_columns(g)
    assert counts["rows"] == len(g["tdoa"]) and counts["cells"] == len(g["cell_key"])
    assert np.array_equal(out["cell_key"], g["cell_key"]), what
    stats = tdoa_analysis.TdoaStats(counts, out)
    for c, (rx0, rx1, tx) in enumerate(g["cell_key"].tolist()):
        rows = np.flatnonzero((cols["rx0"] == rx0) & (cols["rx1"] == rx1) & (cols["tx"] == tx))
        assert np.array_equal(out["order"][out["cell_ptr"][c]:out["cell_ptr"][c + 1]], rows), (what, c)
        assert tdoa_analysis.format_report(stats, c) == str(g["text"][c]), (what, c)
    assert np.array_equal(out["stats"][:, 3:], g["np_stats"][:, 3:]), what
    if counts["robust"]:
        assert np.array_equal(out["mask"], g["is_outlier"][out["order"]]), what
        kept = np.add.reduceat(1 - out["mask"].astype(np.int64), out["cell_ptr"][:-1])
        assert np.array_equal(out["robust_count"], kept), what
    R.assert_tdoa_within_bounds(cols, out, what)
