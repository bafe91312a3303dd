"""thr_beaconsync and thr_tdoastats at their seams, against the NumPy restatement and the exact values
(tests/syncstats_ref.py) with the assertions of tests/test_gpu_syncstats.py: row counts around the wavefront, the
workgroup W and the tile T; a cell of several fragments, a cell per row pair, a cell that starts on a tile's last
position; cuts of exactly 9 and 10 rows; discontinuities at the first and last dsdoa, on both sides of a tile
boundary, and next to each other; a cell of one row; degenerate cuts; filters; for the TDOA statistics cells of
1, 2, 3 and 4 T rows, a constant cell, a far outlier, NaN, cells of one row that hold a number, a NaN and the two
infinities, and the range filters on and off their bounds."""
import os

import numpy as np
import pytest

import syncstats_ref as R
from test_gpu_syncstats import same_discrete
from thrifty_amd import _native, build

pytestmark = pytest.mark.gpu

T, W = (256, 256)       # thr_debug_*_geometry (checked below): the sizes are parametrised at import
JUMP = 8192.0


def scene(cells, seed=0, shuffle=True, equal_soa0=None):
    """cells: (beacon, rx0, rx1, rows, [row indices k whose dsdoa[k] is a jump]) -> (columns, match_ptr, match_idx).
    Every match holds two detections; rx1 runs 20 ppm fast, so dsdoa is about 48 samples a row."""
    g = np.random.default_rng(seed)
    events = []
    for ci, (b, rx0, rx1, n, jumps) in enumerate(cells):
        t = np.cumsum(g.uniform(0.9, 1.1, n)) + g.uniform(0, 1)
        soa0 = np.round((700.0 + 11 * ci + t) * 2.4e6 + g.normal(0, 0.05, n), 8)
        if equal_soa0 and ci in equal_soa0:
            lo, hi = equal_soa0[ci]
            soa0[lo:hi] = soa0[lo]
        shift = np.zeros(n)
        for k in jumps:
            shift[k + 1:] += JUMP
        soa1 = np.round(soa0 * (1 + 20e-6) + 3.0e5 * ci + shift + g.normal(0, 0.05, n), 8)
        events += [(float(t[i]), b, rx0, rx1, float(soa0[i]), float(soa1[i])) for i in range(n)]
    if shuffle:
        events.sort(key=lambda e: e[0])
    m = len(events)
    cols = {"rxid": np.array([[e[2], e[3]] for e in events], np.int32).reshape(-1),
            "txid": np.repeat(np.array([e[1] for e in events], np.int32), 2),
            "soa": np.array([[e[4], e[5]] for e in events]).reshape(-1), "energy": g.uniform(300, 900, 2 * m),
            "noise": g.uniform(10, 20, 2 * m), "idx": np.arange(2 * m, dtype=np.int64) + 100}
    return cols, 2 * np.arange(m + 1, dtype=np.int64), np.arange(2 * m, dtype=np.int64)


def run_and_check(cols, ptr, idx, deg=2, what="", **kw):
    counts, out = _native.beaconsync(cols, ptr, idx, deg, **kw)
    ref_counts, ref = R.beacon_sync_ref(cols, ptr, idx, deg, **kw)
    assert counts == ref_counts, what
    same_discrete(out, ref, what)
    exact = R.exact_beacon_values(cols, out, deg)
    soa = np.asarray(cols["soa"])
    polyfit = {}
    for c in range(counts["cells"]):
        a = int(out["cell_ptr"][c])
        for k in range(int(out["cut_ptr"][c]), int(out["cut_ptr"][c + 1])):
            if out["cut_flags"][k] == R.CUT_FITTED:
                lo, hi = a + int(out["cut_left"][k]), a + int(out["cut_right"][k])
                _, res = R.polyfit_residuals(soa[out["row_det"][lo:hi, 0]], soa[out["row_det"][lo:hi, 1]], deg)
                polyfit[k] = float(np.max(np.abs(res - exact["residual"][lo:hi])))
    worst = R.assert_beacon_within_bounds(cols, out, exact, polyfit, what)
    print("%s: residuals at most %.2f of the floor from the exact ones" % (what, worst))
    return counts, out


def test_geometry_is_the_one_the_cases_were_sized_for():
    assert _native.syncstats_geometry("beaconsync") == (T, W) and _native.syncstats_geometry("tdoastats") == (T, W)
    source = open(os.path.join(build.CSRC, "syncstats.hip")).read()
    shared = open(os.path.join(build.CSRC, "seg_reduce.hpp")).read()      # the tile and the workgroup are the shared reduction's
    assert '#include "seg_reduce.hpp"' in source
    assert "constexpr int kTile = %d;" % T in shared and "constexpr int kBlock = %d;" % W in shared
    assert "constexpr int kMinCut = 8;" in source


@pytest.mark.parametrize("n", sorted({1, 2, 9, 10, 63, 64, 65, W - 1, W + 1, T - 1, T, T + 1, 2 * T + 1}))
def test_row_counts(n):
    jumps = [n // 3, n // 3 + 14] if n > 60 else []
    counts, out = run_and_check(*scene([(0, 0, 1, n, jumps)], seed=n), deg=2, what="n=%d" % n)
    assert counts["rows"] == n and out["disc_idx"].tolist() == jumps
    if n == 1:
        assert np.isnan(out["cell_stats"][0]).all() and out["cell_flags"][0] == R.CELL_NO_FIT and counts["cuts"] == 1
    assert (out["cell_counts"][0, 2] > 0) == (n >= 10)      # rows 1 .. 9 are the shortest cut that is fitted


@pytest.mark.parametrize("deg", [1, 2, 3])
def test_one_cell_of_three_tiles_and_a_bit(deg):
    n = 3 * T + 5
    jumps = [0, T - 2, T - 1, T, 2 * T + 40, 2 * T + 41, n - 2]   # first and last dsdoa, around a tile boundary, adjacent
    counts, out = run_and_check(*scene([(5, 1, 4, n, jumps)], seed=deg), deg=deg, what="3T+5 deg %d" % deg)
    assert counts["cells"] == 1 and out["disc_idx"].tolist() == jumps and counts["cuts"] == len(jumps) + 1
    lengths = (out["cut_right"] - out["cut_left"]).tolist()
    assert lengths == [-1, T - 3, 0, 0, T + 39, 0, n - 2 * T - 44, 1]
    assert out["cut_flags"].tolist() == [0, 1, 0, 0, 1, 0, 1, 0]


def test_cuts_of_exactly_nine_and_ten_rows_and_eight():
    # edges 0 | 10 | 21 | 30 | n: cuts [1, 10) = 9 rows, [11, 21) = 10 rows, [22, 30) = 8 rows (not fitted), the rest
    counts, out = run_and_check(*scene([(0, 0, 1, 120, [10, 21, 30])], seed=4), what="9 / 10 / 8")
    assert (out["cut_right"] - out["cut_left"]).tolist() == [9, 10, 8, 89] and out["cut_flags"].tolist() == [1, 1, 0, 1]
    assert np.isnan(out["cut_disc_soa"]).tolist() == [False, False, True, True]
    assert np.isnan(out["residual"][[0, 10, 21, 22, 29, 30]]).all() and not np.isnan(out["residual"][[1, 9, 11, 20, 31]]).any()


def test_a_cell_per_row_pair_and_cells_across_tile_boundaries():
    cells = [(b, r0, r1, 2, []) for b in range(40) for r0 in range(3) for r1 in range(r0 + 1, 4)]      # 240 cells of 2 rows
    counts, out = run_and_check(*scene(cells, seed=5), what="pairs")
    assert counts["cells"] == 240 and counts["cuts"] == 240 and np.all(out["cell_flags"] == R.CELL_NO_FIT)
    # a cell that starts on a tile's last position, after one of T - 1 rows; negative ids order before positive ones
    cells = [(-3, -2, 7, T - 1, [100]), (-3, 0, 7, 2 * T, [T - 100, T]), (2, -2, 0, 30, [])]
    counts, out = run_and_check(*scene(cells, seed=6), deg=3, what="tile's last position")
    assert out["cell_key"].tolist() == [[-3, -2, 7], [-3, 0, 7], [2, -2, 0]] and out["cell_ptr"].tolist() == [0, T - 1, 3 * T - 1, 3 * T + 29]


def test_match_order_decides_row_order_and_longer_matches_give_every_pair():
    cols, ptr, idx = scene([(0, 0, 1, 50, [20]), (0, 0, 2, 50, []), (1, 1, 2, 40, [])], seed=7, shuffle=False)
    order = np.random.default_rng(8).permutation(len(ptr) - 1)          # matches out of time order: rows follow the matches
    idx2 = np.concatenate([idx[ptr[m]:ptr[m + 1]] for m in order])
    counts, out = run_and_check(cols, ptr, idx2, what="permuted matches")
    assert not np.all(np.diff(out["row_det"][:50, 0]) > 0)
    # three receivers in one match: three rows, one per cell; the first detection's txid names the beacon
    g = np.random.default_rng(9)
    n = 60
    t = np.cumsum(g.uniform(0.9, 1.1, n))
    soa = np.round(np.column_stack([(700 + t) * 2.4e6 * (1 + p) for p in (0.0, 15e-6, 40e-6)]) + g.normal(0, 0.05, (n, 3)), 8)
    cols = {"rxid": np.tile(np.array([4, 2, 9], np.int32), n), "txid": np.tile(np.array([6, -1, -1], np.int32), n),
            "soa": soa.reshape(-1), "energy": g.uniform(300, 900, 3 * n), "noise": g.uniform(10, 20, 3 * n),
            "idx": np.arange(3 * n, dtype=np.int64)}
    counts, out = run_and_check(cols, 3 * np.arange(n + 1, dtype=np.int64), np.arange(3 * n, dtype=np.int64), what="triples")
    assert out["cell_key"].tolist() == [[6, 2, 4], [6, 2, 9], [6, 4, 9]] and counts["rows"] == 3 * n
    assert np.all(out["cell_stats"][[1, 2], 0] > 0) and out["cell_stats"][0, 0] < 0      # (2, 4): rx 4 is the slow one


def test_degenerate_cuts_are_flagged_not_fitted():
    cols, ptr, idx = scene([(0, 0, 1, 60, [30]), (0, 0, 2, 40, [])], seed=10, equal_soa0={0: (1, 30)})
    counts, out = run_and_check(cols, ptr, idx, deg=3, what="equal soa0")
    assert out["cut_flags"].tolist()[:2] == [R.CUT_DEGENERATE, R.CUT_FITTED] and out["cell_counts"][0, 2] == 1
    assert np.isnan(out["cut_fit"][0]).all() and np.isnan(out["cut_snr"][0]) and np.isnan(out["residual"][1:30]).all()
    cols["soa"][5] = np.nan
    counts, out = _native.beaconsync(cols, ptr, idx, 2)
    same_discrete(out, R.beacon_sync_ref(cols, ptr, idx, 2)[1], "a NaN soa")


def test_id_range_that_empties_one_cell_and_lists():
    cols, ptr, idx = scene([(0, 0, 1, 40, [15]), (1, 0, 1, 30, [])], seed=11, shuffle=False)
    first = int(cols["idx"][0])
    counts, out = run_and_check(cols, ptr, idx, what="range", id_range=(first, first + 79))     # all of cell 0, none of cell 1
    assert out["cell_key"].tolist() == [[0, 0, 1]] and counts["rows"] == 40
    counts, out = run_and_check(cols, ptr, idx, what="range end", id_range=(first + 1, first + 100))
    assert out["cell_counts"][:, 0].tolist() == [39, 10]          # both ids must lie inside: row 0 goes, rows 40 .. 49 of cell 1 stay
    with pytest.raises(ValueError, match="selection is empty"):
        _native.beaconsync(cols, ptr, idx, 2, receivers=[0])
    with pytest.raises(ValueError, match="two detections of one receiver"):
        _native.beaconsync(dict(cols, rxid=np.zeros_like(cols["rxid"])), ptr, idx, 2)


# ------------------------------------------------------------------ thr_tdoastats
def tdoa_scene(sizes, seed=0):
    g = np.random.default_rng(seed)
    rows = []
    for ci, n in enumerate(sizes):
        x = g.normal(g.uniform(-300, 300), 4.0, n) / R.LIGHT
        rows += [(ci % 3 - 1, ci % 3 + ci // 3, ci // 2, v) for v in x]
    order = g.permutation(len(rows))
    rows = [rows[i] for i in order]
    n = len(rows)
    return {"rx0": np.array([r[0] for r in rows], np.int32), "rx1": np.array([r[1] for r in rows], np.int32),
            "tx": np.array([r[2] for r in rows], np.int32), "timestamp": 1.7e9 + np.arange(n) * 0.5,
            "det0_idx": 2 * np.arange(n, dtype=np.int64), "det1_idx": 2 * np.arange(n, dtype=np.int64) + 1,
            "tdoa": np.array([r[3] for r in rows])}


def run_tdoa(cols, what="", **kw):
    counts, out = _native.tdoastats(cols, **kw)
    ref_counts, ref = R.tdoa_stats_ref(cols, **kw)
    assert counts == ref_counts, what
    for name in ("cell_key", "cell_ptr", "order", "mask", "robust_count", "median"):
        assert np.array_equal(out[name], ref[name], equal_nan=True), (what, name)
    assert np.array_equal(out["stats"][:, 3:], ref["stats"][:, 3:], equal_nan=True), what
    assert np.array_equal(out["robust_stats"][:, 3:], ref["robust_stats"][:, 3:], equal_nan=True), what
    with np.errstate(all="ignore"):
        for name in ("stats", "robust_stats"):
            assert np.array_equal(np.isnan(out[name]), np.isnan(ref[name])), (what, name)
    R.assert_tdoa_within_bounds(cols, out, what)
    return counts, out


@pytest.mark.parametrize("robust", [False, True])
def test_tdoa_cells_of_every_size(robust):
    sizes = [1, 2, 3, 4, 63, 64, 65, T - 1, T, T + 1, 4 * T, 7, 2 * T + 1]
    counts, out = run_tdoa(tdoa_scene(sizes, seed=1), "sizes", robust=robust)
    assert sorted(np.diff(out["cell_ptr"]).tolist()) == sorted(sizes)
    if robust:
        assert out["mask"][out["cell_ptr"][:-1][np.diff(out["cell_ptr"]) == 1]].sum() == 0     # a cell of one row is left alone


def test_tdoa_constant_cell_far_outlier_and_nan():
    cols = tdoa_scene([40, 30, 12, 41], seed=2)                         # in key order: 40, 41, 30 and 12 rows
    key = cols["rx0"].astype(np.int64) * 100 + cols["rx1"] * 10 + cols["tx"]
    kinds = np.unique(key)
    cols["tdoa"][key == kinds[0]] = 1.251e-7                            # constant: MAD 0, 0 / 0 = NaN keeps every row
    far = np.flatnonzero(key == kinds[1])[5]
    cols["tdoa"][far] += 1e-5                                           # one far outlier
    cols["tdoa"][np.flatnonzero(key == kinds[2])[3]] = np.nan           # a NaN: every statistic NaN, no row masked
    some = np.flatnonzero(key == kinds[3])
    cols["tdoa"][some[:7]] = cols["tdoa"][some[0]]                      # 7 of 12 equal: MAD 0, the other five inf > 3.5
    counts, out = run_tdoa(cols, "special cells", robust=True)
    masked = (np.diff(out["cell_ptr"]) - out["robust_count"]).tolist()
    assert np.diff(out["cell_ptr"]).tolist() == [40, 41, 30, 12]
    assert masked[0] == 0 and masked[1] >= 1 and masked[2:] == [0, 5] and out["mask"][out["order"] == far] == 1
    assert out["median"][0].tolist() == [1.251e-7 * R.LIGHT, 0.0] and out["stats"][0, 1] == 0.0
    assert out["median"][3, 1] == 0.0 and out["robust_stats"][3, 1] == 0.0
    assert np.isnan(out["stats"][2]).all() and np.isnan(out["median"][2]).all() and np.isnan(out["robust_stats"][2]).all()


def test_tdoa_cells_of_one_row_are_never_masked():
    """The shared mask kernel has no case for a cell of one row: its deviation and its MAD are the same number
    (0, or NaN for a value that is not finite), so z is 0 / 0 or NaN and nothing exceeds the threshold."""
    cols = tdoa_scene([1, 1, 1, 1, T + 1], seed=12)
    key = cols["rx0"].astype(np.int64) * 100 + cols["rx1"] * 10 + cols["tx"]
    kinds, rows = np.unique(key, return_counts=True)
    single = kinds[rows == 1]
    assert len(single) == 4                                             # the first keeps its finite value
    for k, v in zip(single[1:], (np.nan, np.inf, -np.inf)):
        cols["tdoa"][key == k] = v
    counts, out = run_tdoa(cols, "cells of one row", robust=True)       # median and mask equal the reference's, NaNs included
    sizes = np.diff(out["cell_ptr"])
    assert sorted(sizes.tolist()) == [1, 1, 1, 1, T + 1]
    first = out["cell_ptr"][:-1][sizes == 1]
    assert not out["mask"][first].any() and np.array_equal(out["robust_count"], sizes)
    x = cols["tdoa"][out["order"][first]] * R.LIGHT
    assert np.array_equal(out["median"][sizes == 1, 0], x, equal_nan=True)      # one value is its own median
    assert np.isfinite(x).sum() == 1 and np.isnan(x).sum() == 1 and sorted(x[np.isinf(x)].tolist()) == [-np.inf, np.inf]
    assert np.array_equal(np.isnan(out["median"][sizes == 1, 1]), ~np.isfinite(x))      # MAD 0 for the finite one, else NaN


def test_tdoa_range_filters_on_and_off_their_bounds():
    cols = tdoa_scene([30, 30, 30], seed=3)
    t = cols["timestamp"]
    for kw in (dict(timestamp=(t[10], t[50])), dict(timestamp=(t[10] + 0.1, t[50] - 0.1)), dict(detidx=(20, 101)),
               dict(detidx=(21, 100)), dict(timestamp=(t[0], t[40]), detidx=(30, 200), robust=True)):
        counts, out = run_tdoa(cols, str(kw), **kw)
    assert counts["rows"] == 26                     # rows 15 .. 40: det ids 30 .. 81
    counts, out = run_tdoa(cols, "on the bounds", timestamp=(t[10], t[50]))
    assert counts["rows"] == 41
    counts, out = run_tdoa(cols, "det ids", detidx=(20, 101))
    assert counts["rows"] == 41                     # rows 10 .. 50: the pair (20, 21) .. (100, 101)
    counts, out = run_tdoa(cols, "det ids off", detidx=(21, 100))
    assert counts["rows"] == 39
    with pytest.raises(ValueError, match="selection is empty"):
        _native.tdoastats(cols, detidx=(21, 21))
