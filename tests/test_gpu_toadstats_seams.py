"""thr_toadstats at its seams, against the NumPy restatement (tests/toadstats_ref.py) with the assertions of
tests/test_gpu_toadstats.py: sizes around the wavefront, the workgroup W and the tile T; cells that are one
fragment, several fragments, or many to a tile; the key's order at the ends of int32; minute boundaries; the
histogram fallback; the offset histogram's edges; NaN, inf and zero noise; selections, errors, resources."""
import numpy as np
import pytest

import toadstats_golden as G
import toadstats_ref as R
from thrifty_amd import _native

pytestmark = pytest.mark.gpu

T, W = (256, 256)       # thr_debug_toadstats_geometry (checked below): the sizes are parametrised at import
I32 = np.iinfo(np.int32)
EVERY = ("cell_rx", "cell_tx", "cell_ptr", "order", "minute_ptr", "minute_hist", "bin_first", "bin_ptr", "bin_hist",
         "offset_hist", "cell_flags", "rx_id", "rx_count")


def scene(n, rx, tx, seed=0):
    g = np.random.default_rng(seed)
    ts = np.sort(g.uniform(0, 900, n))
    rx = np.broadcast_to(np.asarray(rx), (n,)) if np.ndim(rx) else g.integers(0, rx, n)
    tx = np.broadcast_to(np.asarray(tx), (n,)) if np.ndim(tx) else g.integers(-1, tx - 1, n)
    cols = {"rxid": np.array(rx, np.int32), "txid": np.array(tx, np.int32), "carrier_bin": g.integers(-40, 60, n),
            "timestamp": 1.7e9 + np.round(ts, 6), "carrier_offset": g.uniform(-.5, .5, n),
            "carrier_energy": g.uniform(50, 500, n), "carrier_noise": g.uniform(1, 5, n), "energy": g.uniform(500, 5000, n),
            "noise": g.uniform(5, 50, n), "offset": g.uniform(-.5, .5, n)}
    cols["soa"] = np.round(ts * 2.4e6 * (1 + 30e-6 * (cols["rxid"] % 7)) + g.normal(0, 3, n), 8)
    return cols


def run_and_check(cols, sel=None, what=""):
    counts, out = _native.toadstats(cols, sel)
    ulps = G.db_distance_ulps(out["snr_db"], cols, sel)
    print("%s: dB columns at most %.2f ulps from NumPy's (limit %.1f)" % (what, ulps, G.DB_ULPS_LIMIT))
    assert ulps <= G.DB_ULPS_LIMIT
    ref_counts, ref = R.toad_stats_ref(cols, sel, out["snr_db"])        # its dB quantities: the fetched columns
    assert counts == ref_counts
    for name in EVERY:
        assert np.array_equal(out[name], ref[name]), (what, name)
    assert out["offset_edges"].tobytes() == ref["offset_edges"].tobytes(), what
    assert np.array_equal(out["stats"][:, :, 2:], ref["stats"][:, :, 2:], equal_nan=True), what
    assert np.array_equal(out["snr_db"], ref["snr_db"], equal_nan=True)
    exact = R.exact_values(cols, sel, out["snr_db"])
    R.assert_stats_within_bounds(out["stats"], exact["cells"], out["cell_ptr"], what)
    inexact = np.isnan(exact["cells"][:, :, 0])     # a non-finite value in the cell: NumPy's own NaN / inf pattern
    with np.errstate(all="ignore"):
        assert np.array_equal(out["stats"][inexact][:, :2], ref["stats"][inexact][:, :2], equal_nan=True), what
    R.assert_fit_within_bounds(out["rx_fit"], out["residual"], exact, cols, sel, what)
    return counts, out, ref


def test_geometry_is_the_one_the_cases_were_sized_for():
    assert _native.toadstats_geometry() == (T, W)
    csrc = __import__("thrifty_amd.build").build.CSRC
    source = open(__import__("os").path.join(csrc, "toadstats.hip")).read()
    shared = open(__import__("os").path.join(csrc, "seg_reduce.hpp")).read()      # the tile and the workgroup are the shared reduction's
    assert '#include "seg_reduce.hpp"' in source
    assert "constexpr int kTile = %d;" % T in shared and "constexpr int kBlock = %d;" % W in shared


@pytest.mark.parametrize("n", sorted({1, 2, 63, 64, 65, W - 1, W + 1, T - 1, T, T + 1, 2 * T + 1}))
def test_sizes(n):
    run_and_check(scene(n, 2, 3, seed=n), what="n=%d" % n)


def test_one_cell_of_three_fragments_and_a_bit():
    counts, out, _ = run_and_check(scene(3 * T + 5, [4], [2], seed=1), what="one cell")
    assert counts["cells"] == 1 and counts["receivers"] == 1


def test_a_cell_per_row_more_fragments_than_waves():
    n = T + 1
    counts, out, _ = run_and_check(scene(n, np.arange(n)[::-1] // 16, np.arange(n) % 16, seed=2), what="cell per row")
    assert counts["cells"] == n and np.all(np.diff(out["cell_ptr"]) == 1)


def test_a_cell_that_starts_on_a_tiles_last_position():
    n = T + 40
    tx = np.where(np.arange(n) < T - 1, 0, 1)
    counts, out, _ = run_and_check(scene(n, [0], tx, seed=3), what="last position")
    assert out["cell_ptr"].tolist() == [0, T - 1, n]


def test_a_receiver_across_two_tile_boundaries_whose_cells_cross_none():
    per = T // 4
    tx = np.r_[np.arange(10 * per) // per, np.zeros(30, int)]
    rx = np.r_[np.zeros(10 * per, int), np.ones(30, int)]
    order = np.random.default_rng(4).permutation(len(rx))
    counts, out, _ = run_and_check(scene(len(rx), rx[order], tx[order], seed=4), what="receiver run")
    assert out["cell_ptr"][:11].tolist() == [per * k for k in range(11)] and out["rx_count"].tolist() == [10 * per, 30]


def test_ids_at_the_ends_of_int32_sort_signed():
    ids = np.array([I32.min, -5, 0, 7, I32.max])
    g = np.random.default_rng(5)
    counts, out, _ = run_and_check(scene(300, ids[g.integers(0, 5, 300)], ids[g.integers(0, 5, 300)], seed=5), what="int32 ends")
    assert out["rx_id"].tolist() == ids.tolist() and counts["cells"] == 25
    assert out["cell_tx"][:5].tolist() == ids.tolist() and np.all(out["cell_rx"][:5] == I32.min)


def test_minute_boundaries():
    cols = scene(4, [0], [0], seed=6)
    cols["timestamp"] = np.array([0.0, 59.999999, 60.0, 120.0])
    counts, out, _ = run_and_check(cols, what="minutes")
    assert counts["time0"] == 0.0 and out["minute_hist"].tolist() == [2, 1, 1]
    cols = scene(2 * T + 3, [0], [0], seed=7)        # the same inside the LDS counters of a whole-tile fragment
    cols["timestamp"][:] = np.sort(np.r_[0.0, np.tile([59.999999, 60.0, 120.0], (2 * T + 3) // 3 + 1)[:2 * T + 2]])
    run_and_check(cols, what="minutes, whole tiles")


def test_a_minute_range_wider_than_the_lds_counters_falls_back():
    cols = scene(2 * T + 10, [0], [0], seed=8)
    cols["timestamp"][-1] = cols["timestamp"][0] + 5000 * 60.0 + 1.0
    counts, out, _ = run_and_check(cols, what="fallback")
    assert counts["minute_bins"] == out["minute_ptr"][1] > 4096 and out["minute_hist"][-1] == 1
    cols = scene(2 * T, [0], [0], seed=21)      # the cell's range is too wide, each whole tile's own window is not
    cols["timestamp"][T:] += 6000 * 60.0
    counts, out, _ = run_and_check(cols, what="tile window")
    assert counts["minute_bins"] > 6000 and out["minute_hist"][:16].sum() == T == out["minute_hist"][6000:].sum()
    cols = scene(2 * T + 10, [0], [0], seed=9)       # and a carrier-bin range that is
    cols["carrier_bin"][T + 5] = 9000
    counts, out, _ = run_and_check(cols, what="bin fallback")
    assert counts["carrier_bins"] > 4096


def test_offset_histogram_edges():
    cols = scene(T + 30, 2, 2, seed=10)
    cols["offset"][:] = 0.125
    counts, out, _ = run_and_check(cols, what="all equal")
    assert np.all(out["offset_edges"][:, 0] == -0.375) and np.all(out["offset_hist"][:, 5] == np.diff(out["cell_ptr"]))
    cols = scene(T + 30, [0], [0], seed=11)
    cols["offset"][::7] = cols["offset"].max()
    counts, out, _ = run_and_check(cols, what="max repeated")
    assert out["offset_hist"][0, 9] >= len(cols["offset"][::7])
    for lo, hi in ((-0.5, 0.5), (0.1, 0.7), (-3.0, 1e-3)):
        cols = scene(3 * 11, [0], [0], seed=12)
        cols["offset"][:] = np.tile(np.linspace(lo, hi, 11), 3)
        counts, out, _ = run_and_check(cols, what="on every edge")
        assert out["offset_hist"][0].tolist() == [3] * 9 + [6]


def test_nan_and_inf_stay_in_their_cell():
    cols = scene(2 * T, 2, 3, seed=13)
    clean = _native.toadstats(cols)[1]
    cell = np.flatnonzero((cols["rxid"] == 1) & (cols["txid"] == 0))
    cols["energy"][cell[3]] = np.nan
    cols["carrier_offset"][cell[5]] = np.inf
    counts, out, _ = run_and_check(cols, what="nan / inf")
    c = int(np.flatnonzero((out["cell_rx"] == 1) & (out["cell_tx"] == 0))[0])
    assert np.isnan(out["stats"][c, 5]).all() and np.isnan(out["stats"][c, 7]).all()       # energy, its dB
    assert out["stats"][c, 4, 0] == np.inf and np.isnan(out["stats"][c, 4, 1]) and out["stats"][c, 4, 3] == np.inf
    others = np.arange(counts["cells"]) != c
    assert out["stats"][others].tobytes() == clean["stats"][others].tobytes()
    assert out["stats"][c, :4].tobytes() == clean["stats"][c, :4].tobytes()


def test_zero_noise():
    cols = scene(80, 2, 2, seed=14)
    cols["noise"][5] = 0.0
    cols["carrier_noise"][9] = 0.0
    cols["carrier_energy"][9] = 0.0
    counts, out, _ = run_and_check(cols, what="zero noise")
    assert out["snr_db"][5, 1] == np.inf and np.isnan(out["snr_db"][9, 0])


def test_a_non_finite_offset_is_flagged():
    cols = scene(T + 9, [0], np.arange(T + 9) % 3, seed=15)
    cols["offset"][4] = np.nan
    cols["offset"][5] = -np.inf
    counts, out, _ = run_and_check(cols, what="offset flag")
    assert out["cell_flags"].tolist() == [0, _native.TSTATS_FLAG_OFFSET_NONFINITE, _native.TSTATS_FLAG_OFFSET_NONFINITE]
    assert np.isnan(out["offset_edges"][1:]).all() and not out["offset_hist"][1:].any()
    assert out["offset_hist"][0].sum() == out["cell_ptr"][1]


def test_receivers_without_a_line():
    cols = scene(40, np.r_[np.zeros(37, int), 1, 2, 2], 2, seed=16)
    cols["soa"][38:] = 123456.5
    counts, out, _ = run_and_check(cols, what="no line")
    assert out["rx_count"].tolist() == [37, 1, 2]
    assert np.isfinite(out["rx_fit"][0]).all() and np.isnan(out["rx_fit"][1:]).all() and np.isnan(out["residual"][37:]).all()


def test_selections():
    cols = scene(2 * T + 7, 2, 3, seed=17)
    sel = np.arange(0, 2 * T + 7, 2)
    counts, out, _ = run_and_check(cols, sel, what="every other row")
    assert counts["rows"] == len(sel) and set(out["order"].tolist()) == set(sel.tolist())
    run_and_check(cols, np.array([2 * T + 6]), what="one row")
    with pytest.raises(ValueError, match="selection is empty"):
        _native.toadstats(cols, np.zeros(0, np.int64))


def test_the_three_errors_and_the_bin_limit():
    cols = scene(50, 2, 2, seed=18)
    with pytest.raises(ValueError, match="out of range"):
        _native.toadstats(cols, [0, 50])
    with pytest.raises(ValueError, match="strictly ascending"):
        _native.toadstats(cols, [3, 2])
    bad = dict(cols, timestamp=cols["timestamp"].copy())
    bad["timestamp"][7] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        _native.toadstats(bad)
    assert _native.toadstats(bad, [0, 1, 2])[0]["rows"] == 3        # outside the selection: not looked at
    wide = dict(cols, carrier_bin=cols["carrier_bin"].copy())
    wide["carrier_bin"][0], wide["carrier_bin"][1] = I32.min, I32.max
    wide["rxid"], wide["txid"] = np.zeros(50, np.int32), np.zeros(50, np.int32)
    before = _native.live_resources()
    with pytest.raises(ValueError, match=r"exceed 2\^26 bins"):
        _native.toadstats(wide)
    assert _native.live_resources() == before


def test_resources_return_to_baseline_and_fetch_wants_the_exact_size():
    import ctypes as C
    cols = scene(T + 1, 2, 2, seed=19)
    _native.toadstats(cols)
    before = _native.live_resources()
    lib = _native.load_library()
    arrays = [np.ascontiguousarray(cols[name], dtype=kind) for name, kind in _native.TSTATS_COLUMNS]
    handle, counts = C.c_void_p(), _native.ThrTstatsCounts()
    assert lib.thr_toadstats(0, T + 1, *[a.ctypes.data for a in arrays], None, 0, C.byref(handle), C.byref(counts)) == 0
    held = _native.live_resources()
    assert held[0] >= before[0] + len(_native.TSTATS_OUTPUTS) and held[3] == before[3] + 2
    rx = np.zeros(counts.cells, np.int32)
    assert lib.thr_tstats_fetch(handle, 0, rx.ctypes.data, rx.nbytes) == 0
    assert lib.thr_tstats_fetch(handle, 0, rx.ctypes.data, rx.nbytes + 4) == _native.ERR_ARG
    assert lib.thr_tstats_fetch(handle, len(_native.TSTATS_OUTPUTS), rx.ctypes.data, rx.nbytes) == _native.ERR_ARG
    lib.thr_tstats_free(handle)
    assert _native.live_resources() == before
    times = _native.toadstats_times()
    assert len(times) == 5 and all(t >= 0 for t in times) and times[1] > 0
