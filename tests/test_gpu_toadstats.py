"""The detection statistics on the device (thr_toadstats, thrifty_amd.toads_analysis) against the reference's
recorded run (tests/golden/toadstats).  Every discrete output equals the fixture's; min, max and the histogram
edges are equal bit for bit; means and stds are within Higham's bound for a sum in any order of the exact
values ((m + 2) u mean|x| and (m + 4) u (std + mean|x|), u = 2^-53, m the cell's count); the dB columns are
within toadstats_golden.DB_ULPS_LIMIT ulps of NumPy's and their statistics are held to exact values computed
from the fetched columns; the line and its residuals are within (rows + 8) u max|timestamp| of the exact
least-squares line.  The command line prints the reference's text."""
import numpy as np
import pytest

import toadstats_golden as G
import toadstats_ref as R
from thrifty_amd import _native, matchmaker, toads_analysis

pytestmark = pytest.mark.gpu

CASES = [(name, "") for name in G.NAMES] + [("realistic", "m_")]


@pytest.fixture(scope="module")
def golden():
    return {name: G.load(name) for name in G.NAMES}


@pytest.fixture(scope="module")
def computed(golden):
    """toad_stats of every case, once"""
    out = {}
    for name, prefix in CASES:
        g = golden[name]
        out[name, prefix] = toads_analysis.toad_stats(G.columns(g), G.matches(g) if prefix else None)
    return out


def arrays_of(stats):
    return {name: getattr(stats, name) for name in _native.TSTATS_OUTPUTS}


@pytest.mark.parametrize("name,prefix", CASES)
def test_fixture_through_toad_stats(golden, computed, name, prefix):
    stats = computed[name, prefix]
    ulps = G.check(stats.counts, arrays_of(stats), golden[name], prefix, name + prefix)
    print("%s%s: dB columns at most %.2f ulps from NumPy's (limit %.1f)" % (name, prefix, ulps, G.DB_ULPS_LIMIT))
    assert ulps <= G.DB_ULPS_LIMIT


@pytest.mark.parametrize("name,prefix", CASES)
def test_tables_and_cells(golden, computed, name, prefix):
    g, stats = golden[name], computed[name, prefix]
    txids, rxids, counts = toads_analysis.count_table(stats)
    assert np.array_equal(txids, g[prefix + "table_txids"]) and np.array_equal(rxids, g[prefix + "rx_id"])
    assert np.array_equal(counts, g[prefix + "count_table"])
    assert np.array_equal(toads_analysis.mean_energy_table(stats)[2], g[prefix + "mean_energy_table"])
    cell = stats.cell(int(stats.cell_rx[0]), int(stats.cell_tx[0]))
    at = (np.searchsorted(txids, stats.cell_tx[0]), np.searchsorted(rxids, stats.cell_rx[0]))
    assert cell["count"] == counts[at] and np.array_equal(cell["offset_hist"], g[prefix + "offset_hist"][0])


def test_a_second_call_returns_the_same_bits(golden, computed):
    for name, prefix in CASES:
        g = golden[name]
        again = toads_analysis.toad_stats(G.columns(g), G.matches(g) if prefix else None)
        for out in _native.TSTATS_OUTPUTS:
            assert getattr(again, out).tobytes() == getattr(computed[name, prefix], out).tobytes(), (name, out)
        assert again.time0 == computed[name, prefix].time0


# ------------------------------------------------------------------ the command line
def toads_text(g, with_txid=True):
    lines = []
    for i in range(len(g["rxid"])):
        ids = "%d %d " % (g["rxid"][i], g["txid"][i]) if with_txid else "%d " % g["rxid"][i]
        lines.append(ids + "%.6f %d %.8f %d %r %r %r %d %r %r %r" % (
            g["timestamp"][i], i, g["soa"][i], 17, float(g["offset"][i]), float(g["energy"][i]), float(g["noise"][i]),
            g["carrier_bin"][i], float(g["carrier_offset"][i]), float(g["carrier_energy"][i]), float(g["carrier_noise"][i])))
    return "\n".join(lines) + "\n"


def reference_text(g, prefix):
    want = "Timestamps relative to {:.6f}\n".format(float(g[prefix + "time0"]))
    for rx, tx, body in zip(g[prefix + "cell_rx"], g[prefix + "cell_tx"], g[prefix + "text"]):
        want += "# Stats for RX #{}'s detections of TX #{}'s transmissions:\n\n".format(rx, tx) + str(body) + "\n\n"
    return want


@pytest.mark.parametrize("name,prefix", CASES)
def test_main_prints_the_references_text(golden, computed, name, prefix, tmp_path, capsys):
    g = golden[name]
    toads = tmp_path / "data.toads"
    toads.write_text(toads_text(g))
    argv = ["-i", str(toads), "-o", str(tmp_path / "stats.npz")]
    if prefix:
        with open(tmp_path / "data.match", "w") as handle:
            matchmaker.save_matches(G.matches(g), handle)
        argv += ["-m", str(tmp_path / "data.match")]
    assert toads_analysis._main(argv) == 0
    assert capsys.readouterr().out == reference_text(g, prefix) == toads_analysis.format_stats(computed[name, prefix])
    saved = np.load(tmp_path / "stats.npz")
    for out in _native.TSTATS_OUTPUTS:      # the file round-trips the text's columns exactly: the same bits
        assert saved[out].tobytes() == getattr(computed[name, prefix], out).tobytes(), out
    assert float(saved["time0"]) == computed[name, prefix].time0


def test_toad_input_is_one_cell(golden, tmp_path, capsys):
    """Deviation: --toad input has no ids; the reference's split raises, here it is the one cell (-1, -1)."""
    g = golden["sparse"]
    toad = tmp_path / "rx0.toad"
    toad.write_text(toads_text(g, with_txid=False))
    assert toads_analysis._main(["--toad", "--input", str(toad)]) == 0
    text = capsys.readouterr().out
    cols = dict(G.columns(g), rxid=np.full(len(g["rxid"]), -1), txid=np.full(len(g["rxid"]), -1))
    counts, ref = R.toad_stats_ref(cols)
    assert text.count("# Stats for RX #-1's detections of TX #-1's transmissions:") == 1 == counts["cells"]
    assert "Number of detections: %d\n" % len(g["rxid"]) in text
    stats = toads_analysis.toad_stats(cols)
    assert len(stats) == 1 and np.array_equal(stats.order, np.arange(len(g["rxid"])))
    assert np.array_equal(stats.stats[:, G.NOT_DB, 2:], ref["stats"][:, G.NOT_DB, 2:])
    exact = R.exact_values(cols, None, stats.snr_db)
    R.assert_stats_within_bounds(stats.stats, exact["cells"], stats.cell_ptr, "toad")
    R.assert_fit_within_bounds(stats.rx_fit, stats.residual, exact, cols, None, "toad")


def test_detection_objects_and_arrays_are_accepted(golden, computed):
    from thrifty_amd import toads_data
    g = golden["sparse"]
    dets = toads_data._read(toads_text(g).splitlines(), True, True)
    for source in (dets, toads_data.toads_array(dets)):
        stats = toads_analysis.toad_stats(source)
        for out in _native.TSTATS_OUTPUTS:
            assert getattr(stats, out).tobytes() == getattr(computed["sparse", ""], out).tobytes(), out


def test_empty_selection_says_so(golden):
    """Deviation: the reference's np.min raises 'zero-size array to reduction operation'."""
    with pytest.raises(ValueError, match="selection is empty"):
        toads_analysis.toad_stats(G.columns(golden["sparse"]), matches=[])
