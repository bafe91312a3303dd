"""thr_tdoamatrix against the runs of the reference's scripts/tdoa_matrix.py (tests/golden/tdoa_matrix), through the
native call, through tdoa_matrix.tdoa_matrices and through the command line.  Every cell is compared:
 - exact: cell keys, pointers, flags, counts, det / match / timestamp rows, statuses, n_window, n_kept, the mask;
 - rows: every TDOA within ref_err_max of the exact least-squares value and within 2 ref_err_max of the reference's,
   snr relative 1e-14, model_quality relative 1e-12 (tdoa_golden.check_against_fixture's rule); tdmat_nearest bit for bit;
 - the mask also equals is_outlier applied on the host to the device's OWN TDOAs;
 - statistics within the rounding bounds of the exact statistics of the device's own kept rows, and within those
   bounds + 2 ref_err_max * 2.997e8 of the reference's std and mean;
 - the tables equal the script's printed numbers wherever the fixture says the rounding is firm."""
import numpy as np
import pytest

import tdoa_matrix_golden as G
from thrifty_amd import _native, tdoa_matrix

pytestmark = pytest.mark.gpu

_got = {}


def device(name):
    if name not in _got:
        g = G.load(name)
        kw = G.arguments(g)
        kw["model"] = _native.TDOA_MODELS[kw["model"]]
        _got[name] = _native.tdoamatrix(G.columns(g), g["match_ptr"], g["match_idx"], **kw)
    return _got[name]


@pytest.mark.parametrize("name", G.SETS)
def test_fixture_cells_through_the_native_call(name):
    g = G.load(name)
    counts, out = device(name)
    assert counts["cells"] == len(g["cell_key"]) and counts["tasks"] == len(g["status"])
    assert counts["tdoas"] == int(np.sum(g["status"] == G.OK))
    G.check_structure(out, g, name)
    G.check_rows(out, g, name)
    G.check_own_mask_and_stats(out, name)
    G.check_reference_stats(out, g, name)


@pytest.mark.parametrize("name", G.SETS)
def test_fixture_cells_through_tdoa_matrices(name):
    g = G.load(name)
    counts, out = device(name)
    result = tdoa_matrix.tdoa_matrices(G.columns(g), G.matches(g), **G.arguments(g))
    assert result.counts == counts and result.beacons == sorted(g["beacons"].tolist())
    for key in _native.TDMAT_OUTPUTS:
        assert getattr(result, key).tobytes() == out[key].tobytes(), key
    G.check_tables(result, g, name)
    c = int(np.argmax(g["table_count"]))
    cell = result.cell(*g["cell_key"][c].tolist())
    a, b = g["cell_ptr"][c:c + 2]
    assert cell["kept"] == g["table_count"][c] and np.array_equal(cell["outlier"], g["outlier"][a:b] != 0)
    assert np.array_equal(cell["timestamp"], g["task_timestamp"][a:b]) and len(cell["tdoa"]) == b - a


@pytest.mark.parametrize("name", G.SETS)
def test_fixture_cells_through_the_command_line(name, tmp_path, capsys):
    g = G.load(name)
    toads, match, out = tmp_path / "data.toads", tmp_path / "data.match", tmp_path / "m.npz"
    toads.write_text("".join("%d %d %.6f %d %r 7 0.25 %r %r 40 0.1 120.0 6.0\n" % (rx, tx, ts, i, float(soa), float(en), float(no))
                             for i, (rx, tx, ts, soa, en, no) in enumerate(zip(
                                 g["rxid"], g["txid"], g["timestamp"], g["soa"], g["energy"], g["noise"]))))
    match.write_text("".join(" ".join(str(d) for d in g["match_idx"][a:b]) + "\n" for a, b in zip(g["match_ptr"][:-1], g["match_ptr"][1:])))
    argv = [str(toads), str(match), "--beacons"] + [str(b) for b in g["beacons"].tolist()] + ["--model", str(g["model"]), "-o", str(out)]
    assert tdoa_matrix._main(argv) == 0
    text = capsys.readouterr().out
    counts, want = device(name)
    with np.load(out) as f:
        assert str(f["model"]) == str(g["model"]) and float(f["window"]) == 4.0 and f["beacons"].tolist() == sorted(g["beacons"].tolist())
        for key in _native.TDMAT_OUTPUTS:
            assert f[key].tobytes() == want[key].tobytes(), key
    result = tdoa_matrix.TdoaMatrices(counts, want, g["beacons"].tolist(), str(g["model"]))
    assert text == "".join(result.format_report(rx0, rx1) for rx0, rx1 in result.pairs) and text.count("# TDOA count matrix") == len(result.pairs)
    if len(g["receivers"]) > 2:         # one pair alone: the same cells, bit for bit
        rx0, rx1 = result.pairs[-1]
        assert tdoa_matrix._main(argv[:-2] + ["--rx0", str(rx1), "--rx1", str(rx0)]) == 0
        assert capsys.readouterr().out == result.format_report(rx0, rx1)


def test_real_geometry_moves_the_mean_by_the_beacons_tdoa():
    g = G.load("tdmat_realistic")
    rng = np.random.default_rng(5)
    rx_pos = {int(r): rng.uniform(-1000, 1000, 2) for r in g["receivers"]}
    beacon_pos = {int(b): rng.uniform(-1000, 1000, 2) for b in g["beacons"]}
    zero = tdoa_matrix.tdoa_matrices(G.columns(g), G.matches(g), **G.arguments(g))
    real = tdoa_matrix.tdoa_matrices(G.columns(g), G.matches(g), rx_pos=rx_pos, beacon_pos=beacon_pos, **G.arguments(g))
    np.testing.assert_array_equal(real.status, zero.status)
    checked = 0
    for c, (rx0, rx1, b, _) in enumerate(real.cell_key.tolist()):
        shift = np.linalg.norm(rx_pos[rx0] - beacon_pos[b]) - np.linalg.norm(rx_pos[rx1] - beacon_pos[b])
        a, e = real.cell_ptr[c:c + 2]
        if real.cell_counts[c, 4] and np.array_equal(real.outlier[a:e], zero.outlier[a:e]):
            # x = soa1 + beacon_sdoa moves the fit's argument: every TDOA moves by the beacon's own, up to the clocks'
            # rate difference (some 1e-5 of it)
            assert abs((real.cell_stats[c, 0] - zero.cell_stats[c, 0]) - shift) < 1e-3 * max(1.0, abs(shift)), (c, shift)
            checked += 1
    assert checked >= 0.9 * len(real)


def test_two_runs_are_bit_identical_and_resources_come_back():
    g = G.load("tdmat_edges")
    kw = dict(G.arguments(g), model=0)
    before = _native.live_resources()
    first = _native.tdoamatrix(G.columns(g), g["match_ptr"], g["match_idx"], **kw)
    second = _native.tdoamatrix(G.columns(g), g["match_ptr"], g["match_idx"], **kw)
    assert first[0] == second[0] and all(first[1][k].tobytes() == second[1][k].tobytes() for k in _native.TDMAT_OUTPUTS)
    assert _native.live_resources() == before
    assert len(_native.tdoamatrix_times()) == 5 and all(ms >= 0 for ms in _native.tdoamatrix_times())
