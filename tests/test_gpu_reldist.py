"""thr_reldist against the reference's recorded runs (tests/golden/reldist) and the NumPy statement
(tests/reldist_ref.py), over all rows of all cells: indices, hi, flags, raw, x, the three masks, medians and MADs,
counts, the rows within one std, speeds and dopplers exactly; mean and std within syncstats_ref's rounding bounds;
the smoothed curves within the measured tolerance (reldist_ref.SMOOTH_RTOL); two runs bit for bit; one cell alone
and inside a 12-cell call bit for bit; the command line's file."""
import numpy as np
import pytest

import reldist_ref as R
import reldist_scenes as SC
from thrifty_amd import _native, reldist, toads_data

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", SC.NAMES)
@pytest.mark.parametrize("method", ["nearest", "linpol"])
def test_fixture_cells_are_the_references_and_the_statements(name, method):
    g = SC.load(name)
    args, kwargs = SC.golden_input(g, method)
    got = _native.reldist(*args, **kwargs)
    assert SC.check_against_fixture(got[1], g, method, name) >= 1
    R.assert_same(got, R.reldist_ref(*args, **kwargs), what=(name, method))


def test_lists_of_mobiles_and_receivers_and_no_geometry():
    g = SC.load("d")
    args, _ = SC.golden_input(g)
    for kw in (dict(beacons=[7]), dict(beacons=[0, 7], mobiles=[2], receivers=[5, 0, 2]), dict(beacons=[0], mobiles=[1, 7]),
               dict(beacons=[0, 7], receivers=[1, 2], method="nearest", smooth_frac=0.0, thresh=2.0),
               dict(beacons=[3], sample_rate=2.0e6, block_len=8192, carrier_hz=868e6)):
        got = _native.reldist(*args, **kw)
        R.assert_same(got, R.reldist_ref(*args, **kw), kw.get("sample_rate", 2.4e6), str(kw))
    assert np.all(got[1]["cell_flags"] == R.CELL_NO_BEACON) and np.all(np.isnan(got[1]["x"]))      # no match of transmitter 3
    with pytest.raises(ValueError, match="selection is empty"):
        _native.reldist(*args, beacons=[0], mobiles=[9])


def test_two_runs_are_bit_identical_and_resources_come_back():
    args, kwargs = SC.golden_input(SC.load("d"))
    before = _native.live_resources()
    first = _native.reldist(*args, **kwargs)
    second = _native.reldist(*args, **kwargs)
    assert first[0] == second[0] and all(first[1][k].tobytes() == second[1][k].tobytes() for k in _native.RELDIST_OUTPUTS)
    assert _native.live_resources() == before
    assert len(_native.reldist_times()) == 5 and all(ms >= 0 for ms in _native.reldist_times())


def test_one_cell_alone_and_inside_a_twelve_cell_call_agree_bit_for_bit():
    args, kwargs = SC.golden_input(SC.load("d"), smooth_frac=0.2)
    many = _native.reldist(*args, **dict(kwargs, receivers=[0, 1, 5]))
    assert many[0]["cells"] == 12
    alone = _native.reldist(*args, **dict(kwargs, beacons=[0], mobiles=[1], receivers=[1, 5]))
    assert alone[0]["cells"] == 1 and alone[1]["cell_key"].tolist() == [[1, 0, 1, 5]]
    ci = many[1]["cell_key"].tolist().index([1, 0, 1, 5])
    assert 0 < ci < 11
    for ptr, names in (("cell_ptr", ("row_det", "row_match", "nearest_idx", "hi", "row_flags", "raw", "x", "mask1", "dop", "mask3")),
                       ("speed_ptr", ("speed_x", "speed", "mask2")), ("speed_smooth_ptr", ("speed_smooth_x", "speed_smooth")),
                       ("dop_smooth_ptr", ("dop_smooth_x", "dop_smooth"))):
        a, b = many[1][ptr][ci:ci + 2]
        assert b - a == alone[1][ptr][1] > 10
        for name in names:
            assert many[1][name][a:b].tobytes() == alone[1][name].tobytes(), name
    for name in ("cell_stats", "cell_counts", "medians", "cell_flags"):
        assert many[1][name][ci].tobytes() == alone[1][name][0].tobytes(), name


def test_rel_dist_object_and_the_command_lines_file(tmp_path, capsys):
    g = SC.load("e")
    toads, match, out = tmp_path / "rx.toads", tmp_path / "rx.match", tmp_path / "r.npz"
    toads.write_text("".join("%d %d %.6f %d %.8f 7 0.25 500.0 10.0 %d %r 120.0 6.0\n" % (rx, tx, ts, i, soa, cbin, float(coff))
                             for i, (rx, tx, ts, soa, cbin, coff) in enumerate(zip(
                                 g["rxid"], g["txid"], g["timestamp"], g["soa"], g["carrier_bin"], g["carrier_offset"]))))
    match.write_text("".join(" ".join(str(d) for d in g["match_idx"][a:b]) + "\n" for a, b in zip(g["match_ptr"][:-1], g["match_ptr"][1:])))
    for name, pos in (("pos-rx.cfg", "0: 0 0\n1: 8964.1335967 0\n"), ("pos-beacon.cfg", "0: 4939.6 1500\n")):
        (tmp_path / name).write_text(pos)
    argv = [str(toads), str(match), "--beacon", "0", "-r", str(tmp_path / "pos-rx.cfg"), "-b", str(tmp_path / "pos-beacon.cfg")]
    assert reldist._main(argv + ["--all", "-o", str(out)]) == 0
    text = capsys.readouterr().out
    with open(toads, "rb") as f:
        detections = toads_data.toads_array(toads_data.load_toads(f), with_ids=True)
    matches = [g["match_idx"][a:b].tolist() for a, b in zip(g["match_ptr"][:-1], g["match_ptr"][1:])]
    result = reldist.rel_dist(detections, matches, [0], rx_pos={0: (0.0, 0.0), 1: (8964.1335967, 0.0)}, beacon_pos={0: (4939.6, 1500.0)})
    assert text == "# Mobile 1 relative to beacon 0 at RX 0 and RX 1\n" + result.format_report(0)
    assert text.splitlines()[1].startswith("Number of outliers: ") and not text.splitlines()[1].startswith("Number of outliers: 0 ")
    with np.load(out) as f:
        assert str(f["method"]) == "linpol" and float(f["sample_rate"]) == 2.4e6
        for name in _native.RELDIST_OUTPUTS:
            assert f[name].tobytes() == getattr(result, name).tobytes(), name
    assert reldist._main(argv + ["--tx", "1", "--method", "nearest"]) == 0
    assert capsys.readouterr().out.startswith("Number of outliers: ")
    assert reldist._main(argv + ["--tx", "4"]) == 1
    assert "selection is empty" in capsys.readouterr().err
    cell = result.cell(1, 0, 0, 1)
    assert cell["flags"] == 0 and abs(cell["mean"]) < 9000.0 and 0 < cell["std"] < 2000.0        # metres along the baseline
