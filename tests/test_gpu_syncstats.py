"""thr_beaconsync and thr_tdoastats against the reference's recorded runs (tests/golden/syncstats) and the NumPy
restatement (tests/syncstats_ref.py): rows, discontinuities, cuts, masks, min, max and the report's text exactly;
residuals within max(2 polyfit_distance, 32 u max|soa1|) of the exact ones; means, stds, RMS and snr within their
rounding bounds; integer SOAs at the threshold's ties; two runs bit for bit; resources given back."""
import numpy as np
import pytest

import syncstats_golden as G
import syncstats_ref as R
from thrifty_amd import _native, beacon_analysis, tdoa_analysis

pytestmark = pytest.mark.gpu

DISCRETE = ("cell_key", "cell_ptr", "row_det", "row_match", "disc_ptr", "disc_idx", "cut_ptr", "cut_left", "cut_right",
            "cut_flags", "cell_counts", "cell_flags")


def same_discrete(out, ref, what=""):
    for name in DISCRETE:
        assert np.array_equal(out[name], ref[name]), (what, name)
    assert out["sdoa"].tobytes() == ref["sdoa"].tobytes(), what                      # one subtraction
    assert np.array_equal(out["cut_disc_soa"], ref["cut_disc_soa"], equal_nan=True), what
    assert np.array_equal(np.isnan(out["residual"]), np.isnan(ref["residual"])), what


@pytest.mark.parametrize("name,deg", [(n, d) for n in ("realistic", "slow_rx1") for d in (1, 2, 3)])
def test_fixture_cells_are_the_references(name, deg):
    g = G.load(name)
    counts, out = _native.beaconsync(G.beacon_columns(g), g["match_ptr"], g["match_idx"], deg, beacons=G.BEACONS)
    ref_counts, ref = G.restated(name, deg)
    assert counts == ref_counts
    same_discrete(out, ref, name)
    worst = G.check_beacon(counts, out, G.exact(name, deg), g, deg, name)
    dist = R.residual_distances(G.beacon_columns(g), out, G.exact(name, deg))
    print("%s deg %d: device residuals at most %.3g from the exact ones (%.2f of the floor); np.polyfit %.3g"
          % (name, deg, max([d for d, _ in dist.values()] or [0.0]), worst,
             max([float(np.max(v)) for k, v in g.items() if k.endswith("deg%d_polyfit_distance" % deg) and len(v)] or [0.0])))


def test_every_transmitter_without_a_list_and_receiver_and_range_filters():
    g = G.load("realistic")
    cols = G.beacon_columns(g)
    counts, out = _native.beaconsync(cols, g["match_ptr"], g["match_idx"], 2)
    ref_counts, ref = R.beacon_sync_ref(cols, g["match_ptr"], g["match_idx"], 2)
    assert counts == ref_counts and counts["cells"] == 12
    same_discrete(out, ref, "all")
    for kw in (dict(receivers=[2, 0]), dict(beacons=[1, 1, 3], receivers=[1, 2]), dict(id_range=(200, 700)),
               dict(id_range=(int(g["idx"][-1]), int(g["idx"][-1]) + 5), beacons=[])):
        try:
            want = R.beacon_sync_ref(cols, g["match_ptr"], g["match_idx"], 2, **kw)
        except ValueError:
            with pytest.raises(ValueError, match="selection is empty"):
                _native.beaconsync(cols, g["match_ptr"], g["match_idx"], 2, **kw)
            continue
        got = _native.beaconsync(cols, g["match_ptr"], g["match_idx"], 2, **kw)
        assert got[0] == want[0], kw
        same_discrete(got[1], want[1], str(kw))
        R.assert_beacon_within_bounds(cols, got[1], R.exact_beacon_values(cols, got[1], 2), None, str(kw))


def test_analyze_prints_the_references_text_and_returns_its_coefficients(capsys):
    g = G.load("realistic")
    detections = np.zeros(len(g["soa"]), dtype=[("idx", "i4"), ("soa", "f8"), ("energy", "f8"), ("noise", "f8")])
    for name in detections.dtype.names:
        detections[name] = g[name]
    for deg in (1, 2, 3):
        tag = "b1_0_2_deg%d_" % deg
        coefs = beacon_analysis.analyze(detections, g[tag + "matrix"], deg=deg)
        assert capsys.readouterr().out == str(g[tag + "text"])
        assert len(coefs) == len(g[tag + "coefs"]) and all(c.shape == (deg + 1,) for c in coefs)
        a = int(g[tag + "cut_left"][0])
        soa = g["soa"][g[tag + "matrix"]]
        n = int(np.flatnonzero(np.diff(soa[:, 1] - soa[:, 0]) > 1000)[0])       # the first cut: rows a .. n
        fit = sum(float(c) * soa[a:n, 0] ** (deg - k) for k, c in enumerate(coefs[0]))
        assert np.max(np.abs(soa[a:n, 1] - fit)) < 1.0      # a float64 evaluation of raw powers: coarse, but the same curve
    s = G.load("slow_rx1")
    detections = np.zeros(len(s["soa"]), dtype=detections.dtype)
    for name in detections.dtype.names:
        detections[name] = s[name]
    with pytest.raises(ValueError, match="nothing can be fitted"):
        beacon_analysis.analyze(detections, s["b0_0_1_deg2_matrix"])
    assert capsys.readouterr().out == str(s["b0_0_1_deg2_text"]) + beacon_analysis.NO_FIT_TEXT + "\n"


def test_sync_stats_object_and_saved_file(tmp_path):
    g = G.load("realistic")
    matches = [g["match_idx"][a:b].tolist() for a, b in zip(g["match_ptr"][:-1], g["match_ptr"][1:])]
    sync = beacon_analysis.sync_stats(G.beacon_columns(g), matches, beacons=G.BEACONS, deg=2)
    assert len(sync) == 6 and sync.format_report(1) == str(g["b0_0_2_deg2_text"])
    cell = sync.cell(0, 0, 2)
    assert [cut["number"] for cut in cell["cuts"]] == [1, 2, 4] and cell["discontinuities"].tolist() == [31, 78, 82]
    assert all(len(cut["residual"]) == cut["right"] - cut["left"] and cut["coef"].shape == (3,) for cut in cell["cuts"])
    sync.save(tmp_path / "sync.npz")
    with np.load(tmp_path / "sync.npz") as f:
        assert np.array_equal(f["residual"], sync.residual, equal_nan=True) and int(f["deg"]) == 2


def integer_cell(step):
    """21 rows, sdoa steps of 1 except one of `step` at index 7: every sum is exact in any order."""
    sdoa = np.cumsum(np.r_[0.0, np.where(np.arange(20) == 7, float(step), 1.0)])
    soa0 = 1.0e6 * np.arange(21)
    cols = {"rxid": np.tile(np.array([0, 1], np.int32), 21), "txid": np.zeros(42, np.int32),
            "soa": np.column_stack([soa0, soa0 + 5000.0 + sdoa]).reshape(-1), "energy": np.full(42, 300.0),
            "noise": np.full(42, 10.0), "idx": np.arange(42, dtype=np.int64)}
    return cols, 2 * np.arange(22, dtype=np.int64), np.arange(42, dtype=np.int64)


@pytest.mark.parametrize("step,mean,want", [(19, 1.9, []), (20, 1.95, [7])])
def test_integer_soas_decide_the_threshold_at_its_tie(step, mean, want):
    cols, ptr, idx = integer_cell(step)
    counts, out = _native.beaconsync(cols, ptr, idx, 1)
    assert out["cell_stats"][0, 0] == mean == np.mean(np.diff(out["sdoa"]))      # 19 > 19.0 is false, 20 > 19.5 true
    assert out["disc_idx"].tolist() == want
    same_discrete(out, R.beacon_sync_ref(cols, ptr, idx, 1)[1], "step %d" % step)


@pytest.mark.parametrize("robust", [False, True])
def test_tdoa_fixture_is_the_references(robust):
    g = G.load("tdoa")
    counts, out = _native.tdoastats(G.tdoa_columns(g), robust=robust)
    G.check_tdoa(counts, out, g, "device")
    ref_counts, ref = R.tdoa_stats_ref(G.tdoa_columns(g), robust=robust)
    assert counts == ref_counts
    for name in ("median", "mask", "robust_count"):
        assert np.array_equal(out[name], ref[name], equal_nan=True), name
    if robust:
        assert np.array_equal(out["robust_stats"][:, 3:], ref["robust_stats"][:, 3:])
        stats = tdoa_analysis.tdoa_stats(G.tdoa_columns(g), robust=True)
        cell = stats.cell(0, 1, 3)
        assert cell["robust"]["count"] == cell["count"] - int(cell["outlier"].sum()) < cell["count"]
        assert cell["robust"]["std"] < cell["std"]
    else:
        assert all(len(out[name]) == 0 for name in ("robust_stats", "robust_count", "mask", "median"))


def test_two_runs_are_bit_identical_and_resources_come_back():
    g, t = G.load("realistic"), G.load("tdoa")
    before = _native.live_resources()
    first = _native.beaconsync(G.beacon_columns(g), g["match_ptr"], g["match_idx"], 3)
    second = _native.beaconsync(G.beacon_columns(g), g["match_ptr"], g["match_idx"], 3)
    assert first[0] == second[0] and all(first[1][k].tobytes() == second[1][k].tobytes() for k in _native.BSYNC_OUTPUTS)
    first = _native.tdoastats(G.tdoa_columns(t), robust=True)
    second = _native.tdoastats(G.tdoa_columns(t), robust=True)
    assert first[0] == second[0] and all(first[1][k].tobytes() == second[1][k].tobytes() for k in _native.TDSTATS_OUTPUTS)
    with pytest.raises(ValueError, match="selection is empty"):
        _native.tdoastats(G.tdoa_columns(t), timestamp=(0.0, 1.0))
    assert _native.live_resources() == before
    assert all(ms >= 0 for which in ("beaconsync", "tdoastats") for ms in _native.syncstats_times(which))


def test_both_command_lines_on_files(tmp_path, capsys):
    g, t = G.load("realistic"), G.load("tdoa")
    toads, match, tdoa = tmp_path / "data.toads", tmp_path / "data.match", tmp_path / "data.tdoa"
    toads.write_text("".join("%d %d %.6f %d %.8f 7 0.25 %r %r 41 0.1 120.0 6.0\n" % (rx, tx, 1.7e9 + i, i, soa, float(en), float(no))
                             for i, (rx, tx, soa, en, no) in enumerate(zip(g["rxid"], g["txid"], g["soa"], g["energy"], g["noise"]))))
    match.write_text("".join(" ".join(str(d) for d in g["match_idx"][a:b]) + "\n"
                             for a, b in zip(g["match_ptr"][:-1], g["match_ptr"][1:])))
    assert beacon_analysis._main([str(toads), str(match), "--beacon", "1", "--rx0", "2", "--rx1", "0", "--deg", "3"]) == 0
    assert capsys.readouterr().out == str(g["b1_0_2_deg3_text"])
    out = tmp_path / "sync.npz"
    assert beacon_analysis._main([str(toads), str(match), "--all", "-o", str(out)]) == 0
    text = capsys.readouterr().out
    assert text.count("# Beacon ") == 12 and "# Beacon 0 at RX 0 and RX 2\n" + str(g["b0_0_2_deg2_text"]) in text
    with np.load(out) as f:
        assert f["cell_key"].shape == (12, 3) and int(f["deg"]) == 2
    first = int(g["b0_0_1_deg2_matrix"][10, 0])
    assert beacon_analysis._main([str(toads), str(match), "--range", "%d-%d" % (first, first + 300)]) == 0
    assert "Number of detection groups: " in capsys.readouterr().out
    assert beacon_analysis._main([str(toads), str(match), "--beacon", "9"]) == 1
    assert "selection is empty" in capsys.readouterr().err
    tdoa.write_text("".join("%d %.6f %d %d %d %r 30.0 1.0 %d %d\n" % (i, ts, tx, rx0, rx1, float(v * 1e9), d0, d1) for i, (ts, tx, rx0, rx1, v, d0, d1)
                            in enumerate(zip(t["timestamp"], t["tx"], t["rx0"], t["rx1"], t["tdoa"], t["det0_idx"], t["det1_idx"]))))
    assert tdoa_analysis._main([str(tdoa), "--rx0", "1", "--rx1", "0", "--tx", "3", "--robust"]) == 0     # descending: swapped
    text = capsys.readouterr().out
    assert text.startswith(str(t["text"][1]) + "Without 3 outliers:\nTDOA bias: ")
    assert tdoa_analysis._main([str(tdoa), "--all"]) == 0
    assert capsys.readouterr().out.count("TDOA RMS: ") == 11
    assert tdoa_analysis._main([str(tdoa), "--tx", "9"]) == 1
