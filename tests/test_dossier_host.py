"""Detection dossiers without a GPU: the NumPy statement (tests/dossier_ref.py) and the package's views
against the reference's recorded drawings (tests/golden/dossier/), the pick rule, the ABI additions and the
command line's argument handling."""
import os
import re

import numpy as np
import pytest

import dossier_golden as G
import dossier_ref as R
from thrifty_amd import _native, build, detect_analysis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The fixtures hold the reference's numbers: its samples are complex64 and its rms / magnitudes inherit that
# (a few float32 roundings, 6e-8 each), and long series are stored as float32.  Eight float32 epsilons.
FIXTURE_TOL = 8 * 2.0 ** -23
DOSSIER_SYMBOLS = ["thr_dossier_create", "thr_dossier_destroy", "thr_dossier_reset", "thr_dossier_feed",
                   "thr_dossier_feed_card", "thr_dossier_feed_stream", "thr_dossier_result", "thr_dossier_geometry"]


@pytest.fixture(scope="module", params=G.SCENES)
def scene(request):
    g, fx = G.load_scene(request.param), G.load(request.param)
    settings = R.scene_settings(g)
    pos = {int(b): i for i, b in enumerate(g["block_idx"])}
    dossiers = [R.dossier(g["blocks"][pos[int(b)]], int(b), settings, float(fx["sample_rate"])) for b in fx["kept"]]
    return request.param, g, fx, settings, dossiers


def test_the_statement_keeps_the_blocks_the_reference_keeps(scene):
    _, g, fx, settings, dossiers = scene
    assert all(d is not None for d in dossiers)
    detected = [R.numbers(b, int(i), settings)[0] for i, b in zip(g["block_idx"], g["blocks"])]
    assert detected == [bool(v) for v in g["det"]]
    kept, checked, skipped, _ = R.pick(g["block_idx"], detected, [(0, None)], len(detected))
    assert [int(g["block_idx"][k]) for k in kept] == [int(b) for b in fx["kept"]]
    assert (checked, skipped) == (len(detected), len(detected) - len(kept))


def test_every_view_reproduces_the_reference_drawing(scene):
    name, _, fx, _, dossiers = scene
    assert sorted(detect_analysis.PLOT_COMMANDS) == [str(v) for v in fx["views"]]
    worst = ("", 0.0)
    for k, d in enumerate(dossiers):
        for what, err in G.view_errors(d, fx, k):
            assert err <= FIXTURE_TOL, (name, k, what, err)
            worst = max(worst, (what, err), key=lambda t: t[1])
    print(name, "worst view error", worst)


def test_the_fit_reproduces_the_reference_fit(scene):
    _, _, fx, _, dossiers = scene
    for k, d in enumerate(dossiers):
        sc = d.data["scalars"]
        assert sc["fit_valid"] == 1
        assert abs(sc["fit_amplitude"] - fx["fit_amplitude"][k]) <= FIXTURE_TOL * fx["fit_amplitude"][k]
        assert abs(sc["fit_offset"] - fx["fit_offset"][k]) <= FIXTURE_TOL


def test_the_filter_statement_is_the_lfilter_form():
    # carrier_detect._filter: sqrt(lfilter(w^2 reversed, 1, m^2)) behind its delay
    from scipy.signal import lfilter
    rng = np.random.default_rng(3)
    n, w = 1024, 100
    mag = rng.random(n) + 0.1
    f, w2 = R.filter_weights2(n, w)
    assert f == 20 and abs(np.sum(w2) - 1) < 1e-12 and np.allclose(w2, w2[::-1], rtol=0, atol=1e-16)
    want = np.sqrt(lfilter(w2[::-1], 1, mag ** 2))[f // 2:]
    got = R.filtered_spectrum(mag, n, w)
    assert got.shape == (n - f // 2,) and np.allclose(got, want, rtol=1e-13, atol=0)


def test_compensated_samples_are_the_inverse_transform_of_the_shifted_spectrum():
    g = G.load_scene("small")
    settings = R.scene_settings(g)
    _, result, x, data = R.numbers(g["blocks"][0], int(g["block_idx"][0]), settings)
    from oracle import thrifty_np as onp
    shift = -(result.carrier_info.bin + result.carrier_info.offset)
    assert G.rel_l2(data["synced"], np.fft.ifft(onp.shift_and_fft(x, shift))) < 1e-12


@pytest.mark.parametrize("name", ["small", "c2"])
def test_the_statement_at_the_oracles_own_record_is_the_statement(name):
    """numbers_at() runs no detector; fed the record numbers() found it must give numbers()'s data: arrays to
    float64 round-off (1e-12 relative), integers and flags exactly."""
    settings, ref = G.ref_numbers(name)
    g = G.load_scene(name)
    seen = 0
    for block, (_, result, _, want) in zip(g["blocks"], ref):
        if want is None:
            continue
        got = R.numbers_at(block, R.record_of(result), settings)
        seen += 1
        assert sorted(got) == sorted(want)
        assert np.array_equal(got["hist"], want["hist"]) and np.array_equal(got["autocorr"], want["autocorr"])
        for key in ("fft_mag", "filtered", "synced", "synced_fft_mag", "corr"):
            assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype, key
            assert np.array_equal(got[key], want[key]) or G.rel_l2(got[key], want[key]) <= 1e-12, key
        gs, ws = got["scalars"], want["scalars"]
        assert sorted(gs) == sorted(ws)
        for key, w in ws.items():
            if key in ("fit_valid", "peak_start", "peak_len"):
                assert gs[key] == w and isinstance(gs[key], int), key
            elif key == "corr_shifted":
                assert np.array_equal(gs[key], w) or G.rel_l2(gs[key], w) <= 1e-12
            else:
                assert gs[key] == w or abs(gs[key] - w) <= 1e-12 * abs(w), key
    assert seen == int(np.sum(g["carrier_det"]))


def test_the_statement_at_a_record_follows_the_record():
    """... and it is the record's numbers it uses, not a detector's: another bin, sample and noise move the fit's
    validity, the peak window and the thresholds."""
    g = G.load_scene("small")
    settings = R.scene_settings(g)
    _, result, _, want = R.numbers(g["blocks"][0], int(g["block_idx"][0]), settings)
    rec = dict(R.record_of(result), carrier_bin=4, corr_sample=2, carrier_noise=2.0, corr_noise=3.0)
    sc = R.numbers_at(g["blocks"][0], rec, settings)["scalars"]
    assert sc["fit_valid"] == 0 and np.isnan(sc["fit_offset"]) and (sc["peak_start"], sc["peak_len"]) == (0, 8)
    assert sc["carrier_threshold"] == np.sqrt(12 * 4.0) and sc["corr_threshold"] == np.sqrt(12 * 9.0)
    assert sc["rms_unsynced"] == want["scalars"]["rms_unsynced"]
    off = R.numbers_at(g["blocks"][0], R.record_of(result), settings, fit=False)["scalars"]
    assert off["fit_valid"] == 1 and np.isnan(off["fit_amplitude"]) and np.isnan(off["fit_offset"])


PICK_CASES = [      # scene c2: block_idx 5 + 3 i, blocks 53 56 59 62 not detected
    ("8-20,50-", 6, [8, 11, 14, 17, 20, 50], 6, 0),
    ("47-65", 20, [47, 50, 65], 7, 4),
    ("-11,62-", 4, [5, 8, 11, 65], 5, 1),
    ("200-", 20, [], 0, 0),
]


@pytest.mark.parametrize("ranges, max_keep, kept, checked, skipped", PICK_CASES)
def test_pick_rule_on_c2(ranges, max_keep, kept, checked, skipped):
    g = G.load_scene("c2")
    got = R.pick(g["block_idx"], g["det"], detect_analysis.parse_range_list(ranges), max_keep)
    assert [int(g["block_idx"][k]) for k in got[0]] == kept and got[1:3] == (checked, skipped)


def test_pick_rule_reports_carrier_only_blocks_as_skipped():
    g = G.load_scene("c1")
    assert list(g["carrier_det"][6:8]) == [True, True] and list(g["det"][6:8]) == [False, False]
    kept, checked, skipped, lines = R.pick(g["block_idx"], g["det"], [(106, 107)], 5)
    assert kept == [] and (checked, skipped) == (2, 2)
    assert lines == ["Checking block #106", "Skipping block #106", "Checking block #107", "Skipping block #107"]


def test_pick_lines_are_the_reference_lines():
    g, fx = G.load_scene("small"), G.load("small")
    assert str(fx["cli_args"]) == "-i 40-50 -m 3"
    kept, _, _, lines = R.pick(g["block_idx"], g["det"], detect_analysis.parse_range_list("40-50"), 3)
    assert lines == [str(v) for v in fx["cli_lines"]]
    assert [int(g["block_idx"][k]) for k in kept] == [int(v) for v in fx["cli_kept"]]


@pytest.mark.parametrize("text, want", [
    ("1", [(1, 1)]), ("1-100", [(1, 100)]), ("1-", [(1, None)]), ("-100", [(None, 100)]),
    ("1-5, 20-30", [(1, 5), (20, 30)]),
])
def test_parse_range_list(text, want):
    assert detect_analysis.parse_range_list(text) == want


def test_parse_range_list_refuses_what_is_no_range():
    for text in ("a", "1-2-3", "1,b", "3 4"):
        with pytest.raises(ValueError):
            detect_analysis.parse_range_list(text)


def test_block_in_range():
    ranges = detect_analysis.parse_range_list("-3,7,10-12,20-")
    inside = [b for b in range(25) if detect_analysis.block_in_range(b, ranges)]
    assert inside == [0, 1, 2, 3, 7, 10, 11, 12, 20, 21, 22, 23, 24]


def test_abi_additions_are_declared_exported_and_built():
    header = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
    assert re.search(r"#define THR_ABI_VERSION 11\b", header) and _native.ABI_VERSION == 11
    lib = _native.load_library()
    assert lib.thr_abi_version() == 11
    for sym in DOSSIER_SYMBOLS:
        assert re.search(r"\b%s\(" % sym, header) and sym in _native.EXPORTS and getattr(lib, sym), sym
    assert "dossier.hip" in build.SOURCES and "dossier.hpp" in build.HEADERS
    assert build.UNPROFILED_DOSSIER == ("dossier.hip", "dossier.hpp")
    # the binding's view of thr_dossier_scalars: 10 doubles, 4 ints, 11 doubles
    assert _native.DOSSIER_SCALARS_DTYPE.itemsize == 10 * 8 + 4 * 4 + 11 * 8
    assert re.search(r"double corr_shifted\[11\];", header)


def test_csrc_hash_does_not_see_the_dossier_kernels(monkeypatch):
    with_dossier = build.csrc_hash()
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "dossier.hip"])
    monkeypatch.setattr(build, "HEADERS", [h for h in build.HEADERS if h != "dossier.hpp"])
    assert build.csrc_hash() == with_dossier


def test_public_names_mirror_the_reference_module():
    for name in ("ForcibleDetector", "DetectorResult", "parse_range_list", "block_in_range", "_main", "analyze", "Dossier"):
        assert hasattr(detect_analysis, name), name
    assert detect_analysis.DetectorResult._fields == ("detected", "result", "unsynced", "synced", "corr")
    assert len(detect_analysis.PLOT_COMMANDS) == 18
    assert sorted(detect_analysis.FIGURE_COMMANDS) == ["corrs", "overlays", "overview", "spectra", "time"]
    for views in detect_analysis.FIGURE_COMMANDS.values():
        assert set(views) <= set(detect_analysis.PLOT_COMMANDS)


def test_figures_are_tuples_of_views():
    g = G.load_scene("small")
    d = R.dossier(g["blocks"][0], int(g["block_idx"][0]), R.scene_settings(g))
    fig = d.figure("corrs")
    assert [v.name for v in fig] == ["corr", "corr_zoomed", "corr_interpol", "corr_shifted"]
    with pytest.raises(KeyError):
        d.view("nonsense")


def test_save_keys_are_the_references():
    g = G.load_scene("small")
    d = R.dossier(g["blocks"][0], int(g["block_idx"][0]), R.scene_settings(g))
    saved = detect_analysis.save_arrays(d)
    assert sorted(saved) == ["carrier_info", "corr", "corr_info", "synced", "template", "unsynced"]
    assert sorted(saved["carrier_info"]) == ["bin", "energy", "noise", "offset"]
    assert sorted(saved["corr_info"]) == ["energy", "noise", "offset", "sample"]
    arrays = detect_analysis.view_arrays(d, ["corr_shifted", "time"])
    assert {"corr_shifted.line0.y", "corr_shifted.line1.y", "iq.line0.x", "mag_synced.hlines"} <= set(arrays)


def _card(tmp_path):
    path = tmp_path / "in.card"
    path.write_text(str(G.load_scene("small")["card_text"]))
    return str(path)


def test_export_is_refused_with_one_sentence(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as exc:
        detect_analysis._main([_card(tmp_path), "--export", "p"])
    said = str(exc.value)
    assert "--export" in said and said.count(".") == 1 and said.endswith(".") and "\n" not in said


@pytest.mark.parametrize("extra", [["-m", "0"], ["-p", "overview,nonsense"]])
def test_argument_errors_are_reported(tmp_path, monkeypatch, extra):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as exc:
        detect_analysis._main([_card(tmp_path)] + extra)
    assert "analyze_detect" in str(exc.value)


def test_a_range_that_is_none_is_an_argument_error(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as exc:
        detect_analysis._main([_card(tmp_path), "-i", "4-x"])
    assert exc.value.code == 2 and "-i/--blocks" in capsys.readouterr().err
