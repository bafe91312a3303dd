"""Detection dossiers on the device (csrc/dossier.hip): the pick, the kept samples, the
result-time series and scalars, the views and the command line.

Picks are exact: kept block indices, n_checked, n_skipped, and the slots' records byte for byte those the
feed returned.  Series are held to the NumPy statement tests/dossier_ref.py (float64, on the project's
oracle) at the bound tests/test_gpu_parity.py holds the stage dumps to, relative L2 error 5e-6; thresholds,
rms values and line values at 1e-4 relative, the fit offset at the carrier-offset tolerance 2e-4.  The fit
amplitude and the shifted correlation peak have no tolerance of older standing: they were measured against
the reference's recorded numbers (tests/golden/dossier) on the four scenes, and the bound is four times the
largest error seen (the factor covers float32 inputs that differ from box to box):
    fit amplitude     largest relative error 9.75e-8 (c2_stddev) -> TOL_FIT_AMP      = 3.9e-7
    corr_shifted      largest error 2.37e-7 (c2)                 -> TOL_CORR_SHIFTED = 9.5e-7   (of the window's peak)
Per scene (small, c2, c2_stddev, c1): fit amplitude 6.27e-8, 9.35e-8, 9.75e-8, 9.67e-8; corr_shifted 2.16e-7,
2.37e-7, 2.35e-7, 1.67e-7.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import dossier_golden as G
import dossier_ref as R
from thrifty_amd import _native as F
from thrifty_amd import block_data, detect_analysis, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_SERIES = 5e-6           # relative L2, the stage dumps' bound (tests/test_gpu_parity.py)
TOL_REL = 1e-4              # thresholds, rms values, line values
TOL_COFF = 2e-4             # fit offset: the project's carrier-offset tolerance
TOL_FIT_AMP = 3.9e-7        # measured, see above
TOL_CORR_SHIFTED = 9.5e-7   # measured, see above
ALL = ((None, None),)


def engine_of(settings, max_batch=64, **kw):
    return F.Engine(settings.block_len, settings.history_len, settings.template, settings.carrier_thresh,
                    settings.carrier_window, settings.corr_thresh, carrier_len=settings.carrier_len,
                    max_batch=max_batch, **kw)


@pytest.fixture(scope="module")
def engines():
    """engines(scene, **override): one engine per scene and threshold override for the whole module."""
    made = {}

    def get(scene, **override):
        key = (scene, tuple(sorted(override.items())))
        if key not in made:
            made[key] = engine_of(R.scene_settings(G.load_scene(scene), **override))
        return made[key]

    yield get
    for eng in made.values():
        eng.close()


def stamps_of(g):
    return 1000.0 + 0.5 * np.arange(len(g["block_idx"]))


def feed_all(eng, g, ranges, max_keep, batch=None):
    """-> (Dossiers, the records of all feeds)"""
    d = F.Dossiers(eng, ranges, max_keep)
    nb = len(g["blocks"])
    step = batch or nb
    ts = stamps_of(g)
    recs = [d.feed(g["blocks"][i:i + step], ts[i:i + step], g["block_idx"][i:i + step]) for i in range(0, nb, step)]
    return d, np.concatenate(recs)


# ------------------------------------------------------------------ picks (exact)
@pytest.mark.parametrize("ranges, max_keep, kept, checked, skipped", [
    ("8-20,50-", 6, [8, 11, 14, 17, 20, 50], 6, 0),
    ("47-65", 20, [47, 50, 65], 7, 4),
    ("-11,62-", 4, [5, 8, 11, 65], 5, 1),
])
def test_picks_on_c2(engines, ranges, max_keep, kept, checked, skipped):
    g = G.load_scene("c2")
    with feed_all(engines("c2"), g, detect_analysis.parse_range_list(ranges), max_keep)[0] as d:
        assert (d.n_kept, d.n_checked, d.n_skipped) == (len(kept), checked, skipped)
        got = d.result(arrays=())
        assert [int(v) for v in got["records"]["block_idx"]] == kept
        pos = [list(g["block_idx"]).index(b) for b in kept]
        assert [int(p) for p in got["positions"]] == pos
        assert np.array_equal(got["timestamps"], stamps_of(g)[pos])
        plain = engines("c2").detect(g["blocks"], g["block_idx"])[:, 0]
        assert got["records"].tobytes() == plain[pos].tobytes()


def test_nothing_in_range_keeps_nothing(engines):
    g = G.load_scene("c2")
    with feed_all(engines("c2"), g, detect_analysis.parse_range_list("200-"), 20)[0] as d:
        assert (d.n_kept, d.n_checked, d.n_skipped) == (0, 0, 0)
        got = d.result()
        assert len(got["records"]) == 0 and got["fft_mag"].shape == (0, 16384) and got["scalars"].shape == (0,)


def test_forced_thresholds_keep_every_block(engines):
    g = G.load_scene("c2")
    eng = engines("c2", carrier_thresh=(0, 0, 0), corr_thresh=(0, 0, 0))
    with feed_all(eng, g, ALL, 24)[0] as d:
        assert (d.n_kept, d.n_checked, d.n_skipped) == (24, 24, 0)
        assert np.array_equal(d.result(arrays=())["records"]["block_idx"], g["block_idx"])


def test_carrier_without_correlation_is_skipped_on_c1(engines):
    g = G.load_scene("c1")
    d, recs = feed_all(engines("c1"), g, [(106, 107)], 5)
    with d:
        assert np.all(recs["flags"][6:8] & F.FLAG_CARRIER) and not np.any(recs["flags"][6:8] & F.FLAG_CORR)
        assert (d.n_kept, d.n_checked, d.n_skipped) == (0, 2, 2)
    with feed_all(engines("c1"), g, ALL, 20)[0] as d:
        assert [int(v) for v in d.result(arrays=())["records"]["block_idx"]] == [100, 101, 102, 103, 108, 109, 110, 111]
        assert (d.n_checked, d.n_skipped) == (12, 4)


def test_feeding_on_after_the_slots_are_full_changes_nothing(engines):
    g = G.load_scene("c2")
    d, _ = feed_all(engines("c2"), g, ALL, 3)
    with d:
        before = (d.n_kept, d.n_checked, d.n_skipped)
        assert before == (3, 3, 0)
        first = d.result()
        d.feed(g["blocks"][4:9], stamps_of(g)[4:9], g["block_idx"][4:9])
        assert (d.n_kept, d.n_checked, d.n_skipped) == before
        again = d.result()
        for name in first:
            assert first[name].tobytes() == again[name].tobytes(), name


# ------------------------------------------------------------------ batching and input routes
def everything(d):
    got = d.result()
    return (d.n_kept, d.n_checked, d.n_skipped), {k: v.tobytes() for k, v in got.items()}


def test_the_result_does_not_depend_on_the_batching(engines):
    g = G.load_scene("c2")
    ranges = detect_analysis.parse_range_list("8-59,65-")
    runs = []
    for batch in (1, 5, 24):
        d, _ = feed_all(engines("c2"), g, ranges, 17, batch)
        with d:
            runs.append(everything(d))
    # through the .card route: base64 text decoded on the device
    ts = stamps_of(g)
    text = "".join(block_data.card_line(float(t), int(i), b) for t, i, b in zip(ts, g["block_idx"], g["blocks"])).encode()
    chars = ((2 * 16384 + 2) // 3) * 4
    off, at = [], 0
    for line in text.split(b"\n")[:-1]:
        off.append(at + len(line) - chars)
        at += len(line) + 1
    with F.Dossiers(engines("c2"), ranges, 17) as d:
        for lo in (0, 10):
            hi = 10 if lo == 0 else 24
            d.feed_card(text, off[lo:hi], ts[lo:hi], g["block_idx"][lo:hi])
        runs.append(everything(d))
    kept, checked, skipped, _ = R.pick(g["block_idx"], g["det"], ranges, 17)
    assert runs[0][0] == (len(kept), checked, skipped) == (17, 20, 3)
    for other in runs[1:]:
        assert other[0] == runs[0][0]
        for name in runs[0][1]:
            assert other[1][name] == runs[0][1][name], name


def test_a_raw_stream_gives_what_its_framed_blocks_give(engines):
    g = G.load_scene("c2")
    eng = engines("c2")
    n, h = 16384, int(g["history_len"])
    stream = np.ascontiguousarray(g["blocks"][:8]).reshape(-1)
    stride = 2 * (n - h)
    nb = (stream.size - 2 * n) // stride + 1
    framed = np.stack([stream[i * stride:i * stride + 2 * n] for i in range(nb)])
    ts = 5.0 + np.arange(nb)
    with F.Dossiers(eng, ALL, 6) as a, F.Dossiers(eng, ALL, 6) as b:
        ra = a.feed_stream(stream, 300, ts)
        rb = np.concatenate([b.feed(framed[:3], ts[:3], 300 + np.arange(3)), b.feed(framed[3:], ts[3:], 303 + np.arange(nb - 3))])
        assert ra.tobytes() == rb.tobytes() and a.n_kept >= 2
        ea, eb = everything(a), everything(b)
        assert ea[0] == eb[0]
        for name in ea[1]:
            assert ea[1][name] == eb[1][name], name


# ------------------------------------------------------------------ series and scalars
@pytest.mark.parametrize("scene", G.SCENES)
def test_series_and_scalars_match_the_statement(engines, scene):
    g, fx = G.load_scene(scene), G.load(scene)
    settings, ref = G.ref_numbers(scene)
    with feed_all(engines(scene), g, ALL, len(g["blocks"]))[0] as d:
        got = d.result()
        assert (d.filter_width, d.filtered_len) == (2 * (settings.block_len // settings.carrier_len),
                                                    settings.block_len - settings.block_len // settings.carrier_len)
    assert [int(v) for v in got["records"]["block_idx"]] == [int(v) for v in fx["kept"]]
    assert G.rel_l2(got["autocorr"], R.autocorr(settings.template)) < 1e-13
    worst, missed = {}, []

    def note(name, err, tol):        # (every figure is printed before any is asserted)
        worst[name] = max(worst.get(name, 0.0), float(err))
        if not err <= tol:
            missed.append((scene, name, float(err), tol))

    half = d.filter_width // 2
    for k, pos in enumerate(int(p) for p in got["positions"]):
        detected, _, _, want = ref[pos]
        assert detected
        assert np.array_equal(got["hist"][k], want["hist"])
        for name in ("fft_mag", "filtered", "synced", "synced_fft_mag", "corr"):
            note(name, G.rel_l2(got[name][k], want[name]), TOL_SERIES)
        # the filter's lead-in (its first F/2 outputs see the zeros below bin 0) and its last output
        note("filtered lead-in", G.rel_l2(got["filtered"][k][:half], want["filtered"][:half]), TOL_SERIES)
        note("filtered end", abs(got["filtered"][k][-1] - want["filtered"][-1]) / want["filtered"][-1], TOL_SERIES)
        sc, ws = got["scalars"][k], want["scalars"]
        for name in ("rms_unsynced", "rms_synced", "carrier_threshold", "corr_threshold"):
            note(name, abs(sc[name] - ws[name]) / ws[name], TOL_REL)
        for name in ("fft_std", "synced_fft_std", "filtered_std", "corr_std"):
            if ws[name]:
                note(name, abs(sc[name] - ws[name]) / ws[name], TOL_REL)
            else:
                assert sc[name] == 0
        assert sc["fit_valid"] == 1 and (sc["peak_start"], sc["peak_len"]) == (ws["peak_start"], ws["peak_len"])
        note("fit_offset", abs(sc["fit_offset"] - fx["fit_offset"][k]), TOL_COFF)
        # against the reference's own numbers (the fixture)
        note("fit_amplitude", abs(sc["fit_amplitude"] - fx["fit_amplitude"][k]) / fx["fit_amplitude"][k], TOL_FIT_AMP)
        shifted = fx["corr_shifted|0|y"][k][:sc["peak_len"]]        # (c1 has peaks 3 and 4 samples from an end)
        assert len(shifted) == fx["corr_shifted|0|len"][k] and not np.isnan(shifted).any()
        note("corr_shifted", np.max(np.abs(sc["corr_shifted"][:sc["peak_len"]] - shifted)) / np.max(shifted), TOL_CORR_SHIFTED)
    print("MEASURED", scene, " ".join("%s=%.2e" % kv for kv in sorted(worst.items())))
    assert not missed, missed


# ------------------------------------------------------------------ edges
EDGE_N, EDGE_W = 1024, 127


def edge_template():
    return np.asarray(np.load(os.path.join(G.HERE, "golden", "template_extract", "extract_1024.npz"))["template"],
                      dtype=np.float64)


def check_against_statement(got, k, block, block_idx, settings):
    detected, _, _, want = R.numbers(block, block_idx, settings)
    assert detected
    assert np.array_equal(got["hist"][k], want["hist"])
    for name in ("fft_mag", "filtered", "synced", "synced_fft_mag", "corr"):
        assert G.rel_l2(got[name][k], want[name]) <= TOL_SERIES, name
    for name in ("rms_unsynced", "rms_synced", "carrier_threshold", "corr_threshold"):
        assert abs(got["scalars"][k][name] - want["scalars"][name]) <= TOL_REL * want["scalars"][name], name
    return want


def test_a_carrier_bin_below_six_has_no_fit_but_everything_else():
    tpl = edge_template()
    settings = R.DetectorSettings(EDGE_N, 512, EDGE_W, (0, 15, 0), (2, 5), tpl, (0, 15, 0))
    blocks, _ = synth.synth_blocks(np.random.default_rng(41), 4, EDGE_N, tpl, (193, 705), carriers=[4.2, 4.4, 4.6, 4.8])
    eng = engine_of(settings)
    try:
        with F.Dossiers(eng, ALL, 4) as d:
            recs = d.feed(blocks, None, np.arange(4))
            assert d.n_kept == 4 and np.all(recs["carrier_bin"] < 6)
            got = d.result()
        for k in range(4):
            sc = got["scalars"][k]
            assert sc["fit_valid"] == 0 and np.isnan(sc["fit_amplitude"]) and np.isnan(sc["fit_offset"])
            want = check_against_statement(got, k, blocks[k], k, settings)
            assert want["scalars"]["fit_valid"] == 0
            err = np.max(np.abs(sc["corr_shifted"] - want["scalars"]["corr_shifted"])) / np.max(want["scalars"]["corr_shifted"])
            print("MEASURED edge corr_shifted %.2e" % err)
            assert err <= TOL_CORR_SHIFTED, err
    finally:
        eng.close()


@pytest.mark.parametrize("where", ["end", "start"])
def test_the_peak_window_is_clipped_at_the_ends_of_the_correlation(where):
    tpl = edge_template()
    corr_len = EDGE_N - EDGE_W + 1
    # history = template_len - 1: the unique window is the whole correlation, so a peak may sit at either end
    settings = R.DetectorSettings(EDGE_N, EDGE_W - 1, EDGE_W, (0, 15, 0), (2, 60), tpl, (0, 15, 0))
    positions = [corr_len - 3, corr_len - 1] if where == "end" else [2, 0]
    blocks, _ = synth.synth_blocks(np.random.default_rng(43), 2, EDGE_N, tpl, (0, corr_len), positions=positions,
                                   carrier_bins=(10.0, 50.0))
    eng = engine_of(settings)
    try:
        with F.Dossiers(eng, ALL, 2) as d:
            recs = d.feed(blocks, None, np.arange(2))
            assert d.n_kept == 2 and [int(v) for v in recs["corr_sample"]] == positions
            got = d.result()
        for k, p in enumerate(positions):
            sc = got["scalars"][k]
            start, stop = max(0, p - 5), min(corr_len, p + 6)
            assert (sc["peak_start"], sc["peak_len"]) == (start, stop - start) and stop - start < 11
            want = check_against_statement(got, k, blocks[k], k, settings)["scalars"]
            assert (want["peak_start"], want["peak_len"]) == (start, stop - start)
            err = np.max(np.abs(sc["corr_shifted"] - want["corr_shifted"])) / np.max(want["corr_shifted"])
            print("MEASURED clipped corr_shifted %.2e" % err)
            assert err <= TOL_CORR_SHIFTED, err
            assert np.all(sc["corr_shifted"][stop - start:] == 0)
    finally:
        eng.close()


# ------------------------------------------------------------------ views, command line
def small_items(g):
    return [(float(t), int(i), b) for t, i, b in zip(stamps_of(g), g["block_idx"], g["blocks"])]


def test_views_of_the_first_kept_block_of_small_match_the_recorded_drawings():
    g, fx = G.load_scene("small"), G.load("small")
    settings = R.scene_settings(g)
    dossiers = detect_analysis.analyze(small_items(g), settings, [(0, None)], 2, float(fx["sample_rate"]))
    assert [d.result.block for d in dossiers] == [int(v) for v in fx["kept"][:2]]
    derived = {"carrier_peak_unsynced line 1 y": TOL_FIT_AMP + TOL_COFF, "carrier_peak_unsynced line 1 x": TOL_COFF,
               "carrier_peak_unsynced vline": TOL_COFF, "corr_shifted line 0 y": TOL_CORR_SHIFTED,
               "corr_shifted line 1 y": TOL_CORR_SHIFTED}
    for what, err in G.view_errors(dossiers[0], fx, 0):
        tol = derived.get(what, TOL_SERIES if " line " in what else TOL_REL)
        assert err <= tol, (what, err, tol)
    assert np.allclose(dossiers[0].unsynced, R.onp.iq_u8_to_c64(g["blocks"][0]), rtol=0, atol=1e-7)


def test_forcible_detector_answers_one_block():
    g = G.load_scene("small")
    settings = R.scene_settings(g)
    fd = detect_analysis.ForcibleDetector(settings, force_carrier=True, force_corr=True)
    try:
        assert fd.settings.carrier_thresh == (0, 0, 0) and fd.settings.corr_thresh == (0, 0, 0)
        for pos in (4, 0):          # block 48 is not detected unless forced
            r = fd(7.0, int(g["block_idx"][pos]), g["blocks"][pos])
            assert r.detected and r.result.block == int(g["block_idx"][pos]) and r.synced.shape == (4096,)
            assert np.allclose(np.abs(r.synced), np.abs(R.onp.iq_u8_to_c64(g["blocks"][pos])), rtol=0, atol=1e-6)
    finally:
        fd.close()


def test_the_command_line_end_to_end(tmp_path):
    g, fx = G.load_scene("small"), G.load("small")
    (tmp_path / "in.card").write_text(str(g["card_text"]))
    np.save(tmp_path / "tpl.npy", g["template"])
    argv = [sys.executable, "-m", "thrifty_amd.detect_analysis", "in.card", "-i", "40-50", "-m", "3", "--save", "p",
            "--views", "p", "-z", "tpl.npy", "-b", "4096", "-y", str(int(g["history_len"])), "-w", "5-60", "-t", "12*snr",
            "-u", "12*snr", "-s", "2.2M", "-p", "corrs,fft"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    done = subprocess.run(argv, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr
    said = [line for line in done.stdout.splitlines() if line.startswith(("Checking", "Skipping"))]
    assert said == [str(v) for v in fx["cli_lines"]]
    _, ref = G.ref_numbers("small")
    for k, block in enumerate(int(v) for v in fx["cli_kept"]):
        saved = np.load(tmp_path / ("p_%d.npz" % block), allow_pickle=True)
        assert sorted(saved.files) == ["carrier_info", "corr", "corr_info", "synced", "template", "unsynced"]
        want = ref[list(g["block_idx"]).index(block)][3]
        assert G.rel_l2(saved["synced"], want["synced"]) <= TOL_SERIES
        assert G.rel_l2(saved["corr"], want["corr"]) <= TOL_SERIES
        # ... and the fixture's own series (float32), where it stores this block
        if k < int(fx["n_full"]):
            assert G.rel_l2(np.real(saved["synced"]), fx["iq_synced|0|y"][k]) <= TOL_SERIES
            assert G.rel_l2(np.abs(saved["corr"]), fx["corr|0|y"][k]) <= TOL_SERIES
        views = np.load(tmp_path / ("p_%d_views.npz" % block))
        assert {"corr.line0.y", "corr_shifted.line1.y", "fft.hlines", "fft.vlines"} <= set(views.files)
    assert len(list(tmp_path.glob("p_*.npz"))) == 6


# ------------------------------------------------------------------ arguments, resources
def test_create_refuses_bad_arguments(engines):
    g = G.load_scene("c2")
    eng = engines("c2")
    for ranges, max_keep in ([[(0, 1)] * 17, 5], [ALL, 0], [ALL, (256 << 20) // (8 * 16384) + 1]):
        with pytest.raises(F.NativeError) as exc:
            F.Dossiers(eng, ranges, max_keep)
        assert "(code %d)" % F.ERR_ARG in str(exc.value)
    F.Dossiers(eng, [(0, 1)] * 16, (256 << 20) // (8 * 16384)).close()
    settings = R.scene_settings(g)
    for kw in (dict(preshift_num=21), dict(fastdet=True)):
        other = engine_of(settings._replace(carrier_thresh=(100.0, 2.0, 0), corr_thresh=(100.0, 2.0, 0)), **kw)
        try:
            with pytest.raises(F.NativeError) as exc:
                F.Dossiers(other, ALL, 5)
            assert "(code %d)" % F.ERR_ARG in str(exc.value)
        finally:
            other.close()
    two = engine_of(settings._replace(template=np.stack([settings.template, settings.template[::-1]])))
    try:
        with pytest.raises(F.NativeError) as exc:
            F.Dossiers(two, ALL, 5)
        assert "(code %d)" % F.ERR_ARG in str(exc.value)
    finally:
        two.close()


def test_a_dossier_takes_one_sample_format(engines):
    g = G.load_scene("c2")
    with F.Dossiers(engines("c2"), ALL, 5) as d:
        d.feed(g["blocks"][:2], None, g["block_idx"][:2])
        with pytest.raises(F.NativeError) as exc:
            d.feed(np.stack([R.onp.iq_u8_to_c64(b) for b in g["blocks"][2:4]]), None, g["block_idx"][2:4])
        assert "(code %d)" % F.ERR_ARG in str(exc.value)
        d.reset()
        d.feed(np.stack([R.onp.iq_u8_to_c64(b) for b in g["blocks"][2:4]]), None, g["block_idx"][2:4])
        assert d.n_kept == 2 and not d.result(arrays=("hist",))["hist"].any()


def test_destroy_gives_back_what_the_dossier_took(engines):
    g = G.load_scene("c2")
    eng = engines("c2")
    eng.detect(g["blocks"][:2], g["block_idx"][:2])         # (the engine's own lazy buffers exist)
    before = F.live_resources()
    d = F.Dossiers(eng, ALL, 4)
    d.feed(g["blocks"][:6], None, g["block_idx"][:6])
    assert d.result()["fft_mag"].shape == (4, 16384)
    assert F.live_resources() != before
    d.close()
    assert F.live_resources() == before
