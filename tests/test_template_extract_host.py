"""Host side of template extraction (thrifty_amd.template_extract / template_generate): no GPU needed.

The fixtures' own consistency -- the reference's template, which went through an FFT round trip of the
shifted block, against the direct float64 formula on the stored input block (the identity the device
kernel rests on) -- the two command lines' arguments, template_generate's output and sentence, the
.tpl round trip, and the library's refusal of handle variants an extraction is not offered for.
"""
import os

import numpy as np
import pytest

import conftest
from thrifty_amd import _native, build, fastdet, synth, template_extract, template_generate

def load_golden(name):
    return conftest.load_golden("template_extract/" + name)


FIXTURES = ["extract_1024", "extract_2048", "extract_16384"]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_template_is_the_magnitude_of_the_input_block(name):
    """abs(ifft(shifted spectrum)) == |input samples|: the stored reference template against the direct
    float64 formula on the stored block.  1e-13 bounds the reference's FFT round trip (measured 1.4e-15)."""
    g = load_golden(name)
    w = len(g["template"])
    for pick in ("", "2"):
        k = int(g["chosen" + pick])
        assert g["det"][k] and abs(g["soff"][k]) <= float(g["max_offset" + pick])
        cut = template_extract.direct_template(g["blocks"][k], int(g["sample"][k]), w)
        err = np.max(np.abs(cut - g["template_ref" + pick]))
        print("%s pick%s: block %d, max |direct - reference| = %.3g" % (name, pick or "1", k, err))
        assert err <= 1e-13


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_picks_are_what_the_stored_verdicts_say(name):
    g = load_golden(name)
    assert g["blocks"].shape == (48, 2 * int(g["block_len"])) and g["blocks"].dtype == np.uint8
    for pick in ("", "2"):
        ok = g["det"] & (np.abs(g["soff"]) <= float(g["max_offset" + pick]))
        assert int(ok.sum()) == int(g["n_qualifying" + pick])
        energy = np.where(ok, g["energy"], -np.inf)
        assert int(np.argmax(energy)) == int(g["chosen" + pick])      # (argmax: the first of equals)
        # the margins the generator asserts: float32 energies held to 2e-5, offsets to 5e-6
        assert np.sort(energy)[-2] <= energy.max() * (1 - 1e-4)
        assert np.all(np.abs(np.abs(g["soff"][g["det"]]) - float(g["max_offset" + pick])) > 1e-3)
    assert int(g["chosen"]) != int(g["chosen2"])


def test_direct_template_takes_u8_and_complex_blocks_alike():
    g = load_golden("extract_1024")
    k, w = int(g["chosen"]), len(g["template"])
    from thrifty_amd.block_data import raw_to_complex
    a = template_extract.direct_template(g["blocks"][k], int(g["sample"][k]), w)
    b = template_extract.direct_template(raw_to_complex(g["blocks"][k]), int(g["sample"][k]), w)
    assert np.array_equal(a, b)
    assert abs(a.mean()) < 1e-15 and a.shape == (w,)


# ------------------------------------------------------------------ template_generate
@pytest.mark.parametrize("argv, nbits, index, sps", [
    (["7", "-s", "1M", "-p", "1M"], 7, 0, 1.0),
    (["8", "3", "--sample-rate", "2M", "--chip-rate", "1M"], 8, 3, 2.0),
    (["10", "2"], 10, 2, 2.4e6 / 0.999707e6),
])
def test_template_generate_writes_the_gold_template_and_says_so(tmp_path, capsys, monkeypatch, argv, nbits, index, sps):
    monkeypatch.chdir(tmp_path)                  # (no detector.cfg here: the defaults)
    out = tmp_path / "t.npy"
    assert template_generate.main(argv + ["-o", str(out)]) == 0
    got = np.load(out)
    assert np.array_equal(got, synth.gold_template(nbits, index, sps))
    said = capsys.readouterr().out.strip()
    sample_rate = {1.0: 1e6, 2.0: 2e6}.get(sps, 2.4e6)
    chip_rate = sample_rate / sps
    symbols = 2 ** nbits - 1
    assert said == "Generated new template: {} symbols @ {:.6f} MHz = {:.3f} ms --> {} samples @ {:.6f} Msps".format(
        symbols, chip_rate / 1e6, symbols / chip_rate * 1e3, len(got), sample_rate / 1e6)


def test_template_generate_defaults(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    args = template_generate.build_parser().parse_args(["9"])
    assert (args.length, args.index, args.output) == (9, 0, "template.npy")
    assert template_generate.main(["5"]) == 0 and os.path.exists(tmp_path / "template.npy")
    with pytest.raises(SystemExit):
        template_generate.build_parser().parse_args([])
    with pytest.raises(ValueError):
        template_generate.main(["4"])            # no preferred pair for 4 bits


# ------------------------------------------------------------------ template_extract's command line
def test_template_extract_arguments(tmp_path):
    card = tmp_path / "rx.card"
    card.write_bytes(b"")
    p = template_extract.build_parser()
    a = p.parse_args([str(card)])
    assert (a.output, a.raw, a.tpl, a.max_offset, a.plot) == ("capture.npy", False, None, 0.2, False)
    a.input.close()
    a = p.parse_args([str(card), "--raw", "-o", "x.npy", "--tpl", "x.tpl", "--max-offset", "0.05", "-p"])
    assert (a.output, a.raw, a.tpl, a.max_offset, a.plot) == ("x.npy", True, "x.tpl", 0.05, True)
    a.input.close()
    with pytest.raises(SystemExit):
        p.parse_args([])
    assert template_extract.MAX_OFFSET == 0.2


def test_template_extract_takes_the_reference_setting_keys(tmp_path, monkeypatch):
    """The setting keys go through settings.load_args like detect_cli's: flags and detector.cfg."""
    from thrifty_amd.settings import load_args
    monkeypatch.chdir(tmp_path)
    card = tmp_path / "rx.card"
    card.write_bytes(b"")
    (tmp_path / "detector.cfg").write_text("block_size: 2048\ntemplate: base.npy\n")
    keys = ["sample_rate", "block_size", "block_history", "carrier_window", "carrier_threshold", "corr_threshold",
            "template"]
    config, args = load_args(template_extract.build_parser(), keys,
                             argv=[str(card), "-y", "1024", "-w", "2-60", "-u", "12*snr", "--max-offset", "0.1"])
    args.input.close()
    assert (config.block_size, config.block_history, config.template) == (2048, 1024, "base.npy")
    assert config.corr_threshold == (0.0, 12.0, 0.0) and args.max_offset == 0.1


def test_sentence_is_the_reference_sentence():
    from thrifty_amd import toads_data
    res = toads_data.DetectionResult(1475000001.25, 42, 1.0, toads_data.CarrierSyncInfo(10, 0.1, 1.0, 0.1),
                                     toads_data.CorrDetectionInfo(700, -0.0123, 55.5, 1.5), -1)
    assert template_extract.sentence(res) == (
        "Captured template from block #42 (timestamp: 1475000001.250000): offset=-0.012; corr_ampl=55.5")


def test_tpl_round_trip(tmp_path):
    g = load_golden("extract_1024")
    path = str(tmp_path / "t.tpl")
    fastdet.save_tpl(path, g["template_ref"])
    back = fastdet.load_tpl(path)
    assert back.dtype == np.float32 and np.array_equal(back, g["template_ref"].astype(np.float32))
    assert os.path.getsize(path) == 2 + 4 * len(back)


# ------------------------------------------------------------------ the library
def _lib_or_skip():
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libthriftyhip.so not built")
    return _native.load_library()


def test_extraction_kernels_do_not_touch_the_profiled_hash():
    assert "template_extract.hip" in build.SOURCES and "run_extract.hip" in build.SOURCES
    assert "template_extract.hpp" in build.HEADERS and "run_extract.hip" in build.HOST_ONLY
    assert set(build.UNPROFILED_EXTRACT) == {"template_extract.hip", "template_extract.hpp"}


@pytest.mark.parametrize("header", ["run_loop.hpp", "host_internal.hpp"])
def test_csrc_hash_does_not_see_a_host_only_header(monkeypatch, header):
    # the host headers: listed (a change rebuilds), host only, and for that reason alone outside csrc_hash()
    assert header in build.HEADERS and header in build.HOST_ONLY
    with_header = build.csrc_hash()
    monkeypatch.setattr(build, "HEADERS", [h for h in build.HEADERS if h != header])
    assert build.csrc_hash() == with_header
    monkeypatch.undo()
    monkeypatch.setattr(build, "HOST_ONLY", tuple(h for h in build.HOST_ONLY if h != header))
    assert build.csrc_hash() != with_header


def test_native_exports_and_abi_of_the_extraction():
    lib = _lib_or_skip()
    assert _native.ABI_VERSION == 11 == lib.thr_abi_version()
    for sym in ("thr_extract_create", "thr_extract_destroy", "thr_extract_reset", "thr_extract_feed",
                "thr_extract_feed_card", "thr_extract_feed_stream", "thr_extract_result", "thr_run_extract_card",
                "thr_run_extract_stream"):
        assert sym in _native.EXPORTS and getattr(lib, sym)


def test_null_arguments_are_refused_with_a_sentence():
    import ctypes as C
    lib = _lib_or_skip()
    x = C.c_void_p()
    assert lib.thr_extract_create(None, 0.2, C.byref(x)) == _native.ERR_ARG and b"null" in lib.thr_last_error()
    assert lib.thr_extract_reset(None) == _native.ERR_ARG
    assert lib.thr_extract_result(None, None, None, None, 0, None) == _native.ERR_ARG
    assert lib.thr_extract_feed(None, None, 0, None, None, 1, None) == _native.ERR_ARG
    lib.thr_extract_destroy(None)                # (like free(NULL))
