"""Host side of the capture survey (no GPU): the wiring of thr_survey_* into the header, the symbol list and
the build, the energy-from-sums identity, and CaptureSurvey's interval bookkeeping, lead-in rule and command
line against the NumPy stand-in for the engine (tests/survey_ref.py)."""
import io
import os
import re

import numpy as np
import pytest

import survey_ref
from thrifty_amd import _native, build, cli, survey

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["thr_survey_create", "thr_survey_destroy", "thr_survey_reset", "thr_survey_shift", "thr_survey_pending",
           "thr_survey_feed", "thr_survey_feed_stream", "thr_debug_survey_geometry"]


def test_thr_survey_is_declared_listed_and_built():
    header = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
    assert "#define THR_ABI_VERSION 11" in header and _native.ABI_VERSION == 11
    assert "typedef struct thr_survey thr_survey;" in header
    assert re.search(r"\bint thr_survey_create\(thr_handle\* h, int integrate, thr_survey\*\* out\);", header)
    assert re.search(r"\bint thr_survey_feed_stream\(thr_survey\* s, const uint8_t\* stream, size_t n_bytes,", header)
    for sym in SYMBOLS:
        assert re.search(r"\b%s\(" % sym, header) and sym in _native.EXPORTS
    assert callable(_native.Survey) and callable(survey.CaptureSurvey)
    assert "survey.hip" in build.SOURCES and "survey.hpp" in build.HEADERS
    assert build.UNPROFILED_SURVEY == ("survey.hip", "survey.hpp")
    assert "survey" not in cli.COMMANDS


def test_the_built_library_exports_thr_survey():
    assert os.path.exists(_native.LIB_PATH), "the library is not built: python -m thrifty_amd.build"
    lib = _native.load_library()
    assert all(getattr(lib, sym) for sym in SYMBOLS)


def test_csrc_hash_does_not_see_survey_hip(monkeypatch):
    with_survey = build.csrc_hash()
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "survey.hip"])
    monkeypatch.setattr(build, "HEADERS", [s for s in build.HEADERS if s != "survey.hpp"])
    assert build.csrc_hash() == with_survey
    monkeypatch.undo()
    monkeypatch.setattr(build, "UNPROFILED_SURVEY", ())
    assert build.csrc_hash() != with_survey


@pytest.mark.parametrize("n", [1024, 16384, 65536])
def test_energy_from_sums_is_the_sum_of_squared_samples(n):
    rng = np.random.default_rng(n)
    blocks = np.stack([rng.integers(0, 256, 2 * n).astype(np.uint8),
                       rng.integers(126, 130, 2 * n).astype(np.uint8),
                       np.full(2 * n, 127, np.uint8), np.full(2 * n, 128, np.uint8),
                       np.zeros(2 * n, np.uint8), np.full(2 * n, 255, np.uint8)])
    got = survey.energy_from_sums(survey_ref.sums(blocks), n)
    want = survey_ref.energy(blocks)
    assert np.all(np.abs(got - want) <= 1e-12 * want), (got, want)
    assert survey.OFFSET == float(np.float32(127.4))


def _capture(n, h, n_new_blocks, seed=5):
    """a stream of exactly n_new_blocks * (n - h) new samples"""
    return np.random.default_rng(seed).integers(100, 156, 2 * (n - h) * n_new_blocks).astype(np.uint8).tobytes()


def _run(n, h, k, data, batch):
    backend = survey_ref.RefBackend(n, h, k)
    with survey.CaptureSurvey(n, h, integrate=k, batch_size=batch, backend=backend) as s:
        return list(s(io.BytesIO(data))), backend


@pytest.mark.parametrize("n,h,lead", [(64, 0, 0), (64, 20, 1), (64, 40, 2), (64, 48, 3), (64, 21, 1)])
def test_lead_in_blocks_are_not_surveyed(n, h, lead):
    k, total = 3, 12
    data = _capture(n, h, total)
    got, backend = _run(n, h, k, data, batch=4)
    # the reference's block i ends (i + 1) (n - h) samples into the stream; blocks lead .. are stream bytes only
    step = 2 * (n - h)
    whole = np.frombuffer(data, dtype=np.uint8)
    blocks = np.stack([whole[(i + 1) * step - 2 * n:(i + 1) * step] for i in range(lead, total)])
    mean_mag, hist, sums = survey_ref.survey(blocks, k)
    assert len(got) == (total - lead) // k == len(mean_mag)
    for j, interval in enumerate(got):
        assert interval.first_block == lead + j * k and interval.n_blocks == k
        assert np.array_equal(interval.hist, hist[j])
        assert np.array_equal(interval.block_sums, sums[j * k:(j + 1) * k])
        assert np.allclose(interval.mean_mag, mean_mag[j], rtol=0, atol=2.0 ** -(backend.shift + 1) + 1e-9)
    # an odd block_len - history_len goes through host-packed blocks, an even one through the stream form
    assert {c[0] for c in backend.calls} == ({"feed"} if (n - h) % 2 else {"feed_stream"})


@pytest.mark.parametrize("batch", [1, 2, 5, 64])
def test_intervals_do_not_depend_on_the_batching(batch):
    n, h, k = 64, 16, 4
    data = _capture(n, h, 23)
    want, _ = _run(n, h, k, data, batch=64)
    got, _ = _run(n, h, k, data, batch=batch)
    assert len(got) == len(want) == (23 - 1) // k          # the trailing partial interval is never reported
    for a, b in zip(got, want):
        assert a.first_block == b.first_block and np.array_equal(a.mean_mag, b.mean_mag)
        assert np.array_equal(a.hist, b.hist) and np.array_equal(a.block_sums, b.block_sums)


def test_interval_properties():
    n, k = 64, 2
    blocks = np.stack([np.full(2 * n, 0, np.uint8), np.full(2 * n, 255, np.uint8)])
    blocks[1, :64] = 130
    _, hist, sums = survey_ref.survey(blocks, k)
    v = survey.SurveyInterval(7, k, np.arange(n, dtype=np.float64), hist[0], sums)
    energy = survey_ref.energy(blocks)
    assert np.allclose(v.block_energy, energy, rtol=1e-12)
    assert v.norm == pytest.approx(np.sqrt(energy).mean(), rel=1e-12)
    assert v.rms_per_sample == pytest.approx(np.sqrt(energy.sum() / (k * n)), rel=1e-12)
    assert np.array_equal(v.mean_hist, hist[0] / 2.0)
    assert v.saturation == (128 + 64) / 256.0
    assert v.dc == pytest.approx((blocks.astype(np.float64).mean() - float(np.float32(127.4))) / 128, rel=1e-12)
    bins, mag = v.shifted()
    assert bins[0] == -n // 2 and bins[n // 2] == 0 and mag[n // 2] == 0.0 and mag[0] == n // 2
    assert np.array_equal(bins % n, np.fft.fftshift(np.arange(n)))


SIGNATURE_CASES = [(64, 3), (64, 5), (1024, 3), (1024, 5), (16384, 1), (16384, 3), (16384, 4), (16384, 8), (16384, 20)]


@pytest.mark.parametrize("n,k", SIGNATURE_CASES)
def test_signature_blocks_name_their_rows_on_the_oracle(n, k):
    """tests/test_gpu_survey_seams.py decides row assignment by the K largest bins of a row being the tone
    bins of that row's blocks.  The oracle alone passes that, with room: the K-th tone bin is at least 4
    times the largest other bin.  Smallest factor measured over these cases: 5.32 (n = 64, K = 5); 6.84 at
    1024 (K = 5) and 7.62 at 16384 (K = 20)."""
    nb = {20: 45, 1: 20}.get(k, 29)
    blocks = survey_ref.signature_blocks(nb, n, seed=5)
    assert blocks.shape == (nb, 2 * n) and blocks.dtype == np.uint8
    tail = survey_ref.signature_tail(n)
    for b in (0, 1, nb - 1):
        assert np.all(blocks[b, 2 * n - tail:] == (7 * b + 1) % 256)
    backend = survey_ref.RefBackend(n, 0, k)
    parts = [backend.feed(blocks[lo:lo + 8]) for lo in range(0, nb, 8)]         # the stand-in's own open interval
    spec, hist, sums = [np.concatenate([p[i] for p in parts]) for i in range(3)]
    mean_mag, want_hist, want_sums = survey_ref.survey(blocks, k)
    assert len(spec) == nb // k and np.array_equal(hist, want_hist) and np.array_equal(sums, want_sums)
    worst = np.inf
    for j in range(len(spec)):
        assert survey_ref.top_bins(spec[j], k) == survey_ref.tone_bins(j, k, n), j
        assert survey_ref.top_bins(mean_mag[j], k) == survey_ref.tone_bins(j, k, n), j
        worst = min(worst, survey_ref.tone_margin(spec[j], j, k, n))
    print("signature blocks n=%d K=%d: smallest tone margin %.2f" % (n, k, worst))
    assert worst >= 4.0
    # a row one block late holds another set of bins: the assertion tells the two apart
    assert survey_ref.tone_bins(0, k, n) != sorted(survey_ref.tone_bin(b, n) for b in range(1, k + 1))


def test_signature_blocks_refuse_a_window_with_a_repeated_bin():
    assert len({survey_ref.tone_bin(b, 64) for b in range(32)}) == 32
    assert survey_ref.tone_bin(32, 64) == survey_ref.tone_bin(0, 64)
    with pytest.raises(AssertionError):
        survey_ref.tone_bins(0, 33, 64)


def test_parser_and_command_line(tmp_path):
    parser = survey.build_parser()
    assert parser.get_default("integrate") == 100 and parser.get_default("output") is None
    assert {s for a in parser._actions for s in a.option_strings} >= {"-i", "--integrate", "--rms", "--hist", "--fft", "-o"}
    with pytest.raises(SystemExit):
        parser.parse_args(["x", "--rms", "--hist"])
    n, h, k = 64, 16, 3
    path = tmp_path / "capture.bin"
    path.write_bytes(_capture(n, h, 11))
    want, _ = _run(n, h, k, path.read_bytes(), batch=64)
    common = [str(path), "-i", str(k), "--block-size", str(n), "--history", str(h)]

    def run(*extra):
        text = io.StringIO()
        assert survey.main(common + list(extra), out=text, backend=survey_ref.RefBackend(n, h, k)) == 0
        return text.getvalue().splitlines()

    assert run() == run("--rms") == [repr(v.norm) for v in want]
    assert run("--hist") == [" ".join(str(int(c)) for c in v.hist) for v in want]
    lines = run("--fft", "-o", str(tmp_path / "out.npz"))
    assert len(lines) == len(want) * (n + 1) and lines[0].split() == [str(-n // 2), repr(float(want[0].mean_mag[n // 2]))]
    saved = np.load(str(tmp_path / "out.npz"))
    assert saved["first_block"].tolist() == [v.first_block for v in want] and int(saved["integrate"]) == k
    assert np.array_equal(saved["mean_mag"], np.stack([v.mean_mag for v in want]))
    assert np.array_equal(saved["hist"], np.stack([v.hist for v in want]))
    assert np.array_equal(saved["block_sums"], np.stack([v.block_sums for v in want]))
    assert np.array_equal(saved["norm"], [v.norm for v in want])
