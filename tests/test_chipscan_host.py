"""Host side of the chip-rate scan (no GPU): the wiring of thr_chipscan into the header, the symbol list and
the build, the float64 restatement (tests/chipscan_ref.py) against the reference's recorded results
(tests/golden/chipscan), the staircase claim the scan rests on, the length / rate-interval arithmetic, and
the scan's bookkeeping and command line through the NumPy stand-in for the engine."""
import io
import json
import os
import re

import numpy as np
import pytest

import chipscan_ref
from thrifty_amd import _native, build, chip_rate_search, cli, synth
from thrifty_amd.block_data import card_line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "chipscan")
SYMBOLS = ["thr_chipscan", "thr_debug_chipscan_geometry", "thr_debug_chipscan_budget", "thr_debug_chipscan_times",
           "thr_debug_chipscan_fill", "thr_debug_chipscan_groups"]


def test_thr_chipscan_is_declared_listed_and_built():
    header = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
    assert "#define THR_ABI_VERSION 11" in header and _native.ABI_VERSION == 11
    assert re.search(r"\+ thr_chipscan / thr_debug_chipscan_geometry", header)
    assert re.search(r"typedef struct thr_chip_record \{[^}]*int32_t sample;[^}]*uint32_t flags;[^}]*float energy, noise;"
                     r"[^}]*double offset;\s*\} thr_chip_record;", header)
    assert re.search(r"\bint thr_chipscan\(thr_handle\* h, const void\* samples, int format, size_t n_blocks,", header)
    assert re.search(r"\bint thr_debug_chipscan_geometry\(thr_handle\* h, size_t n_lengths, int\* candidates_per_chunk, "
                     r"int\* paired\);", header)
    assert re.search(r"\+ thr_debug_chipscan_fill / _groups", header)
    assert re.search(r"\bint thr_debug_chipscan_fill\(thr_handle\* h, size_t workgroups\);", header)
    assert re.search(r"\bint thr_debug_chipscan_groups\(thr_handle\* h, size_t n_blocks, size_t n_cand, int\* groups, "
                     r"int\* per_group\);", header)
    assert callable(_native.ChipScan.set_fill) and callable(_native.ChipScan.groups)
    for sym in SYMBOLS:
        assert re.search(r"\b%s\(" % sym, header) and sym in _native.EXPORTS
    assert _native.CHIP_RECORD_DTYPE.itemsize == 24 and callable(_native.ChipScan)
    assert "chipscan.hip" in build.SOURCES and "chipscan.hpp" in build.HEADERS
    assert build.UNPROFILED_CHIPSCAN == ("chipscan.hip", "chipscan.hpp")
    assert not any("chip" in name for name in cli.COMMANDS)
    source = open(os.path.join(build.CSRC, "chipscan.hpp")).read()
    assert int(re.search(r"constexpr int kChipMaxChips = (\d+);", source).group(1)) == _native.CHIP_MAX_CHIPS


def test_the_built_library_exports_thr_chipscan():
    assert os.path.exists(_native.LIB_PATH), "the library is not built: python -m thrifty_amd.build"
    lib = _native.load_library()
    assert all(getattr(lib, sym) for sym in SYMBOLS)


def test_csrc_hash_is_the_recorded_one_and_does_not_see_chipscan(monkeypatch):
    recorded = {run["csrc_sha16"] for run in _walk(json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json"))))}
    assert recorded == {build.csrc_hash()}
    with_scan = build.csrc_hash()
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "chipscan.hip"])
    monkeypatch.setattr(build, "HEADERS", [s for s in build.HEADERS if s != "chipscan.hpp"])
    assert build.csrc_hash() == with_scan
    monkeypatch.undo()
    monkeypatch.setattr(build, "UNPROFILED_CHIPSCAN", ())
    assert build.csrc_hash() != with_scan


def _walk(node):
    """every dict of a JSON tree that records a csrc_sha16"""
    if isinstance(node, dict):
        if "csrc_sha16" in node:
            yield node
        for v in node.values():
            for hit in _walk(v):
                yield hit
    elif isinstance(node, list):
        for v in node:
            for hit in _walk(v):
                yield hit


# ------------------------------------------------------------------ the restatement against the reference
@pytest.fixture(scope="module")
def golden():
    return {name: np.load(os.path.join(GOLDEN, name + ".npz")) for name in ("base", "mixed")}


@pytest.fixture(scope="module")
def restated(golden):
    out = {}
    for name, g in golden.items():
        chips = synth.gold_code(int(g["nbits"]), int(g["index"]))
        out[name] = chipscan_ref.scan(g["blocks"], chips, g["lengths"], int(g["carrier_len"]))
    return out


def test_the_scenes_are_the_fixtures_blocks(golden):
    block, _, lengths = chipscan_ref.base_scene()
    assert np.array_equal(golden["base"]["blocks"][0], block) and np.array_equal(golden["base"]["lengths"], lengths)
    assert lengths[0] == 2431 and lengths[-1] == 2491 and len(lengths) == 61
    blocks, _, lengths = chipscan_ref.mixed_scene()
    assert np.array_equal(golden["mixed"]["blocks"], blocks) and np.array_equal(golden["mixed"]["lengths"], lengths)
    assert sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN)) < 300 << 10


@pytest.mark.parametrize("name", ["base", "mixed"])
def test_restatement_equals_the_reference(golden, restated, name):
    g, r = golden[name], restated[name]
    ok = g["carrier_ok"]
    assert np.array_equal((r["flags"][:, 0] & 1) != 0, ok)
    assert np.array_equal(r["sample"], g["sample"])
    assert np.array_equal((r["flags"] & 2) != 0, g["detected"])
    for field in ("energy", "noise", "offset"):
        want = g[field]
        assert np.all(np.abs(r[field] - want) <= 1e-12 * np.abs(want)), field
    assert np.all(r["sample"][~ok] == -1) and np.all(r["flags"][~ok] == 0) and np.all(r["energy"][~ok] == 0)
    assert np.all(g["detected"][ok])


def test_base_scene_is_what_the_issue_measured(golden, restated):
    g, r = golden["base"], restated["base"][0]
    order = np.argsort(-r["energy"])
    assert g["lengths"][order[0]] == 2461 and abs(r["energy"][order[0]] - 366.3) < 0.05
    assert g["lengths"][order[1]] == 2459 and abs(1 - r["energy"][order[1]] / r["energy"][order[0]] - 0.198) < 1e-3
    assert r["sample"][order[0]] == 3000
    assert r["top2_gap"].min() > 1e-4          # no (block, length) pair of this scene is a near-tie


def test_best_length_scores_at_least_what_nelder_mead_found(golden):
    g = golden["base"]
    result = chip_rate_search.scan(g["blocks"], float(g["sample_rate"]), float(g["chip_rate"]), int(g["nbits"]),
                                   int(g["index"]), lengths=g["lengths"], backend=chipscan_ref.RefBackend())
    assert result.best_length == 2461 and result.carrier_ok.tolist() == [True]
    score = dict(zip(result.lengths.tolist(), result.score))
    # (both runs started inside the rate interval of the nominal length, 2455)
    assert all(chip_rate_search.nominal_length(float(g["sample_rate"]), r, 1023) == 2455 for r in g["nm_start"])
    for length in g["nm_length"]:
        assert score[result.best_length] >= score[int(length)]
    lo, hi = result.best_interval
    assert lo < result.best_rate <= hi
    assert chip_rate_search.nominal_length(result.sample_rate, result.best_rate, 1023) == 2461


def test_the_seam_scenes_are_what_their_docstrings_say():
    """the float64 figures that tests/test_gpu_chipscan_seams.py rests on (carrier_len 2455)"""
    n = chipscan_ref.N

    def restate(scene):
        blocks, chips, lengths = scene()
        ref = chipscan_ref.scan(blocks, chips, lengths, 2455)
        ok = (ref["flags"] & 1) != 0
        return lengths, ref, ok, int((ok & (ref["top2_gap"] < chipscan_ref.TIE)).sum())

    lengths, ref, ok, ties = restate(chipscan_ref.lane_scene)
    assert ok.all() and ok.size == 51 and ties == 1 and lengths[0] == 2461
    assert ref["sample"][:, 0].tolist() == chipscan_ref.LANE_LAGS and np.all(ref["offset"][:, 0] != 0)
    assert 1.05 <= ref["curvature"][:, 0].min() < 1.06 and max(chipscan_ref.LANE_LAGS) == n - 2461 - 1
    lengths, ref, ok, ties = restate(chipscan_ref.mask_scene)
    assert ok.all() and ties == 0 and ref["sample"][0].tolist() == [13923, 13922, 13919, 13914, 13108, 12881]
    assert np.array_equal(ref["sample"][0, :4], n - lengths[:4]) and np.all(ref["offset"][0, :4] == 0)
    assert ref["top2_gap"][0, :4].min() >= 0.14 and np.all(ref["offset"][0, 4:] != 0)
    lengths, ref, ok, ties = restate(chipscan_ref.length_scene)
    assert ok[:, 0].tolist() == [True] * 4 + [False] + [True] * 4 and ok.sum() == 104 and ties == 0
    assert 4.6e-4 < ref["top2_gap"][ok].min() < 4.7e-4 and lengths[0] == 1 and lengths[-1] == n - 2
    lengths, ref, ok, ties = restate(chipscan_ref.group_scene)
    assert ok[:, 0].tolist() == [True] * 4 + [False] + [True] * 11 and ok.sum() == 1050 and ties == 4
    assert len(lengths) == 70 and ties <= 0.05 * ok.sum()


# ------------------------------------------------------------------ the staircase and its arithmetic
def test_the_template_depends_on_the_rate_through_its_length_alone():
    rng = np.random.default_rng(3)
    fs = 2.4e6
    for nbits, index in ((10, 0), (10, 3), (7, 1), (11, 0)):
        code = synth.gold_code(nbits, index)
        for rate in rng.uniform(0.95e6, 1.05e6, 50):
            length = int(fs / rate * len(code))
            got = synth.gold_template(nbits, index, fs / rate)
            assert len(got) == length and np.array_equal(got, chipscan_ref.template(code, length))
            assert np.array_equal(got, synth.gold_template(nbits, index, (length + 0.5) / len(code)))


@pytest.mark.parametrize("fs,rate,n_chips", [(2.4e6, 1.0e6, 1023), (2.4e6, 0.999707e6, 1023), (2.048e6, 1.023e6, 2047),
                                             (1.0e6, 1.0e6, 127), (2.2e6, 1.1e6, 31)])
def test_lengths_and_rate_intervals_round_trip(fs, rate, n_chips):
    lengths = chip_rate_search.lengths_for(fs, rate, n_chips, 0.01)
    centre = int(fs / rate * n_chips)
    assert lengths.dtype == np.int32 and np.array_equal(lengths, np.arange(lengths[0], lengths[-1] + 1))
    assert lengths[0] == int(np.ceil(centre * 0.99)) and lengths[-1] == int(np.floor(centre * 1.01))
    assert centre in lengths
    previous_hi = None
    for length in lengths[::-1]:        # descending lengths = ascending rates
        lo, hi = chip_rate_search.rate_interval(int(length), fs, n_chips)
        assert lo < hi
        assert int(fs / hi * n_chips) == length and int(fs / np.nextafter(hi, np.inf) * n_chips) == length - 1
        assert int(fs / lo * n_chips) == length + 1 and int(fs / np.nextafter(lo, np.inf) * n_chips) == length
        assert abs(hi - fs * n_chips / length) <= 1e-9 * hi
        if previous_hi is not None:
            assert lo == previous_hi    # the intervals tile the rates
        previous_hi = hi
    assert chip_rate_search.lengths_for(fs, rate, n_chips, 0.0).tolist() == [centre]


# ------------------------------------------------------------------ bookkeeping and command line
def test_scan_refuses_bad_lengths_and_blocks_without_a_carrier():
    block, _, _ = chipscan_ref.base_scene()
    backend = chipscan_ref.RefBackend()
    for bad in ([0], [16383], [2455, -1], []):
        with pytest.raises(ValueError, match="template lengths"):
            chip_rate_search.scan(block, 2.4e6, 1.0e6, 10, lengths=bad, backend=backend)
    assert not backend.calls
    with pytest.raises(ValueError, match="Preferred pairs"):
        chip_rate_search.scan(block, 2.4e6, 1.0e6, 4, backend=backend)
    quiet = chipscan_ref.quiet_block(np.random.default_rng(1))
    with pytest.raises(ValueError, match="none of the 1 block"):
        chip_rate_search.scan(quiet, 2.4e6, 1.0e6, 10, lengths=[2455], backend=backend)


def test_score_is_the_float64_mean_over_the_blocks_with_a_carrier():
    blocks, _, lengths = chipscan_ref.mixed_scene()
    backend = chipscan_ref.RefBackend()
    result = chip_rate_search.scan(blocks, 2.4e6, 1.0e6, 10, lengths=lengths, backend=backend)
    assert backend.carrier_len == 2455 and backend.carrier_thresh == (100.0, 0.0, 0.0) and backend.calls == [(3, 5)]
    assert result.carrier_ok.tolist() == [True, False, True] and result.score.dtype == np.float64
    assert np.array_equal(result.score, result.energy[[0, 2]].astype(np.float64).mean(axis=0))
    assert result.lengths.tolist() == lengths.tolist()
    assert result.best_length == 2461 and result.best_index == 1       # the FIRST of the two equal columns
    assert np.array_equal(result.energy[:, 1], result.energy[:, 4])
    assert np.all(result.sample[1] == -1) and not result.detected[1].any() and result.detected[[0, 2]].all()
    assert result.sample[0, 1] == 700 and result.sample[2, 1] == 9000


def test_command_line(tmp_path, capsys):
    parser = chip_rate_search.build_parser()
    positional = [a.dest for a in parser._actions if not a.option_strings]
    assert positional == ["card_file", "block_id", "sample_rate", "chip_rate", "bit_length", "code_index"]
    assert {s for a in parser._actions for s in a.option_strings} >= {"--span", "--all-blocks", "--raw", "--block-size",
                                                                      "--history", "-o", "-p", "--plot"}
    blocks, _, _ = chipscan_ref.mixed_scene()
    card = tmp_path / "capture.card"
    card.write_text("# a comment\n" + "".join(card_line(10.0 + i, 40 + i, blocks[i]) for i in range(3)))
    common = [str(card), "42", "2.4M", "1.0M", "10", "--span", "0.003"]

    def run(argv):
        text = io.StringIO()
        backend = chipscan_ref.RefBackend()
        assert chip_rate_search.main(argv, out=text, backend=backend) == 0
        return text.getvalue().splitlines(), backend

    lengths = chip_rate_search.lengths_for(2.4e6, 1.0e6, 1023, 0.003)
    assert lengths.tolist() == list(range(2448, 2463))
    lines, backend = run(common + ["-o", str(tmp_path / "scan.npz")])
    assert backend.calls == [(1, len(lengths))] and len(lines) == len(lengths) + 1
    want = chip_rate_search.scan(blocks[2], 2.4e6, 1.0e6, 10, span=0.003, backend=chipscan_ref.RefBackend())
    assert lines[:-1] == list(want.lines())
    lo, hi = chip_rate_search.rate_interval(2461, 2.4e6, 1023)
    assert lines[13] == ".. try length 2461 (chip rate %.3f–%.3f) -> %r" % (lo, hi, float(want.score[13]))
    assert lines[-1].startswith("Best chip rate: %r (length 2461," % want.best_rate) and "1 of 1 block" in lines[-1]
    saved = np.load(str(tmp_path / "scan.npz"))
    assert saved["lengths"].tolist() == lengths.tolist() and int(saved["best_length"]) == 2461
    assert float(saved["best_rate"]) == want.best_rate == 2.4e6 * 1023 / 2461.5
    assert np.array_equal(saved["energy"], want.energy) and np.array_equal(saved["score"], want.score)
    assert saved["carrier_ok"].tolist() == [True] and saved["best_interval"].tolist() == [lo, hi]
    # every block of the file: the quiet one does not count
    lines, backend = run(common + ["--all-blocks"])
    assert backend.calls == [(3, len(lengths))] and "2 of 3 block" in lines[-1]
    # a block that is not in the file, and one without a carrier
    with pytest.raises(ValueError, match="Could not find block with index 7"):
        chip_rate_search.main([str(card), "7", "2.4M", "1.0M", "10"], out=io.StringIO(), backend=chipscan_ref.RefBackend())
    with pytest.raises(ValueError, match="none of the 1 block"):
        chip_rate_search.main([str(card), "41", "2.4M", "1.0M", "10"], out=io.StringIO(), backend=chipscan_ref.RefBackend())
    # a raw capture: block 1 of (16384, history 0) is the file's second 32768 bytes
    raw = tmp_path / "capture.bin"
    raw.write_bytes(blocks[1].tobytes() + blocks[0].tobytes())
    lines, backend = run([str(raw), "1", "2.4M", "1.0M", "10", "--span", "0.003", "--raw", "--block-size", "16384",
                          "--history", "0"])
    first = chip_rate_search.scan(blocks[0], 2.4e6, 1.0e6, 10, span=0.003, backend=chipscan_ref.RefBackend())
    assert lines[:-1] == list(first.lines())
    # plots
    assert chip_rate_search.main(common + ["-p"], out=io.StringIO(), backend=chipscan_ref.RefBackend()) == 2
    assert "plots are not part of this port" in capsys.readouterr().err


def test_search_returns_the_best_rate():
    block, _, _ = chipscan_ref.base_scene()
    text = io.StringIO()
    rate = chip_rate_search.search(block, 1.0e6, 10, 0, 2.4e6, span=0.003, out=text, backend=chipscan_ref.RefBackend())
    assert rate == 2.4e6 * 1023 / 2461.5 and len(text.getvalue().splitlines()) == 15
