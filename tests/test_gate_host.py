"""Host side of the carrier gate (thrifty_amd.fastcard, thr_format_card): no GPU needed.

Parsing against the cases of fastcard/parse.c and cardet_normalize_window, the skip / index /
window-offset arithmetic against the reference's native raw reader, the .card line writer against
block_data.card_line and both card readers, the command line's option letters and refusals, and the
counter-freshness rule: the gate's kernels must not change build.csrc_hash().
"""
import base64
import io
import json
import os
import re

import numpy as np
import pytest

from thrifty_amd import _native, block_data, build, fastcard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib_or_skip():
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libthriftyhip.so not built")
    return _native.load_library()


def test_gate_kernels_do_not_touch_the_profiled_hash():
    prof = json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json")))
    shas = set(re.findall(r'"csrc_sha16": "([0-9a-f]+)"', json.dumps(prof)))
    assert shas, "no csrc_sha16 recorded"
    assert shas == {build.csrc_hash()}
    assert "card_gate.hip" in build.SOURCES and "card_gate.hpp" in build.HEADERS
    assert set(build.UNPROFILED) == {"card_gate.hip", "card_gate.hpp"}


@pytest.mark.parametrize("text, want", [
    ("100c2s", (100.0, 2.0)), ("0c0s", (0.0, 0.0)), ("1.5c", (1.5, 0.0)), ("2s100c", (100.0, 2.0)),
    ("7", (7.0, 0.0)), ("3s", (0.0, 3.0)), ("1e3c.5s", (1000.0, 0.5)), ("", (0.0, 0.0)),
    ("0.1c", (float(np.float32(0.1)), 0.0)),          # float32, like fargs_t's
])
def test_threshold_strings_parse_like_parse_c(text, want):
    assert fastcard.parse_threshold(text) == want


@pytest.mark.parametrize("text", ["abc", "1x", "1c2c", "1s2s", "100c2", "c", "1c 2s x", "--1c"])
def test_bad_threshold_strings_are_refused(text):
    # ("100c2": the trailing 2 is a second constant -- parse.c's case '\0' falls into the constant)
    with pytest.raises(ValueError):
        fastcard.parse_threshold(text)


@pytest.mark.parametrize("text, want", [
    ("0--1", (0, -1)), ("7-110", (7, 110)), ("-5--1", (-5, -1)), ("5", (5, 5)), ("110-7", (110, 7)),
    ("5-", (5, 5)), ("1--1", (1, -1)),
])
def test_window_strings_parse_like_parse_c(text, want):
    assert fastcard.parse_window(text) == want


def test_bad_window_string_is_refused():
    for text in ("abc", "", "-"):
        with pytest.raises(ValueError):
            fastcard.parse_window(text)


@pytest.mark.parametrize("lo, hi, n, want", [
    (0, -1, 16384, (0, 16383)), (1, -1, 16384, (1, 16383)), (7, 110, 16384, (7, 110)),
    (-5, -1, 64, (59, 63)), (-1, -5, 64, (59, 63)), (110, 7, 16384, (7, 110)), (0, 0, 64, (0, 0)),
    (63, 63, 64, (63, 63)), (-64, -1, 64, (0, 63)),
])
def test_window_normalisation_like_cardet(lo, hi, n, want):
    assert fastcard.normalize_window(lo, hi, n) == want


@pytest.mark.parametrize("lo, hi, n", [(-1, 0, 64), (-5, 10, 64), (0, 64, 64), (64, 70, 64), (-65, -1, 64),
                                       (3, -65, 64)])
def test_refused_windows_like_cardet(lo, hi, n):
    with pytest.raises(ValueError):
        fastcard.normalize_window(lo, hi, n)


def _gate_formula_block(data, i, skip, n, h):
    """The bytes the gate's formula addresses for kept block i: zero bytes where it is negative."""
    off = fastcard.window_offset(i, skip, n, h)
    blk = np.zeros(2 * n, dtype=np.uint8)
    if off < 0:
        blk[-off:] = data[:2 * n + off]
    else:
        blk[:] = data[off:off + 2 * n]
    return blk


# history <, = and > block_len - history
@pytest.mark.parametrize("n, h", [(64, 20), (64, 32), (64, 50), (128, 120), (64, 0)])
@pytest.mark.parametrize("skip", [0, 1, 3, 7])
def test_skip_index_and_offset_arithmetic_against_the_reference_raw_reader(tmp_path, n, h, skip):
    from oracle import ref_readers
    if not ref_readers.available():
        pytest.skip("oracle/_ref is not built (build() compiles it where the reference checkout is)")
    rng = np.random.default_rng(n * 1000 + h * 10 + skip)
    new = n - h
    data = rng.integers(0, 256, size=2 * new * 23 + 2 * new - 1, dtype=np.uint8)   # 23 blocks and a short tail
    path = tmp_path / "x.bin"
    data.tofile(str(path))
    ref, rc = ref_readers.read_blocks(str(path), n, h, card=False, initial=np.zeros(2 * n, dtype=np.uint8))
    assert rc == 1 and len(ref) == 23
    assert [r[2] for r in ref] == list(range(23))                # the reader's own index++ per block
    assert fastcard.kept_blocks(data.size, skip, n, h) == 23 - skip
    for i in range(23 - skip):
        # fastcard_cli.c:151-169 drops the first `skip` blocks; fastcard.c:108-110 starts the reader's
        # index at -skip, so the first kept block has index 0: kept block i is the reader's block i + skip
        np.testing.assert_array_equal(ref[i + skip][3], _gate_formula_block(data, i, skip, n, h), err_msg=str(i))
        if i + skip >= -(-h // new):
            assert fastcard.window_offset(i, skip, n, h) >= 0    # a window of the stream, read in place


def _slots_of(blocks, block_len, fill=0xA5):
    stride, chars = _native.gate_slot_stride(block_len), _native.gate_payload_chars(block_len)
    slots = np.full((len(blocks), stride), fill, dtype=np.uint8)
    for k, b in enumerate(blocks):
        enc = base64.b64encode(b.tobytes())
        assert len(enc) == chars
        slots[k, :chars] = np.frombuffer(enc, dtype=np.uint8)
        slots[k, chars] = 0x0A
    return slots


STAMPS = [0.0, 1.5, 1234567890.123456, 17.9999996, 17.9999994, 1e9 + 0.9999996, 0.0000005, 0.0000015,
          2.5e-6, 1700000000.9999995, 3.25, -1.25]
INDICES = [0, 1, -1, -7, 2 ** 31, 2 ** 31 + 5, 2 ** 40, -2 ** 33, 12345, 7, 8, 9]


@pytest.mark.parametrize("block_len", [64, 128])        # 2 N mod 3 = 2 and 1
def test_format_card_equals_card_line_and_reads_back(tmp_path, block_len):
    _lib_or_skip()
    rng = np.random.default_rng(5)
    blocks = rng.integers(0, 256, size=(len(STAMPS), 2 * block_len), dtype=np.uint8)
    text = _native.format_card(STAMPS, INDICES, _slots_of(blocks, block_len), block_len)
    want = "".join(block_data.card_line(t, i, b) for t, i, b in zip(STAMPS, INDICES, blocks))
    assert text.decode() == want
    assert "18.000000 -7 " in want and "17.999999 " in want      # the carry into the seconds
    # read back by thr_frame_card ...
    ts, idx, off, nxt = _native.frame_card(text, 0, len(text), block_len, True, 100)
    assert nxt == len(text) and idx.tolist() == INDICES
    chars = _native.gate_payload_chars(block_len)
    for k in range(len(STAMPS)):
        assert ts[k] == float(want.split("\n")[k].split(" ")[0])
        if STAMPS[k] >= 0:        # (card_line's divmod writes -1.25 as "-2.750000": text equality is what counts there)
            assert abs(ts[k] - STAMPS[k]) <= 0.5000001e-6
        np.testing.assert_array_equal(np.frombuffer(base64.b64decode(text[off[k]:off[k] + chars]), np.uint8), blocks[k])
    # ... by the Python card reader ...
    got = list(block_data.card_reader(io.StringIO(want)))
    assert [g[1] for g in got] == INDICES
    for g, b in zip(got, blocks):
        np.testing.assert_array_equal(g[2].raw, b)


@pytest.mark.parametrize("block_len", [64, 128])
def test_format_card_read_back_by_the_reference_card_reader(tmp_path, block_len):
    """(non-negative timestamps: the reference's native card reader parses "%ld.%ld")"""
    _lib_or_skip()
    rng = np.random.default_rng(5)
    blocks = rng.integers(0, 256, size=(len(STAMPS), 2 * block_len), dtype=np.uint8)
    from oracle import ref_readers
    if not ref_readers.available():
        pytest.skip("oracle/_ref is not built: the reference's native card reader is not available")
    keep = [k for k, t in enumerate(STAMPS) if t >= 0]
    path = tmp_path / "x.card"
    path.write_bytes(_native.format_card([STAMPS[k] for k in keep], [INDICES[k] for k in keep],
                                         _slots_of(blocks[keep], block_len), block_len))
    ref, rc = ref_readers.read_blocks(str(path), block_len, 0, card=True)
    assert rc == 1 and len(ref) == len(keep)
    for (sec, usec, index, raw), k in zip(ref, keep):
        assert (sec, usec) == divmod(int(round(STAMPS[k] * 1e6)), 1000000)
        assert index == INDICES[k]
        np.testing.assert_array_equal(raw, blocks[k])


def test_format_card_checks_its_arguments():
    lib = _lib_or_skip()
    import ctypes as C
    used = C.c_size_t(0)
    buf = np.zeros(16, dtype=np.uint8)
    ts, idx = np.zeros(1), np.zeros(1, dtype=np.int64)
    slots = np.zeros(_native.gate_slot_stride(64), dtype=np.uint8)
    rc = lib.thr_format_card(ts.ctypes.data, idx.ctypes.data, slots.ctypes.data, slots.size,
                             _native.gate_payload_chars(64), 1, buf.ctypes.data, buf.size, C.byref(used))
    assert rc == _native.ERR_ARG and b"need" in lib.thr_last_error()
    ts[0] = float("nan")
    big = np.zeros(4096, dtype=np.uint8)
    rc = lib.thr_format_card(ts.ctypes.data, idx.ctypes.data, slots.ctypes.data, slots.size,
                             _native.gate_payload_chars(64), 1, big.ctypes.data, big.size, C.byref(used))
    assert rc == _native.ERR_ARG and b"timestamp" in lib.thr_last_error()


def test_slot_geometry():
    for n in (64, 512, 2048, 4096, 8192, 16384, 32768, 65536):
        chars, stride = _native.gate_payload_chars(n), _native.gate_slot_stride(n)
        assert chars == len(base64.b64encode(bytes(2 * n))) and (2 * n) % 3 in (1, 2)
        assert stride % 16 == 0 and chars + 1 <= stride < chars + 1 + 16


def test_cli_option_letters_defaults_and_refusals(capsys):
    p = fastcard.build_parser()
    a = p.parse_args([])
    assert (a.input, a.block_len, a.history, a.skip, a.carrier_window, a.threshold, a.card, a.quiet) == (
        "-", 16384, 4920, 1, "0--1", "100c2s", False, False)
    g = fastcard.gate_from_args(a)                           # fastcard's defaults, fargs.c:6-14
    assert (g.block_len, g.history_len, g.skip, g.threshold, g.window, g.bins) == (
        16384, 4920, 1, (100.0, 2.0), (0, -1), (0, 16383))
    a = p.parse_args("-i x.bin -o y.card -b 4096 -h 1000 -k 3 -w 7-110 -t 5c1.5s --card -q".split())
    assert (a.input, a.output, a.block_len, a.history, a.skip, a.card, a.quiet) == (
        "x.bin", "y.card", 4096, 1000, 3, True, True)
    g = fastcard.gate_from_args(a)
    assert (g.history_len, g.bins, g.threshold) == (1000, (7, 110), (5.0, 1.5))
    assert fastcard.gate_from_args(p.parse_args(["-h", "4920"])).history_len == 4920     # -h is the history
    with pytest.raises(SystemExit) as e:
        p.parse_args(["--help"])
    assert e.value.code == 0 and "--history" in capsys.readouterr().out
    for argv in (["-i", "rtlsdr"], ["-f", "433.83M"], ["-s", "2.4M"], ["-g", "10"], ["-d", "1"],
                 ["--wisdom-file", "w"], ["-m", "w"]):
        with pytest.raises(SystemExit) as e:
            fastcard.gate_from_args(p.parse_args(argv))
        assert "out of scope" in str(e.value.code) and ". " not in str(e.value.code), argv     # one sentence
    for argv in (["-w", "-5-3"], ["-t", "1x"], ["-w", "0-16384"], ["-b", "1000"]):
        with pytest.raises(SystemExit):
            fastcard.gate_from_args(p.parse_args(argv))


def test_card_header_lines_start_with_a_hash():
    text = fastcard.card_header(16384, 4920, (0, -1), (100.0, 2.0), start_time=12.5)
    lines = text.splitlines()
    assert len(lines) == 3 and all(ln.startswith("#") for ln in lines) and text.endswith("\n")
    assert lines[0] == ("# arguments: { carrier_bin: '0--1', threshold: '100c+2s', block_size: 16384, "
                        "history_size: 4920 }")
    assert lines[1].startswith("# tool: 'thrifty_amd.fastcard") and lines[2] == "# start_time: 12.500000"
    # the readers skip them
    assert list(block_data.card_reader(io.StringIO(text))) == []


def test_native_exports_and_abi_of_the_gate():
    assert _native.ABI_VERSION >= 10 and _native.VARIANT_GATE == 3
    for sym in ("thr_gate", "thr_gate_stream", "thr_gate_card", "thr_gate_slot_stride", "thr_format_card"):
        assert sym in _native.EXPORTS
    header = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
    assert "#define THR_VARIANT_GATE 3" in header
