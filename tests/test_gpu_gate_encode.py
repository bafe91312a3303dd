"""GPU tests of the carrier gate's byte-moving path: k_b64_encode and the order-preserving list of
passed blocks, EXACT against base64.b64encode (no tolerance).  With threshold `0c0s` every block whose
spectrum is not all zero passes (u8 samples always leave a DC line), so the encode path is tested
apart from the verdict; a constant-only threshold picks single blocks for the list shapes.
"""
import base64
import io
import os

import numpy as np
import pytest

from thrifty_amd import _native as F
from thrifty_amd import block_data, fastcard, synth

pytestmark = pytest.mark.gpu

FILL = 0x5A


def _patterns(rng, n_bytes):
    ramp = (np.arange(n_bytes) % 256).astype(np.uint8)
    # every 6-bit value at every position of a quantum: bytes stepping by 1, by 4 (top sextet), and a
    # 3-byte-periodic sweep of all 64 values in each of the four sextets
    q = np.zeros((64, 3), dtype=np.uint8)
    v = np.arange(64)
    q[:, 0] = (v << 2) | (v >> 4)
    q[:, 1] = ((v & 15) << 4) | (v >> 2)
    q[:, 2] = ((v & 3) << 6) | v
    sweep = np.resize(q.reshape(-1), n_bytes)
    return [rng.integers(0, 256, n_bytes, dtype=np.uint8), np.zeros(n_bytes, np.uint8),
            np.full(n_bytes, 255, np.uint8), ramp, sweep, np.roll(ramp, 1), np.roll(sweep, 2)]


def _check_slots(slots, n_passed, want_blocks, block_len, total_slots):
    stride, chars = F.gate_slot_stride(block_len), F.gate_payload_chars(block_len)
    assert n_passed == len(want_blocks)
    sl = slots[:total_slots * stride].reshape(total_slots, stride)
    for k, blk in enumerate(want_blocks):
        want = base64.b64encode(np.asarray(blk, np.uint8).tobytes())
        got = sl[k, :chars].tobytes()
        assert got[:16] == want[:16], (k, "first group")
        assert got[-16:] == want[-16:], (k, "last group / padded tail")
        assert got.endswith(b"=" * (3 - 2 * block_len % 3))
        assert got == want, k
        assert sl[k, chars] == 0x0A, (k, "newline")
        assert np.all(sl[k, chars + 1:] == FILL), (k, "bytes behind the newline are the caller's")
    assert np.all(sl[n_passed:] == FILL), "slots behind the last passed one are the caller's"
    assert np.all(slots[total_slots * stride:] == FILL)


# 2 N mod 3 = 1: 2048, 8192, 512, 32768;  = 2: 4096, 16384
@pytest.mark.parametrize("block_len", [2048, 8192, 4096, 16384, 32768, 512])
def test_every_payload_is_canonical_base64(block_len):
    rng = np.random.default_rng(block_len)
    blocks = np.stack(_patterns(rng, 2 * block_len))
    eng = F.Engine.gate(block_len, 0, (0, -1), (0.0, 0.0), max_batch=16)
    info = eng.path_info()
    assert info["correlate_kernel"] == "none" and info["n_templates"] == 0
    stride = F.gate_slot_stride(block_len)
    slots = np.full((len(blocks) + 2) * stride + 5, FILL, dtype=np.uint8)
    rec, n, slots = eng.gate_blocks(blocks, slots=slots)
    assert np.all(rec["flags"] == F.FLAG_CARRIER) and rec["block_idx"].tolist() == list(range(len(blocks)))
    assert np.all(rec["corr_sample"] == -1) and np.all(rec["reserved"] == 0)      # threshold 0.0f
    _check_slots(slots, n, blocks, block_len, len(blocks) + 2)
    eng.close()


@pytest.mark.parametrize("history", [1022, 1020, 1018, 1024])      # 2 (N - H) mod 16 = 4, 8, 12, 0
def test_windows_that_are_only_4_byte_aligned(history):
    n = 2048
    step = 2 * (n - history)
    assert step % 16 == {1022: 4, 1020: 8, 1018: 12, 1024: 0}[history]
    rng = np.random.default_rng(history)
    stream = rng.integers(0, 256, 2 * n + 10 * step + 3, dtype=np.uint8)
    eng = F.Engine.gate(n, history, (0, -1), (0.0, 0.0), max_batch=4)      # 11 blocks: three chunks
    slots = np.full(12 * F.gate_slot_stride(n), FILL, dtype=np.uint8)
    rec, k, slots = eng.gate_stream(stream, first_block_idx=100, slots=slots)
    assert len(rec) == 11 and rec["block_idx"].tolist() == list(range(100, 111))
    _check_slots(slots, k, [stream[i * step:i * step + 2 * n] for i in range(11)], n, 12)
    eng.close()


def _tone_blocks(n, which, count):
    """`count` blocks of quantiser-zero bytes; the ones listed in `which` carry a strong tone at bin 50."""
    blocks = np.full((count, 2 * n), 127, dtype=np.uint8)
    t = np.arange(n)
    tone = 0.5 * np.exp(2j * np.pi * 50 * t / n)
    for i in which:
        blocks[i] = block_data.complex_to_raw(tone * (1 + 1e-4 * i))      # (below full scale for every i used here)
    return blocks


@pytest.mark.parametrize("which, count, max_batch", [
    ([], 7, 8), (list(range(7)), 7, 8), ([0], 7, 8), ([6], 7, 8), ([0], 1, 8), ([], 1, 8),
    ([0, 5], 6, 5), ([4, 5], 6, 5), ([1, 3, 4, 9, 10, 11], 13, 4), (list(range(0, 2500, 3)), 2500, 2500),
])
def test_list_shapes_and_slot_order(which, count, max_batch):
    n = 2048
    blocks = _tone_blocks(n, which, count)
    eng = F.Engine.gate(n, 0, (0, -1), (1e5, 0.0), max_batch=max_batch)      # tone power (0.5 N)^2 ~ 1e6
    slots = np.full((count + 1) * F.gate_slot_stride(n), FILL, dtype=np.uint8)
    idx = np.arange(count, dtype=np.int64) * 7 - 3
    rec, k, slots = eng.gate_blocks(blocks, block_idx=idx, slots=slots)
    assert np.flatnonzero(rec["flags"] & F.FLAG_CARRIER).tolist() == which
    assert np.array_equal(rec["block_idx"], idx)
    assert np.all(rec["carrier_bin"][which] == 50)
    assert np.all(rec["reserved"] == np.float32(1e5).view(np.uint32))
    _check_slots(slots, k, blocks[which], n, count + 1)       # slot order == input order
    eng.close()


def test_capacity_is_checked_before_any_device_work():
    n = 2048
    eng = F.Engine.gate(n, 0, (0, -1), (0.0, 0.0), max_batch=4)
    blocks = _tone_blocks(n, [0], 3)
    small = np.full(3 * F.gate_slot_stride(n) - 1, FILL, dtype=np.uint8)
    with pytest.raises(F.NativeError, match="payload slots"):
        eng.gate_blocks(blocks, slots=small)
    assert np.all(small == FILL)
    eng.close()


def test_detect_entry_points_refuse_a_gate_handle_and_bad_windows_raise():
    eng = F.Engine.gate(2048, 0, (0, -1), (0.0, 0.0), max_batch=4)
    with pytest.raises(F.NativeError, match="gate") as e:
        eng.detect(_tone_blocks(2048, [], 2))
    assert e.value.args[0].endswith("(code %d)" % F.ERR_STATE)
    with pytest.raises(F.NativeError, match="gate"):
        eng.submit(_tone_blocks(2048, [], 2))
    eng.close()
    for win in ((-1, 0), (-5, 10), (0, 2048), (-2049, -1)):
        with pytest.raises(F.NativeError, match="window"):
            F.Engine.gate(2048, 0, win, (0.0, 0.0))


def test_written_file_through_the_reference_card_reader(tmp_path):
    from oracle import ref_readers
    if not ref_readers.available():
        pytest.fail("oracle/_ref/libfastcard_readers.so did not travel with the tree")
    n, h, skip = 2048, 1022, 1
    step = 2 * (n - h)
    rng = np.random.default_rng(77)
    data = rng.integers(0, 256, step * 40 + 11, dtype=np.uint8)
    raw_path, card_path = tmp_path / "x.bin", tmp_path / "x.card"
    data.tofile(str(raw_path))
    with fastcard.CarrierGate(n, h, (0, -1), (0.0, 0.0), skip=skip, batch_size=16) as gate:
        stats = gate.run(str(raw_path), str(card_path), timestamp=1234.9999996)
    assert stats["blocks"] == stats["passed"] == 40 - skip
    text = card_path.read_bytes()
    assert text.startswith(b"# arguments: { carrier_bin: '0--1', threshold: '0c+0s', block_size: 2048, history_size: 1022 }\n")
    assert stats["text_bytes"] == sum(len(ln) + 1 for ln in text.split(b"\n") if ln and not ln.startswith(b"#"))
    raw_ref, rc = ref_readers.read_blocks(str(raw_path), n, h, card=False, initial=np.zeros(2 * n, np.uint8))
    assert rc == 1 and len(raw_ref) == 40
    card_ref, rc = ref_readers.read_blocks(str(card_path), n, h, card=True)
    assert rc == 1 and len(card_ref) == 40 - skip
    for i, (sec, usec, index, raw) in enumerate(card_ref):
        # (the raw reader stamps a block with ITS wall clock; the gate was given one timestamp for the run)
        assert (sec, usec, index) == (1235, 0, i)
        np.testing.assert_array_equal(raw, raw_ref[i + skip][3], err_msg=str(i))
    # the reader interface yields what card_reader yields for that file
    with fastcard.CarrierGate(n, h, (0, -1), (0.0, 0.0), skip=skip, batch_size=16) as gate:
        got = list(gate(open(str(raw_path), "rb"), timestamp=1234.9999996))
    want = list(block_data.card_reader(open(str(card_path))))
    assert len(got) == len(want) == 39
    for a, b in zip(got, want):
        assert a[0] == b[0] and a[1] == b[1]
        np.testing.assert_array_equal(a[2].raw, b[2].raw)
        np.testing.assert_array_equal(np.asarray(a[2]), np.asarray(b[2]))


def test_zero_history_lead_in_blocks(tmp_path):
    """skip = 0: the first blocks start in front of the stream; their missing history is zero bytes."""
    n, h = 2048, 1500                         # ceil(h / (n - h)) = 3 lead-in blocks
    step = 2 * (n - h)
    rng = np.random.default_rng(3)
    data = rng.integers(0, 256, step * 9, dtype=np.uint8)
    with fastcard.CarrierGate(n, h, (0, -1), (0.0, 0.0), skip=0, batch_size=4) as gate:
        got = list(gate(data.tobytes(), timestamp=5.0))
    assert [g[1] for g in got] == list(range(9))
    padded = np.concatenate([np.zeros(2 * h, np.uint8), data])
    for i, g in enumerate(got):
        np.testing.assert_array_equal(g[2].raw, padded[i * step:i * step + 2 * n], err_msg=str(i))


def test_round_trip_through_detect_card_equals_detect_stream(tmp_path):
    n, h = 16384, 4096
    tpl = synth.gold_template(10, 2)
    from oracle import thrifty_np as onp
    win = onp.unique_window(n, h, len(tpl))
    rng = np.random.default_rng(11)
    blocks, _ = synth.synth_blocks(rng, 12, n, tpl, win, signal_frac=0.6)
    step = 2 * (n - h)
    stream = np.concatenate([blocks[0]] + [b[2 * h:] for b in blocks[1:]])      # any overlapping stream will do
    n_blocks = (stream.size - 2 * n) // step + 1
    gate = F.Engine.gate(n, h, (0, -1), (0.0, 0.0), max_batch=5)
    rec, k, slots = gate.gate_stream(stream)
    assert k == n_blocks == len(rec)
    text = F.format_card(np.full(k, 1000.25), rec["block_idx"], slots, n)
    gate.close()
    det = F.Engine(n, h, tpl, (0, 15, 0), (7, 110), (0, 15, 0), max_batch=5)
    ts, idx, off, _ = F.frame_card(text, 0, len(text), n, True, 100)
    assert idx.tolist() == list(range(n_blocks)) and np.all(ts == 1000.25)
    rec_card = det.detect_card(text, off, idx).copy()
    rec_stream = det.detect_stream(stream)
    assert rec_card.tobytes() == rec_stream.tobytes()
    assert (rec_stream["flags"] & F.FLAG_CORR).any()
    det.close()


def test_card_identity_gating_a_card_with_0c0s_returns_its_lines(tmp_path):
    n = 4096
    rng = np.random.default_rng(9)
    blocks = rng.integers(0, 256, (9, 2 * n), dtype=np.uint8)
    lines = [block_data.card_line(100.5 + i * 0.125, 1000 - 3 * i, b) for i, b in enumerate(blocks)]
    src = "# a comment\n" + "".join(lines[:4]) + "\n" + "".join(lines[4:])
    in_path, out_path = tmp_path / "in.card", tmp_path / "out.card"
    in_path.write_text(src)
    with fastcard.CarrierGate(n, 0, (0, -1), (0.0, 0.0), skip=0, batch_size=4) as gate:
        info = io.StringIO()
        gate.run(str(in_path), str(out_path), card=True, info=info)
    out = [ln + "\n" for ln in out_path.read_text().split("\n") if ln and not ln.startswith("#")]
    assert out == lines
    assert info.getvalue().count("block #") == 9 and "Read 9 blocks." in info.getvalue()
    # skip drops the first lines, whatever the reader (fastcard_cli.c:151-169)
    with fastcard.CarrierGate(n, 0, (0, -1), (0.0, 0.0), skip=2, batch_size=4) as gate:
        buf = io.BytesIO()
        gate.run(str(in_path), buf, card=True)
    assert buf.getvalue().decode() == "".join(lines[2:])
    # an invalid payload is refused
    bad = lines[0][:60] + "!" + lines[0][61:]
    with fastcard.CarrierGate(n, 0, (0, -1), (0.0, 0.0), skip=0) as gate:
        with pytest.raises(F.NativeError, match="base64"):
            gate.run(bad.encode(), io.BytesIO(), card=True)
