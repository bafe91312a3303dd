"""GPU tests of the in-library file loop of the carrier gate, thr_run_gate_stream / thr_run_gate_card:
its output must equal, byte for byte, what the batch entry points give when driven from Python
(thr_gate* + thr_format_card), whatever the batch size; statistics, the record sink, skip and the
zero-history lead-in blocks, and a failing descriptor."""
import os

import numpy as np
import pytest

from thrifty_amd import _native as F
from thrifty_amd import block_data, fastcard

pytestmark = pytest.mark.gpu


def _python_path(gate, data, card, timestamp):
    """The same file gated batch by batch from Python: (text, records of every block)."""
    text, recs = [], []
    for ts, rec_all, rec, slots in gate._batches(data, card, timestamp):
        recs.append(rec_all)
        text.append(F.format_card(ts, rec["block_idx"], slots, gate.block_len))
    return b"".join(text), np.concatenate(recs) if recs else np.zeros(0, dtype=F.RECORD_DTYPE)


def _stream(n, h, nblk, seed, tone_every=3):
    rng = np.random.default_rng(seed)
    new = n - h
    z = rng.normal(0, 0.02, new * nblk) + 1j * rng.normal(0, 0.02, new * nblk)
    t = np.arange(new)
    for b in range(0, nblk, tone_every):
        z[b * new:(b + 1) * new] += 0.3 * np.exp(2j * np.pi * 50.0 * t / n)
    return np.concatenate([block_data.complex_to_raw(z), np.zeros(7, np.uint8)])       # (and a short tail)


@pytest.mark.parametrize("n, h, skip, batch", [(2048, 1022, 1, 7), (2048, 1500, 0, 4), (2048, 1500, 2, 64),
                                               (16384, 4920, 1, 16), (2048, 0, 0, 5)])
@pytest.mark.parametrize("threshold", [(0.0, 0.0), (0.0, 60.0)])
def test_run_gate_stream_equals_the_python_path(tmp_path, n, h, skip, batch, threshold):
    data = _stream(n, h, 45, n + h + skip)
    with fastcard.CarrierGate(n, h, (7, 110), threshold, skip=skip, batch_size=batch) as gate:
        want_text, want_rec = _python_path(gate, data.tobytes(), False, 77.25)
        total = fastcard.kept_blocks(data.size, skip, n, h)
        assert len(want_rec) == total == 45 - skip
        rec = np.zeros(total + 3, dtype=F.RECORD_DTYPE)
        path = tmp_path / "out.card"
        with open(str(path), "wb") as f:
            st = gate.engine().run_gate(data, out_fd=f.fileno(), skip=skip, timestamp=77.25, batch_blocks=batch,
                                        rec_out=rec)
        assert path.read_bytes() == want_text
        assert rec[:total].tobytes() == want_rec.tobytes() and not rec[total:].tobytes().strip(b"\0")
        passed = int((want_rec["flags"] & F.FLAG_CARRIER != 0).sum())
        assert (st["blocks"], st["passed"], st["bytes_in"], st["text_bytes"]) == (total, passed, data.size, len(want_text))
        assert st["batches"] >= -(-total // batch) and st["total_s"] > 0 and st["gate_s"] > 0
        assert all(st[k] >= 0 for k in ("frame_s", "wait_s", "format_s", "write_s"))
        if threshold[1]:
            assert 0 < passed < total
        # through CarrierGate.run, mapped file and input window included: the same lines behind the header
        raw = tmp_path / "x.bin"
        data.tofile(str(raw))
        st2 = gate.run(str(raw), str(tmp_path / "run.card"), timestamp=77.25)
        body = b"".join(ln + b"\n" for ln in (tmp_path / "run.card").read_bytes().split(b"\n")
                        if ln and not ln.startswith(b"#"))
        assert body == want_text and st2["passed"] == passed
        # no descriptor: verdicts only
        st3 = gate.engine().run_gate(data, out_fd=None, skip=skip, batch_blocks=batch)
        assert (st3["blocks"], st3["passed"], st3["text_bytes"]) == (total, passed, 0)


def test_run_gate_card_copies_the_input_lines(tmp_path):
    n = 4096
    rng = np.random.default_rng(4)
    blocks = rng.integers(0, 256, (11, 2 * n), dtype=np.uint8)
    blocks[3] = 127
    blocks[8] = 127                      # two blocks without anything above the threshold
    lines = [block_data.card_line(100.5 + i, 50 - i, b) for i, b in enumerate(blocks)]
    text = ("# header\n" + "".join(lines[:5]) + "\n" + "".join(lines[5:])).encode()
    with fastcard.CarrierGate(n, 0, (1, -1), (1e4, 0.0), skip=0, batch_size=4) as gate:
        want_text, want_rec = _python_path(gate, text, True, None)
        assert want_text.decode() == "".join(ln for i, ln in enumerate(lines) if i not in (3, 8))
        for skip in (0, 2, 5, 20):
            gate.skip = skip
            rec = np.zeros(11, dtype=F.RECORD_DTYPE)
            path = tmp_path / ("out%d.card" % skip)
            with open(str(path), "wb") as f:
                st = gate.engine().run_gate(text, card=True, out_fd=f.fileno(), skip=skip, batch_blocks=4, rec_out=rec)
            keep = [i for i in range(skip, 11) if i not in (3, 8)]
            assert path.read_text() == "".join(lines[i] for i in keep)
            assert (st["blocks"], st["passed"]) == (max(0, 11 - skip), len(keep))
            assert rec[:st["blocks"]].tobytes() == want_rec[skip:].tobytes()
        gate.skip = 0


def test_run_gate_errors(tmp_path):
    n, h = 2048, 1022
    data = _stream(n, h, 12, 5)
    with fastcard.CarrierGate(n, h, (0, -1), (0.0, 0.0), skip=1, batch_size=4) as gate:
        eng = gate.engine()
        rd, wr = os.pipe()
        os.close(rd)
        os.close(wr)
        with pytest.raises(F.NativeError, match="write") as e:
            eng.run_gate(data, out_fd=wr, skip=1, batch_blocks=4)
        assert e.value.args[0].endswith("(code %d)" % F.ERR_DEVICE)
        with pytest.raises(F.NativeError, match="rec_out"):
            eng.run_gate(data, skip=1, batch_blocks=4, rec_out=np.zeros(5, dtype=F.RECORD_DTYPE))
        with pytest.raises(F.NativeError, match="malformed|payload|card"):
            eng.run_gate(b"1.0 2 abc\n", card=True)
        # the handle still works
        st = eng.run_gate(data, skip=1, batch_blocks=4)
        assert st["blocks"] == st["passed"] == 11
    det = F.Engine(n, h, np.ones(16), (0, 15, 0), (7, 110), (0, 15, 0), max_batch=4)
    with pytest.raises(F.NativeError, match="not a carrier gate"):
        det.run_gate(data)
    det.close()
