"""GPU tests of thr_run_extract_card / thr_run_extract_stream on the paths they share with thr_run_card /
thr_run_stream (csrc/run_loop.hpp): the IndexError block, the sinks, the argument checks and bad input in
the middle of a file.  Every comparison is exact -- between two runs of the engine, or with counts read off
the fixture -- so there is no tolerance here.  What the extraction loop does differently from the detect
loop (its `blocks` count stops at the IndexError block, it runs without a sink) is pinned as it is."""
import os

import numpy as np
import pytest

import conftest
import test_gpu_detector_api as api
import test_gpu_template_extract as tx
from thrifty_amd import _native as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small():
    """(fixture, engine, its 48 blocks as .card text): extract_1024, the module-wide engine of the extraction tests."""
    g = tx.load_golden("extract_1024")
    return g, tx.engine_of("extract_1024"), tx.card_text(g)


def read_back(path):
    with open(path, "rb") as f:
        return f.read()


# ------------------------------------------------------------------ 1. the IndexError block
@pytest.mark.parametrize("batch", [2, 6])
def test_index_error_block_ends_the_extraction_run(batch):
    g = conftest.load_golden("c2_straddle")
    bad = np.flatnonzero(g["index_error"])
    assert list(bad) == [1, 4]
    lines = api.card_text(g).splitlines(True)                   # ("# synthetic", then one line per block)
    text = "".join(lines).encode()
    clean = "".join(ln for i, ln in enumerate(lines) if i - 1 not in set(bad.tolist())).encode()
    eng = F.Engine(int(g["block_len"]), int(g["history_len"]), g["template"], g["carrier_thresh"],
                   tuple(int(v) for v in g["carrier_window"]), g["corr_thresh"], carrier_len=len(g["template"]),
                   max_batch=8)
    with F.Extraction(eng) as x:
        rec_out = np.zeros(8, dtype=F.RECORD_DTYPE)
        st = x.run(text, card=True, batch_blocks=batch, rec_out=rec_out)
        assert st["index_error"] and st["index_error_at"] == 1
        assert st["index_error_block"] == int(g["block_idx"][1])
        assert st["blocks"] == 1                                # (up to the IndexError block, nothing behind it)
        assert st["detections"] == int(g["det"][:1].sum()) == 1
        assert int(rec_out[0]["block_idx"]) == int(g["block_idx"][0]) and not rec_out[1]["flags"]
        # the engine still detects, and after a reset the extraction runs through a clean file
        rec = eng.detect(g["blocks"][:1], g["block_idx"][:1])[:, 0]
        assert rec[0]["corr_sample"] == g["sample"][0]
        x.reset()
        st = x.run(clean, card=True, batch_blocks=batch)
        assert not st["index_error"] and st["blocks"] == 4 and st["detections"] == 4
        assert st["index_error_block"] == -1
        assert int(x.result(len(g["template"]))[0]["block_idx"]) in (0, 2, 3, 5)
    eng.close()


# ------------------------------------------------------------------ 2. same sink, same bytes
def both_loops(eng, tmp_path, extraction, plain):
    """Run `extraction(x, fd, rec)` and `plain(fd, rec)` into a descriptor and a record array each
    -> ((stats, text, records), (stats, text, records))."""
    out = []
    with F.Extraction(eng) as x:
        for name, call in (("x.toad", lambda fd, rec: extraction(x, fd, rec)), ("p.toad", plain)):
            path, rec = str(tmp_path / name), np.zeros(64, dtype=F.RECORD_DTYPE)
            fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
            try:
                st = call(fd, rec)
            finally:
                os.close(fd)
            out.append((st, read_back(path), rec))
    return out


def assert_same_sink(got, want, n):
    (st_a, text_a, a), (st_b, text_b, b) = got, want
    assert text_a == text_b and text_a.count(b"\n") == n
    assert a[:n].tobytes() == b[:n].tobytes() and not a[n:]["flags"].any()
    assert st_a["detections"] == st_b["detections"] == n
    assert st_a["text_bytes"] == st_b["text_bytes"] == len(text_a)
    assert st_a["blocks"] == st_b["blocks"] and st_a["batches"] == st_b["batches"]
    assert st_a["bytes_in"] == st_b["bytes_in"]


@pytest.mark.parametrize("batch", [1, 7])           # (48 = 6 * 7 + 6: the last batch is short)
def test_card_text_into_the_same_sinks_gives_the_detect_loops_bytes(small, tmp_path, batch):
    g, eng, text = small
    got, want = both_loops(
        eng, tmp_path,
        lambda x, fd, rec: x.run(text, card=True, batch_blocks=batch, out_fd=fd, rxid=0, rec_out=rec),
        lambda fd, rec: eng.run_card(text, out_fd=fd, rxid=0, batch_blocks=batch, rec_out=rec))
    n = int(g["det"].sum())
    assert_same_sink(got, want, n)
    assert got[0]["blocks"] == 48 and got[0]["batches"] == -(-48 // batch)
    ts = F.frame_card(text, 0, len(text), int(g["block_len"]), True, 1000)[0]
    stamps = np.ascontiguousarray(got[2][:n]["reserved"]).view(np.float64)     # one stamp per block: the lines' own
    assert len(set(ts)) > 1 and np.array_equal(stamps, ts[g["det"]])


@pytest.mark.parametrize("batch", [1, 7])
def test_raw_stream_into_the_same_sinks_gives_the_detect_loops_bytes(small, tmp_path, batch):
    g, eng, _ = small
    data = g["blocks"][20:34].tobytes()             # (as raw_capture of test_gpu_template_extract: 27 blocks behind the lead-in)
    got, want = both_loops(
        eng, tmp_path,
        lambda x, fd, rec: x.run(data, card=False, first_block_idx=1, timestamp=0.0, batch_blocks=batch, out_fd=fd,
                                 rxid=0, rec_out=rec),
        lambda fd, rec: eng.run_stream(data, first_block_idx=1, out_fd=fd, rxid=0, batch_blocks=batch, rec_out=rec,
                                       timestamp=0.0))
    n = want[0]["detections"]
    assert n >= 10                                  # (the whole bursts)
    assert_same_sink(got, want, n)
    assert got[0]["blocks"] == 27 and got[0]["batches"] == -(-27 // batch)
    assert not got[2][:n]["reserved"].any()         # one stamp per batch: the 0.0 that was asked for


# ------------------------------------------------------------------ 3. the argument checks
def test_run_arguments_are_checked(small):
    g, eng, text = small
    with F.Extraction(eng) as x:
        with pytest.raises(F.NativeError, match="more detections than rec_capacity"):
            x.run(text, rec_out=np.zeros(2, dtype=F.RECORD_DTYPE))
        x.reset()
        with pytest.raises(F.NativeError, match="batch_blocks %d exceeds the handle's max_batch" % (eng.max_batch + 1)):
            x.run(text, batch_blocks=eng.max_batch + 1)
        other = F.Engine(int(g["block_len"]), int(g["history_len"]), g["template"], g["carrier_thresh"],
                         tuple(int(v) for v in g["carrier_window"]), g["corr_thresh"],
                         carrier_len=len(g["template"]), max_batch=8)
        with F.Extraction(other) as y:
            y._eng = eng                            # (Extraction.run takes the handle from its engine)
            with pytest.raises(F.NativeError, match="belongs to another handle"):
                y.run(text)
            y._eng = other
        other.close()
        st = x.run(text)                            # no sink at all is fine here (not for thr_run_card)
        assert st["blocks"] == 48 and st["detections"] == int(g["det"].sum()) and st["text_bytes"] == 0


# ------------------------------------------------------------------ 4. bad input in the middle of a file
def test_bad_input_in_the_middle_ends_the_run_and_leaves_the_handle_usable(small):
    g, eng, text = small
    lines = text.decode().splitlines()
    pay = lines[6].split(" ")[2]
    # (1) a payload too short: the host framing refuses the line; (2) an invalid base64 character: the
    # device decode flags it at collect.  Batches of 3: lines 0-5 are the two batches before the bad one's
    malformed = "\n".join(lines[:6] + [lines[6][:-8]] + lines[7:]) + "\n"
    invalid = "\n".join(lines[:6] + [" ".join(lines[6].split(" ")[:2]) + " " + pay[:50] + "!" + pay[51:]]
                        + lines[7:]) + "\n"
    with F.Extraction(eng) as x:
        for bad, word in ((malformed, "payload"), (invalid, "base64")):
            x.reset()
            with pytest.raises(F.NativeError, match=word) as exc:
                x.run(bad.encode(), card=True, batch_blocks=3)
            st = exc.value.args[2]
            assert st["blocks"] == 6 and st["detections"] == int(g["det"][:6].sum())
            assert not st["index_error"] and st["index_error_block"] == -1
            # no ticket is left open: the handle detects, and the extraction runs again
            rec = eng.detect(g["blocks"][:2], g["block_idx"][:2])[:, 0]
            assert rec[0]["corr_sample"] == g["sample"][0]
            x.reset()
            assert x.run(text, batch_blocks=3)["blocks"] == 48
