"""GPU tests of template extraction (csrc/template_extract.hip, run_extract.hip, thrifty_amd.template_extract)
against the reference's own best_detection / extract_template (tests/golden/template_extract/).

Tolerance of the template, 1e-12 absolute: its values are O(1) and W <= 1023 here; a float64 sum of W
terms errs by at most about W * 2^-53 * max|x| ~ 2e-13, and the reference's FFT round trip adds 1.4e-15
(tests/test_template_extract_host.py).  Everything else -- the chosen block, its corr_sample, the number
of qualifying records, and every comparison between two runs of the engine -- is exact.
"""

import numpy as np
import pytest

import conftest
from extract_ref import TOL, cuts, same
from thrifty_amd import _native as F
from thrifty_amd import block_data, fastdet, synth, template_extract
from thrifty_amd.detect import Detector, DetectorSettings

pytestmark = pytest.mark.gpu

def load_golden(name):
    return conftest.load_golden("template_extract/" + name)


FIXTURES = ["extract_1024", "extract_2048", "extract_16384"]
_engines = {}


def engine_of(name):
    """One engine per fixture for the whole module (max_batch 64 > the 48 blocks)."""
    if name not in _engines:
        g = load_golden(name)
        _engines[name] = F.Engine(int(g["block_len"]), int(g["history_len"]), g["template"], g["carrier_thresh"],
                                  tuple(int(v) for v in g["carrier_window"]), g["corr_thresh"],
                                  carrier_len=len(g["template"]), max_batch=64)
    return _engines[name]


def settings_of(g, template=None):
    tpl = g["template"] if template is None else template
    return DetectorSettings(block_len=int(g["block_len"]), history_len=int(g["history_len"]), carrier_len=len(tpl),
                            carrier_thresh=tuple(g["carrier_thresh"]), template=tpl,
                            carrier_window=tuple(int(v) for v in g["carrier_window"]),
                            corr_thresh=tuple(g["corr_thresh"]))


def run(name, blocks, idx, stamps, sizes=48, max_offset=0.2):
    """Feed `blocks` in batches -> (record, timestamp, template, n_qualifying)."""
    g = load_golden(name)
    with F.Extraction(engine_of(name), max_offset) as x:
        for lo, hi in cuts(len(blocks), sizes):
            recs = x.feed(blocks[lo:hi], stamps[lo:hi], idx[lo:hi])
            assert np.array_equal(recs["block_idx"], idx[lo:hi])
        return x.result(len(g["template"]))


# ------------------------------------------------------------------ 1. parity with the reference
@pytest.mark.parametrize("fmt", ["u8", "c64"])
@pytest.mark.parametrize("pick", ["", "2"])
@pytest.mark.parametrize("name", FIXTURES)
def test_parity_with_the_reference(name, pick, fmt):
    g = load_golden(name)
    blocks = g["blocks"] if fmt == "u8" else np.stack([block_data.raw_to_complex(b) for b in g["blocks"]])
    rec, ts, tpl, nq = run(name, blocks, g["block_idx"], g["timestamps"], max_offset=float(g["max_offset" + pick]))
    k = int(g["chosen" + pick])
    err = float(np.max(np.abs(tpl - g["template_ref" + pick])))
    print("%s pick%s %s: block #%d, n_qualifying %d, max |template - reference| = %.3g"
          % (name, pick or "1", fmt, k, nq, err))
    assert int(rec["block_idx"]) == int(g["block_idx"][k]) and ts == float(g["timestamps"][k])
    assert int(rec["corr_sample"]) == int(g["sample"][k])
    assert nq == int(g["n_qualifying" + pick])
    assert rec["flags"] & F.FLAG_CORR and abs(rec["corr_offset"] - g["soff"][k]) <= 5e-6
    assert err <= TOL


# ------------------------------------------------------------------ 2. independence of batching
@pytest.mark.parametrize("name", FIXTURES)
def test_result_does_not_depend_on_the_batching(name):
    g = load_golden(name)
    args = (g["blocks"], g["block_idx"], g["timestamps"])
    whole = run(name, *args, sizes=48)
    for sizes in (1, 5, [47, 1]):
        assert same(whole, run(name, *args, sizes=sizes)), sizes
    # the winner in another batch: the run reversed (batches of 5: #1 of extract_2048 moves from the
    # first batch to the last)
    back = run(name, *(a[::-1].copy() for a in args), sizes=5)
    assert same(whole, back)


# ------------------------------------------------------------------ 3. the tie rule
@pytest.mark.parametrize("sizes", [5, 49])
@pytest.mark.parametrize("name", ["extract_1024", "extract_16384"])
def test_of_equal_energies_the_earlier_block_wins(name, sizes):
    g = load_golden(name)
    k = int(g["chosen"])
    base = run(name, g["blocks"], g["block_idx"], g["timestamps"])
    twin = g["blocks"][k:k + 1]
    # a byte-identical copy LATER in the run, under another index: the original stays the winner
    later = run(name, np.concatenate([g["blocks"], twin]), np.append(g["block_idx"], 9001),
                np.append(g["timestamps"], 5000.0), sizes=sizes)
    assert int(later[0]["block_idx"]) == int(g["block_idx"][k]) and later[1] == float(g["timestamps"][k])
    assert later[2].tobytes() == base[2].tobytes() and later[3] == base[3] + 1
    # the copy EARLIER in the run: now the copy wins
    earlier = run(name, np.concatenate([twin, g["blocks"]]), np.append(9001, g["block_idx"]),
                  np.append(5000.0, g["timestamps"]), sizes=sizes)
    assert int(earlier[0]["block_idx"]) == 9001 and earlier[1] == 5000.0
    assert earlier[2].tobytes() == base[2].tobytes() and earlier[3] == base[3] + 1
    for field in ("corr_sample", "corr_energy", "corr_offset", "carrier_bin"):
        assert earlier[0][field] == base[0][field] == later[0][field]


# ------------------------------------------------------------------ 4. input layouts
def card_text(g):
    return "".join(block_data.card_line(float(t), int(i), b)
                   for t, i, b in zip(g["timestamps"] + 0.25, g["block_idx"], g["blocks"])).encode()


@pytest.mark.parametrize("name", ["extract_1024", "extract_2048"])
def test_card_text_gives_what_the_blocks_give(name):
    g = load_golden(name)
    n, w = int(g["block_len"]), len(g["template"])
    text = card_text(g)
    ts, idx, off, end = F.frame_card(text, 0, len(text), n, True, 1000)
    assert end == len(text) and np.array_equal(idx, g["block_idx"])
    want = run(name, g["blocks"], idx, ts)
    eng = engine_of(name)
    with F.Extraction(eng) as x:
        x.feed_card(text, off, ts, idx)
        assert same(want, x.result(w)) and x.result(w)[1] == want[1]
        for batch in (1, 7):
            x.reset()
            st = x.run(text, card=True, batch_blocks=batch)
            assert st["blocks"] == 48 and st["batches"] == -(-48 // batch) and not st["index_error"]
            assert st["detections"] == int(g["det"].sum()) and st["text_bytes"] == 0
            got = x.result(w)
            assert same(want, got) and got[1] == want[1]


@pytest.fixture(scope="module")
def raw_capture(tmp_path_factory):
    """A raw capture at N = 1024, H = 512: 14 fixture blocks back to back, so every other one of the 28
    overlapping blocks holds a whole burst; the first block has the reference's zero history."""
    g = load_golden("extract_1024")
    path = str(tmp_path_factory.mktemp("raw") / "rx.raw")
    with open(path, "wb") as f:
        f.write(g["blocks"][20:34].tobytes())
    return path


def framed_reference(path, name="extract_1024"):
    """block_reader's framing on the host -> the extraction of those blocks through feed()."""
    g = load_golden(name)
    n, h, w = int(g["block_len"]), int(g["history_len"]), len(g["template"])
    with open(path, "rb") as f:
        items = list(block_data.block_reader(f, n, h))
    assert len(items) == 28 and [i for _, i, _ in items] == list(range(28))
    with F.Extraction(engine_of(name)) as x:
        x.feed(np.asarray(items[0][2], dtype=np.complex64)[None], [0.0], [0])        # zero history: complex64
        raws = np.stack([np.asarray(b.raw, dtype=np.uint8) for _, _, b in items[1:]])
        x.feed(raws, np.zeros(27), np.arange(1, 28))
        return x.result(w)


def test_raw_stream_gives_what_the_framed_blocks_give(raw_capture):
    g = load_golden("extract_1024")
    w = len(g["template"])
    want = framed_reference(raw_capture)
    assert want[3] >= 10                        # (the whole bursts)
    data = open(raw_capture, "rb").read()
    lead = np.zeros(1024, dtype=np.complex64)
    lead[512:] = block_data.raw_to_complex(np.frombuffer(data[:1024], dtype=np.uint8))
    with F.Extraction(engine_of("extract_1024")) as x:
        def lead_in():
            x.reset()
            x.feed(lead[None], [0.0], [0])
        lead_in()
        recs = x.feed_stream(data, first_block_idx=1, timestamps=np.zeros(27))
        assert np.array_equal(recs["block_idx"], np.arange(1, 28))
        assert same(want, x.result(w))
        for batch in (1, 7):
            lead_in()
            st = x.run(data, card=False, first_block_idx=1, timestamp=0.0, batch_blocks=batch)
            assert st["blocks"] == 27 and st["batches"] == -(-27 // batch)
            assert same(want, x.result(w))


def test_winner_in_the_zero_history_lead_in_is_kept_as_complex64(raw_capture):
    """The kept block may be a complex64 lead-in block while everything after it is u8."""
    g = load_golden("extract_1024")
    k, w = int(g["chosen"]), len(g["template"])
    z = block_data.raw_to_complex(g["blocks"][k])[None]
    others = np.delete(g["blocks"], k, axis=0)
    with F.Extraction(engine_of("extract_1024")) as x:
        x.feed(z, [1.5], [77])
        x.feed(others, np.zeros(47), np.arange(47))
        rec, ts, tpl, nq = x.result(w)
    assert int(rec["block_idx"]) == 77 and ts == 1.5 and nq == int(g["n_qualifying"])
    assert np.max(np.abs(tpl - g["template_ref"])) <= TOL


# ------------------------------------------------------------------ 5. the keep buffer survives
@pytest.mark.parametrize("name", FIXTURES)
def test_kept_block_survives_the_reuse_of_the_input_buffers(name):
    g = load_golden(name)
    k = int(g["chosen"])
    order = np.concatenate([np.arange(k - k % 12, k - k % 12 + 12), np.delete(np.arange(48), np.s_[k - k % 12:k - k % 12 + 12])])
    got = run(name, g["blocks"][order], g["block_idx"][order], g["timestamps"][order], sizes=12)   # winner's batch first
    assert int(got[0]["block_idx"]) == int(g["block_idx"][k])
    assert np.max(np.abs(got[2] - g["template_ref"])) <= TOL
    assert same(got, run(name, g["blocks"], g["block_idx"], g["timestamps"]))


# ------------------------------------------------------------------ 6. nothing qualifies
def test_nothing_qualifies_is_an_error_with_a_sentence_and_reset_recovers():
    import ctypes as C
    g = load_golden("extract_1024")
    n, w = int(g["block_len"]), len(g["template"])
    noise, _ = synth.synth_blocks(np.random.default_rng(3), 20, n, g["template"], (193, 705), signal_frac=0.0)
    eng = engine_of("extract_1024")
    with F.Extraction(eng) as x:
        recs = x.feed(noise)
        assert not np.any(recs["flags"] & F.FLAG_CORR)
        with pytest.raises(ValueError, match="no detection qualified"):
            x.result(w)
        nq = C.c_uint64(99)
        rc = eng._lib.thr_extract_result(x._x, None, None, None, 0, C.byref(nq))
        assert rc == F.ERR_STATE and nq.value == 0 and b"20 blocks" in eng._lib.thr_last_error()
        x.reset()
        x.feed(g["blocks"], g["timestamps"], g["block_idx"])
        rec, _, tpl, _ = x.result(w)
        assert int(rec["block_idx"]) == int(g["block_idx"][int(g["chosen"])])
        assert np.max(np.abs(tpl - g["template_ref"])) <= TOL
    with pytest.raises(ValueError, match="no detection qualified"):     # detections, but none with offset 0
        run("extract_1024", g["blocks"], g["block_idx"], g["timestamps"], max_offset=0.0)


def test_unsupported_handle_variants_are_refused():
    g = load_golden("extract_1024")
    n, h, tpl, thr, win = 1024, 512, g["template"], (0, 15, 0), (2, 60)
    others = [F.Engine(n, h, tpl, thr, win, thr, max_batch=8, preshift_num=21),
              F.Engine(n, h, tpl, (100.0, 2.0, 0), win, (100.0, 2.0, 0), max_batch=8, fastdet=True),
              F.Engine(n, h, np.stack([tpl, -tpl]), thr, win, thr, max_batch=8),
              F.Engine.gate(n, h, window=win, max_batch=8)]
    for eng, word in zip(others, ("preshift", "fastdet", "ONE base template", "carrier-gate")):
        with pytest.raises(F.NativeError, match=word) as err:
            F.Extraction(eng)
        assert "code -1" in str(err.value)
        eng.close()


# ------------------------------------------------------------------ 7. the command line and extract()
def _flags(g, base_path):
    return ["-b", str(int(g["block_len"])), "-y", str(int(g["history_len"])), "-w", "2-60", "-t", "15*snr",
            "-u", "15*snr", "-z", base_path]


def test_command_line_on_a_card_file(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    g = load_golden("extract_1024")
    k = int(g["chosen"])
    np.save("base.npy", g["template"])
    with open("rx.card", "wb") as f:
        f.write(b"# a header line\n" + card_text(g))
    assert template_extract.main(["rx.card", "-o", "new.npy", "--tpl", "new.tpl"] + _flags(g, "base.npy")) == 0
    new = np.load("new.npy")
    assert new.dtype == np.float64 and np.max(np.abs(new - g["template_ref"])) <= TOL
    assert np.array_equal(fastdet.load_tpl("new.tpl"), new.astype(np.float32))
    said = capsys.readouterr().out.strip().splitlines()[-1]
    assert said.startswith("Captured template from block #%d (timestamp: %.6f): offset=%+.3f; corr_ampl="
                           % (g["block_idx"][k], g["timestamps"][k] + 0.25, g["soff"][k]))
    assert abs(float(said.split("corr_ampl=")[1]) - g["energy"][k]) <= 2e-5 * g["energy"][k]
    # the second pick through the same door
    assert template_extract.main(["rx.card", "-o", "new2.npy", "--max-offset", repr(float(g["max_offset2"]))]
                                 + _flags(g, "base.npy")) == 0
    assert np.max(np.abs(np.load("new2.npy") - g["template_ref2"])) <= TOL
    assert ("block #%d " % g["block_idx"][int(g["chosen2"])]) in capsys.readouterr().out
    # the extracted template detects the block it came from
    with open("rx.card", "rb") as f, Detector(settings_of(g, new), block_data.CardStream(f, 1024)) as det:
        hits = {res.block: res for detected, res in det if detected}
    assert int(g["block_idx"][k]) in hits
    assert hits[int(g["block_idx"][k])].corr_info.sample == int(g["sample"][k])


def test_command_line_on_a_raw_capture(tmp_path, monkeypatch, capsys, raw_capture):
    monkeypatch.chdir(tmp_path)
    g = load_golden("extract_1024")
    np.save("base.npy", g["template"])
    want = framed_reference(raw_capture)
    assert template_extract.main([raw_capture, "--raw", "-o", "new.npy"] + _flags(g, "base.npy")) == 0
    assert np.load("new.npy").tobytes() == want[2].tobytes()
    assert ("block #%d " % want[0]["block_idx"]) in capsys.readouterr().out
    # the same capture from a pipe-like source: batches through feed / feed_stream
    with open(raw_capture, "rb") as f:
        items = list(block_data.block_reader(f, 1024, 512))
    tpl, res = template_extract.extract(settings_of(g), items)
    assert tpl.tobytes() == want[2].tobytes() and res.block == int(want[0]["block_idx"])
    assert res.corr_info.sample == int(want[0]["corr_sample"])
    with pytest.raises(SystemExit, match="no detection qualified"):
        template_extract.main([raw_capture, "--raw", "--max-offset", "0"] + _flags(g, "base.npy"))
