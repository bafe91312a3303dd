"""GPU tests of the averaged templates (csrc/template_average.hip, thr_extract_average*) against the statement
in plain Python integers (tests/average_ref.py).

Every expectation comes from average_ref on the records the engine itself returned, as the extraction's tests
do, so detection parity is not at stake here.  acc_e, acc_q, count and n_unclassified are EXACT (integer sums).
The template and the standard error are compared within the cut's bound of tests/test_gpu_template_extract.py,
max(1e-12, 4 W 2^-53 max|x|): the device sums W float64 terms in a fixed tree, NumPy pairwise.  Between two runs
of the engine every output is byte for byte the same, whatever the batching and the input form.
"""
import ctypes as C

import numpy as np
import pytest

import average_ref
import conftest
from extract_ref import cuts, qualifying, same
from thrifty_amd import _native as F
from thrifty_amd import block_data

pytestmark = pytest.mark.gpu

FIXTURES = ["extract_1024", "extract_2048", "extract_16384"]      # N / H / W: 1024/512/127, 2048/1024/510, 16384/4096/1023
MAX_OFFSET = 0.2
_engines = {}


def load_golden(name):
    return conftest.load_golden("template_extract/" + name)


def engine_of(name):
    """One engine per fixture for the whole module (max_batch 64)."""
    if name not in _engines:
        g = load_golden(name)
        _engines[name] = F.Engine(int(g["block_len"]), int(g["history_len"]), g["template"], g["carrier_thresh"],
                                  tuple(int(v) for v in g["carrier_window"]), g["corr_thresh"],
                                  carrier_len=len(g["template"]), max_batch=64)
    return _engines[name]


class Outputs(object):
    """Everything an armed extraction gives back, and the records that went into it."""

    def __init__(self, x, w, records, n_classes):
        self.records = records
        try:
            self.best = x.result(w)
        except ValueError:
            self.best = None
        self.count, self.n_unclassified = x.average_counts()
        self.classes = []
        for k in range(max(1, n_classes)):
            try:
                self.classes.append(x.average_result(k, w))
            except ValueError:
                self.classes.append(None)

    def blob(self):
        """Every output's bytes, in one string."""
        parts = [self.count.tobytes(), repr(self.n_unclassified).encode()]
        if self.best is not None:
            parts += [self.best[0].tobytes(), repr(self.best[1]).encode(), self.best[2].tobytes(),
                      repr(self.best[3]).encode()]
        for c in self.classes:
            parts += [b"-"] if c is None else [a.tobytes() for a in c]
        return b"|".join(parts)


def armed_run(eng, w, feed, classes=(), max_offset=MAX_OFFSET):
    """`feed(x)` feeds an extraction with averaging armed and returns the records in feed order."""
    with F.Extraction(eng, max_offset) as x:
        x.average(classes)
        return Outputs(x, w, feed(x), len(classes))


def dense(blocks, sizes=None):
    """One feed() of all the blocks, or feeds of `sizes`; block b carries index 7 + 3 b and timestamp 100 + b."""
    idx, stamps = 7 + 3 * np.arange(len(blocks)), 100.0 + np.arange(len(blocks))

    def feed(x):
        return np.concatenate([x.feed(blocks[lo:hi], stamps[lo:hi], idx[lo:hi])
                               for lo, hi in cuts(len(blocks), sizes or len(blocks))])
    return feed


def check(out, blocks, w, classes=(), max_offset=MAX_OFFSET, label=""):
    """The outputs against the statement on the run's own records: sums and counts exact, finish within the bound."""
    acc_e, acc_q, count, n_uncl = average_ref.accumulate(blocks, out.records, w, max_offset, classes)
    assert [int(c) for c in out.count[:len(count)]] == count and not out.count[len(count):].any()
    assert out.n_unclassified == n_uncl
    for k, got in enumerate(out.classes):
        if count[k] == 0:
            assert got is None
            continue
        tpl, sem, got_e, got_q = got
        assert np.array_equal(got_e, acc_e[k]) and np.array_equal(got_q, acc_q[k])
        want_tpl, want_sem, _ = average_ref.finish(acc_e[k], acc_q[k], count[k])
        tol = average_ref.tolerance(w, want_tpl)
        err_t, err_s = float(np.max(np.abs(tpl - want_tpl))), float(np.max(np.abs(sem - want_sem)))
        print("%s class %d: count %d, max |template - statement| = %.3g, max |sem - statement| = %.3g (bound %.3g)"
              % (label, k, count[k], err_t, err_s, tol))
        assert err_t <= tol and err_s <= tol
    return count, n_uncl


def split_classes(records, max_offset=MAX_OFFSET):
    """Two ranges that cut the qualifying records' carrier_bin + carrier_offset at their median, taken from a
    run's own records; a few of the lowest stay outside both."""
    v = np.sort([average_ref.record_value(r) for r in records[qualifying(records, max_offset)]])
    assert len(v) >= 4
    return [(float(v[1]), float(v[len(v) // 2])), (float(np.nextafter(v[len(v) // 2], np.inf)), float(v[-1]))]


# ------------------------------------------------------------------ 1. the statement, exactly
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("name", FIXTURES)
def test_sums_and_counts_are_the_statements(name, split):
    g = load_golden(name)
    eng, w, blocks = engine_of(name), len(g["template"]), g["blocks"]
    classes = split_classes(armed_run(eng, w, dense(blocks)).records) if split else ()
    out = armed_run(eng, w, dense(blocks), classes)
    count, n_uncl = check(out, blocks, w, classes, label="%s%s" % (name, " split" if split else ""))
    assert sum(count) + n_uncl == int(qualifying(out.records, MAX_OFFSET).sum()) == out.best[3]
    if split:
        assert count[0] >= 1 and count[1] >= 1 and n_uncl == 1
    # a repeated call gives the same bytes, and so does a repeated run
    assert armed_run(eng, w, dense(blocks), classes).blob() == out.blob()
    with F.Extraction(eng) as x:
        x.average(classes)
        x.feed(blocks)
        first = x.average_result(0, w)
        again = x.average_result(0, w)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))


# ------------------------------------------------------------------ 2. the single best is untouched
@pytest.mark.parametrize("name", FIXTURES)
def test_single_best_result_is_the_same_bytes_armed_or_not(name):
    g = load_golden(name)
    eng, w = engine_of(name), len(g["template"])
    with F.Extraction(eng) as x:
        x.feed(g["blocks"], g["timestamps"], g["block_idx"])
        plain = x.result(w)
        with pytest.raises(F.NativeError, match="not armed"):
            x.average_counts()
    for classes in ((), [(0.0, 1.0)]):          # (the second: every record unclassified)
        with F.Extraction(eng) as x:
            x.average(classes)
            x.feed(g["blocks"], g["timestamps"], g["block_idx"])
            armed = x.result(w)
        assert same(plain, armed) and plain[1] == armed[1]


# ------------------------------------------------------------------ 3. batching and input forms
def card_of(blocks):
    text = "".join(block_data.card_line(100.0 + i, i, b) for i, b in enumerate(blocks)).encode()
    ts, idx, off, end = F.frame_card(text, 0, len(text), blocks.shape[1] // 2, True, len(blocks) + 1)
    assert end == len(text)
    return text, ts, idx, off


@pytest.mark.parametrize("name", ["extract_1024", "extract_2048"])
def test_batching_and_card_text_give_identical_bytes(name):
    g = load_golden(name)
    eng, w = engine_of(name), len(g["template"])
    blocks = np.concatenate([g["blocks"]] * 3)                  # 144 blocks: chunks of 64 are 64 + 64 + 16
    classes = split_classes(armed_run(eng, w, dense(g["blocks"])).records)
    text, ts, idx, off = card_of(blocks)

    def stamped(sizes):
        def feed(x):
            return np.concatenate([x.feed(blocks[lo:hi], ts[lo:hi], idx[lo:hi]) for lo, hi in cuts(len(blocks), sizes)])
        return feed

    want = armed_run(eng, w, stamped(144), classes)             # one dense call (three chunks inside it)
    check(want, blocks, w, classes, label=name + " x 3")
    for sizes in (1, 7, 64):
        assert armed_run(eng, w, stamped(sizes), classes).blob() == want.blob(), sizes
    got = armed_run(eng, w, lambda x: x.feed_card(text, off, ts, idx), classes)
    assert got.blob() == want.blob()

    def whole_file(batch):
        def feed(x):
            recs = np.zeros(len(blocks), dtype=F.RECORD_DTYPE)
            st = x.run(text, card=True, batch_blocks=batch)
            assert st["blocks"] == len(blocks) and not st["index_error"]
            return recs
        return feed

    for batch in (7, 64):
        got = armed_run(eng, w, whole_file(batch), classes)      # thr_run_extract_card
        assert got.blob() == want.blob(), batch


def test_raw_stream_gives_the_bytes_of_its_framed_blocks():
    """14 fixture blocks back to back at N = 1024, H = 512: 27 overlapping blocks at a stride of 1024 bytes."""
    g = load_golden("extract_1024")
    eng, w = engine_of("extract_1024"), len(g["template"])
    data = g["blocks"][20:34].tobytes()
    buf = np.frombuffer(data, dtype=np.uint8)
    raws = np.stack([buf[1024 * j:1024 * j + 2048] for j in range(27)])
    want = armed_run(eng, w, lambda x: x.feed(raws, np.zeros(27), np.arange(1, 28)))
    count, _ = check(want, raws, w, label="framed stream")
    assert count[0] >= 10                       # (the whole bursts)
    got = armed_run(eng, w, lambda x: x.feed_stream(data, first_block_idx=1, timestamps=np.zeros(27)))
    assert np.array_equal(got.records["block_idx"], np.arange(1, 28)) and got.blob() == want.blob()
    for batch in (1, 7):                        # thr_run_extract_stream
        def feed(x, batch=batch):
            st = x.run(data, card=False, first_block_idx=1, timestamp=0.0, batch_blocks=batch)
            assert st["blocks"] == 27 and st["batches"] == -(-27 // batch)
            return want.records
        assert armed_run(eng, w, feed).blob() == want.blob(), batch


# ------------------------------------------------------------------ 4. what it is for
def test_averaged_template_is_closer_to_the_waveform_than_the_single_best():
    """The condition of tests/test_template_average_host.py on the device's output: 64 noisy transmissions of one
    filtered waveform; the r.m.s. error against the noise-free waveform, after the best scalar fit, is SMALLER
    for the averaged template than for the single best block's.  A condition, not a factor."""
    cap = average_ref.benefit_capture()
    eng = F.Engine(cap["n"], cap["h"], cap["base"], (0, 15, 0), (2, 60), (0, 15, 0), carrier_len=cap["w"], max_batch=64)
    try:
        out = armed_run(eng, cap["w"], dense(cap["blocks"]))
    finally:
        eng.close()
    check(out, cap["blocks"], cap["w"], label="benefit capture")
    assert out.count[0] >= 48
    err_avg = average_ref.fit_error(out.classes[0][0], cap["clean"])
    err_one = average_ref.fit_error(out.best[2], cap["clean"])
    print("averaged over %d: rms error %.4g; single best: %.4g; ratio %.3f"
          % (out.count[0], err_avg, err_one, err_avg / err_one))
    assert err_avg < err_one
    # the standard error says so too: its mean is below the single block's error
    assert float(np.mean(out.classes[0][1])) < err_one


def test_counts_survive_an_empty_class():
    g = load_golden("extract_1024")
    eng, w = engine_of("extract_1024"), len(g["template"])
    with F.Extraction(eng) as x:
        x.average([(-9.0, -8.0)])
        recs = x.feed(g["blocks"])
        with pytest.raises(ValueError, match="no detection qualified for class 0"):
            x.average_result(0, w)
        count, n_uncl = x.average_counts()
        assert not count.any() and n_uncl == int(qualifying(recs, MAX_OFFSET).sum()) >= 10
        acc = np.ones(w, dtype=np.uint64)
        rc = eng._lib.thr_extract_average_result(x._x, 0, None, None, w, acc.ctypes.data, None)
        assert rc == F.ERR_STATE and not acc.any()
        assert eng._lib.thr_extract_average_result(x._x, 1, None, None, w, None, None) == F.ERR_ARG
        small = np.zeros(w - 1)
        assert eng._lib.thr_extract_average_result(x._x, 0, small.ctypes.data, None, w - 1, None, None) == F.ERR_ARG
        n = C.c_uint64(0)
        assert eng._lib.thr_extract_average_counts(x._x, None, C.byref(n)) == 0 and n.value == n_uncl


# ------------------------------------------------------------------ 5. extract() and the command line
def _flags(g, base_path):
    return ["-b", str(int(g["block_len"])), "-y", str(int(g["history_len"])), "-w", "2-60", "-t", "15*snr",
            "-u", "15*snr", "-z", base_path]


def _settings(g):
    from thrifty_amd.detect import DetectorSettings
    tpl = g["template"]
    return DetectorSettings(block_len=int(g["block_len"]), history_len=int(g["history_len"]), carrier_len=len(tpl),
                            carrier_thresh=tuple(g["carrier_thresh"]), template=tpl,
                            carrier_window=tuple(int(v) for v in g["carrier_window"]), corr_thresh=tuple(g["corr_thresh"]))


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    """Fixture extract_1024 as a .card file with its base template, and what the library itself gives for it: the
    records, and per table of ranges the counts and every class's outputs."""
    g = load_golden("extract_1024")
    d = tmp_path_factory.mktemp("cli")
    text, ts, idx, off = card_of(g["blocks"])
    (d / "rx.card").write_bytes(b"# a header line\n" + text)
    np.save(str(d / "base.npy"), g["template"])
    eng, w = engine_of("extract_1024"), len(g["template"])
    one = armed_run(eng, w, lambda x: x.feed_card(text, off, ts, idx))
    v = np.sort([average_ref.record_value(r) for r in one.records[qualifying(one.records, MAX_OFFSET)]])
    # tx 5 and tx 9 share the records above the lowest; tx 7 holds the lowest alone; nobody reaches tx 3
    ranges = {5: (float(v[1]), float(v[len(v) // 2])), 9: (float(np.nextafter(v[len(v) // 2], np.inf)), float(v[-1])),
              7: (float(v[0]), float(v[0])), 3: (1000.0, 2000.0)}
    (d / "freqmap.cfg").write_text("".join("%d: %r - %r\n" % (t, lo, hi) for t, (lo, hi) in ranges.items())
                                   + "@4: 0\n@6: 0.5\n")
    mapped = armed_run(eng, w, lambda x: x.feed_card(text, off, ts, idx), list(ranges.values()))
    assert [int(c) for c in mapped.count[:4]] == [len(v) // 2, len(v) - len(v) // 2 - 1, 1, 0] and mapped.n_unclassified == 0
    return {"dir": d, "g": g, "w": w, "one": one, "ranges": ranges, "mapped": mapped, "n": len(v)}


def test_extract_returns_the_average_beside_its_result(capture):
    from thrifty_amd import template_extract
    g, w, d = capture["g"], capture["w"], capture["dir"]

    def run(**kw):
        with open(str(d / "rx.card"), "rb") as f:
            return template_extract.extract(_settings(g), block_data.CardStream(f, int(g["block_len"])), **kw)

    plain = run()
    assert type(plain) is tuple and len(plain) == 2
    got = run(average=True)
    template, result = got                                     # it keeps its result ...
    assert template.tobytes() == plain[0].tobytes() == capture["one"].best[2].tobytes()
    assert result.block == plain[1].block and result.timestamp == plain[1].timestamp
    avg = got.average                                          # ... and adds the average
    want = capture["one"]
    assert avg.txids == [0] and avg.count.tolist() == [capture["n"]] and avg.n_unclassified == 0
    assert avg.templates.shape == avg.sem.shape == avg.acc_e.shape == avg.acc_q.shape == (1, w)
    for have, ref in zip((avg.templates[0], avg.sem[0], avg.acc_e[0], avg.acc_q[0]), want.classes[0]):
        assert have.dtype == ref.dtype and have.tobytes() == ref.tobytes()
    # a {txid: (lo, hi)} dict: rows in the dict's order, NaN rows for the class nobody reaches
    got = run(average=True, classes=capture["ranges"])
    avg, want = got.average, capture["mapped"]
    assert got[0].tobytes() == plain[0].tobytes()
    assert avg.txids == [5, 9, 7, 3] and avg.count.tolist() == [int(c) for c in want.count[:4]]
    assert avg.n_unclassified == 0 and avg.templates.shape == (4, w)
    for k in range(3):
        for have, ref in zip((avg.templates[k], avg.sem[k], avg.acc_e[k], avg.acc_q[k]), want.classes[k]):
            assert have.tobytes() == ref.tobytes()
    assert np.isnan(avg.templates[3]).all() and np.isnan(avg.sem[3]).all()
    assert not avg.acc_e[3].any() and not avg.acc_q[3].any() and want.classes[3] is None
    # a list of ranges: classes 0 .. K-1; a raw capture is refused with the reason, before any feed
    lst = run(average=True, classes=list(capture["ranges"].values())[:2]).average
    assert lst.txids == [0, 1] and lst.count.tolist() == avg.count.tolist()[:2] and lst.n_unclassified == 1
    assert lst.templates[1].tobytes() == avg.templates[1].tobytes()
    with open(str(d / "rx.card"), "rb") as f:
        with pytest.raises(ValueError, match="u8 blocks"):
            template_extract.extract(_settings(g), block_data.RawStream(f, 1024, 512), average=True)


def test_command_line_writes_the_averaged_template(capture, monkeypatch, capsys):
    from thrifty_amd import fastdet, template_extract
    g, w, want = capture["g"], capture["w"], capture["one"]
    monkeypatch.chdir(capture["dir"])
    flags = _flags(g, "base.npy")
    # without --average: today's output, and none of the new files
    assert template_extract.main(["rx.card", "-o", "single.npy"] + flags) == 0
    single_said = capsys.readouterr().out.strip().splitlines()
    assert len(single_said) == 1 and single_said[0].startswith("Captured template from block #")
    assert np.load("single.npy").tobytes() == want.best[2].tobytes()
    # --average, no map
    assert template_extract.main(["rx.card", "-o", "captured.npy", "--average", "--npz", "sums.npz", "--tpl", "captured.tpl"]
                                 + flags) == 0
    said = capsys.readouterr().out.strip().splitlines()
    tpl, sem, acc_e, acc_q = want.classes[0]
    assert said[-2] == single_said[0]                           # the reference's sentence for the single best block
    assert said[-1] == "Averaged %d detections; template rms / mean sem = %.1f" % (
        capture["n"], np.sqrt(np.mean(tpl ** 2)) / np.mean(sem))
    new = np.load("captured.npy")
    assert new.dtype == np.float64 and new.tobytes() == tpl.tobytes() and new.tobytes() != want.best[2].tobytes()
    assert np.array_equal(fastdet.load_tpl("captured.tpl"), tpl.astype(np.float32))
    z = np.load("sums.npz")
    assert z["templates"].tobytes() == tpl.tobytes() and z["sem"].tobytes() == sem.tobytes()
    assert z["acc_e"].tobytes() == acc_e.tobytes() and z["acc_q"].tobytes() == acc_q.tobytes()
    assert z["count"].tolist() == [capture["n"]] and int(z["n_unclassified"]) == 0 and z["txids"].tolist() == [0]


def test_command_line_writes_one_template_per_transmitter(capture, monkeypatch, capsys):
    import os
    from thrifty_amd import fastdet, template_extract
    g, w, want = capture["g"], capture["w"], capture["mapped"]
    monkeypatch.chdir(capture["dir"])
    flags = _flags(g, "base.npy")
    argv = ["rx.card", "-o", "percls.npy", "--average", "--freq-map", "freqmap.cfg", "--rxid", "4"]
    assert template_extract.main(argv + ["--min-count", "2", "--npz", "percls.npz", "--tpl", "percls.tpl"] + flags) == 0
    said = capsys.readouterr().out.strip().splitlines()
    assert said[0].startswith("Captured template from block #") and len(said) == 4
    for line, k, txid in zip(said[1:3], (0, 1), (5, 9)):
        tpl, sem = want.classes[k][:2]
        assert line == "tx %d -> percls.tx%d.npy: Averaged %d detections; template rms / mean sem = %.1f" % (
            txid, txid, int(want.count[k]), np.sqrt(np.mean(tpl ** 2)) / np.mean(sem))
        assert np.load("percls.tx%d.npy" % txid).tobytes() == tpl.tobytes()
        assert np.array_equal(fastdet.load_tpl("percls.tx%d.tpl" % txid), tpl.astype(np.float32))
    assert said[3] == "Fewer than 2 detections, no template: tx 7 (1), tx 3 (0)"       # named, and not written
    for name in ("percls.npy", "percls.tx7.npy", "percls.tx3.npy", "percls.tx7.tpl", "percls.tpl"):
        assert not os.path.exists(name), name
    z = np.load("percls.npz")
    assert z["txids"].tolist() == [5, 9, 7, 3] and z["count"].tolist() == [int(c) for c in want.count[:4]]
    for k in range(3):
        assert z["templates"][k].tobytes() == want.classes[k][0].tobytes()
        assert z["acc_e"][k].tobytes() == want.classes[k][2].tobytes()
    assert np.isnan(z["templates"][3]).all() and np.isnan(z["sem"][3]).all()
    # the default --min-count 1 writes tx 7 too; receiver 6's ranges lie 0.5 higher, so the lowest record falls out
    assert template_extract.main(argv + flags) == 0
    said = capsys.readouterr().out.strip().splitlines()
    assert os.path.exists("percls.tx7.npy") and said[-1] == "Fewer than 1 detections, no template: tx 3 (0)"
    assert np.load("percls.tx7.npy").tobytes() == want.classes[2][0].tobytes()
    assert template_extract.main(argv[:-1] + ["6", "-o", "rx6.npy"] + flags) == 0
    said = capsys.readouterr().out
    assert "qualifying detections matched no transmitter of the map" in said and "tx 7 (0)" in said
    # nobody reaches the count: an exit with a sentence, after the short transmitters were named
    with pytest.raises(SystemExit, match="no transmitter reached 1000 detections"):
        template_extract.main(argv + ["--min-count", "1000", "-o", "none.npy"] + flags)
    assert "tx 5 (%d), tx 9 (%d), tx 7 (1), tx 3 (0)" % (want.count[0], want.count[1]) in capsys.readouterr().out
    assert not os.path.exists("none.tx5.npy")
