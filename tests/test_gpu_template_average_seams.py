"""The averaging kernels (csrc/template_average.hip) at the places where such code breaks: the tile of 256
samples (W below it, exactly it, with a tail), the chunk of C = 32 records (fewer, exactly, one more, many), a
class change inside a chunk and at its boundary, odd and even corr_sample, the first and the last lag of the
unique window with the cut ending on the last sample of the batch's last block, 2304 qualifying records in one
launch, the block lengths 4096, 16384 and 65536, saturated bytes, every shape of the class table, and the object's states.

Every expectation comes from tests/average_ref.py on the records the engine itself returned, and the sums and
counts are compared EXACTLY; each test asserts from those records that it reached the case it is named after.
Template and standard error: the cut's bound, max(1e-12, 4 W 2^-53 max|x|) (tests/test_gpu_template_average.py).

Geometry and material: those of tests/test_gpu_extract_seams.py (fixture extract_1024's N = 1024, H = 512,
W = 127, noise fillers that never detect, 15 planted bursts that always do, the dense run of 2304 blocks).
"""
import ctypes

import numpy as np
import pytest

import average_ref
import conftest
import test_gpu_extract_seams as seams
from extract_ref import qualifying, window_of
from test_gpu_template_average import MAX_OFFSET, armed_run, check, dense
from thrifty_amd import _native as F
from thrifty_amd import block_data, synth

pytestmark = pytest.mark.gpu

C = 32                          # kAvgChunk of csrc/template_average.hip: records per workgroup
N, H, BIG = seams.N, seams.H, seams.BIG


@pytest.fixture(scope="module")
def mat():
    return seams.Material()


@pytest.fixture(scope="module")
def engines(mat):
    made = {}

    def get(max_batch, n=N, h=H, tpl=None, thresh=seams.THRESH, window=seams.CARRIER_WINDOW, key=None):
        key = key or (max_batch, n, h, len(mat.tpl if tpl is None else tpl))
        if key not in made:
            t = mat.tpl if tpl is None else tpl
            made[key] = F.Engine(n, h, t, thresh, window, thresh, carrier_len=len(t), max_batch=max_batch)
        return made[key]

    yield get
    for eng in made.values():
        eng.close()


def plants_of(mat, at):
    """Position -> one of the 15 signal blocks, in turn."""
    return {int(p): mat.signal[i % len(mat.signal)] for i, p in enumerate(at)}


def values_of(records):
    ok = qualifying(records, MAX_OFFSET)
    return np.array([average_ref.record_value(r) for r in records[ok]])


# ------------------------------------------------------------------ a. records per launch
@pytest.mark.parametrize("count", [0, 1, 2, C - 1, C, C + 1])
def test_qualifying_records_per_launch(mat, engines, count):
    """A batch of 70 blocks = chunks of 32 + 32 + 6 in ONE launch, `count` of them bursts spread over all three."""
    eng = engines(BIG)
    at = (np.arange(count) * 69) // max(1, count - 1) if count > 1 else np.arange(count) + 33
    plants = plants_of(mat, at)
    blocks = mat.planted(70, plants)
    out = armed_run(eng, mat.w, dense(blocks))
    assert seams.only_the_plants_detect(out.records, plants) and len(plants) == count
    got, n_uncl = check(out, blocks, mat.w, label="%d of 70" % count)
    assert got == [count] and n_uncl == 0
    if count == 0:
        assert out.classes == [None] and out.best is None and not out.count.any()
        with F.Extraction(eng) as x:
            x.average(())
            x.feed(blocks)
            assert eng._lib.thr_extract_average_result(x._x, 0, None, None, 0, None, None) == F.ERR_STATE
            assert b"no detection qualified" in eng._lib.thr_last_error()
    if count >= 2:
        parity = out.records["corr_sample"][sorted(plants)] % 2
        assert count < 4 or (parity.min() == 0 and parity.max() == 1)      # odd and even corr_sample
        assert armed_run(eng, mat.w, dense(blocks, sizes=C - 1)).blob() == out.blob()


def test_every_lane_of_many_chunks(mat, engines):
    """2304 blocks in one launch (72 chunks), more than a thousand of them qualifying, in two classes."""
    eng = engines(BIG)
    first = armed_run(eng, mat.w, dense(mat.dense))
    v = np.sort(values_of(first.records))
    classes = [(float(v[0]), float(v[len(v) // 3])), (float(v[len(v) // 3]), float(v[-2]))]     # overlap at one value
    out = armed_run(eng, mat.w, dense(mat.dense), classes)
    count, n_uncl = check(out, mat.dense, mat.w, classes, label="dense")
    assert 1000 <= sum(count) <= BIG - 500 and min(count) >= 300 and n_uncl == 1
    assert check(first, mat.dense, mat.w, label="dense, one class")[0] == [sum(count) + 1]
    for sizes in (1025, C + 1):
        assert armed_run(eng, mat.w, dense(mat.dense, sizes=sizes), classes).blob() == out.blob(), sizes


def test_2304_qualifying_records_in_one_launch(mat, engines):
    """Every one of the 72 chunks of a launch full: the 15 signal blocks in turn, 2304 records, all qualifying."""
    eng = engines(BIG)
    blocks = mat.signal[np.arange(BIG) % len(mat.signal)]
    out = armed_run(eng, mat.w, dense(blocks))
    assert int(qualifying(out.records, MAX_OFFSET).sum()) == BIG
    count, n_uncl = check(out, blocks, mat.w, label="2304 of 2304")
    assert count == [BIG] and n_uncl == 0 and out.best[3] == BIG
    # three classes that interleave in every chunk (the signal blocks' own values), the same launch
    v = np.sort(np.unique(values_of(out.records)))
    assert len(v) == len(mat.signal)
    classes = [(float(v[0]), float(v[4])), (float(v[5]), float(v[9])), (float(v[10]), float(v[14]))]
    three = armed_run(eng, mat.w, dense(blocks), classes)
    count, n_uncl = check(three, blocks, mat.w, classes, label="2304 of 2304, three classes")
    assert sum(count) == BIG and min(count) >= 5 * (BIG // 15) and n_uncl == 0
    assert np.array_equal(sum(c[2] for c in three.classes), out.classes[0][2])
    assert armed_run(eng, mat.w, dense(blocks, sizes=1025)).blob() == out.blob()


# ------------------------------------------------------------------ b. class changes and the chunk
@pytest.mark.parametrize("layout", ["inside a chunk", "at the chunk boundary"])
def test_class_change(mat, engines, layout):
    eng = engines(BIG)
    probe = armed_run(eng, mat.w, dense(np.stack([mat.strong, mat.mid])))
    va, vb = values_of(probe.records)
    assert va != vb
    classes = [(va, va), (vb, vb)]              # lo == hi == a record's own carrier_bin + carrier_offset
    order = ([0, 1] * C) if layout == "inside a chunk" else ([0] * C + [1] * C)
    blocks = np.stack([mat.strong, mat.mid])[order]
    out = armed_run(eng, mat.w, dense(blocks), classes)
    count, n_uncl = check(out, blocks, mat.w, classes, label=layout)
    assert count == [C, C] and n_uncl == 0
    cls = [average_ref.class_of(average_ref.record_value(r), classes) for r in out.records]
    assert cls == order and cls[C - 1] != cls[C]
    # the other layout holds the same SET of records: the same sums
    other = np.stack([mat.strong, mat.mid])[order[::-1]]
    again = armed_run(eng, mat.w, dense(other), classes)
    assert all(np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) for a, b in zip(out.classes, again.classes))
    assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
               for a, b in zip(out.classes, again.classes))


# ------------------------------------------------------------------ c. the class table
def test_shapes_of_the_class_table(mat, engines):
    eng = engines(BIG)
    plants = plants_of(mat, np.arange(15) * 4 + 3)
    blocks = mat.planted(64, plants)
    none = armed_run(eng, mat.w, dense(blocks))
    assert seams.only_the_plants_detect(none.records, plants)
    v = np.sort(values_of(none.records))
    assert len(np.unique(v)) == 15
    tables = {
        "one range": [(float(v[0]), float(v[-1]))],
        "one range, lo == hi": [(float(v[7]), float(v[7]))],
        "overlapping": [(float(v[0]), float(v[9])), (float(v[5]), float(v[-1])), (float(v[5]), float(v[5]))],
        "a class nobody reaches": [(float(v[0]), float(v[-1])), (1000.0, 2000.0)],
        "every record unclassified": [(-20.0, -10.0), (float(np.nextafter(v[-1], np.inf)), 4000.0)],
        # 16: one per value (edges equal to the values themselves), the last one wide and empty
        "sixteen": [(float(a), float(a)) for a in v] + [(2000.0, 3000.0)],
    }
    for name, classes in tables.items():
        out = armed_run(eng, mat.w, dense(blocks), classes)
        count, n_uncl = check(out, blocks, mat.w, classes, label=name)
        want = {"one range": ([15], 0), "one range, lo == hi": ([1], 14), "overlapping": ([5, 9, 1], 0),
                "a class nobody reaches": ([15, 0], 0), "every record unclassified": ([0, 0], 15),
                "sixteen": ([1] * 15 + [0], 0)}[name]
        assert (count, n_uncl) == want, name
        assert out.best[2].tobytes() == none.best[2].tobytes()              # the single best: untouched
    # 17 ranges, an infinite bound, lo > hi: refused with a sentence
    with F.Extraction(eng) as x:
        o = F.ThrAverageOpts()
        for n_classes, lo, hi, word in ((17, 0.0, 1.0, "n_classes is 17"), (-1, 0.0, 1.0, "n_classes is -1"),
                                        (2, float("inf"), 1.0, "not finite"), (2, 0.0, float("nan"), "not finite"),
                                        (2, 2.0, 1.0, "lo 2 > hi 1")):
            o.n_classes = n_classes
            for k in range(16):
                o.lo[k], o.hi[k] = 0.0, 1.0
            o.lo[1], o.hi[1] = lo, hi
            assert eng._lib.thr_extract_average(x._x, ctypes.byref(o)) == F.ERR_ARG
            assert word.encode() in eng._lib.thr_last_error(), word


# ------------------------------------------------------------------ d. tiles of the cut, block lengths
def generated(mat, case):
    n, h, make, w = seams.edge_cases()[case]
    tpl = np.asarray(make(mat), dtype=np.float64)
    lo, hi = window_of(n, h, w)
    noise, _ = synth.synth_blocks(np.random.default_rng(seams.EDGE_NOISE_SEED), 3, n, tpl, (lo, hi), signal_frac=0.0)
    bursts, _ = synth.synth_blocks(np.random.default_rng(seams.EDGE_SEED), 5, n, tpl, (lo, hi), amp=0.4,
                                   carrier_bins=seams.CARRIER_BINS)
    return n, h, tpl, np.concatenate([noise[:2], bursts, noise[2:]]), seams.THRESH, seams.CARRIER_WINDOW


def golden(name):
    g = conftest.load_golden(name)
    return (int(g["block_len"]), int(g["history_len"]), g["template"], g["blocks"], tuple(g["carrier_thresh"]),
            tuple(int(v) for v in g["carrier_window"]))


TILE_CASES = {"W127 N1024": lambda m: golden("template_extract/extract_1024"),       # below one tile
              "W256 N2048": lambda m: generated(m, "W256"),                          # exactly one tile
              "W510 N2048": lambda m: golden("template_extract/extract_2048"),       # a tile and a tail of 254
              "W512 N2048": lambda m: generated(m, "W512"),                          # exactly two tiles
              "W1023 N16384": lambda m: golden("template_extract/extract_16384"),    # four tiles, the last short of 1
              "W510 N4096": lambda m: golden("small"),
              "W4094 N65536": lambda m: golden("c3")}                                # 16 tiles, the last of 254


@pytest.mark.parametrize("case", sorted(TILE_CASES))
def test_tiles_of_the_cut_and_block_lengths(mat, engines, case):
    n, h, tpl, blocks, thresh, window = TILE_CASES[case](mat)
    w = len(tpl)
    assert "W%d N%d" % (w, n) == case
    eng = engines(32, n, h, tpl, thresh, window, key=case)
    out = armed_run(eng, w, dense(blocks))
    count, _ = check(out, blocks, w, label=case)
    assert count[0] >= 2
    assert armed_run(eng, w, dense(blocks, sizes=3)).blob() == out.blob()
    # halves of the run, as two classes, add up to the whole: nothing of one tile leaks into another
    v = np.sort(values_of(out.records))
    classes = [(float(v[0]), float(v[len(v) // 2 - 1])), (float(v[len(v) // 2]), float(v[-1]))]
    two = armed_run(eng, w, dense(blocks), classes)
    check(two, blocks, w, classes, label=case + ", two classes")
    if len(np.unique(v)) == len(v):
        assert np.array_equal(two.classes[0][2] + two.classes[1][2], out.classes[0][2])
        assert np.array_equal(two.classes[0][3] + two.classes[1][3], out.classes[0][3])


# ------------------------------------------------------------------ e. the edges of the unique window
def edge_geometry(mat):
    """N = 1024 with H = W - 1 = 126: the unique window is [0, 898), so the first lag's cut begins on the block's
    first sample and the last lag's cut ends on its last."""
    n, h, w = N, mat.w - 1, mat.w
    lo, hi = window_of(n, h, w)
    assert (lo, hi) == (0, n - w + 1) and hi - 1 + w == n
    return n, h, w, lo, hi


@pytest.mark.parametrize("edge", ["first", "last"])
def test_cut_at_the_edges_of_the_block_in_the_last_block_of_the_batch(mat, engines, edge):
    n, h, w, lo, hi = edge_geometry(mat)
    lag = lo if edge == "first" else hi - 1
    eng = engines(8, n, h, mat.tpl, key="edges")
    noise, _ = synth.synth_blocks(np.random.default_rng(seams.EDGE_NOISE_SEED), 7, n, mat.tpl, (lo, hi), signal_frac=0.0)
    burst, _ = synth.synth_blocks(np.random.default_rng(seams.EDGE_SEED), 1, n, mat.tpl, (lo, hi), positions=[lag],
                                  amp=0.4, carrier_bins=seams.CARRIER_BINS)
    blocks = np.concatenate([noise, burst])                 # max_batch 8: the burst is the LAST block of the batch
    out = armed_run(eng, w, dense(blocks))
    ok = qualifying(out.records, MAX_OFFSET)
    assert ok[7] and int(out.records["corr_sample"][7]) == lag
    assert lag + w == n if edge == "last" else lag == 0
    count, _ = check(out, blocks, w, label="%s lag %d" % (edge, lag))
    assert count[0] == int(ok.sum()) >= 1
    # the same block through card text and as the last block of a raw stream's last batch
    text = "".join(block_data.card_line(1.0 + i, i, b) for i, b in enumerate(blocks)).encode()
    ts, idx, off, end = F.frame_card(text, 0, len(text), n, True, 9)
    card = armed_run(eng, w, lambda x: x.feed_card(text, off, ts, idx))
    assert card.classes[0][2].tobytes() == out.classes[0][2].tobytes()
    assert card.classes[0][0].tobytes() == out.classes[0][0].tobytes()


def test_last_block_of_a_raw_stream(mat, engines):
    """27 overlapping blocks in batches of 8 (8 + 8 + 8 + 3): the stream's last block ends the staged bytes."""
    eng = engines(8)
    source = mat.filler(14)
    source[1], source[3], source[13] = mat.weak, mat.mid, mat.strong
    data = source.tobytes()
    buf = np.frombuffer(data, dtype=np.uint8)
    stride = 2 * (N - H)
    raws = np.stack([buf[stride * j:stride * j + 2 * N] for j in range(27)])
    want = armed_run(eng, mat.w, lambda x: x.feed(raws, np.zeros(27), np.arange(27)))
    count, _ = check(want, raws, mat.w, label="framed stream")
    assert count[0] >= 3 and qualifying(want.records, MAX_OFFSET)[26]
    got = armed_run(eng, mat.w, lambda x: x.feed_stream(data, first_block_idx=0, timestamps=np.zeros(27)))
    assert got.records.tobytes() == want.records.tobytes() and got.blob() == want.blob()


# ------------------------------------------------------------------ f. saturated bytes
def saturated(mat, rng, position, carrier):
    """A burst so strong that the quantiser clips: both components sit at 0 or 255 for most of the cut."""
    z = rng.normal(0, 0.02, N) + 1j * rng.normal(0, 0.02, N)
    k = np.arange(mat.w)
    z[position:position + mat.w] += 3.0 * (mat.tpl + 1) / 2 * np.exp(2j * np.pi * carrier * (k + position) / N)
    f = np.asarray(z).astype(np.complex64).view(np.float32) * 128 + 127.4
    return np.clip(f, 0, 255).astype(np.uint8)


def test_saturated_bytes_are_summed_exactly(mat, engines):
    eng = engines(BIG)
    rng = np.random.default_rng(701)
    bursts = np.stack([saturated(mat, rng, p, c) for p, c in ((300, 20.3), (411, 31.0), (522, 44.6))])
    blocks = np.concatenate([mat.filler(2), bursts, mat.filler(1)])
    out = armed_run(eng, mat.w, dense(blocks))
    ok = qualifying(out.records, MAX_OFFSET)
    assert ok[2:5].any()
    pairs = np.concatenate([blocks[b][2 * s:2 * (s + mat.w)].reshape(-1, 2)
                            for b, s in zip(np.flatnonzero(ok), out.records["corr_sample"][ok])])
    both = lambda v: int(np.sum((pairs[:, 0] == v) & (pairs[:, 1] == v)))
    assert both(0) >= 5 and both(255) >= 5                  # (0, 0) and (255, 255): the largest q there is
    count, _ = check(out, blocks, mat.w, label="saturated")
    assert count[0] == int(ok.sum())
    assert int(out.classes[0][3].max()) >= 2 * 637 ** 2


# ------------------------------------------------------------------ g. the object's states
def test_reset_arming_and_complex_input(mat, engines):
    eng = engines(BIG)
    blocks = mat.planted(8, {2: mat.strong, 5: mat.mid})
    with F.Extraction(eng) as x:
        x.average(())
        x.feed(blocks)
        first = x.average_result(0, mat.w)
        assert x.average_counts()[0][0] == 2
        # arming or disarming after a feed: refused, and nothing changes
        for classes in ((), [(0.0, 100.0)], None):
            with pytest.raises(F.NativeError, match="before the first feed") as err:
                x.average(classes)
            assert "code -3" in str(err.value)
        assert x.average_counts()[0][0] == 2
        # complex64 while armed: refused with the reason
        z = np.stack([block_data.raw_to_complex(b) for b in blocks]).astype(np.complex64)
        with pytest.raises(F.NativeError, match="exact integers of the u8 quantiser") as err:
            x.feed(z)
        assert "code -1" in str(err.value)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, x.average_result(0, mat.w)))
        # reset zeroes the sums and keeps the arming
        x.reset()
        count, n_uncl = x.average_counts()
        assert not count.any() and n_uncl == 0
        acc = np.ones(mat.w, dtype=np.uint64)
        assert eng._lib.thr_extract_average_result(x._x, 0, None, None, mat.w, acc.ctypes.data, acc.ctypes.data) == F.ERR_STATE
        assert not acc.any()
        x.feed(blocks[:4])
        assert x.average_counts()[0][0] == 1
        half = x.average_result(0, mat.w)
        assert np.array_equal(half[2] + armed_run(eng, mat.w, dense(blocks[4:])).classes[0][2], first[2])
        # after a reset the arming may change; disarmed, complex64 is taken again and nothing is summed
        x.reset()
        x.average(None)
        x.feed(z)
        with pytest.raises(F.NativeError, match="not armed"):
            x.average_counts()
        assert int(x.result(mat.w)[3]) == 2
