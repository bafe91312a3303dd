"""The template-extraction kernels (csrc/template_extract.hip) and their hook in the chunk loop
(csrc/pipeline.hip: extract_after_chunk) at the places where such code breaks: lanes, DPP rows, waves
and loop trips of k_best_fold, ties across those seams, chunks inside one call, the keep buffer over
time, the inclusive offset limit, the edges of the cut, and the 4096 / 65536 block lengths.

Every expectation about the CHOICE is exact and comes from tests/extract_ref.py on the records the
engine itself returned: the chosen block_idx, the timestamp (distinct per block), n_qualifying and the
winner record's bytes.  No energy or offset margin is involved.

Tolerance of the TEMPLATE against extract_ref.expected_template (float64 host formula): the derivation
of tests/test_gpu_template_extract.py -- a float64 sum of W terms of size O(1) errs by at most
W * 2^-53 * max|x| -- gives TOL = 1e-12 for W <= 1023.  For golden c3 (W = 4094) the same bound is
computed from W and max|expected_template|, times 4 for the four dependent passes (mean, deviation,
scale, recentre): max(1e-12, 4 * bound).  Between two runs of the engine the template is bit-identical.

Geometry: that of fixture extract_1024 (N = 1024, H = 512, W = 127, its template, thresholds and
windows) unless a test says otherwise.  A run is noise everywhere except at planted positions.  The
seeds below were checked on the CPU with oracle.thrifty_np.OracleDetector: none of the 16 noise blocks
passes even the carrier stage, every signal block is detected with |offset| <= 0.034 and the energies
of STRONG > MID > WEAK are 24.8 > 20.0 > 15.6; every test still asserts that from the returned records.
"""
import ctypes as C
import io

import numpy as np
import pytest

import conftest
from extract_ref import TOL, cuts, expected_pick, expected_template, qualifying, same, window_of
from thrifty_amd import _native as F
from thrifty_amd import block_data, synth

pytestmark = pytest.mark.gpu

N, H = 1024, 512
BIG = 2304                     # blocks of one k_best_fold launch: 1024 + 1024 + 256, three trips of its loop
NOISE_SEED, SIGNAL_SEED, DENSE_SEED, ORDER_SEED, EDGE_NOISE_SEED, EDGE_SEED = 101, 201, 301, 401, 501, 601
AMPS = np.linspace(0.16, 0.44, 15)
STRONG, MID, WEAK = 14, 10, 6                                    # indices into AMPS / the signal pool
DENSE_AMPS = (0.04, 0.05, 0.06, 0.08, 0.12, 0.2, 0.3, 0.4, 0.45)  # 256 blocks each; the weakest are not detected
THRESH, CARRIER_WINDOW, CARRIER_BINS = (0, 15, 0), (2, 60), (5.0, 55.0)


class Material(object):
    """Built once per module, never written to."""

    def __init__(self):
        g = conftest.load_golden("template_extract/extract_1024")
        self.tpl = tpl = g["template"]
        self.w = len(tpl)
        self.win = win = window_of(N, H, self.w)
        assert (int(g["block_len"]), int(g["history_len"]), self.w, win) == (N, H, 127, (193, 705))
        self.noise, _ = synth.synth_blocks(np.random.default_rng(NOISE_SEED), 16, N, tpl, win, signal_frac=0.0)
        rng = np.random.default_rng(SIGNAL_SEED)
        self.signal = np.concatenate([synth.synth_blocks(rng, 1, N, tpl, win, amp=float(a), carrier_bins=CARRIER_BINS)[0]
                                      for a in AMPS])
        rng = np.random.default_rng(DENSE_SEED)
        dense = np.concatenate([synth.synth_blocks(rng, BIG // len(DENSE_AMPS), N, tpl, win, amp=a, sigma=0.03,
                                                   carrier_bins=CARRIER_BINS)[0] for a in DENSE_AMPS])
        self.dense = dense[np.random.default_rng(ORDER_SEED).permutation(BIG)]
        for a in (self.noise, self.signal, self.dense):
            a.setflags(write=False)
        self.strong, self.mid, self.weak = self.signal[STRONG], self.signal[MID], self.signal[WEAK]

    def filler(self, n):
        """n noise blocks (the pool of 16, repeated), writable."""
        return self.noise[np.arange(n) % len(self.noise)].copy()

    def planted(self, n, plants):
        blocks = self.filler(n)
        for pos, block in plants.items():
            blocks[pos] = block
        return blocks


@pytest.fixture(scope="module")
def mat():
    return Material()


@pytest.fixture(scope="module")
def engines(mat):
    """engines(max_batch) / engines(max_batch, n, h, template, ...): one engine per setting for the whole
    module, closed at its teardown."""
    made = {}

    def get(max_batch, n=N, h=H, tpl=None, thresh=THRESH, window=CARRIER_WINDOW, key=None):
        key = key or (max_batch, n, h, len(mat.tpl if tpl is None else tpl))
        if key not in made:
            t = mat.tpl if tpl is None else tpl
            made[key] = F.Engine(n, h, t, thresh, window, thresh, carrier_len=len(t), max_batch=max_batch)
        return made[key]

    yield get
    for eng in made.values():
        eng.close()


def stamp_of(pos):
    return 1000.0 + pos


def idx_of(pos):
    return 7 + 3 * pos


class Feeder(object):
    """An extraction plus what went into it: the blocks and the records in feed order."""

    def __init__(self, eng, w, max_offset=0.2, tol=TOL, idx_of=idx_of):
        """tol: the template's tolerance, or a function of the expected template that gives it."""
        self.x = F.Extraction(eng, max_offset)
        self.eng, self.w, self.max_offset, self.tol, self.idx_of = eng, w, max_offset, tol, idx_of
        self.blocks, self.recs = [], []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.x.close()

    def _meta(self, n):
        pos = np.arange(len(self.blocks), len(self.blocks) + n)
        return stamp_of(pos), self.idx_of(pos)

    def took(self, blocks, recs):
        _, idx = self._meta(len(blocks))
        assert np.array_equal(recs["block_idx"], idx)
        self.blocks.extend(blocks)
        self.recs.append(recs)
        return recs

    def feed(self, blocks, sizes=None):
        """u8 [B, 2N] or complex64 [B, N], in one feed() or cut into `sizes`."""
        for lo, hi in cuts(len(blocks), sizes or len(blocks)):
            stamps, idx = self._meta(hi - lo)
            self.took(blocks[lo:hi], self.x.feed(blocks[lo:hi], stamps, idx))
        return self

    def feed_card(self, blocks):
        stamps, idx = self._meta(len(blocks))
        text = "".join(block_data.card_line(float(t), int(i), b) for t, i, b in zip(stamps, idx, blocks)).encode()
        ts, ix, off, end = F.frame_card(text, 0, len(text), self.eng.block_len, True, len(blocks) + 1)
        assert end == len(text) and np.array_equal(ix, idx) and np.array_equal(ts, stamps)
        self.took(blocks, self.x.feed_card(text, off, ts, ix))
        return self

    def reset(self):
        self.x.reset()
        self.blocks, self.recs = [], []

    def records(self):
        return np.concatenate(self.recs)

    def n_qualifying_of_an_empty_result(self):
        nq = C.c_uint64(99)
        rc = self.eng._lib.thr_extract_result(self.x._x, None, None, None, 0, C.byref(nq))
        assert rc == F.ERR_STATE
        return nq.value

    def check(self, label):
        """result() against the references -> (position, result).  Exact but for the template."""
        recs = self.records()
        want = expected_pick(recs, self.max_offset)
        if want is None:
            with pytest.raises(ValueError, match="no detection qualified"):
                self.x.result(self.w)
            assert self.n_qualifying_of_an_empty_result() == 0
            return None, None
        pos, count = want
        res = self.x.result(self.w)
        rec, ts, tpl, nq = res
        ref = expected_template(self.blocks[pos], recs["corr_sample"][pos], self.w)
        err = float(np.max(np.abs(tpl - ref)))
        tol = self.tol(ref) if callable(self.tol) else self.tol
        print("%s: position %d of %d, n_qualifying %d, max |template - expected_template| = %.3g (tolerance %.3g)"
              % (label, pos, len(recs), nq, err, tol))
        assert nq == count
        assert int(rec["block_idx"]) == self.idx_of(pos) and ts == stamp_of(pos)
        assert rec.tobytes() == recs[pos].tobytes()
        assert err <= tol
        again = self.x.result(self.w)
        assert same(res, again) and again[1] == ts
        return pos, res


def run(eng, w, blocks, sizes=None, max_offset=0.2, label="run", tol=TOL):
    """One whole run through a fresh extraction -> (records, position, result)."""
    with Feeder(eng, w, max_offset, tol) as f:
        f.feed(blocks, sizes)
        pos, res = f.check(label)
        return f.records(), pos, res


def equal(a, b):
    """same(), and the timestamp."""
    return same(a, b) and a[1] == b[1]


def only_the_plants_detect(recs, plants, max_offset=0.2):
    """The precondition of every planted run: no noise filler has FLAG_CORR, every plant qualifies."""
    corr = (recs["flags"] & F.FLAG_CORR) != 0
    at = sorted(plants)
    return np.array_equal(np.flatnonzero(corr), at) and bool(np.all(qualifying(recs, max_offset)[at]))


# ------------------------------------------------------------------ a. lanes, rows, waves, trips
FOLD_BATCHES = (65, 1025, 2049)       # each leaves a lone record in a new wave / a new trip of the fold's loop


@pytest.mark.parametrize("p", [0, 15, 16, 47, 48, 63, 64, 1023, 1024, 2047, 2048, 2303])
def test_winner_at_a_lane_row_wave_or_trip_seam(mat, engines, p):
    big = engines(BIG)
    plants = {p: mat.strong, (p + 700) % BIG: mat.mid, (p + 1500) % BIG: mat.weak}
    blocks = mat.planted(BIG, plants)
    recs, pos, res = run(big, mat.w, blocks, label="winner at %d" % p)          # ONE k_best_fold launch, three trips
    assert only_the_plants_detect(recs, plants)
    assert pos == p and res[3] == 3
    _, pos2, res2 = run(big, mat.w, blocks, label="  again")
    assert pos2 == p and equal(res, res2)
    for size in FOLD_BATCHES:
        _, pos_s, res_s = run(big, mat.w, blocks, sizes=size, label="  batches of %d" % size)
        assert pos_s == p and equal(res, res_s), size


@pytest.mark.parametrize("order", ["shuffled", "reversed"])
def test_dense_runs_count_and_pick_what_numpy_does(mat, engines, order):
    """Every lane of every wave of every trip holds a record with a burst; the weakest are not detected."""
    big = engines(BIG)
    blocks = mat.dense if order == "shuffled" else mat.dense[::-1].copy()
    recs, pos, res = run(big, mat.w, blocks, label="dense " + order)
    ok = qualifying(recs, 0.2)
    assert 1000 <= int(ok.sum()) <= BIG - 500          # a mix ...
    assert ok.reshape(BIG // 16, 16).any(axis=1).all()  # ... in every DPP row of every wave of every trip
    assert res[3] == int(ok.sum())
    for size in FOLD_BATCHES:
        _, pos_s, res_s = run(big, mat.w, blocks, sizes=size, label="  batches of %d" % size)
        assert pos_s == pos and equal(res, res_s), size


# ------------------------------------------------------------------ b. ties across the seams
TIES = [(5, 1029),         # the same thread on two trips
        (1000, 1029),      # a later thread holds the earlier block
        (63, 64),          # a wave seam
        (1023, 1024),      # a trip seam
        (2303, 0)]         # the last record of the last trip against the first of the first


@pytest.mark.parametrize("pair", TIES)
def test_of_equal_energies_across_a_seam_the_earlier_block_wins(mat, engines, pair):
    big = engines(BIG)
    first, last = min(pair), max(pair)
    runner_up = (first + 300) % BIG
    assert runner_up not in pair
    plants = {first: mat.strong, last: mat.strong, runner_up: mat.mid}
    blocks = mat.planted(BIG, plants)
    cut = (first + last + 1) // 2                      # first < cut <= last: the twins in different feed() calls
    results = []
    for sizes in (None, [cut, BIG - cut]):
        recs, pos, res = run(big, mat.w, blocks, sizes=sizes, label="twins at %d and %d, %s" % (first, last, sizes))
        assert only_the_plants_detect(recs, plants)
        # the engine is deterministic: the same bytes give bit-equal energies wherever they sit
        assert recs["corr_energy"][first].tobytes() == recs["corr_energy"][last].tobytes()
        assert recs["corr_energy"][runner_up] < recs["corr_energy"][first]
        assert pos == first and res[3] == 3
        results.append(res)
    assert equal(results[0], results[1])


# ------------------------------------------------------------------ c. chunking inside one call
@pytest.mark.parametrize("p", [0, 7, 8, 15, 16, 48, 49])
def test_chunks_of_one_call(mat, engines, p):
    """max_batch 8, 50 blocks in ONE call: 7 chunks (the last of 2) over the alternating pipe buffers;
    the hook sees first = 0, 8, ..., 48."""
    small, big = engines(8), engines(BIG)
    runner_up = (p + 20) % 50
    assert runner_up // 8 != p // 8
    plants = {p: mat.strong, runner_up: mat.mid}
    blocks = mat.planted(50, plants)
    recs, pos, res = run(small, mat.w, blocks, label="one feed of 50, winner at %d" % p)
    assert only_the_plants_detect(recs, plants)
    assert pos == p and res[3] == 2
    _, pos8, res8 = run(small, mat.w, blocks, sizes=8, label="  feeds of 8")
    _, posb, resb = run(big, mat.w, blocks, label="  max_batch %d" % BIG)
    assert pos8 == posb == p and equal(res, res8) and equal(res, resb)
    with Feeder(small, mat.w) as f:
        posc, resc = f.feed_card(blocks).check("  card text")
        assert only_the_plants_detect(f.records(), plants)
    assert posc == p and equal(res, resc)


@pytest.mark.parametrize("slot", [9, 13])
def test_chunks_of_one_raw_stream(mat, engines, slot):
    """14 blocks back to back = 27 overlapping blocks behind the zero-history lead-in; the strongest
    burst lies in source block `slot`, so the winner is block i > 0 of the third / fourth chunk of the
    stream (i * stride, not i * block bytes, into the staged bytes)."""
    small, big = engines(8), engines(BIG)
    source = mat.filler(14)
    source[1], source[3], source[slot] = mat.weak, mat.mid, mat.strong
    data = source.tobytes()
    items = list(block_data.block_reader(io.BytesIO(data), N, H))
    assert len(items) == 28 and [i for _, i, _ in items] == list(range(28))
    lead = np.asarray(items[0][2], dtype=np.complex64)[None]
    raws = np.stack([np.asarray(b.raw, dtype=np.uint8) for _, _, b in items[1:]])
    consecutive = lambda pos: 100 + pos             # (a stream numbers its blocks consecutively)
    # the reference: the host's framing, block by block
    with Feeder(big, mat.w, idx_of=consecutive) as f:
        f.feed(lead).feed(raws, sizes=1)
        pos, want = f.check("stream, slot %d: host framing block by block" % slot)
    assert pos >= 1 + 16 and (pos - 1) % 8 != 0 and want[3] >= 3
    # the framed blocks in ONE call of the small engine: four chunks of dense u8 blocks
    with Feeder(small, mat.w, idx_of=consecutive) as f:
        f.feed(lead).feed(raws)
        pos_f, got = f.check("  host framing in one call")
    assert pos_f == pos and equal(want, got)
    # the stream itself, framed on the device, with per-block timestamps
    with Feeder(small, mat.w, idx_of=consecutive) as f:
        f.feed(lead)
        stamps, idx = f._meta(27)
        f.took(raws, f.x.feed_stream(data, first_block_idx=int(idx[0]), timestamps=stamps))
        pos_s, got = f.check("  feed_stream")
    assert pos_s == pos and equal(want, got)


# ------------------------------------------------------------------ d. the keep buffer over time
def test_keep_buffer_follows_the_winner_so_far(mat, engines):
    """improve, nothing better, only noise, improve again, noise: result() after each batch."""
    big = engines(BIG)
    noise = mat.filler(5)
    batches = [np.stack([noise[0], mat.mid, noise[1]]), np.stack([noise[2], mat.weak, noise[3], noise[4]]),
               noise, np.stack([noise[1], noise[0], mat.strong]), noise[:3]]
    with Feeder(big, mat.w) as f:
        seen = []
        for k, batch in enumerate(batches):
            pos, res = f.feed(batch).check("keep over time, batch %d" % k)
            seen.append((pos, res[3]))
        assert only_the_plants_detect(f.records(), {1: 0, 4: 0, 14: 0})
    assert seen == [(1, 1), (1, 2), (1, 2), (14, 3), (14, 3)]


@pytest.mark.parametrize("order", ["u8 then complex64", "complex64 then u8"])
def test_kept_block_changes_its_format_with_the_winner(mat, engines, order):
    big = engines(BIG)
    noise = mat.filler(3)
    one, two = np.stack([noise[0], mat.mid, noise[1]]), np.stack([noise[2], mat.strong])
    _, pos, want = run(big, mat.w, np.concatenate([one, two]), label="all u8")      # the u8 route
    assert pos == 4
    z = lambda blocks: np.stack([block_data.raw_to_complex(b) for b in blocks]).astype(np.complex64)
    with Feeder(big, mat.w) as f:
        if order == "u8 then complex64":
            pos1, res1 = f.feed(one).check(order + ": first batch")
            pos2, res2 = f.feed(z(two)).check(order + ": second batch")
        else:
            pos1, res1 = f.feed(z(one)).check(order + ": first batch")
            pos2, res2 = f.feed(two).check(order + ": second batch")
    assert (pos1, res1[3], pos2, res2[3]) == (1, 1, 4, 2)
    assert res2[2].tobytes() == want[2].tobytes() and res2[1] == want[1]
    assert res1[2].tobytes() != res2[2].tobytes()


def test_equal_energy_twin_in_a_later_batch_changes_nothing(mat, engines):
    big = engines(BIG)
    noise = mat.filler(3)
    with Feeder(big, mat.w) as f:
        pos, first = f.feed(np.stack([noise[0], mat.strong, noise[1]])).check("twin: first batch")
        assert pos == 1
        pos, second = f.feed(np.stack([noise[2], mat.strong])).check("twin: the twin as u8")
        assert pos == 1 and second[3] == 2
        z = block_data.raw_to_complex(mat.strong).astype(np.complex64)[None]
        pos, third = f.feed(z).check("twin: the twin as complex64")
        recs = f.records()
    assert pos == 1 and third[3] == 3
    assert recs["corr_energy"][1].tobytes() == recs["corr_energy"][4].tobytes() == recs["corr_energy"][5].tobytes()
    for later in (second, third):               # record (its block_idx), timestamp and template: the first one's
        assert later[0].tobytes() == first[0].tobytes() and later[1] == first[1] == stamp_of(1)
        assert later[2].tobytes() == first[2].tobytes()


def test_reset_forgets_the_run(mat, engines):
    big = engines(BIG)
    noise = mat.filler(6)
    with Feeder(big, mat.w) as f:
        pos, _ = f.feed(np.stack([noise[0], mat.strong, noise[1]])).check("before the reset")
        assert pos == 1
        f.reset()
        pos, _ = f.feed(noise).check("after the reset, noise only")
        assert pos is None and not np.any(f.records()["flags"] & F.FLAG_CORR)
        # a weaker burst than the forgotten winner, at a position the first run did not reach
        pos, res = f.feed(np.stack([noise[2], mat.weak])).check("after the reset, a weaker burst")
        assert pos == 7 and res[3] == 1


# ------------------------------------------------------------------ e. the inclusive limit
def test_offset_limit_is_inclusive(mat, engines):
    """max_offset set to a record's own |corr_offset| admits it; the next double towards zero does not."""
    big = engines(BIG)
    blocks = mat.dense[:192]
    recs, winner, _ = run(big, mat.w, blocks, label="limit 0.2")
    ok = qualifying(recs, 0.2)
    assert ok.sum() >= 50
    without = recs.copy()
    without["flags"][winner] &= ~np.uint32(F.FLAG_CORR)
    runner_up, _ = expected_pick(without, 0.2)
    assert runner_up != winner and ok[runner_up]
    offsets = np.abs(recs["corr_offset"].astype(np.float64))
    for who, at in (("runner-up", runner_up), ("winner", winner)):
        a = float(offsets[at])
        below = float(np.nextafter(a, 0))
        assert 0 < below < a <= 0.2 and int((offsets[ok] == a).sum()) == 1
        recs_a, pos_a, res_a = run(big, mat.w, blocks, max_offset=a, label="limit = |offset| of the %s" % who)
        recs_b, pos_b, res_b = run(big, mat.w, blocks, max_offset=below, label="limit just below it")
        assert recs_a.tobytes() == recs.tobytes() == recs_b.tobytes()
        assert qualifying(recs_a, a)[at] and not qualifying(recs_b, below)[at]
        count_b = 0 if res_b is None else res_b[3]
        assert res_a[3] == count_b + 1
        if who == "winner":
            assert pos_a == winner and pos_b != winner          # the pick changes at the boundary
        elif a < offsets[winner]:
            assert pos_a == runner_up and pos_b != runner_up


# ------------------------------------------------------------------ f. the cut's edges
def edge_cases():
    """(N, H, template, W): W = 256 is one full trip of the cut's 256 threads, 512 two; 127 not even one."""
    return {"W256": (2048, 1024, lambda m: synth.gold_template(8, 2, sps=256 / 255), 256),
            "W512": (2048, 1024, lambda m: synth.gold_template(9, 2, sps=512 / 511), 512),
            "W127": (N, H, lambda m: m.tpl, 127)}


@pytest.mark.parametrize("edge", ["first", "last"])
@pytest.mark.parametrize("case", ["W256", "W512", "W127"])
def test_cut_at_the_edges_of_the_unique_window(mat, engines, case, edge):
    """One strong burst at the first / last lag a block owns (checked with the oracle on the CPU: detected
    at exactly that lag with |offset| <= 0.07 at every geometry here)."""
    n, h, make, w = edge_cases()[case]
    tpl = np.asarray(make(mat), dtype=np.float64)
    assert len(tpl) == w
    lo, hi = window_of(n, h, w)
    assert hi - lo == n - h and hi - 1 + w <= n
    lag = lo if edge == "first" else hi - 1
    eng = engines(16, n, h, tpl)
    noise, _ = synth.synth_blocks(np.random.default_rng(EDGE_NOISE_SEED), 4, n, tpl, (lo, hi), signal_frac=0.0)
    burst, _ = synth.synth_blocks(np.random.default_rng(EDGE_SEED), 1, n, tpl, (lo, hi), positions=[lag], amp=0.4,
                                  carrier_bins=CARRIER_BINS)
    blocks = np.concatenate([noise[:2], burst, noise[2:]])
    recs, pos, res = run(eng, w, blocks, label="%s, burst at the %s lag %d" % (case, edge, lag))
    assert only_the_plants_detect(recs, {2: 0})
    assert pos == 2 and int(res[0]["corr_sample"]) == lag
    assert abs(float(np.mean(res[2]))) <= 1e-15 * w
    _, _, res2 = run(eng, w, blocks, label="  again")
    assert equal(res, res2)


# ------------------------------------------------------------------ g. other block lengths
@pytest.mark.parametrize("name", ["small", "c3"])
def test_other_block_lengths(engines, name):
    """N = 4096 (golden small, W = 510) and N = 65536 (golden c3, W = 4094: the long path, and a copy
    loop of k_keep_block that makes 2 (u8) and 8 (complex64) trips).  Both goldens have more than two
    records that qualify at max_offset 0.2."""
    g = conftest.load_golden(name)
    n, h, tpl, blocks = int(g["block_len"]), int(g["history_len"]), g["template"], g["blocks"]
    w = len(tpl)
    eng = engines(32, n, h, tpl, tuple(g["carrier_thresh"]), tuple(int(v) for v in g["carrier_window"]), key=name)
    # the bound of the module docstring from this golden's W and max|expected_template|
    tol = TOL if w <= 1023 else (lambda ref: max(1e-12, 4 * w * 2.0 ** -53 * float(np.max(np.abs(ref)))))
    recs, pos, res = run(eng, w, blocks, label="%s u8" % name, tol=tol)
    assert qualifying(recs, 0.2).sum() >= 2 and res[3] == int(qualifying(recs, 0.2).sum())
    z = np.stack([block_data.raw_to_complex(b) for b in blocks]).astype(np.complex64)
    recs_z, pos_z, res_z = run(eng, w, z, label="%s complex64" % name, tol=tol)
    assert pos_z == pos and res_z[2].tobytes() == res[2].tobytes() and res_z[1] == res[1]
    # in batches that put the winner into a later call, and in one-block calls
    for sizes in (1, 3):
        _, pos_s, res_s = run(eng, w, blocks, sizes=sizes, label="  batches of %d" % sizes, tol=tol)
        assert pos_s == pos and equal(res, res_s)
