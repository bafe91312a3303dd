"""K7, the order-preserving record compaction (k_compact_count / k_compact_scan / k_compact_scatter,
detect16k_carrier.hip; thr_compact_device), against boolean indexing -- with no tolerance: the
kernels move 64-byte records, so a mistake drops, duplicates, reorders or tears one.

The kernels have four seams of their own: a wave (64 records: the ballot prefix), a row (256: the
wave counts of one row are summed in LDS), a tile (2048: one workgroup, one entry of the scan) and a
scan chunk (1024 tiles = 2 097 152 records: k_compact_scan walks the tile counts 1024 at a time and
carries the running total in LDS).  The rows below put the record count on either side of each of
them and make the keep pattern change on them; the largest count takes three trips of the scan loop
with a partial last tile.

Records are synthetic: every field is a function of the record's index, so that each of the four
float4s a copy is made of names the record it came from.  The output buffer is pre-filled with a
sentinel byte; what lies past the kept records must still hold it (a scatter that writes one record
too many would otherwise go unseen).  thr_compact_device does not promise in-place compaction
(`d_in` and `d_out` must not overlap), so that is not tested.

  (a) without a GPU: the table holds every seam it claims, a non-zero carry into a second and a third
      scan trip occurs, the record builder marks all four float4s, the largest case's size
  (b) every (count, pattern) row against boolean indexing, small counts first, the large ones after
      them and a small one again after the largest -- all on ONE engine: the tile scratch buffer grows
      on demand and is then reused for fewer tiles
  (c) the (nb, 4) record array of a four-template engine, compacted, equals boolean indexing of
      its flattened form

Seeded mutations on scratch builds (every one only lowers a destination index or changes the count,
so all stores stay inside the output buffer): `carry = total` in k_compact_scan fails the 8 rows of
more than one trip (at two trips only the count is wrong), dropping `c +` from the tile offset fails
7 of them; neither is seen by the 2^20-record run of test_gpu_fullsize.py.  `if (w + 1 < wv)` in
k_compact_scatter's `before` sum fails 112 rows here, the first at 65 records, and
test_gpu_fullsize.py too."""
import numpy as np
import pytest

from oracle import thrifty_np as onp
from thrifty_amd import _native as F
from thrifty_amd import synth

WAVE, ROW, TILE = 64, 256, 2048          # detect16k_carrier.hip: 64 lanes, CMP_T, CMP_TILE
CHUNK = 1024 * TILE                      # records per trip of k_compact_scan's loop
REC = F.RECORD_DTYPE.itemsize
SENTINEL = 0xC5
PAD = 8                                  # sentinel records behind the last one that may be written
ALL_BITS = 0xFFFFFFFF
# flag words that are NOT a detection (no FLAG_CORR) and flag words that are; 7 and 5 of them, so that
# a pattern with a period of 2, 64, 256 or 2048 records still meets every word
DROPPED = (0, F.FLAG_CARRIER, F.FLAG_INDEX_ERROR, F.FLAG_FIT_UNCONVERGED, ALL_BITS & ~F.FLAG_CORR,
           F.FLAG_CARRIER | F.FLAG_INT_OFFSET, F.FLAG_INT_OFFSET)
KEPT = (F.FLAG_CORR, F.FLAG_CORR | F.FLAG_CARRIER, ALL_BITS, F.FLAG_CORR | F.FLAG_FIT_UNCONVERGED,
        F.FLAG_CORR | F.FLAG_CARRIER | F.FLAG_INT_OFFSET)

SMALL_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 3 * TILE + 100]
CHUNK_EDGE_SIZES = [CHUNK - 1, CHUNK + 1]
LARGEST = 2 * CHUNK + TILE + 1           # three trips, the last tile holds one record


def _idx(n):
    return np.arange(n, dtype=np.int64)


# keep patterns: name -> mask of n records
PATTERNS = {
    "none": lambda n: np.zeros(n, dtype=bool),
    "all": lambda n: np.ones(n, dtype=bool),
    "first_only": lambda n: _idx(n) == 0,
    "last_only": lambda n: _idx(n) == n - 1,
    "every_other": lambda n: (_idx(n) & 1) == 1,
    "waves_alternate": lambda n: ((_idx(n) // WAVE) & 1) == 0,
    "rows_alternate": lambda n: ((_idx(n) // ROW) & 1) == 1,
    "all_but_lane0": lambda n: (_idx(n) % WAVE) != 0,
    "all_but_lane63": lambda n: (_idx(n) % WAVE) != WAVE - 1,
    "tile_empty_between_full": lambda n: ((_idx(n) // TILE) % 3) != 1,
    "chunks_empty_full": lambda n: ((_idx(n) // CHUNK) & 1) == 1,      # carry 0 into trip 2
    "chunks_full_empty": lambda n: ((_idx(n) // CHUNK) & 1) == 0,      # carry 2 097 152 into trip 2
    "random_1pct": lambda n: np.random.default_rng(101).random(n) < 0.01,
    "random_50pct": lambda n: np.random.default_rng(150).random(n) < 0.50,
    "random_99pct": lambda n: np.random.default_rng(199).random(n) < 0.99,
}
LARGE_PATTERNS = ["all", "none", "chunks_empty_full", "chunks_full_empty", "every_other", "random_50pct",
                  "tile_empty_between_full"]
CHUNK_EDGE_PATTERNS = ["all", "last_only", "random_99pct"]

# (count, pattern) in the order they run on the one engine
SMALL_CASES = [(n, p) for n in SMALL_SIZES for p in PATTERNS]
LARGE_CASES = ([(n, p) for n in CHUNK_EDGE_SIZES for p in CHUNK_EDGE_PATTERNS]
               + [(LARGEST, p) for p in LARGE_PATTERNS])
AFTER_CASES = [(257, "all_but_lane0"), (TILE + 1, "random_50pct"), (1, "all"), (0, "none")]
CASES = SMALL_CASES + LARGE_CASES + AFTER_CASES


def make_records(n, mask):
    """n records whose every field is a function of the record's index; `flags` says kept / dropped
    according to `mask`, cycling through the flag words of either kind."""
    i = _idx(n)
    rec = np.zeros(n, dtype=F.RECORD_DTYPE)
    # float4 0: block_idx, flags, template_id
    rec["block_idx"] = i * 1000003 - 7
    rec["template_id"] = (i & 3).astype(np.int32)
    # float4 1: carrier_bin, corr_sample, carrier_offset
    rec["carrier_bin"] = i.astype(np.int32)
    rec["corr_sample"] = (~i).astype(np.int32)
    rec["carrier_offset"] = i.astype(np.float64) + 0.25
    # float4 2: corr_offset, carrier_energy, carrier_noise
    rec["corr_offset"] = -(i.astype(np.float64)) - 0.5
    rec["carrier_energy"] = (i % (1 << 24)).astype(np.float32)
    rec["carrier_noise"] = ((i >> 8) % (1 << 24)).astype(np.float32) + 0.5
    # float4 3: corr_energy, corr_noise, reserved
    rec["corr_energy"] = ((i * 3) % (1 << 24)).astype(np.float32)
    rec["corr_noise"] = (i % 8191).astype(np.float32)
    rec["reserved"] = i.astype(np.uint64) ^ np.uint64(0xA5A5A5A5A5A5A5A5)
    kept = np.asarray(KEPT, dtype=np.uint32)[i % len(KEPT)]
    dropped = np.asarray(DROPPED, dtype=np.uint32)[i % len(DROPPED)]
    rec["flags"] = np.where(mask, kept, dropped)
    return rec


def expected(rec):
    """The reference: boolean indexing."""
    return rec[(rec["flags"] & F.FLAG_CORR) != 0]


def carries(mask):
    """The running total k_compact_scan carries into its 2nd, 3rd ... trip."""
    return [int(mask[:k].sum()) for k in range(CHUNK, len(mask), CHUNK)]


# ---------------------------------------------------------------------------------------------
# (a) the table, without a GPU
# ---------------------------------------------------------------------------------------------
def test_the_flag_words_are_what_they_claim():
    assert all(not (f & F.FLAG_CORR) for f in DROPPED) and all(f & F.FLAG_CORR for f in KEPT)
    for name in ("FLAG_CARRIER", "FLAG_INDEX_ERROR", "FLAG_FIT_UNCONVERGED"):
        assert getattr(F, name) in DROPPED, name
    assert (ALL_BITS & ~F.FLAG_CORR) in DROPPED and ALL_BITS in KEPT
    assert len(DROPPED) % 2 == 1 and len(KEPT) % 2 == 1


def test_every_float4_of_a_record_names_its_index():
    n = 3 * TILE + 5
    rec = make_records(n, PATTERNS["every_other"](n))
    quads = rec.view(np.uint8).reshape(n, 4, 16)
    for q in range(4):
        # flags aside (float4 0 also holds block_idx), no two records share a float4: a copy that takes
        # one float4 from a neighbour -- or from any other record of these tiles -- is visible
        rows = {quads[i, q].tobytes() for i in range(n)}
        assert len(rows) == n, q
    # and the expected output depends on nothing but FLAG_CORR
    flags = rec["flags"]
    assert set(np.unique(flags[(flags & F.FLAG_CORR) == 0]).tolist()) == set(DROPPED)
    assert set(np.unique(flags[(flags & F.FLAG_CORR) != 0]).tolist()) == set(KEPT)
    assert len(expected(rec)) == n // 2


def test_the_table_holds_every_seam_it_claims():
    sizes = {n for n, _ in CASES}
    # either side of a wave, a row, a tile, two tiles, a scan
    # chunk, and three trips with a partial last tile
    for edge in (WAVE, ROW, TILE, 2 * TILE, CHUNK):
        assert {edge - 1, edge + 1} <= sizes, edge
    assert {0, 1, WAVE, ROW, TILE, 2 * TILE} <= sizes
    assert LARGEST == 2 * 1024 * 2048 + 2049 and LARGEST in sizes
    assert -(-LARGEST // CHUNK) == 3 and LARGEST % TILE == 1
    assert -(-(CHUNK - 1) // CHUNK) == 1 and -(-(CHUNK + 1) // CHUNK) == 2
    # every pattern runs at every small count; the named ones at the large counts
    assert set(SMALL_CASES) == {(n, p) for n in SMALL_SIZES for p in PATTERNS}
    assert len(set(SMALL_CASES + LARGE_CASES)) == len(SMALL_CASES) + len(LARGE_CASES)
    assert set(LARGE_CASES) >= {(LARGEST, p) for p in ("all", "none", "chunks_empty_full", "chunks_full_empty")}
    # order: small, then large, then small again (the tile scratch grows, then serves fewer tiles)
    order = [n for n, _ in CASES]
    first_large = min(k for k, n in enumerate(order) if n >= CHUNK - 1)
    last_large = max(k for k, n in enumerate(order) if n >= CHUNK - 1)
    assert max(order[:first_large]) < CHUNK - 1 and max(order[last_large + 1:]) <= TILE + 1
    assert order[last_large] == LARGEST and len(order) - last_large - 1 >= 3

    n = 3 * TILE + 100
    m = {p: f(n) for p, f in PATTERNS.items()}
    assert not m["none"].any() and m["all"].all()
    assert m["first_only"].sum() == 1 and m["first_only"][0]
    assert m["last_only"].sum() == 1 and m["last_only"][-1]
    assert np.array_equal(m["every_other"][:4], [False, True, False, True])
    w = m["waves_alternate"]
    assert w[:WAVE].all() and not w[WAVE:2 * WAVE].any() and w[2 * WAVE]      # changes at a wave boundary
    r = m["rows_alternate"]
    assert not r[:ROW].any() and r[ROW:2 * ROW].all()
    assert not m["all_but_lane0"][::WAVE].any() and m["all_but_lane0"].sum() == n - len(range(0, n, WAVE))
    assert not m["all_but_lane63"][WAVE - 1::WAVE].any() and m["all_but_lane63"][:WAVE - 1].all()
    t = m["tile_empty_between_full"]
    assert t[:TILE].all() and not t[TILE:2 * TILE].any() and t[2 * TILE:3 * TILE].all()
    for p, frac in (("random_1pct", 0.01), ("random_50pct", 0.5), ("random_99pct", 0.99)):
        assert abs(m[p].mean() - frac) < 0.02 and 0 < m[p].sum() < n
        assert np.array_equal(m[p], PATTERNS[p](n))                            # seeded
    # a tile that keeps nothing and one that keeps everything occur at a count with a partial last tile
    assert (TILE + 1, "tile_empty_between_full") in CASES and (2 * TILE + 1, "all") in CASES


def test_the_scan_carry_is_exercised():
    """Carry into the second trip: 0 in one row, a whole chunk in another; carry into the third trip
    non-zero; and rows where only part of a chunk is kept."""
    seen2, seen3 = set(), set()
    for n, p in LARGE_CASES:
        c = carries(PATTERNS[p](n))
        assert len(c) == -(-n // CHUNK) - 1
        if len(c) >= 1:
            seen2.add(c[0])
        if len(c) >= 2:
            seen3.add(c[1])
    assert 0 in seen2 and CHUNK in seen2 and any(0 < v < CHUNK for v in seen2)
    assert CHUNK in seen3 and 2 * CHUNK in seen3 and any(v not in (0, CHUNK, 2 * CHUNK) for v in seen3)
    assert carries(PATTERNS["chunks_empty_full"](LARGEST)) == [0, CHUNK]
    assert carries(PATTERNS["chunks_full_empty"](LARGEST)) == [CHUNK, CHUNK]
    # two trips: the chunk-edge counts
    assert carries(PATTERNS["all"](CHUNK + 1)) == [CHUNK] and carries(PATTERNS["all"](CHUNK - 1)) == []


def test_the_largest_case_fits_comfortably():
    # ~270 MB of records in, the same out (+ the sentinel pad), against 288 GB of HBM; on the host the
    # input, the expected output and the device's answer are alive together: under 1 GB
    assert 265e6 < LARGEST * REC < 275e6
    assert 3 * (LARGEST + PAD) * REC < 1e9
    assert LARGEST < 1 << 30                                   # thr_compact_device's own limit


# ---------------------------------------------------------------------------------------------
# (b) against boolean indexing, on a GPU
# ---------------------------------------------------------------------------------------------
def _engine(n_templates=1):
    n, h = 16384, 4096
    tpls = np.stack([synth.gold_template(10, 2 + t) for t in range(n_templates)]).astype(np.float64)
    return F.Engine(n, h, tpls if n_templates > 1 else tpls[0], (0, 15, 0), (7, 110), (0, 15, 0), max_batch=16)


def compact_and_check(torch, dev, eng, rec, label):
    n = len(rec)
    want = expected(rec).view(np.uint8).reshape(-1, REC)
    d_in = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy() if n else np.zeros(REC, np.uint8)).to(dev)
    d_out = torch.full(((n + PAD) * REC,), SENTINEL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()            # the fills ran on torch's stream, the engine has its own
    n_kept = eng.compact_device(d_in.data_ptr(), n, d_out.data_ptr())
    got = d_out.cpu().numpy()
    assert n_kept == len(want), (label, n_kept, len(want))
    body, rest = got[:n_kept * REC].reshape(-1, REC), got[n_kept * REC:]
    if not np.array_equal(body, want):
        first = int(np.flatnonzero((body != want).any(axis=1))[0])
        raise AssertionError("%s: output record %d is %r, expected %r" % (
            label, first, body[first].view(F.RECORD_DTYPE)[0], want[first].view(F.RECORD_DTYPE)[0]))
    assert body.tobytes() == want.tobytes(), label
    assert (rest == SENTINEL).all(), "%s: bytes past the %d kept records were written, first at byte %d" % (
        label, n_kept, int(np.flatnonzero(rest != SENTINEL)[0]))


@pytest.fixture(scope="module")
def shared():
    """ONE engine for the whole table, in table order: its tile scratch grows with the large counts and
    then serves the small ones that follow."""
    import torch
    eng = _engine()
    yield torch, torch.device("cuda", 0), eng
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,pattern", CASES, ids=["%d_%s_%d" % (n, p, k) for k, (n, p) in enumerate(CASES)])
def test_compaction_equals_boolean_indexing(shared, n, pattern):
    torch, dev, eng = shared
    compact_and_check(torch, dev, eng, make_records(n, PATTERNS[pattern](n)), "%d records, %s" % (n, pattern))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 65, 257, 2049])
def test_a_fresh_engine_at_each_seam(n):
    """The first compaction of an engine allocates the tile scratch: the first count past each seam on
    an engine of its own."""
    import torch
    eng = _engine()
    for pattern in ("all", "every_other", "all_but_lane0", "random_50pct"):
        compact_and_check(torch, torch.device("cuda", 0), eng, make_records(n, PATTERNS[pattern](n)),
                          "%d records, %s" % (n, pattern))
    eng.close()


# ---------------------------------------------------------------------------------------------
# (c) the record layout of a four-template engine
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_four_template_records_compact_like_their_flattened_form():
    """detect() of a T-template engine returns (nb, T) records, block-major; the four-template
    benchmark leg compacts exactly that buffer as nb * T records."""
    import torch
    n, h, nb = 16384, 4096, 300
    eng = _engine(4)
    assert eng.n_templates == 4
    rng = np.random.default_rng(44)
    blocks = np.empty((nb, 2 * n), dtype=np.uint8)
    for t in range(4):              # a quarter of the blocks carry each template's burst, a fifth are noise only
        tpl = synth.gold_template(10, 2 + t).astype(np.float64)
        part, _ = synth.synth_blocks(rng, nb // 4, n, tpl, onp.unique_window(n, h, len(tpl)), signal_frac=0.8)
        blocks[t::4] = part
    rec = eng.detect(blocks, np.arange(nb) * 5 - 40)
    assert rec.shape == (nb, 4) and rec.dtype == F.RECORD_DTYPE
    flat = rec.reshape(-1)
    keep = (flat["flags"] & F.FLAG_CORR) != 0
    # detections and empty records both occur, in the block-major order of the (nb, 4) array
    assert keep.any() and (~keep).any() and np.array_equal(flat["template_id"], np.tile(np.arange(4), nb))
    assert np.array_equal(flat["block_idx"], np.repeat(np.arange(nb) * 5 - 40, 4))
    compact_and_check(torch, torch.device("cuda", 0), eng, flat, "four templates, %d blocks" % nb)
    eng.close()
