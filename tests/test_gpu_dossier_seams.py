"""k_pick and k_keep_slots (csrc/dossier.hip) where a batch holds more records than one trip of the pick's
workgroup covers: 2500 seeded blocks of 1024 samples in ONE batch, about half of them carrying a signal.
The slots must be the detected records in feed order -- boolean indexing of the plain detect records,
exactly -- with the cut of a smaller `max_keep` falling inside a trip, and every slot must hold the samples
of ITS block (the byte histogram of a slot is the histogram of the block at the slot's position).
Further down the same blocks, permuted so that detected ones sit on both sides of the trip boundaries
1023 | 1024 and 2047 | 2048 and fed under irregular block indices: cuts before, on and behind a boundary,
sixteen ranges, second feeds that start with slots filled, a trip that admits nothing; the pick rule is
dossier_ref.pick() on the plain detect records.  1223 of the 2500 blocks are detected, so a `max_keep` of
1300 keeps them all."""
import numpy as np
import pytest

import conftest
import dossier_ref as R
from oracle import thrifty_np as onp
from thrifty_amd import _native as F
from thrifty_amd import synth

pytestmark = pytest.mark.gpu

N, H, NB, SEED = 1024, 512, 2500, 20251
TOL_REL = 1e-4              # rms values (tests/test_gpu_dossier.py)


@pytest.fixture(scope="module")
def run():
    g = conftest.load_golden("template_extract/extract_1024")
    tpl = np.asarray(g["template"], dtype=np.float64)
    pad = H - len(tpl) + 1
    window = (pad // 2, N - len(tpl) + 1 - (pad - pad // 2))
    blocks, _ = synth.synth_blocks(np.random.default_rng(SEED), NB, N, tpl, window, signal_frac=0.5,
                                   carrier_bins=(5.0, 55.0))
    blocks.setflags(write=False)
    eng = F.Engine(N, H, tpl, (0, 15, 0), (2, 60), (0, 15, 0), max_batch=NB)
    idx = 7 + 2 * np.arange(NB)
    plain = eng.detect(blocks, idx)[:, 0]
    both = F.FLAG_CARRIER | F.FLAG_CORR
    detected = (plain["flags"] & both) == both
    assert 1000 < detected.sum() < 1500       # about half: more than one trip of 1024 records holds
    yield eng, blocks, idx, plain, detected
    eng.close()


@pytest.mark.parametrize("max_keep", [2000, 700])
def test_slots_are_the_detected_records_in_feed_order(run, max_keep):
    eng, blocks, idx, plain, detected = run
    stamps = 0.25 * np.arange(NB)
    with F.Dossiers(eng, ((None, None),), max_keep) as d:
        recs = d.feed(blocks, stamps, idx)
        assert recs.tobytes() == plain.tobytes()
        want = np.flatnonzero(detected)[:max_keep]
        last = want[-1] if len(want) == max_keep else NB - 1      # where the reference's loop stops
        assert d.n_kept == len(want)
        assert (d.n_checked, d.n_skipped) == (last + 1, int((~detected[:last + 1]).sum()))
        if max_keep == 700:
            assert want[-1] % 1024 not in (0, 1023) and want[-1] > 1024     # the cut lies inside the second trip
        got = d.result(arrays=("hist",))
        assert got["records"].tobytes() == plain[want].tobytes()
        assert np.array_equal(got["positions"], want.astype(np.uint64))
        assert np.array_equal(got["timestamps"], stamps[want])
        for k in (0, 1, len(want) // 2, len(want) - 2, len(want) - 1):
            assert np.array_equal(got["hist"][k], np.bincount(blocks[want[k]], minlength=256)), k
        same = sum(np.array_equal(got["hist"][k], np.bincount(blocks[want[k]], minlength=256)) for k in range(len(want)))
        assert same == len(want)


def test_complex64_slots_hold_their_own_blocks(run):
    """The complex64 copy of k_keep_slots across a trip: 1200 blocks as complex64, every slot's rms is the rms of
    the block at the slot's position (1e-4 relative, test_gpu_dossier.py's bound for rms values)."""
    eng, blocks, idx, plain, detected = run
    cx = np.stack([onp.iq_u8_to_c64(b) for b in blocks[:1200]])
    with F.Dossiers(eng, ((None, None),), 700) as d:
        recs = d.feed(cx, None, idx[:1200])
        assert recs.tobytes() == plain[:1200].tobytes()        # (complex64 input gives the u8 records)
        want = np.flatnonzero(detected[:1200])[:700]
        assert d.n_kept == len(want) > 500 and want[-1] > 1024
        got = d.result(arrays=("hist", "scalars"))
    assert np.array_equal(got["positions"], want.astype(np.uint64)) and not got["hist"].any()
    rms = np.sqrt(np.mean(np.abs(cx[want].astype(np.complex128)) ** 2, axis=1))
    assert np.all(np.abs(got["scalars"]["rms_unsynced"] - rms) <= TOL_REL * rms)
    assert len(np.unique(np.round(rms / (TOL_REL * rms.mean())))) > 100      # (the blocks' rms do differ by more)


# ------------------------------------------------------------------ cuts on a trip's edge, ranges, second feeds
TRIP = 1024
EDGE_PATTERN = {1022: False, 1023: True, 1024: True, 1025: False, 2047: True, 2048: True}
IDX_IRREGULAR = (np.arange(NB) * 7919) % 5003 - 1500        # distinct, not monotonic, some negative
STAMPS = 0.25 * np.arange(NB)


def edge_order(detected):
    """A permutation of the blocks that puts detected / undetected ones where EDGE_PATTERN says (each position
    takes the nearest later block of the kind it needs)."""
    order = np.arange(NB)
    for pos, want in EDGE_PATTERN.items():
        if detected[order[pos]] != want:
            other = next(p for p in range(pos + 1, NB) if p not in EDGE_PATTERN and detected[order[p]] == want)
            order[[pos, other]] = order[[other, pos]]
    return order


@pytest.fixture(scope="module")
def seamed(run):
    """The 2500 blocks with detected ones on both sides of the trip boundaries 1023 | 1024 and 2047 | 2048,
    under irregular block indices -> (engine, blocks, plain records, detected, every block's histogram)"""
    eng, blocks, _, _, detected = run
    blocks = blocks[edge_order(detected)]
    blocks.setflags(write=False)
    plain = eng.detect(blocks, IDX_IRREGULAR)[:, 0]
    detected = (plain["flags"] & (F.FLAG_CARRIER | F.FLAG_CORR)) == (F.FLAG_CARRIER | F.FLAG_CORR)
    assert {pos: bool(detected[pos]) for pos in EDGE_PATTERN} == EDGE_PATTERN     # detection does not depend on position
    hists = np.stack([np.bincount(b, minlength=256) for b in blocks])
    return eng, blocks, plain, detected, hists


def check_pick(d, got, plain, detected, hists, ranges, max_keep):
    kept, checked, skipped, _ = R.pick(IDX_IRREGULAR, detected, ranges, max_keep)
    assert (d.n_kept, d.n_checked, d.n_skipped) == (len(kept), checked, skipped)
    assert np.array_equal(got["positions"], np.array(kept, dtype=np.uint64))
    assert got["records"].tobytes() == plain[kept].tobytes()
    assert np.array_equal(got["timestamps"], STAMPS[kept])
    assert np.array_equal(got["hist"], hists[kept])
    return kept


@pytest.mark.parametrize("beyond", [-1, 0, 1])
def test_a_cut_before_on_and_behind_a_trip_boundary(seamed, beyond):
    eng, blocks, plain, detected, hists = seamed
    max_keep = int(detected[:TRIP].sum()) + beyond
    with F.Dossiers(eng, ((None, None),), max_keep) as d:
        assert d.feed(blocks, STAMPS, IDX_IRREGULAR).tobytes() == plain.tobytes()
        got = d.result(arrays=("hist",))
        kept = check_pick(d, got, plain, detected, hists, ((None, None),), max_keep)
    # the last slot: before the trip's last record, that record, the next trip's first
    assert len(kept) == max_keep and d.n_checked == kept[-1] + 1
    assert kept[-1] < TRIP - 2 if beyond < 0 else kept[-1] == (TRIP - 1, TRIP)[beyond]


def sixteen_ranges():
    v = IDX_IRREGULAR
    bands = [(int(lo), int(lo) + 150) for lo in np.linspace(-1300, 3100, 10)]
    return [(int(v[1023]), int(v[1023])), (int(v[2047]), int(v[2047])), (int(v[1024]), int(v[1024]) + 40),
            (int(v[2048]) - 40, int(v[2048])), (None, -1400), (3400, None)] + bands


@pytest.mark.parametrize("max_keep", [5, 300, 2000])
def test_sixteen_ranges_over_irregular_block_indices(seamed, max_keep):
    eng, blocks, plain, detected, hists = seamed
    ranges = sixteen_ranges()
    assert len(ranges) == 16 and any(lo == hi for lo, hi in ranges) and any(hi is None for _, hi in ranges)
    with F.Dossiers(eng, ranges, max_keep) as d:
        d.feed(blocks, STAMPS, IDX_IRREGULAR)
        got = d.result(arrays=("hist",))
        kept = check_pick(d, got, plain, detected, hists, ranges, max_keep)
    assert d.n_skipped > 0
    if max_keep == 2000:        # no cut: the ranges' edge records on both sides of both boundaries are kept
        assert 300 < len(kept) < 2000 and {1023, 1024, 2047, 2048} <= set(kept) and d.n_checked < NB
    else:
        assert len(kept) == max_keep


@pytest.mark.parametrize("split", [1500, 300])
def test_a_second_feed_that_starts_with_slots_filled(seamed, split):
    """k_keep_slots with batch_first != 0: the second feed's pick goes on from the first feed's slots (1500 + 1000:
    the rest is filled in its first trip; 300 + 2200: over two trips)."""
    eng, blocks, plain, detected, hists = seamed
    runs = []
    for cuts in ((0, NB), (0, split, NB)):
        with F.Dossiers(eng, ((None, None),), 1300) as d:
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                d.feed(blocks[lo:hi], STAMPS[lo:hi], IDX_IRREGULAR[lo:hi])
                if hi == split:
                    assert 0 < d.n_kept == detected[:split].sum() < 1100       # slots filled, more to fill
            got = d.result()
            check_pick(d, got, plain, detected, hists, ((None, None),), 1300)
            runs.append(((d.n_kept, d.n_checked, d.n_skipped), got))
    assert runs[0][0] == runs[1][0] and runs[0][0][0] == min(1300, detected.sum()) > 1100
    for name in runs[0][1]:
        assert runs[0][1][name].tobytes() == runs[1][1][name].tobytes(), name


def test_a_trip_that_admits_nothing_before_one_that_does(seamed):
    eng, blocks, plain, detected, hists = seamed
    picked = [1024, 1025, 1100, 1500, 2047, 2048, 2049, 2300, 2499]       # single block indices, none in the first trip
    ranges = [(int(IDX_IRREGULAR[p]), int(IDX_IRREGULAR[p])) for p in picked]
    with F.Dossiers(eng, ranges, 20) as d:
        d.feed(blocks, STAMPS, IDX_IRREGULAR)
        got = d.result(arrays=("hist",))
        kept = check_pick(d, got, plain, detected, hists, ranges, 20)
    assert kept == [p for p in picked if detected[p]] and {1024, 2047, 2048} <= set(kept) and 1025 not in kept
    assert (d.n_checked, d.n_skipped) == (len(picked), len(picked) - len(kept))
