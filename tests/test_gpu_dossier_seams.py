"""k_pick and k_keep_slots (csrc/dossier.hip) where a batch holds more records than one trip of the pick's
workgroup covers: 2500 seeded blocks of 1024 samples in ONE batch, about half of them carrying a signal.
The slots must be the detected records in feed order -- boolean indexing of the plain detect records,
exactly -- with the cut of a smaller `max_keep` falling inside a trip, and every slot must hold the samples
of ITS block (the byte histogram of a slot is the histogram of the block at the slot's position)."""
import numpy as np
import pytest

import conftest
from thrifty_amd import _native as F
from thrifty_amd import synth

pytestmark = pytest.mark.gpu

N, H, NB, SEED = 1024, 512, 2500, 20251


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
