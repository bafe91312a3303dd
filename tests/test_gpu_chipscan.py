"""The chip-rate scan on the device (thr_chipscan, _native.ChipScan, thrifty_amd.chip_rate_search) against
the float64 restatement tests/chipscan_ref.py, which test_chipscan_host.py pins to the reference's recorded
results.  Per (block, length): `sample` and `flags` exact, `energy` and `noise` within 1e-4 relative (the
project's float tolerance), `offset` within 1e-3 absolute where the reference's three log-magnitudes are not
within 1e-4 of collinear.  The index comparison leaves out a pair only where the reference's two largest
window magnitudes lie within 1e-4 relative of each other, at most 5 % of a case, none in the base scene.
Every comparison prints its largest deviations before it asserts (pytest -s)."""
import numpy as np
import pytest

import chipscan_ref
from chipscan_ref import REL, compare, engine, same     # (shared with test_gpu_chipscan_seams.py, unchanged)
from thrifty_amd import _native, chip_rate_search

pytestmark = pytest.mark.gpu

N = 16384


@pytest.fixture(scope="module")
def eng():
    e = engine(2455)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cs(eng):
    return _native.ChipScan(eng)


@pytest.fixture(scope="module")
def refs():
    """every scene's blocks, chips, lengths and float64 reference, computed once"""
    out = {}
    for name, carrier_len in (("base", 2455), ("mixed", 2455), ("edge", 2455), ("long", 4913), ("seam", 2455)):
        blocks, chips, lengths = getattr(chipscan_ref, name + "_scene")()
        blocks = np.atleast_2d(blocks)
        out[name] = (blocks, chips, lengths, chipscan_ref.scan(blocks, chips, lengths, carrier_len))
    return out


# ------------------------------------------------------------------ scenes against the restatement
def test_base_scene(cs, refs):
    blocks, chips, lengths, ref = refs["base"]
    assert len(lengths) == 61
    got, car = cs.scan(blocks, chips, lengths, with_carrier=True)
    assert compare(got, ref, "base", max_excluded=0.0) == 0
    best = int(np.argmax(got["energy"][0]))
    assert lengths[best] == 2461 and got["sample"][0, best] == 3000
    assert car["flags"].tolist() == [1] and car["carrier_bin"].tolist() == [40] and car["corr_sample"].tolist() == [-1]
    assert abs(car["carrier_offset"][0] - 0.3) < 0.05 and car["corr_energy"][0] == 0


@pytest.mark.parametrize("picked", [[2461], [2461, 2459], [2465, 2461, 2461, 2440], [2491, 2490, 2431]])
def test_output_order_is_the_lists(cs, refs, picked):
    blocks, chips, lengths, ref = refs["base"]
    cols = [int(np.flatnonzero(lengths == length)[0]) for length in picked]
    got = cs.scan(blocks, chips, np.array(picked, dtype=np.int32))
    compare(got, ref[:, cols], "picked %s" % picked)
    # a (block, length) pair does not depend on its neighbours in the list
    assert same(got, cs.scan(blocks, chips, lengths)[:, cols])


def test_short_and_long_templates(refs):
    blocks, chips, lengths, ref = refs["long"]
    assert len(chips) == 2047 and lengths[0] == N - 2 and ref["sample"][0, 0] == 1
    e = engine(4913)
    try:
        got = _native.ChipScan(e).scan(blocks, chips, lengths)
    finally:
        e.close()
    compare(got, ref, "long")


def test_peaks_at_the_first_and_the_last_lag(cs, refs):
    blocks, chips, lengths, ref = refs["edge"]
    assert ref["sample"][0, 0] == 0 and ref["sample"][1, 0] == N - 2461 and np.all(ref["offset"][:, 0] == 0)
    got = cs.scan(blocks, chips, lengths)
    compare(got, ref, "edge")
    assert np.all(got["offset"][:, 0] == 0) and np.all((got["flags"][:, 0] & 2) != 0)


def test_mixed_blocks(cs, refs):
    blocks, chips, lengths, ref = refs["mixed"]
    assert (ref["flags"][:, 0] & 1).tolist() == [1, 0, 1]
    got, car = cs.scan(blocks, chips, lengths, with_carrier=True)
    compare(got, ref, "mixed")
    assert (car["flags"] & 1).tolist() == [1, 0, 1] and car["carrier_bin"][[0, 2]].tolist() == [13, N - 301]
    assert same(got[:, 1], got[:, 4])          # the repeated length
    # the quiet block in the middle does not disturb its neighbours
    assert same(got[[0, 2]], cs.scan(blocks[[0, 2]], chips, lengths))
    # complex64 input takes the same path behind the converter
    x = np.stack([chipscan_ref.onp.iq_u8_to_c64(b) for b in blocks])
    compare(cs.scan(x, chips, lengths), ref, "mixed, complex64")


# ------------------------------------------------------------------ seams
def test_block_chunks_and_candidate_chunks(refs):
    blocks, chips, lengths, ref = refs["seam"]
    assert blocks.shape[0] == 9 and len(lengths) == 17
    whole = engine(2455, max_batch=16)
    cut = engine(2455, max_batch=4)             # 9 blocks: chunks of 4, 4 and 1
    try:
        a, b = _native.ChipScan(whole), _native.ChipScan(cut)
        per, paired = a.geometry(len(lengths))
        assert per == len(lengths) and not paired and a.geometry(100000)[0] == 512
        got, car = a.scan(blocks, chips, lengths, with_carrier=True)
        compare(got, ref, "seam")
        got_cut, car_cut = b.scan(blocks, chips, lengths, with_carrier=True)
        assert same(got, got_cut) and same(car, car_cut)
        assert car["block_idx"].tolist() == list(range(9))
        # the template bank in chunks of 8 candidates: 17 = 8 + 8 + 1, and one above a chunk: 9 = 8 + 1
        b.set_bank_budget(8 * 16384 * 8)
        assert b.geometry(17) == (8, False) and b.geometry(3) == (3, False)
        assert same(got, b.scan(blocks, chips, lengths))
        assert same(got[:, :9], b.scan(blocks, chips, lengths[:9]))
        b.set_bank_budget(0)
        assert b.geometry(17) == (17, False)
    finally:
        whole.close()
        cut.close()


def test_calls_are_independent_and_the_handle_gives_everything_back(refs):
    blocks, chips, lengths, ref = refs["mixed"]
    baseline = _native.live_resources()
    fresh = engine(2455)
    want = _native.ChipScan(fresh).scan(blocks, chips, lengths)
    fresh.close()
    assert _native.live_resources() == baseline
    e = engine(2455)
    try:
        scan = _native.ChipScan(e)
        other = refs["base"]
        first = scan.scan(blocks, chips, lengths)
        scan.scan(other[0], other[1], other[2])              # another shape in between
        second = scan.scan(blocks, chips, lengths)
        e.detect(blocks)                                       # the handle's own detect path in between
        third = scan.scan(blocks, chips, lengths)
        assert same(first, want) and same(second, want) and same(third, want)
        ms = scan.times()
        assert len(ms) == 3 and all(v > 0 for v in ms)
    finally:
        e.close()
    assert _native.live_resources() == baseline


# ------------------------------------------------------------------ refusals
def refused(code, fn, *args):
    before = _native.live_resources()
    with pytest.raises(_native.NativeError, match=r"\(code %d\)" % code) as err:
        fn(*args)
    assert _native.live_resources() == before           # nothing was allocated: no device work
    return str(err.value)


def test_refusals(eng, cs, refs):
    blocks, chips, lengths, _ = refs["base"]
    for bad in ([0], [N - 1], [2461, N - 1], [2461, -5], []):
        refused(-1, cs.scan, blocks, chips, np.array(bad, dtype=np.int32))
    refused(-1, cs.scan, blocks, np.zeros(2048, np.uint8), lengths)
    refused(-1, cs.scan, blocks, np.zeros(0, np.uint8), lengths)
    refused(-1, cs.scan, blocks, np.full(1023, 2, np.uint8), lengths)
    refused(-1, cs.scan, blocks[:0], chips, lengths)
    short = engine(600, block_len=4096)
    gate = _native.Engine.gate(N, 0, max_batch=4)
    multipass = engine(2455, path="multipass")
    try:
        text = refused(-1, _native.ChipScan(short).scan, np.zeros((1, 2 * 4096), np.uint8), chips, lengths)
        assert "block_len 4096" in text and "not supported" in text
        with pytest.raises(_native.NativeError, match=r"\(code -[13]\)"):
            _native.ChipScan(gate).scan(blocks, chips, lengths)
        refused(-1, _native.ChipScan(multipass).scan, blocks, chips, lengths)
        refused(-1, _native.ChipScan(short).geometry, 3)
    finally:
        short.close()
        gate.close()
        multipass.close()
    # while a submitted batch is open
    ticket = eng.submit(blocks)
    try:
        with pytest.raises(_native.NativeError, match=r"\(code -3\)"):
            cs.scan(blocks, chips, lengths)
    finally:
        eng.collect(ticket)
    assert cs.scan(blocks, chips, lengths[:2]).shape == (1, 2)


# ------------------------------------------------------------------ the tool
def test_scan_through_the_module(refs):
    blocks, chips, lengths, ref = refs["mixed"]
    result = chip_rate_search.scan(blocks, 2.4e6, 1.0e6, 10, lengths=lengths)
    want = chip_rate_search.scan(blocks, 2.4e6, 1.0e6, 10, lengths=lengths,
                                 backend=chipscan_ref.RefBackend())
    assert result.best_length == want.best_length == 2461 and result.carrier_ok.tolist() == [True, False, True]
    assert np.array_equal(result.sample, want.sample) and np.array_equal(result.detected, want.detected)
    assert np.all(np.abs(result.score - want.score) <= REL * want.score)
    assert result.best_rate == want.best_rate
