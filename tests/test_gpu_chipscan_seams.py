"""The chip-rate scan kernels (csrc/chipscan.hip) at the seams tests/test_gpu_chipscan.py does not reach, with
that file's yardstick (chipscan_ref.compare: REL, OFFSET_ABS, TIE, CURVATURE -- nothing new):

* the candidate loop of k_chip_scan.  A launch cuts a chunk's candidates into groups, one workgroup walks a
  group, and with the default cut on a 256-CU device every shape of the other file comes out at ONE candidate
  per group: the prefetch of the next bank slice, the parity of the reduction's double buffer, the reuse of
  the LDS rows behind the previous candidate's barrier and a short last group run there in no test.
  thr_debug_chipscan_fill moves the cut and thr_debug_chipscan_groups reports it; a pair's arithmetic does
  not depend on its place in a loop, so every cut must give the bytes of the one-candidate-per-group run,
  which the rest of the suite pins to the float64 restatement;
* peaks on the seams of the lag map n = n1 * 1024 + 2t + e (lane_scene): the three magnitudes of the offset
  fit come from ownership arithmetic that crosses thread, wave and row boundaries;
* a window mask that decides (mask_scene): more power just beyond a candidate's last lag than inside;
* template lengths at the edges of k_chip_bank's sample map (length_scene).

The scenes and their float64 figures: tests/chipscan_ref.py, asserted on the host by test_chipscan_host.py.

Candidates per group: 70 candidates cannot be cut into groups of exactly 16, the depth of the measured
workload (ceil(70 / 4) = 18, ceil(70 / 5) = 14), so the group scene runs at 14 and at 18 and its first 64
lengths run at exactly 16.

Not here: exact power ties between two lags (the first-maximum rule across waves).  No input was found that
yields bit-equal float32 powers after two transforms without being degenerate for the carrier stage too, and
a faked one would pin nothing."""
import numpy as np
import pytest

import chipscan_ref
from chipscan_ref import compare, engine, same
from thrifty_amd import _native

pytestmark = pytest.mark.gpu

N = 16384
CARRIER_LEN = 2455
# workgroups per launch aimed at -> candidates per group of 16 blocks x 70 candidates: one group per
# candidate, an even split, a short last group (70 = 23 * 3 + 1), either side of the measured workload's 16
# (70 = 5 * 14 = 3 * 18 + 16), one group per block
FILLS = [(16 * 70, 70, 1), (16 * 35, 35, 2), (16 * 24, 24, 3), (16 * 5, 5, 14), (16 * 4, 4, 18), (16, 1, 70)]
DEEP = 16 * 4


@pytest.fixture(scope="module")
def refs():
    """every scene's blocks, chips, lengths and float64 reference, computed once"""
    out = {}
    for name in ("lane", "mask", "length", "group"):
        blocks, chips, lengths = getattr(chipscan_ref, name + "_scene")()
        out[name] = (blocks, chips, lengths, chipscan_ref.scan(blocks, chips, lengths, CARRIER_LEN))
    return out


@pytest.fixture(scope="module")
def eng():
    e = engine(CARRIER_LEN, max_batch=16)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cs(eng):
    return _native.ChipScan(eng)


@pytest.fixture(scope="module")
def baseline(cs, refs):
    """the group scene with the default cut: (records, carrier records)"""
    blocks, chips, lengths, _ = refs["group"]
    cs.set_fill(0)
    cs.set_bank_budget(0)
    return cs.scan(blocks, chips, lengths, with_carrier=True)


def default_fill(cs):
    """the workgroups a launch aims at by default: one block's candidates get a group each up to that many"""
    fill = 1
    while cs.groups(1, fill + 1)[1] == 1:
        fill += 1
    return fill


# ------------------------------------------------------------------ lanes, mask, lengths
def test_peaks_on_thread_wave_and_row_seams(cs, refs):
    blocks, chips, lengths, ref = refs["lane"]
    assert lengths[0] == 2461 and ref["sample"][:, 0].tolist() == chipscan_ref.LANE_LAGS
    got = cs.scan(blocks, chips, lengths)
    compare(got, ref, "lane")
    assert got["sample"][:, 0].tolist() == chipscan_ref.LANE_LAGS
    assert np.all(got["offset"][:, 0] != 0) and np.all((got["flags"][:, 0] & 2) != 0)


def test_the_window_mask_decides(cs, refs):
    blocks, chips, lengths, ref = refs["mask"]
    assert np.array_equal(ref["sample"][0, :4], N - lengths[:4]) and np.all(ref["offset"][0, :4] == 0)
    got = cs.scan(blocks, chips, lengths)
    assert compare(got, ref, "mask", max_excluded=0.0) == 0
    assert np.array_equal(got["sample"][0, :4], N - lengths[:4])
    assert np.all(got["offset"][0, :4] == 0.0)


def test_template_lengths_at_the_banks_edges(cs, refs):
    blocks, chips, lengths, ref = refs["length"]
    assert lengths.tolist() == [1, 2, 3, 64, 1023, 1024, 1025, 4097, 8191, 8192, 8193, N - 3, N - 2]
    got = cs.scan(blocks, chips, lengths)
    assert compare(got, ref, "length", max_excluded=0.0) == 0


# ------------------------------------------------------------------ the candidate loop
def test_the_loop_runs_and_changes_nothing(cs, refs, baseline):
    blocks, chips, lengths, ref = refs["group"]
    assert blocks.shape[0] == 16 and len(lengths) == 70
    base, _ = baseline
    compare(base, ref, "group, default cut")
    fill = default_fill(cs)
    groups, per = cs.groups(16, 70)
    print("default cut: %d workgroups aimed at, groups(16, 70) = (%d, %d)" % (fill, groups, per))
    assert (groups - 1) * per < 70 <= groups * per
    if fill <= 2 * 280:         # (a device of at most 280 CUs; beyond, the default is one candidate per group)
        assert per >= 2
    try:
        for fill, want_groups, want_per in FILLS:
            cs.set_fill(fill)
            assert cs.groups(16, 70) == (want_groups, want_per), fill
            print("fill %d: groups(16, 70) = (%d, %d)" % ((fill,) + cs.groups(16, 70)))
            assert same(cs.scan(blocks, chips, lengths), base), fill
        # the measured workload's depth itself: 64 candidates in 4 groups of 16
        cs.set_fill(DEEP)
        assert cs.groups(16, 64) == (4, 16)
        assert same(cs.scan(blocks, chips, lengths[:64]), base[:, :64])
    finally:
        cs.set_fill(0)
    assert cs.groups(16, 70) == (groups, per)
    assert same(cs.scan(blocks, chips, lengths), base)


def test_the_loop_across_bank_chunks_and_block_chunks(refs, baseline):
    blocks, chips, lengths, _ = refs["group"]
    base, car = baseline
    cut = engine(CARRIER_LEN, max_batch=4)          # 16 blocks: chunks of 4, the quiet block first in its chunk
    b = _native.ChipScan(cut)
    try:
        b.set_bank_budget(40 * 16384 * 8)         # 70 candidates: chunks of 40 and 30
        b.set_fill(4 * 14)
        assert b.geometry(70) == (40, False)
        # 40 = 13 * 3 + 1; the second chunk has fewer groups and another stride of the statistics
        assert b.groups(4, 40) == (14, 3) and b.groups(4, 30) == (10, 3)
        print("fill 56: groups(4, 40) = (%d, %d), groups(4, 30) = (%d, %d)" % (b.groups(4, 40) + b.groups(4, 30)))
        got, got_car = b.scan(blocks, chips, lengths, with_carrier=True)
        assert same(got, base) and same(got_car, car)
        assert got_car["block_idx"].tolist() == list(range(16))
    finally:
        b.set_fill(0)
        b.set_bank_budget(0)
        cut.close()


def test_a_quiet_block_inside_a_loop(cs, refs, baseline):
    blocks, chips, lengths, ref = refs["group"]
    base, _ = baseline
    assert not (ref["flags"][4] & 1).any() and (ref["flags"][[3, 5]] & 1).all()
    try:
        cs.set_fill(16)
        assert cs.groups(16, 70) == (1, 70)         # one workgroup per block walks all 70
        got = cs.scan(blocks, chips, lengths)
    finally:
        cs.set_fill(0)
    quiet = got[4]
    assert np.all(quiet["sample"] == -1) and np.all(quiet["flags"] == 0)
    assert np.all(quiet["energy"] == 0) and np.all(quiet["noise"] == 0) and np.all(quiet["offset"] == 0)
    assert same(got[3], base[3]) and same(got[5], base[5])
    compare(got, ref, "group, one group per block")


def test_back_to_back_calls_share_the_statistics_buffer(cs, refs, baseline):
    """the ChipStats buffer is reused and the m2 entries of neighbours outside [0, N) are never written: the
    mask scene's records (peaks at corr_len - 1) lie between two scans of the group scene, at other strides"""
    blocks, chips, lengths, _ = refs["group"]
    m_blocks, m_chips, m_lengths, m_ref = refs["mask"]
    base, _ = baseline
    try:
        cs.set_fill(DEEP)
        assert cs.groups(16, 70) == (4, 18)         # 70 = 3 * 18 + 16
        first = cs.scan(blocks, chips, lengths)
        between = cs.scan(m_blocks, m_chips, m_lengths)
        third = cs.scan(blocks, chips, lengths)
    finally:
        cs.set_fill(0)
    assert same(first, third) and same(first, base)
    compare(between, m_ref, "mask, between two group scans", max_excluded=0.0)
