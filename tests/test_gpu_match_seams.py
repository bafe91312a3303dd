"""`thr_match` at the seams of its kernels.  Every expectation is tests/match_ref.py's (itself held to
the reference's fixtures by tests/test_match_host.py), exact; a few cases also spell the answer out.
W is the workgroup size of every kernel of csrc/match.hip: sizes around a wave (64) and around W,
groups and (group, receiver) runs that cross workgroup boundaries, leader chains one past a power of
two (the last pointer-doubling round decides), and the comparisons at their edges."""
import numpy as np
import pytest

from match_ref import match_ref, to_csr
from thrifty_amd import _native

pytestmark = pytest.mark.gpu

W = _native.MATCH_WORKGROUP
NAN = float("nan")


def check(rx, tx, ts, en, window, min_match=2):
    """Device == sequential statement; -> (matches, misses, collisions) as lists."""
    want = match_ref(rx, tx, ts, en, window, min_match)
    ptr, idx, misses, collisions = _native.match(rx, tx, ts, en, window, min_match)
    want_ptr, want_idx = to_csr(want[0])
    assert ptr.tolist() == want_ptr
    assert idx.tolist() == want_idx
    assert misses.tolist() == want[1]
    assert [tuple(p) for p in collisions.tolist()] == want[2]
    return want


def grid_set(n, seed, n_rx=4, tx_lo=-1, tx_hi=3, rx_lo=0):
    """Timestamps on a 0.25 grid (sorted), energies from {1, 2, 3}: edges and ties everywhere."""
    rng = np.random.default_rng(seed)
    ts = np.sort(0.25 * rng.integers(0, max(2, n // 6), n))
    return (rng.integers(rx_lo, rx_lo + n_rx, n), rng.integers(tx_lo, tx_hi, n), ts,
            rng.integers(1, 4, n).astype(float))


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, W - 1, W, W + 1, 2 * W + 1, 20011])
def test_sizes_around_waves_and_workgroups(n):
    rx, tx, ts, en = grid_set(n, n)
    for window in (0.0, 0.5):
        check(rx, tx, ts, en, window)


def test_group_across_a_workgroup_boundary():
    n = 2 * W
    ts = np.arange(n, dtype=float)
    ts[W - 3:W + 4] = ts[W - 3]                     # one group of seven over positions W-3 .. W+3
    rx = np.arange(n) % 3
    matches, misses, _ = check(rx, np.zeros(n, int), ts, np.ones(n), 0.5)
    group = list(range(W - 3, W + 4))               # receivers in first-appearance order; ties: each one's last
    assert matches == [[max(j for j in group if rx[j] == r) for r in dict.fromkeys(rx[group].tolist())]]
    assert len(misses) == n - 7


@pytest.mark.parametrize("members", [65, W + 1, 3 * W])
def test_one_group_two_receivers_running_winner_across_seams(members):
    rng = np.random.default_rng(members)
    rx, en = rng.integers(0, 2, members), rng.integers(1, 4, members).astype(float)
    rx[:2] = [1, 0]
    matches, misses, collisions = check(rx, np.full(members, 7), np.zeros(members), en, 0.0)
    assert len(matches) == 1 and len(matches[0]) == 2 and misses == [] and len(collisions) == members - 2
    # a long strictly decreasing run keeps its first, a long constant run ends at its last
    down = np.arange(members, 0, -1).astype(float)
    matches, _, collisions = check(np.zeros(members, int), np.zeros(members, int), np.zeros(members), down, 0.0, 1)
    assert matches == [[0]] and collisions == [(0, j) for j in range(1, members)]
    matches, _, collisions = check(np.zeros(members, int), np.zeros(members, int), np.zeros(members), np.ones(members), 0.0, 1)
    assert matches == [[members - 1]] and collisions == [(j - 1, j) for j in range(1, members)]


@pytest.mark.parametrize("leaders", [1, 2, 3, 255, 256, 257, 65537])
def test_leader_chain_in_one_txid(leaders):
    ts = np.arange(leaders, dtype=float)
    rx = np.arange(leaders) % 2
    _, misses, _ = check(rx, np.zeros(leaders, int), ts, np.ones(leaders), 0.5)
    assert misses == list(range(leaders))            # each detection its own group
    if leaders <= 257:                                # two detections per group, two receivers: all match
        ts2, rx2 = np.repeat(ts, 2), np.tile([0, 1], leaders)
        matches, _, _ = check(rx2, np.zeros(2 * leaders, int), ts2, np.ones(2 * leaders), 0.5)
        assert matches == [[2 * g, 2 * g + 1] for g in range(leaders)]


def test_two_txids_interleaved_element_by_element():
    n = 2 * W + 1
    rng = np.random.default_rng(11)
    ts = 0.25 * (np.arange(n) // 2)
    check(rng.integers(0, 3, n), np.arange(n) % 2, ts, rng.integers(1, 4, n).astype(float), 0.5)
    check(rng.integers(0, 3, n), np.where(np.arange(n) % 2, -1, 5), ts, rng.integers(1, 4, n).astype(float), 0.25)


def test_window_edge_is_inclusive_and_one_ulp_above_is_not():
    t0, window = 1.7e9 + 0.1, 0.2
    edge = t0 + window                                # the float64 sum the comparison uses
    matches, misses, _ = check([0, 1], [0, 0], [t0, edge], [1.0, 1.0], window)
    assert matches == [[0, 1]] and misses == []
    matches, misses, _ = check([0, 1], [0, 0], [t0, np.nextafter(edge, np.inf)], [1.0, 1.0], window)
    assert matches == [] and misses == [0, 1]
    for t0, window in ((0.1, 0.2), (1.0, 1e-9), (3.0, 0.25)):
        edge = t0 + window
        check([0, 1, 2], [0, 0, 0], [t0, edge, np.nextafter(edge, np.inf)], [1.0] * 3, window)


def test_window_zero_groups_equal_timestamps():
    ts = np.repeat([0.0, 1.0, 1.5, 7.0], [5, 1, W, 3])
    n = len(ts)
    rng = np.random.default_rng(3)
    check(rng.integers(0, 3, n), rng.integers(0, 2, n), ts, rng.integers(1, 4, n).astype(float), 0.0)
    check(rng.integers(0, 3, n), rng.integers(0, 2, n), ts, rng.integers(1, 4, n).astype(float), -1.0)


def test_energy_rule():
    one = [0, 0, 0, 0]
    matches, _, collisions = check(one, one, [0.0] * 4, [2.0] * 4, 0.0, 1)        # ties: the later one
    assert matches == [[3]] and collisions == [(0, 1), (1, 2), (2, 3)]
    matches, _, collisions = check(one[:3], one[:3], [0.0] * 3, [3.0, 2.0, 1.0], 0.0, 1)    # larger earlier stays
    assert matches == [[0]] and collisions == [(0, 1), (0, 2)]
    matches, _, collisions = check(one, one, [0.0] * 4, [1.0, 3.0, 3.0, 2.0], 0.0, 1)
    assert matches == [[2]] and collisions == [(0, 1), (1, 2), (2, 3)]
    matches, _, collisions = check(one[:3], one[:3], [0.0] * 3, [5.0, NAN, 3.0], 0.0, 1)    # NaN takes over, then loses
    assert matches == [[2]] and collisions == [(0, 1), (1, 2)]
    for en in ([NAN, 5.0, 3.0], [5.0, 3.0, NAN], [NAN, NAN, NAN], [5.0, NAN, NAN, 7.0], [9.0, NAN, 3.0, 1.0],
               [-np.inf, -np.inf, NAN, -np.inf], [0.0, -0.0, 0.0], [np.inf, np.inf]):
        k = len(en)
        check([0] * k, [0] * k, [0.0] * k, en, 0.0, 1)
    rng = np.random.default_rng(17)                 # NaNs sprinkled over runs that cross workgroups
    n = 3 * W
    en = rng.integers(1, 4, n).astype(float)
    en[rng.random(n) < 0.1] = NAN
    check(rng.integers(0, 2, n), np.zeros(n, int), np.zeros(n), en, 0.0)


@pytest.mark.parametrize("min_match", [0, 1, 2, 4, 5])
def test_min_match(min_match):
    rx, tx, ts, en = grid_set(2 * W + 1, 23)          # four receivers: 5 is one more than there are
    matches, misses, _ = check(rx, tx, ts, en, 0.5, min_match)
    if min_match <= 1:
        assert misses == []
    if min_match == 5:
        assert matches == []


def test_negative_ids():
    rx, tx, ts, en = grid_set(2 * W + 1, 29, n_rx=5, tx_lo=-2, tx_hi=2, rx_lo=-3)
    check(rx, tx, ts, en, 0.5)
    check(np.full(5, -2**31), np.full(5, -2**31), np.zeros(5), np.ones(5), 0.0, 1)
    check([2**31 - 1, -2**31, 0, -1, 2**31 - 1], [-1] * 5, np.zeros(5), np.ones(5), 0.0)


def test_seventy_receivers_in_one_group_keep_first_appearance_order():
    rng = np.random.default_rng(31)
    first = rng.permutation(70) - 20
    rx = np.concatenate([first, rng.permutation(70) - 20])
    en = rng.integers(1, 4, 140).astype(float)
    matches, _, collisions = check(rx, np.zeros(140, int), np.zeros(140), en, 0.0)
    assert len(matches) == 1 and len(collisions) == 70
    assert [int(rx[i]) for i in matches[0]] == first.tolist()


def test_one_group_per_txid_and_one_group_per_detection():
    rx, tx, ts, en = grid_set(2 * W + 1, 37)
    matches, misses, _ = check(rx, tx, ts, en, 1e9)
    assert len(matches) + len(misses) == len(set(tx.tolist()))
    ts = np.arange(len(ts), dtype=float)
    matches, misses, collisions = check(rx, tx, ts, en, 0.0)
    assert matches == [] and misses == list(range(len(ts))) and collisions == []
