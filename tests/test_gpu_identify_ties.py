"""`identify` on the device (csrc/identify.hip) where TIES decide the answer.  test_gpu_identify.py
draws continuous timestamps and energies, so it never asks whether the four radix-sort passes and
the output order are stable, whether the duplicate rule compares with `<` or `<=`, whether the
map ranges are closed, which of two overlapping ranges wins, on which side of a window edge a bin
falls, or what the order-preserving keys do with negative numbers and with -0.0.  Every set below is
built so that one of those decides a detection's fate; all outputs are compared with the oracle
(`onp.auto_classify`, `onp.classify_by_map`, `onp.duplicate_mask`, `onp.filter_order`) as arrays,
with no tolerance.

  (a) without a GPU: each set holds the tie / edge / sign / wrap it claims, the oracle decides it the
      way the set's note says, and the oracle's two sorts are the STABLE ones (np.lexsort with the
      input position as the last key)
  (b) thr_identify against the oracle on every set

The zero-sign set found a discrepancy: key_f64 mapped -0.0 below +0.0, so a detection stamped -0.0
was sorted in front of one stamped 0.0 that preceded it in the input, while NumPy's sorts -- the
reference's rule -- compare them equal and keep the input order.  key_f64 now takes the key of
+0.0 for a zero of either sign.

Seeded mutations on scratch builds: `<=` for `<` in k_dup_mask's first comparison fails 13 sets here
and none of test_gpu_identify.py; `freq < map[m].hi` fails map_edges and n_70001 (and
test_python_api_and_cli of test_gpu_identify.py, on the identify_map fixture); swapping the block and txid sort
passes fails 10 sets here and 5 tests there."""
import numpy as np
import pytest

from oracle import thrifty_np as onp
from thrifty_amd import _native as F

INF = np.inf


def rows_of(fm):
    return [(rx, tx, lo, hi) for rx, m in fm.items() for tx, (lo, hi) in m.items()]


def cols(rxid, block, ts, cbin, coff, energy, fm=None, **notes):
    n = len(rxid)
    c = dict(rxid=np.asarray(rxid, dtype=np.int32), block=np.asarray(block, dtype=np.int32),
             ts=np.asarray(ts, dtype=np.float64), cbin=np.asarray(cbin, dtype=np.int32),
             coff=np.asarray(coff, dtype=np.float64), energy=np.asarray(energy, dtype=np.float64), fm=fm)
    assert all(len(c[k]) == n for k in ("block", "ts", "cbin", "coff", "energy"))
    c.update(notes)
    return c


def oracle(c):
    """-> (txid, keep mask, kept order) by the pinned NumPy restatement of the reference."""
    if c["fm"] is None:
        tx, _ = onp.auto_classify(c["rxid"], c["cbin"])
    else:
        tx = onp.classify_by_map(c["rxid"], c["cbin"], c["coff"], c["fm"])
    keep = onp.duplicate_mask(c["rxid"], tx, c["block"], c["ts"], c["energy"])
    return tx, keep, onp.filter_order(keep, c["ts"])


def freq_of(cbin, coff):
    """bin + offset the way k_classify_map forms it: double(bin) + offset in float64."""
    return np.asarray(cbin, dtype=np.int32).astype(np.float64) + np.asarray(coff, dtype=np.float64)


def offset_for(cbin, target):
    """The carrier offset that puts float(bin) + offset EXACTLY on `target`."""
    off = np.float64(target) - np.float64(cbin)
    assert np.float64(cbin) + off == np.float64(target)
    return off


# three transmitters' bins per receiver for the automatic mode: narrow, well separated clusters
def clustered_bins(rng, n, rxid, centres=(30, 61, 93)):
    tx = rng.integers(0, len(centres), n)
    return (np.asarray(centres)[tx] + rxid + np.round(rng.normal(0, 0.7, n))).astype(np.int32)


# ---------------------------------------------------------------------------------------------
# the sets
# ---------------------------------------------------------------------------------------------
def heavy_ties(n, n_stamps, seed, n_blocks=40, n_energies=3):
    """A few distinct timestamps (or one) over thousands of detections, a few distinct energies, a
    small block range: most detections tie with others in (rx, tx, block, timestamp), so the
    duplicate sort and the output order fall back on the input position all the time."""
    rng = np.random.default_rng(seed)
    rxid = rng.integers(0, 3, n).astype(np.int32)
    stamps = 1.7e9 + np.arange(n_stamps) * 0.125
    return cols(rxid, rng.integers(0, n_blocks, n), stamps[rng.integers(0, n_stamps, n)],
                clustered_bins(rng, n, rxid), rng.uniform(-0.5, 0.5, n),
                np.asarray([80.0, 120.0, 160.0, 200.0])[rng.integers(0, n_energies, n)], None,
                n_stamps=n_stamps)


def equal_energies():
    """Pairs in adjacent blocks of one (rx, tx), blocks far from every other pair's: equal energies
    (both survive: the rule is `<`), then one energy moved by one ulp each way (the smaller one goes)."""
    e = 123.456
    up, down = np.nextafter(e, INF), np.nextafter(e, -INF)
    pairs = [(e, e), (e, up), (e, down), (up, e), (down, e), (up, up), (down, up)]
    rxid, block, ts, energy, want = [], [], [], [], []
    for rx in (0, 1):
        for g, (a, b) in enumerate(pairs):
            rxid += [rx, rx]
            block += [100 * g + 10, 100 * g + 11]
            ts += [1000.0 + g, 1000.0 + g + 0.005]
            energy += [a, b]
            want += [not a < b, not b < a]
    n = len(rxid)
    fm = {0: {0: (0.0, 100.0)}, 1: {0: (0.0, 100.0)}}
    return cols(rxid, block, ts, np.full(n, 50), np.zeros(n), energy, fm, want_keep=np.asarray(want))


MAP_LO, MAP_HI = 30.25, 33.75


def map_edges():
    """bin + offset exactly on `lo` and on `hi` of a range (inclusive), one ulp outside each; the same
    with the range's ends moved by one ulp instead; two overlapping ranges (the later row wins, in
    either order of their txids); a receiver the map does not know (-1, dropped)."""
    below, above = np.nextafter(MAP_LO, -INF), np.nextafter(MAP_HI, INF)
    fm = {0: {3: (MAP_LO, MAP_HI)},
          1: {5: (40.0, 50.0), 6: (45.0, 55.0)},                 # 45 .. 50 matches both: 6 is later
          2: {6: (45.0, 55.0), 5: (40.0, 50.0)},                 # ... here 5 is later
          4: {7: (np.nextafter(MAP_LO, INF), np.nextafter(MAP_HI, -INF))},     # the ends moved inwards
          5: {}}                                                 # a receiver without rows
    det = [  # (rx, bin, target frequency, expected txid)
        (0, 30, MAP_LO, 3), (0, 31, MAP_LO, 3), (0, 30, below, -1), (0, 33, MAP_HI, 3), (0, 34, MAP_HI, 3),
        (0, 33, above, -1), (0, 34, above, -1), (0, 32, 32.0, 3),
        (1, 42, 42.0, 5), (1, 45, 45.0, 6), (1, 47, 47.3, 6), (1, 50, 50.0, 6), (1, 52, 52.0, 6),
        (1, 40, 40.0, 5), (1, 55, 55.0, 6), (1, 56, 55.5, -1),
        (2, 42, 42.0, 5), (2, 45, 45.0, 5), (2, 47, 47.3, 5), (2, 50, 50.0, 5), (2, 52, 52.0, 6),
        (4, 30, MAP_LO, -1), (4, 30, np.nextafter(MAP_LO, INF), 7), (4, 34, MAP_HI, -1),
        (4, 33, np.nextafter(MAP_HI, -INF), 7),
        (5, 32, 32.0, -1), (5, 47, 47.0, -1),
    ]
    n = len(det)
    return cols([d[0] for d in det], np.arange(n) * 10, 50.0 + np.arange(n), [d[1] for d in det],
                [offset_for(d[1], d[2]) for d in det], np.full(n, 100.0), fm,
                want_tx=np.asarray([d[3] for d in det]), target=np.asarray([d[2] for d in det]))


def auto_edges():
    """Automatic windows.  Receiver 0: two clusters and one detection whose bin IS the edge computed
    between them (np.digitize: edges[e] <= x, so it belongs to the upper window), one a bin below
    it.  Receiver 1: a single bin (one window, [bin, bin + 1)).  Receivers 2 and 3: disjoint bin
    ranges, far apart -- the device histograms all receivers over the union of their ranges."""
    rng = np.random.default_rng(8)
    rx0 = np.concatenate([np.full(300, 20), np.full(200, 21), np.full(250, 41), np.full(250, 42)])
    _, e0 = onp.auto_classify(np.zeros(len(rx0), int), rx0)
    edge = int(e0[0][1])                                # the mid-point between the two clusters
    rx0 = np.concatenate([rx0, [edge, edge - 1, edge + 1]])
    rx1 = np.full(64, 77)
    rx2 = np.repeat([10, 11, 14, 15], [90, 60, 70, 80])
    rx3 = np.repeat([500, 501, 519, 520], [40, 50, 60, 70])
    cbin = np.concatenate([rx0, rx1, rx2, rx3])
    rxid = np.repeat([0, 1, 2, 3], [len(rx0), len(rx1), len(rx2), len(rx3)])
    n = len(cbin)
    perm = rng.permutation(n)
    return cols(rxid[perm], rng.integers(0, 400, n), 10.0 + rng.integers(0, 50, n) * 0.5, cbin[perm],
                rng.uniform(-0.5, 0.5, n), rng.integers(1, 4, n) * 50.0, None, edge=edge)


def signs(auto, seed=5):
    """Negative carrier bins, block indices and timestamps mixed with positive ones (key_i32 /
    key_f64 must order them as integers / reals), with blocks -1 and 0 -- adjacent across the
    sign change -- in every (rx, tx)."""
    rng = np.random.default_rng(seed)
    n = 4000
    rxid = rng.integers(0, 2, n).astype(np.int32)
    cbin = clustered_bins(rng, n, rxid, centres=(-60, -3, 45))
    block = rng.integers(-40, 40, n)
    ts = np.round(rng.uniform(-3.0, 3.0, n), 1) + 0.0     # 61 values around zero, both signs (no -0.0: zero_signs)
    energy = rng.integers(1, 5, n) * 25.0
    fm = None
    if not auto:
        fm = {int(r): {t: (c + r - 2.5, c + r + 2.5) for t, c in enumerate((-60, -3, 45))} for r in range(2)}
    return cols(rxid, block, ts, cbin, rng.uniform(-0.5, 0.5, n), energy, fm)


def wrap(first_is_larger, other_receiver, n_fill):
    """np.roll wraps: the FIRST element of the sorted order has the LAST as its predecessor (and the
    last has the first as its successor).  Here the first sits in block 11 and the last in block 10,
    so the rule compares them although nothing physical relates them -- it looks at neither rxid nor
    txid; the one with less energy is dropped.  Fillers in between are far from both."""
    fm = {0: {0: (0.0, 10.0), 1: (20.0, 30.0)}, 1: {0: (0.0, 10.0), 1: (20.0, 30.0)}}
    e_first, e_last = (200.0, 100.0) if first_is_larger else (100.0, 200.0)
    # sorted by (rx, tx, block, ts): (0, 0, 11) is the smallest key; the largest is (0, 1, 10) or (1, 1, 10)
    last_rx = 1 if other_receiver else 0
    rxid = [last_rx] + [0] * n_fill + [0]              # input order: last, fillers, first
    tx_bin = [25] + [5] * n_fill + [5]
    block = [10] + [1000 + 7 * k for k in range(n_fill)] + [11]
    energy = [e_last] + [150.0] * n_fill + [e_first]
    n = len(rxid)
    return cols(rxid, block, 5.0 + np.arange(n), tx_bin, np.zeros(n), energy, fm,
                first=n - 1, last=0, dropped=0 if first_is_larger else n - 1)


def sized(n, auto):
    """Generic sets at the thread-block seams (256 threads per workgroup in every identify kernel):
    quantised timestamps and energies, many adjacent blocks."""
    rng = np.random.default_rng(7000 + n)
    rxid = rng.integers(0, 4, n).astype(np.int32)
    cbin = clustered_bins(rng, n, rxid)
    block = rng.integers(0, max(2, n // 3), n)
    ts = 1.7e9 + block * 0.5 + rng.integers(0, 2, n) * 0.25
    fm = None
    if not auto:
        fm = {int(r): {t: (c + r - 2.5, c + r + 2.5) for t, c in enumerate((30, 61, 93))} for r in range(4)}
    return cols(rxid, block, ts, cbin, rng.integers(-2, 3, n) * 0.25, rng.integers(1, 4, n) * 60.0, fm)


def zero_signs():
    """Timestamps 0.0 and -0.0 in one set: equal to every NumPy sort, which therefore keeps their
    input order -- in the duplicate sort (same rx, tx, block) and in the output order."""
    rng = np.random.default_rng(2)
    n = 600
    ts = np.where(rng.random(n) < 0.5, 0.0, -0.0)
    ts[:4] = [0.0, -0.0, 0.0, -0.0]                       # +0 in front of -0 at the very start
    ts[rng.random(n) < 0.1] = 1.0
    ts[rng.random(n) < 0.1] = -1.0
    fm = {0: {0: (0.0, 100.0)}}
    return cols(np.zeros(n, int), rng.integers(0, 30, n), ts, np.full(n, 50), np.zeros(n),
                rng.integers(1, 4, n) * 60.0, fm)


SETS = {
    "ties_4_stamps": lambda: heavy_ties(6000, 4, 1),
    "ties_all_equal": lambda: heavy_ties(5000, 1, 2),
    "ties_all_equal_one_energy": lambda: heavy_ties(3000, 1, 3, n_blocks=12, n_energies=1),
    "equal_energies": equal_energies,
    "map_edges": map_edges,
    "auto_edges": auto_edges,
    "signs_auto": lambda: signs(True),
    "signs_map": lambda: signs(False),
    "wrap_first_larger": lambda: wrap(True, False, 5),
    "wrap_last_larger": lambda: wrap(False, False, 5),
    "wrap_other_receiver_first_larger": lambda: wrap(True, True, 5),
    "wrap_other_receiver_last_larger": lambda: wrap(False, True, 5),
    "wrap_two_elements": lambda: wrap(False, False, 0),
    "n_1_auto": lambda: sized(1, True),
    "n_1_map": lambda: sized(1, False),
    "n_2": lambda: sized(2, False),
    "n_255": lambda: sized(255, True),
    "n_256": lambda: sized(256, False),
    "n_257": lambda: sized(257, True),
    "n_70001": lambda: sized(70001, False),
    "n_70001_ties": lambda: heavy_ties(70001, 3, 4, n_blocks=500),
    "zero_signs": zero_signs,
}


# ---------------------------------------------------------------------------------------------
# (a) without a GPU
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_the_oracle_sorts_are_the_stable_ones(name):
    """np.lexsort is stable, np.argsort(kind="stable") is: both equal a lexsort whose last key is the
    input position -- the rule the device's LSD radix passes (timestamp, block, txid, rxid, each
    stable, starting from the identity) must reproduce."""
    c = SETS[name]()
    tx, keep, order = oracle(c)
    n = len(tx)
    pos = np.arange(n)
    full = np.lexsort((pos, c["ts"], c["block"], tx, c["rxid"]))
    assert np.array_equal(full, np.lexsort((c["ts"], c["block"], tx, c["rxid"])))
    blk, en, txs = c["block"][full], c["energy"][full], tx[full]
    drop = (((blk == np.roll(blk, 1) + 1) & (en < np.roll(en, 1)))
            | ((blk == np.roll(blk, -1) - 1) & (en < np.roll(en, -1))) | (txs == -1))
    mask = np.empty(n, dtype=bool)
    mask[full] = ~drop
    assert np.array_equal(mask, keep)
    by_ts = np.lexsort((pos, c["ts"]))
    assert np.array_equal(by_ts[keep[by_ts]], order)


def test_the_tie_sets_tie():
    for name, stamps in (("ties_4_stamps", 4), ("ties_all_equal", 1), ("ties_all_equal_one_energy", 1),
                         ("n_70001_ties", 3)):
        c = SETS[name]()
        tx, keep, order = oracle(c)
        assert len(np.unique(c["ts"])) == stamps and len(c["ts"]) >= 3000
        # whole sort keys that occur more than once: the input position decides among them
        keys = np.stack([c["rxid"], tx, c["block"]]).T
        _, counts = np.unique(np.column_stack([keys, c["ts"]]), axis=0, return_counts=True)
        assert (counts > 1).sum() > 100, name
        # stable output order: equal timestamps come out in input order, and the order is not the identity
        assert all(np.all(np.diff(order[c["ts"][order] == v]) > 0) for v in np.unique(c["ts"]))
        if len(np.unique(c["energy"])) == 1:             # no energy is smaller than another: nothing goes
            assert keep.all() and (tx != -1).all()
        else:
            assert 0.02 < keep.mean() < 0.98, (name, keep.mean())
        # equal energies in adjacent blocks of one (rx, tx) occur too
        srt = np.lexsort((c["ts"], c["block"], tx, c["rxid"]))
        adj = (np.diff(c["block"][srt]) == 1) & (np.diff(c["energy"][srt]) == 0)
        assert adj.sum() > 10, name


def test_equal_energies_survive_and_one_ulp_decides():
    c = equal_energies()
    tx, keep, _ = oracle(c)
    assert (tx == 0).all() and np.array_equal(keep, c["want_keep"])
    e = c["energy"]
    assert keep[0] and keep[1] and e[0] == e[1]                       # equal: both kept
    assert not keep[2] and keep[3] and e[3] == np.nextafter(e[2], INF)   # one ulp more on the right
    assert keep[4] and not keep[5] and e[5] == np.nextafter(e[4], -INF)  # one ulp less on the right
    assert c["want_keep"].sum() == 2 * (4 + 5)


def test_map_edges_are_exact():
    c = map_edges()
    f = freq_of(c["cbin"], c["coff"])
    assert np.array_equal(f, c["target"])                # the device forms exactly the intended frequency
    assert (f == MAP_LO).sum() >= 2 and (f == MAP_HI).sum() >= 2
    assert (f == np.nextafter(MAP_LO, -INF)).sum() == 1 and (f == np.nextafter(MAP_HI, INF)).sum() == 2
    tx, keep, _ = oracle(c)
    assert np.array_equal(tx, c["want_tx"])
    assert np.array_equal(keep, tx != -1)                # blocks are 10 apart: only the unidentified go
    rx = c["rxid"]
    both = (f >= 45.0) & (f <= 50.0)
    assert (tx[(rx == 1) & both] == 6).all() and (tx[(rx == 2) & both] == 5).all() and ((rx == 1) & both).sum() == 3
    assert (tx[rx == 5] == -1).all() and 5 not in [r[0] for r in rows_of(c["fm"])]


def test_auto_edges_sit_where_claimed():
    c = auto_edges()
    tx, edges = onp.auto_classify(c["rxid"], c["cbin"])
    e0 = edges[0]
    assert len(e0) == 3 and int(e0[1]) == c["edge"] and 21 < c["edge"] < 41      # still the edge with the extras in
    rx, b = c["rxid"], c["cbin"]
    on, under = (rx == 0) & (b == c["edge"]), (rx == 0) & (b == c["edge"] - 1)
    assert on.sum() == 1 and under.sum() == 1 and tx[on][0] == 1 and tx[under][0] == 0
    assert len(edges[1]) == 2 and list(edges[1]) == [77, 78] and (tx[rx == 1] == 0).all()
    assert b[rx == 2].max() < b[rx == 3].min() - 400
    for r in (2, 3):
        assert len(edges[r]) == 3 and set(tx[rx == r].tolist()) == {0, 1}


def test_sign_sets_cross_zero():
    for auto in (True, False):
        c = signs(auto)
        for k in ("cbin", "block", "ts"):
            assert (c[k] < 0).sum() > 400 and (c[k] > 0).sum() > 400, k
        assert not (np.signbit(c["ts"]) & (c["ts"] == 0)).any() and (c["ts"] == 0).any()
        tx, keep, order = oracle(c)
        assert set(tx.tolist()) >= {0, 1, 2} and (~keep).sum() > 200 and keep.sum() > 200
        srt = np.lexsort((c["ts"], c["block"], tx, c["rxid"]))
        blk = c["block"][srt]
        assert ((blk[:-1] == -1) & (blk[1:] == 0)).sum() >= 4         # -1 next to 0 in sorted order
        assert np.all(np.diff(c["ts"][order]) >= 0) and c["ts"][order][0] < 0 < c["ts"][order][-1]


@pytest.mark.parametrize("first_is_larger", [True, False])
@pytest.mark.parametrize("other_receiver", [True, False])
def test_the_wrap_pair_is_first_and_last(first_is_larger, other_receiver):
    for n_fill in (5, 0):
        c = wrap(first_is_larger, other_receiver, n_fill)
        tx, keep, _ = oracle(c)
        srt = np.lexsort((c["ts"], c["block"], tx, c["rxid"]))
        assert srt[0] == c["first"] and srt[-1] == c["last"]
        assert c["block"][srt[0]] == c["block"][srt[-1]] + 1
        assert (c["rxid"][srt[0]] != c["rxid"][srt[-1]]) == other_receiver and tx[srt[0]] != tx[srt[-1]]
        want = np.ones(len(tx), dtype=bool)
        want[c["dropped"]] = False                       # only the wrap drops anything
        assert np.array_equal(keep, want)


def test_sizes_and_zero_signs():
    sizes = sorted(len(SETS[k]()["rxid"]) for k in SETS if k.startswith("n_"))
    assert sizes[:6] == [1, 1, 2, 255, 256, 257] and sizes[-1] > 65536
    for k in ("n_1_auto", "n_1_map"):
        tx, keep, order = oracle(SETS[k]())
        assert keep.tolist() == [tx[0] != -1] and tx[0] != -1          # its own neighbour both ways: kept
    c = zero_signs()
    ts = c["ts"]
    neg = np.signbit(ts) & (ts == 0)
    pos = ~np.signbit(ts) & (ts == 0)
    assert neg.sum() > 100 and pos.sum() > 100 and (ts == 1.0).any() and (ts == -1.0).any()
    _, keep, order = oracle(c)
    zeros = order[ts[order] == 0]
    assert np.all(np.diff(zeros) > 0)                    # input order among the zeros of either sign
    z = np.signbit(ts[zeros])
    assert (~z[:-1] & z[1:]).sum() > 20                  # ... with +0.0 in front of -0.0 many times


# ---------------------------------------------------------------------------------------------
# (b) on a GPU
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SETS))
def test_identify_equals_the_oracle(name):
    c = SETS[name]()
    want_tx, want_keep, want_order = oracle(c)
    txid, keep, order = F.identify(c["rxid"], c["block"], c["ts"], c["cbin"], c["coff"], c["energy"],
                                   None if c["fm"] is None else rows_of(c["fm"]))
    assert np.array_equal(txid, want_tx)
    assert np.array_equal(keep, want_keep)
    assert np.array_equal(order, want_order)
    for extra in ("want_tx", "want_keep"):               # what the set's own note says
        if extra in c:
            assert np.array_equal({"want_tx": txid, "want_keep": keep}[extra], c[extra])
