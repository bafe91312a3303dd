"""A synthetic multi-receiver scene for the post-detect chain's tests, and the STAGED device path the
fused call is held to (identify.integrate_columns -> matchmaker.match_columns -> tdoa_est.tdoa_columns ->
pos_est.pos_columns on the same inputs).

The scene: receivers on a ring of 1 km, two beacons and three mobiles inside it, a transmission every
0.125 s in turn; every receiver's clock is a polynomial of degree 2 of true time plus 0.05 samples of
noise, and a detection's SoA includes the propagation delay, so the TDOAs and positions are sensible.
On top: duplicates in the neighbouring block (identify drops them), detections whose carrier bin is in no
range of the map (dropped), second detections by the same receiver a few blocks on (collisions),
transmissions one receiver saw (misses), mobile transmissions two receivers saw (underdetermined groups)
and mobile transmissions before the first beacon."""
import numpy as np

from thrifty_amd import identify, kitchen_sink, matchmaker, pos_est, tdoa_est

FS, C, NEW_LEN = 2.4e6, 2.997e8, 12288
RING = [(1000.0, 0.0), (0.0, 1000.0), (-1000.0, 0.0), (0.0, -1000.0)]
TX_POS = {0: (300.0, 400.0), 1: (-200.0, -350.0), 2: (120.0, -80.0), 3: (-420.0, 260.0), 4: (510.0, 330.0)}
RING_1D = [(0.0,), (1500.0,)]               # the 1-D set: two receivers on a line, everything between them
TX_POS_1D = {0: (400.0,), 1: (1100.0,), 2: (700.0,), 3: (200.0,), 4: (1300.0,)}
BEACONS = (0, 1)
TX_ORDER = (2, 3, 4, 0, 1)                 # the mobiles send first: transmissions before the first beacon
OFFSET = [3e9, 7e9, 1.1e10, 5e9]
PPM = [0.0, 0.2e-6, -0.12e-6, 0.07e-6]
SKEW = [0.0, 0.012, -0.02, 0.007]
BIN_OF_TX = {tx: 40 + 10 * tx for tx in TX_POS}
BIN_OF_RX = [0, 2, 4, 6]
COLUMNS = kitchen_sink.COLUMNS


def settings(rx_ids=(0, 1, 2, 3), automatic=False, beacons=BEACONS, rx_pos=None, extra_beacons=(), line=False):
    ring, tx_pos = (RING_1D, TX_POS_1D) if line else (RING, TX_POS)
    freqmap = None if automatic else {
        rx: {tx: (BIN_OF_TX[tx] + BIN_OF_RX[k] - 3.0, BIN_OF_TX[tx] + BIN_OF_RX[k] + 3.0) for tx in sorted(TX_POS)}
        for k, rx in enumerate(rx_ids)}
    if rx_pos is None:
        rx_pos = {rx: np.array(ring[k]) for k, rx in enumerate(rx_ids)}
    beacon_pos = {tx: np.array(tx_pos[tx]) for tx in beacons}
    beacon_pos.update({tx: np.array([50.0 * tx, -20.0][:len(ring[0])]) for tx in extra_beacons})
    return kitchen_sink.PostdetectSettings(tx_freqs=freqmap, match_window=0.2, tdoa_est_window=8.0, rx_pos=rx_pos,
                                           beacon_pos=beacon_pos, sample_rate=FS)


def columns(n_events, seed=5, rx_ids=(0, 1, 2, 3), tx_order=TX_ORDER, extras=True, seen=0.9, only=None, line=False):
    """Raw detection columns, transmission after transmission.  `only`: the receivers (positions in
    rx_ids) that see anything at all."""
    rng = np.random.default_rng(seed)
    ring, tx_pos = (RING_1D, TX_POS_1D) if line else (RING, TX_POS)
    rows = []

    def detect(k, tx, t, block_shift=0, stamp_shift=0.0, gain=1.0, stray=False):
        delay = float(np.sqrt(np.sum(np.subtract(ring[k], tx_pos[tx]) ** 2))) / C
        arrival = t + delay
        soa = OFFSET[k] + FS * (1 + PPM[k]) * arrival + 2e-3 * (k + 1) * arrival * arrival + float(rng.normal(0, 0.05))
        soa += block_shift * NEW_LEN
        rows.append((rx_ids[k], int(soa // NEW_LEN), round(1000.0 + t + SKEW[k] + float(rng.normal(0, 1e-3)) + stamp_shift, 6),
                     5 if stray else BIN_OF_TX[tx] + BIN_OF_RX[k] + int(rng.integers(-1, 2)), float(rng.uniform(-0.5, 0.5)),
                     soa, gain * float(rng.uniform(50, 200)), float(rng.uniform(1, 3))))

    for e in range(n_events):
        tx, t = tx_order[e % len(tx_order)], 10.0 + 0.125 * e
        who = [k for k in range(len(rx_ids)) if rng.random() < seen]
        if extras and e % 17 == 16:
            who = [0]                                  # one receiver: a miss
        if extras and e % 13 == 12 and tx not in BEACONS and not line:
            who = [0, 1]                               # a mobile two receivers saw: an underdetermined group
        if only is not None:
            who = [k for k in who if k in only]
        for k in who:
            detect(k, tx, t)
            if not extras:
                continue
            roll = rng.random()
            if roll < 0.10:
                rows[-1] = rows[-1][:6] + (rows[-1][6] + 300.0,) + rows[-1][7:]
                detect(k, tx, t, block_shift=1, stamp_shift=1e-4, gain=0.2)      # weaker, next block: a duplicate
            elif roll < 0.13:
                detect(k, tx, t, stray=True)                                      # a bin the map does not hold
            elif roll < 0.18:
                detect(k, tx, t, block_shift=3, stamp_shift=5e-3)                 # the same receiver again: a collision
    kinds = (np.int32, np.int32, np.float64, np.int32, np.float64, np.float64, np.float64, np.float64)
    return {name: np.array([row[c] for row in rows], dtype=kind) for c, (name, kind) in enumerate(zip(COLUMNS, kinds))}


def head(cols, n):
    return {name: col[:n].copy() for name, col in cols.items()}


def staged(cols, st, min_match=2, deg=2):
    """The four staged column calls -> a dict with postdetect_columns' keys (without `counts`)."""
    txid, keep, order = identify.integrate_columns(cols, st.tx_freqs)
    toads = {name: np.asarray(cols[name])[order] for name in ("rxid", "timestamp", "soa", "energy", "noise")}
    toads["txid"] = txid[order]
    ptr, idx, misses, collisions = matchmaker.match_columns(toads, st.match_window, min_match)
    rx_pos = {rx: np.asarray(p, dtype=float) for rx, p in st.rx_pos.items()}
    beacon_pos = {tx: np.asarray(p, dtype=float) for tx, p in st.beacon_pos.items()}
    td = tdoa_est.tdoa_columns(toads, ptr, idx, st.tdoa_est_window, beacon_pos, rx_pos, st.sample_rate, deg)
    rows = td["tdoas"]
    ps = pos_est.pos_columns(td["group_ptr"], rows["rx0"], rows["rx1"], rows["tdoa"], rows["snr"], rx_pos)
    out = {"txid": txid, "keep": keep, "kept_order": order, "match_ptr": ptr, "match_idx": idx, "misses": misses,
           "collisions": collisions}
    out.update(td)
    out.update(ps)
    return out


FLOATS = ("timestamp", "pos", "dop", "snr")
EXACT = ("txid", "keep", "kept_order", "match_ptr", "match_idx", "misses", "collisions", "group_id", "group_ptr", "tx",
         "failures", "n_window", "n_kept", "status", "iters")


def assert_identical(got, want):
    """Every output bit for bit (floats by their bytes, so that a NaN equals itself)."""
    for name in EXACT:
        assert np.asarray(got[name]).shape == np.asarray(want[name]).shape, name
        assert np.array_equal(got[name], want[name]), name
    for name in FLOATS:
        a, b = np.ascontiguousarray(got[name], dtype=np.float64), np.ascontiguousarray(want[name], dtype=np.float64)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), name
    assert got["tdoas"].dtype == want["tdoas"].dtype and got["tdoas"].shape == want["tdoas"].shape
    assert got["tdoas"].tobytes() == want["tdoas"].tobytes(), "tdoas"
