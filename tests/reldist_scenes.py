"""The inputs of the reldist tests: the recorded scenes of tests/golden/reldist (made by
tests/golden/make_golden_reldist.py from the reference's script) and the seam scenes, which are built here.
`every_input()` lists all of them -- it is what `python tests/reldist_ref.py` measures the smoother's tolerance on."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reldist")
NAMES = ("a", "b", "c", "d", "e", "f")
COLUMNS = ("rxid", "txid", "soa", "timestamp", "carrier_bin", "carrier_offset", "idx")
RATE = 2.4e6
# the script's three constants, metres: distance(b, rx1) - distance(b, rx0), distance(rx1, rx0), distance(b, rx1)
SCRIPT_METRES = (-917.888911019, 8964.1335967, 4024.48549105)


def assemble(transmissions):
    """Detection columns and CSR matches from [(txid, {rxid: (soa, timestamp, carrier_bin, carrier_offset)})],
    one match per transmission, detections in the order of the dict."""
    cols = {name: [] for name in COLUMNS}
    ptr, idx = [0], []
    for tx, dets in transmissions:
        for rx, (soa, ts, cbin, coff) in dets.items():
            idx.append(len(cols["soa"]))
            for name, value in zip(COLUMNS, (rx, tx, soa, ts, cbin, coff, len(cols["soa"]))):
                cols[name].append(value)
        ptr.append(len(idx))
    kinds = {"rxid": np.int32, "txid": np.int32, "idx": np.int64}
    cols = {name: np.array(v, kinds.get(name, np.float64)) for name, v in cols.items()}
    return cols, np.array(ptr, np.int64), np.array(idx, np.int64)


def synth(schedule, rx_pos, seed, beacon_pos=None, noise=0.05, drop=0.0):
    """A line of receivers (rx_pos: {rxid: metres}), beacons at beacon_pos ({txid: metres}), every other transmitter
    walking between the first two receivers.  schedule: [(txid, seconds)].  Receiver clocks differ by tens of ppm
    and an offset; `drop` is the share of detections that are missing (never leaving a transmission with one)."""
    rng = np.random.default_rng(seed)
    beacon_pos = beacon_pos or {}
    ppm = {rx: 1.0 + 1e-6 * rng.uniform(-30, 30) for rx in rx_pos}
    off = {rx: float(rng.integers(0, 5000)) for rx in rx_pos}
    lo, hi = sorted(rx_pos.values())[:2]
    out = []
    for tx, t in schedule:
        pos = beacon_pos.get(tx)
        if pos is None:
            pos = lo + (hi - lo) * (0.45 + 0.3 * np.sin(t / 40.0 + tx))
            vel = (hi - lo) * 0.3 / 40.0 * np.cos(t / 40.0 + tx)
        else:
            vel = 0.0
        dets = {}
        for rx, p in rx_pos.items():
            if len(rx_pos) > 2 and rng.uniform() < drop:
                continue
            delay = abs(pos - p) / 3e8
            doppler = -vel * np.sign(pos - p) / 3e8 * 433e6 / (RATE / 16384)       # bins
            carrier = 300.0 + 7.0 * tx + doppler + rng.normal(0, 0.002)
            dets[rx] = ((t + delay) * RATE * ppm[rx] + off[rx] + rng.normal(0, noise), 1000.0 + t + delay,
                        float(np.floor(carrier)), carrier - np.floor(carrier))
        if len(dets) >= 2:
            out.append((tx, dets))
    return out


def interleaved(n, beacon_every=4, mobiles=(1,), beacons=(0,), step=0.25, first_beacon=True):
    """n transmissions `step` seconds apart: every beacon_every-th slot is a beacon's, the others the mobiles'."""
    schedule, k = [], 0
    for i in range(n):
        if i % beacon_every == 0:
            schedule.append((beacons[(i // beacon_every) % len(beacons)], i * step))
        else:
            schedule.append((mobiles[k % len(mobiles)], i * step))
            k += 1
    return schedule if first_beacon else schedule[1:]


def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as f:
        return {k: f[k] for k in f.files}


def golden_input(g, method="linpol", **more):
    kwargs = dict(beacons=g["beacons"].tolist(), method=method, geometry=g["geometry"].tolist())
    kwargs.update(more)
    return ({name: g[name] for name in COLUMNS}, g["match_ptr"], g["match_idx"]), kwargs


def check_against_fixture(out, g, method, what):
    """Every row of every cell: the script's nearest index, its raw (where it defines one) and its three masks."""
    seen = 0
    for ci, key in enumerate(out["cell_key"].tolist()):
        tag = "m%d_b%d_%d_%d_" % tuple(key)
        a, b = out["cell_ptr"][ci:ci + 2]
        sa, sb = out["speed_ptr"][ci:ci + 2]
        assert np.array_equal(out["nearest_idx"][a:b], g[tag + "nearest"]), (what, tag)
        if method == "nearest" or tag + "raw_linpol" in g:
            assert out["raw"][a:b].tobytes() == g[tag + "raw_" + method].tobytes(), (what, tag)
            seen += 1
        assert np.array_equal(out["mask1"][a:b] != 0, g[tag + "mask1_" + method]), (what, tag)
        assert np.array_equal(out["mask2"][sa:sb] != 0, g[tag + "mask2_" + method]), (what, tag)
        assert np.array_equal(out["mask3"][a:b] != 0, g[tag + "mask3"]), (what, tag)
    assert sum(k.endswith("_nearest") and "raw" not in k and "mask" not in k for k in g) == len(out["cell_key"]), what
    return seen


def sized_cells(counts, seed=5, beacon_rows=40, **how):
    """One beacon (txid 0), mobiles 1.. with exactly counts[i - 1] rows each, two receivers."""
    span = float(max(counts) + 2)
    schedule = [(0, t) for t in np.linspace(0.0, span, beacon_rows)]
    for i, n in enumerate(counts):
        schedule += [(i + 1, 0.37 + 0.013 * i + t) for t in (np.arange(n) * (span - 1.0) / max(n, 1))]
    schedule.sort(key=lambda s: s[1])
    return assemble(synth(schedule, {0: 0.0, 1: 9000.0}, seed, {0: 4000.0}, **how))


def seam_inputs(tile):
    """name -> (args, kwargs) of the seam scenes; `tile` is the reductions' tile length."""
    T = tile
    out = {}
    sizes = [T - 1, T + 1, 1, 2, 3, T, 2 * T + 1]      # cell 1 starts at position T - 1; cells 2-4 share a tile
    for method in ("nearest", "linpol"):
        out["sizes_" + method] = (sized_cells(sizes), dict(beacons=[0], method=method))
    out["thresh_half"] = (sized_cells([2, 3, 9]), dict(beacons=[0], thresh=0.5))        # two rows: both masked, no speed
    for nb in (1, 2):
        out["nb_%d" % nb] = (sized_cells([5, 1, 12], beacon_rows=nb), dict(beacons=[0]))
    # every mobile row before the first beacon row (mobile 1), after the last (mobile 2), both in one call
    txs = synth([(1, t) for t in np.arange(6) * 0.5] + [(0, 10.0 + t) for t in np.arange(5)] +
                [(2, 20.0 + t) for t in np.arange(7) * 0.5], {0: 0.0, 1: 9000.0}, 8, {0: 4000.0})
    for method in ("nearest", "linpol"):
        out["outside_" + method] = (assemble(txs), dict(beacons=[0], method=method))
    # x = 0, 0, 0, 0, big: MAD = 0, the big one is masked (inf), the others are kept (NaN); integer SOAs
    flat = [(0, {0: (1000.0 * i, 1000.0 + i, 300.0, 0.25), 1: (1000.0 * i + 50.0, 1000.0 + i, 300.0, 0.5)}) for i in range(8)]
    flat += [(1, {0: (1000.0 * i + 500.0, 1000.5 + i, 310.0, 0.0), 1: (1000.0 * i + 560.0 + (64.0 if i == 4 else 0.0), 1000.5 + i, 310.0, 0.25)})
             for i in range(5)]
    out["mad_zero"] = (assemble(flat), dict(beacons=[0], method="nearest"))
    # orders: beacon 0's soa at rx0 steps back once (mobile cells of beacon 0 unsorted, of beacon 5 not);
    # mobile 2's timestamps step back once (unsorted only while smoothing)
    txs = synth(interleaved(120, 3, mobiles=(1, 2), beacons=(0, 5)), {0: 0.0, 1: 9000.0}, 9, {0: 4000.0, 5: 6000.0})
    b0 = [i for i, (tx, _) in enumerate(txs) if tx == 0]
    txs[b0[3]], txs[b0[4]] = txs[b0[4]], txs[b0[3]]
    m2 = [i for i, (tx, _) in enumerate(txs) if tx == 2]
    txs[m2[5]][1][0] = txs[m2[5]][1][0][:1] + (txs[m2[5]][1][0][1] - 3.0,) + txs[m2[5]][1][0][2:]
    for frac in (0.0, 0.25):
        out["unsorted_frac_%g" % frac] = (assemble(txs), dict(beacons=[0, 5], smooth_frac=frac))
    # a NaN soa in one row of mobile 1; mobile 2 is untouched
    txs = synth(interleaved(90, 3, mobiles=(1, 2)), {0: 0.0, 1: 9000.0}, 10, {0: 4000.0})
    m1 = [i for i, (tx, _) in enumerate(txs) if tx == 1]
    txs[m1[7]][1][1] = (np.nan,) + txs[m1[7]][1][1][1:]
    out["nan_row"] = (assemble(txs), dict(beacons=[0]))
    # the smoother: series of m points (dopplers; m - 1 speeds) under three fractions -- k = m at frac 1 (1, 2, 3, 4,
    # 63 .. 66 around a wave), k = 63, 64, 65 inside longer series at frac 0.5 (windows pinned at both ends and moving
    # between), k = 2 at the default fraction
    lengths = [1, 2, 3, 4, 63, 64, 65, 66, 126, 127, 128, 129, 130, 131]
    for frac in (1.0, 0.5, 0.025):
        out["smooth_frac_%g" % frac] = (sized_cells(lengths, seed=12), dict(beacons=[0], smooth_frac=frac))
    # integer timestamps one second apart: every even window has a tie; then all timestamps equal: h = 0
    for name, stamp in (("ties", lambda i: float(i)), ("equal_abscissae", lambda i: 7.0)):
        txs = []
        rng = np.random.default_rng(13)
        for i in range(40):
            txs.append((0, {0: (2.4e6 * i, 1000.0 + stamp(i), 300.0, 0.25), 1: (2.4e6 * i + 77.0, 1000.0 + stamp(i), 300.0, 0.5)}))
            for tx in (1, 2)[:1 if i % 2 else 2]:
                txs.append((tx, {0: (2.4e6 * i + 1.1e6 + tx, 1000.0 + stamp(i), 310.0, float(rng.integers(0, 64)) / 64),
                                 1: (2.4e6 * i + 1.1e6 + tx + float(rng.integers(90, 140)), 1000.0 + stamp(i), 310.0,
                                     float(rng.integers(0, 64)) / 64)}))
        for frac in (0.2, 0.25):
            out["%s_frac_%g" % (name, frac)] = (assemble(txs), dict(beacons=[0], smooth_frac=frac))
    return out


def every_input():
    """name -> (args, kwargs): every call the two GPU test files make."""
    from thrifty_amd import _native
    out = {}
    for name in NAMES:
        g = load(name)
        for method in ("nearest", "linpol"):
            out["golden_%s_%s" % (name, method)] = golden_input(g, method)
    out.update(seam_inputs(_native.reldist_geometry()[0]))
    return out
