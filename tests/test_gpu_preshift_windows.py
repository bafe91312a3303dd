"""The fused PreshiftDetector / fastdet kernel (k_preshift, detect16k_preshift.hip) and its
multi-pass twin (g_carrier_stats -> k_fit_preshift -> g_mult_preshift) at the rolls and edges
where their own index arithmetic can go wrong.  k_preshift does not share the default path's
carrier or peak search: it has its own windowed first-max (with the reference's `peak_idx > N`
quirk), finds the owners of bins peak -+ 1 by digit arithmetic, applies the roll as a gather from a
bank stored in a permuted layout (s_mod split into digits s1 = s & 15, s2 = (s >> 4) & 31,
s3 = s >> 9 with carries), picks the bank by rint((frac + 0.5) (num - 1)), and extracts the
correlation peak's neighbours across 1024-lag rows.  The rows below plant carriers so that every
digit of s_mod (preshift and fastdet) and every owner digit of peak -+ 1 occurs, put bursts on
the correlation window's edges and on both sides of every 1024-lag seam, reach each of the 16
k_preshift instantiations (u8 / complex64 x carrier stddev x correlation stddev x parabolic-only),
and run the multi-pass pipeline at the other block lengths.  The parabolic, no-stddev carrier
window edges of k_preshift are in test_gpu_carrier_windows.py and are not repeated here.

  (a) without a GPU: the digit arithmetic restated, the table covers every digit and carry, each
      planted carrier peaks at the claimed bin, each stddev row's verdict flip is real
  (b) the engine reports the kernel the row names
  (c) records against OraclePreshiftDetector / OracleFastdet, u8 and complex64 input, with the
      roll and bank word of `reserved` checked on every block
  (d) at 16384, the fused kernel and path="multipass" agree"""
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import soak_util  # noqa: E402
from oracle import thrifty_np as onp  # noqa: E402
from thrifty_amd import _native as F  # noqa: E402
from thrifty_amd import synth  # noqa: E402

N16 = 16384
FUSED, MULTI = "k_preshift", "g_* (multi-pass)"
THR, FD_THR = (0, 15, 0), (0.0, 200.0, 0.0)      # magnitude-domain / fastdet's power-domain
CAR_STD, COR_STD = (0, 15, 2000.0), (0, 15, 1000.0)
TONE, BURST = 0.012, 0.3
MAX_BATCH = 64


def template(name):
    if name == "g127":
        return synth.gold_template(7, 2, 1.0).astype(np.float64)
    if name == "g1023":
        return synth.gold_template(10, 2, 1.0).astype(np.float64)
    if name == "g4094":
        return synth.gold_template(11, 2, 2.0).astype(np.float64)
    if name == "g6141":
        return synth.gold_template(11, 2, 3.0).astype(np.float64)
    assert name == "r4914"                                  # the deployed geometry's length
    return np.sign(np.random.default_rng(1).normal(0, 1, 4914))


def corr_window(n, h, tpl_name):
    return onp.unique_window(n, h, len(template(tpl_name)))


def digits(s):
    return s & 15, (s >> 4) & 31, s >> 9


def roll_of(n, claim):
    """s_mod for a carrier record at `claim` (|carrier offset| < 0.5): (-claim) mod N, for the
    preshift rule rint(-(bin + offset)) and for fastdet's -argmax alike."""
    return (-claim) % n


# the s_mod sweep: s3 = 0 .. 31 with s2 a permutation of 0 .. 31 and s1 = 0 .. 15 twice, and three
# more so that every s2 value also meets s1 > 0 (a carry into it) and one roll has no carry at all
SWEEP = [(i % 16) + 16 * ((11 * i + 3) % 32) + 512 * i for i in range(32)]
SWEEP += [7 + 16 * 3 + 512 * 5, 1 + 16 * 19 + 512 * 9, 512 * 7]
NAMED_BINS = [0, 1, 15, 16, 17, 31, 32, 511, 512, 513, 1023, 1024, 8191, 8192, 8193, 15871, 15872,
              16368, 16382, 16383]
DELTAS = (0.12, -0.17, 0.21, -0.09, 0.15, -0.2, 0.07, -0.13)


def _rows():
    rows = []

    def add(rid, n, h, tpl, win, planted, kind="preshift", interp="parabolic", num=21, cthr=THR,
            xthr=THR, edge="", flips=()):
        """planted: [(carrier bin + delta, claimed record bin, burst lag or None for a random
        lag of the window, tone amplitude, burst amplitude)]"""
        rows.append(dict(id=rid, n=n, h=h, tpl=tpl, win=win, planted=planted, kind=kind, interp=interp,
                         num=num, cthr=cthr, xthr=xthr, edge=edge, flips=tuple(flips),
                         kernel=FUSED if n == N16 else MULTI))

    def at(bins, n=N16, small=(0, 1)):
        """carriers at `bins` + delta; bins next to bin 0 / N - 1 (and the u8 DC spike) get
        |delta| = 0.1"""
        out = []
        for i, b in enumerate(bins):
            d = DELTAS[i % len(DELTAS)]
            if b % n in small or b % n in (n - 1, n - 2):
                d = 0.1 if d > 0 else -0.1
            out.append((b + d, b % n, None, TONE, BURST))
        return out

    sweep_bins = [(N16 - s) % N16 for s in SWEEP]
    for interp in ("parabolic", "none", "gaussian", "cosine"):
        add("full_%s" % interp, N16, 4096, "g1023", (0, -1), at(NAMED_BINS + sweep_bins), interp=interp,
            edge="window (0, -1): every s1 / s2 / s3 digit of s_mod and every owner digit of "
                 "peak -+ 1; bin N - 1 raises IndexError unless the interpolator is none")
    for interp in ("none", "gaussian", "cosine"):
        planted = [(d, N16, None, TONE, BURST) for d in (0.1, -0.1, 0.06, -0.08)] + at([5, -7, 12, -12, 1, -1])
        add("sic_%s" % interp, N16, 4096, "g1023", (-12, 12), planted, interp=interp,
            edge="window (-12, 12), carrier at bin 0: the reference's bin N (none: a record at bin N "
                 "rolled by -N; others: IndexError)")
    add("fastdet_full", N16, 4096, "g1023", (0, 16383), at(NAMED_BINS + sweep_bins), kind="fastdet",
        cthr=FD_THR, xthr=FD_THR, edge="fastdet, the whole spectrum: every digit of (N - peak) & (N - 1)")
    add("fastdet_bin0", N16, 4096, "g1023", (0, 5), at([0, 0, 0, 0, 3]), kind="fastdet", cthr=FD_THR,
        xthr=FD_THR, edge="fastdet peak at bin 0: a wraps to X[N - 1]")
    add("fastdet_top", N16, 4096, "g1023", (-5, -1), at([-1, -1, -1, -1, -3]), kind="fastdet",
        cthr=FD_THR, xthr=FD_THR, edge="fastdet peak at bin N - 1: c wraps to X[0]")
    # bank index rule: carriers over a whole bin of sub-bin offsets
    for num in (1, 2, 3, 21, 101, 1001):
        planted = [(40 + d, 40, None, TONE, BURST) for d in np.linspace(-0.42, 0.42, 29)]
        add("bank_%d" % num, N16, 4096, "g1023", (7, 110), planted, num=num,
            edge="bank index rint((frac + 0.5) (num - 1)) and its clamp, num %d" % num)
    # correlation window edges and 1024-lag row seams
    for h, tname in ((4096, "g1023"), (1022, "g1023"), (3070, "g1023"), (3072, "g1023"), (4920, "r4914")):
        lo, hi = corr_window(N16, h, tname)
        lags = [lo, lo + 1, hi - 1, hi - 2]
        for m in range(1, N16 // 1024 + 1):
            lags += [v for v in (1024 * m - 1, 1024 * m, 1024 * m + 1) if lo <= v < hi]
        if lo < 1024:
            lags += [lo + 300, 700]
        lags = sorted(set(lags))
        planted = [(c, b, lag, TONE, BURST) for (c, b, _, _, _), lag in
                   zip(at([40 + (i * 7) % 60 for i in range(len(lags))]), lags)]
        add("corr_%d_%d" % (h, len(template(tname))), N16, h, tname, (7, 110), planted,
            edge="bursts at lo, lo + 1, hi - 1, hi - 2 of [%d, %d) and on both sides of every "
                 "1024-lag seam inside it" % (lo, hi))
    # stddev terms: a carrier ladder and a burst ladder, thresholds where dropping the term flips
    # a verdict; the bursts of the burst ladder alternate with the last kept lag
    lo, hi = corr_window(N16, 1022, "g1023")
    rng = np.random.default_rng(7)
    ladder = [(40 + DELTAS[i % 8], 40, int(rng.integers(lo, hi)), TONE * s, BURST * s)
              for i, s in enumerate(np.geomspace(0.3, 1.5, 12))]
    ladder += [(40 + DELTAS[i % 8], 40, hi - 1 if i % 2 else int(rng.integers(lo, hi)), 0.02, BURST * s)
               for i, s in enumerate(np.geomspace(0.02, 0.5, 12))]
    for name, interp, cthr, xthr in (("car_parabolic", "parabolic", CAR_STD, THR),
                                     ("cor_parabolic", "parabolic", THR, COR_STD),
                                     ("both_parabolic", "parabolic", CAR_STD, COR_STD),
                                     ("car_gaussian", "gaussian", CAR_STD, THR),
                                     ("cor_cosine", "cosine", THR, COR_STD),
                                     ("both_none", "none", CAR_STD, COR_STD)):
        flips = (["carrier"] if cthr[2] else []) + (["correlation"] if xthr[2] else [])
        add("std_%s" % name, N16, 1022, "g1023", (7, 110), ladder, interp=interp, cthr=cthr, xthr=xthr,
            flips=flips, edge="stddev terms %s (window of every kept lag, bursts at the last one)" % flips)
    # the multi-pass pipeline at the other block lengths
    for n, h, tname in ((1024, 256, "g127"), (8192, 2048, "g1023"), (32768, 8192, "g4094"),
                        (65536, 8192, "g6141")):
        lo, hi = corr_window(n, h, tname)
        edges = [lo, lo + 1, hi - 1, hi - 2]
        roll = [(n - s) % n for s in (3, 17, n // 4 + 5, n // 2 - 1, 3 * n // 4 + 33, n - 20, n // 8 + 7)]
        full = [(c, b, edges[i % 4], t, a) for i, (c, b, _, t, a) in
                enumerate(at([0, 1, n - 1, n // 2] + roll, n=n))]
        add("mp_full_%d" % n, n, h, tname, (0, -1), full,
            edge="multi-pass, window (0, -1): bins 0 and N - 1, a short roll sweep, correlation edges")
        wrap = [(d, n, lo, TONE, BURST) for d in (0.1, -0.1)] + at([5, -7, 12, -12, 1, -1], n=n)
        add("mp_sic_%d" % n, n, h, tname, (-12, 12), wrap, edge="multi-pass wrapping window, bin N: IndexError")
        add("mp_sic_none_%d" % n, n, h, tname, (-12, 12), wrap, interp="none",
            edge="multi-pass wrapping window, none: a record at bin N rolled by -N")
        # (at 1024 a carrier or burst is some 150 / 500 times the noise power, not 1000s)
        fd_thr = FD_THR if n > 1024 else (0.0, 50.0, 0.0)
        add("mp_fastdet_%d" % n, n, h, tname, (0, n - 1), full, kind="fastdet", cthr=fd_thr, xthr=fd_thr,
            edge="multi-pass fastdet: bins 0 and N - 1, a short roll sweep, correlation edges")
    return rows


ROWS = _rows()
IDS = [r["id"] for r in ROWS]
BY_ID = dict(zip(IDS, ROWS))
R16 = [r for r in ROWS if r["n"] == N16]


def make_blocks(r):
    n, tpl = r["n"], template(r["tpl"])
    w = len(tpl)
    lo, hi = corr_window(n, r["h"], r["tpl"])
    rng = np.random.default_rng(zlib.crc32(r["id"].encode()))
    k, kk = np.arange(n), np.arange(w)
    out, lags = [], []
    for car, _, lag, tone, burst in r["planted"]:
        lag = int(rng.integers(lo, hi)) if lag is None else lag
        z = rng.normal(0, 0.02, n) + 1j * rng.normal(0, 0.02, n)
        # a continuous carrier (a one-bin main lobe: the peak bin is unambiguous) under the burst
        z += tone * np.exp(2j * np.pi * car * k / n)
        z[lag:lag + w] += burst * (tpl + 1) / 2 * np.exp(2j * np.pi * car * (kk + lag) / n)
        out.append(synth.quantise_iq(z))
        lags.append(lag)
    return np.stack(out), np.array(lags)


def interp_arg(r):
    return "parabolic" if r["kind"] == "fastdet" else r["interp"]


def engine(r, **kw):
    tpl = template(r["tpl"])
    if r["kind"] == "fastdet":
        return F.Engine(r["n"], r["h"], tpl, r["cthr"], r["win"], r["xthr"], max_batch=MAX_BATCH,
                        fastdet=True, **kw)
    return F.Engine(r["n"], r["h"], tpl, r["cthr"], r["win"], r["xthr"], max_batch=MAX_BATCH,
                    preshift_num=r["num"], interpolator=r["interp"], **kw)


def oracle_config(r, blocks, cthr=None, xthr=None):
    return (blocks, r["n"], r["h"], template(r["tpl"]), cthr or r["cthr"], r["win"], xthr or r["xthr"],
            None, r["num"], interp_arg(r), r["kind"] == "fastdet")


def oracle_peak(r, block):
    """The record bin the oracle's carrier search gives (the reference's first-max, sic bin N)."""
    n = r["n"]
    spec = np.fft.fft(onp.iq_u8_to_c64(block))
    if r["kind"] == "fastdet":
        p = (spec.real.astype(np.float32) ** 2 + spec.imag.astype(np.float32) ** 2).astype(np.float32)
        lo, hi = onp.fastdet_window(r["win"][0], r["win"][1], n)
        return int(np.argmax(p[lo:hi + 1])) + lo
    return onp.carrier_peak(np.abs(spec), r["win"])[0]


def bank_rule(peak, offset, num):
    """k_preshift's bank index from the record's own (widened float32) carrier offset."""
    shift = -(np.float64(peak) + np.float64(offset))
    frac = shift - np.round(shift)
    return int(min(max(np.round((frac + 0.5) * (num - 1)), 0), num - 1))


# ---------------------------------------------------------------------------------------------
# (a) the table and the kernel's index arithmetic (no GPU)
# ---------------------------------------------------------------------------------------------
def gather_positions(s):
    """k_preshift's gather restated: for every thread t of 512 and register slot k3, the bank
    position it reads for bin k = k1 + 16 k2 + 512 k3, and the carries it took."""
    t = np.arange(512)[:, None]
    k3 = np.arange(32)[None, :]
    s1, s2, s3 = digits(s)
    k1s = (t >> 5) + s1
    k2s = (t & 31) + s2 + (k1s >> 4)
    q3 = s3 + (k2s >> 5)
    pos = ((k3 + q3) & 31) * 512 + ((k1s & 15) * 32 + (k2s & 31))
    k = (t >> 5) + 16 * (t & 31) + 512 * k3
    return pos, k, (k1s >> 4).ravel(), (k2s >> 5).ravel()


def bank_position(k):
    """build_preshift_bank's layout of bin k on the 16384 path."""
    return ((k >> 9) * 16 + (k & 15)) * 32 + ((k >> 4) & 31)


def neighbour_owners(peak):
    """The neighbour publish restated: {bin: k3 slot} that the owners of bins peak -+ 1 publish."""
    t = np.arange(512)
    kbase = (t >> 5) + 16 * (t & 31)
    u = (kbase - peak + 1) & (N16 - 1)
    r, k3s = u & 511, (32 - (u >> 9)) & 31
    own = (r == 0) | (r == 2)
    return {int(kbase[i] + 512 * k3s[i]): int(k3s[i]) for i in np.flatnonzero(own)}


def corr_neighbours(pk):
    """k_preshift's correlation neighbour extraction restated: {d: lag} that some thread writes
    into m2[d], from the column 2 t + e and row n1s it holds."""
    out = {}
    for j in range(1024):
        delta = pk - 1 - j
        d = (-delta) & 1023
        n1s = (delta + d) >> 10
        if d < 3 and 0 <= n1s < 16:
            assert d not in out
            out[d] = n1s * 1024 + j
    return out


def test_the_table_covers_every_digit_and_edge_it_claims():
    assert len(set(IDS)) == len(IDS)
    for r in ROWS:
        assert 4 <= len(r["planted"]) <= MAX_BATCH, r["id"]
        assert r["kernel"] == (FUSED if r["n"] == N16 else MULTI)
    # the gather reads Tc[(k + s) mod N] for every s of the table, and the sweep meets every digit
    # value with and without a carry into it
    for kind in ("preshift", "fastdet"):
        for interp in (("parabolic", "none", "gaussian", "cosine") if kind == "preshift" else ("parabolic",)):
            rows = [r for r in R16 if r["kind"] == kind and interp_arg(r) == interp and r["win"][:1] == (0,)
                    and r["id"].startswith(("full", "fastdet_full"))]
            assert len(rows) == 1, (kind, interp)
            ss = {roll_of(N16, b) for _, b, _, _, _ in rows[0]["planted"]}
            seen1, seen2, seen3, carry1, carry2, k3s = set(), set(), set(), set(), set(), set()
            for s in ss:
                pos, k, c1, c2 = gather_positions(s)
                assert np.array_equal(pos, bank_position((k + s) % N16)), s
                s1, s2, s3 = digits(s)
                seen1.add(s1)
                seen2.add(s2)
                seen3.add(s3)
                carry1 |= {(s2, c) for c in set(c1.tolist())}
                carry2 |= {(s3, c) for c in set(c2.tolist())}
            for _, b, _, _, _ in rows[0]["planted"]:
                own = neighbour_owners(b)
                for nb in ((b - 1) % N16, b + 1):
                    if nb < N16:
                        assert own[nb] == nb >> 9, (b, nb, own)
                        k3s.add(nb >> 9)
            assert seen1 == set(range(16)) and seen2 == seen3 == set(range(32)), (kind, interp)
            assert carry1 == {(v, c) for v in range(32) for c in (0, 1)}, (kind, interp)
            assert carry2 == {(v, c) for v in range(32) for c in (0, 1)}, (kind, interp)
            assert 0 in ss and k3s == set(range(32)), (kind, interp)
            assert {b for _, b, _, _, _ in rows[0]["planted"]} >= set(NAMED_BINS)
    # the correlation rows: peaks in row 0, on every seam inside the window, and the extraction
    # hands k_finish exactly lags pk - 1 .. pk + 1 that exist
    for r in R16:
        if not r["id"].startswith("corr_"):
            continue
        lo, hi = corr_window(N16, r["h"], r["tpl"])
        _, lags = make_blocks(r)
        assert {lo, lo + 1, hi - 1, hi - 2} <= set(lags.tolist())
        for m in range(1, 16):
            for v in (1024 * m - 1, 1024 * m, 1024 * m + 1):
                assert (v in lags) == (lo <= v < hi), (r["id"], v)
        for pk in lags:
            assert corr_neighbours(int(pk)) == {d: pk - 1 + d for d in range(3) if pk - 1 + d >= 0}
    assert (0 in make_blocks(BY_ID["corr_1022_1023"])[1]) and (N16 - 1023 in make_blocks(BY_ID["corr_1022_1023"])[1])
    assert min(make_blocks(BY_ID["corr_3070_1023"])[1]) == 1024
    # the instantiations: (carrier stddev, correlation stddev, parabolic-only) x u8 / c64 input
    inst = {(bool(r["cthr"][2]), bool(r["xthr"][2]), interp_arg(r) == "parabolic") for r in R16}
    assert inst == {(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)}
    assert {r["kind"] for r in ROWS if r["n"] != N16} == {"preshift", "fastdet"}
    assert {r["n"] for r in ROWS} == {1024, 8192, N16, 32768, 65536}
    assert {r["num"] for r in ROWS if r["id"].startswith("bank_")} == {1, 2, 3, 21, 101, 1001}


def test_each_planted_carrier_peaks_at_the_claimed_bin():
    for r in ROWS:
        blocks, _ = make_blocks(r)
        got = [oracle_peak(r, b) for b in blocks]
        want = [b for _, b, _, _, _ in r["planted"]]
        if r["id"].startswith("std_"):
            # (the weak end of the carrier ladder may peak on noise: no claim there)
            assert sum(g == w for g, w in zip(got, want)) >= 18, (r["id"], got)
            continue
        assert got == want, (r["id"], got, want)


def test_each_stddev_row_flips_a_verdict_without_its_term():
    configs, keys = [], []
    for r in R16:
        if not r["flips"]:
            continue
        blocks, _ = make_blocks(r)
        configs.append(oracle_config(r, blocks))
        keys.append((r["id"], "row"))
        if "carrier" in r["flips"]:
            configs.append(oracle_config(r, blocks, cthr=r["cthr"][:2] + (0,)))
            keys.append((r["id"], "carrier"))
        if "correlation" in r["flips"]:
            configs.append(oracle_config(r, blocks, xthr=r["xthr"][:2] + (0,)))
            keys.append((r["id"], "correlation"))
    out = dict(zip(keys, soak_util.run_oracle_many(configs, procs=8, chunk=8)))
    assert len({k[0] for k in keys}) == 6
    for (rid, what), rows in out.items():
        if what == "row":
            continue
        base = out[(rid, "row")]
        if what == "carrier":
            flipped = [i for i, (a, b) in enumerate(zip(base, rows)) if a[1] != b[1]]
        else:
            flipped = [i for i, (a, b) in enumerate(zip(base, rows)) if a[1] and b[1] and a[5] != b[5]]
        assert flipped, (rid, what)


# ---------------------------------------------------------------------------------------------
# the oracle, once for the file
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    data, configs = {}, []
    for r in ROWS:
        blocks, lags = make_blocks(r)
        data[r["id"]] = dict(blocks=blocks, lags=lags)
        configs.append(oracle_config(r, blocks))
    for r, rows in zip(ROWS, soak_util.run_oracle_many(configs, procs=8, chunk=16)):
        data[r["id"]]["oracle"] = rows
    return data


_FLIPS = []   # (row, block) whose bank differs from the oracle's, over the whole file


def check(r, rec, d, tag):
    n, rows, blocks, lags = r["n"], d["oracle"], d["blocks"], d["lags"]
    fd = r["kind"] == "fastdet"
    n_car = n_cor = 0
    for i, row in enumerate(rows):
        g = rec[i]
        where = (r["id"], tag, i, g, row)
        claim = r["planted"][i][1]
        if row is None:      # the reference's IndexError
            assert g["flags"] & F.FLAG_INDEX_ERROR and not g["flags"] & F.FLAG_CARRIER, where
            assert g["carrier_bin"] == claim and g["reserved"] == 0, where
            continue
        cbin, cdet, coff, cen, samp, det, en, off, noise, cnoise, last, int_off = row
        assert not g["flags"] & F.FLAG_INDEX_ERROR, where
        assert g["carrier_bin"] == cbin, where
        assert bool(g["flags"] & F.FLAG_CARRIER) == cdet, where
        np.testing.assert_allclose(g["carrier_energy"], cen, rtol=2e-5, err_msg=str(where))
        np.testing.assert_allclose(g["carrier_noise"], cnoise, rtol=1e-4, err_msg=str(where))
        if not cdet:
            assert g["reserved"] == 0, where
            continue
        n_car += 1
        assert bool(g["flags"] & F.FLAG_INT_OFFSET) == (int_off and r["interp"] == "cosine" and not fd), where
        np.testing.assert_allclose(g["carrier_offset"], coff, atol=1e-4, err_msg=str(where))
        # reserved: the roll the oracle took (high word) and the bank the rule gives for the
        # engine's own offset (low word)
        hi_w = int(np.uint32(g["reserved"] >> np.uint64(32)).astype(np.int32))
        lo_w = int(g["reserved"] & np.uint64(0xFFFFFFFF))
        assert hi_w == last[0], where
        assert lo_w == (0 if fd else bank_rule(g["carrier_bin"], g["carrier_offset"], r["num"])), where
        want = dict(sample=samp, det=det, energy=en, offset=off, noise=noise)
        if lo_w != last[2]:
            # a bank flip: a bank boundary lies between the two offsets, and the oracle at the
            # engine's (roll, bank) gives the record
            num = r["num"]
            fr = sorted([-(cbin + coff) - last[0], -(cbin + float(g["carrier_offset"])) - last[0]])
            assert abs(lo_w - last[2]) == 1, where
            edge = (min(lo_w, last[2]) + 0.5) / (num - 1) - 0.5
            assert fr[0] <= edge <= fr[1], (where, fr, edge)
            orc = onp.OraclePreshiftDetector(n, r["h"], template(r["tpl"]), r["cthr"], r["win"], r["xthr"],
                                             num=num, interpolator=r["interp"])
            res = orc.detect_u8(i, blocks[i], force=(hi_w, lo_w))
            want = dict(sample=res.corr.sample, det=res.corr.detected, energy=res.corr.energy,
                        offset=res.corr.offset, noise=res.corr.noise)
            if (r["id"], i) not in _FLIPS:
                _FLIPS.append((r["id"], i))
        assert g["corr_sample"] == want["sample"], where
        assert bool(g["flags"] & F.FLAG_CORR) == want["det"], where
        np.testing.assert_allclose(g["corr_energy"], want["energy"], rtol=1e-4, err_msg=str(where))
        if fd:
            np.testing.assert_allclose(g["corr_noise"], want["noise"], rtol=1e-3, atol=1e-3, err_msg=str(where))
        else:
            np.testing.assert_allclose(g["corr_noise"], want["noise"], rtol=1e-4, err_msg=str(where))
        if want["det"]:
            n_cor += 1
            np.testing.assert_allclose(g["corr_offset"], want["offset"], atol=1e-4, err_msg=str(where))
            if r["planted"][i][2] is not None and r["planted"][i][4] >= BURST:
                assert g["corr_sample"] == lags[i], where      # the planted lag is the one reached
    assert len(_FLIPS) <= 2, _FLIPS
    # (not vacuous)
    assert n_car >= min(4, len(rows) // 2) and n_cor >= min(4, len(rows) // 3), (r["id"], n_car, n_cor)


# ---------------------------------------------------------------------------------------------
# (b) the kernel, (c) the oracle, (d) fused against multi-pass
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=IDS)
def test_the_engine_reports_the_kernel_of_the_row(r):
    eng = engine(r)
    info = eng.path_info()
    eng.close()
    assert info["carrier_kernel"] == info["correlate_kernel"] == r["kernel"], (r["id"], info)
    if r["n"] == N16:
        eng = engine(r, path="multipass")
        info = eng.path_info()
        eng.close()
        assert info["carrier_kernel"] == info["correlate_kernel"] == MULTI, (r["id"], info)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["auto", "multipass"])
@pytest.mark.parametrize("r", ROWS, ids=IDS)
def test_records_equal_the_oracle(r, path, cases):
    if path == "multipass" and r["n"] != N16:
        return      # (the auto path of these lengths is the multi-pass pipeline)
    d = cases[r["id"]]
    eng = engine(r, path=path)
    idx = np.arange(len(d["blocks"]))
    check(r, eng.detect(d["blocks"], idx)[:, 0], d, path + "/u8")
    check(r, eng.detect(np.stack([onp.iq_u8_to_c64(b) for b in d["blocks"]]), idx)[:, 0], d, path + "/c64")
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("r", R16, ids=[r["id"] for r in R16])
def test_the_fused_kernel_and_the_multi_pass_pipeline_agree(r, cases):
    blocks = cases[r["id"]]["blocks"]
    fast_eng, slow_eng = engine(r), engine(r, path="multipass")
    fast, slow = fast_eng.detect(blocks)[:, 0], slow_eng.detect(blocks)[:, 0]
    fast_eng.close()
    slow_eng.close()
    for f in ("carrier_bin", "flags", "corr_sample", "reserved"):
        assert np.array_equal(fast[f], slow[f]), (r["id"], f, fast[f], slow[f])
    car = (fast["flags"] & F.FLAG_CARRIER) != 0
    assert car.sum() >= 4
    for f in ("carrier_energy", "carrier_noise", "corr_energy"):
        np.testing.assert_allclose(fast[f], slow[f], rtol=2e-5, err_msg=f)
    np.testing.assert_allclose(fast["carrier_offset"], slow["carrier_offset"], atol=2e-5)
    det = (fast["flags"] & F.FLAG_CORR) != 0
    np.testing.assert_allclose(fast["corr_offset"][det], slow["corr_offset"][det], atol=2e-5)
