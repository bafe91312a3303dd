"""The correlate stage at its window edges and section seams, for every block length outside 16384
(test_gpu_window_geometry.py and test_gpu_sections16k.py pin that one).  Each correlate kernel has
its own window and seam logic:

  k_correlate_seg     32768 / 65536: overlap-save sections of 16384 samples (detect_seg.hip,
                      handle.hip: plan_sections), per-section peaks merged by k_finish
  k_correlate_sub     32768 / 65536 unsectioned (templates too long to section, path="unsectioned",
                      stage dumps): the fused kernel, or k_correlate_sub + k_combine in chunks of
                      long_chunk work-list slots when a batch has fewer carrier-positive blocks than
                      fused_grid (pipeline.hip: run_batch_long)
  k_correlate_small   1024 ... 8192: 16 / R1 blocks per workgroup, lags visited as n1 * 1024 + column
  g_* (multi-pass)    every other power of two

Every row of the table below names the kernel, sections and window-row specialisation the engine
must report, and the edge or seam it sits on.  Bursts are planted on the window edges, on both sides
of every seam, on lag 0 / the last kept lag where the window holds them, and just outside the window.

  (a) long blocks: the reported form; each row on the boundary it claims (no GPU); records against
      the CPU oracle (u8 and complex64 input); path="generic_rows" byte for byte, path="unsectioned"
      to float32 rounding; four templates
  (b) the k_correlate_sub schedule: one, two and three chunks of the two-kernel form and both sides
      of its switch to the fused kernel, against batches of three blocks and the oracle; its stage dumps
  (c) short blocks against the oracle and the multi-pass pipeline
  (d) multi-pass block lengths against the oracle"""
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
from test_gpu_sections16k import _close  # noqa: E402

M = 16384
THR = (0, 15, 0)
XTHR_STD = (0, 12, 0.5)
SEG, SUB, SMALL, MULTI = "k_correlate_seg", "k_correlate_sub", "k_correlate_small", "g_* (multi-pass)"
GENERIC = (-1, -1)


def row(n, h, w, form, nsec, geom, why, win, point, **claims):
    """claims: seam_lo / seam_hi = g (the window edge is section g's first owned lag), empty / one =
    sections owning no / exactly one window lag, owns = {g: [lo, hi)}, lag0 / last = the window
    holds lag 0 / the last kept lag, std = corr_thresh with a stddev term."""
    return dict(n=n, h=h, w=w, form=form, nsec=nsec, geom=geom, why=why, win=win, point=point, **claims)


# ---------------------------------------------------------------------------------------------
# (a) long blocks: (N, history, template length) -> what the engine reports, and why the row is here
# ---------------------------------------------------------------------------------------------
LONG = [
    row(65536, 4096, 4094, SEG, 5, (0, 3), "sectioned", (1, 61441), "configs[2]: the row table (0, 3)"),
    row(65536, 4093, 4094, SEG, 5, (0, 3), "sectioned", (0, 61443), "lag 0 and the last kept lag, still (0, 3)",
        lag0=True, last=True),
    row(65536, 28671, 4094, SEG, 5, GENERIC, "sectioned", (12289, 49154), "starts on seam 1",
        seam_lo=1, empty=[0], one=[4]),
    row(65536, 31744, 1023, SEG, 5, GENERIC, "sectioned", (15361, 49153), "both edges on seams",
        seam_lo=1, seam_hi=4, empty=[0, 4]),
    row(65536, 31742, 1023, SEG, 5, GENERIC, "sectioned", (15360, 49154), "sections 0 and 4 own one lag each",
        one=[0, 4]),
    row(65536, 1022, 1023, SEG, 5, GENERIC, "sectioned", (0, 64514), "a ragged 4th section",
        lag0=True, last=True, owns={3: (46081, 49153)}),
    row(65536, 9500, 9361, SEG, 8, GENERIC, "sectioned", (70, 56106), "8 sections, the most allowed"),
    row(65536, 9500, 9362, SUB, 0, GENERIC, "geometry", (69, 56105), "one sample too long to section"),
    row(65536, 6001, 4094, SEG, 5, GENERIC, "sectioned", (954, 60489), "stddev term: sums tile [0, corr_len)",
        std=True),
    row(32768, 4096, 4094, SEG, 3, GENERIC, "sectioned", (1, 28673), "3 sections, a short middle one",
        owns={1: (12289, 16385)}),
    row(32768, 28671, 4094, SEG, 3, GENERIC, "sectioned", (12289, 16386), "the middle section plus one lag",
        seam_lo=1, empty=[0], one=[2], owns={1: (12289, 16385)}),
    row(32768, 1022, 1023, SEG, 3, GENERIC, "sectioned", (0, 31746), "lag 0; a middle section of 1024 lags",
        lag0=True, last=True, owns={1: (15361, 16385)}),
]

# (c) short blocks and (d) multi-pass block lengths: Gold templates of 2^b - 1 chips
SHORT = [
    row(1024, 126, 127, SMALL, 0, GENERIC, "block_len", (0, 898), "H = W - 1", lag0=True, last=True),
    row(1024, 1000, 127, SMALL, 0, GENERIC, "block_len", (437, 461), "narrow"),
    row(2048, 254, 255, SMALL, 0, GENERIC, "block_len", (0, 1794), "H = W - 1", lag0=True, last=True),
    row(2048, 2024, 255, SMALL, 0, GENERIC, "block_len", (885, 909), "narrow"),
    row(4096, 510, 511, SMALL, 0, GENERIC, "block_len", (0, 3586), "H = W - 1", lag0=True, last=True),
    row(4096, 2558, 511, SMALL, 0, GENERIC, "block_len", (1024, 2562), "starts on row 1", row_lo=True),
    row(4096, 3585, 511, SMALL, 0, GENERIC, "block_len", (1537, 2048), "ends on row 2", row_hi=True),
    row(4096, 4072, 511, SMALL, 0, GENERIC, "block_len", (1781, 1805), "narrow"),
    row(8192, 1022, 1023, SMALL, 0, GENERIC, "block_len", (0, 7170), "H = W - 1", lag0=True, last=True),
    row(8192, 5118, 1023, SMALL, 0, GENERIC, "block_len", (2048, 5122), "starts on row 2", row_lo=True),
    row(8192, 3073, 1023, SMALL, 0, GENERIC, "block_len", (1025, 6144), "ends on row 6", row_hi=True),
    row(8192, 8168, 1023, SMALL, 0, GENERIC, "block_len", (3573, 3597), "narrow"),
]
MULTIPASS = [
    row(512, 62, 63, MULTI, 0, GENERIC, "block_len", (0, 450), "H = W - 1", lag0=True, last=True),
    row(512, 200, 63, MULTI, 0, GENERIC, "block_len", (69, 381), "interior"),
    row(131072, 12281, 12282, MULTI, 0, GENERIC, "block_len", (0, 118791), "H = W - 1", lag0=True, last=True),
    row(131072, 16384, 12282, MULTI, 0, GENERIC, "block_len", (2051, 116739), "interior"),
]
ROWS = LONG + SHORT + MULTIPASS


def row_id(r):
    return "%d_%d_%d%s" % (r["n"], r["h"], r["w"], "_std" if r.get("std") else "")


LONG_IDS = [row_id(r) for r in LONG]
SHORT_IDS = [row_id(r) for r in SHORT]
# the rows run with four templates
T4_IDS = ["65536_4096_4094", "65536_31744_1023"]


def template(w, k=0):
    """A +-1 template of w samples: Gold codes where the length is one, else seeded random signs."""
    gold = {63: (6, 1.0), 127: (7, 1.0), 255: (8, 1.0), 511: (9, 1.0), 1023: (10, 1.0), 4094: (11, 2.0),
            12282: (11, 6.0)}
    if w in gold:
        t = synth.gold_template(gold[w][0], 2 + k, gold[w][1]).astype(np.float64)
        assert len(t) == w
        return t
    rng = np.random.default_rng(w * 8 + k)
    return np.where(rng.random(w) < 0.5, -1.0, 1.0)


def cwin_of(n):
    return (3, 60) if n <= 1024 else (7, 110)


def xthr_of(r):
    return XTHR_STD if r.get("std") else THR


# ---------------------------------------------------------------------------------------------
# restatements of the planner and of the row-table pick (the engine's answer is the truth: the
# GPU tests below compare them with what the handle reports)
# ---------------------------------------------------------------------------------------------
def plan_restated(n, h, w):
    """handle.hip: plan_sections -> [dict(start, win_lo, win_hi, sum_lo, sum_hi)] (block lags)."""
    v = M - w + 1
    if n <= M or v < 4:
        return []
    stride = (v - 2) & ~1
    nseg = (n - M + stride - 1) // stride + 1
    if nseg > 8:
        return []
    corr_len = n - w + 1
    lo, hi = onp.unique_window(n, h, w)
    out, own_lo = [], 0
    for g in range(nseg):
        start = min(g * stride, n - M)
        own_hi = min((g + 1) * stride, n - M) + 1 if g + 1 < nseg else corr_len
        wl = max(own_lo, lo)
        out.append(dict(start=start, win_lo=wl, win_hi=max(min(own_hi, hi), wl), sum_lo=own_lo, sum_hi=own_hi))
        own_lo = own_hi
    return out


def row_geom_restated(plan, std=False):
    """correlate16k.hpp: row_geom_applies + correlate16k_geom.hpp: pick_row_geom with RLO = 0 (the
    sections' owned lags start at 0 or 1): one (0, RHI) must fit the window of every section."""
    if std or not plan:
        return GENERIC

    def applies(hi, w_lo, w_hi):
        return (hi == 0 or (16 - hi) * 1024 > w_hi) and 1024 >= w_lo and (15 - hi) * 1024 <= w_hi
    for hi in range(4, -1, -1):
        if all(applies(hi, s["win_lo"] - s["start"], s["win_hi"] - s["start"]) for s in plan):
            return (0, hi)
    return GENERIC


def seams(plan):
    """The first owned lag of every section but the first."""
    return [s["sum_lo"] for s in plan[1:]]


# ---------------------------------------------------------------------------------------------
# without a GPU: every row sits where it claims
# ---------------------------------------------------------------------------------------------
def test_every_row_sits_on_the_boundary_it_claims():
    assert len(set(row_id(r) for r in ROWS)) == len(ROWS)
    for r in ROWS:
        n, h, w = r["n"], r["h"], r["w"]
        lo, hi = onp.unique_window(n, h, w)
        corr_len = n - w + 1
        assert (lo, hi) == r["win"], (row_id(r), lo, hi)
        assert r.get("lag0", False) == (lo == 0) and r.get("last", False) == (hi == corr_len), row_id(r)
        if r.get("row_lo"):
            assert lo % 1024 == 0 and lo > 0, row_id(r)
        if r.get("row_hi"):
            assert hi % 1024 == 0, row_id(r)
        plan = F.plan_sections(n, h, w)
        if r["form"] != SEG:
            assert plan == [] and r["nsec"] == 0
            continue
        assert plan == plan_restated(n, h, w), row_id(r)
        assert len(plan) == r["nsec"]
        assert row_geom_restated(plan, r.get("std")) == r["geom"], row_id(r)
        own = [(s["win_lo"], s["win_hi"]) for s in plan]
        assert [g for g, (a, b) in enumerate(own) if a == b] == r.get("empty", []), (row_id(r), own)
        assert [g for g, (a, b) in enumerate(own) if b - a == 1] == r.get("one", []), (row_id(r), own)
        for g, want in r.get("owns", {}).items():
            assert own[g] == want, (row_id(r), g, own[g])
        for key, edge in (("seam_lo", lo), ("seam_hi", hi)):
            on = [g for g in range(1, len(plan)) if plan[g]["sum_lo"] == edge]
            assert on == ([r[key]] if key in r else []), (row_id(r), key, on)
        # the sums tile every kept lag (what a stddev term needs), the windows the unique window
        assert plan[0]["sum_lo"] == 0 and plan[-1]["sum_hi"] == corr_len
        assert all(a["sum_hi"] == b["sum_lo"] for a, b in zip(plan, plan[1:]))
        assert own[0][0] == max(lo, 0) and max(b for _, b in own) == hi
    # the 9362-sample row is the first length that does not section at 65536
    assert F.plan_sections(65536, 9500, 9361) and not F.plan_sections(65536, 9500, 9362)


def test_the_table_reaches_every_row_geometry_the_long_path_can_report():
    """Over every template length that sections and a spread of histories, the sectioned path can
    pick only (0, 3) -- a section owns V - 2 lags, and only W = 4094 / 4095 give every section of
    65536 (no ragged one) a window ending in row 12 -- or the generic kernel.  The table holds both."""
    reach = set()
    for n in (32768, 65536):
        for w in range(2, 9400):
            for h in (w - 1, w + 1, w + 500, w + 2000):
                plan = plan_restated(n, h, w)
                if plan:
                    reach.add(row_geom_restated(plan))
                if w % 331 == 0:
                    assert F.plan_sections(n, h, w) == plan, (n, h, w)
    assert reach == {(0, 3), GENERIC}
    assert {r["geom"] for r in LONG if r["form"] == SEG} == reach
    assert {r["form"] for r in ROWS} == {SEG, SUB, SMALL, MULTI}


# ---------------------------------------------------------------------------------------------
# blocks
# ---------------------------------------------------------------------------------------------
def burst_lags(r, rng, n_random):
    """Window edges, both sides of every seam, lag 0 and the last kept lag, 1024-lag row boundaries
    (short blocks), then random lags -- inside the window; last, the kept lags just outside it
    (lo - 1, hi), whose peak the window test must drop."""
    n, h, w = r["n"], r["h"], r["w"]
    lo, hi = r["win"]
    lags = [lo, lo + 1, lo + 2, hi - 1, hi - 2, hi - 3, 0, n - w]
    for s in seams(plan_restated(n, h, w)) if r["form"] == SEG else []:
        lags += [s - 2, s - 1, s, s + 1]
    if r["form"] == SMALL:
        for k in range(1, n // 1024):
            lags += [1024 * k - 1, 1024 * k]
    lags = [p for p in dict.fromkeys(lags) if lo <= p < hi]
    outside = [p for p in (lo - 1, hi) if 0 <= p <= n - w]
    return lags + [int(p) for p in rng.integers(lo, hi, n_random)] + outside


def noise_block(rng, n, tone):
    """Noise only, or noise and a strong bare tone inside the carrier window.  Both are carrier-
    negative: the tone holds more than half the block's energy, so the reference's noise estimate
    sqrt((sum |X|^2 - 2 peak^2) / (N - 1)) is NaN and no threshold passes (carrier_detect.py:99-107)."""
    z = rng.normal(0, 0.02, n) + 1j * rng.normal(0, 0.02, n)
    if tone:
        z = z + 0.05 * np.exp(2j * np.pi * 20.3 * np.arange(n) / n)
    return synth.quantise_iq(z)


def make_blocks(r, tpls, n_random, odd_positive=False):
    """Bursts at burst_lags (block i carries template i % T), and a noise or tone block after every
    fourth burst.  odd_positive: an odd count of carrier-positive blocks (the bursts), so that the
    last group of 16 / R1 short blocks is partly filled whatever R1 is."""
    n = r["n"]
    rng = np.random.default_rng(zlib.crc32(row_id(r).encode()) + len(tpls))
    lags = burst_lags(r, rng, n_random)
    cw = cwin_of(n)
    cbins = (cw[0] + 5.0, min(cw[1] - 5.0, n / 8.0))
    bursts = [synth.synth_blocks(rng, 1, n, tpls[i % len(tpls)], r["win"], positions=np.array([p]),
                                 carrier_bins=cbins)[0][0] for i, p in enumerate(lags)]
    blocks, kinds = [], []
    for i, b in enumerate(bursts):
        blocks.append(b)
        kinds.append(1)
        if i % 4 == 3:
            tone = (i // 4) % 2 == 0
            blocks.append(noise_block(rng, n, tone))
            kinds.append(2 if tone else 0)
    if odd_positive and len(bursts) % 2 == 0:
        blocks.append(blocks[0])
        kinds.append(1)
        lags.append(lags[0])
    return np.stack(blocks), np.array(kinds), lags


# ---------------------------------------------------------------------------------------------
# (b) the k_correlate_sub schedule
# ---------------------------------------------------------------------------------------------
def long_chunk_blocks(block_len, n_templates):
    """detect_long.hip: long_chunk_blocks -- work-list slots per chunk of the two-kernel form (the
    d_k0 exchange of one chunk kept near 128 MiB)."""
    return max(16, (128 << 20) // (8 * block_len * n_templates))


SCHED = [  # (N, history, template length, path)
    (65536, 4096, 4094, "unsectioned"),
    (32768, 4096, 4094, "unsectioned"),
    (65536, 9500, 9362, "auto"),
]
SCHED_IDS = ["%d_%d_%s" % (n, w, p) for n, _, w, p in SCHED]
SCHED_T, SCHED_BATCH, SCHED_DISTINCT, SCHED_POS = 4, 256, 48, 32


def sched_tpls(w):
    return np.stack([template(w, k) for k in range(SCHED_T)])


def sched_blocks(n, h, w):
    """48 distinct blocks: 32 carry a burst (block j template j % 4), 16 are noise only -- their
    carrier verdict must be negative."""
    rng = np.random.default_rng(n + w)
    tpls = sched_tpls(w)
    win = onp.unique_window(n, h, w)
    pos = [synth.synth_blocks(rng, 1, n, tpls[j % SCHED_T], win, carrier_bins=(12.0, 100.0))[0][0]
           for j in range(SCHED_POS)]
    neg = [noise_block(rng, n, False) for _ in range(SCHED_DISTINCT - SCHED_POS)]
    return np.stack(pos + neg)


def sched_order(n, w, p):
    """A batch of 256 slots with p carrier-positive ones at random places: slot -> distinct block."""
    rng = np.random.default_rng(p * 7 + n + w)
    order = np.empty(SCHED_BATCH, dtype=np.int64)
    where = rng.permutation(SCHED_BATCH)
    order[where[:p]] = np.arange(p) % SCHED_POS
    order[where[p:]] = SCHED_POS + np.arange(SCHED_BATCH - p) % (SCHED_DISTINCT - SCHED_POS)
    return order


# ---------------------------------------------------------------------------------------------
# the oracle: one pool of workers for the whole file
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    data, configs, keys = {}, [], []

    def add(key, blocks, n, h, tpl, xthr):
        configs.append((blocks, n, h, tpl, THR, cwin_of(n), xthr, None, 0))
        keys.append(key)
    for r in ROWS:
        tpl = template(r["w"])
        blocks, kinds, lags = make_blocks(r, [tpl], 20 if r["n"] > 8192 else 24, odd_positive=r["form"] == SMALL)
        data[row_id(r)] = dict(blocks=blocks, kinds=kinds, lags=lags)
        add((row_id(r), 0), blocks, r["n"], r["h"], tpl, xthr_of(r))
    for r in LONG:
        if row_id(r) not in T4_IDS:
            continue
        tpls = [template(r["w"], k) for k in range(4)]
        blocks, kinds, lags = make_blocks(r, tpls, 8)
        data[(row_id(r), 4)] = dict(blocks=blocks, kinds=kinds, lags=lags)
        for t in range(4):
            add(((row_id(r), 4), t), blocks, r["n"], r["h"], tpls[t], THR)
    for (n, h, w, path), sid in zip(SCHED, SCHED_IDS):
        blocks = sched_blocks(n, h, w)
        data[sid] = dict(blocks=blocks)
        for t, tpl in enumerate(sched_tpls(w)):
            add((sid, t), blocks, n, h, tpl, THR)
    for key, rows in zip(keys, soak_util.run_oracle_many(configs, procs=16, chunk=8)):
        data[key[0]].setdefault("oracle", {})[key[1]] = rows
    return data


def corr_off_per_bin(r):
    """A 1023-sample burst in a block of 32768 or 65536 has a carrier lobe 32 or 64 bins wide against
    the 7 fitted bins: the kernels' float32 fit and the oracle's float64 one part by up to ~5e-4 bins,
    and the shift carries that into the correlation peak.  There corr_offset may move with the
    carrier offset's deviation (samples per bin, test_gpu_carrier_windows.py's rule); elsewhere 5e-6."""
    return 0.5 if r["n"] > 8192 and r["n"] / r["w"] > 24 else 0.0


def check_against_oracle(rec, rows, blocks, only=None, per_bin=0.0):
    mism, worst, ties = soak_util.compare(rec, rows, blocks, F.FLAG_CARRIER, F.FLAG_CORR, F.FLAG_INDEX_ERROR,
                                          only=only, flag_fit=F.FLAG_FIT_UNCONVERGED)
    assert mism == dict(bin=0, carrier=0, sample=0, det=0, index_error=0), (mism, worst, ties)
    assert not ties, ties
    assert worst["energy"] <= 2e-5 and worst["noise"] <= 2e-5, worst
    if not per_bin:
        assert worst["offset"] <= 5e-6, worst
        return
    for i, row in enumerate(rows):
        g = rec[i]
        if row is None or isinstance(row, soak_util.FitUnconverged) or not row[5] or not g["flags"] & F.FLAG_CORR:
            continue
        assert abs(g["corr_offset"] - row[7]) <= 5e-6 + per_bin * abs(g["carrier_offset"] - row[2]), (i, g, row)


def engine(r, tpls=None, **kw):
    tp = template(r["w"]) if tpls is None else tpls
    return F.Engine(r["n"], r["h"], tp, THR, cwin_of(r["n"]), xthr_of(r), **kw)


def c64(blocks):
    return np.stack([onp.iq_u8_to_c64(b) for b in blocks])


def found_peaks(rec):
    return set(rec["corr_sample"][(rec["flags"] & F.FLAG_CORR) != 0].tolist())


# ---------------------------------------------------------------------------------------------
# (a) long blocks
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=[row_id(r) for r in ROWS])
def test_the_engine_reports_the_form_of_the_row(r):
    eng = engine(r, max_batch=8)
    info = eng.path_info()
    assert info["correlate_kernel"] == r["form"], (row_id(r), info)
    assert info["why_unsectioned"] == r["why"], (row_id(r), info)
    assert eng.sections() == ((r["nsec"], M) if r["nsec"] else (0, 0)), row_id(r)
    assert eng.correlate_geom() == r["geom"] and info["rows"] == r["geom"], (row_id(r), info)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("r", LONG, ids=LONG_IDS)
def test_long_records_at_the_window_edges_and_seams_equal_the_oracle(r, cases):
    d = cases[row_id(r)]
    blocks, rows = d["blocks"], d["oracle"][0]
    nb = len(blocks)
    eng = engine(r, max_batch=128)
    rec = eng.detect(blocks, np.arange(nb))[:, 0]
    check_against_oracle(rec, rows, blocks, per_bin=corr_off_per_bin(r))
    rc = eng.detect(c64(blocks), np.arange(nb))[:, 0]
    check_against_oracle(rc, rows, blocks, per_bin=corr_off_per_bin(r))
    eng.close()
    assert (d["kinds"] == 0).sum() >= 2 and (d["kinds"] == 2).sum() >= 2
    assert np.array_equal((rec["flags"] & F.FLAG_CARRIER) != 0, d["kinds"] == 1)
    found = found_peaks(rec)
    lo, hi = r["win"]
    assert {lo, hi - 1} <= found, (lo, hi)
    for s in seams(plan_restated(r["n"], r["h"], r["w"])) if r["form"] == SEG else []:
        assert {s - 1, s} & set(range(lo, hi)) <= found, s
    if r.get("lag0"):
        assert 0 in found
    if r.get("last"):
        assert r["n"] - r["w"] in found


@pytest.mark.gpu
@pytest.mark.parametrize("r", LONG, ids=LONG_IDS)
def test_long_paths_agree(r, cases):
    """The window test in every row (generic_rows): byte for byte; the unsectioned kernels: exact
    fields, float fields to float32 rounding."""
    blocks = cases[row_id(r)]["blocks"]
    nb = len(blocks)
    eng, gen, uns = engine(r, max_batch=128), engine(r, max_batch=128, path="generic_rows"), \
        engine(r, max_batch=128, path="unsectioned")
    assert gen.correlate_geom() == GENERIC and gen.sections() == eng.sections()
    assert uns.sections() == (0, 0) and uns.path_info()["correlate_kernel"] == SUB
    for data in (blocks, c64(blocks)):
        rec = eng.detect(data, np.arange(nb))[:, 0]
        assert gen.detect(data, np.arange(nb))[:, 0].tobytes() == rec.tobytes()
        ref = uns.detect(data, np.arange(nb))[:, 0]
        _close(rec, ref, (ref["flags"] & F.FLAG_CORR) != 0)
        assert ((ref["flags"] & F.FLAG_CORR) != 0).sum() >= nb // 2
    for e in (eng, gen, uns):
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rid", T4_IDS)
def test_long_rows_with_four_templates_equal_the_oracle_per_template(rid, cases):
    r = LONG[LONG_IDS.index(rid)]
    d = cases[(rid, 4)]
    blocks, nb = d["blocks"], len(d["blocks"])
    tpls = np.stack([template(r["w"], k) for k in range(4)])
    eng = engine(r, tpls, max_batch=128)
    assert eng.path_info()["correlate_kernel"] == SEG and eng.correlate_geom() == r["geom"]
    rec = eng.detect(blocks, np.arange(nb))
    assert rec.shape == (nb, 4)
    gen = engine(r, tpls, max_batch=128, path="generic_rows")
    assert gen.detect(blocks, np.arange(nb)).tobytes() == rec.tobytes()
    for t in range(4):
        assert np.array_equal(rec[:, t]["template_id"], np.full(nb, t))
        check_against_oracle(rec[:, t], d["oracle"][t], blocks, per_bin=corr_off_per_bin(r))
        # every burst is found by its own template at the lag it was put
        mine = np.flatnonzero(d["kinds"] == 1)[t::4]
        assert np.all(rec[mine, t]["flags"] & F.FLAG_CORR)
        lags = np.array(d["lags"][t::4])
        inside = (lags >= r["win"][0]) & (lags < r["win"][1])
        assert inside.sum() >= 4 and rec[mine, t]["corr_sample"][inside].tolist() == lags[inside].tolist()
    for e in (eng, gen):
        e.close()


# ---------------------------------------------------------------------------------------------
# (b) the k_correlate_sub schedule
# ---------------------------------------------------------------------------------------------
def sched_counts(n, n_cu):
    chunk = min(SCHED_BATCH, long_chunk_blocks(n, SCHED_T))
    fused_grid = min(SCHED_BATCH, n_cu)
    ps = [chunk, chunk + 1, 2 * chunk + 1, fused_grid - 1, fused_grid]
    return chunk, fused_grid, sorted(p for p in set(ps) if p <= SCHED_BATCH)


@pytest.mark.gpu
@pytest.mark.parametrize("si", range(len(SCHED)), ids=SCHED_IDS)
def test_the_two_kernel_chunks_and_the_fused_switch_equal_small_batches(si, cases):
    """k_correlate_sub + k_combine run in chunks of long_chunk work-list slots (slot_base > 0 from
    the second chunk on) while a batch has fewer carrier-positive blocks than fused_grid, the fused
    kernel from there.  The same arithmetic, so every batch must equal batches of three blocks (the
    form the oracle tests pin) byte for byte; the distinct blocks are checked against the oracle."""
    import torch
    n, h, w, path = SCHED[si]
    sid = SCHED_IDS[si]
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    chunk, fused_grid, ps = sched_counts(n, n_cu)
    if si == 0:
        assert chunk == 64 and [p for p in ps if p < fused_grid][:3] == [64, 65, 129]
    if si == 1:
        assert chunk == 128 and [p for p in ps if p < fused_grid][:2] == [128, 129]
    assert ps[-2:] == [fused_grid - 1, fused_grid], (ps, n_cu)
    d = cases[sid]
    distinct = d["blocks"]
    tpls = sched_tpls(w)
    big = F.Engine(n, h, tpls, THR, (7, 110), THR, max_batch=SCHED_BATCH, path=path)
    small = F.Engine(n, h, tpls, THR, (7, 110), THR, max_batch=3, path=path)
    assert big.path_info()["correlate_kernel"] == SUB and big.sections() == (0, 0)
    if path == "auto":
        assert big.path_info()["why_unsectioned"] == "geometry"
    chunks_seen = set()
    for p in ps:
        order = sched_order(n, w, p)
        idx = order + 1000
        rec = big.detect(distinct[order], idx)
        assert int(((rec[:, 0]["flags"] & F.FLAG_CARRIER) != 0).sum()) == p, p
        chunks_seen.add(-(-p // chunk) if p < fused_grid else "fused")
        assert rec.tobytes() == small.detect(distinct[order], idx).tobytes(), p
        # every copy of a distinct block gives the same records
        present = np.unique(order)
        first = np.array([int(np.flatnonzero(order == j)[0]) for j in present])
        where = np.searchsorted(present, order)
        assert rec[first][where].tobytes() == rec.tobytes(), p
        for t in range(SCHED_T):
            rows = [d["oracle"][t][j] for j in present]
            check_against_oracle(rec[first, t], rows, distinct[present])
    assert {1, 2, "fused"} <= chunks_seen and (si == 1 or 3 in chunks_seen), chunks_seen
    # the positive distinct blocks are detected by their own template
    rec = big.detect(distinct[:SCHED_POS], np.arange(SCHED_POS))
    assert all(rec[j, j % SCHED_T]["flags"] & F.FLAG_CORR for j in range(SCHED_POS))
    for e in (big, small):
        e.close()


@pytest.mark.gpu
def test_stage_dumps_of_a_sparse_multi_chunk_batch_equal_the_oracle():
    """The dump forms of k_correlate_sub and k_combine, three chunks of the two-kernel form: the
    shifted spectrum and the correlation of blocks spread over the batch, for a template other than
    the first."""
    n, h, w, path = SCHED[0]
    tpls = sched_tpls(w)
    distinct = sched_blocks(n, h, w)
    p = 2 * long_chunk_blocks(n, SCHED_T) + 1
    order = sched_order(n, w, p)
    eng = F.Engine(n, h, tpls, THR, (7, 110), THR, max_batch=SCHED_BATCH, path=path)
    rec = eng.detect(distinct[order], np.arange(SCHED_BATCH))
    pos = np.flatnonzero(order < SCHED_POS)
    assert len(pos) == p == int(((rec[:, 0]["flags"] & F.FLAG_CARRIER) != 0).sum())
    xhat, corr = eng.debug_stage(distinct[order], template_id=1)
    eng.close()
    orc = onp.OracleDetector(n, h, list(tpls), THR, (7, 110), THR)
    bank = onp.TemplateBank(tpls[1], n, h)
    mine = [i for i in pos if order[i] % SCHED_T == 1]      # (blocks that carry template 1)
    for i in (mine[0], mine[1], mine[len(mine) // 2], mine[-1]):
        (res, data) = orc.detect_u8(0, distinct[order[i]], want_data=True)
        assert rec[i, 1]["carrier_bin"] == res[1].carrier.bin and rec[i, 1]["corr_sample"] == res[1].corr.sample
        assert abs(rec[i, 1]["carrier_offset"] - res[1].carrier.offset) <= 2e-4
        # the float32 fit parts from the oracle's by ~1e-5 bins, a phase ramp of +-pi 1e-5 across the
        # block: the dumps are pinned to float64 transforms of the block shifted by the record's OWN
        # carrier estimate, and to the oracle's (fit and all) to the fit's precision
        x = onp.iq_u8_to_c64(distinct[order[i]]).astype(np.complex128)
        xh = onp.shift_and_fft(x, -(float(rec[i, 1]["carrier_bin"]) + float(rec[i, 1]["carrier_offset"])))
        co = onp.despread(xh, bank)
        assert np.linalg.norm(xhat[i] - xh) / np.linalg.norm(xh) < 5e-6
        assert np.linalg.norm(corr[i][:len(co)] - co) / np.linalg.norm(co) < 5e-6
        xh_o, co_o = data[1]
        assert np.linalg.norm(xhat[i] - xh_o) / np.linalg.norm(xh_o) < 1e-4
        assert np.linalg.norm(corr[i][:len(co_o)] - co_o) / np.linalg.norm(co_o) < 1e-4


# ---------------------------------------------------------------------------------------------
# (c) short blocks, (d) multi-pass block lengths
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("r", SHORT + MULTIPASS, ids=SHORT_IDS + [row_id(r) for r in MULTIPASS])
def test_short_and_multi_pass_records_at_the_window_edges_equal_the_oracle(r, cases):
    d = cases[row_id(r)]
    blocks, rows = d["blocks"], d["oracle"][0]
    nb = len(blocks)
    eng = engine(r, max_batch=256)
    rec = eng.detect(blocks, np.arange(nb))[:, 0]
    eng.close()
    check_against_oracle(rec, rows, blocks, only=d["kinds"] == 1)
    assert np.array_equal((rec["flags"] & F.FLAG_CARRIER) != 0, d["kinds"] == 1)
    lo, hi = r["win"]
    found = found_peaks(rec)
    assert {lo, hi - 1} <= found, (lo, hi)
    if r.get("lag0"):
        assert {0, r["n"] - r["w"]} <= found
    if r["form"] == SMALL:
        # an odd count of carrier-positive blocks: the last group of 16 / R1 is partly filled
        assert int(((rec["flags"] & F.FLAG_CARRIER) != 0).sum()) % 2 == 1
        assert {b for k in range(1, r["n"] // 1024) for b in (1024 * k - 1, 1024 * k) if lo <= b < hi} <= found
        slow = engine(r, max_batch=256, path="multipass")
        ref = slow.detect(blocks, np.arange(nb))[:, 0]
        slow.close()
        for f in ("flags", "carrier_bin", "corr_sample"):
            assert np.array_equal(rec[f], ref[f]), f
