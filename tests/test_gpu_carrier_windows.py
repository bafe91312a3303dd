"""The carrier stage at its selection boundaries.  The handle picks one of about ten carrier kernel
forms from the block length, the carrier window (win_lo, count of window_indices) and the stddev
term: handle.hip (car_prune), detect16k_carrier.hip, long_carrier_form (detect_common.hpp).  Every
row of the table below sits exactly on one side of one boundary of that rule (or on an edge of the
spectrum: a wrapping window, bin 0, bin N - 1, a window of N bins) and names the kernel it must
select.  Carriers are planted on, just inside and just outside each window edge, and on bins 0 .. 2
and -1 .. -4 where the window holds them (the reference's quirks: a wrapping window whose argmax is
bin 0 reports bin N and raises IndexError, peak + 3 >= N raises, negative fit neighbours wrap).

  (a) the engine reports the form the rule names (Engine.path_info)
  (b) without a GPU: each row sits on the boundary it claims, and the rule names its kernel
  (c) every record against the CPU oracle, u8 and complex64 input
  (d) the multi-pass pipeline gives the same bins, flags and energies
  (e) carrier_len W / 2 and 2 W against the oracle with the same carrier_len"""
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

# block_len -> (history, Gold register bits, samples per chip).  W >= N / 12, so that carrier_len
# W / 2 and 2 W both keep N / carrier_len <= 24, where the Dirichlet fit is well conditioned
# (DESIGN.md section 4).
GEOMETRY = {256: (64, 5, 1.0), 1024: (256, 7, 1.0), 4096: (1024, 9, 1.0), 8192: (2048, 10, 1.0),
            16384: (4096, 11, 1.0), 32768: (8192, 11, 2.0), 65536: (8192, 11, 3.0),
            131072: (16384, 11, 6.0)}
THR, THR_STD = (0, 15, 0), (0, 12, 1.0)
PRESHIFT_NUM = 21

PRUNED, SHIFTED, FULL = "k_carrier_pruned", "k_carrier_pruned (pre-shifted window)", "k_carrier"
DIT, SUB_PRUNED, SUB = "k_carrier_dit+k_select_dit", "k_carrier_sub_pruned+k_select", "k_carrier_sub+k_select"
SMALL, MULTI, PRESHIFT = "k_carrier_small", "g_* (multi-pass)", "k_preshift"


def window(n, win):
    """(win_lo, count, end): the FFT index the window starts at, its bins (clamped to N, as
    window_indices in handle.hip does) and the end of the window + fit margin, win_lo + count + 3."""
    lo, hi = onp.window_to_indices(win[0], win[1], n)
    count = min(hi - lo + 1, n)
    return lo, count, lo + count + 3


def carrier_form(n, lo, count, std, preshift=0):
    """The selection rule, as stated for the kernels' users: which carrier kernel a default-path
    engine of this geometry runs."""
    if preshift:
        return PRESHIFT if n == 16384 else MULTI
    prune = not std and lo >= 3
    if n == 16384:
        if prune and lo + count + 3 <= 128:
            return PRUNED
        return SHIFTED if not std and count + 6 <= 128 else FULL
    if n in (32768, 65536):
        if prune and lo + count + 3 <= 128:
            return DIT
        return SUB_PRUNED if prune and lo + count + 3 <= 128 * (n // 16384) else SUB
    return SMALL if n in (1024, 2048, 4096, 8192) else MULTI


def _rows():
    rows = []

    def add(n, win, form, edge=None, std=False, pre=0):
        # edge: (quantity, its value on this row, step, the form one step across) or None
        rows.append(dict(n=n, win=win, std=std, pre=pre, form=form, edge=edge))

    n = 16384
    add(n, (3, 110), PRUNED, ("win_lo", 3, -1, SHIFTED))
    add(n, (2, 110), SHIFTED, ("win_lo", 2, +1, PRUNED))
    add(n, (5, 124), PRUNED, ("end", 128, +1, SHIFTED))
    add(n, (5, 125), SHIFTED, ("end", 129, -1, PRUNED))
    add(n, (200, 321), SHIFTED, ("count", 122, +1, FULL))
    add(n, (200, 322), FULL, ("count", 123, -1, SHIFTED))
    for win in ((0, 100), (1, 100), (-1, 100), (-60, 61)):      # the pre-shift base win_lo - 3 wraps
        add(n, win, SHIFTED, ("win_lo", window(n, win)[0], None, None))
    add(n, (-20, -1), SHIFTED)                                  # the top of the spectrum
    add(n, (0, -1), FULL)                                       # ALLBINS
    add(n, (1, -1), FULL)                                       # windowed, N - 1 bins
    add(n, (-(n - 1), n - 1), FULL)                             # 2N - 1 bins from win_lo 1: clamped to N
    add(n, (7, 110), FULL, std=True)                            # stddev term: no pruning
    for n in (32768, 65536):
        span = 128 * (n // 16384)
        add(n, (3, 110), DIT, ("win_lo", 3, -1, SUB))
        add(n, (2, 110), SUB, ("win_lo", 2, +1, DIT))            # (no mode 2 on long blocks)
        add(n, (5, 124), DIT, ("end", 128, +1, SUB_PRUNED))
        add(n, (5, 125), SUB_PRUNED, ("end", 129, -1, DIT))
        add(n, (5, span - 4), SUB_PRUNED, ("end", span, +1, SUB))
        add(n, (5, span - 3), SUB, ("end", span + 1, -1, SUB_PRUNED))
        add(n, (-10, 10), SUB)
        add(n, (-20, -1), SUB)
        add(n, (0, -1), SUB, std=True)
        add(n, (-(n // 2 - 1), n // 2 - 3), SUB, ("count", n - 3, None, None))   # k_select's win_w clamped to N
    add(65536, (300, 400), SUB_PRUNED)                          # starts above bin 128
    for n in (1024, 4096, 8192, 256, 131072):
        form = SMALL if 1024 <= n <= 8192 else MULTI
        for win in ((-10, 10), (-20, -1), (1, -1), (-(n - 1), n - 1), (5, n // 10), (-(n // 6), -(n // 12))):
            add(n, win, form)
        add(n, (0, -1), form, std=True)
    for win in ((-12, 12), (-20, -1), (2, 110), (200, 322)):
        add(16384, win, PRESHIFT, pre=PRESHIFT_NUM)
    return rows


ROWS = _rows()


def row_id(r):
    return "%d_%d_%d%s%s" % (r["n"], r["win"][0], r["win"][1], "_std" if r["std"] else "",
                             "_preshift" if r["pre"] else "")


IDS = [row_id(r) for r in ROWS]
# one row per kernel form for the carrier_len variants
CL_ROWS = [r for r in ROWS if row_id(r) in (
    "16384_3_110", "16384_2_110", "16384_200_322", "16384_0_-1", "32768_3_110", "65536_5_508",
    "32768_2_110", "65536_0_-1_std", "4096_-10_10", "1024_0_-1_std", "256_-10_10", "131072_-20_-1")]


# ---------------------------------------------------------------------------------------------
# (b) the table itself (no GPU)
# ---------------------------------------------------------------------------------------------
def test_every_row_sits_on_the_boundary_it_claims():
    assert len(set(IDS)) == len(IDS)
    assert {r["form"] for r in ROWS} == {PRUNED, SHIFTED, FULL, DIT, SUB_PRUNED, SUB, SMALL, MULTI, PRESHIFT}
    assert len(CL_ROWS) == 12 and {r["form"] for r in CL_ROWS} == {
        PRUNED, SHIFTED, FULL, DIT, SUB_PRUNED, SUB, SMALL, MULTI}
    for r in ROWS:
        n = r["n"]
        lo, count, end = window(n, r["win"])
        assert carrier_form(n, lo, count, r["std"], r["pre"]) == r["form"], r
        if r["edge"] is None:
            continue
        qty, value, step, across = r["edge"]
        assert {"win_lo": lo, "count": count, "end": end}[qty] == value, (r, lo, count, end)
        if step is None:
            continue
        # one step across the boundary selects the other form: the row is ON the boundary
        lo2, count2 = (lo + step, count) if qty == "win_lo" else (lo, count + step)
        assert carrier_form(n, lo2, count2, r["std"], r["pre"]) == across, r
    # the rows the issue names by geometry
    w = {row_id(r): window(r["n"], r["win"]) for r in ROWS}
    assert w["16384_0_-1"] == (0, 16384, 16387)
    assert w["16384_1_-1"][:2] == (1, 16383)
    assert w["16384_-16383_16383"][:2] == (1, 16384)
    assert w["16384_-60_61"][:2] == (16384 - 60, 122)
    assert w["16384_-1_100"][0] - 3 < 16384 < w["16384_-1_100"][0] + w["16384_-1_100"][1]
    for n in (32768, 65536):
        assert w["%d_%d_%d" % (n, -(n // 2 - 1), n // 2 - 3)][:2] == (n // 2 + 1, n - 3)
        assert w["%d_%d_%d" % (n, -(n // 2 - 1), n // 2 - 3)][1] + 6 > n
    assert w["65536_300_400"][0] > 128 and w["65536_300_400"][2] <= 512


# ---------------------------------------------------------------------------------------------
# blocks and the oracle
# ---------------------------------------------------------------------------------------------
def template(n):
    h, bits, sps = GEOMETRY[n]
    return h, synth.gold_template(bits, 2, sps).astype(np.float64)


def placements(n, lo, count):
    """Signed carrier bins: on, inside and outside both window edges, the middle, and bins
    0 .. 2 / -1 .. -4 where the window holds bin 0 or N - 1.  No exact half-bin offsets (the two
    bins' magnitudes would tie)."""
    hi = lo + count - 1
    bins = [lo, lo + 0.3, lo - 0.45, lo - 1.3, hi, hi - 0.3, hi + 0.45, hi + 1.3, lo + (count - 1) // 2 + 0.23]
    zero_or_top = (0 - lo) % n < count or (n - 1 - lo) % n < count
    if zero_or_top:
        bins += [0, 1, 2, -1, -2, -3, -4]
    out = []
    for b in bins:
        s = (b + n / 2) % n - n / 2          # signed, in [-N/2, N/2)
        if all(abs(s - o) > 1e-9 for o in out):
            out.append(s)
    return np.array(out), zero_or_top


def make_blocks(r):
    n = r["n"]
    h, tpl = template(n)
    lo, count, _ = window(n, r["win"])
    car, zero_or_top = placements(n, lo, count)
    rng = np.random.default_rng(zlib.crc32(row_id(r).encode()))
    # (amp 0.6 where the window holds bin 0: the carrier outweighs the u8 quantiser's DC spike)
    blocks, _ = synth.synth_blocks(rng, len(car), n, tpl, onp.unique_window(n, h, len(tpl)),
                                   signal_frac=1.0, amp=0.6 if zero_or_top else 0.3, carriers=car)
    return blocks, car


def cthr_of(r):
    return THR_STD if r["std"] else THR


@pytest.fixture(scope="module")
def cases():
    """Every row's blocks, and the oracle's records for them and for the carrier_len variants --
    one pool of 8 workers for the whole file."""
    data, configs, keys = {}, [], []
    for r in ROWS:
        blocks, car = make_blocks(r)
        h, tpl = template(r["n"])
        data[row_id(r)] = dict(blocks=blocks, car=car)
        configs.append((blocks, r["n"], h, tpl, cthr_of(r), r["win"], THR, None, r["pre"]))
        keys.append((row_id(r), None))
    for r in CL_ROWS:
        h, tpl = template(r["n"])
        for cl in (len(tpl) // 2, 2 * len(tpl)):
            configs.append((data[row_id(r)]["blocks"], r["n"], h, tpl, cthr_of(r), r["win"], THR, cl, 0))
            keys.append((row_id(r), cl))
    for (rid, cl), rows in zip(keys, soak_util.run_oracle_many(configs, procs=8, chunk=4)):
        data[rid]["oracle" if cl is None else ("oracle", cl)] = rows
    return data


def engine(r, **kw):
    h, tpl = template(r["n"])
    return F.Engine(r["n"], h, tpl, cthr_of(r), r["win"], THR, max_batch=32, preshift_num=r["pre"], **kw)


_TIES = []   # carrier-bin ties (compare's rule) over the whole file


def check_against_oracle(r, rec, rows, blocks, car, corr_off_per_bin=0.0):
    """corr_off_per_bin: allow corr_offset to move with the carrier offset's deviation (samples per
    bin), for fits the oracle itself pins less tightly (see test_carrier_len_other_than_...)."""
    n = r["n"]
    # float bounds of the fit and what follows it only where the oracle's bin is the planted
    # carrier's; elsewhere the in-window maximum may be the DC spike, whose fit is ill-conditioned
    near = np.array([row is not None and abs((row[0] - c + n / 2) % n - n / 2) <= 1.5
                     for row, c in zip(rows, car)])
    flags = (F.FLAG_CARRIER, F.FLAG_CORR, F.FLAG_INDEX_ERROR)
    mism, worst, ties = soak_util.compare(rec, rows, blocks, *flags, only=near, flag_fit=F.FLAG_FIT_UNCONVERGED)
    _, worst_all, _ = soak_util.compare(rec, rows, blocks, *flags, flag_fit=F.FLAG_FIT_UNCONVERGED)
    _TIES.extend((row_id(r), i) for i in ties)
    assert mism == dict(bin=0, carrier=0, sample=0, det=0, index_error=0), (mism, worst, ties)
    assert len(_TIES) <= 1, _TIES
    # the carrier's energy and noise do not depend on the fit: every block
    assert worst_all["car_energy"] <= 2e-5 and worst_all["car_noise"] <= 2e-5, worst_all
    # (not vacuous: the blocks that are no IndexError carry a detected carrier)
    n_det = sum(1 for row in rows if row is not None and row[1])
    assert n_det >= 4 and near.sum() >= 4, (near, rows)
    if r["pre"]:
        # (PreshiftDetector: a float32 three-point parabola and a bank of pre-shifted templates,
        # test_gpu_preshift.py's bounds)
        assert worst["car_off"] <= 1e-4 and worst["energy"] <= 1e-4 and worst["offset"] <= 1e-4, worst
    else:
        assert worst["car_off"] <= 2e-4, worst
        assert worst["energy"] <= 2e-5 and worst["noise"] <= 2e-5, worst
        if not corr_off_per_bin:
            assert worst["offset"] <= 5e-6, worst
        for i in np.flatnonzero(near):
            row, g = rows[i], rec[i]
            if isinstance(row, soak_util.FitUnconverged) or not row[5] or not g["flags"] & F.FLAG_CORR:
                continue
            bound = 5e-6 + corr_off_per_bin * abs(g["carrier_offset"] - row[2])
            assert abs(g["corr_offset"] - row[7]) <= bound, (i, g, row)


# ---------------------------------------------------------------------------------------------
# (a) selection, (c) oracle parity, (d) multi-pass, (e) carrier_len
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=IDS)
def test_the_engine_selects_the_form_of_the_row(r):
    eng = engine(r)
    assert eng.path_info()["carrier_kernel"] == r["form"], (row_id(r), eng.path_info())
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=IDS)
def test_records_at_the_window_edges_equal_the_oracle(r, cases):
    d = cases[row_id(r)]
    blocks, car, rows = d["blocks"], d["car"], d["oracle"]
    eng = engine(r)
    idx = np.arange(len(blocks))
    rec = eng.detect(blocks, idx)[:, 0]
    check_against_oracle(r, rec, rows, blocks, car)
    rec_c = eng.detect(np.stack([onp.iq_u8_to_c64(b) for b in blocks]), idx)[:, 0]
    check_against_oracle(r, rec_c, rows, blocks, car)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("r", [r for r in ROWS if r["form"] != MULTI], ids=[row_id(r) for r in ROWS if r["form"] != MULTI])
def test_the_multi_pass_pipeline_agrees(r, cases):
    blocks = cases[row_id(r)]["blocks"]
    fast_eng, slow_eng = engine(r), engine(r, path="multipass")
    assert slow_eng.path_info()["carrier_kernel"] == MULTI
    fast, slow = fast_eng.detect(blocks)[:, 0], slow_eng.detect(blocks)[:, 0]
    fast_eng.close()
    slow_eng.close()
    assert np.array_equal(fast["carrier_bin"], slow["carrier_bin"])
    assert np.array_equal(fast["flags"], slow["flags"])
    assert np.array_equal(fast["corr_sample"], slow["corr_sample"])
    np.testing.assert_allclose(fast["carrier_energy"], slow["carrier_energy"], rtol=2e-5)
    np.testing.assert_allclose(fast["carrier_noise"], slow["carrier_noise"], rtol=2e-5)
    car = (fast["flags"] & F.FLAG_CARRIER) != 0
    assert car.sum() >= 4
    np.testing.assert_allclose(fast["corr_energy"][car], slow["corr_energy"][car], rtol=2e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("factor", [0.5, 2])
@pytest.mark.parametrize("r", CL_ROWS, ids=[row_id(r) for r in CL_ROWS])
def test_carrier_len_other_than_the_template_length(r, factor, cases):
    d = cases[row_id(r)]
    _, tpl = template(r["n"])
    cl = len(tpl) // 2 if factor == 0.5 else 2 * len(tpl)
    assert r["n"] / cl <= 24
    eng = engine(r, carrier_len=cl)
    rec = eng.detect(d["blocks"], np.arange(len(d["blocks"])))[:, 0]
    eng.close()
    # With a lobe width other than the burst's the fit is pinned less tightly: the kernels' float32
    # fit and the oracle's float64 one part by up to ~6e-5 bins (inside 2e-4), and the shift carries
    # that into the correlation peak -- on the oracle alone, moving the shift by 6e-5 bins moves
    # corr_offset by up to 2.1e-5 samples (0.34 samples per bin) on these blocks.
    check_against_oracle(r, rec, d[("oracle", cl)], d["blocks"], d["car"], corr_off_per_bin=0.5)
