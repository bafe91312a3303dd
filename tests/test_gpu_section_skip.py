"""k_correlate_4k's skip rule (csrc/detect16k_sec.hip): a section whose energy
bound (1 + 2^-7) * sum |x|^2 * sum t^2 lies below a peak already found in the same block is not
transformed.  The records must stay what the form that transforms every section gives
(path="generic_rows"), byte for byte, on plain synthetic blocks and on blocks built against the rule;
the number of skipped sections must lie between what the rule gives in float64 with margins 2^-6 and
2^-8, and be a real share of the work.

The exact-tie case (two identical copies of the burst in sections 0 and 3): the two peaks are equal in
exact arithmetic, but the sections' shift phasors differ, so in float32 -- and in the oracle's float64 --
they differ by rounding and the rounding decides which lag np.argmax takes.  What is asserted there: the
skipping engine equals the generic one byte for byte (section 3 is searched, k_finish's strict > keeps
the lowest lag of equal powers), the sample is one of the two lags, and it is the oracle's unless the
oracle's own two magnitudes agree to the 3e-6 the suite allows corr_energy (an inherent tie, as
soak_util.compare treats carrier bins)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import soak_util  # noqa: E402
from oracle import thrifty_np as onp  # noqa: E402
from thrifty_amd import _native as F  # noqa: E402
from thrifty_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

N, H, W = 16384, 4096, 1023
THR = (0, 15, 0)
CWIN = (7, 110)
NB = 768          # ticket mode needs more than 2 x 1024 items: more than 512 carrier-positive blocks
NB_SMALL = 64     # 256 items: single-section tickets, nothing may be skipped
PER_CASE = 8
AMP, SIGMA = 0.3, 0.02


def _burst(z, tpl, p, car, amp=AMP):
    n = np.arange(W)
    z[p:p + W] += amp * (tpl + 1) / 2 * np.exp(2j * np.pi * car * (n + p) / N)


def _noise(rng, sigma=SIGMA):
    return rng.normal(0, sigma, N) + 1j * rng.normal(0, sigma, N)


def _adversarial(rng, tpl, secs, lo, hi):
    """-> (u8 blocks, {case: slice}, tie positions).  Float samples are edited before quantising."""
    out, where, k = [], {}, 0

    def case(name, zs):
        nonlocal k
        assert len(zs) >= PER_CASE
        out.extend(synth.quantise_iq(z) for z in zs)
        where[name] = slice(k, k + len(zs))
        k += len(zs)

    cars = rng.uniform(12.0, 100.0, 64)
    ci = iter(cars)

    def one(p, car=None):
        z = _noise(rng)
        _burst(z, tpl, int(p), next(ci) if car is None else car)
        return z

    first = [s["win_lo"] for s in secs]
    last = [s["win_hi"] - 1 for s in secs]
    case("first_owned_lag", [one(p) for p in first * 2])
    case("last_owned_lag", [one(p) for p in last * 2])
    case("window_edges", [one(p) for p in [lo, hi - 1] * 4])
    # the burst's 1023 samples inside the 1024 samples two sections share: [start of g + 1, start of g + 4096)
    inside = [secs[g + 1]["start"] + d for g in range(3) for d in (0, 1)]
    assert all(secs[g]["start"] + 4096 - secs[g + 1]["start"] == 1024 for g in range(3))
    case("inside_the_overlap", [one(p) for p in inside + inside[:2]])
    # two copies, equal amplitude, the same place in sections 0 and 3.  Four blocks without noise and with a
    # carrier for which the two copies are the same bytes (car * 9216 / N whole), four with noise
    d0 = 700
    p0, p3 = secs[0]["start"] + d0, secs[3]["start"] + d0
    assert p3 - p0 == 9216 and secs[0]["win_lo"] <= p0 < secs[0]["win_hi"] and secs[3]["win_lo"] <= p3 < secs[3]["win_hi"]
    ties = []
    for j in range(PER_CASE):
        z = np.zeros(N, dtype=complex) if j < 4 else _noise(rng)
        car = 16.0 * (1 + j) if j < 4 else next(ci)
        _burst(z, tpl, p0, car)
        _burst(z, tpl, p3, car)
        ties.append(z)
    case("two_equal_copies", ties)
    # a burst in one end section and, in the other, a carrier segment without the code of 4 x the burst's
    # energy (0.3^2 x 2048 against 0.3^2 / ... x 512 ones): its section's bound is large, its peak is not
    seg = []
    for j in range(PER_CASE + 4):
        burst_sec, tone_sec = (3, 0) if j < PER_CASE else (0, 3)
        car = next(ci)
        z = _noise(rng)
        _burst(z, tpl, secs[burst_sec]["win_lo"] + 300 + 150 * j, car)
        a = secs[tone_sec]["start"] + 600
        z[a:a + 2048] += AMP * np.exp(2j * np.pi * car * np.arange(a, a + 2048) / N)
        seg.append(z)
    assert AMP ** 2 * 2048 >= 4 * np.sum((AMP * (tpl + 1) / 2) ** 2)
    case("uncoded_segment", seg)
    # section 0 only: the burst ends in front of section 1's first sample
    p_max = secs[1]["start"] - W
    case("section_0_only", [one(p) for p in rng.integers(secs[0]["win_lo"], p_max, PER_CASE)])
    # a carrier without the code: 1500 samples of it (a tone over the whole block leaves the carrier stage's
    # noise estimate without a value and never reaches the correlate stage)
    tones = []
    for a in rng.integers(lo, hi - 1500, PER_CASE):
        z = _noise(rng)
        z[a:a + 1500] += 0.2 * np.exp(2j * np.pi * next(ci) * np.arange(a, a + 1500) / N)
        tones.append(z)
    case("tone_without_code", tones)
    return np.stack(out), where, (p0, p3)


def _simulate(blocks, rec, bank, secs):
    """The rule in float64: per carrier-positive block the sections' energies and peak powers (the
    oracle's correlation at the engine's own carrier estimate), natural order -> sections skipped with
    margins 2^-6 / 2^-8, and per block with 2^-7."""
    s_lo = s_hi = 0
    per_block = np.zeros(len(blocks), dtype=int)
    for i in np.flatnonzero((rec["flags"] & F.FLAG_CARRIER) != 0):
        x = onp.iq_u8_to_c64(blocks[i]).astype(np.complex128)
        xhat = onp.shift_and_fft(x, -(np.int64(rec["carrier_bin"][i]) + np.float64(rec["carrier_offset"][i])))
        p2 = np.abs(onp.despread(xhat, bank)) ** 2
        e = np.abs(x) ** 2
        best = 0.0
        for g, s in enumerate(secs):
            bound = e[s["start"]:s["start"] + 4096].sum() * bank.energy
            if g > 0:
                s_lo += (1 + 2.0 ** -6) * bound < best
                s_hi += (1 + 2.0 ** -8) * bound < best
                per_block[i] += (1 + 2.0 ** -7) * bound < best
            best = max(best, p2[s["win_lo"]:s["win_hi"]].max())
    return s_lo, s_hi, per_block


@pytest.fixture(scope="module")
def run():
    rng = np.random.default_rng(20261019)
    tpl = synth.gold_template(10, 2)
    lo, hi = onp.unique_window(N, H, W)
    secs = F.plan_sections(N, H, W)
    assert len(secs) == 4
    adv, where, tie_pos = _adversarial(rng, tpl, secs, lo, hi)
    plain, _ = synth.synth_blocks(rng, NB - len(adv), N, tpl, (lo, hi))
    blocks = np.concatenate([adv, plain])
    assert len(blocks) == NB and len(plain) >= 512
    out = dict(blocks=blocks, where=where, tie_pos=tie_pos, n_adv=len(adv), secs=secs, tpl=tpl)
    for name, nb in (("big", NB), ("small", NB_SMALL)):
        eng = F.Engine(N, H, tpl, THR, CWIN, THR, max_batch=nb)
        gen = F.Engine(N, H, tpl, THR, CWIN, THR, max_batch=nb, path="generic_rows")
        assert eng.sections() == (4, 4096) and gen.sections() == (4, 4096)
        assert eng.section_counts() == (0, 0)
        out[name] = eng.detect(blocks[:nb], np.arange(nb))[:, 0].copy()
        out[name + "_counts"] = eng.section_counts()
        assert eng.section_counts() == (0, 0)       # read and zeroed
        out[name + "_generic"] = gen.detect(blocks[:nb], np.arange(nb))[:, 0].copy()
        out[name + "_generic_counts"] = gen.section_counts()
        if name == "big":
            # the same blocks as complex64 (the energy is a float32 sum there), resident on the device: the
            # host entry stages complex64 input in chunks of 512 blocks, which are single-section tickets
            import torch
            dev = torch.device("cuda")
            c64 = torch.from_numpy(((blocks.astype(np.float32) - 127.4) / 128).view(np.complex64)).to(dev)
            idx = torch.arange(nb, dtype=torch.int64, device=dev)
            d_out = torch.zeros((2, nb, 64), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            for k, e in enumerate((eng, gen)):
                e.detect_device(c64.data_ptr(), F.THR_IN_C64, nb, d_out[k].data_ptr(), idx.data_ptr())
                e.sync()
            out["c64_counts"] = eng.section_counts()
            out["c64"], out["c64_generic"] = (d_out[k].cpu().numpy().view(F.RECORD_DTYPE).reshape(-1) for k in range(2))
        eng.close()
        gen.close()
    return out


def test_records_equal_the_form_that_transforms_every_section(run):
    for name, nb in (("big", NB), ("small", NB_SMALL)):
        rec, ref = run[name], run[name + "_generic"]
        assert rec.dtype.itemsize == 64 and len(rec) == nb
        positive = int(((rec["flags"] & F.FLAG_CARRIER) != 0).sum())
        assert positive == nb                       # every block reaches the correlate stage
        diff = np.flatnonzero((rec.view(np.uint8).reshape(nb, 64) != ref.view(np.uint8).reshape(nb, 64)).any(axis=1))
        assert diff.size == 0, (name, diff[:8], rec[diff[:2]], ref[diff[:2]])
        assert rec.tobytes() == ref.tobytes()
        done, skipped = run[name + "_counts"]
        print(name, "computed", done, "skipped", skipped)
        assert done + skipped == 4 * positive
        assert run[name + "_generic_counts"] == (4 * positive, 0)    # the cross-check form skips nothing
    assert run["small_counts"] == (4 * NB_SMALL, 0)                   # single-section tickets
    assert run["big_counts"][1] > 0


def test_adversarial_blocks_equal_the_oracle(run):
    n_adv, blocks, rec, where = run["n_adv"], run["blocks"], run["big"], run["where"]
    omp = os.environ.get("OMP_NUM_THREADS")     # (oracle_rows is written for worker processes and sets it)
    try:
        _, rows = soak_util.oracle_rows((0, blocks[:n_adv], N, H, run["tpl"], THR, CWIN, THR))
    finally:
        os.environ.pop("OMP_NUM_THREADS", None)
        if omp is not None:
            os.environ["OMP_NUM_THREADS"] = omp
    tie = where["two_equal_copies"]
    only = np.ones(n_adv, dtype=bool)
    only[tie] = False
    # (the tie blocks' rows are checked below: compare() counts a sample on the other copy as a mismatch)
    strict = [i for i in range(n_adv) if only[i]]
    mism, worst, ties = soak_util.compare(rec[strict], [rows[i] for i in strict], blocks[strict], F.FLAG_CARRIER, F.FLAG_CORR)
    print("oracle:", mism, worst, ties)
    assert mism == dict(bin=0, carrier=0, sample=0, det=0, index_error=0), (mism, worst)
    assert not ties
    assert worst["offset"] <= 5e-6 and worst["energy"] <= 2e-5 and worst["noise"] <= 2e-5, worst
    det = (rec["flags"] & F.FLAG_CORR) != 0
    secs = run["secs"]
    lo, hi = onp.unique_window(N, H, W)
    for name in ("first_owned_lag", "last_owned_lag", "window_edges", "inside_the_overlap", "section_0_only"):
        assert det[where[name]].all(), name
    found = set(rec["corr_sample"][:n_adv][det[:n_adv]].tolist())
    assert {s["win_lo"] for s in secs} | {s["win_hi"] - 1 for s in secs} | {lo, hi - 1} <= found
    assert {secs[g + 1]["start"] + d for g in range(3) for d in (0, 1)} <= found
    # the uncoded segment's section is searched and does not win: the burst's lag is found
    seg = where["uncoded_segment"]
    assert det[seg].all()
    for j, i in enumerate(range(seg.start, seg.stop)):
        burst_sec = 3 if j < PER_CASE else 0
        assert rec["corr_sample"][i] == secs[burst_sec]["win_lo"] + 300 + 150 * j
    assert not det[where["tone_without_code"]].any()
    # two equal copies
    p0, p3 = run["tie_pos"]
    bank = onp.TemplateBank(run["tpl"], N, H)
    for i in range(tie.start, tie.stop):
        row = rows[i]
        assert row is not None and not isinstance(row, soak_util.FitUnconverged)
        assert bool(rec["flags"][i] & F.FLAG_CORR) and row[5]
        assert rec["corr_sample"][i] in (p0, p3)
        if rec["corr_sample"][i] != row[4]:
            x = onp.iq_u8_to_c64(blocks[i])
            mag = np.abs(onp.despread(onp.shift_and_fft(x, -(np.int64(row[0]) + row[2])), bank))
            print("tie block", i, "engine", rec["corr_sample"][i], "oracle", row[4], mag[p0], mag[p3])
            assert abs(mag[p0] - mag[p3]) <= 3e-6 * max(mag[p0], mag[p3])
        else:
            assert abs(rec["corr_energy"][i] - row[6]) <= 2e-5 * row[6]


def test_the_skipping_is_real_and_bounded(run):
    rec, secs = run["big"], run["secs"]
    bank = onp.TemplateBank(run["tpl"], N, H)
    s_lo, s_hi, per_block = _simulate(run["blocks"], rec, bank, secs)
    done, skipped = run["big_counts"]
    positive = int(((rec["flags"] & F.FLAG_CARRIER) != 0).sum())
    plain = per_block[run["n_adv"]:]
    print("skipped", skipped, "bounds", s_lo, s_hi, "plain share %.4f" % (plain.sum() / (4.0 * len(plain))))
    assert s_lo <= skipped <= s_hi
    assert done + skipped == 4 * positive
    # the plain synthetic part: a condition, not a measurement (the rule's float64 model on 600 such blocks: 33.6 %).
    # The engine's own count there is the total less the adversarial part's, which the margins bracket
    adv_lo, adv_hi, _ = _simulate(run["blocks"][:run["n_adv"]], rec[:run["n_adv"]], bank, secs)
    assert len(plain) >= 512
    assert skipped - adv_hi >= 0.25 * 4 * len(plain), (skipped, adv_hi)
    # a burst in section 0 only: sections 1 .. 3 go
    assert (per_block[run["where"]["section_0_only"]] == 3).all()


def test_complex64_input_skips_the_same_way(run):
    rec, ref = run["c64"], run["c64_generic"]
    assert rec.tobytes() == ref.tobytes()
    positive = int(((rec["flags"] & F.FLAG_CARRIER) != 0).sum())
    done, skipped = run["c64_counts"]
    s_lo, s_hi, _ = _simulate(run["blocks"], rec, onp.TemplateBank(run["tpl"], N, H), run["secs"])
    print("complex64: computed", done, "skipped", skipped, "bounds", s_lo, s_hi)
    assert positive == NB and done + skipped == 4 * positive
    assert s_lo <= skipped <= s_hi
