"""Shared by tests/test_gpu_soak.py and tests/tools/soak_parity.py: the CPU oracle spread over
worker processes (spawned -- the parent holds a HIP context), and the record comparison."""
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class FitUnconverged(tuple):
    """Oracle row of a block on which the reference's carrier fit dies: SciPy's curve_fit raises
    RuntimeError("Optimal parameters not found") and carrier_sync.py:189 does not catch it.  Row-shaped
    (the oracle's carrier bin and verdict, the rest zero) so that callers indexing rows keep working;
    compare() counts it as a carrier mismatch unless the record carries THR_FLAG_FIT_UNCONVERGED."""


def oracle_rows(args):
    """(worker) -> (lo, [(cbin, cdet, coff, cenergy, sample, det, energy, offset, noise, cnoise), ...]).
    args: (lo, blocks, n, h, tpl, cthr, cwin, xthr[, carrier_len[, preshift_num[, interpolator[,
    fastdet]]]]); carrier_len None: the template's length; preshift_num > 0: OraclePreshiftDetector
    with that many templates and that carrier interpolator (default "parabolic"), whose rows end in
    two more fields: the (int_shift, frac_shift, template index) it chose (None without a carrier)
    and whether the carrier offset is the Python int 0; fastdet true: OracleFastdet, its powers
    given as roots (the record's units), ending in (-argmax, 0.0, 0) and False."""
    os.environ["OMP_NUM_THREADS"] = "1"
    lo, blocks, n, h, tpl, cthr, cwin, xthr = args[:8]
    carrier_len = args[8] if len(args) > 8 else None
    preshift_num = args[9] if len(args) > 9 else 0
    interpolator = args[10] if len(args) > 10 else "parabolic"
    fastdet = bool(args[11]) if len(args) > 11 else False
    from oracle import thrifty_np as onp
    if fastdet:
        orc = onp.OracleFastdet(n, h, tpl, cthr, cwin, xthr)
        return lo, [_fastdet_row(orc.detect_u8(lo + i, b)) for i, b in enumerate(blocks)]
    if preshift_num:
        orc = onp.OraclePreshiftDetector(n, h, tpl, cthr, cwin, xthr, num=preshift_num, interpolator=interpolator)
    else:
        orc = onp.OracleDetector(n, h, tpl, cthr, cwin, xthr, carrier_len=carrier_len)
    out = []
    for i in range(len(blocks)):
        try:
            r = orc.detect_u8(lo + i, blocks[i])
            if not preshift_num:
                (r,) = r
        except IndexError:      # the reference raises when peak_idx + 3 >= N (carrier_sync.py:187)
            out.append(None)
            continue
        except RuntimeError:    # curve_fit gave up (carrier_sync.py:189)
            mag = np.abs(np.fft.fft(onp.iq_u8_to_c64(blocks[i])))
            det, idx, peak, noise, _ = onp.carrier_detect(mag, cthr, cwin)
            out.append(FitUnconverged((idx, bool(det), 0.0, float(peak), -1, False, 0.0, 0.0, 0.0, float(noise))))
            continue
        c = r.corr
        row = (r.carrier.bin, bool(r.carrier.detected), float(r.carrier.offset), float(r.carrier.energy),
               int(c.sample) if c else -1, bool(c.detected) if c else False,
               float(c.energy) if c else 0.0, float(c.offset) if c else 0.0,
               float(c.noise) if c else 0.0, float(r.carrier.noise))
        out.append(row + (orc.last, isinstance(r.carrier.offset, int)) if preshift_num else row)
    return lo, out


def _fastdet_row(w):
    return (w.argmax, bool(w.carrier), float(w.carrier_offset), float(np.sqrt(w.carrier_max)),
            int(w.peak_idx), bool(w.detected), float(np.sqrt(w.peak_power)), float(w.peak_offset),
            float(np.sqrt(w.noise_power)), float(np.sqrt(w.carrier_noise)),
            (-int(w.argmax), 0.0, 0) if w.carrier else None, False)


def run_oracle(blocks, n, h, tpl, cthr, cwin, xthr, procs=None, chunk=64, carrier_len=None, preshift_num=0,
               interpolator="parabolic", fastdet=False):
    return run_oracle_many([(blocks, n, h, tpl, cthr, cwin, xthr, carrier_len, preshift_num, interpolator, fastdet)],
                           procs=procs, chunk=chunk)[0]


def run_oracle_many(configs, procs=None, chunk=64):
    """Several oracle runs in one pool of workers: configs = [(blocks, n, h, tpl, cthr, cwin, xthr,
    carrier_len, preshift_num[, interpolator[, fastdet]]), ...] -> [rows of each config]."""
    procs = procs or max(1, min(32, (os.cpu_count() or 2) // 2))
    jobs, where = [], []
    for c, (blocks, *rest) in enumerate(configs):
        for s in range(0, len(blocks), chunk):
            jobs.append((s, blocks[s:s + chunk], *rest))
            where.append(c)
    out_rows = [[None] * len(c[0]) for c in configs]
    # (an executor, not mp.Pool: a worker that dies raises BrokenProcessPool instead of being
    # respawned forever, and every result has a deadline)
    from concurrent.futures import ProcessPoolExecutor
    with ProcessPoolExecutor(min(procs, len(jobs)), mp_context=mp.get_context("spawn")) as pool:
        for c, (lo, out) in zip(where, pool.map(oracle_rows, jobs, timeout=900)):
            out_rows[c][lo:lo + len(out)] = out
    return out_rows


def compare(rec, rows, blocks, flag_carrier=1, flag_corr=2, flag_index_error=4, only=None, flag_fit=16):
    """-> (mismatch counts, worst deviations, [indices of carrier-bin ties]).  Exact fields (bin,
    sample, verdicts) are counted over every block; the worst deviations only over the blocks
    where `only` (bool array) is set, when given.  A FitUnconverged row is a carrier mismatch
    unless the record carries `flag_fit`."""
    from oracle import thrifty_np as onp
    mism = dict(bin=0, carrier=0, sample=0, det=0, index_error=0)
    worst = dict(energy=0.0, offset=0.0, car_off=0.0, car_energy=0.0, noise=0.0, car_noise=0.0)
    ties = []
    for i, row in enumerate(rows):
        r = rec[i]
        if row is None or (r["flags"] & flag_index_error):
            mism["index_error"] += (row is None) != bool(r["flags"] & flag_index_error)
            continue
        if isinstance(row, FitUnconverged):
            mism["bin"] += r["carrier_bin"] != row[0]
            mism["carrier"] += not (r["flags"] & flag_fit)
            continue
        cbin, cdet, coff, cen, samp, det, en, off, noise = row[:9]
        if r["carrier_bin"] != cbin:
            # inherent tie: the two bins' float32 magnitudes are equal (to an ulp) in NumPy itself and
            # the two FFT implementations round differently -- counted apart, never silently
            mag = np.abs(np.fft.fft(onp.iq_u8_to_c64(blocks[i])))
            a, b = np.float32(mag[int(r["carrier_bin"]) % len(mag)]), np.float32(mag[cbin % len(mag)])
            if abs(a - b) <= np.spacing(max(a, b)):
                ties.append(i)
                continue
            mism["bin"] += 1
            continue
        mism["carrier"] += bool(r["flags"] & flag_carrier) != cdet
        if not cdet or bool(r["flags"] & flag_carrier) != cdet:
            continue
        mism["sample"] += r["corr_sample"] != samp
        mism["det"] += bool(r["flags"] & flag_corr) != det
        if only is not None and not only[i]:
            continue
        worst["car_energy"] = max(worst["car_energy"], abs(r["carrier_energy"] - cen) / abs(cen))
        if len(row) > 9:
            worst["car_noise"] = max(worst["car_noise"], abs(r["carrier_noise"] - row[9]) / abs(row[9]))
        worst["car_off"] = max(worst["car_off"], abs(r["carrier_offset"] - coff))
        if r["corr_sample"] == samp:
            worst["energy"] = max(worst["energy"], abs(r["corr_energy"] - en) / abs(en))
            worst["noise"] = max(worst["noise"], abs(r["corr_noise"] - noise) / abs(noise))
            if det and bool(r["flags"] & flag_corr):
                worst["offset"] = max(worst["offset"], abs(r["corr_offset"] - off))
    return mism, worst, ties
