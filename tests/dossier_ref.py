"""Plain float64 NumPy statement of the detection dossiers on the project's oracle
(oracle/thrifty_np.py: carrier stage, shift, correlation stage): the pick rule, the per-block series and
scalars, the carrier fit and the shifted correlation peak.  `dossier()` wraps the numbers in the package's
`Dossier`, so that its views can be held against the reference's recorded drawings without a GPU, and the
device's arrays against these."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import thrifty_np as onp  # noqa: E402
from thrifty_amd import toads_data  # noqa: E402
from thrifty_amd.detect import DetectorSettings  # noqa: E402

SAMPLE_RATE = 2.2e6
AUTOCORR_LAGS = 17
PEAK_WINDOW = 11


def scene_settings(g, **override):
    """DetectorSettings of a committed scene fixture (tests/golden/<scene>.npz)."""
    tpl = np.asarray(g["template"], dtype=np.float64)
    s = DetectorSettings(int(g["block_len"]), int(g["history_len"]), len(tpl), tuple(float(v) for v in g["carrier_thresh"]),
                         tuple(int(v) for v in g["carrier_window"]), tpl, tuple(float(v) for v in g["corr_thresh"]))
    return s._replace(**override)


def in_ranges(block_idx, ranges):
    return any((lo is None or block_idx >= lo) and (hi is None or block_idx <= hi) for lo, hi in ranges)


def pick(block_idx, detected, ranges, max_keep):
    """The pick rule -> (positions kept, n_checked, n_skipped, the lines the reference's loop prints)."""
    kept, lines, checked, skipped = [], [], 0, 0
    for pos, (idx, det) in enumerate(zip(block_idx, detected)):
        if len(kept) >= max_keep:
            break
        if not in_ranges(int(idx), ranges):
            continue
        checked += 1
        lines.append("Checking block #{}".format(int(idx)))
        if det:
            kept.append(pos)
        else:
            skipped += 1
            lines.append("Skipping block #{}".format(int(idx)))
    return kept, checked, skipped, lines


def filter_weights2(n, w):
    """Squared unit-energy Dirichlet weights of F + 1 taps, F = 2 * (n // w) -> (F, weights^2)."""
    f = 2 * (n // w)
    c = onp.dirichlet(np.arange(-(f // 2), f // 2 + 1), n, w)
    return f, (c / np.sqrt(np.sum(c ** 2))) ** 2


def filtered_spectrum(mag, n, w):
    """sqrt(sum_j w_j^2 m[i + j]^2), j = -F/2 .. F/2, m = 0 below bin 0, for i < n - F/2."""
    f, w2 = filter_weights2(n, w)
    half = f // 2
    padded = np.concatenate([np.zeros(half), np.asarray(mag, dtype=np.float64) ** 2])
    rows = n - half
    acc = np.zeros(rows)
    for k in range(f + 1):
        acc += w2[k] * padded[k:k + rows]
    return np.sqrt(acc)


def compensate(x, shift):
    """x[n] * exp(2 pi i shift (n / N - 1/2)) with the phase reduced in turns."""
    n = len(x)
    turns = shift * (np.arange(n) / n - 0.5)
    turns -= np.rint(turns)
    return np.asarray(x, dtype=np.complex128) * np.exp(2j * np.pi * turns)


def shifted_peak(corr, peak, offset):
    """|time shift by `offset` of corr[peak - 5 : peak + 6]| (clipped) -> (start, magnitudes)."""
    start, stop = max(0, peak - PEAK_WINDOW // 2), min(len(corr), peak + PEAK_WINDOW // 2 + 1)
    cut = np.asarray(corr[start:stop], dtype=np.complex128)
    moved = np.fft.ifft(np.fft.fft(cut) * np.exp(2j * np.pi * offset * np.fft.fftfreq(len(cut))))
    return start, np.abs(moved)


def autocorr(template):
    t = np.asarray(template, dtype=np.float64)
    return np.array([np.sum(t[lag:] * t[:len(t) - lag]) if lag < len(t) else 0.0 for lag in range(AUTOCORR_LAGS)])


def threshold(coeffs, noise, std):
    return float(np.sqrt(coeffs[0] + coeffs[1] * noise ** 2 + (coeffs[2] * std ** 2 if coeffs[2] else 0.0)))


def numbers(block, block_idx, settings, timestamp=0.0):
    """One block through the oracle -> (detected, DetectionResult, unsynced, data dict) or, without a carrier,
    (False, DetectionResult, unsynced, None).  `data` has the device's arrays and scalars in float64."""
    block = np.asarray(block)
    x = onp.iq_u8_to_c64(block) if block.dtype == np.uint8 else block.astype(np.complex64)
    n, w = settings.block_len, settings.carrier_len
    det = onp.OracleDetector(n, settings.history_len, [np.asarray(settings.template)], settings.carrier_thresh,
                             settings.carrier_window, settings.corr_thresh, carrier_len=w)
    (res,), ((xhat, corr),) = det.detect_block(block_idx, x, want_data=True)
    car = res.carrier
    cinfo = toads_data.CarrierSyncInfo(int(car.bin), float(car.offset), np.float32(car.energy), np.float32(car.noise))
    if xhat is None:
        return False, toads_data.DetectionResult(timestamp, block_idx, None, cinfo, None, -1), x, None
    cs = res.corr
    xinfo = toads_data.CorrDetectionInfo(int(cs.sample), float(cs.offset), float(cs.energy), float(cs.noise))
    result = toads_data.DetectionResult(timestamp, block_idx, res.soa, cinfo, xinfo, -1)
    fft_mag = np.abs(np.fft.fft(x))
    filtered = filtered_spectrum(fft_mag, n, w)
    synced = compensate(x, -(int(car.bin) + float(car.offset)))
    synced_mag = np.abs(xhat)
    corr_mag = np.abs(corr)
    want_car, want_cor = bool(settings.carrier_thresh[2]), bool(settings.corr_thresh[2])
    stds = dict(fft_std=np.std(fft_mag) if want_car else 0.0, synced_fft_std=np.std(synced_mag) if want_car else 0.0,
                filtered_std=np.std(filtered) if want_car else 0.0, corr_std=np.std(corr_mag) if want_cor else 0.0)
    fit_valid = 6 <= car.bin <= n - 7
    amp, off = onp.dirichlet_fit(fft_mag, int(car.bin), n, w) if fit_valid else (np.nan, np.nan)
    start, moved = shifted_peak(corr, int(cs.sample), float(cs.offset))
    shifted = np.zeros(PEAK_WINDOW)
    shifted[:len(moved)] = moved
    scalars = dict(rms_unsynced=float(np.sqrt(np.mean(np.abs(x.astype(np.complex128)) ** 2))),
                   rms_synced=float(np.sqrt(np.mean(np.abs(synced) ** 2))),
                   carrier_threshold=threshold(settings.carrier_thresh, float(cinfo.noise), stds["fft_std"]),
                   corr_threshold=threshold(settings.corr_thresh, float(cs.noise), stds["corr_std"]),
                   fit_amplitude=float(amp), fit_offset=float(off), fit_valid=int(fit_valid), peak_start=start,
                   peak_len=len(moved), corr_shifted=shifted, **{k: float(v) for k, v in stds.items()})
    hist = np.bincount(block, minlength=256) if block.dtype == np.uint8 else np.zeros(256, np.int64)
    data = dict(hist=hist, fft_mag=fft_mag, filtered=filtered, synced=synced, synced_fft_mag=synced_mag, corr=corr,
                scalars=scalars, autocorr=autocorr(settings.template))
    return bool(cs.detected), result, x, data


def numbers_at(block, record, settings, fit=True):
    """The `data` dict of `numbers()` at a GIVEN record: carrier bin and offset, correlation sample and offset
    and both noise values are read from `record` (a mapping or a NumPy record with the fields carrier_bin,
    carrier_offset, corr_sample, corr_offset, carrier_noise, corr_noise); no detector runs.  Everything else is
    evaluated at that record's shift with the oracle's own functions.  Fed the oracle's record it returns what
    `numbers()` returns.  `fit=False` leaves the Dirichlet fit out (NaN) where it is ill conditioned."""
    block = np.asarray(block)
    x = onp.iq_u8_to_c64(block) if block.dtype == np.uint8 else block.astype(np.complex64)
    n, w = settings.block_len, settings.carrier_len
    cbin, coff = int(record["carrier_bin"]), float(record["carrier_offset"])
    sample, soff = int(record["corr_sample"]), float(record["corr_offset"])
    cnoise, xnoise = float(record["carrier_noise"]), float(record["corr_noise"])
    bank = onp.TemplateBank(np.asarray(settings.template), n, settings.history_len)
    fft_mag = np.abs(np.fft.fft(x))
    filtered = filtered_spectrum(fft_mag, n, w)
    xhat = onp.shift_and_fft(x, -(np.int64(cbin) + coff))
    corr = onp.despread(xhat, bank)
    synced = compensate(x, -(cbin + coff))
    synced_mag = np.abs(xhat)
    corr_mag = np.abs(corr)
    want_car, want_cor = bool(settings.carrier_thresh[2]), bool(settings.corr_thresh[2])
    stds = dict(fft_std=np.std(fft_mag) if want_car else 0.0, synced_fft_std=np.std(synced_mag) if want_car else 0.0,
                filtered_std=np.std(filtered) if want_car else 0.0, corr_std=np.std(corr_mag) if want_cor else 0.0)
    fit_valid = 6 <= cbin <= n - 7
    amp, off = onp.dirichlet_fit(fft_mag, cbin, n, w) if fit_valid and fit else (np.nan, np.nan)
    start, moved = shifted_peak(corr, sample, soff)
    shifted = np.zeros(PEAK_WINDOW)
    shifted[:len(moved)] = moved
    scalars = dict(rms_unsynced=float(np.sqrt(np.mean(np.abs(x.astype(np.complex128)) ** 2))),
                   rms_synced=float(np.sqrt(np.mean(np.abs(synced) ** 2))),
                   carrier_threshold=threshold(settings.carrier_thresh, cnoise, stds["fft_std"]),
                   corr_threshold=threshold(settings.corr_thresh, xnoise, stds["corr_std"]),
                   fit_amplitude=float(amp), fit_offset=float(off), fit_valid=int(fit_valid), peak_start=start,
                   peak_len=len(moved), corr_shifted=shifted, **{k: float(v) for k, v in stds.items()})
    hist = np.bincount(block, minlength=256) if block.dtype == np.uint8 else np.zeros(256, np.int64)
    return dict(hist=hist, fft_mag=fft_mag, filtered=filtered, synced=synced, synced_fft_mag=synced_mag, corr=corr,
                scalars=scalars, autocorr=autocorr(settings.template))


def record_of(result):
    """The record fields `numbers_at` reads, from the DetectionResult `numbers()` returns."""
    c, x = result.carrier_info, result.corr_info
    return dict(carrier_bin=c.bin, carrier_offset=c.offset, carrier_noise=c.noise, corr_sample=x.sample,
                corr_offset=x.offset, corr_noise=x.noise)


def dossier(block, block_idx, settings, sample_rate=SAMPLE_RATE, timestamp=0.0):
    """The package's Dossier over the oracle's float64 numbers (None if the block is not detected)."""
    from thrifty_amd.detect_analysis import Dossier
    detected, result, x, data = numbers(block, block_idx, settings, timestamp)
    return Dossier(result, x, data, settings, sample_rate) if detected else None
