#!/usr/bin/env python3
"""Generate tests/golden/chipscan/*.npz by RUNNING THE REFERENCE (build container only: needs the
reference checkout, read-only):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_chipscan.py

For the scenes of tests/chipscan_ref.py it runs the reference's own DefaultSynchronizer on every block and,
per candidate length, its template_generate.generate and SoaEstimator exactly as scripts/chip_rate_search.py
does (thresholds (0, 0, 0), history = len(template) - 1), and stores the u8 blocks, the lengths and per
(block, length) sample / energy / noise / offset / detected.  For the base scene it also runs that script's
own `search` (SciPy Nelder-Mead, xtol 100) from two starting rates and stores where each run ended.  Before saving it asserts what the
issue states about the base scene.  Data only; nothing of the reference's source is stored."""
import builtins
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np
import scipy
import scipy.optimize  # noqa: F401  (the reference's script says `import scipy` and uses scipy.optimize)

REF = os.environ.get("THRIFTY_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
builtins.xrange = range  # gold.py is Python-2 era

from thrifty import block_data, template_generate  # noqa: E402
from thrifty.carrier_sync import DefaultSynchronizer  # noqa: E402
from thrifty.signal_utils import Signal  # noqa: E402
from thrifty.soa_estimator import SoaEstimator  # noqa: E402

import chipscan_ref  # noqa: E402  (scene generator only)

OUT = os.path.join(HERE, "chipscan")


def reference_scan(blocks, nbits, index, lengths, carrier_len):
    blocks = np.atleast_2d(blocks)
    n_chips = (1 << nbits) - 1
    shape = (len(blocks), len(lengths))
    out = {"sample": np.full(shape, -1, np.int32), "energy": np.zeros(shape), "noise": np.zeros(shape),
           "offset": np.zeros(shape), "detected": np.zeros(shape, bool), "carrier_ok": np.zeros(len(blocks), bool)}
    spectra = []
    for b, raw in enumerate(blocks):
        block = Signal(block_data.raw_to_complex(raw))      # what card_reader yields
        sync = DefaultSynchronizer(thresh_coeffs=(100, 0, 0), window=None, block_len=len(block),
                                   carrier_len=carrier_len)
        shifted_fft, _ = sync(block)
        spectra.append(shifted_fft)
        if shifted_fft is None:
            continue
        out["carrier_ok"][b] = True
        for k, length in enumerate(lengths):
            # any sps inside the length's interval gives this template (asserted: the staircase)
            template = template_generate.generate(nbits, index, (int(length) + 0.5) / n_chips)
            assert len(template) == length
            est = SoaEstimator(template=template, thresh_coeffs=(0, 0, 0), block_len=len(shifted_fft),
                               history_len=len(template) - 1)
            detected, info, _ = est(shifted_fft)
            out["sample"][b, k], out["energy"][b, k] = info.sample, info.energy
            out["noise"][b, k], out["offset"][b, k], out["detected"][b, k] = info.noise, info.offset, detected
    return out, spectra


def reference_search(shifted_fft, chip_rate, nbits, index, sample_rate):
    """scripts/chip_rate_search.py's own search(), as that script runs it"""
    spec = importlib.util.spec_from_file_location("ref_chip_rate_search", os.path.join(REF, "scripts", "chip_rate_search.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with contextlib.redirect_stdout(io.StringIO()):
        return float(mod.search(fft=shifted_fft, initial_chip_rate=chip_rate, bit_length=nbits, code_index=index,
                                sample_rate=sample_rate))


def main():
    os.makedirs(OUT, exist_ok=True)
    versions = "numpy %s scipy %s" % (np.__version__, scipy.__version__)

    base = chipscan_ref.BASE
    block, chips, lengths = chipscan_ref.base_scene()
    ref_chips = template_generate.generate(base["nbits"], base["index"], 1.0) > 0
    assert np.array_equal(ref_chips, chips), "synth.gold_code is not the reference's code"
    out, spectra = reference_scan(block, base["nbits"], base["index"], lengths, base["carrier_len"])
    energy = out["energy"][0]
    order = np.argsort(-energy)
    best, second = int(lengths[order[0]]), int(lengths[order[1]])
    drop = 1 - energy[order[1]] / energy[order[0]]
    ours = chipscan_ref.scan(block, chips, lengths, base["carrier_len"])[0]
    print("base: best %d energy %.4f, runner-up %d (%.1f %% lower), smallest top-2 gap %.2e"
          % (best, energy[order[0]], second, 100 * drop, ours["top2_gap"].min()))
    assert best == 2461 and abs(energy[order[0]] - 366.3) < 0.05
    assert second == 2459 and abs(drop - 0.198) < 0.001
    assert abs(ours["top2_gap"].min() - 5.3e-4) < 0.05e-4
    # Nelder-Mead as the script runs it, from the middle of the nominal length's rate interval and from the
    # round figure an operator would type (both give the nominal template, length 2455)
    n_chips = len(chips)
    assert int(base["sample_rate"] / base["chip_rate"] * n_chips) == 2455
    nm_start = np.array([base["sample_rate"] * n_chips / 2455.5, base["chip_rate"]])
    assert all(int(base["sample_rate"] / r * n_chips) == 2455 for r in nm_start)
    nm_rate = np.array([reference_search(spectra[0], r, base["nbits"], base["index"], base["sample_rate"])
                        for r in nm_start])
    nm_length = np.array([int(base["sample_rate"] / r * n_chips) for r in nm_rate])
    for start, rate, length in zip(nm_start, nm_rate, nm_length):
        print("base: Nelder-Mead from %.3f ended at %.3f = length %d" % (start, rate, length))
    assert nm_length[0] == 2461
    np.savez_compressed(os.path.join(OUT, "base.npz"), blocks=block[None, :], lengths=lengths, nbits=base["nbits"],
                        index=base["index"], carrier_len=base["carrier_len"], sample_rate=base["sample_rate"],
                        chip_rate=base["chip_rate"], nm_start=nm_start, nm_rate=nm_rate, nm_length=nm_length,
                        versions=versions, **out)

    blocks, chips, lengths = chipscan_ref.mixed_scene()
    out, _ = reference_scan(blocks, 10, 0, lengths, 2455)
    assert out["carrier_ok"].tolist() == [True, False, True]
    np.savez_compressed(os.path.join(OUT, "mixed.npz"), blocks=blocks, lengths=lengths, nbits=10, index=0,
                        carrier_len=2455, versions=versions, **out)
    for name in sorted(os.listdir(OUT)):
        print(name, os.path.getsize(os.path.join(OUT, name)), "bytes")


if __name__ == "__main__":
    main()
