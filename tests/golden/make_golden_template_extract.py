#!/usr/bin/env python3
"""Generate the template-extraction fixtures (template_extract/extract_*.npz) by RUNNING THE REFERENCE.

Run in the build container only (needs the reference checkout, read-only):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_template_extract.py

Per geometry: 48 seeded synthetic u8 blocks (thrifty_amd.synth.synth_blocks) go through the
reference's own ``Detector(yield_data=True)``, ``template_extract.best_detection`` and
``template_extract.extract_template``; the blocks, the settings, the per-block verdicts and the
reference's template are stored as .npz data.  A second pick uses a `max_offset` taken from the data
so that the overall strongest detection is excluded and another block wins.  Nothing of the
reference's source is stored -- only inputs and numeric outputs.
"""
import builtins
import os
import sys

import numpy as np
import scipy

REF = os.environ.get("THRIFTY_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
builtins.xrange = range  # gold.py:77 is Python-2 era

from thrifty import block_data, gold, template_extract, template_generate  # noqa: E402
from thrifty.detect import Detector, DetectorSettings  # noqa: E402
from thrifty.signal_utils import Signal  # noqa: E402

from thrifty_amd import synth  # noqa: E402  (input generator only)

N_BLOCKS = 48
MAX_OFFSET = 0.2            # template_extract.MAX_OFFSET
OFFSET_MARGIN = 1e-3        # no |soff| this close to a max_offset: the engine's offsets are held to 5e-6
ENERGY_MARGIN = 1e-4        # runner-up at least this far (relative) below the winner: float32 energies, held to 2e-5

KEYS = ["block_len", "history_len", "carrier_thresh", "carrier_window", "corr_thresh", "template", "blocks",
        "block_idx", "timestamps", "versions", "det", "energy", "soff", "sample",
        "max_offset", "chosen", "n_qualifying", "template_ref",
        "max_offset2", "chosen2", "n_qualifying2", "template_ref2"]

# name -> (block, history, template, carrier window, carrier bins of the synthetic bursts, noise sigma, seed).
# The seeds are the first (from 5) for which the assertions below hold; at two samples per chip the
# correlation peak is so broad that every |soff| lies below 0.01 at synth_blocks' default noise, closer
# together than the margin -- that geometry gets more noise.
GEOMETRIES = {
    "extract_1024": (1024, 512, lambda: template_generate.resample(gold.gold(7, 2), 1.0), (2, 60), (5.0, 55.0),
                     0.02, 11),
    "extract_2048": (2048, 1024, lambda: template_generate.resample(gold.gold(8, 2), 2.0), (2, 60), (5.0, 55.0),
                     0.1, 5),
    "extract_16384": (16384, 4096, lambda: template_generate.resample(gold.gold(10, 2), 1.0), (7, 110),
                      (10.0, 100.0), 0.02, 6),
}


def window_of(n, h, w):
    pad = h - w + 1
    left = pad // 2
    return left, (n - w + 1) - (pad - left)


def reference_pick(settings, items, max_offset):
    """-> (position of the chosen block, the reference's template)."""
    signal, result = template_extract.best_detection(Detector(settings, iter(items), yield_data=True), max_offset)
    template = template_extract.extract_template(signal, result, len(settings.template))
    return int(result.timestamp) - 1000, np.asarray(template, dtype=np.float64)


def check_margins(name, det, energy, soff, max_offset, chosen):
    a = np.abs(soff[det])
    assert np.all(np.abs(a - max_offset) > OFFSET_MARGIN), (name, max_offset, np.sort(a))
    ok = det & (np.abs(soff) <= max_offset)
    order = np.argsort(energy[ok])[::-1]
    best, second = energy[ok][order[0]], energy[ok][order[1]]
    assert np.flatnonzero(ok)[order[0]] == chosen, (name, chosen)
    assert second <= best * (1 - ENERGY_MARGIN), (name, "runner-up within %.1e" % ENERGY_MARGIN, best, second)
    return int(ok.sum()), (best - second) / best


def make(name, seed=None, save=True):
    n, h, make_tpl, window, bins, sigma, seed0 = GEOMETRIES[name]
    seed = seed0 if seed is None else seed
    tpl = np.asarray(make_tpl(), dtype=np.float64)
    w = len(tpl)
    rng = np.random.default_rng(seed)
    blocks, _ = synth.synth_blocks(rng, N_BLOCKS, n, tpl, window_of(n, h, w), carrier_bins=bins, sigma=sigma)
    settings = DetectorSettings(n, h, w, (0, 15, 0), window, tpl, (0, 15, 0))
    idx = np.arange(N_BLOCKS) * 3 + 7
    stamps = 1000.0 + np.arange(N_BLOCKS)          # (the position in the run, recoverable from the result)
    items = [(stamps[i], int(idx[i]), Signal(block_data.raw_to_complex(blocks[i]))) for i in range(N_BLOCKS)]

    det = np.zeros(N_BLOCKS, bool)
    energy, soff = np.zeros(N_BLOCKS), np.zeros(N_BLOCKS)
    sample = np.full(N_BLOCKS, -1, np.int64)
    for i, (detected, res, _, _) in enumerate(Detector(settings, iter(items), yield_data=True)):
        det[i] = detected
        if res.corr_info is not None:
            energy[i], soff[i], sample[i] = res.corr_info.energy, res.corr_info.offset, res.corr_info.sample

    chosen, template_ref = reference_pick(settings, items, MAX_OFFSET)
    nq, gap = check_margins(name, det, energy, soff, MAX_OFFSET, chosen)

    # second pick: a max_offset halfway between two adjacent sorted |soff| below the winner's, so that
    # the overall strongest detection no longer qualifies (the widest such gap)
    v = np.sort(np.abs(soff[det]))
    j = int(np.searchsorted(v, abs(soff[chosen])))
    assert j >= 2, (name, "the winner has (almost) the smallest |soff|")
    k = int(np.argmax(np.diff(v[:j + 1])))
    max_offset2 = float((v[k] + v[k + 1]) / 2)
    chosen2, template_ref2 = reference_pick(settings, items, max_offset2)
    assert chosen2 != chosen
    nq2, gap2 = check_margins(name, det, energy, soff, max_offset2, chosen2)

    meta = dict(
        block_len=n, history_len=h, carrier_thresh=np.array(settings.carrier_thresh, float),
        carrier_window=np.array(window, np.int64), corr_thresh=np.array(settings.corr_thresh, float), template=tpl,
        blocks=blocks, block_idx=idx, timestamps=stamps,
        versions="numpy %s scipy %s python %s" % (np.__version__, scipy.__version__, sys.version.split()[0]),
        det=det, energy=energy, soff=soff, sample=sample,
        max_offset=MAX_OFFSET, chosen=chosen, n_qualifying=nq, template_ref=template_ref,
        max_offset2=max_offset2, chosen2=chosen2, n_qualifying2=nq2, template_ref2=template_ref2)
    assert sorted(meta) == sorted(KEYS)
    if not save:
        return
    path = os.path.join(HERE, "template_extract", name + ".npz")
    np.savez_compressed(path, **meta)
    print("%-14s det=%d  pick #%d of %d (gap %.1e)  max_offset2=%.4f: pick #%d of %d (gap %.1e)  %.0f KiB" % (
        name, det.sum(), chosen, nq, gap, max_offset2, chosen2, nq2, gap2, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    for name in GEOMETRIES:
        make(name)
