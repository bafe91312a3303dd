"""Plain float64 NumPy restatement of the chip-rate scan on the project's oracle
(oracle/thrifty_np.py: carrier stage, shift, correlation stage), the seeded scenes the tests share, and
`RefBackend`, which stands in for _native.ChipScan where there is no GPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import thrifty_np as onp  # noqa: E402
from thrifty_amd import synth  # noqa: E402

N = 16384
CARRIER_THRESH = (100.0, 0.0, 0.0)
FLAG_CARRIER, FLAG_CORR = 1, 2

# what the restatement returns per (block, length): the record's fields in float64, and what the GPU
# tests gate their comparisons on
REF_DTYPE = np.dtype([("sample", "<i4"), ("flags", "<u4"), ("energy", "<f8"), ("noise", "<f8"), ("offset", "<f8"),
                      ("top2_gap", "<f8"),      # (largest - second largest window magnitude) / largest
                      ("curvature", "<f8")])    # |2 log b - log a - log c| of the peak's three magnitudes


def template(chips, length):
    """+-1 template of `length` samples: sample i is chip (i * n_chips) // length"""
    chips = np.asarray(chips).astype(bool)
    return np.where(chips, 1, -1)[np.arange(length) * len(chips) // length]


def carrier_stage(block, carrier_len, carrier_thresh=CARRIER_THRESH, window=None):
    """-> (oracle CarrierStage, shifted spectrum or None) of one block (u8 [2N] or complex [N])"""
    block = np.asarray(block)
    x = onp.iq_u8_to_c64(block) if block.dtype == np.uint8 else block.astype(np.complex64)
    det = onp.OracleDetector(len(x), 0, [np.ones(1)], carrier_thresh, window, (0, 0, 0), carrier_len=carrier_len)
    car, xhat, _ = det.carrier_stage(x)
    return car, xhat


def scan_spectrum(xhat, chips, lengths):
    """one block's records: the oracle's correlation stage with thresholds (0, 0, 0) and history L - 1"""
    out = np.zeros(len(lengths), dtype=REF_DTYPE)
    for k, length in enumerate(lengths):
        bank = onp.TemplateBank(template(chips, int(length)), len(xhat), int(length) - 1)
        assert bank.window == (0, bank.corr_len)
        cs, corr = onp.soa_estimate(xhat, bank, (0, 0, 0))
        mag = np.abs(corr)
        top = np.sort(mag)[-2:]
        r = out[k]
        r["sample"], r["flags"] = cs.sample, FLAG_CARRIER | (FLAG_CORR if cs.detected else 0)
        r["energy"], r["noise"], r["offset"] = cs.energy, cs.noise, cs.offset
        r["top2_gap"] = (top[1] - top[0]) / top[1]
        if 0 < cs.sample < len(mag) - 1:
            a, b, c = np.log(mag[cs.sample - 1:cs.sample + 2])
            r["curvature"] = abs(2 * b - a - c)
    return out


def scan(blocks, chips, lengths, carrier_len, carrier_thresh=CARRIER_THRESH, window=None):
    """-> REF_DTYPE [B, K]; a block without a carrier: sample -1, everything else 0"""
    blocks = np.asarray(blocks)
    if blocks.ndim == 1:
        blocks = blocks[None, :]
    out = np.zeros((len(blocks), len(lengths)), dtype=REF_DTYPE)
    for b, block in enumerate(blocks):
        car, xhat = carrier_stage(block, carrier_len, carrier_thresh, window)
        if xhat is None:
            out[b]["sample"] = -1
        else:
            out[b] = scan_spectrum(xhat, chips, lengths)
    return out


class RefBackend(object):
    """_native.ChipScan's `scan` on the host (records in _native.CHIP_RECORD_DTYPE)."""

    def __init__(self, carrier_len=None, carrier_thresh=CARRIER_THRESH):
        self.carrier_len, self.carrier_thresh = carrier_len, carrier_thresh
        self.calls = []

    def configure(self, block_len, carrier_len, carrier_thresh):
        self.carrier_len, self.carrier_thresh = carrier_len, carrier_thresh

    def close(self):
        pass

    def scan(self, blocks, chips, lengths, with_carrier=False):
        from thrifty_amd import _native
        ref = scan(blocks, chips, lengths, self.carrier_len, self.carrier_thresh)
        self.calls.append(ref.shape)
        out = np.zeros(ref.shape, dtype=_native.CHIP_RECORD_DTYPE)
        for name in out.dtype.names:
            out[name] = ref[name]
        return out


# ------------------------------------------------------------------------------------------ scenes
def burst_block(rng, chips, length, lag, carrier_bin=40.3, amp=0.3, sigma=0.05):
    """One u8 block: complex noise (sigma per component, the real parts drawn first), the on-off keyed
    template of `length` samples at `lag`, the whole block mixed to `carrier_bin`, quantised."""
    z = rng.normal(0, sigma, N) + 1j * rng.normal(0, sigma, N)
    z[lag:lag + length] += amp * (template(chips, length) + 1) / 2
    z = z * np.exp(2j * np.pi * carrier_bin * np.arange(N) / N)
    return synth.quantise_iq(z)


def quiet_block(rng):
    """A block no carrier threshold of 100 passes: bytes 127 / 128 with mean 127.4 (no DC, |X| of a few units)"""
    return np.where(rng.random(2 * N) < 0.4, 128, 127).astype(np.uint8)


BASE = dict(nbits=10, index=0, true_length=2461, lag=3000, carrier_len=2455, sample_rate=2.4e6, chip_rate=1.0e6,
            lengths=np.arange(2431, 2492, dtype=np.int32))


def base_scene():
    """-> (u8 block [2N], chips, lengths): ISSUE's base scene, seed 5"""
    chips = synth.gold_code(BASE["nbits"], BASE["index"])
    block = burst_block(np.random.default_rng(5), chips, BASE["true_length"], BASE["lag"])
    return block, chips, BASE["lengths"]


MIXED_LENGTHS = np.array([2470, 2461, 1023, 512, 2461], dtype=np.int32)


def mixed_scene():
    """-> (u8 blocks [3, 2N], chips, lengths): a burst, a quiet block, another burst; lengths with a repeat,
    a descent, sps 1 and fewer samples than chips"""
    rng = np.random.default_rng(11)
    chips = synth.gold_code(10, 0)
    blocks = np.stack([burst_block(rng, chips, 2461, 700, carrier_bin=12.7), quiet_block(rng),
                       burst_block(rng, chips, 2461, 9000, carrier_bin=-301.2)])
    return blocks, chips, MIXED_LENGTHS


def edge_scene():
    """-> (u8 blocks [2, 2N], chips, lengths): the length-2461 burst at lag 0 and at the last lag, N - 2461"""
    rng = np.random.default_rng(23)
    chips = synth.gold_code(10, 0)
    blocks = np.stack([burst_block(rng, chips, 2461, 0, carrier_bin=77.25),
                       burst_block(rng, chips, 2461, N - 2461, carrier_bin=5.5)])
    return blocks, chips, np.array([2461, 2459], dtype=np.int32)


def long_scene():
    """-> (u8 block [2N], chips, lengths): 2047 chips over 16382 samples at lag 1 (corr_len 3), beside a
    length at sps 1 and one below it"""
    rng = np.random.default_rng(29)
    chips = synth.gold_code(11, 0)
    block = burst_block(rng, chips, N - 2, 1, carrier_bin=-20.4)
    return block, chips, np.array([N - 2, 2047, 16000, 1500], dtype=np.int32)


def seam_scene(n_blocks=9):
    """-> (u8 blocks [n_blocks, 2N], chips, lengths): bursts of length 2461 at scattered lags and carrier bins,
    block 4 quiet; 17 lengths around 2461"""
    rng = np.random.default_rng(31)
    chips = synth.gold_code(10, 0)
    blocks = []
    for b in range(n_blocks):
        if b == 4:
            blocks.append(quiet_block(rng))
        else:
            blocks.append(burst_block(rng, chips, 2461, int(rng.integers(1, N - 2461 - 1)),
                                      carrier_bin=float(rng.uniform(-500, 500))))
    return np.stack(blocks), chips, np.arange(2453, 2470, dtype=np.int32)
