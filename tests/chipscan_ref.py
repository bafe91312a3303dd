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


# ------------------------------------------------------------------------------------------ the GPU tests' yardstick
# (tests/test_gpu_chipscan.py and tests/test_gpu_chipscan_seams.py share it)
REL = 1e-4          # energy, noise
OFFSET_ABS = 1e-3
TIE = 1e-4          # top-2 gap below which the index is not compared
CURVATURE = 1e-4    # |2 log b - log a - log c| below which the offset is not compared


def engine(carrier_len, max_batch=16, block_len=N, **kw):
    """an ordinary handle with the tuning tool's carrier setup; its own template is never used by the scan"""
    from thrifty_amd import _native
    own = np.where(np.arange(64) % 3 == 0, 1.0, -1.0)
    return _native.Engine(block_len, 63, own, CARRIER_THRESH, None, (0.0, 0.0, 0.0),
                          carrier_len=carrier_len, max_batch=max_batch, **kw)


def compare(got, ref, what, max_excluded=0.05):
    """the device's records against `scan`'s (test_gpu_chipscan.py's docstring); returns the number of pairs
    the index comparison left out"""
    assert got.shape == ref.shape
    ok = (ref["flags"] & 1) != 0
    assert np.array_equal((got["flags"] & 1) != 0, ok), what
    quiet = got[~ok]
    assert np.all(quiet["sample"] == -1) and np.all(quiet["flags"] == 0) and np.all(quiet["energy"] == 0), what
    assert np.all(quiet["noise"] == 0) and np.all(quiet["offset"] == 0), what
    tie = ok & (ref["top2_gap"] < TIE)
    sure = ok & ~tie
    e_dev = np.abs(got["energy"][ok] - ref["energy"][ok]) / ref["energy"][ok]
    n_dev = np.abs(got["noise"][ok] - ref["noise"][ok]) / ref["noise"][ok]
    smooth = sure & (ref["curvature"] > CURVATURE)
    o_dev = np.abs(got["offset"][smooth] - ref["offset"][smooth])
    print("%s: %d pairs, %d ties left out, energy %.2e noise %.2e offset %.2e (over %d)"
          % (what, ok.sum(), tie.sum(), e_dev.max(initial=0), n_dev.max(initial=0), o_dev.max(initial=0), smooth.sum()))
    assert tie.sum() <= max_excluded * max(1, ok.sum()), what
    assert np.array_equal(got["sample"][sure], ref["sample"][sure]), what
    assert np.array_equal(got["flags"][ok], ref["flags"][ok]), what
    assert np.all(e_dev <= REL) and np.all(n_dev <= REL), what
    assert np.all(o_dev <= OFFSET_ABS), what
    assert np.all(got["offset"][sure & (ref["offset"] == 0)] == 0), what      # (the first and the last lag)
    return int(tie.sum())


def same(a, b):
    return a.tobytes() == b.tobytes()


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


# The scenes of tests/test_gpu_chipscan_seams.py (carrier_len 2455 throughout).  The figures in their
# docstrings are this file's float64 results; tests/test_chipscan_host.py asserts them.
LANE_LAGS = [1, 2, 63, 64, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 8191, 8192, 13312, 13921, 13922]
LANE_LENGTHS = np.array([2461, 2460, 2462], dtype=np.int32)


def lane_scene():
    """-> (u8 blocks [17, 2N], chips, lengths): the length-2461 burst at the seams of the scan kernel's lag map
    n = n1 * 1024 + 2t + e (wave w owns the lags 128w .. 128w + 127 of every row): even and odd lags, both
    sides of a wave seam (127 / 128) and of a row seam (1023 / 1024, where lag pk - 1 belongs to thread 511
    of the row below), the row seam of the last wave (8191 / 8192), pk = 1 (a neighbour at lag 0), 13312 =
    13 * 1024 (the last row a 2461-window reaches), corr_len - 3 and corr_len - 2 (a neighbour at the last
    searched lag).  Seed 41.  Restatement: the peak of length 2461 is the planted lag in all 17 blocks,
    1 of the 51 pairs is a near-tie (top-2 gap < 1e-4), the smallest curvature at 2461 is 1.05."""
    rng = np.random.default_rng(41)
    chips = synth.gold_code(10, 0)
    blocks = [burst_block(rng, chips, 2461, lag, carrier_bin=float(rng.uniform(-500, 500))) for lag in LANE_LAGS]
    return np.stack(blocks), chips, LANE_LENGTHS


MASK_LENGTHS = np.array([2461, 2462, 2465, 2470, 2500, 3000], dtype=np.int32)


def mask_scene():
    """-> (u8 block [1, 2N], chips, lengths): edge_scene's burst of length 2461 at the last lag, 13923, against
    longer templates, whose windows [0, N - L] end before it.  Restatement: peaks [13923, 13922, 13919, 13914,
    13108, 12881]; for the first four lengths that is corr_len - 1 (offset 0, top-2 gaps >= 0.15), and for
    2462, 2465 and 2470 the largest |corr| of all N lags lies just beyond the window: a window one lag too
    long, or none, finds another peak, one a lag too short finds corr_len - 2 with a fitted offset.  No ties."""
    blocks, chips, _ = edge_scene()
    return blocks[1:2], chips, MASK_LENGTHS


LENGTH_LENGTHS = np.array([1, 2, 3, 64, 1023, 1024, 1025, 4097, 8191, 8192, 8193, 16381, 16382], dtype=np.int32)


def length_scene():
    """-> (u8 blocks [9, 2N], chips, lengths): seam_scene's blocks against template lengths at the edges of the
    bank kernel's sample map n = n1 * 1024 + 2t, 2t + 1: a single thread's samples, a row, half the block,
    the longest length, each with its odd and even neighbours.  The bursts are the long ones of seam_scene
    (a burst of a few samples carries no carrier line).  Restatement: every block but the quiet one has a
    carrier, 0 near-ties of 104 pairs, the smallest top-2 gap is 4.7e-4."""
    blocks, chips, _ = seam_scene()
    return blocks, chips, LENGTH_LENGTHS


def group_scene():
    """-> (u8 blocks [16, 2N], chips, lengths): seam_scene(16) (block 4 quiet) against the 70 lengths 2427 ..
    2496 -- enough candidates per block that a workgroup of the scan walks several of them.  Restatement:
    4 near-ties of 1050 pairs."""
    blocks, chips, _ = seam_scene(16)
    return blocks, chips, np.arange(2427, 2497, dtype=np.int32)
