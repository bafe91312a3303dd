"""Chip-rate scan: fine-tune the estimated chip rate of a positioning signal, on an MI355X.

    python -m thrifty_amd.chip_rate_search capture.card 17 2.4M 1.0M 10          # one block, +-1 %
    python -m thrifty_amd.chip_rate_search capture.card 0 2.4M 1.0M 10 --all-blocks --span 0.02 -o scan.npz
    python -m thrifty_amd.chip_rate_search capture.bin 3 2.4M 1.0M 10 --raw --block-size 16384 --history 4920

A transmitter's crystal puts its chip rate tens to hundreds of ppm off nominal, and a Gold-code template
at the wrong rate loses most of its correlation peak.  The template depends on the chip rate through its
length alone -- `synth.gold_template` takes L = int(sample_rate / chip_rate * n_chips) samples and picks
chip (i * n_chips) // L for sample i -- so every chip rate in (fs n_chips / (L + 1), fs n_chips / L] gives
the SAME template, and the peak energy as a function of the chip rate is a staircase.  Scanning every
integer length in a range is therefore exhaustive and deterministic; no optimiser is involved.

Per (block, length) the engine returns what the detector's correlation stage returns with thresholds
(0, 0, 0) and history L - 1 on the block's carrier-shifted spectrum: the first maximum of |corr| over
the lags [0, block_len - L], the noise figure with template energy L, the Gaussian sub-sample offset.
The score of a length is the mean peak energy over the blocks that have a carrier (float64); the best
length is the first maximum of the score.  The carrier setup is the tuning tool's own: constant
threshold 100, every bin, Dirichlet width int(n_chips * sample_rate / chip_rate).
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from thrifty_amd import synth
from thrifty_amd.setting_parsers import metric_float

CARRIER_THRESHOLD = (100.0, 0.0, 0.0)
DEFAULT_SPAN = 0.01
FLAG_CARRIER, FLAG_CORR = 1, 2
PLOT_ANSWER = "chip_rate_search: plots are not part of this port; use -o scan.npz and plot the arrays"


def nominal_length(sample_rate, chip_rate, n_chips):
    """samples of the template at this chip rate, as synth.gold_template counts them"""
    return int(sample_rate / chip_rate * n_chips)


def lengths_for(sample_rate, chip_rate, n_chips, span=DEFAULT_SPAN):
    """int32 array of every integer length within +-`span` (a fraction) of the nominal one, ascending"""
    centre = nominal_length(sample_rate, chip_rate, n_chips)
    lo = max(1, int(np.ceil(centre * (1.0 - span))))
    hi = int(np.floor(centre * (1.0 + span)))
    return np.arange(lo, max(lo, hi) + 1, dtype=np.int32)


def _top_rate(length, sample_rate, n_chips):
    """the largest float chip rate whose template still has `length` samples or more"""
    rate = sample_rate * n_chips / length
    while nominal_length(sample_rate, rate, n_chips) < length:
        rate = np.nextafter(rate, 0.0)
    while nominal_length(sample_rate, np.nextafter(rate, np.inf), n_chips) >= length:
        rate = np.nextafter(rate, np.inf)
    return float(rate)


def rate_interval(length, sample_rate, n_chips):
    """(lo, hi): exactly the chip rates lo < rate <= hi give a template of `length` samples (the ends are
    floats of the sampler's own arithmetic, not of the real-number formula)"""
    return _top_rate(length + 1, sample_rate, n_chips), _top_rate(length, sample_rate, n_chips)


class ChipScanResult(object):
    """lengths int32 [K]; energy, noise float32 [B, K]; sample int32 [B, K]; offset float64 [B, K];
    detected bool [B, K]; carrier_ok bool [B]; score float64 [K]."""

    def __init__(self, lengths, records, sample_rate, n_chips):
        self.sample_rate, self.n_chips = float(sample_rate), int(n_chips)
        self.lengths = np.asarray(lengths, dtype=np.int32)
        self.energy, self.noise = records["energy"].copy(), records["noise"].copy()
        self.sample, self.offset = records["sample"].copy(), records["offset"].copy()
        self.detected = (records["flags"] & FLAG_CORR) != 0
        self.carrier_ok = (records["flags"][:, 0] & FLAG_CARRIER) != 0
        if not self.carrier_ok.any():
            raise ValueError("chip-rate scan: none of the %d block(s) has a carrier" % len(records))
        self.score = self.energy[self.carrier_ok].astype(np.float64).mean(axis=0)

    @property
    def best_index(self):
        return int(np.argmax(self.score))

    @property
    def best_length(self):
        return int(self.lengths[self.best_index])

    @property
    def best_interval(self):
        return rate_interval(self.best_length, self.sample_rate, self.n_chips)

    @property
    def best_rate(self):
        return self.sample_rate * self.n_chips / (self.best_length + 0.5)

    def lines(self):
        """one line per candidate, in the order of `lengths`"""
        for length, score in zip(self.lengths, self.score):
            lo, hi = rate_interval(int(length), self.sample_rate, self.n_chips)
            yield ".. try length %d (chip rate %.3f–%.3f) -> %r" % (length, lo, hi, float(score))

    def save(self, path):
        lo, hi = self.best_interval
        np.savez(path, lengths=self.lengths, energy=self.energy, noise=self.noise, sample=self.sample,
                 offset=self.offset, detected=self.detected, carrier_ok=self.carrier_ok, score=self.score,
                 best_length=self.best_length, best_rate=self.best_rate, best_interval=np.array([lo, hi]),
                 sample_rate=self.sample_rate, n_chips=self.n_chips)


def _as_blocks(blocks):
    """u8 [B, 2N] or complex64 [B, N], and N"""
    a = np.asarray(blocks)
    if a.ndim == 1:
        a = a[None, :]
    if a.dtype == np.uint8:
        return np.ascontiguousarray(a), a.shape[1] // 2
    return np.ascontiguousarray(a.astype(np.complex64)), a.shape[1]


def scan(blocks, sample_rate, chip_rate, bit_length, code_index=0, span=DEFAULT_SPAN, lengths=None,
         device_id=0, max_batch=2048, backend=None):
    """Scan `blocks` (u8 [B, 2N] or complex [B, N]; one block may be 1-D) against the Gold code
    (bit_length, code_index) at every template length within +-span of the nominal one (or at `lengths`)
    -> ChipScanResult.  `backend`: an object with _native.ChipScan's `scan` to use instead of the device
    (tests); its `configure(block_len, carrier_len, carrier_thresh)` is called first if it has one."""
    data, block_len = _as_blocks(blocks)
    chips = synth.gold_code(bit_length, code_index).astype(np.uint8)
    n_chips = len(chips)
    if lengths is None:
        lengths = lengths_for(sample_rate, chip_rate, n_chips, span)
    lengths = np.asarray(lengths, dtype=np.int32).reshape(-1)
    if lengths.size == 0 or lengths.min() < 1 or lengths.max() > block_len - 2:
        raise ValueError("chip-rate scan: template lengths must lie in [1, %d]" % (block_len - 2))
    carrier_len = nominal_length(sample_rate, chip_rate, n_chips)
    engine = None
    if backend is None:
        from thrifty_amd import _native
        # (the engine wants a template of its own; the scan never uses it)
        own = synth.gold_template(bit_length, code_index)
        engine = _native.Engine(block_len, len(own) - 1, own, CARRIER_THRESHOLD, None, (0.0, 0.0, 0.0),
                                carrier_len=carrier_len, device_id=device_id,
                                max_batch=max(1, min(int(max_batch), len(data))))
        backend = _native.ChipScan(engine)
    elif hasattr(backend, "configure"):
        backend.configure(block_len=block_len, carrier_len=carrier_len, carrier_thresh=CARRIER_THRESHOLD)
    try:
        records = backend.scan(data, chips, lengths)
    finally:
        if engine is not None:
            backend.close()
            engine.close()
    return ChipScanResult(lengths, records, sample_rate, n_chips)


def search(block, initial_chip_rate, bit_length, code_index, sample_rate, span=DEFAULT_SPAN, out=None, **kwargs):
    """The chip rate whose template correlates best with `block`: the middle of the best length's rate
    interval.  With `out`, one line per candidate is written to it."""
    result = scan(block, sample_rate, initial_chip_rate, bit_length, code_index, span=span, **kwargs)
    if out is not None:
        _emit(out, result.lines())
    return result.best_rate


def _emit(out, lines):
    for line in lines:
        try:
            out.write(line + "\n")
        except UnicodeEncodeError:      # a stream that cannot say "–"
            out.write(line.replace("–", "-") + "\n")


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("card_file", type=argparse.FileType("rb"), default="-",
                        help=".card file (or, with --raw, a raw u8 I/Q capture) holding the positioning signal")
    parser.add_argument("block_id", type=int, help="index of the block to match against")
    parser.add_argument("sample_rate", type=metric_float, help="sample rate of the capture")
    parser.add_argument("chip_rate", type=metric_float, help="estimated chip rate")
    parser.add_argument("bit_length", type=int, help="register length n of the Gold code: 2^n - 1 chips")
    parser.add_argument("code_index", nargs="?", type=int, default=0, help="which code of that family [default: 0]")
    parser.add_argument("--span", type=float, default=DEFAULT_SPAN,
                        help="scan the template lengths within this fraction of the nominal one [default: %(default)s]")
    parser.add_argument("--all-blocks", action="store_true", help="scan every block of the file; block_id is ignored")
    parser.add_argument("--raw", action="store_true", help="the file is a raw capture, framed by --block-size / --history")
    parser.add_argument("--block-size", type=int, default=16384, help="--raw: samples per block [default: %(default)s]")
    parser.add_argument("--history", type=int, default=0, help="--raw: samples of overlap [default: %(default)s]")
    parser.add_argument("-o", "--output", default=None, help="save the scan's arrays (.npz)")
    parser.add_argument("-p", "--plot", action="store_true", help="not part of this port")
    return parser


def _read_blocks(args):
    """the chosen blocks as one array: u8 [B, 2N] where every block has its bytes, else complex64 [B, N]"""
    from thrifty_amd.block_data import block_reader, card_reader
    source = args.card_file.buffer if hasattr(args.card_file, "buffer") else args.card_file
    reader = block_reader(source, args.block_size, args.history) if args.raw else card_reader(source)
    chosen = [blk for _, idx, blk in reader if args.all_blocks or idx == args.block_id]
    if not chosen:
        raise ValueError("no blocks in the file" if args.all_blocks else
                         "Could not find block with index %d" % args.block_id)
    if all(blk.raw is not None for blk in chosen):
        return np.stack([np.asarray(blk.raw, dtype=np.uint8) for blk in chosen])
    return np.stack([np.asarray(blk, dtype=np.complex64) for blk in chosen])


def main(argv=None, out=None, backend=None):
    out = sys.stdout if out is None else out
    args = build_parser().parse_args(argv)
    if args.plot:
        sys.stderr.write(PLOT_ANSWER + "\n")
        return 2
    result = scan(_read_blocks(args), args.sample_rate, args.chip_rate, args.bit_length, args.code_index,
                  span=args.span, backend=backend)
    _emit(out, result.lines())
    lo, hi = result.best_interval
    _emit(out, ["Best chip rate: %r (length %d, chip rates %r–%r, %d of %d block(s) with a carrier)"
                % (result.best_rate, result.best_length, lo, hi, int(result.carrier_ok.sum()), len(result.carrier_ok))])
    if args.output:
        result.save(args.output)
    return 0


if __name__ == "__main__":
    sys.exit(main())
