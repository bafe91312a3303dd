"""Capture survey: what an operator reads off a raw capture before detecting anything, on an MI355X.

    python -m thrifty_amd.survey capture.bin -i 100 -o survey.npz     # everything, as arrays
    python -m thrifty_amd.survey capture.bin --rms                    # one noise figure per interval
    python -m thrifty_amd.survey capture.bin --hist                   # 256 byte counts per interval
    python -m thrifty_amd.survey capture.bin --fft                    # bin and mean magnitude lines

The capture is cut into blocks of `block_size` samples overlapping by `block_history`, like everywhere
else, and the blocks into consecutive intervals of `integrate`; a trailing partial interval is never
reported.  Per interval (definitions: DESIGN.md 3.11):

  mean spectrum  (1/K) sum_b |FFT(x_b)[k]|, natural bin order (`shifted()` for the plot's order);
  histogram      of the byte values of the interval's blocks (history bytes of overlapping blocks are
                 counted in both blocks);
  norm           (1/K) sum_b sqrt(sum_n |x_b[n]|^2): the square root of the SUM over a block, averaged
                 over the interval.  This is the quantity the reference's noise_rms.py means to print;
                 as committed that script stops at its first block (a method is named where it should
                 be called), so there is no reference output to compare with.

The device returns integers only (sums of rint(|X| 2^S), byte counts, per-block sum v and sum v^2), so
an interval has the same bits however the capture is cut into batches; the divisions happen here, once,
in float64.

The one deviation: the reference's first ceil(H / (N - H)) blocks contain its all-zero initial history,
which has no byte form.  They are not surveyed: interval 0 starts at the first block made of stream bytes
only, and `first_block` carries the reference's index of that block.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from thrifty_amd.block_data import RawStream
from thrifty_amd.settings import load_args

OFFSET = np.float64(np.float32(127.4))      # raw_to_complex: x = (v - OFFSET) / 128
DEFAULT_INTEGRATE = 100


def energy_from_sums(block_sums, block_len):
    """sum_n |x[n]|^2 of blocks from their byte sums (sum v, sum v^2): x = (v - c) / 128 per byte, so the
    energy is (sum v^2 - 2 c sum v + 2 N c^2) / 128^2 -- every term and the first difference exact in
    float64 (c has 24 bits, the sums stay below 2^34)."""
    s = np.asarray(block_sums, dtype=np.uint64).reshape(-1, 2)
    s1, s2 = s[:, 0].astype(np.float64), s[:, 1].astype(np.float64)
    return ((s2 - 2.0 * OFFSET * s1) + 2.0 * block_len * OFFSET * OFFSET) / 16384.0


class SurveyInterval(object):
    """One interval of `n_blocks` blocks from the reference's block index `first_block` on: `mean_mag`
    float64 [N] (natural bin order), `hist` uint64 [256], `block_sums` uint64 [n_blocks, 2]."""

    def __init__(self, first_block, n_blocks, mean_mag, hist, block_sums):
        self.first_block, self.n_blocks = int(first_block), int(n_blocks)
        self.mean_mag, self.hist, self.block_sums = mean_mag, hist, block_sums

    @property
    def block_len(self):
        return len(self.mean_mag)

    @property
    def block_energy(self):
        """sum |x|^2 of every block, float64 [n_blocks]"""
        return energy_from_sums(self.block_sums, self.block_len)

    @property
    def norm(self):
        """mean over the blocks of sqrt(sum |x|^2) -- noise_rms.py's number"""
        return float(np.sqrt(self.block_energy).mean())

    @property
    def rms_per_sample(self):
        """sqrt of the mean |x|^2 over every sample of the interval"""
        return float(np.sqrt(self.block_energy.sum() / (self.n_blocks * self.block_len)))

    @property
    def mean_hist(self):
        """counts per block (fft_analysis.py's histogram)"""
        return self.hist / float(self.n_blocks)

    @property
    def saturation(self):
        """share of the bytes that sit on a rail (0 or 255)"""
        return float(int(self.hist[0]) + int(self.hist[255])) / float(self.hist.sum())

    @property
    def dc(self):
        """mean of (v - c) / 128 over every byte, I and Q together"""
        total = float(self.hist.sum())
        return float((np.arange(256, dtype=np.float64) * self.hist).sum() / total - OFFSET) / 128.0

    def shifted(self):
        """-> (bins int64 [N] from -N/2 up, mean_mag in that order): the order the spectrum is plotted in"""
        n = self.block_len
        return np.arange(n, dtype=np.int64) - n // 2, np.fft.fftshift(self.mean_mag)


def _packed(view, n_blocks, block_len, step):
    """the overlapping blocks of a stream view, copied out back to back"""
    buf = np.frombuffer(view, dtype=np.uint8)
    return np.lib.stride_tricks.as_strided(buf, (n_blocks, 2 * block_len), (step, 1), writeable=False).copy()


class CaptureSurvey(object):
    """survey = CaptureSurvey(16384, 4920, integrate=100); for interval in survey(stream): ...

    `stream`: a binary file object (a regular file is mapped, a pipe read in batches) or a RawStream.
    The engine is a carrier-gate handle, which builds no template spectra.  `backend`: an object with
    _native.Survey's `feed` / `feed_stream` / `shift` / `close` to use instead of the device (tests)."""

    def __init__(self, block_len, history_len=0, integrate=DEFAULT_INTEGRATE, device_id=0, batch_size=None,
                 backend=None):
        self.block_len, self.history_len, self.integrate = int(block_len), int(history_len), int(integrate)
        if self.integrate < 1:
            raise ValueError("integrate must be >= 1")
        self.batch_size = int(batch_size or 2048)
        self._engine = None
        if backend is None:
            from thrifty_amd import _native
            self._engine = _native.Engine.gate(self.block_len, self.history_len, device_id=device_id,
                                               max_batch=self.batch_size)
            backend = _native.Survey(self._engine, self.integrate)
        self._backend = backend

    def close(self):
        if self._backend is not None:
            self._backend.close()
            self._backend = None
        if self._engine is not None:
            self._engine.close()
            self._engine = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __call__(self, stream):
        return self.intervals(stream)

    def intervals(self, stream):
        """Generator of SurveyInterval over the whole stream (the survey starts over: reset)."""
        reader = stream if isinstance(stream, RawStream) else RawStream(stream, self.block_len, self.history_len)
        if (reader.size, reader.history) != (self.block_len, self.history_len):
            raise ValueError("the reader frames %d/%d, the survey %d/%d" % (reader.size, reader.history,
                                                                           self.block_len, self.history_len))
        backend, k = self._backend, self.integrate
        backend.reset()
        scale = float(k) * 2.0 ** backend.shift
        step = 2 * (self.block_len - self.history_len)
        first, done = None, 0
        waiting = np.zeros((0, 2), dtype=np.uint64)
        # a mapped file: the library page-locks it ahead of the chunks' copies (Engine.input_window)
        windowed = self._engine is not None and reader.mapped and reader.device_framing and len(reader.mapped_span())
        if windowed:
            self._engine.input_window(reader.mapped_span())
        try:
            for kind, _, idxs, data in iter(lambda: reader.next_batch(self.batch_size), None):
                if kind != "u8":
                    continue        # the lead-in: blocks that reach before the stream's first byte
                if first is None:
                    first = int(idxs[0])
                if reader.device_framing:
                    spec, hist, sums = backend.feed_stream(data)
                else:
                    spec, hist, sums = backend.feed(_packed(data, len(idxs), self.block_len, step))
                waiting = np.concatenate([waiting, sums])
                for j in range(len(spec)):
                    yield SurveyInterval(first + done * k, k, spec[j].astype(np.float64) / scale, hist[j], waiting[:k])
                    waiting = waiting[k:]
                    done += 1
        finally:
            if windowed:
                self._engine.input_window(None)


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("input", nargs="?", type=argparse.FileType("rb"), default="-",
                        help="raw u8 I/Q capture ('-': standard input)")
    parser.add_argument("-i", "--integrate", type=int, default=DEFAULT_INTEGRATE,
                        help="blocks per interval [default: %(default)s]")
    what = parser.add_mutually_exclusive_group()
    what.add_argument("--rms", action="store_true", help="print the norm of every interval (the default)")
    what.add_argument("--hist", action="store_true", help="print the 256 byte counts of every interval")
    what.add_argument("--fft", action="store_true", help="print 'bin mean_magnitude' lines per interval")
    parser.add_argument("-o", "--output", default=None, help="save every interval's arrays (.npz)")
    return parser


def _print(interval, args, out):
    if args.hist:
        out.write(" ".join(str(int(c)) for c in interval.hist) + "\n")
    elif args.fft:
        for b, m in zip(*interval.shifted()):
            out.write("%d %r\n" % (b, float(m)))
        out.write("\n")
    else:
        out.write("%r\n" % interval.norm)


def save(path, intervals, block_len, history_len, integrate):
    """Every interval's arrays in one .npz: first_block [J], mean_mag [J, N], hist [J, 256],
    block_sums [J, K, 2], norm [J]."""
    np.savez(path, block_len=block_len, history_len=history_len, integrate=integrate,
             first_block=np.array([v.first_block for v in intervals], dtype=np.int64),
             mean_mag=np.array([v.mean_mag for v in intervals], dtype=np.float64).reshape(-1, block_len),
             hist=np.array([v.hist for v in intervals], dtype=np.uint64).reshape(-1, 256),
             block_sums=np.array([v.block_sums for v in intervals], dtype=np.uint64).reshape(-1, integrate, 2),
             norm=np.array([v.norm for v in intervals], dtype=np.float64))


def main(argv=None, out=None, backend=None):
    out = sys.stdout if out is None else out
    config, args = load_args(build_parser(), ["block_size", "block_history"], argv=argv)
    source = args.input.buffer if hasattr(args.input, "buffer") else args.input
    kept = []
    with CaptureSurvey(config.block_size, config.block_history, integrate=args.integrate, backend=backend) as survey:
        for interval in survey(source):
            _print(interval, args, out)
            if args.output:
                kept.append(interval)
    if args.output:
        save(args.output, kept, config.block_size, config.block_history, args.integrate)
    return 0


if __name__ == "__main__":
    sys.exit(main())
