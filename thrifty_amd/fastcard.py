"""Carrier gate: raw capture -> carrier verdict -> .card, on the GPU.

Stands in for the reference's native `fastcard -i <file> [--card] -o <out.card>` (fastcard/
fastcard_cli.c; the reference's fastcard_capture.py spawns that binary, here it is a module):

    python -m thrifty_amd.fastcard -i capture.bin -o rx.card [-b N] [-h H] [-k K] [-w MIN-MAX]
                                   [-t 100c2s] [--card] [-q]

Every block of the input runs through the engine's carrier stage; cardet's power-domain verdict
(fastcard/cardet.c:7-41) picks the blocks that hold a carrier, and only those are base64-encoded --
on the device -- and written as `.card` lines `<sec>.<usec> <block_idx> <base64>`.

Framing is the reference's (raw_reader.c:15-46, fastcard_cli.c:151-169): a block is the last
`history` samples of the previous block plus `block_len - history` new ones; the first `skip`
blocks are read and dropped, and the first block that is kept has index 0.  So kept block i is the
window that starts 2 * (block_len - history) * (i + skip) - 2 * history bytes into the stream and is
read in place.  ONE deviation: where that offset is negative (skip < ceil(history / (block_len -
history))) the missing history is zero BYTES here; the reference leaves it uninitialised
(reader.c:49 is a malloc).

Capture hardware is out of scope: `-i rtlsdr`, the tuner options and
`--wisdom-file` are refused.
"""
from __future__ import annotations

import argparse
import base64
import math
import mmap
import os
import re
import sys
import time

import numpy as np

from thrifty_amd import block_data

DEFAULT_BLOCK_LEN = 16384       # fargs.c:6-14
DEFAULT_HISTORY_LEN = 4920
DEFAULT_THRESHOLD = "100c2s"
DEFAULT_WINDOW = "0--1"
DEFAULT_SKIP = 1
TOOL = "thrifty_amd.fastcard (MI355X carrier gate)"

_C_FLOAT = re.compile(r"\s*[+-]?(?:(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?|inf(?:inity)?|nan)", re.I)
_C_INT = re.compile(r"\s*[+-]?\d+")


def parse_threshold(text):
    """'<constant>c<snr>s' -> (constant, snr) as float32 values, like parse_theshold_str
    (fastcard/parse.c:54-99): numbers in any order, each followed by 'c' (constant), 's' (snr) or the
    end of the string (constant); a missing one is 0; a second constant or snr, or anything else, is
    refused (ValueError)."""
    const = snr = np.float32(0)
    got_const = got_snr = False
    at = 0
    while True:
        m = _C_FLOAT.match(text, at)
        if not m:
            break
        value = np.float32(float(m.group(0)))
        at = m.end()
        tail = text[at:at + 1]
        if tail in ("c", ""):
            if got_const:
                raise ValueError("Argument '--threshold' contains more than one value for constant.")
            const, got_const = value, True
            at += len(tail)
        elif tail == "s":
            if got_snr:
                raise ValueError("Argument '--threshold' contains more than one value for SNR.")
            snr, got_snr = value, True
            at += 1
        # (any other character: the next number match fails on it, and it is reported below)
    if at != len(text):
        raise ValueError("Argument '--threshold' contains an invalid value.")
    return float(const), float(snr)


def parse_window(text):
    """'<min>-<max>' -> (min, max) like parse_carrier_str (fastcard/parse.c:39-52, sscanf "%d-%d"):
    a single number is min = max; what follows the numbers is ignored; no number at all is refused."""
    m = _C_INT.match(text)
    if not m:
        raise ValueError("Argument '--carrier' contains an invalid value.")
    lo = hi = int(m.group(0))
    if text[m.end():m.end() + 1] == "-":
        m2 = _C_INT.match(text, m.end() + 1)
        if m2:
            hi = int(m2.group(0))
    return lo, hi


def normalize_window(lo, hi, block_len):
    """cardet_normalize_window (fastcard/cardet.c:43-70) -> inclusive, non-wrapping (min, max):
    negative ends count from the end, min < 0 <= max and ends outside the spectrum are refused
    (ValueError), reversed ends are swapped."""
    if lo < 0 and hi >= 0:
        raise ValueError("Carrier frequency window range not supported.")
    if lo < 0:
        lo += block_len
    if hi < 0:
        hi += block_len
    if not (0 <= lo < block_len and 0 <= hi < block_len):
        raise ValueError("Carrier frequency window out of range.")
    return (hi, lo) if hi < lo else (lo, hi)


def window_offset(i, skip, block_len, history_len):
    """Byte offset into the raw stream of kept block i (negative: the block starts in the zero
    history in front of the stream)."""
    return 2 * (block_len - history_len) * (i + skip) - 2 * history_len


def kept_blocks(n_bytes, skip, block_len, history_len):
    """Blocks a raw stream of n_bytes yields behind the skipped ones (a short tail is dropped)."""
    return max(0, n_bytes // (2 * (block_len - history_len)) - skip)


def card_header(block_len, history_len, window, threshold, start_time=None):
    """The '#' lines fastcard puts in front of a .card FILE (fargs_print_card_header, fargs.c:194-214),
    with this tool's name in `# tool:`."""
    t = time.time() if start_time is None else start_time
    us = int(round(t * 1e6))
    return ("# arguments: { carrier_bin: '%d-%d', threshold: '%gc+%gs', block_size: %d, history_size: %d }\n"
            "# tool: '%s'\n"
            "# start_time: %d.%06d\n" % (window[0], window[1], threshold[0], threshold[1], block_len, history_len,
                                         TOOL, us // 1000000, us % 1000000))


def _whole_input(src):
    """-> a bytes-like object holding the whole input: the mmap of a regular file, else everything
    the stream delivers (a path, '-' for stdin, a binary file object or bytes-like)."""
    if isinstance(src, (bytes, bytearray, memoryview, mmap.mmap, np.ndarray)):
        return src
    if isinstance(src, str):
        if src == "-":
            return sys.stdin.buffer.read()
        with open(src, "rb") as f:
            if os.fstat(f.fileno()).st_size == 0:
                return b""
            return mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
    mapped, at = block_data._map_regular_file(src)
    if mapped is not None:
        return memoryview(mapped)[at:]
    return src.read()


class CarrierGate(object):
    """fastcard as an object.  `window` = (min, max) bins as fastcard's -w takes them, `threshold` =
    (constant, snr) in the power domain (or the strings the CLI takes).

        gate = CarrierGate(16384, 4920, (7, 110), (100, 2))
        gate.run("capture.bin", "rx.card")                 # the file loop; gate.stats afterwards
        for t, idx, block in gate(open("capture.bin", "rb")):   # what card_reader yields for that file
            ...
    """

    def __init__(self, block_len=DEFAULT_BLOCK_LEN, history_len=DEFAULT_HISTORY_LEN, window=(0, -1),
                 threshold=(100.0, 2.0), skip=DEFAULT_SKIP, device_id=0, batch_size=None):
        self.block_len, self.history_len = int(block_len), int(history_len)
        if self.block_len < 1 or self.block_len & (self.block_len - 1):
            raise ValueError("block_len %d is not a power of two" % self.block_len)
        if not 0 <= self.history_len < self.block_len:
            raise ValueError("history must be shorter than the block")
        self.window = parse_window(window) if isinstance(window, str) else (int(window[0]), int(window[1]))
        self.threshold = parse_threshold(threshold) if isinstance(threshold, str) else (
            float(np.float32(threshold[0])), float(np.float32(threshold[1])))
        self.bins = normalize_window(self.window[0], self.window[1], self.block_len)
        self.skip = int(skip)
        if self.skip < 0:
            raise ValueError("skip must not be negative")
        self.device_id = int(device_id)
        # a batch's payload slots are batch * 8/3 * block_len bytes of host memory: 64 MiB of input by default
        self.batch_size = int(batch_size) if batch_size else max(1, (64 << 20) // (2 * self.block_len))
        self.payload_chars = (2 * self.block_len + 2) // 3 * 4
        self.stats = {}
        self._eng = None

    # ---- engine ----------------------------------------------------------------------------
    def engine(self):
        if self._eng is None:
            from thrifty_amd import _native
            self._eng = _native.Engine.gate(self.block_len, self.history_len, self.window, self.threshold,
                                            device_id=self.device_id, max_batch=self.batch_size)
        return self._eng

    def close(self):
        if self._eng is not None:
            self._eng.close()
            self._eng = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- batches ---------------------------------------------------------------------------
    def _raw_batches(self, buf, timestamp):
        """-> (timestamps, records, n_passed, slots) per batch of a raw u8 I/Q stream."""
        eng = self.engine()
        n, h = self.block_len, self.history_len
        step = 2 * (n - h)
        if step % 4:
            raise ValueError("raw-stream framing needs an even block_len - history_len")
        data = np.frombuffer(buf, dtype=np.uint8)
        total = kept_blocks(data.size, self.skip, n, h)
        self.stats["bytes_in"] = int(data.size)
        i = 0
        # blocks that start in front of the stream: the missing history is zero bytes
        lead = []
        while i < total and window_offset(i, self.skip, n, h) < 0:
            off = window_offset(i, self.skip, n, h)
            blk = np.zeros(2 * n, dtype=np.uint8)
            blk[-off:] = data[:2 * n + off]
            lead.append(blk)
            i += 1
        if lead:
            t0 = time.time()
            rec, k, slots = eng.gate_blocks(np.stack(lead), np.arange(len(lead), dtype=np.int64))
            self.stats["gate_s"] += time.time() - t0
            yield [t0 if timestamp is None else timestamp] * len(lead), rec, k, slots
        while i < total:
            nb = min(self.batch_size, total - i)
            off = window_offset(i, self.skip, n, h)
            t0 = time.time()
            rec, k, slots = eng.gate_stream(data[off:off + (nb - 1) * step + 2 * n], first_block_idx=i)
            self.stats["gate_s"] += time.time() - t0
            yield [t0 if timestamp is None else timestamp] * nb, rec, k, slots
            i += nb

    def _card_batches(self, buf):
        """The same for .card text: timestamps and indices come from the input lines."""
        from thrifty_amd import _native
        eng = self.engine()
        self.stats["bytes_in"] = len(buf)
        pos, end, skip = 0, len(buf), self.skip
        while pos < end:
            ts, idx, off, nxt = _native.frame_card(buf, pos, end, self.block_len, True, self.batch_size)
            if nxt == pos and not len(off):
                break
            pos = nxt
            if skip:                         # (the first `skip` blocks are read and dropped, whatever the reader)
                drop = min(skip, len(off))
                ts, idx, off, skip = ts[drop:], idx[drop:], off[drop:], skip - drop
            if not len(off):
                continue
            t0 = time.time()
            rec, k, slots = eng.gate_card(buf, off, idx)
            self.stats["gate_s"] += time.time() - t0
            yield ts, rec, k, slots

    def _batches(self, src, card, timestamp):
        self.stats = {"blocks": 0, "passed": 0, "bytes_in": 0, "text_bytes": 0, "total_s": 0.0, "gate_s": 0.0,
                      "format_s": 0.0, "write_s": 0.0}
        buf = _whole_input(src)
        gen = self._card_batches(buf) if card else self._raw_batches(buf, timestamp)
        for ts, rec, k, slots in gen:
            self.stats["blocks"] += len(rec)
            self.stats["passed"] += k
            passed = rec["flags"] & 1 != 0
            yield np.asarray(ts, dtype=np.float64)[passed], rec, rec[passed], slots

    # ---- the reader interface ----------------------------------------------------------------
    def __call__(self, stream, card=False, timestamp=None):
        """Iterate the passed blocks of `stream` as `block_data.card_reader` would yield them from
        the written file: (timestamp, block_idx, IQBlock)."""
        return self._iter(stream, card, timestamp)

    def _iter(self, stream, card, timestamp):
        stride, chars = self.engine().slot_stride, self.engine().payload_chars
        for ts, _, rec, slots in self._batches(stream, card, timestamp):
            for k in range(len(rec)):
                raw = np.frombuffer(base64.b64decode(slots[k * stride:k * stride + chars].tobytes()), dtype=np.uint8)
                us = int(round(ts[k] * 1e6))          # (a .card line holds microseconds)
                yield (float("%d.%06d" % divmod(us, 1000000)), int(rec["block_idx"][k]),
                       block_data.IQBlock(block_data.raw_to_complex(raw), raw))

    # ---- the file loop -------------------------------------------------------------------------
    def run(self, input, output, card=False, info=None, header=None, timestamp=None):
        """`fastcard -i input [--card] -o output`: gate the whole input, write the .card text -- ONE call
        into the library (thr_run_gate_stream / thr_run_gate_card: the calling thread frames and gates
        batches, a library thread assembles the lines and writes them to the output's descriptor).
        input: a path ('-' = stdin, read to its end first), a binary file object or bytes; output: a path
        ('-' = stdout), an object with a descriptor, any other binary file object (the text is spooled
        through a temporary file) or None (verdicts only).  info: a text stream for fastcard's info lines
        (None: quiet).  header: write the '#' header (default: when output is a path other than '-').
        -> the statistics (thr_gate_run_stats), also in `.stats`."""
        import tempfile
        own = spool = None
        if isinstance(output, str):
            if header is None:
                header = output != "-"
            out = sys.stdout.buffer if output == "-" else open(output, "wb")
            own = None if output == "-" else out
        else:
            out = output
        buf = _whole_input(input)
        eng = self.engine()
        windowed = False
        try:
            if info is not None:
                info.write("block size: %d; history length: %d\n" % (self.block_len, self.history_len))
                info.write("carrier bin window: min = %d; max = %d\n" % self.window)
                info.write("threshold: constant = %g; snr = %g\n\n" % self.threshold)
                if self.skip > 0:
                    info.write("\nSkipping %d block(s)... done\n\n" % self.skip)
            fd = None
            if out is not None:
                if header:
                    out.write(card_header(self.block_len, self.history_len, self.window, self.threshold).encode())
                out.flush()
                try:
                    fd = out.fileno()
                except (AttributeError, OSError, ValueError):
                    spool = tempfile.TemporaryFile()
                    fd = spool.fileno()
            rec = None
            if info is not None:          # (a record per block, for the info lines of the passed ones)
                size = len(buf)
                most = size // (self.payload_chars + 4) + 1 if card else kept_blocks(size, 0, self.block_len, self.history_len)
                from thrifty_amd import _native
                rec = np.zeros(max(1, most), dtype=_native.RECORD_DTYPE)
            if isinstance(buf, (mmap.mmap, memoryview)) and len(buf):
                eng.input_window(buf)
                windowed = True
            self.stats = eng.run_gate(buf, card=card, out_fd=fd, skip=self.skip, timestamp=timestamp,
                                      batch_blocks=self.batch_size, rec_out=rec)
            if spool is not None:
                spool.seek(0)
                while True:
                    piece = spool.read(1 << 24)
                    if not piece:
                        break
                    out.write(piece)
                out.flush()
            if info is not None:
                rec = rec[:self.stats["blocks"]]
                rec = rec[rec["flags"] & 1 != 0]
                thr = rec["reserved"].astype(np.uint32).view(np.float32)
                for r, t in zip(rec, thr):
                    info.write("block #%d: mag[%d] = %.1f (thresh = %.1f, noise = %.1f)\n" % (
                        r["block_idx"], r["carrier_bin"], r["carrier_energy"],
                        math.sqrt(t) if t >= 0 else float("nan"), r["carrier_noise"]))
                info.write("\nRead %d blocks.\n%d blocks passed the carrier gate.\n" % (
                    self.stats["blocks"], self.stats["passed"]))
                info.flush()
        finally:
            if windowed:
                eng.input_window(None)
            if spool is not None:
                spool.close()
            if own is not None:
                own.close()
            if isinstance(input, str) and isinstance(buf, mmap.mmap):      # (a mapping this call made)
                buf.close()
        return self.stats


_OUT_OF_SCOPE = ("capture hardware is out of scope of this engine (no RTL-SDR reader, no FFT wisdom): "
                 "record the raw u8 I/Q to a file and pass it with -i.")


def build_parser():
    """fastcard's option letters (fargs.c:29-77): -h is the history length, so the parser is built
    without argparse's own -h and keeps --help."""
    p = argparse.ArgumentParser(prog="python -m thrifty_amd.fastcard", add_help=False,
                                description="Carrier gate on the GPU: raw u8 I/Q capture (or .card) -> .card")
    p.add_argument("--help", action="help", help="show this help message and exit")
    p.add_argument("-i", "--input", default="-", metavar="<FILE>", help="input file ('-' for stdin) [default: stdin]")
    p.add_argument("--card", action="store_true", help="input is a .card file instead of binary data")
    p.add_argument("-o", "--output", default=None, metavar="<FILE>", help="output .card file ('-' for stdout)")
    p.add_argument("-m", "--wisdom-file", default=None, metavar="<FILE>", help="refused: " + _OUT_OF_SCOPE)
    p.add_argument("-b", "--block-len", type=int, default=DEFAULT_BLOCK_LEN, metavar="<length>")
    p.add_argument("-h", "--history", type=int, default=DEFAULT_HISTORY_LEN, metavar="<length>",
                   help="samples at the beginning of a block copied from the end of the previous one [default: 4920]")
    p.add_argument("-k", "--skip", type=int, default=DEFAULT_SKIP, metavar="<num_blocks>")
    for short, name in (("-f", "--frequency"), ("-s", "--sample-rate"), ("-g", "--gain"), ("-d", "--device-index")):
        p.add_argument(short, name, default=None, help="refused: tuner option")
    p.add_argument("-w", "--carrier-window", default=DEFAULT_WINDOW, metavar="<min>-<max>")
    p.add_argument("-t", "--threshold", default=DEFAULT_THRESHOLD, metavar="<constant>c<snr>s")
    p.add_argument("-q", "--quiet", action="store_true")
    return p


def gate_from_args(args):
    """-> CarrierGate for parsed arguments; SystemExit with one sentence for what is out of scope."""
    if args.input == "rtlsdr" or args.wisdom_file is not None or any(
            v is not None for v in (args.frequency, args.sample_rate, args.gain, args.device_index)):
        raise SystemExit("thrifty_amd.fastcard: " + _OUT_OF_SCOPE)
    try:
        return CarrierGate(args.block_len, args.history, args.carrier_window, args.threshold, skip=args.skip)
    except ValueError as exc:
        raise SystemExit("thrifty_amd.fastcard: %s" % exc)


def main(argv=None):
    args = build_parser().parse_args(argv)
    gate = gate_from_args(args)
    # info lines on stdout, or on stderr when the card itself goes to stdout (fastcard_cli.c:105-111)
    info = None if args.quiet else sys.stderr if args.output == "-" else sys.stdout
    with gate:
        gate.run(args.input, args.output, card=args.card, info=info)
    return 0


if __name__ == "__main__":
    sys.exit(main())
