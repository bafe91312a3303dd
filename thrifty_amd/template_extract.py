"""Template extraction: capture -> template.npy, on an MI355X.

    python -m thrifty_amd.template_generate 10 0 -o base.npy
    python -m thrifty_amd.template_extract rx.card --template base.npy -o captured.npy
    python -m thrifty_amd.detect rx.card --template captured.npy ...

The capture is scanned by the ordinary detect pipeline with the base template; the device keeps the
detection with the largest correlation energy among those whose sub-sample offset is at most
`max_offset`, and the input samples of that block.  The new template is the magnitude of
`template_len` samples from the correlation peak on, scaled by 2 / (mean + std) and centred -- the
reference's `thrifty template_extract` (template_extract.py:36-58), whose detour through the shifted
spectrum is not needed: the carrier shift is a unit-modulus phasor per sample, so the magnitude of the
shifted signal is the magnitude of the input."""
from __future__ import annotations

import argparse
import sys

import numpy as np

from thrifty_amd import _native
from thrifty_amd.block_data import CardStream, RawStream, raw_to_complex
from thrifty_amd.detect import Detector, DetectorSettings
from thrifty_amd.setting_parsers import normalize_freq_range
from thrifty_amd.settings import load_args

MAX_OFFSET = 0.2
SENTENCE = "Captured template from block #{} (timestamp: {:.6f}): offset={:+.3f}; corr_ampl={}"


def direct_template(block, sample, template_len):
    """The extraction formula on the host, float64 throughout: `block` is one block's samples (u8 I/Q
    bytes or complex), `sample` the correlation peak.  What the device kernel computes (the tests and
    DESIGN.md 3.6.1 hold the reference's FFT round trip against it)."""
    block = np.asarray(block)
    z = raw_to_complex(block) if block.dtype == np.uint8 else block
    z = np.asarray(z, dtype=np.complex64)[sample:sample + template_len]
    mag = np.hypot(z.real.astype(np.float64), z.imag.astype(np.float64))
    mag = mag * (2.0 / (mag.mean() + mag.std()))
    return mag - mag.mean()


def _stop_at_index_error(det, recs):
    bad = np.flatnonzero(recs["flags"] & _native.FLAG_INDEX_ERROR)
    if len(bad):
        raise det._index_error(recs["carrier_bin"][bad[0]])


def _feed_mapped(det, x):
    """A mapped .card / raw file: the whole-file loop inside the library."""
    if det._card is not None:
        view, _ = det._card.take_rest()
        return x.run(view, card=True, batch_blocks=det.batch_size)
    raw, stats = det._raw, None
    while raw.in_lead_in:            # the zero-history lead-in blocks have no u8 form: complex64 batches
        batch = raw.next_batch(det.batch_size)
        if batch is None:
            return stats
        _, stamps, idxs, data = batch
        _stop_at_index_error(det, x.feed(data, stamps, idxs))
    view, first, n = raw.take_rest()
    if n:
        stats = x.run(view, card=False, first_block_idx=first, batch_blocks=det.batch_size)
    return stats


def _feed_batches(det, x):
    """Anything else -- a pipe behind a batch reader, or any iterable of (timestamp, index, block)."""
    size = det.batch_size
    if det._card is not None:
        for stamps, idxs, text, off in iter(lambda: det._card.next_batch(size), None):
            _stop_at_index_error(det, x.feed_card(text, off, stamps, idxs))
    elif det._raw is not None:
        for kind, stamps, idxs, data in iter(lambda: det._raw.next_batch(size), None):
            recs = (x.feed(data, stamps, idxs) if kind == "c64"
                    else x.feed_stream(data, int(idxs[0]), stamps))
            _stop_at_index_error(det, recs)
    else:
        pending = []
        for item in det.blocks:
            pending.append(item)
            if len(pending) == size:
                _feed_items(det, x, pending)
                pending = []
        if pending:
            _feed_items(det, x, pending)


def _feed_items(det, x, items):
    stamps, idxs, blocks = zip(*items)
    _stop_at_index_error(det, x.feed(det._stack(blocks), stamps, idxs))


def extract(settings, blocks, max_offset=MAX_OFFSET, device_id=0, batch_size=None):
    """-> (template float64[len(settings.template)], DetectionResult of the block it was cut from).
    `blocks`: a `CardStream` / `RawStream` (a mapped file runs inside the library, a pipe in batches) or
    any iterable of `(timestamp, block_idx, block)`.  ValueError if no detection qualifies; IndexError
    where the reference's loop raises one (carrier_sync.py:187)."""
    det = Detector(settings, blocks, device_id=device_id, batch_size=batch_size)
    try:
        with _native.Extraction(det._engine, max_offset) as x:
            reader = det._card if det._card is not None else det._raw
            if reader is not None and reader.mapped:
                stats = _feed_mapped(det, x)
                det._finish_library_loop()
                if stats is not None and stats["index_error"]:
                    raise det._index_error(stats["index_error_bin"])
            else:
                _feed_batches(det, x)
            rec, timestamp, template, _ = x.result(len(settings.template))
        return template, det._result(timestamp, int(rec["block_idx"]), rec)[1]
    finally:
        det.close()


def sentence(result):
    corr = result.corr_info
    return SENTENCE.format(result.block, result.timestamp, corr.offset, corr.energy)


def _plot(template, base, offset):
    """The new template over the base template, the latter moved by the detection's sub-sample offset."""
    try:
        import matplotlib.pyplot as plt
    except ImportError:
        raise SystemExit("-p/--plot needs matplotlib, which is not installed")
    _, axes = plt.subplots()
    for label, shift, data in (("extracted", 0.0, template), ("base", offset, base)):
        axes.plot(np.arange(len(data)) - shift, data, ".-", label=label)
    axes.set_xlabel("sample")
    axes.legend()
    plt.show()


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("input", type=argparse.FileType("rb"), default="-", help="capture ('-': standard input)")
    parser.add_argument("-o", "--output", default="capture.npy", help="the new template (.npy) [default: capture.npy]")
    parser.add_argument("--raw", action="store_true", help="the capture is raw u8 I/Q, not .card text")
    parser.add_argument("--tpl", metavar="FILE", default=None, help="also write the template in fastdet's .tpl format")
    parser.add_argument("--max-offset", dest="max_offset", type=float, default=MAX_OFFSET,
                        help="largest |sub-sample offset| of a detection that may be chosen [default: %(default)s]")
    parser.add_argument("-p", "--plot", action="store_true", help="plot the new template over the base template")
    return parser


def main(argv=None):
    keys = ["sample_rate", "block_size", "block_history", "carrier_window", "carrier_threshold", "corr_threshold",
            "template"]
    config, args = load_args(build_parser(), keys, argv=argv)
    base = np.load(config.template)
    settings = DetectorSettings(
        block_len=config.block_size, history_len=config.block_history, carrier_len=len(base),
        carrier_thresh=config.carrier_threshold, template=base, corr_thresh=config.corr_threshold,
        carrier_window=normalize_freq_range(config.carrier_window, config.sample_rate / config.block_size))
    reader = (RawStream(args.input, config.block_size, config.block_history) if args.raw
              else CardStream(args.input, config.block_size))
    try:
        template, result = extract(settings, reader, max_offset=args.max_offset)
    except ValueError as exc:
        raise SystemExit("template_extract: %s" % exc)
    np.save(args.output, template)
    if args.tpl:
        from thrifty_amd.fastdet import save_tpl
        save_tpl(args.tpl, template)
    print(sentence(result))
    if args.plot:
        _plot(template, base, result.corr_info.offset)
    return 0


if __name__ == "__main__":
    sys.exit(main())
