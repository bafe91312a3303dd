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
shifted signal is the magnitude of the input.

    python -m thrifty_amd.template_extract rx.card --template base.npy -o captured.npy --average
    python -m thrifty_amd.template_extract rx.card --template base.npy -o captured.npy --average \\
        --freq-map freqmap.cfg --rxid 0

With --average the device also sums the cut of EVERY qualifying detection: the averaged
template goes to the output, or with a frequency map one captured.tx<ID>.npy per transmitter."""
from __future__ import annotations

import argparse
import collections
import os
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


Average = collections.namedtuple("Average", "templates sem count n_unclassified acc_e acc_q txids")
Average.__doc__ = """The averaged templates of an extraction (thr_extract_average*): templates[K][W] and sem[K][W]
(float64; NaN rows for a class no detection fell into), count[K], n_unclassified, the integer sums acc_e[K][W]
and acc_q[K][W] (uint64), and txids[K] (the keys of a `classes` dict, else 0 .. K-1)."""


class Extracted(tuple):
    """extract()'s (template, result) with the averaged templates as `.average`."""
    average = None


def class_ranges(classes):
    """`classes` of extract(): None / a list of (lo, hi) / {txid: (lo, hi)} -> (txids, [(lo, hi)])."""
    if classes is None:
        return [0], []
    if isinstance(classes, dict):
        txids, ranges = list(classes.keys()), [tuple(classes[t]) for t in classes]
    else:
        ranges = [tuple(r) for r in classes]
        txids = list(range(len(ranges)))
    if len(ranges) > _native.AVERAGE_MAX_CLASSES:
        raise ValueError("an extraction averages at most %d classes, %d given" % (_native.AVERAGE_MAX_CLASSES, len(ranges)))
    return txids, [(float(lo), float(hi)) for lo, hi in ranges]


def _average_of(x, w, txids):
    count, n_unclassified = x.average_counts()
    k = len(txids)
    templates, sem = np.full((k, w), np.nan), np.full((k, w), np.nan)
    acc_e, acc_q = np.zeros((k, w), dtype=np.uint64), np.zeros((k, w), dtype=np.uint64)
    for c in range(k):
        if count[c]:
            templates[c], sem[c], acc_e[c], acc_q[c] = x.average_result(c, w)
    return Average(templates, sem, count[:k].copy(), n_unclassified, acc_e, acc_q, list(txids))


def extract(settings, blocks, max_offset=MAX_OFFSET, device_id=0, batch_size=None, average=False, classes=None):
    """-> (template float64[len(settings.template)], DetectionResult of the block it was cut from).
    `blocks`: a `CardStream` / `RawStream` (a mapped file runs inside the library, a pipe in batches) or
    any iterable of `(timestamp, block_idx, block)`.  ValueError if no detection qualifies; IndexError
    where the reference's loop raises one (carrier_sync.py:187).
    average=True: the same pair with `.average` (an `Average`): every qualifying detection's cut summed on the
    device, per class; `classes` is a list of (lo, hi) ranges of carrier_bin + carrier_offset or a
    {txid: (lo, hi)} dict (inclusive, the last match wins), None: one class.  u8 input only."""
    txids, ranges = class_ranges(classes) if average else (None, None)
    if average and isinstance(blocks, RawStream):
        raise ValueError("average=True takes u8 blocks (.card input, or an iterable of u8 blocks): a raw capture's "
                         "zero-history lead-in blocks are complex, and the sums are exact integers of the u8 quantiser")
    det = Detector(settings, blocks, device_id=device_id, batch_size=batch_size)
    try:
        with _native.Extraction(det._engine, max_offset) as x:
            if average:
                x.average(ranges)
            reader = det._card if det._card is not None else det._raw
            if reader is not None and reader.mapped:
                stats = _feed_mapped(det, x)
                det._finish_library_loop()
                if stats is not None and stats["index_error"]:
                    raise det._index_error(stats["index_error_bin"])
            else:
                _feed_batches(det, x)
            rec, timestamp, template, _ = x.result(len(settings.template))
            averaged = _average_of(x, len(settings.template), txids) if average else None
        if not average:
            return template, det._result(timestamp, int(rec["block_idx"]), rec)[1]
        out = Extracted((template, det._result(timestamp, int(rec["block_idx"]), rec)[1]))
        out.average = averaged
        return out
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
    parser.add_argument("--average", action="store_true",
                        help="write the average over EVERY qualifying detection instead of the single best block")
    parser.add_argument("--min-count", dest="min_count", type=int, default=1,
                        help="--average: fewest detections a template is written from [default: %(default)s]")
    parser.add_argument("--freq-map", dest="freq_map", type=argparse.FileType("r"), default=None,
                        help="--average: transmitter frequency map; one <output>.tx<ID>.npy per transmitter")
    parser.add_argument("--rxid", type=int, default=None, help="--freq-map: this receiver's ID in the map")
    parser.add_argument("--npz", metavar="FILE", default=None,
                        help="--average: also keep the sums, the counts and the standard error (.npz)")
    return parser


AVERAGED = "Averaged {} detections; template rms / mean sem = {:.1f}"


def average_classes(args):
    """The command line's averaging arguments, checked before anything touches the device ->
    None (one class) or {txid: (lo, hi)}.  SystemExit with a sentence on what cannot be done."""
    if not args.average:
        for name, flag, unset in (("freq_map", "--freq-map", None), ("npz", "--npz", None), ("rxid", "--rxid", None),
                                  ("min_count", "--min-count", 1)):
            if getattr(args, name) != unset:
                raise SystemExit("template_extract: %s belongs to --average" % flag)
        return None
    if args.raw:
        raise SystemExit("template_extract: --average takes .card input: a raw capture's zero-history lead-in "
                         "blocks are complex, and the sums are exact integers of the u8 quantiser")
    if args.min_count < 1:
        raise SystemExit("template_extract: --min-count must be at least 1, not %d" % args.min_count)
    if args.freq_map is None:
        if args.rxid is not None:
            raise SystemExit("template_extract: --rxid belongs to --freq-map")
        return None
    if args.rxid is None:
        raise SystemExit("template_extract: --freq-map needs --rxid, the receiver whose ranges apply")
    from thrifty_amd.identify import load_freqmap
    with args.freq_map as f:
        freqmap = load_freqmap(f)
    if args.rxid not in freqmap:
        raise SystemExit("template_extract: receiver %d is not in the frequency map (it has %s)"
                         % (args.rxid, ", ".join("@%d" % r for r in sorted(freqmap)) or "no receiver"))
    ranges = freqmap[args.rxid]
    if len(ranges) > _native.AVERAGE_MAX_CLASSES:
        raise SystemExit("template_extract: the map has %d transmitters, an extraction averages at most %d ranges"
                         % (len(ranges), _native.AVERAGE_MAX_CLASSES))
    return ranges


def _said_of(template, sem, count):
    return AVERAGED.format(int(count), float(np.sqrt(np.mean(template ** 2)) / np.mean(sem)))


def _write_average(args, avg, mapped):
    """The averaged templates' files and sentences."""
    from thrifty_amd.fastdet import save_tpl
    stem, ext = os.path.splitext(args.output)
    short = []
    for k, txid in enumerate(avg.txids):
        if avg.count[k] < args.min_count:
            short.append((txid, int(avg.count[k])))
            continue
        name = "%s.tx%d%s" % (stem, txid, ext) if mapped else args.output
        np.save(name, avg.templates[k])
        if args.tpl:
            tstem, text = os.path.splitext(args.tpl)
            save_tpl("%s.tx%d%s" % (tstem, txid, text) if mapped else args.tpl, avg.templates[k])
        said = _said_of(avg.templates[k], avg.sem[k], avg.count[k])
        print("tx %d -> %s: %s" % (txid, name, said) if mapped else said)
    if short:
        print("Fewer than %d detections, no template: %s"
              % (args.min_count, ", ".join("tx %d (%d)" % s for s in short)))
    if mapped and avg.n_unclassified:
        print("%d qualifying detections matched no transmitter of the map" % avg.n_unclassified)
    if args.npz:
        np.savez(args.npz, templates=avg.templates, sem=avg.sem, count=avg.count, acc_e=avg.acc_e, acc_q=avg.acc_q,
                 n_unclassified=np.uint64(avg.n_unclassified), txids=np.asarray(avg.txids, dtype=np.int64))
    return len(short) < len(avg.txids)


def main(argv=None):
    keys = ["sample_rate", "block_size", "block_history", "carrier_window", "carrier_threshold", "corr_threshold",
            "template"]
    config, args = load_args(build_parser(), keys, argv=argv)
    classes = average_classes(args)
    base = np.load(config.template)
    settings = DetectorSettings(
        block_len=config.block_size, history_len=config.block_history, carrier_len=len(base),
        carrier_thresh=config.carrier_threshold, template=base, corr_thresh=config.corr_threshold,
        carrier_window=normalize_freq_range(config.carrier_window, config.sample_rate / config.block_size))
    reader = (RawStream(args.input, config.block_size, config.block_history) if args.raw
              else CardStream(args.input, config.block_size))
    try:
        got = extract(settings, reader, max_offset=args.max_offset, average=args.average, classes=classes)
    except ValueError as exc:
        raise SystemExit("template_extract: %s" % exc)
    template, result = got
    if args.average:
        print(sentence(result))
        if not _write_average(args, got.average, classes is not None):
            raise SystemExit("template_extract: no transmitter reached %d detections" % args.min_count)
        if args.plot:
            _plot(got.average.templates[int(np.argmax(got.average.count))], base, 0.0)
        return 0
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
