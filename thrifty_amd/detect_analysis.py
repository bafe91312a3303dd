"""Detection dossiers: what the reference's `thrifty analyze_detect` shows, as numbers, on an MI355X.

    python -m thrifty_amd.detect_analysis rx.card -i 1000-2000 -m 20 --template tpl.npy --save sig --views v

The capture goes through the ordinary detect pipeline; behind every batch the device hands the first
`-m` blocks that are detected, and whose index lies in the `-i` ranges, a slot each and keeps their
samples (`_native.Dossiers`).  Per kept block the device then delivers what the
reference's plots are drawn from: byte histogram, spectrum, Dirichlet-filtered spectrum, thresholds,
frequency-compensated samples, their spectrum, the correlation, the carrier fit and the shifted
correlation peak.  A `Dossier` turns them into *views*: per plot command of the reference the x / y
series and the horizontal and vertical line values it would draw.  The views only slice, reorder, scale
and evaluate the two short interpolation curves; there are no plots here (`--export` and the Qt viewer
are refused).
"""
from __future__ import annotations

import argparse
import base64
import re
import sys
from collections import namedtuple

import numpy as np

from thrifty_amd import _native, util
from thrifty_amd.block_data import CardStream, block_reader, raw_to_complex
from thrifty_amd.detect import Detector, DetectorSettings
from thrifty_amd.detect_cli import SummaryLineFormatter
from thrifty_amd.setting_parsers import normalize_freq_range
from thrifty_amd.settings import load_args
from thrifty_amd.stages import unique_window

DetectorResult = namedtuple("DetectorResult", ["detected", "result", "unsynced", "synced", "corr"])
View = namedtuple("View", ["name", "lines", "hlines", "vlines"])      # (label, x, y) / (label, value) / (label, value)

PLOT_COMMANDS = ("hist", "iq", "mag", "iq_synced", "mag_synced", "template", "fft", "fft_window", "fft_synced",
                 "filtered_fft", "carrier_peak_unsynced", "carrier_peak_synced", "psd", "psd_synced", "corr",
                 "corr_zoomed", "corr_interpol", "corr_shifted")
FIGURE_COMMANDS = {
    "overview": ("hist", "mag_synced", "fft_window", "corr"),
    "time": ("iq", "mag_synced"),
    "overlays": ("template", "template", "template", "template"),      # full / start / centre / end: one series
    "spectra": ("fft_window", "psd_synced", "carrier_peak_unsynced", "carrier_peak_synced"),
    "corrs": ("corr", "corr_zoomed", "corr_interpol", "corr_shifted"),
}
NO_PLOTS = "analyze_detect on the device delivers numbers (--save, --views), not plots: {} is not offered."
_RANGE = re.compile(r"\s*(\d+)?\s*(-)?\s*(\d+)?\s*\Z")


def parse_range_list(string):
    """'1-5, 20-, -3, 7' -> [(1, 5), (20, None), (None, 3), (7, 7)]: closed ranges, open ends are None."""
    out = []
    for part in string.split(","):
        hit = _RANGE.match(part)
        if hit is None:
            raise ValueError("'" + string + "' is not a range of numbers.")
        lo, dash, hi = hit.groups()
        if dash is None:
            if hi is not None:
                raise ValueError("'" + string + "' is not a range of numbers.")
            hi = lo
        out.append((None if lo is None else int(lo), None if hi is None else int(hi)))
    return out


def block_in_range(block_idx, ranges):
    return any((lo is None or block_idx >= lo) and (hi is None or block_idx <= hi) for lo, hi in ranges)


def _dirichlet(x, n, w):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.sin(np.pi * w * x / n) / np.sin(np.pi * x / n) / w
    d[np.isnan(d)] = 1
    return d


def _window_bins(window, n):
    """The carrier window's two edges as signed bins (what the spectrum views mark)."""
    lo, hi = window
    if abs(lo) >= n or abs(hi) >= n:
        raise ValueError("Frequency window out of range: {} - {}".format(lo, hi))
    if lo < 0 <= hi:
        lo, hi = n + lo, n + hi
    lo, hi = (v + n if v < 0 else v for v in (lo, hi))
    if hi < lo:
        lo, hi = hi, lo
    return util.fft_bin(lo, n), util.fft_bin(hi, n)


class Dossier(object):
    """Everything about one kept block.  `result` is the DetectionResult, `unsynced` the block's samples,
    `synced` / `corr` the frequency-compensated samples and the correlation; `data` holds the device's other
    arrays (hist, fft_mag, filtered, synced_fft_mag), its scalars and the template's autocorrelation."""

    def __init__(self, result, unsynced, data, settings, sample_rate):
        self.result, self.unsynced = result, unsynced
        self.synced, self.corr = data["synced"], data["corr"]
        self.data, self.settings, self.sample_rate = data, settings, sample_rate
        self.detected = True

    # ---- pieces shared by several views
    def _scalar(self, name):
        return float(self.data["scalars"][name])

    def _samples(self, name, signal, mag=False, iq=False, rms=None):
        lines = []
        if mag:
            lines.append(("Mag", np.arange(len(signal)), np.abs(signal)))
        if iq:
            lines += [("Real", np.arange(len(signal)), np.real(signal)), ("Imag", np.arange(len(signal)), np.imag(signal))]
        hlines = [("RMS", rms)] if rms is not None else []
        hlines.append(("Noise", float(self.result.carrier_info.noise) / np.sqrt(len(signal))))
        return View(name, lines, hlines, [])

    def _threshold(self, std_name):
        """The carrier threshold over a spectrum whose standard deviation the device reports as `std_name`."""
        c = self.settings.carrier_thresh
        noise = float(self.result.carrier_info.noise)
        std = self._scalar(std_name) if c[2] else 0.0
        return float(np.sqrt(c[0] + c[1] * noise ** 2 + c[2] * std ** 2))

    def _spectrum(self, name, mag, std_name, label="", scaled=False, window=False):
        n = len(mag)
        bins = np.arange(n) - n // 2
        if scaled:      # power spectral density in dB / Hz over kHz
            y_scale, x_scale = np.sqrt(1 / (n * self.sample_rate)), self.sample_rate / n / 1e3
            transf = lambda v: 20 * np.log10(v * y_scale)      # noqa: E731
        else:
            x_scale, transf = 1, lambda v: v * 1               # noqa: E731
        lines = [(label, bins * x_scale, transf(np.fft.fftshift(mag)))]
        hlines = [("Threshold", float(transf(self._threshold(std_name)))),
                  ("Noise", float(transf(float(self.result.carrier_info.noise))))]
        vlines = []
        if window and self.settings.carrier_window:
            vlines = [("", float(v)) for v in _window_bins(self.settings.carrier_window, self.settings.block_len)]
        return View(name, lines, hlines, vlines)

    def _peak_window(self, length):
        peak = self.result.corr_info.sample
        start, stop = max(0, peak - length // 2), min(len(self.corr), peak + length // 2 + 1)
        return start, stop, peak - start

    # ---- the 18 plot commands
    def view(self, name):
        s, res, d = self.settings, self.result, self.data
        n = s.block_len
        if name == "hist":
            return View(name, [("", np.arange(256), d["hist"] / n / 2 * 100)], [], [])
        if name == "iq":
            return self._samples(name, self.unsynced, iq=True)
        if name == "mag":
            return self._samples(name, self.unsynced, mag=True, rms=self._scalar("rms_unsynced"))
        if name == "iq_synced":
            return self._samples(name, self.synced, iq=True)
        if name == "mag_synced":
            return self._samples(name, self.synced, mag=True, rms=self._scalar("rms_synced"))
        if name == "template":
            start = res.corr_info.sample
            cut = self.synced[start:start + len(s.template)]
            ook = np.asarray(s.template, dtype=np.float64) - np.min(s.template)
            ook = ook * np.sqrt(np.mean(np.abs(cut) ** 2)) / np.sqrt(np.mean(ook ** 2))
            overlay = self._samples(name, cut, mag=True)
            return overlay._replace(lines=[("Template", np.arange(len(ook)) + res.corr_info.offset, ook)] + overlay.lines)
        if name in ("fft", "fft_window"):
            return self._spectrum(name, d["fft_mag"], "fft_std", label="FFT", window=True)
        if name == "fft_synced":
            return self._spectrum(name, d["synced_fft_mag"], "synced_fft_std")
        if name == "filtered_fft":
            return self._spectrum(name, d["filtered"], "filtered_std", label="FFT", window=True)
        if name == "psd":
            return self._spectrum(name, d["fft_mag"], "fft_std", scaled=True)
        if name == "psd_synced":
            return self._spectrum(name, d["synced_fft_mag"], "synced_fft_std", scaled=True)
        if name == "carrier_peak_unsynced":
            peak = res.carrier_info.bin
            start, stop = max(0, peak - 6), min(n, peak + 7)
            mags = d["fft_mag"][start:stop]
            idx = np.arange(len(mags)) - (peak - start)
            lines, vlines = [("FFT", idx, mags)], [("", float("nan"))]
            if d["scalars"]["fit_valid"]:
                amp, off = self._scalar("fit_amplitude"), self._scalar("fit_offset")
                sub = np.arange(-off, len(mags) - off, 0.1) - (peak - start)
                lines.append(("Interpolation", sub + off, np.abs(_dirichlet(sub, n, s.carrier_len)) * amp))
                vlines = [("", off)]
            else:       # too close to the spectrum's edge for the seven-point fit
                lines.append(("Interpolation", np.zeros(0), np.zeros(0)))
            return View(name, lines, [], vlines)
        if name == "carrier_peak_synced":
            idx = np.arange(-6, 7)
            mags = d["synced_fft_mag"]
            return View(name, [("FFT (synced)", idx, mags[idx]),
                               ("Interpolation", idx, np.abs(_dirichlet(idx, n, s.carrier_len)) * mags[0])], [], [])
        corr_mag_of = lambda a, b: np.abs(self.corr[a:b])      # noqa: E731
        peak, offset = res.corr_info.sample, res.corr_info.offset
        if name == "corr":
            lo, hi = unique_window(n, s.history_len, len(s.template))
            return View(name, [("Corr", np.arange(len(self.corr)), np.abs(self.corr))],
                        [("Noise", float(res.corr_info.noise)), ("Threshold", self._scalar("corr_threshold"))],
                        [("", float(lo)), ("", float(hi)), ("", float(peak + offset))])
        if name == "corr_zoomed":
            start, stop = max(0, peak - 200), min(len(self.corr), peak + 200)
            return View(name, [("Corr", np.arange(stop - start) + start, corr_mag_of(start, stop))], [],
                        [("", float(peak + offset))])
        if name == "corr_interpol":
            start, stop, at = self._peak_window(10)
            mags = corr_mag_of(start, stop).astype(np.float64)
            lines = [("Xcorr", np.arange(len(mags)) - at, mags)]
            if 0 < at < len(mags) - 1:      # the three-point log parabola through the peak
                y1, y2, y3 = np.log(mags[at - 1:at + 2])
                off = 0.5 * (y3 - y1) / (2 * y2 - y1 - y3)
                a = (y1 - y2) / ((off + 1) ** 2 - off ** 2)
                x = np.linspace(off - 2, off + 2, 50)
                lines.append(("Interpolation", x, np.exp(a * (x - off) ** 2 + (y1 - a * (off + 1) ** 2))))
            return View(name, lines, [], [("", float(offset))])
        if name == "corr_shifted":
            sc = d["scalars"]
            start, at = int(sc["peak_start"]), peak - int(sc["peak_start"])
            mags = np.asarray(sc["corr_shifted"][:int(sc["peak_len"])], dtype=np.float64)
            idx = np.arange(len(mags)) - at
            auto = np.asarray(d["autocorr"], dtype=np.float64)[np.abs(idx)]
            return View(name, [("Shifted xcorr", idx, mags), ("Autocorr", idx, auto * (mags[at] / auto[at]))], [], [])
        raise KeyError("unknown view '{}' (one of: {})".format(name, ", ".join(PLOT_COMMANDS)))

    def figure(self, name):
        """The views of one of the reference's five figure commands, in subplot order."""
        return tuple(self.view(v) for v in FIGURE_COMMANDS[name])


class ForcibleDetector(object):
    """A detector whose verdicts can be forced: `force_carrier` / `force_corr` set that stage's threshold
    to (0, 0, 0) and the engine handle is created with them.  Called with one block it returns a
    DetectorResult; `synced` and `corr` are delivered for detected blocks (None otherwise)."""

    def __init__(self, settings, force_carrier=False, force_corr=False, blocks=None, device_id=0, batch_size=None):
        stages = (("carrier_thresh", force_carrier), ("corr_thresh", force_corr))
        self.settings = settings._replace(**{name: (0, 0, 0) for name, forced in stages if forced})
        self._one = None        # a one-slot dossier for __call__, made on first use
        self.detector = Detector(self.settings, blocks, device_id=device_id, batch_size=batch_size)

    def close(self):
        if self._one is not None:
            self._one.close()
            self._one = None
        self.detector.close()

    def __call__(self, timestamp, block_idx, block):
        if self._one is None:
            self._one = _native.Dossiers(self.detector._engine, ((None, None),), 1)
        self._one.reset()
        recs = self._one.feed(self.detector._stack([block]), [timestamp], [block_idx])
        detected, result = self.detector._result(timestamp, block_idx, recs[0])
        if not self._one.n_kept:
            return DetectorResult(detected, result, block, None, None)
        got = self._one.result(arrays=("synced", "corr"))
        return DetectorResult(detected, result, block, got["synced"][0], got["corr"][0])


def _as_complex(block):
    block = np.asarray(block)
    raw = getattr(block, "raw", None)
    if block.dtype == np.uint8:
        return raw_to_complex(block)
    return raw_to_complex(raw) if raw is not None and block.dtype != np.complex64 else block.astype(np.complex64)


def scan(forcible, blocks, ranges, max_keep, log=None):
    """Feed `blocks` (a CardStream, or any iterable of (timestamp, block_idx, block)) through the detector
    until `max_keep` blocks are kept or the input ends -> (Dossiers object, the kept blocks' samples).
    `log` receives the reference's "Checking block #i" / "Skipping block #i" lines, derived from the records."""
    det = forcible.detector
    dos = _native.Dossiers(det._engine, ranges, max_keep)
    kept_samples = []
    state = {"kept": 0}

    def after(recs, stamps, fetch):
        new = dos.n_kept - state["kept"]
        if log is not None:
            left = new if dos.full else None      # the loop ends with the record that fills the last slot
            both = _native.FLAG_CARRIER | _native.FLAG_CORR
            for rec in recs:
                if left == 0:
                    break
                idx = int(rec["block_idx"])
                if not block_in_range(idx, ranges):
                    continue
                log("Checking block #{}".format(idx))
                if int(rec["flags"]) & both == both:
                    left = None if left is None else left - 1
                else:
                    log("Skipping block #{}".format(idx))
        if new:
            got = dos.result(state["kept"], new, arrays=())
            base = dos_fed[0]
            kept_samples.extend(fetch(int(p) - base) for p in got["positions"])
            state["kept"] = dos.n_kept
        dos_fed[0] += len(recs)

    dos_fed = [0]
    size = det.batch_size
    if isinstance(blocks, CardStream):
        chars = blocks.payload_chars
        for stamps, idxs, text, off in iter(lambda: blocks.next_batch(size), None):
            recs = dos.feed_card(text, off, stamps, idxs)
            view = memoryview(text)
            after(recs, stamps, lambda i: raw_to_complex(np.frombuffer(
                base64.b64decode(bytes(view[int(off[i]):int(off[i]) + chars])), dtype=np.uint8)))
            if dos.full:
                break
    else:
        pending = []

        def flush():
            stamps, idxs, blks = zip(*pending)
            recs = dos.feed(det._stack(blks), stamps, idxs)
            after(recs, stamps, lambda i: _as_complex(blks[i]))
            del pending[:]

        for item in blocks:
            pending.append(item)
            if len(pending) == size:
                flush()
                if dos.full:
                    break
        if pending and not dos.full:
            flush()
    return dos, kept_samples


def analyze(blocks_or_stream, settings, ranges=((None, None),), max_keep=20, sample_rate=2.2e6, force_carrier=False,
            force_corr=False, log=None, device_id=0, batch_size=None):
    """-> list of `Dossier`, one per kept block, in feed order."""
    forcible = ForcibleDetector(settings, force_carrier, force_corr, device_id=device_id, batch_size=batch_size)
    try:
        dos, samples = scan(forcible, blocks_or_stream, ranges, max_keep, log)
        with dos:
            got = dos.result()
            out = []
            for k in range(dos.n_kept):
                rec = got["records"][k]
                _, result = forcible.detector._result(float(got["timestamps"][k]), int(rec["block_idx"]), rec)
                data = {name: got[name][k] for name in _native.DOSSIER_ARRAYS}
                data["autocorr"] = got["autocorr"]
                out.append(Dossier(result, samples[k], data, forcible.settings, sample_rate))
            return out
    finally:
        forcible.close()


def scalar_lines(dossier, names):
    """The views' horizontal and vertical line values as text, one line per view that has any."""
    out = []
    for name in names:
        for v in (dossier.figure(name) if name in FIGURE_COMMANDS else (dossier.view(name),)):
            marks = ["{}={:.6g}".format(label or "h", value) for label, value in v.hlines]
            marks += ["{}={:.6g}".format(label or "v", value) for label, value in v.vlines]
            if marks:
                out.append("  {}: {}".format(v.name, ", ".join(marks)))
    return out


def view_arrays(dossier, names):
    """Every requested view's arrays under '<view>.line<j>.x' / '.y', '<view>.hlines', '<view>.vlines'."""
    out = {}
    for name in names:
        for v in (dossier.figure(name) if name in FIGURE_COMMANDS else (dossier.view(name),)):
            for j, (label, x, y) in enumerate(v.lines):
                out["{}.line{}.x".format(v.name, j)] = np.asarray(x)
                out["{}.line{}.y".format(v.name, j)] = np.asarray(y)
                out["{}.line{}.label".format(v.name, j)] = np.array(label)
            out[v.name + ".hlines"] = np.array([value for _, value in v.hlines], dtype=np.float64)
            out[v.name + ".hlabels"] = np.array([label for label, _ in v.hlines], dtype=str)
            out[v.name + ".vlines"] = np.array([value for _, value in v.vlines], dtype=np.float64)
    return out


def save_arrays(dossier):
    """What --save stores per kept block, under the reference's keys."""
    return dict(unsynced=dossier.unsynced, synced=dossier.synced, corr=dossier.corr,
                template=dossier.settings.template, carrier_info=dict(dossier.result.carrier_info._asdict()),
                corr_info=dict(dossier.result.corr_info._asdict()))


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("input", type=argparse.FileType("rb"), default="data.card", help="input data ('-': standard input)")
    parser.add_argument("--raw", action="store_true", help="input data is raw binary data")
    parser.add_argument("-f", "--force_cardet", action="store_true", help="force carrier detection")
    parser.add_argument("-F", "--force_corrdet", action="store_true", help="force correlation peak detection")
    parser.add_argument("-i", "--blocks", type=parse_range_list, default="0-", help="indices of blocks to look at")
    parser.add_argument("-m", "--max", type=int, default=20, help="maximum number of blocks")
    parser.add_argument("-p", "--plot", type=str, default="overview,time,overlays,spectra,corrs",
                        help="which views: " + ", ".join(PLOT_COMMANDS + tuple(FIGURE_COMMANDS)))
    parser.add_argument("--export", type=str, nargs="?", const="plot", help="(not offered: no plots)")
    parser.add_argument("--save", type=str, nargs="?", const="signals",
                        help="save detection signals to PREFIX_<block>.npz")
    parser.add_argument("--views", type=str, nargs="?", const="views",
                        help="save the requested views' arrays to PREFIX_<block>_views.npz")
    return parser


def _main(argv=None):
    keys = ["sample_rate", "block_size", "block_history", "carrier_window", "carrier_threshold", "corr_threshold",
            "template"]
    config, args = load_args(build_parser(), keys, argv=argv)
    if args.export:
        raise SystemExit(NO_PLOTS.format("--export"))
    if args.max < 1:
        raise SystemExit("analyze_detect: -m/--max must be at least 1")
    cmds = args.plot.split(",")
    for cmd in cmds:
        if cmd not in PLOT_COMMANDS and cmd not in FIGURE_COMMANDS:
            raise SystemExit("analyze_detect: unknown view '{}'".format(cmd))
    template = np.load(config.template)
    settings = DetectorSettings(
        block_len=config.block_size, history_len=config.block_history, carrier_len=len(template),
        carrier_thresh=config.carrier_threshold, template=template, corr_thresh=config.corr_threshold,
        carrier_window=normalize_freq_range(config.carrier_window, config.sample_rate / config.block_size))
    reader = (block_reader(args.input, config.block_size, config.block_history) if args.raw
              else CardStream(args.input, config.block_size))
    try:
        dossiers = analyze(reader, settings, args.blocks, args.max, config.sample_rate, args.force_cardet,
                           args.force_corrdet, log=print)
    except _native.NativeError as exc:
        raise SystemExit("analyze_detect: %s" % exc)
    for dossier in dossiers:
        block = dossier.result.block
        if args.save:
            np.savez("{}_{}.npz".format(args.save, block), **save_arrays(dossier))
        if args.views:
            np.savez("{}_{}_views.npz".format(args.views, block), **view_arrays(dossier, cmds))
    if not args.save and not args.views:
        liner = SummaryLineFormatter(config.sample_rate, settings.block_len, add_dt=False)
        for dossier in dossiers:
            print(liner(True, dossier.result))
            for line in scalar_lines(dossier, cmds):
                print(line)
    return 0


if __name__ == "__main__":
    sys.exit(_main())
