#!/usr/bin/env python3
"""Generate the dossier fixtures (dossier/<scene>.npz) by RUNNING THE REFERENCE's detect_analysis.

Run in the build container only (needs the reference checkout, read-only):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_dossier.py

The reference module imports PyQt4 and matplotlib's Qt4 backend at its top, but its Plotter only ever
calls methods of the axes it is given.  Stub modules stand in for the imports and a recording axes (below,
ours) stands in for matplotlib's: every ``plot`` / ``axhline`` / ``axvline`` call of the 18 plot commands is
recorded, for every block the reference's ``ForcibleDetector`` detects among the inputs of the committed
scenes.  Stored per scene (data only, nothing of the reference's source):

    kept [K]                       block indices of the detected blocks, in feed order
    <view>|labels, |hlabels        labels of the view's lines and horizontal lines
    <view>|hlines [K, nh], |vlines [K, nv]
    <view>|<j>|len [K]             length of line j
    <view>|<j>|x, |y               the series: float64 [K, L] (NaN-padded) for lines of at most 130 points,
                                   float32 [FULL, L] for the first FULL kept blocks otherwise (longer scenes
                                   keep only the views in LONG_VIEWS, to stay below the size limit)
    fit_amplitude [K], fit_offset [K]   what the reference's two-parameter carrier fit returns
    cli_args, cli_lines, cli_kept  (scene `small`) the lines the reference's loop prints for those arguments
"""
import builtins
import os
import sys
import types

import numpy as np
import scipy

REF = os.environ.get("THRIFTY_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
builtins.xrange = range


class _Stub(types.ModuleType):
    """An importable nothing: any attribute is a class that can be subclassed and called."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (object,), {"__init__": lambda self, *a, **k: None})


for _name in ("PyQt4", "PyQt4.QtGui", "PyQt4.QtCore", "matplotlib.backends.backend_qt4agg"):
    sys.modules[_name] = _Stub(_name)
sys.modules["PyQt4"].QtGui = sys.modules["PyQt4.QtGui"]
sys.modules["PyQt4"].QtCore = sys.modules["PyQt4.QtCore"]

from thrifty import block_data, detect_analysis  # noqa: E402
from thrifty.detect import DetectorSettings  # noqa: E402
from thrifty.signal_utils import Signal  # noqa: E402

SCENES = ("small", "c2", "c2_stddev", "c1")
SAMPLE_RATE = 2.2e6
SHORT = 130                 # series of at most this many points are stored for every kept block
FULL = {"small": 2}         # kept blocks whose long series are stored (default 1)
# long series kept for the scenes of 16384-sample blocks: one of each distinct array
LONG_VIEWS = ("hist", "iq_synced", "fft", "fft_synced", "filtered_fft", "corr", "corr_zoomed")
SIZE_LIMIT = 984 * 1024     # the largest fixture committed before this one
CLI_ARGS = "-i 40-50 -m 3"


class RecordingAxes(object):
    """What a plot command draws: plot() -> lines, axhline() -> hlines, axvline() -> vlines."""

    def __init__(self):
        self.lines, self.hlines, self.vlines = [], [], []

    def plot(self, *args, **kwargs):
        if len(args) == 1:
            y = np.asarray(args[0], dtype=np.float64)
            x = np.arange(len(y), dtype=np.float64)
        else:
            x, y = (np.asarray(a, dtype=np.float64) for a in args[:2])
        self.lines.append((kwargs.get("label", ""), x, y))

    def axhline(self, y=0, **kwargs):
        self.hlines.append((kwargs.get("label", ""), float(y)))

    def axvline(self, x=0, **kwargs):
        self.vlines.append((kwargs.get("label", ""), float(x)))

    def __getattr__(self, name):      # set_xlim, legend, grid, ...: nothing to record
        return lambda *a, **k: None


def scene_settings(g):
    tpl = np.asarray(g["template"], dtype=np.float64)
    return DetectorSettings(int(g["block_len"]), int(g["history_len"]), len(tpl), tuple(g["carrier_thresh"]),
                            tuple(int(v) for v in g["carrier_window"]), tpl, tuple(g["corr_thresh"]))


def reference_loop(settings, items, ranges, max_keep):
    """The reference's _main loop (its own detector and range test) -> detections, printed lines."""
    detector = detect_analysis.ForcibleDetector(settings)
    detections, lines = [], []
    for timestamp, block_idx, block in items:
        if not detect_analysis.block_in_range(block_idx, ranges):
            continue
        lines.append("Checking block #{}".format(block_idx))
        detection = detector(timestamp, block_idx, block)
        if detection.detected:
            detections.append(detection)
            if len(detections) >= max_keep:
                break
        else:
            lines.append("Skipping block #{}".format(block_idx))
    return detections, lines


def make(scene):
    g = np.load(os.path.join(HERE, scene + ".npz"), allow_pickle=False)
    settings = scene_settings(g)
    items = [(float(i), int(b), Signal(block_data.raw_to_complex(raw)))
             for i, (b, raw) in enumerate(zip(g["block_idx"], g["blocks"]))]
    detections, _ = reference_loop(settings, items, detect_analysis.parse_range_list("0-"), len(items))
    kept = np.array([d.result.block for d in detections], dtype=np.int64)
    assert list(kept) == [int(b) for b, d in zip(g["block_idx"], g["det"]) if d], scene
    n_full = FULL.get(scene, 1)
    views = sorted(detect_analysis._PLOT_COMMAND_STRINGS)
    recorded = {v: [] for v in views}
    fit = []
    for d in detections:
        plotter = detect_analysis.Plotter(d, settings, SAMPLE_RATE)
        for v in views:
            ax = RecordingAxes()
            detect_analysis._PLOT_COMMAND_STRINGS[v](plotter, ax)
            recorded[v].append(ax)
        peak = d.result.carrier_info.bin
        fit.append(plotter.carrier_interpolator(d.unsynced.fft.mag, peak))
    out = dict(kept=kept, sample_rate=SAMPLE_RATE, views=np.array(views), n_full=n_full,
               fit_amplitude=np.array([f[0] for f in fit]), fit_offset=np.array([f[1] for f in fit]),
               versions="numpy %s scipy %s python %s" % (np.__version__, scipy.__version__, sys.version.split()[0]))
    for v in views:
        axes = recorded[v]
        first = axes[0]
        for ax in axes:     # the same drawing calls for every block
            assert [l[0] for l in ax.lines] == [l[0] for l in first.lines], (scene, v)
            assert [h[0] for h in ax.hlines] == [h[0] for h in first.hlines], (scene, v)
            assert len(ax.vlines) == len(first.vlines), (scene, v)
        out[v + "|labels"] = np.array([l[0] for l in first.lines], dtype=str)
        out[v + "|hlabels"] = np.array([h[0] for h in first.hlines], dtype=str)
        out[v + "|hlines"] = np.array([[h[1] for h in ax.hlines] for ax in axes], dtype=np.float64).reshape(len(axes), -1)
        out[v + "|vlines"] = np.array([[x[1] for x in ax.vlines] for ax in axes], dtype=np.float64).reshape(len(axes), -1)
        for j in range(len(first.lines)):
            lens = np.array([len(ax.lines[j][2]) for ax in axes], dtype=np.int64)
            out["%s|%d|len" % (v, j)] = lens
            if lens.max() <= SHORT:
                for axis, col in (("x", 1), ("y", 2)):
                    a = np.full((len(axes), lens.max()), np.nan)
                    for k, ax in enumerate(axes):
                        a[k, :lens[k]] = ax.lines[j][col]
                    out["%s|%d|%s" % (v, j, axis)] = a
            elif int(g["block_len"]) <= 4096 or v in LONG_VIEWS:
                assert np.all(lens[:n_full] == lens[0]), (scene, v)
                for axis, col in (("x", 1), ("y", 2)):
                    out["%s|%d|%s" % (v, j, axis)] = np.array([ax.lines[j][col] for ax in axes[:n_full]], dtype=np.float32)
    if scene == "small":
        ranges, max_keep = detect_analysis.parse_range_list("40-50"), 3
        dets, lines = reference_loop(settings, items, ranges, max_keep)
        out.update(cli_args=CLI_ARGS, cli_lines=np.array(lines), cli_kept=np.array([d.result.block for d in dets]))
    path = os.path.join(HERE, "dossier", scene + ".npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= SIZE_LIMIT, (scene, size)
    print("%-10s kept=%d  %d views  %.0f KiB" % (scene, len(kept), len(views), size / 1024))


if __name__ == "__main__":
    for name in SCENES:
        make(name)
