"""Detection statistics of a .toads file: the numbers of the reference's `thrifty analyze_toads`.

    python -m thrifty_amd.toads_analysis [-i data.toads] [-m data.match] [--toad] [-o stats.npz]

Per (receiver, transmitter) cell: count, mean, population std, min and max of carrier peak / noise / SNR,
carrier bin and offset, correlation peak / noise / SNR and offset; detections per minute; the carrier-bin
histogram; numpy.histogram(offset, 10).  Per receiver: the straight line timestamp ~ a * soa + b (1 / a is
the receiver's sample rate against its system clock) with every row's residual, the residuals' population
std and their largest magnitude.  Everything is computed on the device in one call (thr_toadstats,
csrc/toadstats.hip); the report printed is the reference's text (toads_analysis.py: print_rxtx_stats).
No plots: the numbers behind the reference's figures are arrays of `ToadStats` (and of the `-o` file).

Deviations from the reference, each with a test (tests/test_gpu_toadstats*.py):
 - `--toad` input (no id columns) is one cell (-1, -1); the reference's split raises there;
 - an empty selection is a ValueError that says so (the reference's np.min raises an unrelated one);
 - a cell with a non-finite `offset` gets NaN edges, a zero histogram and a flag (np.histogram raises);
 - a receiver with fewer than two distinct `soa` gets a NaN line and NaN residuals;
 - a non-finite timestamp in the selection, a match index out of range or repeated, and histograms that
   would together exceed 2^26 counters (a stray timestamp years away) are ValueErrors;
 - the line is fitted in u = (soa - mean) / max|soa - mean| on timestamp - mean, not on the raw Vandermonde
   matrix of np.polyfit: same line, more digits;
 - minutes are floor(timestamp / 60) (one float64 division), where the reference's floor_divide goes through fmod.
Two tables of the reference's scripts/tdoa_matrix.py come from the same numbers: `count_table`,
`mean_energy_table`; `match_length_histogram` needs the matches only.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from thrifty_amd import _native, matchmaker, toads_data

QUANTITIES = _native.TSTATS_QUANTITIES
# the report: label, quantity, formats of mean / std / min / max (the reference's print_stats)
_REPORT = (
    ("Carrier peak", 0, ".1f", ".2f", ".1f", ".1f"),
    ("Carrier noise", 1, ".1f", ".2f", ".1f", ".1f"),
    ("Carrier SNR (dB)", 2, ".1f", ".2f", ".1f", ".1f"),
    ("Carrier bin", 3, ".0f", ".3f", ".0f", ".0f"),
    ("Carrier offset", 4, ".3f", ".3f", ".3f", ".3f"),
    ("Corr peak", 5, ".1f", ".2f", ".1f", ".1f"),
    ("Corr noise", 6, ".1f", ".2f", ".1f", ".1f"),
    ("Corr SNR (dB)", 7, ".1f", ".2f", ".1f", ".1f"),
    ("Corr offset", 8, ".3f", ".3f", ".3f", ".3f"),
)
_STAT_NAMES = ("mean", "std", "min", "max")
_CELL_HEADER = "# Stats for RX #{}'s detections of TX #{}'s transmissions:\n"


class ToadStats(object):
    """The arrays of one thr_toadstats call, one attribute per output (cell_rx, cell_tx, cell_ptr, order,
    stats, snr_db, minute_ptr, minute_hist, bin_first, bin_ptr, bin_hist, offset_edges, offset_hist,
    cell_flags, rx_id, rx_count, rx_fit, residual), plus `time0` and `counts`."""

    def __init__(self, counts, arrays):
        self.counts = dict(counts)
        self.time0 = counts["time0"]
        self.names = tuple(arrays)
        for name, value in arrays.items():
            setattr(self, name, value)

    def __len__(self):
        return len(self.cell_rx)

    def index(self, rx, tx):
        hit = np.flatnonzero((self.cell_rx == rx) & (self.cell_tx == tx))
        if len(hit) == 0:
            raise KeyError("no detections of TX %r at RX %r" % (tx, rx))
        return int(hit[0])

    def cell(self, rx, tx):
        """Everything about one (receiver, transmitter) pair as a dict: count, the nine quantities' stats by
        name, `rows` (input indices in input order: the cell's time series) and the three histograms."""
        c = self.index(rx, tx)
        rows = self.order[self.cell_ptr[c]:self.cell_ptr[c + 1]]
        out = {"rx": int(rx), "tx": int(tx), "count": len(rows), "rows": rows, "flags": int(self.cell_flags[c]),
               "minute_hist": self.minute_hist[self.minute_ptr[c]:self.minute_ptr[c + 1]],
               "bin_first": int(self.bin_first[c]), "bin_hist": self.bin_hist[self.bin_ptr[c]:self.bin_ptr[c + 1]],
               "offset_edges": self.offset_edges[c], "offset_hist": self.offset_hist[c]}
        for q, name in enumerate(QUANTITIES):
            out[name] = dict(zip(_STAT_NAMES, self.stats[c, q].tolist()))
        return out

    def save(self, path):
        np.savez(path, time0=np.float64(self.time0), **{name: getattr(self, name) for name in self.names})


def _as_columns(detections):
    """The eleven columns from a dict of columns, a toads_array, or a sequence of DetectionResult."""
    if isinstance(detections, dict):
        return detections
    if not isinstance(detections, np.ndarray):
        detections = list(detections)
        with_ids = any(d.rxid is not None or d.txid is not None for d in detections)
        detections = toads_data.toads_array(detections, with_ids=with_ids)
    return {name: detections[name] for name, _ in _native.TSTATS_COLUMNS}


def toad_stats(detections, matches=None, device_id=0):
    """Statistics of `detections` (DetectionResult objects, a toads_array, or a dict of the eleven columns);
    with `matches` (lists of detection indices) only of the matched ones.  ValueError for an empty selection,
    a non-finite timestamp, or match indices that are out of range or repeated."""
    sel = None
    if matches is not None:
        sel = np.sort(np.concatenate([np.asarray(m, dtype=np.int64) for m in matches] + [np.zeros(0, dtype=np.int64)]))
    counts, arrays = _native.toadstats(_as_columns(detections), sel, device_id=device_id)
    return ToadStats(counts, arrays)


def format_cell(stats, c):
    """The reference's ten lines for cell number `c`."""
    lines = ["Number of detections: {}".format(int(stats.cell_ptr[c + 1] - stats.cell_ptr[c]))]
    for label, q, *formats in _REPORT:
        parts = ("{}={:{}}".format(name, value, fmt) for name, value, fmt in zip(_STAT_NAMES, stats.stats[c, q], formats))
        lines.append(label + ": " + ", ".join(parts))
    return "\n".join(lines) + "\n"


def format_stats(stats):
    """The whole report: the time origin, then per cell the header, a blank line, the ten lines, two blank lines."""
    text = ["Timestamps relative to {:.6f}\n".format(stats.time0)]
    for c in range(len(stats)):
        text += [_CELL_HEADER.format(stats.cell_rx[c], stats.cell_tx[c]), "\n", format_cell(stats, c), "\n\n"]
    return "".join(text)


def _table(stats, value):
    rxids, txids = np.unique(stats.cell_rx), np.unique(stats.cell_tx)
    table = np.zeros((len(txids), len(rxids)), dtype=np.int64)
    table[np.searchsorted(txids, stats.cell_tx), np.searchsorted(rxids, stats.cell_rx)] = value
    return txids, rxids, table


def count_table(stats):
    """(txids, rxids, int64[transmitters][receivers]): detections per pair."""
    return _table(stats, np.diff(stats.cell_ptr))


def mean_energy_table(stats):
    """(txids, rxids, int64[transmitters][receivers]): int(mean correlation peak), 0 for an empty pair."""
    return _table(stats, [int(v) for v in stats.stats[:, 5, 0]])


def match_length_histogram(matches):
    """{receivers in a match: number of such matches}, by length."""
    lengths, counts = np.unique([len(m) for m in matches], return_counts=True)
    return dict(zip(lengths.tolist(), counts.tolist()))


def format_table(title, txids, rxids, table):
    """Plain aligned text: a title line, a header of receiver ids, one row per transmitter."""
    rows = [["v TX / RX >"] + [str(r) for r in rxids]] + [[str(t)] + [str(v) for v in row]
                                                          for t, row in zip(txids, table.tolist())]
    widths = [max(len(row[k]) for row in rows) for k in range(len(rows[0]))]
    lines = ["  ".join(word.rjust(w) for word, w in zip(row, widths)) for row in rows]
    lines.insert(1, "  ".join("-" * w for w in widths))
    return title + "\n" + "\n".join(lines) + "\n"


_CLI = (
    (("--toad",), dict(dest="toad", action="store_true", help="input data is .toad data instead of .toads")),
    (("-i", "--input"), dict(type=argparse.FileType("rb"), default="data.toads",
                             help=".toads data ('-' streams from stdin)")),
    (("-m", "--match"), dict(type=argparse.FileType("rb"), default=None, help="exclude unmatched detections")),
    (("-o", "--output"), dict(default=None, help="save every array of the statistics (.npz)")),
)


def _parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for flags, options in _CLI:
        parser.add_argument(*flags, **options)
    return parser


def _main(argv=None):
    args = _parser().parse_args(argv)
    load = toads_data.load_toad if args.toad else toads_data.load_toads
    detections = toads_data.toads_array(load(args.input), with_ids=not args.toad)
    matches = matchmaker.load_matches(args.match) if args.match else None
    stats = toad_stats(detections, matches)
    sys.stdout.write(format_stats(stats))
    if args.output:
        stats.save(args.output)
    return 0


if __name__ == "__main__":
    sys.exit(_main())
