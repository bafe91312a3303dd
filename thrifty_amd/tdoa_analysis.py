"""How good are the TDOAs?  The numbers of the reference's `thrifty analyze_tdoa`, for every cell at once.

    python -m thrifty_amd.tdoa_analysis [tdoa] [--rx0 R --rx1 R --tx T] [--timestamp A-B] [--detidx A-B]
                                        [--robust] [--all] [-o stats.npz]

Per (rx0, rx1, tx) cell of a .tdoa file, on tdoa * 2.997e8 metres: bias (mean), population standard deviation
and RMS -- the reference's three lines -- and count, min and max.  With --robust the same again over the rows
that the reference's stat_tools.is_outlier keeps (modified z-score over the median absolute deviation, 3.5; a
cell of one row is left alone, as in scripts/tdoa_matrix.py).  One device call (thr_tdoastats,
csrc/syncstats.hip) covers every cell; `variance_table`, `mean_table` and `count_table` are the per-transmitter
tabulation of scripts/tdoa_matrix.py for one receiver pair, from an existing .tdoa (its re-estimation per
beacon, the beacon x transmitter matrices themselves, is `thrifty_amd.tdoa_matrix`).  No plot: `TdoaStats.cell`
gives the rows behind the reference's figure.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from thrifty_amd import _native, tdoa_est

_STAT_NAMES = ("mean", "std", "rms", "min", "max")


class TdoaStats(object):
    """The arrays of one thr_tdoastats call, one attribute per output (cell_key, cell_ptr, order, stats,
    robust_stats, robust_count, mask, median), plus `robust` and `counts`."""

    def __init__(self, counts, arrays):
        self.counts = dict(counts)
        self.robust = bool(counts["robust"])
        self.names = tuple(arrays)
        for name, value in arrays.items():
            setattr(self, name, value)

    def __len__(self):
        return len(self.cell_key)

    def index(self, rx0, rx1, tx):
        hit = np.flatnonzero(np.all(self.cell_key == (rx0, rx1, tx), axis=1))
        if len(hit) == 0:
            raise KeyError("no TDOA of TX %r between RX %r and RX %r" % (tx, rx0, rx1))
        return int(hit[0])

    def cell(self, rx0, rx1, tx):
        """One cell as a dict: count, the five statistics by name, `rows` (input rows in input order) and, with
        robust statistics, `robust` (count and the five again), `median`, `mad` and the rows' `outlier` mask."""
        c = self.index(rx0, rx1, tx)
        a, b = self.cell_ptr[c], self.cell_ptr[c + 1]
        out = {"rx0": int(rx0), "rx1": int(rx1), "tx": int(tx), "count": int(b - a), "rows": self.order[a:b]}
        out.update(zip(_STAT_NAMES, self.stats[c].tolist()))
        if self.robust:
            out["robust"] = dict(zip(_STAT_NAMES, self.robust_stats[c].tolist()), count=int(self.robust_count[c]))
            out["median"], out["mad"] = self.median[c].tolist()
            out["outlier"] = self.mask[a:b].astype(bool)
        return out

    def save(self, path):
        np.savez(path, robust=self.robust, **{name: getattr(self, name) for name in self.names})


def tdoa_stats(matrix, timestamp=None, detidx=None, robust=False, device_id=0):
    """Statistics of every (rx0, rx1, tx) cell of `matrix` (what tdoa_est.load_tdoa_matrix returns, or a dict of
    its columns); `timestamp` and `detidx` are closed (first, last) ranges, `detidx` on both detection ids.
    ValueError for an empty selection."""
    counts, arrays = _native.tdoastats(matrix, timestamp, detidx, robust, device_id=device_id)
    return TdoaStats(counts, arrays)


def format_report(stats, c, robust=False):
    """The reference's three lines for cell number `c` (of the rows the outlier mask keeps with `robust`)."""
    mean, std, rms = (stats.robust_stats if robust else stats.stats)[c, :3]
    return "TDOA bias: %.3f m\nTDOA std dev: %.3f m\nTDOA RMS: %.3f m\n" % (mean, std, rms)


def _per_tx(stats, rx0, rx1, values):
    hit = np.flatnonzero((stats.cell_key[:, 0] == rx0) & (stats.cell_key[:, 1] == rx1))
    return stats.cell_key[hit, 2], np.asarray(values)[hit]


def variance_table(stats, rx0, rx1, robust=False):
    """(txids, standard deviation in metres rounded to 0.1) of the receiver pair."""
    return _per_tx(stats, rx0, rx1, np.around((stats.robust_stats if robust else stats.stats)[:, 1], 1))


def mean_table(stats, rx0, rx1, robust=False):
    """(txids, mean in metres rounded to 0.1) of the receiver pair."""
    return _per_tx(stats, rx0, rx1, np.around((stats.robust_stats if robust else stats.stats)[:, 0], 1))


def count_table(stats, rx0, rx1, robust=False):
    """(txids, number of TDOAs) of the receiver pair."""
    return _per_tx(stats, rx0, rx1, stats.robust_count if robust else np.diff(stats.cell_ptr))


def _span(kind):
    def parse(text):
        first, last = (kind(word) for word in text.split("-"))
        return first, last
    return parse


_CLI = (
    (("tdoa",), dict(nargs="?", type=argparse.FileType("r"), default="data.tdoa", help="tdoa data ('-' streams from stdin)")),
    (("--rx0",), dict(type=int, default=0, help="receiver ID of the first receiver")),
    (("--rx1",), dict(type=int, default=1, help="receiver ID of the second receiver")),
    (("--tx",), dict(type=int, default=0, help="ID of the mobile unit")),
    (("--timestamp",), dict(type=_span(int), default=None, help="only TDOAs within a range of timestamps, A-B")),
    (("--detidx",), dict(type=_span(int), default=None, help="only TDOAs within a range of detection IDs, A-B")),
    (("--robust",), dict(action="store_true", help="also without the outliers of the modified z-score")),
    (("--all",), dict(action="store_true", help="every (rx0, rx1, tx) cell instead of one")),
    (("-o", "--output"), dict(default=None, help="save every array (.npz)")),
)


def _parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for flags, options in _CLI:
        parser.add_argument(*flags, **options)
    return parser


def _main(argv=None):
    args = _parser().parse_args(argv)
    rx0, rx1 = sorted((args.rx0, args.rx1))         # given in descending order: swapped, as the reference does
    matrix = tdoa_est.load_tdoa_matrix(args.tdoa)
    try:
        stats = tdoa_stats(matrix, args.timestamp, args.detidx, args.robust)
        cells = range(len(stats)) if args.all else [stats.index(rx0, rx1, args.tx)]
    except (ValueError, KeyError) as err:
        sys.stderr.write("%s\n" % (err.args[0] if err.args else err))
        return 1
    for c in cells:
        if args.all:
            sys.stdout.write("# TX {2} between RX {0} and RX {1}\n".format(*stats.cell_key[c]))
        sys.stdout.write(format_report(stats, c))
        if args.robust:
            sys.stdout.write("Without %d outliers:\n" % (stats.cell_ptr[c + 1] - stats.cell_ptr[c] - stats.robust_count[c]))
            sys.stdout.write(format_report(stats, c, robust=True))
    if args.output:
        stats.save(args.output)
    return 0


if __name__ == "__main__":
    sys.exit(_main())
