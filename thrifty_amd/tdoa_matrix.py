"""Which beacon is off?  The numbers of the reference's scripts/tdoa_matrix.py, for every (rx0 < rx1, beacon,
transmitter) cell of a deployment in one device call.

    python -m thrifty_amd.tdoa_matrix [toads] [matches] --beacons B [B ...] [--tx T ...] [--rx R ...]
                                      [--rx0 R --rx1 R | --all] [-w 4] [-s 2.4e6] [--model M --deg D]
                                      [-r pos-rx.cfg -b pos-beacon.cfg] [-o tdoa_matrix.npz]

`thrifty tdoa` ties two receivers' clocks together with every beacon in the window at once; a beacon whose position
is wrong, or that one receiver hears through multipath, bends every TDOA a little and `analyze_tdoa` shows a bias
without a culprit.  Here the TDOAs of every transmitter are estimated again, once per beacon, with the matches of that
beacon ALONE as the clock model (thr_tdoamatrix, csrc/tdoamatrix.hip: thr_tdoa_model's arithmetic per task), a
second outlier mask runs over the TDOAs of a cell, and per receiver pair a beacon x transmitter matrix of standard
deviation, mean and count comes out.  A column that disagrees between the beacon rows names the beacon; a beacon
measured against another beacon has a known answer, which is the real test of the synchronisation.

What is reproduced: `calculate_tdoas` (the extraction of one detection per receiver per match, the rule of at least
three matches of the beacon and of the transmitter, `estimate_tdoas` with window 4 and the zero geometry, the
`is_outlier` mask when there is more than one TDOA) and the three tables of `print_tdoa_matrix`, rounded as it
rounds.  Not here: the plots, `tabulate`, the hard-wired `range(4)` receivers and `range(5)` transmitters (the lists
are arguments), the `timeval` / `--now` cut, the match step inside the script (this module reads `data.match`), and
its count and mean-peak tables (they are `toads_analysis`'s).

Without `-r` / `-b` the geometry is the script's zeros: a cell's mean is the transmitter's TDOA minus the beacon's.
With them the real `beacon_sdoa` is used, and a cell's mean is the transmitter's own TDOA.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from thrifty_amd import _native, matchmaker, tdoa_est, toads_data
from thrifty_amd.beacon_analysis import _as_csr

LIGHT = 2.997e8
CELL_TOO_FEW = _native.TDMAT_CELL_TOO_FEW
OK, NO_MODEL, OUT_OF_RANGE, SKIPPED = _native.TDMAT_OK, _native.TDMAT_NO_MODEL, _native.TDMAT_OUT_OF_RANGE, _native.TDMAT_SKIPPED
MAX_BEACONS = _native.TDMAT_MAX_BEACONS


class TdoaMatrices(object):
    """The arrays of one thr_tdoamatrix call, one attribute per output (_native.TDMAT_OUTPUTS), plus `counts`,
    `beacons` (ascending), `model`, `deg`, `window` and `sample_rate`."""

    def __init__(self, counts, arrays, beacons, model="poly", deg=2, window=4.0, sample_rate=2.4e6):
        self.counts = dict(counts)
        self.names = tuple(arrays)
        for name, value in arrays.items():
            setattr(self, name, value)
        self.beacons = sorted(int(b) for b in beacons)
        self.model, self.deg, self.window, self.sample_rate = str(model), int(deg), float(window), float(sample_rate)

    def __len__(self):
        return len(self.cell_key)

    @property
    def cells(self):
        """[(rx0, rx1, beacon, tx)] in the order of the arrays."""
        return [tuple(key) for key in self.cell_key.tolist()]

    @property
    def pairs(self):
        """[(rx0, rx1)] that have a cell, ascending."""
        return sorted(set((int(k[0]), int(k[1])) for k in self.cell_key.tolist()))

    def index(self, rx0, rx1, beacon, tx):
        hit = np.flatnonzero(np.all(self.cell_key == (rx0, rx1, beacon, tx), axis=1))
        if len(hit) == 0:
            raise KeyError("no match of transmitter %r holds receivers %r and %r (beacon %r)" % (tx, rx0, rx1, beacon))
        return int(hit[0])

    def cell(self, rx0, rx1, beacon, tx):
        """One cell as a dict: the counts, the statistics (metres), median and MAD (seconds), and per task the
        `timestamp`, `tdoa` (seconds) and `outlier` rows behind the script's plot, with `status`, `n_window`,
        `n_kept`, `snr`, `model_quality`, `rows` (the two detections) and `matches`."""
        c = self.index(rx0, rx1, beacon, tx)
        a, b = self.cell_ptr[c:c + 2]
        out = {"rx0": int(rx0), "rx1": int(rx1), "beacon": int(beacon), "tx": int(tx), "flags": int(self.cell_flags[c]),
               "too_few": bool(self.cell_flags[c] & CELL_TOO_FEW), "rows": self.task_det[a:b], "matches": self.task_match[a:b],
               "timestamp": self.timestamp[a:b], "tdoa": self.tdoa[a:b], "outlier": self.outlier[a:b] != 0,
               "status": self.status[a:b], "n_window": self.n_window[a:b], "n_kept": self.n_kept[a:b], "snr": self.snr[a:b],
               "model_quality": self.model_quality[a:b]}
        out.update(zip(("beacon_rows", "tx_rows", "tdoas", "failures", "kept"), self.cell_counts[c].tolist()))
        out.update(zip(("mean", "std", "rms", "min", "max"), self.cell_stats[c].tolist()))
        out.update(zip(("median", "mad"), self.medians[c].tolist()))
        return out

    def _table(self, rx0, rx1, values, kind):
        sel = np.flatnonzero((self.cell_key[:, 0] == rx0) & (self.cell_key[:, 1] == rx1))
        beacons = np.array(self.beacons, dtype=np.int64)
        txids = np.unique(np.concatenate([self.cell_key[sel, 3].astype(np.int64), beacons]))
        table = np.zeros((len(beacons), len(txids)), dtype=kind)
        table[np.searchsorted(beacons, self.cell_key[sel, 2]), np.searchsorted(txids, self.cell_key[sel, 3])] = values[sel]
        return beacons, txids, table

    def _rounded(self, column):
        kept = self.cell_counts[:, 4] > 0
        return np.where(kept, np.around(np.where(kept, self.cell_stats[:, column], 0.0), 1), 0.0)

    def variance_table(self, rx0, rx1):
        """(beacons, txids, float64[beacons][txids]): the standard deviation of the kept TDOAs in metres, rounded to
        0.1 as the script rounds (its "variance matrix"); 0.0 for a cell without a kept TDOA and where there is none."""
        return self._table(rx0, rx1, self._rounded(1), np.float64)

    def mean_table(self, rx0, rx1):
        """(beacons, txids, float64[beacons][txids]): the mean of the kept TDOAs in metres, rounded to 0.1; 0.0 as above."""
        return self._table(rx0, rx1, self._rounded(0), np.float64)

    def count_table(self, rx0, rx1):
        """(beacons, txids, int64[beacons][txids]): the kept TDOAs; 0 as above."""
        return self._table(rx0, rx1, self.cell_counts[:, 4], np.int64)

    def format_report(self, rx0, rx1):
        return format_report(self, rx0, rx1)

    def save(self, path):
        np.savez(path, beacons=np.array(self.beacons, np.int32), model=self.model, deg=self.deg, window=self.window,
                 sample_rate=self.sample_rate, **{name: getattr(self, name) for name in self.names})


def _as_columns(detections):
    if isinstance(detections, dict):
        return detections
    if not isinstance(detections, np.ndarray):
        detections = toads_data.toads_array(list(detections), with_ids=True)
    return {name: detections[name] for name, _ in _native.TDMAT_COLUMNS}


def _distance(a, b):
    delta = np.asarray(a, dtype=float) - np.asarray(b, dtype=float)
    return np.sqrt(np.sum(delta ** 2))


def tdoa_matrices(detections, matches, beacons, receivers=None, targets=None, window=4.0, sample_rate=2.4e6, model="poly",
                  deg=2, rx_pos=None, beacon_pos=None, device_id=0):
    """The per-beacon TDOA matrices of every (rx0 < rx1, beacon, transmitter) cell -> TdoaMatrices.  `detections`:
    DetectionResult objects, a toads_array, or a dict of the columns rxid, txid, timestamp, soa, energy, noise;
    `matches`: lists of detection indices, or (match_ptr, match_idx); `beacons`: the beacons' transmitter ids (at most
    MAX_BEACONS); `receivers`: None for all; `targets`: None for every transmitter present, the beacons included;
    `model`: a name of tdoa_est.MODELS; `rx_pos` and `beacon_pos` ({id: coordinates in metres}, both or neither): the
    real geometry instead of the script's zeros.  ValueError for what thr_tdoamatrix refuses."""
    cols = _as_columns(detections)
    ptr, idx = _as_csr(matches)
    if model not in _native.TDOA_MODELS:
        raise ValueError("tdoa_matrices: model must be one of %s, not %r" % (", ".join(sorted(_native.TDOA_MODELS)), model))
    beacons = [int(b) for b in np.atleast_1d(beacons).tolist()]
    if (rx_pos is None) != (beacon_pos is None):
        raise ValueError("tdoa_matrices: rx_pos and beacon_pos come together")
    dist = None
    if rx_pos is not None:
        if receivers is None:
            receivers = sorted(set(np.asarray(cols["rxid"])[idx].tolist()))
        receivers = [int(r) for r in np.atleast_1d(receivers).tolist()]
        dist = np.array([[_distance(rx_pos[r], beacon_pos[b]) for b in beacons] for r in receivers],
                        dtype=np.float64).reshape(len(receivers), len(beacons))
    counts, arrays = _native.tdoamatrix(cols, ptr, idx, beacons, receivers, targets, dist, window, sample_rate,
                                        _native.TDOA_MODELS[model], deg, device_id=device_id)
    return TdoaMatrices(counts, arrays, beacons, model, deg, window, sample_rate)


def format_table(title, beacons, txids, table):
    """Plain aligned text in the layout of toads_analysis.format_table: a title line, a header of transmitter ids, one
    row per beacon."""
    rows = [["v beacon/tx >"] + [str(t) for t in txids]] + [[str(b)] + [str(v) for v in row] for b, row in zip(beacons, table.tolist())]
    widths = [max(len(row[k]) for row in rows) for k in range(len(rows[0]))]
    lines = ["  ".join(word.rjust(w) for word, w in zip(row, widths)) for row in rows]
    lines.insert(1, "  ".join("-" * w for w in widths))
    return title + "\n" + "\n".join(lines) + "\n"


def format_report(result, rx0, rx1):
    """The script's three headed tables for one receiver pair."""
    out = "# TDOA matrices for RX {} and RX {}\n".format(rx0, rx1)
    out += format_table("# TDOA variance matrix for {} and {}:".format(rx0, rx1), *result.variance_table(rx0, rx1)) + "\n"
    out += format_table("# TDOA mean matrix for {} and {}:".format(rx0, rx1), *result.mean_table(rx0, rx1)) + "\n"
    out += format_table("# TDOA count matrix for {} and {}:".format(rx0, rx1), *result.count_table(rx0, rx1)) + "\n\n"
    return out


_CLI = (
    (("toads",), dict(nargs="?", type=argparse.FileType("rb"), default="data.toads", help="toads data ('-' streams from stdin)")),
    (("matches",), dict(nargs="?", type=argparse.FileType("rb"), default="data.match", help="match data")),
    (("--beacons",), dict(type=int, nargs="+", required=True, help="transmitter IDs of the beacons")),
    (("--tx",), dict(type=int, nargs="+", default=None, help="transmitter IDs of the columns [default: every one present]")),
    (("--rx",), dict(type=int, nargs="+", default=None, help="receiver IDs [default: every one present]")),
    (("--rx0",), dict(type=int, default=None, help="receiver ID of the first receiver (with --rx1: one pair)")),
    (("--rx1",), dict(type=int, default=None, help="receiver ID of the second receiver")),
    (("--all",), dict(action="store_true", help="every pair of the receivers [the default without --rx0 / --rx1]")),
    (("-w", "--window-size"), dict(dest="window_size", type=float, default=4.0,
                                   help="largest difference in timestamp between a beacon transmission and the transmission "
                                        "it helps to estimate [default: the script's 4]")),
    (("-s", "--sample-rate"), dict(dest="sample_rate", type=float, default=2.4e6, help="nominal sample rate of receivers")),
    (("--model",), dict(choices=("poly", "weighted_poly", "nearest", "linear"), default="poly",
                        help="clock model built from the beacon's transmissions in the window [default: poly]")),
    (("--deg",), dict(type=int, default=2, help="degree of the two polynomial models (1..3)")),
    (("-r", "--rx-coordinates"), dict(dest="rx_pos", default=None, help="config file with the receivers' coordinates")),
    (("-b", "--beacon-coordinates"), dict(dest="beacon_pos", default=None, help="config file with the beacons' coordinates")),
    (("-o", "--output"), dict(default=None, help="save every array (.npz)")),
)


def _parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for flags, options in _CLI:
        parser.add_argument(*flags, **options)
    return parser


def _selection(parser, args):
    """The receiver list of the call: --rx0 / --rx1 name one pair, --all (or neither) every pair of --rx."""
    if (args.rx0 is None) != (args.rx1 is None):
        parser.error("--rx0 and --rx1 come together")
    if args.rx0 is not None:
        if args.all or args.rx is not None:
            parser.error("--rx0 / --rx1 name one pair: not with --all or --rx")
        if args.rx0 == args.rx1:
            parser.error("--rx0 and --rx1 are two receivers")
        return sorted((args.rx0, args.rx1))
    return args.rx


def _main(argv=None):
    parser = _parser()
    args = parser.parse_args(argv)
    receivers = _selection(parser, args)
    if (args.rx_pos is None) != (args.beacon_pos is None):
        parser.error("-r and -b come together")
    detections = toads_data.toads_array(toads_data.load_toads(args.toads), with_ids=True)
    matches = matchmaker.load_matches(args.matches)
    positions = {name: tdoa_est.load_pos_config(path) if path else None
                 for name, path in (("rx_pos", args.rx_pos), ("beacon_pos", args.beacon_pos))}
    try:
        result = tdoa_matrices(detections, matches, args.beacons, receivers=receivers, targets=args.tx, window=args.window_size,
                               sample_rate=args.sample_rate, model=args.model, deg=args.deg, **positions)
    except ValueError as err:
        sys.stderr.write("%s\n" % err)
        return 1
    for rx0, rx1 in result.pairs:
        sys.stdout.write(format_report(result, rx0, rx1))
    if args.output:
        result.save(args.output)
    return 0


if __name__ == "__main__":
    sys.exit(_main())
