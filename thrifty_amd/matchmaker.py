#!/usr/bin/env python
"""
Match detections from the same transmitter detected by multiple receivers.

GPU counterpart of reference thrifty/matchmaker.py: detections of one txid that fall inside a
timestamp window form a group, every receiver contributes one detection to it (its strongest; later
ones win ties), and a group that enough receivers saw is a match.  Grouping, the per-receiver
selection and the output orders run on the device (`thr_match`, csrc/match.hip); this module keeps the
reference's function names and the `.match` text format on top of it.

One deviation: the detections must be in timestamp order (no NaN) -- the reference returns an
order-dependent result otherwise, this module raises ValueError.
"""
from __future__ import print_function

import argparse
import sys

import numpy as np

from thrifty_amd import _native, toads_data


def _columns(toads):
    n = len(toads)
    cols = {"rxid": np.empty(n, np.int32), "txid": np.empty(n, np.int32),
            "timestamp": np.empty(n, np.float64), "energy": np.empty(n, np.float64)}
    for i, d in enumerate(toads):
        cols["rxid"][i] = -1 if d.rxid is None else d.rxid
        cols["txid"][i] = -1 if d.txid is None else d.txid
        cols["timestamp"][i] = d.timestamp
        cols["energy"][i] = d.corr_info.energy
    return cols


def match_columns(cols, window, min_match=2, device_id=0):
    """-> (match_ptr, match_idx, misses, collisions[k, 2]), int64, for detection columns
    (rxid, txid, timestamp, energy) in timestamp order; match m is match_idx[match_ptr[m]:match_ptr[m + 1]]."""
    return _native.match(cols["rxid"], cols["txid"], cols["timestamp"], cols["energy"], window, min_match, device_id)


def match_toads(toads, window, min_match=2):
    """(matches, misses, collisions) for detections sorted by timestamp: lists of detection indices, one
    per transmission at least `min_match` receivers saw; the first detection of every transmission too
    few saw; the (kept so far, further) pairs of detections one receiver has for one transmission."""
    ptr, idx, misses, collisions = match_columns(_columns(toads), window, min_match)
    ptr, idx = ptr.tolist(), idx.tolist()
    return ([idx[a:b] for a, b in zip(ptr[:-1], ptr[1:])], misses.tolist(),
            [tuple(pair) for pair in collisions.tolist()])


def load_matches(file_):
    """Matches of a .match file (name or open file): one line of indices each; '#' and empty lines skipped."""
    if isinstance(file_, str):
        with open(file_, "r") as handle:
            return load_matches(handle)
    rows = (line.decode() if isinstance(line, bytes) else line for line in file_)
    return [[int(word) for word in row.split()] for row in rows if row.strip() and not row.startswith("#")]


def save_matches(matches, file_):
    """One line per match: its detection indices, space-separated."""
    file_.write("".join(" ".join("%d" % index for index in match) + "\n" for match in matches))


def extract_match_matrix(detections, matches, rxids, txids=None):
    """Rows [index at rxids[0], index at rxids[1], ...] of the matches that hold every receiver of
    `rxids` (and whose transmitter is in `txids`, if given)."""
    wanted = None if txids is None or not len(rxids) else set(txids)
    matrix = []
    for match in matches:
        at = {}
        for index in match:
            at.setdefault(detections[index].rxid, index)
        if all(rx in at for rx in rxids) and (wanted is None or detections[match[0]].txid in wanted):
            matrix.append([at[rx] for rx in rxids])
    return matrix


_CLI = (
    (("input",), dict(nargs="?", type=argparse.FileType("r"), default="data.toads",
                      help=".toads data ('-' streams from stdin) [default: data.toads]")),
    (("-o", "--output"), dict(dest="output", type=argparse.FileType("w"), default="data.match",
                              help="output file ('-' for stdout) [default: data.match]")),
    (("-w", "--window"), dict(dest="window", type=float, default=0.2, help="size of timestamp window in seconds")),
    (("-n", "--num-matches"), dict(dest="num_matches", type=int, default=2,
                                   help="minimum number of receivers that should detect a transmission "
                                        "for a match to be valid")),
    (("-v", "--verbose"), dict(action="store_true", help="Increase output verbosity")),
)
_COLLIDES = "Multiple detections for RX %d and TX %d: detection #%d and #%d collides."     # (the reference's sentence)


def _parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for flags, options in _CLI:
        parser.add_argument(*flags, **options)
    return parser


def _main(argv=None):
    args = _parser().parse_args(argv)
    try:
        toads = sorted(toads_data.load_toads(args.input), key=lambda det: det.timestamp)     # stable
        cols = _columns(toads)
        ptr, idx, misses, collisions = match_columns(cols, args.window, args.num_matches)
        if args.verbose:
            for kept, other in collisions.tolist():
                print(_COLLIDES % (cols["rxid"][kept], cols["txid"][kept], kept, other))
        print("Number of matches:", len(ptr) - 1)
        print("Number of misses:", len(misses))
        print("Number of collisions:", len(collisions))
        ptr, idx = ptr.tolist(), idx.tolist()
        save_matches([idx[a:b] for a, b in zip(ptr[:-1], ptr[1:])], args.output)
    finally:
        if args.input is not sys.stdin:
            args.input.close()
        if args.output is sys.stdout:        # '-': the caller's stream, flushed and left open
            args.output.flush()
        else:
            args.output.close()


if __name__ == "__main__":
    _main()
