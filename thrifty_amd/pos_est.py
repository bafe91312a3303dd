#!/usr/bin/env python
"""
Estimate position from TDOA values.

GPU counterpart of reference thrifty/pos_est.py: every TDOA group (one mobile transmission) becomes a
position.  The solve, the snr mean and the DOP run on the device (`thr_pos`, csrc/pos.hip), one 8-lane
team per group; this module keeps the reference's names, the `.pos` text format and its command line.

With two receivers that have one coordinate the position is the reference's closed form, bit for bit.
Otherwise the sum of squared TDOA residuals is minimised from x0 = (0.1, 0.1) inside the reference's
box (the receivers' extent plus MAX_DIST per axis); a group that names fewer than three receivers
prints `Failed to estimate group #N: Underdetermined` and is dropped, as in the reference.

Deviations from the reference:

* the "first two keys" of `rx_pos` (the 1-D formula's sign depends on them) are its insertion order,
  i.e. the config file's order -- Python 3's meaning of the reference's `keys()[0]`;
* the number of dimensions is read off the first receiver (the reference reads `rx_pos[0]` in the
  solver and dies when there is no receiver 0);
* 3-D coordinates raise ValueError up front (the reference's x0 has two entries, SciPy raises on the
  shapes); so do receivers whose coordinates differ in length, and 1-D coordinates with other than two
  receivers;
* a 1-D group with more than one row raises ValueError (the reference: AssertionError);
* a receiver of any row that `rx_pos` lacks raises KeyError up front;
* a group with a NaN or infinite tdoa, or whose iterate lands on a receiver, prints
  `Failed to estimate group #N: Nonfinite` and is dropped (the reference raises from SciPy);
* the solver is not SciPy's TRF but a Levenberg-Marquardt iteration of our own that ends on the step's
  length, not on the cost: it goes to the same minimum and ends closer to it than the reference does
  (DESIGN.md 3.9).  A group that reaches `max_iter` keeps its last iterate, as the reference returns
  whatever it has.

`.pos` text: one line per position, `group_id timestamp(%.6f) tx dop snr x [y]`, floats as their
shortest round-trip repr -- what the reference's `print(*fields)` emits under Python 3 with current
numpy; under Python 2 it printed 12 significant digits.  `load_positions` reads either form.
"""
from __future__ import print_function

import argparse
import sys

import numpy as np

from thrifty_amd import _native, tdoa_est

SPEED_OF_LIGHT = tdoa_est.SPEED_OF_LIGHT

POSITION_INFO_DTYPE = {
    "names": ("group_id", "timestamp", "tx", "dop", "snr", "x", "y", "z"),
    "formats": ("i4", "f8", "i4", "f8", "f8", "f8", "f8", "f8"),
}

MAX_DIST = 10e3

STATUS_NAMES = ("OK", "UNDERDETERMINED", "UNCONVERGED", "AT_BOUND", "NONFINITE")
_DROPPED = {_native.POS_UNDERDETERMINED: "Underdetermined", _native.POS_NONFINITE: "Nonfinite"}


class EstimationError(Exception):
    pass


def _receiver_table(rx_pos):
    """(ids in insertion order, float64[n_rx, dims]); ValueError for what no solver here takes."""
    ids = list(rx_pos)
    if not ids:
        raise ValueError("rx_pos is empty")
    table = [np.atleast_1d(np.asarray(rx_pos[i], dtype=np.float64)) for i in ids]
    dims = len(table[0])
    if any(row.ndim != 1 or len(row) != dims for row in table):
        raise ValueError("the receivers' coordinates differ in length")
    if dims not in (1, 2):
        raise ValueError("%d-D receiver coordinates: positions are solved in 1 or 2 dimensions" % dims)
    if dims == 1 and len(ids) != 2:
        raise ValueError("1-D coordinates need exactly two receivers, not %d" % len(ids))
    return ids, np.array(table, dtype=np.float64).reshape(len(ids), dims)


def pos_columns(group_ptr, rx0, rx1, tdoa, snr, rx_pos, x0=(0.1, 0.1), max_iter=100, device_id=0):
    """Positions for TDOA rows in CSR form (group g: rows group_ptr[g]:group_ptr[g + 1]; rx0 / rx1 are
    receiver ids, keys of `rx_pos`) -> dict over ALL groups, in order: `pos` float64[g, dims], `dop`,
    `snr`, `status` (index into STATUS_NAMES) and `iters`.  `max_iter=0` evaluates snr and dop at x0."""
    ids, table = _receiver_table(rx_pos)
    ptr = np.asarray(group_ptr, dtype=np.int64)
    rx0, rx1 = np.asarray(rx0, dtype=np.int64), np.asarray(rx1, dtype=np.int64)
    if ptr.ndim != 1 or len(ptr) < 1 or ptr[0] != 0 or np.any(np.diff(ptr) < 0) or ptr[-1] != len(rx0):
        raise ValueError("group_ptr must start at 0, not decrease and end at the number of rows")
    dense = {rx: k for k, rx in enumerate(ids)}
    for rx in np.unique(np.concatenate([rx0, rx1])).tolist():
        if rx not in dense:
            raise KeyError(rx)
    if table.shape[1] == 1 and np.any(np.diff(ptr) != 1):
        raise ValueError("a 1-D group must hold exactly one TDOA")
    if len(ids) > _native.POS_MAX_RECEIVERS:
        raise ValueError("at most %d receivers, not %d" % (_native.POS_MAX_RECEIVERS, len(ids)))
    lookup = np.vectorize(dense.__getitem__, otypes=[np.int32])
    return _native.pos(ptr, lookup(rx0) if len(rx0) else rx0, lookup(rx1) if len(rx1) else rx1, tdoa, snr, table,
                       (0, 1), x0, max_iter, device_id)


def _one_group(tdoa_array, rx_pos):
    out = pos_columns([0, len(tdoa_array)], tdoa_array["rx0"], tdoa_array["rx1"], tdoa_array["tdoa"],
                      tdoa_array["snr"], rx_pos)
    if int(out["status"][0]) in _DROPPED:
        raise EstimationError(_DROPPED[int(out["status"][0])])
    return out["pos"][0], float(out["snr"][0])


def solve_1d(tdoa_array, rx_pos):
    """Simple 1D position estimator for 2xRX: ((x,), snr)."""
    if len(rx_pos) != 2 or any(np.size(p) != 1 for p in rx_pos.values()):
        raise ValueError("solve_1d takes two receivers with one coordinate each")
    coords, snr = _one_group(tdoa_array, rx_pos)
    return (coords[0],), snr


def solve_numerically(tdoa_array, rx_pos):
    """One group through the device's Levenberg-Marquardt solver: (array [x, y], mean snr).
    EstimationError("Underdetermined") with fewer than three distinct receivers."""
    if any(np.size(p) != 2 for p in rx_pos.values()):
        raise ValueError("solve_numerically takes 2-D receiver coordinates")
    return _one_group(tdoa_array, rx_pos)


def dop_matrix(pos, rx_pos, rx_pairs):
    """inv(G'G) for the unit-vector differences G of the receiver pairs at `pos`; None when singular."""
    pairs = list(rx_pairs)
    to_rx = [np.stack([np.atleast_1d(np.asarray(rx_pos[pair[k]], dtype=float)) for pair in pairs]) - np.asarray(pos, float)
             for k in (0, 1)]
    unit = [delta / np.sqrt(np.sum(delta * delta, axis=1, keepdims=True)) for delta in to_rx]
    geometry = unit[0] - unit[1]
    try:
        return np.linalg.inv(geometry.T @ geometry)
    except np.linalg.LinAlgError:
        return None


def dop(pos, rx_pos, rx_pairs):
    matrix = dop_matrix(pos, rx_pos, rx_pairs)
    return -1 if matrix is None else np.sqrt(np.trace(matrix))


def _result_dtype(dims):
    return {"names": POSITION_INFO_DTYPE["names"][:5 + dims], "formats": POSITION_INFO_DTYPE["formats"][:5 + dims]}


def solve(tdoa_groups, rx_pos, max_iter=100):
    """Positions of all TDOA groups (group_id, timestamp, tx, tdoas) in one device call -> structured
    array (POSITION_INFO_DTYPE cut to the dimensions), one record per solved group, in order."""
    groups = list(tdoa_groups)
    _, table = _receiver_table(rx_pos)
    dims = table.shape[1]
    ptr = np.cumsum([0] + [len(group[3]) for group in groups])
    column = lambda name, kind: (np.concatenate([np.asarray(group[3][name], dtype=kind) for group in groups])  # noqa: E731
                                 if groups else np.zeros(0, dtype=kind))
    out = pos_columns(ptr, column("rx0", np.int64), column("rx1", np.int64), column("tdoa", np.float64),
                      column("snr", np.float64), rx_pos, max_iter=max_iter)
    status = out["status"]
    for g in np.flatnonzero(np.isin(status, list(_DROPPED))).tolist():
        print("Failed to estimate group #{}: {}".format(groups[g][0], _DROPPED[int(status[g])]))
    keep = ~np.isin(status, list(_DROPPED))
    results = np.zeros(int(keep.sum()), dtype=_result_dtype(dims))
    results["group_id"] = [group[0] for group, k in zip(groups, keep) if k]
    results["timestamp"] = [group[1] for group, k in zip(groups, keep) if k]
    results["tx"] = [group[2] for group, k in zip(groups, keep) if k]
    results["dop"], results["snr"] = out["dop"][keep], out["snr"][keep]
    for axis, name in enumerate(("x", "y")[:dims]):
        results[name] = out["pos"][keep, axis]
    return results


def save_positions(output, results):
    """One line per position (see the module docstring); `output` is a file name or an open text file."""
    if isinstance(output, str):
        with open(output, "w") as handle:
            return save_positions(handle, results)
    for record in results:
        words = [str(int(record["group_id"])), "%.6f" % record["timestamp"], str(int(record["tx"]))]
        words += [repr(float(record[name])) for name in results.dtype.names[3:]]
        output.write(" ".join(words) + "\n")


def load_positions(fname):
    """The records of a .pos file; the number of columns says how many coordinates there are."""
    if isinstance(fname, str):
        with open(fname, "r") as handle:
            return load_positions(handle)
    rows = [line.decode() if isinstance(line, bytes) else line for line in fname]
    rows = [line.split() for line in rows if line.strip() and not line.lstrip().startswith("#")]
    dims = len(rows[0]) - 5 if rows else 2
    dtype = _result_dtype(dims)
    data = np.zeros(len(rows), dtype=dtype)
    for r, words in enumerate(rows):
        data[r] = tuple(float(w) if fmt == "f8" else int(w) for w, fmt in zip(words, dtype["formats"]))
    return data


_CLI = (
    (("tdoa",), dict(nargs="?", type=argparse.FileType("r"), default="data.tdoa",
                     help="tdoa data (\"-\" streams from stdin)")),
    (("-o", "--output"), dict(dest="output", type=argparse.FileType("w"), default="data.pos",
                              help="output file ('-' for stdout)")),
    (("-r", "--rx-coordinates"), dict(dest="rx_pos", type=argparse.FileType("r"), default="pos-rx.cfg",
                                      help="path to config file that contains the coordinates of the receivers")),
)


def _parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for flags, options in _CLI:
        parser.add_argument(*flags, **options)
    return parser


def _main(argv=None):
    args = _parser().parse_args(argv)
    try:
        tdoa_groups = tdoa_est.load_tdoa_groups(args.tdoa)
        rx_pos = tdoa_est.load_pos_config(args.rx_pos)
        save_positions(args.output, solve(tdoa_groups, rx_pos))
    finally:
        for stream in (args.tdoa, args.rx_pos):
            if stream is not sys.stdin:
                stream.close()
        if args.output is sys.stdout:
            args.output.flush()
        else:
            args.output.close()


if __name__ == "__main__":
    _main()
