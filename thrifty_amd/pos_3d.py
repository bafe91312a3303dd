#!/usr/bin/env python
"""
Estimate position from TDOA values when the receivers' antennas sit at different heights.

    python -m thrifty_amd.pos_3d [data.tdoa] -r pos-rx.cfg -o data.pos
           (--height H [--height-tx TX=H ...] | --free-z [--z0 Z] [--z-range LO HI]) [--npz FILE]

`pos-rx.cfg` is `id: x y z` here.  `thrifty_amd.pos_est` (the reference's `thrifty pos`) solves in a plane and
refuses such a table; dropping the heights from it biases every position by metres (README, "Receivers at
different heights?").  One device call (`thr_pos3`, csrc/pos3.hip; include/thrifty_hip.h states every rule), the
iteration of `thr_pos` with three-dimensional ranges, in one of two modes -- there is no default, because the height
is the deployment's:

* `--height` / `height=`: the transmitter's height is KNOWN (a collar, a vehicle roof, a beacon on a mast) and
  (x, y) are solved for.  As well conditioned as the planar problem, and what a deployment uses daily.  `height` is
  one number, a `{tx: height}` dict, or one value per group.  The records are `thrifty pos`' own 2-D records
  (`group_id timestamp tx dop snr x y`), so `track`, `load_positions` and the reference's tools read them unchanged;
  `dop` is the horizontal dilution given the height.  A group that names fewer than three receivers prints
  `Failed to estimate group #N: Underdetermined` and is dropped.
* `--free-z` / `free_z=True`: (x, y, z) are solved for, inside the reference's box per axis (the receivers' extent
  plus MAX_DIST) or `z_range` on z.  It needs four receivers, and antenna heights that really differ: the vertical
  error grows with cond(G'G), which `vdop` reports per position.  The records add `z` (the reference's dtype), `dop`
  is the reference's `dop()` in three dimensions; `--npz` keeps hdop and vdop.
  The start's height `z0` defaults to the middle of `z_range` when one is given and otherwise to 1 m below the
  lowest receiver.  That is a convention ("the transmitter is below the antennas"), not a measurement: the cost has
  a second, mirrored minimum on the other side of the antennas where they are nearly coplanar, and the start picks
  the side.  Where every receiver has the same height the mirror is exact; a `z0` ON that plane is refused.

A group with a NaN or infinite tdoa, or whose iterate lands on a receiver, prints `Failed to estimate group #N:
Nonfinite` and is dropped, as in `pos_est.solve`.  `--npz FILE` keeps, for ALL groups in order, group_id, pos, dop,
hdop, vdop, rms (the r.m.s. residual in metres), snr, status and iters.
"""
from __future__ import print_function

import argparse
import sys

import numpy as np

from thrifty_amd import _native, pos_est, tdoa_est

MAX_DIST = pos_est.MAX_DIST
STATUS_NAMES = pos_est.STATUS_NAMES
BELOW_LOWEST = 1.0      # the default start is this far below the lowest receiver [m]: a convention
_DROPPED = {_native.POS_UNDERDETERMINED: "Underdetermined", _native.POS_NONFINITE: "Nonfinite"}


def _receiver_table(rx_pos):
    """(ids in insertion order, float64[n_rx, 3]); ValueError for any other table."""
    ids = list(rx_pos)
    if not ids:
        raise ValueError("rx_pos is empty")
    table = [np.atleast_1d(np.asarray(rx_pos[i], dtype=np.float64)) for i in ids]
    if any(row.ndim != 1 or len(row) != 3 for row in table):
        raise ValueError("pos_3d takes receivers with three coordinates (x y z); thrifty_amd.pos_est solves 1-D and 2-D tables")
    if len(ids) > _native.POS_MAX_RECEIVERS:
        raise ValueError("at most %d receivers, not %d" % (_native.POS_MAX_RECEIVERS, len(ids)))
    table = np.array(table, dtype=np.float64).reshape(len(ids), 3)
    if not np.all(np.isfinite(table)):
        raise ValueError("a receiver coordinate is not finite")
    return ids, table


def group_heights(height, n_groups, group_tx=None):
    """One height per group from a number, a {tx: height} dict (with `group_tx`) or a column; ValueError for a
    non-finite height and for a tx the dict lacks (the message names it)."""
    if isinstance(height, dict):
        if group_tx is None:
            raise ValueError("a {tx: height} dict needs group_tx")
        txs = np.asarray(group_tx).tolist()
        if len(txs) != n_groups:
            raise ValueError("group_tx holds one transmitter per group")
        missing = sorted({tx for tx in txs if tx not in height})
        if missing:
            raise ValueError("no height for tx %s" % ", ".join(str(tx) for tx in missing))
        column = np.array([height[tx] for tx in txs], dtype=np.float64).reshape(n_groups)
    elif np.ndim(height) == 0:
        column = np.full(n_groups, float(height), dtype=np.float64)
    else:
        column = np.asarray(height, dtype=np.float64)
        if column.shape != (n_groups,):
            raise ValueError("height holds one value per group")
    if not np.all(np.isfinite(column)):
        raise ValueError("the height must be finite")
    return column


def start_height(table, z0=None, z_range=None):
    """(z0, z_range or None) of a free-z solve, checked: the default start and the refusals of the module docstring."""
    lo, hi = float(table[:, 2].min()) - MAX_DIST, float(table[:, 2].max()) + MAX_DIST
    if z_range is not None:
        z_range = np.asarray(z_range, dtype=np.float64)
        if z_range.shape != (2,) or not np.all(np.isfinite(z_range)) or not z_range[0] < z_range[1]:
            raise ValueError("z_range must be two finite heights with z_lo < z_hi")
        lo, hi = float(z_range[0]), float(z_range[1])
    if z0 is None:
        z0 = 0.5 * (lo + hi) if z_range is not None else float(table[:, 2].min()) - BELOW_LOWEST
    z0 = float(z0)
    if not lo <= z0 <= hi:       # false for a NaN
        raise ValueError("z0 = %r lies outside the z range %r .. %r" % (z0, lo, hi))
    if np.all(table[:, 2] == table[0, 2]) and z0 == table[0, 2]:
        raise ValueError("every receiver sits at the height z0 = %r: the start lies on the mirror plane, where the "
                         "z gradient is exactly zero (give another z0, or the height with height=)" % z0)
    return z0, z_range


def pos3_columns(group_ptr, rx0, rx1, tdoa, snr, rx_pos, height=None, group_tx=None, free_z=False, z0=None, z_range=None,
                 x0=(0.1, 0.1), max_iter=100, device_id=0):
    """Positions for TDOA rows in CSR form (group g: rows group_ptr[g]:group_ptr[g + 1]; rx0 / rx1 are receiver
    ids, keys of `rx_pos`, whose values hold x y z) -> dict over ALL groups, in order: `pos` float64[g, 3], `dop`,
    `hdop`, `vdop`, `rms`, `snr`, `status` (index into STATUS_NAMES) and `iters`.  Exactly one of `height` (a number,
    a {tx: height} dict with `group_tx`, or one value per group) and `free_z=True` (with `z0`, `z_range`) is given."""
    if (height is None) == (not free_z):
        raise ValueError("give the transmitter's height (height=) or free_z=True: there is no default mode")
    ids, table = _receiver_table(rx_pos)
    ptr = np.asarray(group_ptr, dtype=np.int64)
    rx0, rx1 = np.asarray(rx0, dtype=np.int64), np.asarray(rx1, dtype=np.int64)
    if ptr.ndim != 1 or len(ptr) < 1 or ptr[0] != 0 or np.any(np.diff(ptr) < 0) or ptr[-1] != len(rx0):
        raise ValueError("group_ptr must start at 0, not decrease and end at the number of rows")
    dense = {rx: k for k, rx in enumerate(ids)}
    for rx in np.unique(np.concatenate([rx0, rx1])).tolist():
        if rx not in dense:
            raise KeyError(rx)
    start = np.asarray(x0, dtype=np.float64)
    if start.shape != (2,) or not np.all(np.isfinite(start)):
        raise ValueError("x0 holds two finite values")
    if free_z:
        if z0 is not None and not np.isfinite(z0):
            raise ValueError("z0 must be finite")
        z0, z_range = start_height(table, z0, z_range)
        mode, heights = _native.POS3_FREE_Z, None
    else:
        if z0 is not None or z_range is not None:
            raise ValueError("z0 and z_range belong to free_z=True")
        mode, heights, z0 = _native.POS3_KNOWN_HEIGHT, group_heights(height, len(ptr) - 1, group_tx), 0.0
    lookup = np.vectorize(dense.__getitem__, otypes=[np.int32])
    return _native.pos3(ptr, lookup(rx0) if len(rx0) else rx0, lookup(rx1) if len(rx1) else rx1, tdoa, snr, table, mode,
                        heights, (start[0], start[1], z0), z_range, max_iter, device_id)


def solve(tdoa_groups, rx_pos, height=None, free_z=False, z0=None, z_range=None, max_iter=100, details=None):
    """Positions of all TDOA groups (group_id, timestamp, tx, tdoas) in one device call -> structured array, one
    record per solved group, in order: `pos_est.POSITION_INFO_DTYPE` cut after `y` with the height known (a dict is
    looked up by each group's tx) and whole, with `z`, with `free_z=True`.  `details`, a dict, receives the columns
    of `pos3_columns` for ALL groups, and `group_id`."""
    groups = list(tdoa_groups)
    ptr = np.cumsum([0] + [len(group[3]) for group in groups])
    column = lambda name, kind: (np.concatenate([np.asarray(group[3][name], dtype=kind) for group in groups])  # noqa: E731
                                 if groups else np.zeros(0, dtype=kind))
    out = pos3_columns(ptr, column("rx0", np.int64), column("rx1", np.int64), column("tdoa", np.float64),
                       column("snr", np.float64), rx_pos, height=height, group_tx=[group[2] for group in groups],
                       free_z=free_z, z0=z0, z_range=z_range, max_iter=max_iter)
    if details is not None:
        details.update(out, group_id=np.array([group[0] for group in groups], dtype=np.int64))
    status = out["status"]
    dropped = np.isin(status, list(_DROPPED))
    for g in np.flatnonzero(dropped).tolist():
        print("Failed to estimate group #{}: {}".format(groups[g][0], _DROPPED[int(status[g])]))
    keep = ~dropped
    axes = ("x", "y", "z") if free_z else ("x", "y")
    names = pos_est.POSITION_INFO_DTYPE["names"][:5 + len(axes)]
    results = np.zeros(int(keep.sum()), dtype={"names": names, "formats": pos_est.POSITION_INFO_DTYPE["formats"][:len(names)]})
    for field, k in (("group_id", 0), ("timestamp", 1), ("tx", 2)):
        results[field] = [group[k] for group, kept in zip(groups, keep) if kept]
    results["dop"], results["snr"] = out["dop"][keep], out["snr"][keep]
    for axis, name in enumerate(axes):
        results[name] = out["pos"][keep, axis]
    return results


def _tx_height(text):
    tx, sep, value = text.partition("=")
    try:
        if not sep:
            raise ValueError
        return int(tx), float(value)
    except ValueError:
        raise argparse.ArgumentTypeError("%r is not TX=HEIGHT" % text)


def _parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("tdoa", nargs="?", type=argparse.FileType("r"), default="data.tdoa",
                        help="tdoa data (\"-\" streams from stdin)")
    parser.add_argument("-o", "--output", dest="output", type=argparse.FileType("w"), default="data.pos",
                        help="output file ('-' for stdout)")
    parser.add_argument("-r", "--rx-coordinates", dest="rx_pos", type=argparse.FileType("r"), default="pos-rx.cfg",
                        help="path to config file that contains the coordinates (x y z) of the receivers")
    mode = parser.add_mutually_exclusive_group(required=True)
    mode.add_argument("--height", type=float, metavar="H", help="the transmitters' known height [m]: solve x and y")
    mode.add_argument("--free-z", dest="free_z", action="store_true", help="solve x, y and z")
    parser.add_argument("--height-tx", dest="height_tx", type=_tx_height, action="append", nargs="+", default=[],
                        metavar="TX=H", help="the known height of one transmitter (with --height, which serves the others)")
    parser.add_argument("--z0", type=float, help="the start's height with --free-z (default: the middle of --z-range, "
                                                 "else %g m below the lowest receiver)" % BELOW_LOWEST)
    parser.add_argument("--z-range", dest="z_range", type=float, nargs=2, metavar=("LO", "HI"),
                        help="the box on z with --free-z (default: the receivers' heights -+ %g m)" % MAX_DIST)
    parser.add_argument("--npz", help="also keep hdop, vdop, rms, status and iters of every group in this file")
    return parser


def _main(argv=None):
    parser = _parser()
    args = parser.parse_args(argv)
    try:
        overrides = dict(pair for given in args.height_tx for pair in given)
        if args.free_z and overrides:
            parser.error("--height-tx belongs to --height")
        if not args.free_z and (args.z0 is not None or args.z_range is not None):
            parser.error("--z0 and --z-range belong to --free-z")
        tdoa_groups = list(tdoa_est.load_tdoa_groups(args.tdoa))
        rx_pos = tdoa_est.load_pos_config(args.rx_pos)
        details = {}
        if args.free_z:
            results = solve(tdoa_groups, rx_pos, free_z=True, z0=args.z0, z_range=args.z_range, details=details)
        else:
            heights = [overrides.get(int(group[2]), args.height) for group in tdoa_groups]
            results = solve(tdoa_groups, rx_pos, height=heights, details=details)
        pos_est.save_positions(args.output, results)
        if args.npz:
            np.savez(args.npz, **details)
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
