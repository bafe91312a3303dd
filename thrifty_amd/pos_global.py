#!/usr/bin/env python
"""
Which of two positions?  Positions from TDOA values by a global solve: grid starts, the best minimum, and a flag
where two positions fit.

    python -m thrifty_amd.pos_global [data.tdoa] -r pos-rx.cfg -o data.posg [--grid 32] [--starts 4] [--margin M]
                                     [--merge M] [--ratio R] [--noise M] [--pos data.pos] [--map GROUP_ID --npz FILE]

`thrifty pos` (thrifty_amd/pos_est.py) starts every group's iteration from x0 = (0.1, 0.1), a fixed point of the
coordinate frame that has nothing to do with where the receivers are: with an array far from the origin a share of
the groups ends in a worse minimum or on the solver's box, and with three receivers the answer is one of two mirror
positions and nothing says so (the reference: "TODO: use analytic solution or previous position as initial value").
One device call (`thr_posg`, csrc/posg.hip; include/thrifty_hip.h states every rule), 2-D only:

* the cost surface of every group on a `grid` x `grid` raster over the receivers' bounding box grown by `margin_m`;
* the `starts` lowest local-minimum cells are starts for `thrifty pos`' own iteration, beside the fixed x0 (task 0);
* the best minimum (smallest r.m.s. residual among the tasks that converged), the runner-up that lies farther than
  `merge_m` from every better one, and the flags MOVED (1: the fixed start did not reach the best minimum),
  AMBIGUOUS (2: the runner-up's r.m.s. is at most max(`ratio` x the best one's, `floor_m`)) and NO_MINIMUM (4: no
  task converged; the record is then the fixed start's).

grid = 32, starts = 4, merge_m = 1, ratio = 2 and margin_m = the longer side of the receivers' bounding box are
conventions of this interface, not measurements.  `floor_m` (`--noise`) has no meaningful default: pass the
deployment's noise level in metres; 0 leaves the ratio alone, and residuals of a few millimetres then pass for
"twice as good".

`.posg` text: one line per position, `group_id timestamp(%.6f) tx dop snr x y rms x2 y2 rms2 n_minima task flags`,
floats as their shortest round-trip repr (nan where there is no second).
"""
from __future__ import print_function

import argparse
import sys

import numpy as np

from thrifty_amd import _native, pos_est, tdoa_est

MOVED, AMBIGUOUS, NO_MINIMUM = _native.POSG_MOVED, _native.POSG_AMBIGUOUS, _native.POSG_NO_MINIMUM

GLOBAL_DTYPE = {
    "names": ("group_id", "timestamp", "tx", "dop", "snr", "x", "y", "rms", "x2", "y2", "rms2", "n_minima", "task", "flags"),
    "formats": ("i4", "f8", "i4") + ("f8",) * 8 + ("i4",) * 3,
}


def _options(rx_pos, grid, starts, margin_m, merge_m, ratio, floor_m, max_iter=100):
    """(receiver ids, table[n_rx, 2], margin_m) as thr_posg takes them; ValueError for what it would refuse."""
    ids = list(rx_pos)
    if not ids:
        raise ValueError("rx_pos is empty")
    table = [np.atleast_1d(np.asarray(rx_pos[i], dtype=np.float64)) for i in ids]
    if any(row.ndim != 1 or len(row) != len(table[0]) for row in table):
        raise ValueError("the receivers' coordinates differ in length")
    if len(table[0]) != 2:
        raise ValueError("%d-D receiver coordinates: the global solve works in 2 dimensions" % len(table[0]))
    if len(ids) > _native.POS_MAX_RECEIVERS:
        raise ValueError("at most %d receivers, not %d" % (_native.POS_MAX_RECEIVERS, len(ids)))
    table = np.array(table, dtype=np.float64).reshape(len(ids), 2)
    if not np.all(np.isfinite(table)):
        raise ValueError("a receiver coordinate is not finite")
    if grid not in _native.POSG_GRIDS:
        raise ValueError("grid must be one of %r, not %r" % (_native.POSG_GRIDS, grid))
    if int(starts) != starts or not 1 <= int(starts) <= _native.POSG_MAX_STARTS:
        raise ValueError("starts must lie in 1 .. %d, not %r" % (_native.POSG_MAX_STARTS, starts))
    if margin_m is None:
        margin_m = float(np.max(table.max(axis=0) - table.min(axis=0)))
    if not 0.0 < float(margin_m) <= _native.POSG_MAX_MARGIN:
        raise ValueError("margin_m must lie in (0, %g] metres, not %r" % (_native.POSG_MAX_MARGIN, margin_m))
    if not (np.isfinite(merge_m) and float(merge_m) > 0.0):
        raise ValueError("merge_m must be a positive number of metres, not %r" % (merge_m,))
    if not (np.isfinite(ratio) and float(ratio) >= 1.0):
        raise ValueError("ratio must be at least 1 and finite, not %r" % (ratio,))
    if not (np.isfinite(floor_m) and float(floor_m) >= 0.0):
        raise ValueError("floor_m must be finite and not negative, not %r" % (floor_m,))
    if int(max_iter) != max_iter or max_iter < 0:
        raise ValueError("max_iter must be a whole number that is not negative, not %r" % (max_iter,))
    return ids, table, float(margin_m)


def global_columns(group_ptr, rx0, rx1, tdoa, snr, rx_pos, grid=32, starts=4, margin_m=None, merge_m=1.0, ratio=2.0,
                   floor_m=0.0, map_first=0, map_count=0, x0=(0.1, 0.1), max_iter=100, device_id=0):
    """The global solve for TDOA rows in CSR form (group g: rows group_ptr[g]:group_ptr[g + 1]; rx0 / rx1 are receiver
    ids, keys of `rx_pos`) -> dict over ALL groups, in order, of every output of `_native.POSG_OUTPUTS`, plus `counts`,
    `margin_m` and the cell centres `cx`, `cy`.  `map` / `map_min` hold the groups map_first .. map_first + map_count - 1."""
    ids, table, margin_m = _options(rx_pos, grid, starts, margin_m, merge_m, ratio, floor_m, max_iter)
    ptr = np.asarray(group_ptr, dtype=np.int64)
    rx0, rx1 = np.asarray(rx0, dtype=np.int64), np.asarray(rx1, dtype=np.int64)
    if ptr.ndim != 1 or len(ptr) < 1 or ptr[0] != 0 or np.any(np.diff(ptr) < 0) or ptr[-1] != len(rx0):
        raise ValueError("group_ptr must start at 0, not decrease and end at the number of rows")
    if len(ptr) - 1 > (1 << 28) // (int(starts) + 1):
        raise ValueError("too many groups: groups x (starts + 1) may not pass 2^28")
    if int(map_count) != map_count or not 0 <= map_count <= _native.POSG_MAX_MAP:
        raise ValueError("map_count must lie in 0 .. %d, not %r" % (_native.POSG_MAX_MAP, map_count))
    if int(map_first) != map_first or map_first < 0 or map_first + map_count > len(ptr) - 1:
        raise ValueError("the map range %r + %r passes the %d groups" % (map_first, map_count, len(ptr) - 1))
    start = np.asarray(x0, dtype=np.float64)
    if start.shape != (2,) or not np.all(np.isfinite(start)):
        raise ValueError("x0 holds two finite values")
    dense = {rx: k for k, rx in enumerate(ids)}
    for rx in np.unique(np.concatenate([rx0, rx1])).tolist():
        if rx not in dense:
            raise KeyError(rx)
    lookup = np.vectorize(dense.__getitem__, otypes=[np.int32])
    counts, out = _native.posg(ptr, lookup(rx0) if len(rx0) else rx0, lookup(rx1) if len(rx1) else rx1, tdoa, snr, table,
                               margin_m, grid, starts, merge_m, ratio, floor_m, map_first, map_count, x0, max_iter,
                               device_id=device_id)
    out["counts"], out["margin_m"] = counts, margin_m
    out["cx"], out["cy"] = cell_centres(table, margin_m, grid)
    return out


def cell_centres(table, margin_m, grid):
    """(cx, cy) of the search area: the device's expression, so the same bits."""
    table = np.asarray(table, dtype=np.float64)
    lo, hi = table.min(axis=0) - np.float64(margin_m), table.max(axis=0) + np.float64(margin_m)
    return tuple(lo[k] + (np.arange(grid) + 0.5) * ((hi[k] - lo[k]) / grid) for k in (0, 1))


def _flatten(groups):
    ptr = np.cumsum([0] + [len(group[3]) for group in groups])
    column = lambda name, kind: (np.concatenate([np.asarray(group[3][name], dtype=kind) for group in groups])  # noqa: E731
                                 if groups else np.zeros(0, dtype=kind))
    return ptr, column("rx0", np.int64), column("rx1", np.int64), column("tdoa", np.float64), column("snr", np.float64)


def solve(tdoa_groups, rx_pos, grid=32, starts=4, margin_m=None, merge_m=1.0, ratio=2.0, floor_m=0.0, max_iter=100):
    """The global solve of all TDOA groups (group_id, timestamp, tx, tdoas) in one device call -> structured array
    (GLOBAL_DTYPE), one record per solved group, in order.  Dropped groups print `pos_est.solve`'s sentence."""
    groups = list(tdoa_groups)
    _options(rx_pos, grid, starts, margin_m, merge_m, ratio, floor_m, max_iter)
    out = global_columns(*_flatten(groups), rx_pos, grid=grid, starts=starts, margin_m=margin_m, merge_m=merge_m, ratio=ratio,
                         floor_m=floor_m, max_iter=max_iter)
    status = out["status"]
    dropped = pos_est._DROPPED
    for g in np.flatnonzero(np.isin(status, list(dropped))).tolist():
        print("Failed to estimate group #{}: {}".format(groups[g][0], dropped[int(status[g])]))
    keep = ~np.isin(status, list(dropped))
    results = np.zeros(int(keep.sum()), dtype=GLOBAL_DTYPE)
    results["group_id"] = [group[0] for group, k in zip(groups, keep) if k]
    results["timestamp"] = [group[1] for group, k in zip(groups, keep) if k]
    results["tx"] = [group[2] for group, k in zip(groups, keep) if k]
    results["dop"], results["snr"], results["rms"] = out["dop"][keep], out["snr"][keep], out["rms"][keep]
    results["x"], results["y"] = out["pos"][keep, 0], out["pos"][keep, 1]
    results["x2"], results["y2"], results["rms2"] = out["pos2"][keep, 0], out["pos2"][keep, 1], out["rms2"][keep]
    for name in ("n_minima", "task", "flags"):
        results[name] = out[name][keep]
    return results


def surface(tdoa_groups, rx_pos, group_id, grid=32, starts=4, margin_m=None, merge_m=1.0, ratio=2.0, floor_m=0.0, max_iter=100):
    """The cost surface of the group with this id -> dict(map float64[grid, grid] (row j: cy[j], column i: cx[i]),
    map_min, cx, cy, start_cell, start_f, task_pos, task_rms, task_status, pos, pos2, flags)."""
    groups = list(tdoa_groups)
    where = [k for k, group in enumerate(groups) if group[0] == group_id]
    if not where:
        raise ValueError("no group has the id %r" % (group_id,))
    g = where[0]
    out = global_columns(*_flatten(groups), rx_pos, grid=grid, starts=starts, margin_m=margin_m, merge_m=merge_m, ratio=ratio,
                         floor_m=floor_m, map_first=g, map_count=1, max_iter=max_iter)
    res = {"map": out["map"][0], "map_min": out["map_min"][0], "cx": out["cx"], "cy": out["cy"]}
    for name in ("start_cell", "start_f", "task_pos", "task_rms", "task_status", "pos", "pos2", "rms", "rms2", "flags", "task"):
        res[name] = out[name][g]
    return res


def save_global(output, results):
    """One line per position (see the module docstring); `output` is a file name or an open text file."""
    if isinstance(output, str):
        with open(output, "w") as handle:
            return save_global(handle, results)
    for record in results:
        words = [str(int(record["group_id"])), "%.6f" % record["timestamp"], str(int(record["tx"]))]
        words += [repr(float(record[name])) if fmt == "f8" else str(int(record[name]))
                  for name, fmt in zip(GLOBAL_DTYPE["names"][3:], GLOBAL_DTYPE["formats"][3:])]
        output.write(" ".join(words) + "\n")


def load_global(fname):
    """The records of a .posg file."""
    if isinstance(fname, str):
        with open(fname, "r") as handle:
            return load_global(handle)
    rows = [line.decode() if isinstance(line, bytes) else line for line in fname]
    rows = [line.split() for line in rows if line.strip() and not line.lstrip().startswith("#")]
    data = np.zeros(len(rows), dtype=GLOBAL_DTYPE)
    for r, words in enumerate(rows):
        if len(words) != len(GLOBAL_DTYPE["names"]):
            raise ValueError("line %d holds %d fields, a .posg line holds %d" % (r + 1, len(words), len(GLOBAL_DTYPE["names"])))
        data[r] = tuple(float(w) if fmt == "f8" else int(w) for w, fmt in zip(words, GLOBAL_DTYPE["formats"]))
    return data


def format_summary(results):
    """The groups, how many moved away from the fixed start, are ambiguous or have no minimum, and the mean n_minima."""
    flags = np.asarray(results["flags"])
    mean = float(np.mean(results["n_minima"])) if len(results) else float("nan")
    return "{} positions, {} moved, {} ambiguous, {} without a minimum, {:.2f} minima per position\n".format(
        len(results), int(np.count_nonzero(flags & MOVED)), int(np.count_nonzero(flags & AMBIGUOUS)),
        int(np.count_nonzero(flags & NO_MINIMUM)), mean)


_CLI = (
    (("tdoa",), dict(nargs="?", type=argparse.FileType("r"), default="data.tdoa", help="tdoa data (\"-\" streams from stdin)")),
    (("-o", "--output"), dict(dest="output", type=argparse.FileType("w"), default="data.posg", help="output file ('-' for stdout)")),
    (("-r", "--rx-coordinates"), dict(dest="rx_pos", type=argparse.FileType("r"), default="pos-rx.cfg",
                                      help="path to config file that contains the coordinates of the receivers")),
    (("--grid",), dict(type=int, choices=_native.POSG_GRIDS, default=32, help="cells per side of the search raster")),
    (("--starts",), dict(type=int, default=4, help="lowest local minima of the raster that the iteration is started from (1 .. 8)")),
    (("--margin",), dict(dest="margin_m", type=float, default=None, metavar="M",
                         help="metres the search area reaches beyond the receivers (default: the longer side of their bounding box)")),
    (("--merge",), dict(dest="merge_m", type=float, default=1.0, metavar="M", help="positions within this many metres are one minimum")),
    (("--ratio",), dict(type=float, default=2.0, help="a second minimum within RATIO times the best r.m.s. residual is ambiguous")),
    (("--noise",), dict(dest="floor_m", type=float, default=0.0, metavar="M",
                        help="the deployment's noise level [m]: a second minimum whose r.m.s. residual is below it is ambiguous as well")),
    (("--pos",), dict(dest="pos", type=argparse.FileType("w"), default=None, help="also write the positions as a .pos file")),
    (("--map",), dict(dest="map_id", type=int, default=None, metavar="GROUP_ID", help="also save this group's cost surface (needs --npz)")),
    (("--npz",), dict(dest="npz", default=None, metavar="FILE", help="where --map's arrays go")),
)


def _parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for flags, options in _CLI:
        parser.add_argument(*flags, **options)
    return parser


def _main(argv=None):
    args = _parser().parse_args(argv)
    streams = [args.tdoa, args.rx_pos]
    try:
        if (args.map_id is None) != (args.npz is None):
            sys.stderr.write("--map and --npz go together\n")
            return 1
        tdoa_groups = list(tdoa_est.load_tdoa_groups(args.tdoa))
        rx_pos = tdoa_est.load_pos_config(args.rx_pos)
        options = dict(grid=args.grid, starts=args.starts, margin_m=args.margin_m, merge_m=args.merge_m, ratio=args.ratio,
                       floor_m=args.floor_m)
        try:
            results = solve(tdoa_groups, rx_pos, **options)
            if args.map_id is not None:
                np.savez(args.npz, **surface(tdoa_groups, rx_pos, args.map_id, **options))
        except ValueError as err:
            sys.stderr.write("%s\n" % err)
            return 1
        save_global(args.output, results)
        if args.pos is not None:
            positions = np.zeros(len(results), dtype=pos_est._result_dtype(2))
            for name in positions.dtype.names:
                positions[name] = results[name]
            pos_est.save_positions(args.pos, positions)
        (sys.stderr if args.output is sys.stdout else sys.stdout).write(format_summary(results))
        return 0
    finally:
        for stream in streams:
            if stream is not sys.stdin:
                stream.close()
        for stream in (args.output, args.pos):
            if stream is None:
                continue
            if stream is sys.stdout:
                stream.flush()
            else:
                stream.close()


if __name__ == "__main__":
    sys.exit(_main())
