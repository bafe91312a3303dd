#!/usr/bin/env python
"""
Which of two heights?  Positions from receivers with three coordinates by a global solve: grid starts, the best
minimum, and a flag where two positions fit -- among them the mirror image about nearly coplanar antennas.

    python -m thrifty_amd.pos_3d_global [data.tdoa] -r pos-rx.cfg -o data.posg3
           (--height H [--height-tx TX=H ...] | --free-z [--z0 Z] [--z-range LO HI] [--z-grid LO HI] [--grid-z N])
           [--grid 32] [--starts 4] [--margin M] [--merge M] [--ratio R] [--noise M] [--pos data.pos]
           [--map GROUP_ID --npz FILE]

`thrifty_amd.pos_3d` starts every group's iteration from one fixed point.  With z free and antennas that are nearly
coplanar a share of the groups ends in a local minimum hundreds of metres above or below them, and with coplanar
antennas two mirrored heights fit equally; nothing flags either.  One device call (`thr_posg3`, csrc/posg3.hip;
include/thrifty_hip.h states every rule) does for `pos_3d`'s two modes what `thrifty_amd.pos_global` does in the plane:

* the cost of every group on a `grid` x `grid` x `grid_z` volume: x and y over the receivers' bounding box grown by
  `margin_m`, z over `z_grid` (with the height known: one plane at the group's height, `grid_z` = 1);
* the `starts` lowest local-minimum cells are starts for `pos_3d`'s own iteration, beside the fixed start (task 0);
* the best minimum (smallest r.m.s. residual among the tasks that converged), the runner-up that lies farther than
  `merge_m` from every better one, and the flags MOVED (1: the fixed start did not reach the best minimum), AMBIGUOUS
  (2: the runner-up's r.m.s. is at most max(`ratio` x the best one's, `floor_m`)), NO_MINIMUM (4: no task converged --
  a solve that ends on the box is none; the record is then the fixed start's, `pos_3d`'s answer) and MIRROR (8, z free
  only: AMBIGUOUS, and the runner-up lies within `merge_m` of the best HORIZONTALLY: x and y can be trusted, the height
  cannot).

grid = 32, grid_z = 8, starts = 4, merge_m = 1, ratio = 2 and margin_m = the longer horizontal side of the receivers'
bounding box are conventions of this interface, not measurements.  So is the default `z_grid`: `z_range` where one is
given, else min(rz) - s .. max(rz) + s with s = max(the antennas' height spread, 10 m).  `floor_m` (`--noise`) has no
meaningful default: pass the deployment's noise level in metres; 0 leaves the ratio alone.  The grid does not find
everything: a minimum whose basin holds no local-minimum cell is missed, and a group in a flat valley stays
unconverged from every start (README, "Which of two heights?").

`.posg3` text: one line per position, `group_id timestamp(%.6f) tx dop hdop vdop snr x y z rms x2 y2 z2 rms2 n_minima
task flags`, floats as their shortest round-trip repr (nan where there is no second).  `--pos` also writes `pos_3d`'s
record (`group_id timestamp tx dop snr x y` with the height known, with `z` when it is free).
"""
from __future__ import print_function

import argparse
import sys

import numpy as np

from thrifty_amd import _native, pos_est, tdoa_est
from thrifty_amd.pos_3d import MAX_DIST, _DROPPED, _receiver_table, _tx_height, group_heights, start_height

MOVED, AMBIGUOUS, NO_MINIMUM, MIRROR = (_native.POSG3_MOVED, _native.POSG3_AMBIGUOUS, _native.POSG3_NO_MINIMUM,
                                        _native.POSG3_MIRROR)
MIN_Z_MARGIN = 10.0     # the default z_grid reaches at least this far beyond the antennas [m]: a convention

GLOBAL3_DTYPE = {
    "names": ("group_id", "timestamp", "tx", "dop", "hdop", "vdop", "snr", "x", "y", "z", "rms", "x2", "y2", "z2", "rms2",
              "n_minima", "task", "flags"),
    "formats": ("i4", "f8", "i4") + ("f8",) * 12 + ("i4",) * 3,
}


def default_z_grid(table, z_range=None):
    """(zg_lo, zg_hi): `z_range` where one is given, else the antennas' heights grown by s = max(their spread,
    MIN_Z_MARGIN) on either side -- a convention."""
    if z_range is not None:
        return float(z_range[0]), float(z_range[1])
    z = np.asarray(table, dtype=np.float64)[:, 2]
    s = max(float(z.max() - z.min()), MIN_Z_MARGIN)
    return float(z.min()) - s, float(z.max()) + s


def _options(rx_pos, free_z, z_range, z_grid, grid, grid_z, starts, margin_m, merge_m, ratio, floor_m, max_iter=100):
    """(receiver ids, table[n_rx, 3], margin_m, z_grid or None, grid_z) as thr_posg3 takes them; ValueError for what it
    would refuse."""
    ids, table = _receiver_table(rx_pos)
    if grid not in _native.POSG3_GRIDS:
        raise ValueError("grid must be one of %r, not %r" % (_native.POSG3_GRIDS, grid))
    if int(starts) != starts or not 1 <= int(starts) <= _native.POSG3_MAX_STARTS:
        raise ValueError("starts must lie in 1 .. %d, not %r" % (_native.POSG3_MAX_STARTS, starts))
    if margin_m is None:
        margin_m = float(np.max(table[:, :2].max(axis=0) - table[:, :2].min(axis=0)))
    if not 0.0 < float(margin_m) <= _native.POSG3_MAX_MARGIN:
        raise ValueError("margin_m must lie in (0, %g] metres, not %r" % (_native.POSG3_MAX_MARGIN, margin_m))
    if not (np.isfinite(merge_m) and float(merge_m) > 0.0):
        raise ValueError("merge_m must be a positive number of metres, not %r" % (merge_m,))
    if not (np.isfinite(ratio) and float(ratio) >= 1.0):
        raise ValueError("ratio must be at least 1 and finite, not %r" % (ratio,))
    if not (np.isfinite(floor_m) and float(floor_m) >= 0.0):
        raise ValueError("floor_m must be finite and not negative, not %r" % (floor_m,))
    if int(max_iter) != max_iter or max_iter < 0:
        raise ValueError("max_iter must be a whole number that is not negative, not %r" % (max_iter,))
    if not free_z:
        if z_grid is not None or grid_z not in (None, 1):
            raise ValueError("z_grid and grid_z belong to free_z=True: with the height known the grid is one plane")
        return ids, table, float(margin_m), None, 1
    grid_z = 8 if grid_z is None else grid_z
    if int(grid_z) != grid_z or not 2 <= int(grid_z) <= _native.POSG3_MAX_GRID_Z:
        raise ValueError("grid_z must lie in 2 .. %d, not %r" % (_native.POSG3_MAX_GRID_Z, grid_z))
    lo, hi = float(table[:, 2].min()) - MAX_DIST, float(table[:, 2].max()) + MAX_DIST
    if z_range is not None:
        lo, hi = float(z_range[0]), float(z_range[1])
    if z_grid is None:
        z_grid = default_z_grid(table, z_range)
    z_grid = np.asarray(z_grid, dtype=np.float64)
    if z_grid.shape != (2,) or not np.all(np.isfinite(z_grid)) or not z_grid[0] < z_grid[1]:
        raise ValueError("z_grid must be two finite heights with zg_lo < zg_hi")
    if not (lo <= z_grid[0] and z_grid[1] <= hi):
        raise ValueError("z_grid %r .. %r leaves the z box %r .. %r" % (float(z_grid[0]), float(z_grid[1]), lo, hi))
    return ids, table, float(margin_m), (float(z_grid[0]), float(z_grid[1])), int(grid_z)


def global3_columns(group_ptr, rx0, rx1, tdoa, snr, rx_pos, height=None, group_tx=None, free_z=False, z0=None, z_range=None,
                    z_grid=None, grid=32, grid_z=None, starts=4, margin_m=None, merge_m=1.0, ratio=2.0, floor_m=0.0, map_first=0,
                    map_count=0, x0=(0.1, 0.1), max_iter=100, device_id=0):
    """The global solve for TDOA rows in CSR form (group g: rows group_ptr[g]:group_ptr[g + 1]; rx0 / rx1 are receiver
    ids, keys of `rx_pos`, whose values hold x y z) -> dict over ALL groups, in order, of every output of
    `_native.POSG3_OUTPUTS`, plus `counts`, `margin_m`, `z_grid` and the cell centres `cx`, `cy`, `cz` (None with the
    height known).  Exactly one of `height` (a number, a {tx: height} dict with `group_tx`, or one value per group) and
    `free_z=True` (with `z0`, `z_range`, `z_grid`, `grid_z`) is given.  `map` / `map_min` hold the groups map_first ..
    map_first + map_count - 1."""
    if (height is None) == (not free_z):
        raise ValueError("give the transmitter's height (height=) or free_z=True: there is no default mode")
    if free_z and z_range is not None:
        z_range = np.asarray(z_range, dtype=np.float64)
        if z_range.shape != (2,) or not np.all(np.isfinite(z_range)) or not z_range[0] < z_range[1]:
            raise ValueError("z_range must be two finite heights with z_lo < z_hi")
    ids, table, margin_m, z_grid, grid_z = _options(rx_pos, free_z, z_range, z_grid, grid, grid_z, starts, margin_m, merge_m,
                                                    ratio, floor_m, max_iter)
    ptr = np.asarray(group_ptr, dtype=np.int64)
    rx0, rx1 = np.asarray(rx0, dtype=np.int64), np.asarray(rx1, dtype=np.int64)
    if ptr.ndim != 1 or len(ptr) < 1 or ptr[0] != 0 or np.any(np.diff(ptr) < 0) or ptr[-1] != len(rx0):
        raise ValueError("group_ptr must start at 0, not decrease and end at the number of rows")
    if len(ptr) - 1 > (1 << 28) // (int(starts) + 1):
        raise ValueError("too many groups: groups x (starts + 1) may not pass 2^28")
    if int(map_count) != map_count or not 0 <= map_count <= _native.POSG3_MAX_MAP:
        raise ValueError("map_count must lie in 0 .. %d, not %r" % (_native.POSG3_MAX_MAP, map_count))
    if int(map_first) != map_first or map_first < 0 or map_first + map_count > len(ptr) - 1:
        raise ValueError("the map range %r + %r passes the %d groups" % (map_first, map_count, len(ptr) - 1))
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
    counts, out = _native.posg3(ptr, lookup(rx0) if len(rx0) else rx0, lookup(rx1) if len(rx1) else rx1, tdoa, snr, table, mode,
                                margin_m, heights, (start[0], start[1], z0), z_range, z_grid, grid, grid_z, starts, merge_m, ratio,
                                floor_m, map_first, map_count, max_iter, device_id=device_id)
    out["counts"], out["margin_m"], out["z_grid"] = counts, margin_m, z_grid
    out["cx"], out["cy"], out["cz"] = cell_centres(table, margin_m, grid, z_grid, grid_z)
    return out


def cell_centres(table, margin_m, grid, z_grid=None, grid_z=1):
    """(cx, cy, cz) of the search volume: the device's expression, so the same bits; cz is None without `z_grid`."""
    table = np.asarray(table, dtype=np.float64)
    lo, hi = table[:, :2].min(axis=0) - np.float64(margin_m), table[:, :2].max(axis=0) + np.float64(margin_m)
    cx, cy = (lo[k] + (np.arange(grid) + 0.5) * ((hi[k] - lo[k]) / grid) for k in (0, 1))
    if z_grid is None:
        return cx, cy, None
    zlo, zhi = np.float64(z_grid[0]), np.float64(z_grid[1])
    return cx, cy, zlo + (np.arange(grid_z) + 0.5) * ((zhi - zlo) / grid_z)


def _flatten(groups):
    ptr = np.cumsum([0] + [len(group[3]) for group in groups])
    column = lambda name, kind: (np.concatenate([np.asarray(group[3][name], dtype=kind) for group in groups])  # noqa: E731
                                 if groups else np.zeros(0, dtype=kind))
    return ptr, column("rx0", np.int64), column("rx1", np.int64), column("tdoa", np.float64), column("snr", np.float64)


def solve(tdoa_groups, rx_pos, height=None, free_z=False, z0=None, z_range=None, z_grid=None, grid=32, grid_z=None, starts=4,
          margin_m=None, merge_m=1.0, ratio=2.0, floor_m=0.0, max_iter=100, details=None):
    """The global solve of all TDOA groups (group_id, timestamp, tx, tdoas) in one device call -> structured array
    (GLOBAL3_DTYPE), one record per solved group, in order; with the height known `z` is that height (a dict is looked
    up by each group's tx) and `z2` the same.  `grid_z` defaults to 8 with z free.  Dropped groups print
    `pos_3d.solve`'s sentence.  `details`, a dict, receives the columns of `global3_columns` for ALL groups, and
    `group_id`."""
    groups = list(tdoa_groups)
    out = global3_columns(*_flatten(groups), rx_pos, height=height, group_tx=[group[2] for group in groups], free_z=free_z, z0=z0,
                          z_range=z_range, z_grid=z_grid, grid=grid, grid_z=grid_z, starts=starts, margin_m=margin_m,
                          merge_m=merge_m, ratio=ratio, floor_m=floor_m, max_iter=max_iter)
    if details is not None:
        details.update(out, group_id=np.array([group[0] for group in groups], dtype=np.int64))
    status = out["status"]
    dropped = np.isin(status, list(_DROPPED))
    for g in np.flatnonzero(dropped).tolist():
        print("Failed to estimate group #{}: {}".format(groups[g][0], _DROPPED[int(status[g])]))
    keep = ~dropped
    results = np.zeros(int(keep.sum()), dtype=GLOBAL3_DTYPE)
    for field, k in (("group_id", 0), ("timestamp", 1), ("tx", 2)):
        results[field] = [group[k] for group, kept in zip(groups, keep) if kept]
    for name in ("dop", "hdop", "vdop", "snr", "rms", "rms2", "n_minima", "task", "flags"):
        results[name] = out[name][keep]
    for axis, name in enumerate(("x", "y", "z")):
        results[name], results[name + "2"] = out["pos"][keep, axis], out["pos2"][keep, axis]
    return results


def volume(tdoa_groups, rx_pos, group_id, **options):
    """The cost volume of the group with this id (`solve`'s options) -> dict(map float64[grid_z, grid, grid] (plane k:
    cz[k], row j: cy[j], column i: cx[i]; one plane with the height known), map_min, cx, cy, cz, start_cell, start_f,
    task_pos, task_rms, task_status, pos, pos2, rms, rms2, flags, task)."""
    groups = list(tdoa_groups)
    where = [k for k, group in enumerate(groups) if group[0] == group_id]
    if not where:
        raise ValueError("no group has the id %r" % (group_id,))
    g = where[0]
    out = global3_columns(*_flatten(groups), rx_pos, group_tx=[group[2] for group in groups], map_first=g, map_count=1, **options)
    res = {"map": out["map"][0], "map_min": out["map_min"][0], "cx": out["cx"], "cy": out["cy"],
           "cz": np.array([out["pos"][g, 2]]) if out["cz"] is None else out["cz"]}
    for name in ("start_cell", "start_f", "task_pos", "task_rms", "task_status", "pos", "pos2", "rms", "rms2", "flags", "task"):
        res[name] = out[name][g]
    return res


def save_global3(output, results):
    """One line per position (see the module docstring); `output` is a file name or an open text file."""
    if isinstance(output, str):
        with open(output, "w") as handle:
            return save_global3(handle, results)
    for record in results:
        words = [str(int(record["group_id"])), "%.6f" % record["timestamp"], str(int(record["tx"]))]
        words += [repr(float(record[name])) if fmt == "f8" else str(int(record[name]))
                  for name, fmt in zip(GLOBAL3_DTYPE["names"][3:], GLOBAL3_DTYPE["formats"][3:])]
        output.write(" ".join(words) + "\n")


def load_global3(fname):
    """The records of a .posg3 file."""
    if isinstance(fname, str):
        with open(fname, "r") as handle:
            return load_global3(handle)
    rows = [line.decode() if isinstance(line, bytes) else line for line in fname]
    rows = [line.split() for line in rows if line.strip() and not line.lstrip().startswith("#")]
    data = np.zeros(len(rows), dtype=GLOBAL3_DTYPE)
    for r, words in enumerate(rows):
        if len(words) != len(GLOBAL3_DTYPE["names"]):
            raise ValueError("line %d holds %d fields, a .posg3 line holds %d" % (r + 1, len(words), len(GLOBAL3_DTYPE["names"])))
        data[r] = tuple(float(w) if fmt == "f8" else int(w) for w, fmt in zip(words, GLOBAL3_DTYPE["formats"]))
    return data


def positions(results, free_z):
    """`pos_3d`'s record of these results: `pos_est.POSITION_INFO_DTYPE` cut after `y` with the height known, whole with
    z free."""
    names = pos_est.POSITION_INFO_DTYPE["names"][:8 if free_z else 7]
    out = np.zeros(len(results), dtype={"names": names, "formats": pos_est.POSITION_INFO_DTYPE["formats"][:len(names)]})
    for name in names:
        out[name] = results[name]
    return out


def format_summary(results):
    """The groups, how many moved away from the fixed start, are ambiguous, mirrored or have no minimum, and the mean
    n_minima."""
    flags = np.asarray(results["flags"])
    mean = float(np.mean(results["n_minima"])) if len(results) else float("nan")
    return "{} positions, {} moved, {} ambiguous ({} of them in height only), {} without a minimum, {:.2f} minima per position\n".format(
        len(results), int(np.count_nonzero(flags & MOVED)), int(np.count_nonzero(flags & AMBIGUOUS)),
        int(np.count_nonzero(flags & MIRROR)), int(np.count_nonzero(flags & NO_MINIMUM)), mean)


def _parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("tdoa", nargs="?", type=argparse.FileType("r"), default="data.tdoa", help="tdoa data (\"-\" streams from stdin)")
    parser.add_argument("-o", "--output", dest="output", type=argparse.FileType("w"), default="data.posg3",
                        help="output file ('-' for stdout)")
    parser.add_argument("-r", "--rx-coordinates", dest="rx_pos", type=argparse.FileType("r"), default="pos-rx.cfg",
                        help="path to config file that contains the coordinates (x y z) of the receivers")
    mode = parser.add_mutually_exclusive_group(required=True)
    mode.add_argument("--height", type=float, metavar="H", help="the transmitters' known height [m]: solve x and y")
    mode.add_argument("--free-z", dest="free_z", action="store_true", help="solve x, y and z")
    parser.add_argument("--height-tx", dest="height_tx", type=_tx_height, action="append", nargs="+", default=[],
                        metavar="TX=H", help="the known height of one transmitter (with --height, which serves the others)")
    parser.add_argument("--z0", type=float, help="the fixed start's height with --free-z (pos_3d's default)")
    parser.add_argument("--z-range", dest="z_range", type=float, nargs=2, metavar=("LO", "HI"),
                        help="the box on z with --free-z (default: the receivers' heights -+ %g m)" % MAX_DIST)
    parser.add_argument("--z-grid", dest="z_grid", type=float, nargs=2, metavar=("LO", "HI"),
                        help="the heights the search volume spans with --free-z (default: --z-range, else the antennas' heights "
                             "grown by their spread, at least %g m)" % MIN_Z_MARGIN)
    parser.add_argument("--grid-z", dest="grid_z", type=int, default=None, metavar="N",
                        help="planes of the search volume with --free-z (2 .. %d, default 8)" % _native.POSG3_MAX_GRID_Z)
    parser.add_argument("--grid", type=int, choices=_native.POSG3_GRIDS, default=32, help="cells per horizontal side of the search volume")
    parser.add_argument("--starts", type=int, default=4, help="lowest local minima of the volume that the iteration is started from (1 .. 8)")
    parser.add_argument("--margin", dest="margin_m", type=float, default=None, metavar="M",
                        help="metres the search area reaches beyond the receivers (default: the longer side of their bounding box)")
    parser.add_argument("--merge", dest="merge_m", type=float, default=1.0, metavar="M", help="positions within this many metres are one minimum")
    parser.add_argument("--ratio", type=float, default=2.0, help="a second minimum within RATIO times the best r.m.s. residual is ambiguous")
    parser.add_argument("--noise", dest="floor_m", type=float, default=0.0, metavar="M",
                        help="the deployment's noise level [m]: a second minimum whose r.m.s. residual is below it is ambiguous as well")
    parser.add_argument("--pos", dest="pos", type=argparse.FileType("w"), default=None, help="also write the positions as a .pos file")
    parser.add_argument("--map", dest="map_id", type=int, default=None, metavar="GROUP_ID", help="also save this group's cost volume (needs --npz)")
    parser.add_argument("--npz", dest="npz", default=None, metavar="FILE", help="where --map's arrays go")
    return parser


def _main(argv=None):
    parser = _parser()
    args = parser.parse_args(argv)
    streams = [args.tdoa, args.rx_pos]
    try:
        overrides = dict(pair for given in args.height_tx for pair in given)
        if args.free_z and overrides:
            parser.error("--height-tx belongs to --height")
        if not args.free_z and any(v is not None for v in (args.z0, args.z_range, args.z_grid, args.grid_z)):
            parser.error("--z0, --z-range, --z-grid and --grid-z belong to --free-z")
        if (args.map_id is None) != (args.npz is None):
            sys.stderr.write("--map and --npz go together\n")
            return 1
        tdoa_groups = list(tdoa_est.load_tdoa_groups(args.tdoa))
        rx_pos = tdoa_est.load_pos_config(args.rx_pos)
        options = dict(grid=args.grid, starts=args.starts, margin_m=args.margin_m, merge_m=args.merge_m, ratio=args.ratio,
                       floor_m=args.floor_m)
        if args.free_z:
            options.update(free_z=True, z0=args.z0, z_range=args.z_range, z_grid=args.z_grid, grid_z=args.grid_z)
        else:
            options.update(height=[overrides.get(int(group[2]), args.height) for group in tdoa_groups])
        try:
            results = solve(tdoa_groups, rx_pos, **options)
            if args.map_id is not None:
                np.savez(args.npz, **volume(tdoa_groups, rx_pos, args.map_id, **options))
        except ValueError as err:
            sys.stderr.write("%s\n" % err)
            return 1
        save_global3(args.output, results)
        if args.pos is not None:
            pos_est.save_positions(args.pos, positions(results, args.free_z))
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
