#!/usr/bin/env python
"""
Can a 3-D position be trusted?  `pos_quality`'s residuals, error ellipse, row weights and receiver exclusion for
receivers whose antennas sit at different heights.

    python -m thrifty_amd.pos_3d_quality [data.tdoa] -r pos-rx.cfg -o data.posq3
           (--height H [--height-tx TX=H ...] | --free-z [--z0 Z] [--z-range LO HI])
           [--weights snr] [--exclude GATE_M] [--ratio R] [--min-rx N] [--pos data.pos] [--posq data.posq]

`pos-rx.cfg` is `id: x y z`.  One device call (`thr_posq3`, csrc/posq3.hip; include/thrifty_hip.h states every rule):
every group is solved as `thrifty_amd.pos_3d` solves it (the same iteration, csrc/pos3_lm.hpp, in the same two modes,
with the same start, box and refusals), optionally with a weight per row, and then judged as `thrifty_amd.pos_quality`
judges a planar solve:

* `rms` is the root mean square of the (weighted) residuals in metres with the 3-D ranges; `q = inv(A)` the inverse
  normal matrix, `xdop, ydop, zdop = sqrt(q00), sqrt(q11), sqrt(q22)`, and `major`, `minor`, `angle` the ellipse of
  the horizontal block (q00, q01, q11): the marginal covariance of x and y.  With the height known q is the 2 x 2
  inverse, zdop and vdop are 0 and hdop is dop;
* with `exclude_gate_m`, a group whose rms exceeds the gate and that names at least `min_rx` receivers is solved once
  more without each of its receivers; the best of those replaces the full solve when its rms is at most `ratio`
  times the full one.  The gate has no default: it is the deployment's noise level in metres.  `min_rx` defaults to
  the mode's floor: N receivers give N - 1 independent TDOAs and a candidate (N - 1 receivers) must keep one
  redundant arrival, N - 2 > unknowns -- 5 with the height known, 6 with z free.  0.5 and the floors are conventions
  and derivations, not measurements.

`.posq3` text: one line per position, `group_id timestamp(%.6f) tx dop hdop vdop snr x y z rms xdop ydop zdop major
minor angle n_rx n_rows excluded flags`, floats as their shortest round-trip repr; `excluded` is a receiver id or -1,
`flags` the sum of INCONSISTENT (1), EXCLUDED (2) and NO_CANDIDATE (4).  `--pos` writes `pos_3d`'s record (7 columns
with the height known, 8 with z free); `--posq` writes the horizontal part as a `.posq` line of `pos_quality` with
`dop` := `hdop`, which `thrifty_amd.track` reads with its xdop / ydop and the NO_CANDIDATE flag.
"""
from __future__ import print_function

import argparse
import sys

import numpy as np

from thrifty_amd import _native, pos_3d, pos_est, pos_quality, tdoa_est

INCONSISTENT, EXCLUDED, NO_CANDIDATE = _native.POSQ3_INCONSISTENT, _native.POSQ3_EXCLUDED, _native.POSQ3_NO_CANDIDATE
MIN_RX_FLOOR = _native.POSQ3_MIN_RX     # (known height, free z)

QUALITY3_DTYPE = {
    "names": ("group_id", "timestamp", "tx", "dop", "hdop", "vdop", "snr", "x", "y", "z", "rms", "xdop", "ydop", "zdop",
              "major", "minor", "angle", "n_rx", "n_rows", "excluded", "flags"),
    "formats": ("i4", "f8", "i4") + ("f8",) * 14 + ("i4",) * 4,
}


def _options(rx_pos, height, free_z, exclude_gate_m, ratio, min_rx):
    """(ids, table[n_rx, 3], gate, min_rx) as thr_posq3 takes them; ValueError for what it would refuse."""
    if (height is None) == (not free_z):
        raise ValueError("give the transmitter's height (height=) or free_z=True: there is no default mode")
    ids, table = pos_3d._receiver_table(rx_pos)
    gate = 0.0 if exclude_gate_m is None else float(exclude_gate_m)
    if exclude_gate_m is not None and not (np.isfinite(gate) and gate > 0.0):
        raise ValueError("exclude_gate_m must be a positive number of metres (None: no exclusion), not %r" % (exclude_gate_m,))
    if not 0.0 < float(ratio) <= 1.0:
        raise ValueError("ratio must lie in (0, 1], not %r" % (ratio,))
    floor = MIN_RX_FLOOR[1 if free_z else 0]
    if min_rx is None:
        min_rx = floor
    if int(min_rx) != min_rx or not floor <= int(min_rx) <= _native.POS_MAX_RECEIVERS:
        raise ValueError("min_rx must lie in %d .. %d %s, not %r" % (
            floor, _native.POS_MAX_RECEIVERS, "with z free" if free_z else "with the height known", min_rx))
    return ids, table, gate, int(min_rx)


def quality3_columns(group_ptr, rx0, rx1, tdoa, snr, rx_pos, height=None, group_tx=None, free_z=False, z0=None, z_range=None,
                     weights=None, exclude_gate_m=None, ratio=0.5, min_rx=None, x0=(0.1, 0.1), max_iter=100, device_id=0):
    """Position quality for TDOA rows in CSR form (`pos_3d.pos3_columns`' conventions: rx0 / rx1 are receiver ids, keys
    of `rx_pos`, whose values hold x y z; exactly one of `height` and `free_z=True`).  `weights`: None, "snr" (the rows'
    snr) or one value >= 0 per row.  -> dict over ALL groups, in order, of every output of `_native.POSQ3_OUTPUTS` and
    `counts`; `excluded` and `task_rx` are receiver ids (`excluded` -1 for none), `n_rx` / `n_rows` the chosen task's
    receivers and rows, `rms_full` / `rms` the full solve's and the chosen task's."""
    ids, table, gate, min_rx = _options(rx_pos, height, free_z, exclude_gate_m, ratio, min_rx)
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
        z0, z_range = pos_3d.start_height(table, z0, z_range)
        mode, heights = _native.POS3_FREE_Z, None
    else:
        if z0 is not None or z_range is not None:
            raise ValueError("z0 and z_range belong to free_z=True")
        mode, heights, z0 = _native.POS3_KNOWN_HEIGHT, pos_3d.group_heights(height, len(ptr) - 1, group_tx), 0.0
    if isinstance(weights, str):
        if weights != "snr":
            raise ValueError("weights must be None, 'snr' or one value per row, not %r" % (weights,))
        weights = snr
    if weights is not None:
        weights = np.asarray(weights, dtype=np.float64)
        if weights.shape != (len(rx0),):
            raise ValueError("one weight per row: %d rows, weights of shape %r" % (len(rx0), weights.shape))
        if not np.all(np.isfinite(weights)) or np.any(weights < 0.0):
            raise ValueError("a weight is negative or not finite")
    lookup = np.vectorize(dense.__getitem__, otypes=[np.int32])
    counts, out = _native.posq3(ptr, lookup(rx0) if len(rx0) else rx0, lookup(rx1) if len(rx1) else rx1, tdoa, snr, table, mode,
                                heights, weights, gate, ratio, min_rx, (start[0], start[1], z0), z_range, max_iter,
                                device_id=device_id)
    id_of = np.array(ids, dtype=np.int64)
    excluded = out["counts"][:, 2].astype(np.int64)
    out["n_rx"], out["n_rows"] = out["counts"][:, 0].copy(), out["counts"][:, 1].copy()
    out["excluded"] = np.where(excluded >= 0, id_of[np.maximum(excluded, 0)], -1)
    out["task_rx"] = id_of[out["task_rx"]]
    out["rms_full"], out["rms"] = out["rms"][:, 0].copy(), out["rms"][:, 1].copy()
    out["counts"] = counts
    return out


def solve(tdoa_groups, rx_pos, height=None, free_z=False, z0=None, z_range=None, weights=None, exclude_gate_m=None, ratio=0.5,
          min_rx=None, max_iter=100, details=None):
    """Position quality of all TDOA groups (group_id, timestamp, tx, tdoas) in one device call -> structured array
    (QUALITY3_DTYPE), one record per solved group, in order; with the height known (a dict is looked up by each group's
    tx) `z` is that height.  Dropped groups print `pos_3d.solve`'s sentence.  `details`, a dict, receives the columns of
    `quality3_columns` for ALL groups, and `group_id`."""
    groups = list(tdoa_groups)
    _options(rx_pos, height, free_z, exclude_gate_m, ratio, min_rx)
    ptr = np.cumsum([0] + [len(group[3]) for group in groups])
    column = lambda name, kind: (np.concatenate([np.asarray(group[3][name], dtype=kind) for group in groups])  # noqa: E731
                                 if groups else np.zeros(0, dtype=kind))
    out = quality3_columns(ptr, column("rx0", np.int64), column("rx1", np.int64), column("tdoa", np.float64),
                           column("snr", np.float64), rx_pos, height=height, group_tx=[group[2] for group in groups],
                           free_z=free_z, z0=z0, z_range=z_range, weights=weights, exclude_gate_m=exclude_gate_m, ratio=ratio,
                           min_rx=min_rx, max_iter=max_iter)
    if details is not None:
        details.update(out, group_id=np.array([group[0] for group in groups], dtype=np.int64))
    return records(groups, out)


def records(groups, out):
    """The QUALITY3_DTYPE records of the groups that were solved, from the columns of `quality3_columns`."""
    status = out["status"]
    dropped = np.isin(status, list(pos_3d._DROPPED))
    for g in np.flatnonzero(dropped).tolist():
        print("Failed to estimate group #{}: {}".format(groups[g][0], pos_3d._DROPPED[int(status[g])]))
    keep = ~dropped
    results = np.zeros(int(keep.sum()), dtype=QUALITY3_DTYPE)
    for field, k in (("group_id", 0), ("timestamp", 1), ("tx", 2)):
        results[field] = [group[k] for group, kept in zip(groups, keep) if kept]
    for name in ("dop", "hdop", "vdop", "snr", "rms", "n_rx", "n_rows", "excluded", "flags"):
        results[name] = out[name][keep]
    for axis, name in enumerate(("x", "y", "z")):
        results[name] = out["pos"][keep, axis]
    q = out["q"][keep]
    for name, values in zip(("xdop", "ydop", "major", "minor", "angle"), pos_quality.ellipse(q[:, :3])):
        results[name] = values
    with np.errstate(invalid="ignore"):
        results["zdop"] = np.sqrt(q[:, 5])
    return results


def horizontal(results):
    """The horizontal part of QUALITY3_DTYPE records as `pos_quality.QUALITY_DTYPE` records, `dop` := `hdop`."""
    flat = np.zeros(len(results), dtype=pos_quality.QUALITY_DTYPE)
    for name in flat.dtype.names:
        flat[name] = results["hdop" if name == "dop" else name]
    return flat


def save_quality3(output, results):
    """One line per position (see the module docstring); `output` is a file name or an open text file."""
    if isinstance(output, str):
        with open(output, "w") as handle:
            return save_quality3(handle, results)
    for record in results:
        words = [str(int(record["group_id"])), "%.6f" % record["timestamp"], str(int(record["tx"]))]
        words += [repr(float(record[name])) if fmt == "f8" else str(int(record[name]))
                  for name, fmt in zip(QUALITY3_DTYPE["names"][3:], QUALITY3_DTYPE["formats"][3:])]
        output.write(" ".join(words) + "\n")


def load_quality3(fname):
    """The records of a .posq3 file."""
    if isinstance(fname, str):
        with open(fname, "r") as handle:
            return load_quality3(handle)
    rows = [line.decode() if isinstance(line, bytes) else line for line in fname]
    rows = [line.split() for line in rows if line.strip() and not line.lstrip().startswith("#")]
    data = np.zeros(len(rows), dtype=QUALITY3_DTYPE)
    for r, words in enumerate(rows):
        if len(words) != len(QUALITY3_DTYPE["names"]):
            raise ValueError("line %d holds %d fields, a .posq3 line holds %d" % (r + 1, len(words), len(QUALITY3_DTYPE["names"])))
        data[r] = tuple(float(w) if fmt == "f8" else int(w) for w, fmt in zip(words, QUALITY3_DTYPE["formats"]))
    return data


format_summary = pos_quality.format_summary     # the same lines: positions, inconsistent, excluded, per receiver


def _parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("tdoa", nargs="?", type=argparse.FileType("r"), default="data.tdoa",
                        help="tdoa data (\"-\" streams from stdin)")
    parser.add_argument("-o", "--output", dest="output", type=argparse.FileType("w"), default="data.posq3",
                        help="output file ('-' for stdout)")
    parser.add_argument("-r", "--rx-coordinates", dest="rx_pos", type=argparse.FileType("r"), default="pos-rx.cfg",
                        help="path to config file that contains the coordinates (x y z) of the receivers")
    mode = parser.add_mutually_exclusive_group(required=True)
    mode.add_argument("--height", type=float, metavar="H", help="the transmitters' known height [m]: solve x and y")
    mode.add_argument("--free-z", dest="free_z", action="store_true", help="solve x, y and z")
    parser.add_argument("--height-tx", dest="height_tx", type=pos_3d._tx_height, action="append", nargs="+", default=[],
                        metavar="TX=H", help="the known height of one transmitter (with --height, which serves the others)")
    parser.add_argument("--z0", type=float, help="the start's height with --free-z (pos_3d's default)")
    parser.add_argument("--z-range", dest="z_range", type=float, nargs=2, metavar=("LO", "HI"), help="the box on z with --free-z")
    parser.add_argument("--weights", choices=("snr",), default=None, help="weigh every TDOA by this column")
    parser.add_argument("--exclude", dest="gate_m", type=float, default=None, metavar="GATE_M",
                        help="r.m.s. residual [m] above which a group is re-solved without each receiver")
    parser.add_argument("--ratio", type=float, default=0.5, help="a receiver is excluded when that divides the r.m.s. residual by 1 / RATIO")
    parser.add_argument("--min-rx", dest="min_rx", type=int, default=None,
                        help="fewest receivers of a group that may lose one (default: %d with --height, %d with --free-z)" % MIN_RX_FLOOR)
    parser.add_argument("--pos", dest="pos", type=argparse.FileType("w"), default=None, help="also write the positions as a .pos file")
    parser.add_argument("--posq", dest="posq", type=argparse.FileType("w"), default=None,
                        help="also write the horizontal part as a .posq file (dop := hdop)")
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
        common = dict(weights=args.weights, exclude_gate_m=args.gate_m, ratio=args.ratio, min_rx=args.min_rx)
        try:
            if args.free_z:
                results = solve(tdoa_groups, rx_pos, free_z=True, z0=args.z0, z_range=args.z_range, **common)
            else:
                heights = [overrides.get(int(group[2]), args.height) for group in tdoa_groups]
                results = solve(tdoa_groups, rx_pos, height=heights, **common)
        except ValueError as err:
            sys.stderr.write("%s\n" % err)
            return 1
        save_quality3(args.output, results)
        if args.pos is not None:
            positions = np.zeros(len(results), dtype=pos_est._result_dtype(3 if args.free_z else 2))
            for name in positions.dtype.names:
                positions[name] = results[name]
            pos_est.save_positions(args.pos, positions)
        if args.posq is not None:
            pos_quality.save_quality(args.posq, horizontal(results))
        (sys.stderr if args.output is sys.stdout else sys.stdout).write(format_summary(results))
        return 0
    finally:
        for stream in (args.tdoa, args.rx_pos):
            if stream is not sys.stdin:
                stream.close()
        for stream in (args.output, args.pos, args.posq):
            if stream is None:
                continue
            if stream is sys.stdout:
                stream.flush()
            else:
                stream.close()


if __name__ == "__main__":
    sys.exit(_main())
