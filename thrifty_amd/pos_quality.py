#!/usr/bin/env python
"""
Can this position be trusted?  Positions from TDOA values with their residuals, an error ellipse, and the
exclusion of one receiver whose arrivals contradict the others.

    python -m thrifty_amd.pos_quality [data.tdoa] -r pos-rx.cfg -o data.posq [--weights snr] [--exclude GATE_M]
                                      [--ratio R] [--min-rx N] [--pos data.pos]

`thrifty pos` (thrifty_amd/pos_est.py) gives a position `dop` and the mean `snr`; it cannot say that a group's
TDOAs contradict each other, nor act on it.  This module answers the open items of the reference's pos_est.py --
"use SNR or some confidence value as weight", "also return residual or a measure of the quality or confidence of
the estimate", "split DOP into multiple values (one per dimension)" -- in one device call (`thr_posq`,
csrc/posq.hip), 2-D only:

* every group is solved as `thrifty pos` solves it (the same iteration, csrc/pos_lm.hpp), optionally with a
  weight per row, normalised per group so that weights of one are the unweighted solve to the bit;
* `rms` is the root mean square of the (weighted) residuals in metres, `q = inv(A)` the inverse normal matrix:
  `xdop = sqrt(q00)`, `ydop = sqrt(q11)`, and the ellipse `major`, `minor` (square roots of q's eigenvalues) and
  `angle` (degrees from the x axis, 0.5 atan2(2 q01, q00 - q11));
* with `exclude_gate_m`, a group whose rms exceeds the gate and that names at least `min_rx` receivers is solved
  once more without each of its receivers; the best of those replaces the full solve when its rms is at most
  `ratio` times the full one.  The gate has no default: it is the deployment's noise level in metres.  0.5 and 5
  are conventions of this interface, not measurements; with fewer than five receivers a candidate has no
  redundant arrival left and always fits.

`.posq` text: one line per position, `group_id timestamp(%.6f) tx dop snr x y rms xdop ydop major minor angle
n_rx n_rows excluded flags`, floats as their shortest round-trip repr; `excluded` is a receiver id or -1, `flags`
the sum of INCONSISTENT (1), EXCLUDED (2) and NO_CANDIDATE (4).
"""
from __future__ import print_function

import argparse
import sys

import numpy as np

from thrifty_amd import _native, pos_est, tdoa_est

INCONSISTENT, EXCLUDED, NO_CANDIDATE = _native.POSQ_INCONSISTENT, _native.POSQ_EXCLUDED, _native.POSQ_NO_CANDIDATE
MIN_RX_FLOOR = _native.POSQ_MIN_RX

QUALITY_DTYPE = {
    "names": ("group_id", "timestamp", "tx", "dop", "snr", "x", "y", "rms", "xdop", "ydop", "major", "minor", "angle",
              "n_rx", "n_rows", "excluded", "flags"),
    "formats": ("i4", "f8", "i4") + ("f8",) * 10 + ("i4",) * 4,
}


def _options(rx_pos, exclude_gate_m, ratio, min_rx):
    """The receiver table and the gate as thr_posq takes it; ValueError for what it would refuse."""
    ids = list(rx_pos)
    if not ids:
        raise ValueError("rx_pos is empty")
    table = [np.atleast_1d(np.asarray(rx_pos[i], dtype=np.float64)) for i in ids]
    if any(row.ndim != 1 or len(row) != len(table[0]) for row in table):
        raise ValueError("the receivers' coordinates differ in length")
    if len(table[0]) != 2:
        raise ValueError("%d-D receiver coordinates: position quality is computed in 2 dimensions" % len(table[0]))
    if len(ids) > _native.POS_MAX_RECEIVERS:
        raise ValueError("at most %d receivers, not %d" % (_native.POS_MAX_RECEIVERS, len(ids)))
    gate = 0.0 if exclude_gate_m is None else float(exclude_gate_m)
    if exclude_gate_m is not None and not (np.isfinite(gate) and gate > 0.0):
        raise ValueError("exclude_gate_m must be a positive number of metres (None: no exclusion), not %r" % (exclude_gate_m,))
    if not 0.0 < float(ratio) <= 1.0:
        raise ValueError("ratio must lie in (0, 1], not %r" % (ratio,))
    if int(min_rx) != min_rx or not MIN_RX_FLOOR <= int(min_rx) <= _native.POS_MAX_RECEIVERS:
        raise ValueError("min_rx must lie in %d .. %d, not %r" % (MIN_RX_FLOOR, _native.POS_MAX_RECEIVERS, min_rx))
    return ids, np.array(table, dtype=np.float64).reshape(len(ids), 2), gate


def quality_columns(group_ptr, rx0, rx1, tdoa, snr, rx_pos, weights=None, exclude_gate_m=None, ratio=0.5, min_rx=5,
                    x0=(0.1, 0.1), max_iter=100, device_id=0):
    """Position quality for TDOA rows in CSR form (group g: rows group_ptr[g]:group_ptr[g + 1]; rx0 / rx1 are
    receiver ids, keys of `rx_pos`).  `weights`: None, "snr" (the rows' snr) or one value >= 0 per row.
    -> dict over ALL groups, in order, of every output of `_native.POSQ_OUTPUTS` and `counts`; `excluded` and
    `task_rx` are receiver ids (`excluded` -1 for none), `n_rx` / `n_rows` the chosen task's receivers and rows."""
    ids, table, gate = _options(rx_pos, exclude_gate_m, ratio, min_rx)
    ptr = np.asarray(group_ptr, dtype=np.int64)
    rx0, rx1 = np.asarray(rx0, dtype=np.int64), np.asarray(rx1, dtype=np.int64)
    if ptr.ndim != 1 or len(ptr) < 1 or ptr[0] != 0 or np.any(np.diff(ptr) < 0) or ptr[-1] != len(rx0):
        raise ValueError("group_ptr must start at 0, not decrease and end at the number of rows")
    dense = {rx: k for k, rx in enumerate(ids)}
    for rx in np.unique(np.concatenate([rx0, rx1])).tolist():
        if rx not in dense:
            raise KeyError(rx)
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
    counts, out = _native.posq(ptr, lookup(rx0) if len(rx0) else rx0, lookup(rx1) if len(rx1) else rx1, tdoa, snr, table,
                               weights, gate, ratio, min_rx, x0, max_iter, device_id=device_id)
    id_of = np.array(ids, dtype=np.int64)
    excluded = out["counts"][:, 2].astype(np.int64)
    out["n_rx"], out["n_rows"] = out["counts"][:, 0].copy(), out["counts"][:, 1].copy()
    out["excluded"] = np.where(excluded >= 0, id_of[np.maximum(excluded, 0)], -1)
    out["task_rx"] = id_of[out["task_rx"]]
    out["rms_full"], out["rms"] = out["rms"][:, 0].copy(), out["rms"][:, 1].copy()
    out["counts"] = counts
    return out


def ellipse(q):
    """q[n, 3] = (q00, q01, q11) -> (xdop, ydop, major, minor, angle in degrees); NaN where q is."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    q00, q01, q11 = q[:, 0], q[:, 1], q[:, 2]
    with np.errstate(all="ignore"):
        half, diff = 0.5 * (q00 + q11), 0.5 * (q00 - q11)
        root = np.sqrt(diff * diff + q01 * q01)
        major, minor = np.sqrt(half + root), np.sqrt(np.maximum(half - root, 0.0))
        angle = np.degrees(0.5 * np.arctan2(2.0 * q01, q00 - q11))
        return np.sqrt(q00), np.sqrt(q11), major, minor, angle


def solve(tdoa_groups, rx_pos, weights=None, exclude_gate_m=None, ratio=0.5, min_rx=5, max_iter=100):
    """Position quality of all TDOA groups (group_id, timestamp, tx, tdoas) in one device call -> structured array
    (QUALITY_DTYPE), one record per solved group, in order.  Dropped groups print `pos_est.solve`'s sentence."""
    groups = list(tdoa_groups)
    _options(rx_pos, exclude_gate_m, ratio, min_rx)
    ptr = np.cumsum([0] + [len(group[3]) for group in groups])
    column = lambda name, kind: (np.concatenate([np.asarray(group[3][name], dtype=kind) for group in groups])  # noqa: E731
                                 if groups else np.zeros(0, dtype=kind))
    out = quality_columns(ptr, column("rx0", np.int64), column("rx1", np.int64), column("tdoa", np.float64),
                          column("snr", np.float64), rx_pos, weights=weights, exclude_gate_m=exclude_gate_m, ratio=ratio,
                          min_rx=min_rx, max_iter=max_iter)
    status = out["status"]
    dropped = pos_est._DROPPED
    for g in np.flatnonzero(np.isin(status, list(dropped))).tolist():
        print("Failed to estimate group #{}: {}".format(groups[g][0], dropped[int(status[g])]))
    keep = ~np.isin(status, list(dropped))
    results = np.zeros(int(keep.sum()), dtype=QUALITY_DTYPE)
    results["group_id"] = [group[0] for group, k in zip(groups, keep) if k]
    results["timestamp"] = [group[1] for group, k in zip(groups, keep) if k]
    results["tx"] = [group[2] for group, k in zip(groups, keep) if k]
    results["dop"], results["snr"] = out["dop"][keep], out["snr"][keep]
    results["x"], results["y"] = out["pos"][keep, 0], out["pos"][keep, 1]
    results["rms"] = out["rms"][keep]
    for name, values in zip(("xdop", "ydop", "major", "minor", "angle"), ellipse(out["q"][keep])):
        results[name] = values
    for name in ("n_rx", "n_rows", "excluded", "flags"):
        results[name] = out[name][keep]
    return results


def save_quality(output, results):
    """One line per position (see the module docstring); `output` is a file name or an open text file."""
    if isinstance(output, str):
        with open(output, "w") as handle:
            return save_quality(handle, results)
    for record in results:
        words = [str(int(record["group_id"])), "%.6f" % record["timestamp"], str(int(record["tx"]))]
        words += [repr(float(record[name])) if fmt == "f8" else str(int(record[name]))
                  for name, fmt in zip(QUALITY_DTYPE["names"][3:], QUALITY_DTYPE["formats"][3:])]
        output.write(" ".join(words) + "\n")


def load_quality(fname):
    """The records of a .posq file."""
    if isinstance(fname, str):
        with open(fname, "r") as handle:
            return load_quality(handle)
    rows = [line.decode() if isinstance(line, bytes) else line for line in fname]
    rows = [line.split() for line in rows if line.strip() and not line.lstrip().startswith("#")]
    data = np.zeros(len(rows), dtype=QUALITY_DTYPE)
    for r, words in enumerate(rows):
        if len(words) != len(QUALITY_DTYPE["names"]):
            raise ValueError("line %d holds %d fields, a .posq line holds %d" % (r + 1, len(words), len(QUALITY_DTYPE["names"])))
        data[r] = tuple(float(w) if fmt == "f8" else int(w) for w, fmt in zip(words, QUALITY_DTYPE["formats"]))
    return data


def format_summary(results):
    """The groups, how many were inconsistent, how many had a receiver excluded, and the exclusions per receiver."""
    flags = np.asarray(results["flags"])
    excluded = np.asarray(results["excluded"])[(flags & EXCLUDED) != 0]
    lines = ["{} positions, {} inconsistent, {} with a receiver excluded".format(
        len(results), int(np.count_nonzero(flags & INCONSISTENT)), len(excluded))]
    for rx, count in zip(*np.unique(excluded, return_counts=True)):
        lines.append("  RX {}: excluded {} times".format(int(rx), int(count)))
    return "\n".join(lines) + "\n"


_CLI = (
    (("tdoa",), dict(nargs="?", type=argparse.FileType("r"), default="data.tdoa", help="tdoa data (\"-\" streams from stdin)")),
    (("-o", "--output"), dict(dest="output", type=argparse.FileType("w"), default="data.posq", help="output file ('-' for stdout)")),
    (("-r", "--rx-coordinates"), dict(dest="rx_pos", type=argparse.FileType("r"), default="pos-rx.cfg",
                                      help="path to config file that contains the coordinates of the receivers")),
    (("--weights",), dict(choices=("snr",), default=None, help="weigh every TDOA by this column")),
    (("--exclude",), dict(dest="gate_m", type=float, default=None, metavar="GATE_M",
                          help="r.m.s. residual [m] above which a group is re-solved without each receiver")),
    (("--ratio",), dict(type=float, default=0.5, help="a receiver is excluded when that divides the r.m.s. residual by 1 / RATIO")),
    (("--min-rx",), dict(dest="min_rx", type=int, default=5, help="fewest receivers of a group that may lose one")),
    (("--pos",), dict(dest="pos", type=argparse.FileType("w"), default=None, help="also write the positions as a .pos file")),
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
        tdoa_groups = tdoa_est.load_tdoa_groups(args.tdoa)
        rx_pos = tdoa_est.load_pos_config(args.rx_pos)
        try:
            results = solve(tdoa_groups, rx_pos, weights=args.weights, exclude_gate_m=args.gate_m, ratio=args.ratio,
                            min_rx=args.min_rx)
        except ValueError as err:
            sys.stderr.write("%s\n" % err)
            return 1
        save_quality(args.output, results)
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
