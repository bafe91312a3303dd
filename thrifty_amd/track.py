#!/usr/bin/env python
"""
Where was the tag, and how fast?  Tracks from positions: per transmitter a constant-velocity Kalman filter over the
positions in time order, a gate that leaves out the positions the track contradicts, and a fixed-interval smoother.

    python -m thrifty_amd.track [data.pos|data.posq] -o data.track --sigma M --accel A [--speed-prior V] [--gate G]
                                [--rounds N] [--tx T ...] [--filter-only] [--npz FILE]

`thrifty pos` solves each position from one transmission alone, and `thrifty_amd.pos_quality` says how far one
position can be trusted.  This module combines the positions of one transmitter over time -- the last open item of
the reference's pos_est.py ("apply Kalman filter or something to average out the position estimates (move to separate
module)") -- in one device call (`thr_track`, csrc/track.hip), 2-D only.  include/thrifty_hip.h states the model.

* `sigma_m` scales the dilution of precision into metres: with `.posq` columns the measurement variances are
  `(sigma_m * xdop)**2` and `(sigma_m * ydop)**2`, with `.pos` columns both are `(sigma_m * dop)**2 / 2`.  Rows with
  non-finite x or y, a dop that is not finite or not positive, or (`.posq`) the NO_CANDIDATE flag are invalid: they
  are predicted through, not measured.
* `accel` (m/s^2 per sqrt(Hz), i.e. m s^-3/2) is the strength of the white acceleration noise: the filter's
  `q = accel**2` in m^2/s^3.  A tag that changes its velocity by about `a` m/s^2 over times of about `T` s has
  `accel` near `a * sqrt(T)`.  Neither `sigma_m` nor `accel` has a default: they are the deployment's.
* `speed_prior` (10 m/s), `gate` (the 99.9 % point of chi^2 with 2 degrees of freedom), `max_rounds` (4) and LOST
  ("fewer than half of the valid rows were used") are conventions of this interface, not measurements.
* An outlier as a track's FIRST valid row is the known way to lose a track: the filter starts there, and every later
  position contradicts it.  The remedy is to mark that row invalid (drop it from the input).
* The two axes are filtered independently; the full 4-state filter with `.posq`'s q01 is out of scope.

`.track` text: one line per tracked input row in (tx, timestamp) order, `group_id timestamp(%.6f) tx x y vx vy sx sy
speed nis used`, floats as their shortest round-trip repr; x .. vy are the smoothed state (the filtered one with
--filter-only), sx and sy the standard deviations of x and y, speed = hypot(vx, vy) in m/s.
"""
from __future__ import print_function

import argparse
import sys

import numpy as np

from thrifty_amd import _native, pos_est, pos_quality

GATE_999 = _native.TRACK_GATE_999
LOST = _native.TRACK_LOST

TRACK_DTYPE = {
    "names": ("group_id", "timestamp", "tx", "x", "y", "vx", "vy", "sx", "sy", "speed", "nis", "used"),
    "formats": ("i4", "f8", "i4") + ("f8",) * 8 + ("i4",),
}


def _checked(tx, timestamp, x, y, rx, ry, valid, accel, speed_prior, gate, max_rounds):
    """The columns and options as thr_track takes them; ValueError for what it would refuse (before the library loads)."""
    tx = np.asarray(tx)
    cols = [np.asarray(v, dtype=np.float64) for v in (timestamp, x, y, rx, ry)]
    if tx.ndim != 1 or any(v.shape != tx.shape for v in cols):
        raise ValueError("tx, timestamp, x, y, rx and ry are one-dimensional and of one length")
    ok = np.ones(len(tx), dtype=bool) if valid is None else np.asarray(valid).astype(bool)
    if ok.shape != tx.shape:
        raise ValueError("valid holds one value per row")
    if accel is None:
        raise ValueError("accel has no default: it is the deployment's")
    accel, speed_prior, gate = float(accel), float(speed_prior), float(gate)
    if not (np.isfinite(accel) and accel >= 0.0):
        raise ValueError("accel must be finite and not negative, not %r" % (accel,))
    if not (np.isfinite(speed_prior) and speed_prior > 0.0):
        raise ValueError("speed_prior must be finite and positive, not %r" % (speed_prior,))
    if not (np.isfinite(gate) and gate >= 0.0):
        raise ValueError("gate must be finite and not negative (0: no gating), not %r" % (gate,))
    if int(max_rounds) != max_rounds or not 1 <= int(max_rounds) <= 16:
        raise ValueError("max_rounds must lie in 1 .. 16, not %r" % (max_rounds,))
    if not np.all(np.isfinite(cols[0])):
        raise ValueError("a timestamp is not finite")
    if not (np.all(np.isfinite(cols[1][ok])) and np.all(np.isfinite(cols[2][ok]))):
        raise ValueError("a valid row has a position that is not finite")
    for v in cols[3:]:
        if not (np.all(np.isfinite(v[ok])) and np.all(v[ok] > 0.0)):
            raise ValueError("a valid row has a variance that is not finite or not positive")
    return tx.astype(np.int32), cols, (None if valid is None else ok.astype(np.uint8)), accel * accel, speed_prior, gate


def track_columns(tx, timestamp, x, y, rx, ry, valid=None, accel=None, speed_prior=10.0, gate=GATE_999, max_rounds=4,
                  device_id=0):
    """Tracks over one row per position (rx, ry: the measurement variances of the two axes in m^2; accel in
    m s^-3/2, see the module docstring) -> dict of every output of `_native.TRACK_OUTPUTS`, the per-row arrays in
    input row order, and `counts`."""
    tx, cols, mask, q, v0, gate = _checked(tx, timestamp, x, y, rx, ry, valid, accel, speed_prior, gate, max_rounds)
    counts, out = _native.track(tx, *cols, valid=mask, q=q, v0=v0, gate=gate, max_rounds=int(max_rounds), device_id=device_id)
    out["counts"] = counts
    return out


def measurement_columns(positions, sigma_m):
    """(rx, ry, valid) of a structured array from `pos_est.load_positions` or `pos_quality.load_quality`."""
    names = positions.dtype.names
    if "x" not in names or "y" not in names:
        raise ValueError("1-D positions cannot be tracked: thr_track works in 2 dimensions")
    if "z" in names:
        raise ValueError("3-D positions cannot be tracked: thr_track works in 2 dimensions")
    sigma_m = float(sigma_m)
    if not (np.isfinite(sigma_m) and sigma_m > 0.0):
        raise ValueError("sigma_m must be a positive number of metres, not %r" % (sigma_m,))
    x, y = np.asarray(positions["x"], dtype=np.float64), np.asarray(positions["y"], dtype=np.float64)
    valid = np.isfinite(x) & np.isfinite(y)
    with np.errstate(all="ignore"):
        if "xdop" in names:
            xdop, ydop = np.asarray(positions["xdop"], dtype=np.float64), np.asarray(positions["ydop"], dtype=np.float64)
            valid &= np.isfinite(xdop) & np.isfinite(ydop) & (xdop > 0.0) & (ydop > 0.0)
            valid &= (np.asarray(positions["flags"]) & pos_quality.NO_CANDIDATE) == 0
            rx, ry = (sigma_m * xdop) ** 2, (sigma_m * ydop) ** 2
        else:
            dop = np.asarray(positions["dop"], dtype=np.float64)
            valid &= np.isfinite(dop) & (dop > 0.0)
            rx = (sigma_m * dop) ** 2 / 2.0
            ry = rx.copy()
        valid &= np.isfinite(rx) & np.isfinite(ry) & (rx > 0.0) & (ry > 0.0)      # a product that left float64's range
    return rx, ry, valid


def track(positions, sigma_m, accel, speed_prior=10.0, gate=GATE_999, max_rounds=4, filter_only=False, tx=None):
    """Tracks of the positions (a structured array from `pos_est.load_positions` or `pos_quality.load_quality`)
    -> (records, out): one TRACK_DTYPE record per tracked input row in (tx, timestamp) order, and track_columns'
    dict with `rows`, the input rows `out` speaks of (all of them, or those of the transmitters listed in `tx`)."""
    rx, ry, valid = measurement_columns(positions, sigma_m)
    rows = np.arange(len(positions)) if tx is None else np.flatnonzero(np.isin(positions["tx"], list(tx)))
    sub = positions[rows]
    out = track_columns(sub["tx"], sub["timestamp"], sub["x"], sub["y"], rx[rows], ry[rows], valid[rows], accel=accel,
                        speed_prior=speed_prior, gate=gate, max_rounds=max_rounds)
    out["rows"] = rows
    state, var = (out["filt"], out["filt_var"]) if filter_only else (out["smooth"], out["smooth_var"])
    order = out["order"]
    order = order[~np.isnan(state[order, 0])]
    records = np.zeros(len(order), dtype=TRACK_DTYPE)
    records["group_id"], records["timestamp"], records["tx"] = sub["group_id"][order], sub["timestamp"][order], sub["tx"][order]
    for k, name in enumerate(("x", "vx", "y", "vy")):
        records[name] = state[order, k]
    records["sx"], records["sy"] = np.sqrt(var[order, 0]), np.sqrt(var[order, 3])
    records["speed"] = np.sqrt(state[order, 1] * state[order, 1] + state[order, 3] * state[order, 3])
    records["nis"], records["used"] = out["nis"][order], out["used"][order]
    return records, out


def save_tracks(output, records):
    """One line per tracked row (see the module docstring); `output` is a file name or an open text file."""
    if isinstance(output, str):
        with open(output, "w") as handle:
            return save_tracks(handle, records)
    for record in records:
        words = [str(int(record["group_id"])), "%.6f" % record["timestamp"], str(int(record["tx"]))]
        words += [repr(float(record[name])) if fmt == "f8" else str(int(record[name]))
                  for name, fmt in zip(TRACK_DTYPE["names"][3:], TRACK_DTYPE["formats"][3:])]
        output.write(" ".join(words) + "\n")


def load_tracks(fname):
    """The records of a .track file."""
    if isinstance(fname, str):
        with open(fname, "r") as handle:
            return load_tracks(handle)
    rows = [line.decode() if isinstance(line, bytes) else line for line in fname]
    rows = [line.split() for line in rows if line.strip() and not line.lstrip().startswith("#")]
    data = np.zeros(len(rows), dtype=TRACK_DTYPE)
    for r, words in enumerate(rows):
        if len(words) != len(TRACK_DTYPE["names"]):
            raise ValueError("line %d holds %d fields, a .track line holds %d" % (r + 1, len(words), len(TRACK_DTYPE["names"])))
        data[r] = tuple(float(w) if fmt == "f8" else int(w) for w, fmt in zip(words, TRACK_DTYPE["formats"]))
    return data


def format_summary(out):
    """One line per transmitter: rows, used, rejected, mean nis, duration, path, mean speed in km/h, and LOST."""
    lines = []
    for tx, stats, flags in zip(out["track_tx"], out["track_stats"], out["track_flags"]):
        lines.append("TX {}: {} rows, {} used, {} rejected, mean nis {:.3f}, {:.3f} s, path {:.3f} m, mean speed {:.3f} km/h{}".format(
            int(tx), int(stats[0]), int(stats[2]), int(stats[3]), stats[4], stats[5], stats[6], stats[7] * 3.6,
            ", LOST" if int(flags) & LOST else ""))
    return "\n".join(lines) + ("\n" if lines else "")


def load_input(stream):
    """A .pos or a .posq file, told apart by the number of columns."""
    lines = [line.decode() if isinstance(line, bytes) else line for line in stream]
    first = next((line.split() for line in lines if line.strip() and not line.lstrip().startswith("#")), None)
    if first is not None and len(first) == len(pos_quality.QUALITY_DTYPE["names"]):
        return pos_quality.load_quality(lines)
    return pos_est.load_positions(lines)


_CLI = (
    (("positions",), dict(nargs="?", type=argparse.FileType("r"), default="data.pos", help="a .pos or a .posq file (\"-\": stdin)")),
    (("-o", "--output"), dict(dest="output", type=argparse.FileType("w"), default="data.track", help="output file ('-' for stdout)")),
    (("--sigma",), dict(dest="sigma_m", type=float, required=True, metavar="M",
                        help="metres per unit of dop: the range noise of the deployment")),
    (("--accel",), dict(type=float, required=True, metavar="A", help="white acceleration noise [m s^-3/2]; q = A^2")),
    (("--speed-prior",), dict(dest="speed_prior", type=float, default=10.0, metavar="V",
                              help="standard deviation of the velocity at a track's start [m/s]")),
    (("--gate",), dict(type=float, default=GATE_999, metavar="G", help="largest nis of a position that is used (0: no gate)")),
    (("--rounds",), dict(dest="max_rounds", type=int, default=4, metavar="N", help="gate rounds at most (1 .. 16)")),
    (("--tx",), dict(type=int, nargs="+", default=None, metavar="T", help="only these transmitters")),
    (("--filter-only",), dict(dest="filter_only", action="store_true",
                              help="write the filtered states, what a live system would have seen, not the smoothed ones")),
    (("--npz",), dict(default=None, metavar="FILE", help="also save every array of the call")),
)


def _parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for flags, options in _CLI:
        parser.add_argument(*flags, **options)
    return parser


def _main(argv=None):
    args = _parser().parse_args(argv)
    try:
        try:
            positions = load_input(args.positions)
            records, out = track(positions, args.sigma_m, args.accel, speed_prior=args.speed_prior, gate=args.gate,
                                 max_rounds=args.max_rounds, filter_only=args.filter_only, tx=args.tx)
        except ValueError as err:
            sys.stderr.write("%s\n" % err)
            return 1
        save_tracks(args.output, records)
        if args.npz is not None:
            counts = out["counts"]
            arrays = {name: value for name, value in out.items() if name != "counts"}
            arrays.update({"count_" + name: np.int64(value) for name, value in counts.items()})
            np.savez(args.npz, **arrays)
        (sys.stderr if args.output is sys.stdout else sys.stdout).write(format_summary(out))
        return 0
    finally:
        if args.positions is not sys.stdin:
            args.positions.close()
        if args.output is sys.stdout:
            args.output.flush()
        else:
            args.output.close()


if __name__ == "__main__":
    sys.exit(_main())
