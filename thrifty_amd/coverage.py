#!/usr/bin/env python
"""
Where can this deployment position a tag?  A coverage map from the receiver positions and a timing noise, without a
recording: dilution of precision, the predicted and the simulated position error per cell of a raster over the site.

    python -m thrifty_amd.coverage -r pos-rx.cfg --sigma M --gross M [--sigma-rx ID=M ...] [--area X0 Y0 X1 Y1]
                                   [--grid NX NY] [--margin M] [--range M] [--trials T] [--seed S] [-o coverage.npz]
                                   [--raster rms|pred_rms|dop|gross|q95]

One device call (`thr_coverage`, csrc/coverage.hip; include/thrifty_hip.h states every rule), 2-D only.  For every
cell centre p:

* the receivers within `range_m` HEAR the cell (all of them without a range); fewer than three: the cell is UNCOVERED;
* `dop` is the number a `.pos` line would carry there, and `pred_sxx / pred_sxy / pred_syy / pred_rms` the covariance
  of `thrifty pos`' estimator -- unweighted least squares over ALL receiver pairs -- when receiver r's arrival carries
  independent noise of `sigma_m` metres: Cov = inv(N) M inv(N), N = sum g g' over the pairs, M = sum_r sigma_r^2 u_r u_r',
  u_r the signed sum of the rows' gradients that name r (the pairs' noises n_a - n_b share receivers, so the covariance is
  NOT sigma^2 inv(N));
* `trials` noisy transmissions are synthesised (Philox4x32-10 keyed by `seed`, one Box-Muller normal per cell, trial
  and receiver) and each is solved by `thrifty pos`' own iteration from its fixed start `x0`; a trial is GOOD when it
  converged and lies within `gross_m` of the cell centre; `bias_x/y`, `sxx/sxy/syy`, `rms` are taken over the good
  trials, `q50` / `q95` (nearest rank) over all of them, a trial without a position counting as +inf;
* flags: UNCOVERED (1), DEGENERATE (2: dop = -1), LOSSY (4: more than half of the trials are not good).

`sigma_m` and `gross_m` have no default: they are the deployment's.  256 trials, the 95 % point and "half" for LOSSY
are conventions of this interface, not measurements.
"""
from __future__ import print_function

import argparse
import sys

import numpy as np

from thrifty_amd import _native, tdoa_est

UNCOVERED, DEGENERATE, LOSSY = _native.COVERAGE_UNCOVERED, _native.COVERAGE_DEGENERATE, _native.COVERAGE_LOSSY
#: one character per cell, from the smallest value to the largest; see `CoverageMap.format_raster`
LADDER = ".:-=+*#%@"
RASTERS = ("rms", "pred_rms", "dop", "gross", "q95")
_CELL_ARRAYS = (("n_heard", "heard_mask", "flags", "iters_sum") + _native.COVERAGE_PRED + _native.COVERAGE_CELL_COUNTS +
                _native.COVERAGE_STATS)
_KEEP_ARRAYS = tuple(name for name in _native.COVERAGE_OUTPUTS if name.startswith("keep_"))


def _options(rx_pos, sigma_m, gross_m, area, grid, margin_m, range_m, trials, seed, x0, max_iter, keep):
    """Everything thr_coverage takes, checked: ValueError for what it would refuse."""
    ids = list(rx_pos)
    if not ids:
        raise ValueError("rx_pos is empty")
    table = [np.atleast_1d(np.asarray(rx_pos[i], dtype=np.float64)) for i in ids]
    if any(row.ndim != 1 or len(row) != 2 for row in table):
        raise ValueError("the coverage map works in 2 dimensions: every receiver needs two coordinates")
    if len(ids) > _native.POS_MAX_RECEIVERS:
        raise ValueError("at most %d receivers, not %d" % (_native.POS_MAX_RECEIVERS, len(ids)))
    table = np.array(table, dtype=np.float64).reshape(len(ids), 2)
    if not np.all(np.isfinite(table)):
        raise ValueError("a receiver coordinate is not finite")
    if isinstance(sigma_m, dict):
        missing = [i for i in ids if i not in sigma_m]
        if missing or len(sigma_m) != len(ids):
            raise ValueError("sigma_m as a dict needs one entry per receiver id (%r)" % (ids,))
        sigma = np.array([float(sigma_m[i]) for i in ids], dtype=np.float64)
    else:
        sigma = np.full(len(ids), float(sigma_m), dtype=np.float64)
    if not np.all(np.isfinite(sigma)) or np.any(sigma < 0.0):
        raise ValueError("sigma_m must be finite and not negative")
    if not (np.isfinite(gross_m) and float(gross_m) > 0.0):
        raise ValueError("gross_m must be a positive number of metres, not %r" % (gross_m,))
    box_lo, box_hi = table.min(axis=0), table.max(axis=0)
    if area is None:
        if margin_m is None:
            margin_m = float(np.max(box_hi - box_lo))
        if not (np.isfinite(margin_m) and float(margin_m) >= 0.0):
            raise ValueError("margin_m must be finite and not negative, not %r" % (margin_m,))
        lo, hi = box_lo - np.float64(margin_m), box_hi + np.float64(margin_m)
    else:
        corners = np.asarray(area, dtype=np.float64)
        if corners.shape != (4,) and corners.shape != (2, 2):
            raise ValueError("area holds x0, y0, x1, y1")
        lo, hi = corners.reshape(2, 2)
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo < hi)):
        raise ValueError("the area needs finite corners with lo < hi on both axes")
    if np.any(lo < box_lo - _native.POSG_MAX_MARGIN) or np.any(hi > box_hi + _native.POSG_MAX_MARGIN):
        raise ValueError("the area must lie within %g m of the receivers' bounding box (the solver's box)" % _native.POSG_MAX_MARGIN)
    nx, ny = grid
    if int(nx) != nx or int(ny) != ny or nx < 1 or ny < 1 or nx * ny > _native.COVERAGE_MAX_CELLS:
        raise ValueError("grid holds two whole numbers >= 1 whose product is at most %d, not %r" % (_native.COVERAGE_MAX_CELLS, grid))
    if int(trials) != trials or not 1 <= trials <= _native.COVERAGE_MAX_TRIALS:
        raise ValueError("trials must lie in 1 .. %d, not %r" % (_native.COVERAGE_MAX_TRIALS, trials))
    if nx * ny * trials > _native.COVERAGE_MAX_TASKS:
        raise ValueError("cells x trials may not pass %d" % _native.COVERAGE_MAX_TASKS)
    range_m = 0.0 if range_m is None else float(range_m)
    if not np.isfinite(range_m):
        raise ValueError("range_m must be finite")
    if int(seed) != seed or not 0 <= seed < 1 << 64:
        raise ValueError("seed must be a whole number in 0 .. 2^64 - 1, not %r" % (seed,))
    start = np.asarray(x0, dtype=np.float64)
    if start.shape != (2,) or not np.all(np.isfinite(start)):
        raise ValueError("x0 holds two finite values")
    if int(max_iter) != max_iter or max_iter < 0:
        raise ValueError("max_iter must be a whole number that is not negative, not %r" % (max_iter,))
    keep_first, keep_count = (0, 0) if keep is None else keep
    if not 0 <= keep_count <= _native.COVERAGE_MAX_KEEP or keep_first < 0 or keep_first + keep_count > nx * ny:
        raise ValueError("keep = (first cell, count) with count <= %d inside the %d cells, not %r" %
                         (_native.COVERAGE_MAX_KEEP, nx * ny, keep))
    return ids, table, sigma, lo, hi, int(nx), int(ny), range_m, start, int(keep_first), int(keep_count)


class CoverageMap(object):
    """The map: every per-cell array is shaped [ny, nx] (row j: cy[j], column i: cx[i]) and is an attribute -- n_heard,
    heard_mask, flags, iters_sum, dop, pred_sxx, pred_sxy, pred_syy, pred_rms, n_ok, n_at_bound, n_unconverged,
    n_nonfinite, n_good, n_gross, bias_x, bias_y, sxx, sxy, syy, rms, q50, q95 -- beside cx, cy, the receivers (`rx_ids`,
    `rx_pos` [n_rx, 2], `sigma` [n_rx]), the parameters (`params`), the device's `counts` and, when cells were kept,
    `kept` (the keep_* columns)."""

    def __init__(self, arrays, cx, cy, rx_ids, rx_pos, sigma, params, counts=None, kept=None):
        self.arrays = dict(arrays)
        self.cx, self.cy = np.asarray(cx), np.asarray(cy)
        self.rx_ids, self.rx_pos, self.sigma = list(rx_ids), np.asarray(rx_pos), np.asarray(sigma)
        self.params, self.counts, self.kept = dict(params), counts, kept

    def __getattr__(self, name):
        arrays = self.__dict__.get("arrays", {})
        if name in arrays:
            return arrays[name]
        raise AttributeError(name)

    @property
    def shape(self):
        return len(self.cy), len(self.cx)

    def cell(self, i, j):
        """Everything about the cell in column i, row j as a dict of scalars (with its centre x, y)."""
        out = {name: values[j, i].item() for name, values in self.arrays.items()}
        out["x"], out["y"] = float(self.cx[i]), float(self.cy[j])
        return out

    def save(self, npz):
        """All arrays, the receivers and the parameters to one .npz (see `load`)."""
        extra = {"param_" + key: np.asarray(value) for key, value in self.params.items()}
        np.savez(npz, cx=self.cx, cy=self.cy, rx_ids=np.asarray(self.rx_ids), rx_pos=self.rx_pos, sigma=self.sigma,
                 **dict(self.arrays, **extra))

    @classmethod
    def load(cls, npz):
        with np.load(npz) as data:
            arrays = {name: data[name] for name in _CELL_ARRAYS}
            params = {key[len("param_"):]: data[key][()] for key in data.files if key.startswith("param_")}
            return cls(arrays, data["cx"], data["cy"], data["rx_ids"].tolist(), data["rx_pos"], data["sigma"], params)

    def format_summary(self):
        """Covered and lossy cells, the median and the worst rms, and the median of rms / pred_rms."""
        flags = self.flags
        covered = (flags & UNCOVERED) == 0
        rms = self.rms[covered & np.isfinite(self.rms)]
        ok = covered & np.isfinite(self.rms) & np.isfinite(self.pred_rms) & (self.pred_rms > 0)
        ratio = self.rms[ok] / self.pred_rms[ok]
        number = lambda v, f: "%.3f" % f(v) if len(v) else "nan"     # noqa: E731
        return ("{} cells, {} covered, {} degenerate, {} lossy; rms median {} m, worst {} m; "
                "median rms / pred_rms {}\n").format(
                    flags.size, int(covered.sum()), int(np.count_nonzero(flags & DEGENERATE)), int(np.count_nonzero(flags & LOSSY)),
                    number(rms, np.median), number(rms, np.max), number(ratio, np.median))

    def format_raster(self, name="rms"):
        """A text raster of one column, the top line the largest y.  One character per cell: ' ' UNCOVERED, '?' no
        finite value, otherwise LADDER[k], k = floor(9 (v - min) / (max - min)) clipped to 0 .. 8 over the finite
        values of the covered cells ('gross' is n_gross / trials).  The last line names the ladder's ends."""
        if name not in RASTERS:
            raise ValueError("raster must be one of %r, not %r" % (RASTERS, name))
        values = self.n_gross / float(self.params["trials"]) if name == "gross" else np.asarray(getattr(self, name), dtype=np.float64)
        covered = (self.flags & UNCOVERED) == 0
        finite = covered & np.isfinite(values)
        lo, hi = (float(values[finite].min()), float(values[finite].max())) if finite.any() else (0.0, 0.0)
        span = hi - lo
        lines = []
        for j in range(values.shape[0] - 1, -1, -1):
            chars = []
            for i in range(values.shape[1]):
                if not covered[j, i]:
                    chars.append(" ")
                elif not finite[j, i]:
                    chars.append("?")
                else:
                    k = 0 if span == 0.0 else int(len(LADDER) * (values[j, i] - lo) / span)
                    chars.append(LADDER[min(max(k, 0), len(LADDER) - 1)])
            lines.append("".join(chars))
        lines.append("%s: '%s' = %.6g .. '%s' = %.6g (' ' uncovered, '?' no value)" % (name, LADDER[0], lo, LADDER[-1], hi))
        return "\n".join(lines) + "\n"


def coverage_map(rx_pos, sigma_m, gross_m, area=None, grid=(64, 64), margin_m=None, range_m=None, trials=256, seed=0,
                 x0=(0.1, 0.1), max_iter=100, keep=None, slab_groups=0, device_id=0):
    """The coverage map of the receivers `rx_pos` (id -> (x, y)) -> CoverageMap.  `sigma_m`: the arrival noise in metres,
    a scalar or a dict per receiver id.  `gross_m`: a trial farther than this from its cell centre is a gross error.
    `area` = (x0, y0, x1, y1), by default the receivers' bounding box grown by `margin_m` (default: its longer side).
    `keep` = (first cell, count <= 64): the device's own trials of those cells come back as `.kept`."""
    ids, table, sigma, lo, hi, nx, ny, range_m, start, keep_first, keep_count = _options(
        rx_pos, sigma_m, gross_m, area, grid, margin_m, range_m, trials, seed, x0, max_iter, keep)
    counts, out = _native.coverage(table, sigma, lo, hi, nx, ny, gross_m, trials=trials, range_m=range_m, seed=seed, x0=start,
                                   max_iter=max_iter, slab_groups=slab_groups, keep_first=keep_first, keep_count=keep_count,
                                   device_id=device_id)
    arrays = {name: out[name].reshape(ny, nx) for name in ("n_heard", "heard_mask", "flags", "iters_sum")}
    for table_name, names in (("pred", _native.COVERAGE_PRED), ("counts", _native.COVERAGE_CELL_COUNTS), ("stats", _native.COVERAGE_STATS)):
        for k, name in enumerate(names):
            arrays[name] = np.ascontiguousarray(out[table_name][:, k]).reshape(ny, nx)
    params = dict(lo=lo, hi=hi, gross_m=float(gross_m), range_m=range_m, trials=int(trials), seed=int(seed), x0=start,
                  max_iter=int(max_iter))
    kept = {name: out[name] for name in _KEEP_ARRAYS} if keep_count else None
    return CoverageMap(arrays, out["cx"], out["cy"], ids, table, sigma, params, counts=counts, kept=kept)


def _sigma_rx(text):
    ident, _, value = text.partition("=")
    try:
        return int(ident), float(value)
    except ValueError:
        raise argparse.ArgumentTypeError("--sigma-rx takes ID=M, not %r" % text)


_CLI = (
    (("-r", "--rx-coordinates"), dict(dest="rx_pos", type=argparse.FileType("r"), default="pos-rx.cfg",
                                      help="path to config file that contains the coordinates of the receivers")),
    (("--sigma",), dict(dest="sigma_m", type=float, required=True, metavar="M", help="arrival noise of every receiver [m]")),
    (("--gross",), dict(dest="gross_m", type=float, required=True, metavar="M", help="a position farther than this from the truth is a gross error [m]")),
    (("--sigma-rx",), dict(dest="sigma_rx", type=_sigma_rx, action="append", default=[], metavar="ID=M", help="arrival noise of one receiver [m]")),
    (("--area",), dict(type=float, nargs=4, default=None, metavar=("X0", "Y0", "X1", "Y1"), help="the raster's corners (default: the receivers' bounding box grown by --margin)")),
    (("--grid",), dict(type=int, nargs=2, default=(64, 64), metavar=("NX", "NY"), help="cells per axis")),
    (("--margin",), dict(dest="margin_m", type=float, default=None, metavar="M", help="metres the default area reaches beyond the receivers (default: the longer side of their bounding box)")),
    (("--range",), dict(dest="range_m", type=float, default=None, metavar="M", help="a receiver hears a cell within this distance (default: always)")),
    (("--trials",), dict(type=int, default=256, help="simulated transmissions per cell (1 .. 4096)")),
    (("--seed",), dict(type=int, default=0, help="the generator's 64-bit key")),
    (("-o", "--output"), dict(dest="output", default=None, metavar="coverage.npz", help="save every array")),
    (("--raster",), dict(choices=RASTERS, default=None, help="print a text raster of this column")),
)


def _parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for flags, options in _CLI:
        parser.add_argument(*flags, **options)
    return parser


def _main(argv=None):
    args = _parser().parse_args(argv)
    try:
        rx_pos = tdoa_est.load_pos_config(args.rx_pos)
    finally:
        args.rx_pos.close()
    sigma = args.sigma_m
    if args.sigma_rx:
        sigma = {ident: args.sigma_m for ident in rx_pos}
        for ident, value in args.sigma_rx:
            if ident not in sigma:
                sys.stderr.write("--sigma-rx names receiver %d, which the configuration does not list\n" % ident)
                return 1
            sigma[ident] = value
    try:
        result = coverage_map(rx_pos, sigma, args.gross_m, area=args.area, grid=tuple(args.grid), margin_m=args.margin_m,
                              range_m=args.range_m, trials=args.trials, seed=args.seed)
    except ValueError as err:
        sys.stderr.write("%s\n" % err)
        return 1
    if args.output is not None:
        result.save(args.output)
    sys.stdout.write(result.format_summary())
    if args.raster is not None:
        sys.stdout.write(result.format_raster(args.raster))
    return 0


if __name__ == "__main__":
    sys.exit(_main())
