"""How far along the baseline is the tag, and how fast is it moving?  The numbers of the reference's
scripts/reldist_nearest.py, for every (mobile, beacon, rx0 < rx1) cell of a deployment in one device call.

    python -m thrifty_amd.reldist [toads] [matches] --beacon B [--tx T --rx0 R --rx1 R] [--method nearest|linpol]
                                  [-r pos-rx.cfg -b pos-beacon.cfg] [-s RATE] [--block-size N] [--carrier-hz F]
                                  [--frac 0.025] [--all] [-o reldist.npz]

For two receivers, a beacon and a mobile: the mobile's SOA difference minus the beacon's (taken at the nearest
beacon transmission, or interpolated between the two around it) cancels the receivers' clock offset and leaves
TDOA(mobile) - TDOA(beacon) in samples.  A mobile on the baseline at p from rx1 has TDOA 2 p - D, so with
d_beacon = |b - rx1| - |b - rx0|, dist_rx = |rx1 - rx0| and dist_beacon = |b - rx1| (each in samples: metres over
s2m = 2.997e8 / sample_rate) the position relative to the beacon is (raw + d_beacon + dist_rx) / 2 - dist_beacon.
Its difference over time is a speed; the carrier's Doppler difference is a second, independent one.  Both are
smoothed by a local linear regression.  `rel_dist` returns everything (thr_reldist, csrc/reldist.hip);
`format_report` prints the script's lines for a cell and one more.  No plots, and not the script's seven
hand-picked cuts.

Deviations from the script, each with a test (tests/test_gpu_reldist*.py):
 - the geometry, the sample rate, the block length and the carrier frequency are arguments (the script's are one
   recording's constants);
 - with `linpol`, a row outside the beacon's span holds the end row and is flagged (the script is defined for the
   last row only, and raises or wraps around elsewhere);
 - the smoother is the definition in include/thrifty_hip.h -- LOWESS without a robustness iteration, pinned to its
   NumPy statement (tests/reldist_ref.py), not to statsmodels.lowess(it=0), which is not installed where this is
   built and tested;
 - a cell whose beacon rows are not in SOA order (np.searchsorted is undefined there) is flagged and left NaN.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from thrifty_amd import _native, matchmaker, tdoa_est, toads_data
from thrifty_amd.beacon_analysis import _as_csr

LIGHT = 2.997e8
ROW_HELD = _native.RELDIST_ROW_HELD
CELL_UNSORTED, CELL_NO_BEACON = _native.RELDIST_CELL_UNSORTED, _native.RELDIST_CELL_NO_BEACON


def geometry_row(beacon, rx0, rx1, beacon_xy, rx0_xy, rx1_xy, sample_rate):
    """(beacon, rx0, rx1, d_beacon, dist_rx, dist_beacon), the three distances in samples."""
    s2m = LIGHT / sample_rate
    b, p0, p1 = (np.asarray(v, dtype=np.float64) for v in (beacon_xy, rx0_xy, rx1_xy))
    to_rx1, to_rx0 = np.linalg.norm(b - p1), np.linalg.norm(b - p0)
    return (int(beacon), int(rx0), int(rx1), float(to_rx1 - to_rx0) / s2m, float(np.linalg.norm(p1 - p0)) / s2m, float(to_rx1) / s2m)


def geometry_table(rx_pos, beacon_pos, sample_rate):
    """One geometry_row per beacon and receiver pair that both position tables ({id: coordinates}) know."""
    if not rx_pos or not beacon_pos:
        return []
    ids = sorted(rx_pos)
    return [geometry_row(b, r0, r1, beacon_pos[b], rx_pos[r0], rx_pos[r1], sample_rate)
            for b in sorted(beacon_pos) for i, r0 in enumerate(ids) for r1 in ids[i + 1:]]


class RelDist(object):
    """The arrays of one thr_reldist call, one attribute per output (_native.RELDIST_OUTPUTS), plus `counts`,
    `method`, `sample_rate` and `s2m`."""

    def __init__(self, counts, arrays, method, sample_rate):
        self.counts = dict(counts)
        self.names = tuple(arrays)
        for name, value in arrays.items():
            setattr(self, name, value)
        self.method, self.sample_rate, self.s2m = method, float(sample_rate), LIGHT / float(sample_rate)

    def __len__(self):
        return len(self.cell_key)

    @property
    def cells(self):
        """[(mobile, beacon, rx0, rx1)] in the order of the arrays."""
        return [tuple(key) for key in self.cell_key.tolist()]

    def index(self, mobile, beacon, rx0, rx1):
        hit = np.flatnonzero(np.all(self.cell_key == (mobile, beacon, rx0, rx1), axis=1))
        if len(hit) == 0:
            raise KeyError("no match of mobile %r holds receivers %r and %r (beacon %r)" % (mobile, rx0, rx1, beacon))
        return int(hit[0])

    def cell(self, mobile, beacon, rx0, rx1):
        """Everything about one cell as a dict: row arrays and masks, the statistics, the speed and the doppler
        series with their smoothed curves."""
        c = self.index(mobile, beacon, rx0, rx1)
        a, b = self.cell_ptr[c:c + 2]
        out = {"mobile": int(mobile), "beacon": int(beacon), "rx0": int(rx0), "rx1": int(rx1), "flags": int(self.cell_flags[c]),
               "rows": self.row_det[a:b], "matches": self.row_match[a:b], "nearest": self.nearest_idx[a:b], "hi": self.hi[a:b],
               "held": (self.row_flags[a:b] & ROW_HELD) != 0, "raw": self.raw[a:b], "x": self.x[a:b],
               "outlier": self.mask1[a:b] != 0, "doppler": self.dop[a:b], "doppler_outlier": self.mask3[a:b] != 0}
        out.update(zip(("count", "mean", "std", "min", "max", "within_std"), self.cell_stats[c].tolist()))
        out.update(zip(("median", "mad", "speed_median", "speed_mad", "doppler_median", "doppler_mad"), self.medians[c].tolist()))
        a, b = self.speed_ptr[c:c + 2]
        out.update(speed_x=self.speed_x[a:b], speed=self.speed[a:b], speed_outlier=self.mask2[a:b] != 0)
        for stem, name in (("speed", "speed"), ("dop", "doppler")):
            a, b = getattr(self, stem + "_smooth_ptr")[c:c + 2]
            out[name + "_smooth_x"] = getattr(self, stem + "_smooth_x")[a:b]
            out[name + "_smooth"] = getattr(self, stem + "_smooth")[a:b]
        return out

    def format_report(self, c):
        return format_report(self, c)

    def save(self, path):
        np.savez(path, method=self.method, sample_rate=self.sample_rate, **{name: getattr(self, name) for name in self.names})


def _as_columns(detections):
    if isinstance(detections, dict):
        return detections
    if not isinstance(detections, np.ndarray):
        detections = toads_data.toads_array(list(detections), with_ids=True)
    return {name: detections[name] for name, _ in _native.RELDIST_COLUMNS}


def rel_dist(detections, matches, beacons, mobiles=None, receivers=None, method="linpol", sample_rate=2.4e6, block_len=16384,
             carrier_hz=433e6, rx_pos=None, beacon_pos=None, smooth_frac=0.025, thresh=3.5, geometry=None, device_id=0):
    """Relative distance, speed and Doppler of every (mobile, beacon, rx0 < rx1) cell.  `detections`: DetectionResult
    objects, a toads_array, or a dict of the columns rxid, txid, soa, timestamp, carrier_bin, carrier_offset, idx;
    `matches`: lists of detection indices, or (match_ptr, match_idx); `beacons`: the beacons' transmitter ids;
    `mobiles`: None for every other transmitter; `rx_pos` / `beacon_pos`: {id: coordinates in metres}, from which
    the geometry of every cell is taken (zeros without them), or `geometry`: the table itself, rows of
    (beacon, rx0, rx1, d_beacon, dist_rx, dist_beacon) in samples.  ValueError for what thr_reldist refuses."""
    cols = _as_columns(detections)
    ptr, idx = _as_csr(matches)
    if geometry is None:
        geometry = geometry_table(rx_pos, beacon_pos, sample_rate)
    counts, arrays = _native.reldist(cols, ptr, idx, np.atleast_1d(beacons), mobiles, receivers, method, sample_rate, block_len,
                                     carrier_hz, thresh, smooth_frac, geometry, device_id=device_id)
    return RelDist(counts, arrays, method, sample_rate)


def _median(values):
    return float(np.median(values)) if len(values) else float("nan")


def format_report(result, c):
    """The script's three lines for cell number `c`, and one more: the share of kept rows within one standard
    deviation, the medians of the smoothed speed and of the smoothed Doppler in km/h."""
    count, mean, std, _, _, within = result.cell_stats[c]
    rows = int(result.cell_counts[c, 0])
    a, b = result.speed_smooth_ptr[c:c + 2]
    speed = _median(result.speed_smooth[a:b]) * 3.6
    a, b = result.dop_smooth_ptr[c:c + 2]
    doppler = _median(result.dop_smooth[a:b])
    lines = ["Number of outliers: {} / {}".format(rows - int(count), rows), "mean = {}".format(float(mean)),
             "std = {}".format(float(std)),
             "within one std = {:.0f}%; median smoothed speed = {:.1f} km/h; median smoothed Doppler = {:.1f} km/h".format(
                 100.0 * within / count if count else float("nan"), speed, doppler)]
    if result.cell_flags[c] & CELL_NO_BEACON:
        lines.append("No beacon row at this pair of receivers")
    elif result.cell_flags[c] & CELL_UNSORTED:
        lines.append("The rows are not in SOA (or timestamp) order: nothing computed")
    return "\n".join(lines) + "\n"


_CLI = (
    (("toads",), dict(nargs="?", type=argparse.FileType("rb"), default="rx.toads", help="toads data ('-' streams from stdin)")),
    (("matches",), dict(nargs="?", type=argparse.FileType("rb"), default="rx.match", help="match data")),
    (("--beacon",), dict(type=int, action="append", required=True, help="transmitter ID of a beacon (may be repeated)")),
    (("--tx",), dict(type=int, default=1, help="transmitter ID of the mobile")),
    (("--rx0",), dict(type=int, default=0, help="receiver ID of the first receiver")),
    (("--rx1",), dict(type=int, default=1, help="receiver ID of the second receiver")),
    (("--method",), dict(choices=("nearest", "linpol"), default="linpol", help="beacon SOA: nearest row, or interpolated")),
    (("-r", "--rx-coordinates"), dict(dest="rx_pos", default=None, help="config file with the receivers' coordinates")),
    (("-b", "--beacon-coordinates"), dict(dest="beacon_pos", default=None, help="config file with the beacons' coordinates")),
    (("-s", "--sample-rate"), dict(dest="sample_rate", type=float, default=2.4e6, help="sample rate, Hz")),
    (("--block-size",), dict(dest="block_size", type=int, default=16384, help="block length the carrier bins refer to")),
    (("--carrier-hz",), dict(dest="carrier_hz", type=float, default=433e6, help="carrier frequency, Hz")),
    (("--frac",), dict(type=float, default=0.025, help="share of a series in one smoothing window (0: no smoothing)")),
    (("--all",), dict(action="store_true", help="every (mobile, beacon, rx0, rx1) cell instead of one")),
    (("-o", "--output"), dict(default=None, help="save every array (.npz)")),
)


def _parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for flags, options in _CLI:
        parser.add_argument(*flags, **options)
    return parser


def _main(argv=None):
    args = _parser().parse_args(argv)
    detections = toads_data.toads_array(toads_data.load_toads(args.toads), with_ids=True)
    matches = matchmaker.load_matches(args.matches)
    only = {} if args.all else {"mobiles": [args.tx], "receivers": sorted((args.rx0, args.rx1))}
    positions = {name: tdoa_est.load_pos_config(path) if path else None
                 for name, path in (("rx_pos", args.rx_pos), ("beacon_pos", args.beacon_pos))}
    try:
        result = rel_dist(detections, matches, args.beacon, method=args.method, sample_rate=args.sample_rate,
                          block_len=args.block_size, carrier_hz=args.carrier_hz, smooth_frac=args.frac, **positions, **only)
    except ValueError as err:
        sys.stderr.write("%s\n" % err)
        return 1
    for c, key in enumerate(result.cells):
        if args.all:
            sys.stdout.write("# Mobile {} relative to beacon {} at RX {} and RX {}\n".format(*key))
        sys.stdout.write(format_report(result, c))
    if args.output:
        result.save(args.output)
    return 0


if __name__ == "__main__":
    sys.exit(_main())
