"""Are the clocks of two receivers in sync?  The numbers of the reference's `thrifty analyze_beacon`.

    python -m thrifty_amd.beacon_analysis [toads] [matches] [--beacon B --rx0 R --rx1 R] [--range A-B]
                                          [--deg D] [--all] [-o sync.npz]

For a beacon and a pair of receivers: the SOA difference of every match that holds both, the places where it
jumps (a receiver dropped samples), a polynomial of soa at rx1 on soa at rx0 through every stretch between two
jumps, and the residuals in metres.  The reference answers for one (beacon, rx0, rx1) per run; `sync_stats`
answers for every cell of a deployment in one device call (thr_beaconsync, csrc/syncstats.hip) and
`format_report` prints the reference's text for any of them.  No plots: the numbers behind the reference's two
figures are arrays of `BeaconSync` (and of the `-o` file).

Kept from the reference, quirks included: a row is a discontinuity when dsdoa > 10 * mean(dsdoa), which is
sign-sensitive (rx1 slower than rx0: the mean is negative, nearly every row is one); row 0 and every
discontinuity row belong to no cut; nine rows is the shortest cut that is fitted; `Cut #i: 0 outliers`.
Deviations, each with a test (tests/test_gpu_syncstats*.py):
 - the polynomial is fitted in u = (soa0 - mean) / max|soa0 - mean| (np.polyfit: the raw Vandermonde matrix of
   SOAs near 1e9); the raw-basis coefficients `analyze` returns are expanded from the centred ones in exact
   rational arithmetic and rounded once;
 - a cell without a fitted cut is reported as such and `analyze` raises a ValueError that says so (the
   reference's np.concatenate of nothing raises an unrelated one);
 - the metres per sample of the report are 3e8 / sample_rate (the reference's 3e8 / 2.4e6).
"""
from __future__ import annotations

import argparse
import sys
from fractions import Fraction

import numpy as np

from thrifty_amd import _native, matchmaker, toads_data

FITTED = _native.BSYNC_CUT_FITTED
NO_FIT_TEXT = "No cut of more than 8 rows: nothing fitted"


def _expand(centred, mean):
    """sum c_k (x - mean)^k in powers of x (lowest first), Fractions in and out."""
    total, power = [Fraction(0)] * len(centred), [Fraction(1)]
    for c in centred:
        for i, p in enumerate(power):
            total[i] += c * p
        power = [(power[i - 1] if i else 0) - (power[i] if i < len(power) else 0) * mean for i in range(len(power) + 1)]
    return total


def raw_coefficients(fit, deg):
    """float64[deg + 1], highest power first: y_mean + sum c_k ((x - x_mean) / x_scale)^k expanded in powers of x
    in rational arithmetic, each coefficient rounded once.  `fit` is a row of BeaconSync.cut_fit."""
    x_mean, x_scale, y_mean = (Fraction(float(v)) for v in fit[:3])
    total = _expand([Fraction(float(fit[3 + k])) / x_scale ** k for k in range(deg + 1)], x_mean)
    total[0] += y_mean
    return np.array([float(v) for v in reversed(total)])


class BeaconSync(object):
    """The arrays of one thr_beaconsync call, one attribute per output (cell_key, cell_ptr, row_det, row_match,
    sdoa, disc_ptr, disc_idx, cut_ptr, cut_left, cut_right, cut_flags, cut_fit, cut_snr, cut_disc_soa, residual,
    cell_counts, cell_stats, cell_flags), plus `det_id` (the detections' ids), `deg`, `sample_rate`, `counts`."""

    def __init__(self, counts, arrays, det_id, deg, sample_rate):
        self.counts = dict(counts)
        self.names = tuple(arrays)
        for name, value in arrays.items():
            setattr(self, name, value)
        self.det_id, self.deg, self.sample_rate = np.asarray(det_id), int(deg), float(sample_rate)

    def __len__(self):
        return len(self.cell_key)

    def index(self, beacon, rx0, rx1):
        hit = np.flatnonzero(np.all(self.cell_key == (beacon, rx0, rx1), axis=1))
        if len(hit) == 0:
            raise KeyError("no match of beacon %r holds receivers %r and %r" % (beacon, rx0, rx1))
        return int(hit[0])

    def cell(self, beacon, rx0, rx1):
        """Everything about one cell as a dict; `cuts` lists the fitted cuts with the reference's number, the
        raw-basis coefficients (highest power first) and the cut's residuals."""
        c = self.index(beacon, rx0, rx1)
        a, b = self.cell_ptr[c], self.cell_ptr[c + 1]
        out = {"beacon": int(beacon), "rx0": int(rx0), "rx1": int(rx1), "rows": self.row_det[a:b],
               "matches": self.row_match[a:b], "sdoa": self.sdoa[a:b], "residual": self.residual[a:b],
               "discontinuities": self.disc_idx[self.disc_ptr[c]:self.disc_ptr[c + 1]],
               "flags": int(self.cell_flags[c]), "cuts": []}
        out.update(zip(("mean_dsdoa", "std", "max", "snr"), self.cell_stats[c].tolist()))
        for g in range(self.cut_ptr[c], self.cut_ptr[c + 1]):
            if self.cut_flags[g] == FITTED:
                left, right = int(self.cut_left[g]), int(self.cut_right[g])
                out["cuts"].append({"number": int(g - self.cut_ptr[c]) + 1, "left": left, "right": right,
                                    "coef": raw_coefficients(self.cut_fit[g], self.deg), "fit": self.cut_fit[g],
                                    "snr": float(self.cut_snr[g]), "disc_soa": float(self.cut_disc_soa[g]),
                                    "residual": self.residual[a + left:a + right]})
        return out

    def coefficients(self, c):
        """Raw-basis coefficient arrays of cell number `c`, one per fitted cut."""
        cuts = range(self.cut_ptr[c], self.cut_ptr[c + 1])
        return [raw_coefficients(self.cut_fit[g], self.deg) for g in cuts if self.cut_flags[g] == FITTED]

    def format_report(self, c):
        return format_report(self, c)

    def save(self, path):
        np.savez(path, det_id=self.det_id, deg=self.deg, sample_rate=self.sample_rate,
                 **{name: getattr(self, name) for name in self.names})


def _as_columns(detections):
    """The six columns from a dict of columns, a toads_array, or a sequence of DetectionResult."""
    if isinstance(detections, dict):
        return detections
    if not isinstance(detections, np.ndarray):
        detections = toads_data.toads_array(list(detections), with_ids=True)
    return {name: detections[name] for name, _ in _native.BSYNC_COLUMNS}


def _as_csr(matches):
    """(match_ptr, match_idx) from a list of index lists, or from the CSR pair itself -- a tuple of two ndarrays
    with match_ptr[0] == 0 and match_ptr[-1] == len(match_idx); two match LISTS in a tuple are matches."""
    if (isinstance(matches, tuple) and len(matches) == 2 and all(isinstance(part, np.ndarray) and part.ndim == 1 for part in matches)
            and len(matches[0]) and matches[0][0] == 0 and matches[0][-1] == len(matches[1])):
        return matches
    ptr = np.cumsum([0] + [len(m) for m in matches]).astype(np.int64)
    return ptr, np.array([i for m in matches for i in m], dtype=np.int64)


def sync_stats(detections, matches, beacons=None, receivers=None, deg=2, id_range=None, sample_rate=2.4e6, device_id=0):
    """Clock-sync numbers of every (beacon, rx0 < rx1) cell.  `detections`: DetectionResult objects, a
    toads_array, or a dict of the columns rxid, txid, soa, energy, noise, idx; `matches`: lists of detection
    indices, or (match_ptr, match_idx); `beacons` / `receivers`: ids to restrict to; `id_range`: (first, last)
    detection id, both ends included.  ValueError for what thr_beaconsync refuses (an empty selection, a match
    with two detections of one receiver, deg outside 1..3)."""
    cols = _as_columns(detections)
    ptr, idx = _as_csr(matches)
    counts, arrays = _native.beaconsync(cols, ptr, idx, deg, id_range, beacons, receivers, device_id=device_id)
    return BeaconSync(counts, arrays, cols["idx"], deg, sample_rate)


def format_report(sync, c):
    """The reference's text for cell number `c`."""
    a = sync.cell_ptr[c]
    disc = sync.disc_idx[sync.disc_ptr[c]:sync.disc_ptr[c + 1]]
    ids = sync.det_id[sync.row_det[a + disc]].reshape(-1, 2)
    lines = ["Number of detection groups: {}".format(int(sync.cell_counts[c, 0])),
             "Number of discontinuities: {}".format(len(disc)),
             "Discontinuities (index): " + " ".join(str(d) for d in disc),
             "Discontinuities (toad id): " + " ".join(str(pair) for pair in ids)]
    for g in range(sync.cut_ptr[c], sync.cut_ptr[c + 1]):
        if sync.cut_flags[g] == FITTED:
            lines.append("Cut #{}: 0 outliers".format(g - sync.cut_ptr[c] + 1))
    if sync.cell_flags[c] & _native.BSYNC_CELL_NO_FIT:
        lines.append(NO_FIT_TEXT)
    else:
        s2m = 3e8 / sync.sample_rate
        _, std, biggest, snr = sync.cell_stats[c]
        lines.append("residuals: std dev = {:.01f} m; max = {:.01f} m; avg corr snr = {:.01f}".format(
            std * s2m, biggest * s2m, 10 * np.log10(snr)))
    return "\n".join(lines) + "\n"


def analyze(detections, matches, deg=2, sample_rate=2.4e6):
    """The reference's arguments: `detections` a detection array, `matches` a [k][2] matrix of indices into it
    (the beacon's matches at two receivers).  Prints the report, returns one coefficient array per fitted cut."""
    matches = np.asarray(matches, dtype=np.int64).reshape(-1, 2)
    flat = matches.reshape(-1)
    cols = {name: np.asarray(detections[name])[flat] for name in ("soa", "energy", "noise", "idx")}
    cols["rxid"] = np.tile(np.array([0, 1], np.int32), len(matches))
    cols["txid"] = np.zeros(len(flat), np.int32)
    ptr = 2 * np.arange(len(matches) + 1, dtype=np.int64)
    sync = sync_stats(cols, (ptr, np.arange(len(flat), dtype=np.int64)), deg=deg, sample_rate=sample_rate)
    sys.stdout.write(format_report(sync, 0))
    if sync.cell_flags[0] & _native.BSYNC_CELL_NO_FIT:
        raise ValueError("no stretch between two discontinuities has more than 8 rows: nothing can be fitted")
    return sync.coefficients(0)


def fit_poly_model(soa, deg=2):
    """(coef, residuals) of the least-squares polynomial of soa[:, 1] on soa[:, 0] for ONE cut, coefficients
    highest power first.  A host helper in rational arithmetic on the float64 inputs (normal equations solved
    exactly, every number rounded once): the device path is `sync_stats`, which fits all cuts of all cells."""
    soa = np.asarray(soa, dtype=np.float64).reshape(-1, 2)
    x, y = [Fraction(float(v)) for v in soa[:, 0]], [Fraction(float(v)) for v in soa[:, 1]]
    if len(set(x)) <= deg:
        raise ValueError("fit_poly_model: degree %d needs more than %d distinct soa" % (deg, deg))
    mean = sum(x) / len(x)
    u = [v - mean for v in x]
    rows = [[sum(a ** (i + j) for a in u) for j in range(deg + 1)] + [sum(a ** i * b for a, b in zip(u, y))]
            for i in range(deg + 1)]
    for col in range(deg + 1):                  # Gauss-Jordan on exact numbers: any non-zero pivot will do
        piv = next(r for r in range(col, deg + 1) if rows[r][col] != 0)
        rows[col], rows[piv] = rows[piv], rows[col]
        rows[col] = [v / rows[col][col] for v in rows[col]]
        for r in range(deg + 1):
            if r != col:
                rows[r] = [v - rows[r][col] * w for v, w in zip(rows[r], rows[col])]
    centred = [rows[k][-1] for k in range(deg + 1)]
    residuals = np.array([float(b - sum(c * a ** k for k, c in enumerate(centred))) for a, b in zip(u, y)])
    return np.array([float(v) for v in reversed(_expand(centred, mean))]), residuals


def parse_range(text):
    """'A-B' -> (A, B), None -> None."""
    if text is None:
        return None
    first, last = (int(word) for word in text.split("-"))
    return first, last


_CLI = (
    (("toads",), dict(nargs="?", type=argparse.FileType("rb"), default="data.toads", help="toads data ('-' streams from stdin)")),
    (("matches",), dict(nargs="?", type=argparse.FileType("rb"), default="data.match", help="match data")),
    (("--beacon",), dict(type=int, default=0, help="transmitter ID of the beacon")),
    (("--rx0",), dict(type=int, default=0, help="receiver ID of the first receiver")),
    (("--rx1",), dict(type=int, default=1, help="receiver ID of the second receiver")),
    (("--range",), dict(type=parse_range, default=None, help="limit to a range of detection IDs, A-B")),
    (("--deg",), dict(type=int, default=2, help="degree of the polynomial through the SOAs")),
    (("--all",), dict(action="store_true", help="every (beacon, rx0, rx1) cell instead of one")),
    (("-o", "--output"), dict(default=None, help="save every array (.npz)")),
    (("--export",), dict(nargs="?", const=True, default=None, help="(the reference's plot export; not part of this port)")),
)


def _parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for flags, options in _CLI:
        parser.add_argument(*flags, **options)
    return parser


def _main(argv=None):
    args = _parser().parse_args(argv)
    if args.export:
        sys.stderr.write("plots are not part of this port\n")
        return 1
    detections = toads_data.toads_array(toads_data.load_toads(args.toads), with_ids=True)
    matches = matchmaker.load_matches(args.matches)
    only = {} if args.all else {"beacons": [args.beacon], "receivers": sorted((args.rx0, args.rx1))}
    try:
        sync = sync_stats(detections, matches, deg=args.deg, id_range=args.range, **only)
    except ValueError as err:
        sys.stderr.write("%s\n" % err)
        return 1
    for c in range(len(sync)):
        if args.all:
            sys.stdout.write("# Beacon {} at RX {} and RX {}\n".format(*sync.cell_key[c]))
        sys.stdout.write(format_report(sync, c))
    if args.output:
        sync.save(args.output)
    return 0


if __name__ == "__main__":
    sys.exit(_main())
