#!/usr/bin/env python
"""
Estimate TDOA values of mobile unit transmissions from SOA values.

GPU counterpart of reference thrifty/tdoa_est.py: beacon transmissions synchronise the SoA values of
different receivers, and the TDOA of every pair of detections of a mobile transmission is read off a
model of the two receivers' clocks built from the beacon detections around it -- a fitted polynomial
(the default), a weighted one, the nearest beacon transmission, or the line through two of one beacon.
The pair lists, the windows, the outlier mask, the model and the output orders run on the device
(`thr_tdoa_model`, csrc/tdoa.hip); this module keeps the reference's names and the `.tdoa` text format.

The four models are chosen the way the reference's callers choose them, `estimate_tdoas(...,
model_builder=build_model_nearest)`, but `build_model_*` here are SELECTORS of a device model, not
functions: a host callable cannot run inside the device call.  `nearest` and `linear` reproduce the
reference's float64 operations in its order, so their TDOAs are its bits; they need one and two kept
beacon pairs in the window where the polynomial needs `deg + 1`.

What is reproduced, quirks included: the per-receiver-pair beacon lists stay in match order (the
reference's `sort(cmp=...)` never reorders), the window is Python's bisection on that list whether it
is sorted or not, and the outlier mask is numpy's float64 arithmetic operation for operation.  The fit
itself is NOT LAPACK's: it is a least-squares polynomial in a centred and scaled variable, which is
closer to the exact least-squares answer than the reference's raw Vandermonde.

Deviations from the reference:

* a receiver pair that no beacon match covers is an empty window, so the pair is a failure (the
  reference dies with KeyError);
* kept abscissae with fewer than `deg + 1` distinct values are a failure (the reference returns
  LAPACK's minimum-norm solution with a RankWarning);
* `linear`: two chosen beacon pairs with the same det0 SoA are a failure (the reference dies with
  ZeroDivisionError); `weighted_poly`: a kept beacon pair whose det0 SoA equals the mobile det0's is a
  failure (the reference's weights turn inf / NaN and it appends a NaN row);
* a match with two detections of one receiver raises ValueError before anything is launched (the
  reference hits `assert rxid0 < rxid1`); so does an empty match.  A receiver of any match that
  `rx_pos` lacks raises KeyError up front (the reference raises it when it first needs the position).

A match is taken to hold detections of ONE transmitter, as `matchmaker` makes them: whether it is a
beacon match, and which beacon, is read off its first detection.  The reference reads the beacon of
every pair off that pair's det0, so a hand-made match that mixes txids would differ.

Windows of up to 256 beacon pairs are ranked from on-chip memory; longer ones are correct but slow (the
rank count is quadratic in the window and then recomputes its operands).

`.tdoa` text: one line per TDOA, `group_id timestamp(%.06f) tx rx0 rx1 tdoa[ns] snr model_quality
det0_idx det1_idx`, floats as their shortest round-trip repr -- what the reference's `print(*record)`
emits under Python 3 with current numpy; under Python 2 it printed 12 significant digits.  The loaders
read either form.
"""
from __future__ import print_function

import argparse
import collections
import sys

import numpy as np

from thrifty_amd import _native, matchmaker, toads_data
from thrifty_amd.settings import parse_kvconfig

SPEED_OF_LIGHT = 2.997e8
MAX_TDOA = 30e3 / SPEED_OF_LIGHT

TdoaInfo = collections.namedtuple("TdoaInfo", ["rx0", "rx1", "tdoa", "snr", "model_quality", "det0_idx", "det1_idx"])
TdoaGroup = collections.namedtuple("TdoaGroup", ["group_id", "timestamp", "tx", "tdoas"])

TDOA_DTYPE = {"names": ("rx0", "rx1", "tdoa", "snr", "model_quality", "det0_idx", "det1_idx"),
              "formats": ("i4", "i4", "f8", "f8", "f8", "i4", "i4")}
MATRIX_DTYPE = {"names": ("group_id", "timestamp", "tx") + TDOA_DTYPE["names"],
                "formats": ("i4", "f8", "i4") + TDOA_DTYPE["formats"]}


class DeviceModel(object):
    """Selects one of the TDOA models of `thr_tdoa_model`; stands where the reference has a model builder."""

    def __init__(self, name, code, takes_deg):
        self.name, self.code, self.takes_deg = name, code, takes_deg

    def __call__(self, *args, **kwargs):
        raise NotImplementedError(
            "'%s' runs inside the device call thr_tdoa_model; pass it as estimate_tdoas(..., model_builder=...) "
            "or tdoa_columns(..., model=...) instead of calling it" % self.name)

    def __repr__(self):
        return "<device tdoa model %r>" % self.name


build_model_poly = DeviceModel("poly", _native.TDOA_MODELS["poly"], True)
build_model_weighted_poly = DeviceModel("weighted_poly", _native.TDOA_MODELS["weighted_poly"], True)
build_model_nearest = DeviceModel("nearest", _native.TDOA_MODELS["nearest"], False)
build_model_linear = DeviceModel("linear", _native.TDOA_MODELS["linear"], False)
default_model = build_model_poly
MODELS = {sel.name: sel for sel in (build_model_poly, build_model_weighted_poly, build_model_nearest,
                                    build_model_linear)}


def _model(model):
    """A selector, or one of the names of MODELS -> the selector."""
    if isinstance(model, DeviceModel):
        return model
    if isinstance(model, str) and model in MODELS:
        return MODELS[model]
    raise TypeError("the TDOA model must be one of tdoa_est.build_model_poly, build_model_weighted_poly, "
                    "build_model_nearest, build_model_linear (or their names %s), not %r: host callables cannot "
                    "run inside the device call" % (", ".join(sorted(MODELS)), model))


def _columns(detections):
    n = len(detections)
    cols = {"rxid": np.empty(n, np.int32), "txid": np.empty(n, np.int32)}
    cols.update((name, np.empty(n, np.float64)) for name in ("timestamp", "soa", "energy", "noise"))
    for i, d in enumerate(detections):
        cols["rxid"][i] = -1 if d.rxid is None else d.rxid
        cols["txid"][i] = -1 if d.txid is None else d.txid
        cols["timestamp"][i] = d.timestamp
        cols["soa"][i] = d.soa
        cols["energy"][i] = d.corr_info.energy
        cols["noise"][i] = d.corr_info.noise
    return cols


def _distance(a, b):
    delta = np.asarray(a, dtype=float) - np.asarray(b, dtype=float)
    return np.sqrt(np.sum(delta ** 2))


def tdoa_columns(cols, match_ptr, match_idx, window_size, beacon_pos, rx_pos, sample_rate, deg=2, device_id=0,
                 model="poly"):
    """TDOAs for detection columns (rxid, txid, timestamp, soa, energy, noise) and matches in CSR form
    (match m is match_idx[match_ptr[m]:match_ptr[m + 1]]) -> dict: `tdoas` (all rows, TDOA_DTYPE, in
    order), `group_id` / `group_ptr` / `timestamp` / `tx` per group (group g holds rows
    group_ptr[g]:group_ptr[g + 1]), `failures` int64[f, 2], and per detection pair of the mobile
    matches, in order, `n_window` (beacon pairs in its window), `n_kept` (those the outlier mask kept) and
    `picks` int32[n, 2]: what `model` chose, as positions among the kept pairs -- (idx, -1) for `nearest`,
    (low, high) for `linear` (low == -1: no earlier pair of the same beacon), (-1, -1) otherwise.
    `model`: a selector (build_model_*) or its name; `deg` is read by the two polynomials only."""
    model = _model(model)
    ptr, idx = np.asarray(match_ptr, dtype=np.int64), np.asarray(match_idx, dtype=np.int64)
    rxid, txid = np.asarray(cols["rxid"]), np.asarray(cols["txid"])
    if len(ptr) < 1 or ptr[0] != 0 or ptr[-1] != len(idx) or np.any(np.diff(ptr) < 1):
        raise ValueError("matches: every match needs at least one detection")
    if len(idx) and (idx.min() < 0 or idx.max() >= len(rxid)):
        raise ValueError("matches: detection index out of range")
    receivers = np.unique(rxid[idx])
    for rx in receivers.tolist():
        if rx not in rx_pos:
            raise KeyError(rx)
    beacons = sorted(beacon_pos)
    first_tx = txid[idx[ptr[:-1]]]
    match_beacon = np.full(len(ptr) - 1, -1, dtype=np.int32)
    for b, beacon in enumerate(beacons):
        match_beacon[first_tx == beacon] = b
    dist = np.array([[_distance(rx_pos[rx], beacon_pos[beacon]) for beacon in beacons] for rx in receivers.tolist()],
                    dtype=np.float64).reshape(len(receivers), len(beacons))
    dense = np.clip(np.searchsorted(receivers, rxid), 0, max(len(receivers) - 1, 0)).astype(np.int32)
    out = _native.tdoa(dense, cols["timestamp"], cols["soa"], cols["energy"], cols["noise"], ptr, idx, match_beacon,
                       dist if len(receivers) else np.zeros((1, len(beacons))), window_size, sample_rate, deg, device_id,
                       model.code)
    rows = np.zeros(len(out["tdoa"]), dtype=TDOA_DTYPE)
    if len(rows):
        rows["rx0"], rows["rx1"] = receivers[out["row_rx"][:, 0]], receivers[out["row_rx"][:, 1]]
        rows["det0_idx"], rows["det1_idx"] = out["row_det"][:, 0], out["row_det"][:, 1]
    for name in ("tdoa", "snr", "model_quality"):
        rows[name] = out[name]
    gid = out["group_id"]
    # the reference's `tx` is the txid of det0 of the match's last combination
    last_a, last_b = idx[ptr[gid + 1] - 2], idx[ptr[gid + 1] - 1]
    return {"tdoas": rows, "group_id": gid, "group_ptr": out["group_ptr"],
            "timestamp": np.asarray(cols["timestamp"], dtype=np.float64)[idx[ptr[gid]]],
            "tx": txid[np.where(rxid[last_a] <= rxid[last_b], last_a, last_b)],
            "failures": out["failures"], "n_window": out["n_window"], "n_kept": out["n_kept"], "picks": out["picks"]}


def _groups(res):
    ptr = res["group_ptr"].tolist()
    return [TdoaGroup(group_id=int(g), timestamp=float(t), tx=int(tx), tdoas=res["tdoas"][a:b])
            for g, t, tx, a, b in zip(res["group_id"].tolist(), res["timestamp"].tolist(), res["tx"].tolist(),
                                      ptr[:-1], ptr[1:])]


def _model_and_degree(model_builder, model_params, deg):
    """estimate_tdoas' model arguments -> (selector, degree); TypeError for what the reference's
    `model_builder(..., **model_params)` would refuse, and for a builder that is not a selector."""
    model = _model(default_model if model_builder is None else model_builder)
    params = dict(model_params or {})
    if model.takes_deg:
        deg = params.pop("deg", deg)
    if params:
        raise TypeError("build_model_%s() got an unexpected keyword argument %r" % (model.name, sorted(params)[0]))
    return model, deg


def estimate_tdoas(detections, matches, window_size, beacon_pos, rx_pos, sample_rate, deg=2, model_builder=None,
                   model_params=None):
    """(tdoa_groups, failures): one TdoaGroup per mobile match with at least one TDOA (`tdoas` is a
    TDOA_DTYPE array in combination order) and the (det0_idx, det1_idx) pairs no TDOA could be
    estimated for, in the order they occurred.  `model_builder`: one of this module's build_model_*
    selectors (None: default_model); `model_params`: {"deg": d} for the two polynomials, overriding `deg`."""
    model, deg = _model_and_degree(model_builder, model_params, deg)
    ptr = np.cumsum([0] + [len(m) for m in matches]).astype(np.int64)
    idx = np.array([i for m in matches for i in m], dtype=np.int64)
    res = tdoa_columns(_columns(detections), ptr, idx, window_size, beacon_pos, rx_pos, sample_rate, deg, model=model)
    return _groups(res), [tuple(pair) for pair in res["failures"].tolist()]


def save_tdoa_groups(output, tdoa_groups):
    """One line per TDOA (see the module docstring); `output` is a file name or an open text file."""
    if isinstance(output, str):
        with open(output, "w") as handle:
            return save_tdoa_groups(handle, tdoa_groups)
    for group in tdoa_groups:
        for row in group.tdoas:
            print(group.group_id, "%.06f" % group.timestamp, group.tx, row["rx0"], row["rx1"],
                  repr(float(row["tdoa"] * 1e9)), repr(float(row["snr"])), repr(float(row["model_quality"])),
                  row["det0_idx"], row["det1_idx"], file=output)


def load_tdoa_matrix(fname):
    """All rows of a .tdoa file as a MATRIX_DTYPE array, `tdoa` back in seconds."""
    if isinstance(fname, str):
        with open(fname, "r") as handle:
            return load_tdoa_matrix(handle)
    lines = [line.decode() if isinstance(line, bytes) else line for line in fname]
    lines = [line for line in lines if line.strip() and not line.lstrip().startswith("#")]
    data = np.zeros(len(lines), dtype=MATRIX_DTYPE)
    for r, line in enumerate(lines):
        words = line.split()
        data[r] = tuple(float(w) if fmt == "f8" else int(w) for w, fmt in zip(words, MATRIX_DTYPE["formats"]))
    data["tdoa"] /= 1e9
    return data


def groups_to_matrix(groups):
    rows = [(group.group_id, group.timestamp, group.tx) + tuple(tdoa.tolist())
            for group in groups for tdoa in group.tdoas]
    return np.array(rows, dtype=MATRIX_DTYPE)


def load_tdoa_groups(fname):
    """The TdoaGroups of a .tdoa file, in the order their group_id first appears."""
    matrix = load_tdoa_matrix(fname)
    rows = np.zeros(len(matrix), dtype=TDOA_DTYPE)
    for name in TDOA_DTYPE["names"]:
        rows[name] = matrix[name]
    ids = matrix["group_id"]
    firsts = np.sort(np.unique(ids, return_index=True)[1])
    return [TdoaGroup(int(ids[f]), float(matrix["timestamp"][f]), int(matrix["tx"][f]), rows[ids == ids[f]])
            for f in firsts.tolist()]


def load_pos_config(file_):
    """`id: x y [z]` lines -> {id: array of coordinates}."""
    if isinstance(file_, str):
        with open(file_, "r") as handle:
            return load_pos_config(handle)
    return {int(id_): np.array([float(x) for x in pos.split()]) for id_, pos in parse_kvconfig(file_).items()}


_CLI = (
    (("toads",), dict(nargs="?", type=argparse.FileType("r"), default="data.toads",
                      help="toads data (\"-\" streams from stdin)")),
    (("matches",), dict(nargs="?", type=argparse.FileType("r"), default="data.match",
                        help="match data (\"-\" streams from stdin)")),
    (("-o", "--output"), dict(dest="output", type=argparse.FileType("w"), default="data.tdoa",
                              help="output file ('-' for stdout)")),
    (("-r", "--rx-coordinates"), dict(dest="rx_pos", type=argparse.FileType("r"), default="pos-rx.cfg",
                                      help="path to config file that contains the coordinates of the receivers")),
    (("-b", "--beacon-coordinates"), dict(dest="beacon_pos", type=argparse.FileType("r"), default="pos-beacon.cfg",
                                          help="path to config file that contains the coordinates of the beacon "
                                               "transmitters")),
    (("-w", "--window-size"), dict(dest="window_size", type=float, default=8,
                                   help="maximum difference in timestamp between a beacon transmission and a "
                                        "mobile unit transmission for the beacon transmission to be used for "
                                        "estimating the TDOA of the mobile unit transmission")),
    (("-s", "--sample-rate"), dict(dest="sample_rate", type=float, default=2.4e6,
                                   help="nominal sample rate of receivers")),
    (("--model",), dict(dest="model", choices=("poly", "weighted_poly", "nearest", "linear"), default="poly",
                        help="clock model built from the beacon transmissions in the window [default: poly]")),
    (("--deg",), dict(dest="deg", type=int, default=2, help="degree of the two polynomial models (1..3)")),
)


def _parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for flags, options in _CLI:
        parser.add_argument(*flags, **options)
    return parser


def _main(argv=None):
    args = _parser().parse_args(argv)
    try:
        toads = toads_data.load_toads(args.toads)
        matches = matchmaker.load_matches(args.matches)
        rx_pos = load_pos_config(args.rx_pos)
        beacon_pos = load_pos_config(args.beacon_pos)
        tdoa_groups, failures = estimate_tdoas(toads, matches, args.window_size, beacon_pos, rx_pos, args.sample_rate,
                                               deg=args.deg, model_builder=MODELS[args.model])
        print("Number of TDOA estimations:", len(tdoa_groups))
        print("Number of TDOA estimation failures:", len(failures))
        save_tdoa_groups(args.output, tdoa_groups)
    finally:
        for stream in (args.toads, args.matches, args.rx_pos, args.beacon_pos):
            if stream is not sys.stdin:
                stream.close()
        if args.output is sys.stdout:
            args.output.flush()
        else:
            args.output.close()


if __name__ == "__main__":
    _main()
