#!/usr/bin/env python3
"""Golden fixtures for the whole post-detect chain, made by RUNNING THE REFERENCE's
thrifty/kitchen_sink.py (`postdetect`: identify.integrate -> matchmaker.match_toads ->
tdoa_est.estimate_tdoas -> pos_est.solve) on the synthetic scene of tests/postdetect_scene.py.  Needs a
checkout of the reference and SciPy; THRIFTY_REFERENCE names the checkout:

    THRIFTY_REFERENCE=<checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_postdetect.py

The reference's modules are Python 2.  They are imported as they are, with what the generators of the
single stages put in their way (make_golden_identify.py, make_golden_tdoa.py, make_golden_pos.py): the
dictionaries handed in provide `iteritems`, `identify.defaultdict` and `tdoa_est.collections` provide it
too, `tdoa_est.list.sort` takes `cmp`, `pos_est.zip` returns a list, the matcher's matches are made lists,
and the `rx_pos` the position estimator sees has list-returning `keys()` / `values()`.

The scene (about 560 detections): 4 receivers on a ring of 1 km, 2 beacons, 3 mobiles inside it, a clock
of degree 2 plus noise per receiver, neighbouring-block duplicates, detections whose bin is outside the
map, transmissions one receiver saw, collisions, mobile transmissions before the first beacon and mobiles
only two receivers saw.  Three fixtures under tests/golden/postdetect/: `map` (frequency map), `auto`
(automatic mode) and `line` (1-D, two receivers).

Stored per fixture: the inputs (the eight raw columns, the map as rows, rx / beacon tables, windows,
sample rate) and everything the reference returned -- kept_order, txid, the matches as CSR, per group
group_id / timestamp / tx / group_ptr, rows rx0 / rx1 / det0 / det1 / tdoa / snr / model_quality, and per
solved group pos_group_id / pos / dop / pos_snr -- next to `tdoa_np` (tests/tdoa_ref.py on the reference's
toads and matches) and `pos_np` / `dop_np` (tests/pos_ref.py on tdoa_np's rows), with
d_tdoa = max |tdoa_ref - tdoa_np|, d_pos = max |pos_ref - pos_np|, d_dop = max |dop_ref - dop_np|,
d_snr and d_quality (relative).  The device is held to the reference within twice these distances
(tests/test_gpu_postdetect.py): once for the reference's own distance from the NumPy statements, once for
the device's.  Asserted here, while generating: every category above occurs, at least 20 positions, no
group left out, d_tdoa >= 1e-12 s and d_pos >= 1e-5 m (the device-to-NumPy distances on record, 3e-15 s
and <= 1e-6 m, must be small next to the bound)."""
import collections
import functools
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ["THRIFTY_REFERENCE"])
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from thrifty import identify, kitchen_sink, matchmaker, pos_est, tdoa_est, toads_data  # noqa: E402

import pos_ref  # noqa: E402
import postdetect_scene as scene  # noqa: E402
from tdoa_ref import tdoa_ref  # noqa: E402

OUT = os.path.join(HERE, "postdetect")


class Dict2(dict):
    iteritems = dict.items


class DefaultDict2(collections.defaultdict):
    iteritems = collections.defaultdict.items


class ListDict(dict):
    def keys(self):
        return list(dict.keys(self))

    def values(self):
        return list(dict.values(self))


class _List(list):
    def sort(self, cmp=None, **kwargs):
        if cmp is not None:
            kwargs["key"] = functools.cmp_to_key(cmp)
        list.sort(self, **kwargs)


identify.defaultdict = DefaultDict2
tdoa_est.collections = types.SimpleNamespace(defaultdict=DefaultDict2, OrderedDict=collections.OrderedDict,
                                             namedtuple=collections.namedtuple)
tdoa_est.list = _List
tdoa_est.basestring = str
pos_est.zip = lambda *args: list(zip(*args))


def reference(cols, st):
    dets = [toads_data.DetectionResult(float(cols["timestamp"][i]), int(cols["block"][i]), float(cols["soa"][i]),
                                       toads_data.CarrierSyncInfo(int(cols["carrier_bin"][i]), float(cols["carrier_offset"][i]), 9.0, 1.0),
                                       toads_data.CorrDetectionInfo(100, 0.25, float(cols["energy"][i]), float(cols["noise"][i])),
                                       rxid=int(cols["rxid"][i]))
            for i in range(len(cols["rxid"]))]
    where = {id(d): i for i, d in enumerate(dets)}
    freqmap = None if st.tx_freqs is None else Dict2((rx, Dict2(ranges)) for rx, ranges in st.tx_freqs.items())
    settings = kitchen_sink.PostdetectSettings(tx_freqs=freqmap, match_window=st.match_window, tdoa_est_window=st.tdoa_est_window,
                                               rx_pos=Dict2(st.rx_pos), beacon_pos=Dict2(st.beacon_pos),
                                               sample_rate=st.sample_rate)

    def matcher(toads, window):      # (a match is `dict.values()` there: a list under Python 2)
        matches, misses, collisions = matchmaker.match_toads(toads, window)
        return [list(m) for m in matches], misses, collisions

    result = kitchen_sink.postdetect(dets, settings, matcher=matcher,
                                     pos_estimator=lambda tdoas, rx_pos: pos_est.solve(tdoas, ListDict(rx_pos)))
    return dets, [where[id(d)] for d in result.toads], result


def fixture(name, cols, st):
    dets, kept_order, result = reference(cols, st)
    toads, matches, groups, positions = result.toads, [list(m) for m in result.matches], result.tdoas, result.pos
    dims = len(next(iter(st.rx_pos.values())))
    txid = np.array([-1 if d.txid is None else d.txid for d in dets], dtype=np.int32)
    t = {"rxid": [d.rxid for d in toads], "txid": [d.txid for d in toads], "timestamp": [d.timestamp for d in toads],
         "soa": [d.soa for d in toads], "energy": [d.corr_info.energy for d in toads], "noise": [d.corr_info.noise for d in toads]}
    rx_pos = {rx: np.asarray(p, dtype=float) for rx, p in st.rx_pos.items()}
    beacon_pos = {tx: np.asarray(p, dtype=float) for tx, p in st.beacon_pos.items()}
    mine = tdoa_ref(t["rxid"], t["txid"], t["timestamp"], t["soa"], t["energy"], t["noise"], matches, st.tdoa_est_window,
                    beacon_pos, rx_pos, st.sample_rate, 2)
    # ---- the TDOA stage: the same groups and rows, the values side by side
    assert [g.group_id for g in groups] == [g[0] for g in mine["groups"]], "groups differ from tdoa_ref's"
    rows_ref = [row for g in groups for row in g.tdoas]
    rows_np = [row for g in mine["groups"] for row in g[3]]
    assert [(int(r["rx0"]), int(r["rx1"]), int(r["det0_idx"]), int(r["det1_idx"])) for r in rows_ref] == \
        [(r[0], r[1], r[5], r[6]) for r in rows_np], "rows differ from tdoa_ref's"
    column = lambda k: np.array([r[k] for r in rows_np], dtype=np.float64)  # noqa: E731
    ref_col = lambda field: np.array([float(r[field]) for r in rows_ref], dtype=np.float64)  # noqa: E731
    tdoa_np, snr_np, quality_np = column(2), column(3), column(4)
    group_ptr = np.cumsum([0] + [len(g.tdoas) for g in groups]).astype(np.int64)
    # ---- the position stage on tdoa_np's rows
    ids = list(rx_pos)
    table = np.array([np.atleast_1d(rx_pos[rx]) for rx in ids], dtype=np.float64)
    dense = {rx: k for k, rx in enumerate(ids)}
    rx0 = np.array([dense[r[0]] for r in rows_np], dtype=np.int64)
    rx1 = np.array([dense[r[1]] for r in rows_np], dtype=np.int64)
    if dims == 1:
        each = [pos_ref.pos_ref_1d(rx0[r:r + 1], rx1[r:r + 1], tdoa_np[r:r + 1], snr_np[r:r + 1], table) for r in range(len(rx0))]
        assert np.array_equal(np.diff(group_ptr), np.ones(len(groups)))
        solved = {"pos": np.array([e[0] for e in each]), "dop": np.array([e[1] for e in each]), "status": np.array([e[3] for e in each])}
    else:
        solved = pos_ref.pos_ref_groups(group_ptr, rx0, rx1, tdoa_np, snr_np, table)
    keep = np.isin(np.asarray(solved["status"]), (0, 2, 3))         # OK, UNCONVERGED, AT_BOUND: the reference keeps those
    gid = np.array([g.group_id for g in groups], dtype=np.int64)
    assert positions["group_id"].tolist() == gid[keep].tolist(), "a group is left out by one side only"
    pos_np, dop_np = np.asarray(solved["pos"], dtype=np.float64).reshape(len(gid), dims)[keep], np.asarray(solved["dop"])[keep]
    pos_refd = np.stack([positions[axis] for axis in ("x", "y")[:dims]], axis=1)
    d = {"d_tdoa": float(np.abs(ref_col("tdoa") - tdoa_np).max()), "d_pos": float(np.abs(pos_refd - pos_np).max()),
         "d_dop": float(np.abs(positions["dop"] - dop_np).max()),
         "d_snr": float(np.abs(ref_col("snr") / snr_np - 1).max()),
         "d_quality": float(np.abs(ref_col("model_quality") / quality_np - 1).max())}
    # ---- the scene's categories
    n_under = len(gid) - int(keep.sum())
    lens = [len(m) for m in matches]
    first_beacon = min(i for i, m in enumerate(matches) if toads[m[0]].txid in beacon_pos)
    _, misses, collisions = matchmaker.match_toads(toads, st.match_window)
    assert len(kept_order) < len(dets), "no duplicate"
    assert st.tx_freqs is None or (txid == -1).any(), "no detection outside the map"
    assert misses and collisions, "no miss or no collision"
    assert first_beacon > 0, "no mobile transmission before the first beacon"
    assert len(positions) >= 20, "fewer than 20 positions"
    if dims == 2:
        assert n_under > 0 and 2 in lens, "no mobile that only two receivers saw"
    assert d["d_tdoa"] >= 1e-12 and (dims == 1 or d["d_pos"] >= 1e-5), d
    fm = np.zeros((0, 4)) if st.tx_freqs is None else np.array(
        [(rx, tx, lo, hi) for rx, ranges in st.tx_freqs.items() for tx, (lo, hi) in ranges.items()], dtype=np.float64)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(
        os.path.join(OUT, name + ".npz"), freqmap=fm, match_window=st.match_window, tdoa_window=st.tdoa_est_window,
        sample_rate=st.sample_rate, rx_ids=np.array(ids, dtype=np.int64), rx_xyz=table,
        beacon_ids=np.array(list(beacon_pos), dtype=np.int64), beacon_xyz=np.array([np.atleast_1d(beacon_pos[b]) for b in beacon_pos]),
        txid=txid, kept_order=np.array(kept_order, dtype=np.int64),
        match_ptr=np.cumsum([0] + lens).astype(np.int64), match_idx=np.array([i for m in matches for i in m], dtype=np.int64),
        misses=np.array(misses, dtype=np.int64), collisions=np.array(collisions, dtype=np.int64).reshape(-1, 2),
        group_id=gid, group_timestamp=np.array([g.timestamp for g in groups]), group_tx=np.array([g.tx for g in groups], dtype=np.int64),
        group_ptr=group_ptr, rx0=ref_col("rx0").astype(np.int64), rx1=ref_col("rx1").astype(np.int64),
        det0=ref_col("det0_idx").astype(np.int64), det1=ref_col("det1_idx").astype(np.int64), tdoa=ref_col("tdoa"),
        snr=ref_col("snr"), model_quality=ref_col("model_quality"), tdoa_np=tdoa_np,
        pos_group_id=np.asarray(positions["group_id"], dtype=np.int64), pos=pos_refd, dop=np.asarray(positions["dop"], dtype=np.float64),
        pos_snr=np.asarray(positions["snr"], dtype=np.float64), pos_np=pos_np, dop_np=dop_np,
        **dict({name_: np.float64(v) for name_, v in d.items()}, **{"col_" + c: cols[c] for c in scene.COLUMNS}))
    print(name, "n", len(dets), "kept", len(kept_order), "matches", len(matches), "misses", len(misses), "collisions", len(collisions),
          "groups", len(gid), "positions", len(positions), "underdetermined", n_under, d)


if __name__ == "__main__":
    fixture("map", scene.columns(140), scene.settings())
    fixture("auto", scene.columns(140, seed=6), scene.settings(automatic=True))
    fixture("line", scene.columns(140, seed=7, rx_ids=(0, 1), line=True), scene.settings(rx_ids=(0, 1), line=True))
