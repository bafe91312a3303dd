"""thr_tdoamatrix on synthetic inputs against the NumPy statement (tests/tdoa_matrix_ref.py), with the comparison rules
of tests/test_gpu_tdoa_matrix.py: structure, statuses, n_window, n_kept and the cell mask exact; the mask also against
is_outlier on the device's own TDOAs and the statistics against the exact statistics of its own kept rows
(tdoa_matrix_golden.check_own_mask_and_stats); snr relative 1e-14, model_quality relative 1e-12.  The TDOA bound is
tests/test_gpu_tdoa_seams.py's: both sides fit in the same centred, scaled variable, the device through the Gram
system (condition cond(V)^2) -- 16 * cond(V)^2 * 2^-52 * spread / sample_rate per task, cond and spread from the
statement.  The seams: task counts around the four tasks of a workgroup; a cell boundary on a tile boundary of the
segmented reductions and one row past it, with more tiles than workgroups; a beacon that is also a target; a target
absent at one receiver; the beacon list at its cap; zero cells; every argument error."""
import numpy as np
import pytest

import tdoa_matrix_golden as G
from tdoa_matrix_ref import tdoa_matrix_ref
from thrifty_amd import _native

pytestmark = pytest.mark.gpu

FS = 2.4e6
LIGHT = 2.997e8


def scene(seed, n_rx, times, heard=None, noise=0.05):
    """times: {tx: [t]}; heard: {tx: receivers} (all by default) -> (columns, match_ptr, match_idx), matches in time order."""
    rng = np.random.default_rng(seed)
    rx_pos = rng.uniform(-1500, 1500, (n_rx, 2))
    tx_pos = {tx: rng.uniform(-1200, 1200, 2) for tx in times}
    offset, rate = rng.uniform(1e3, 9e3, n_rx).round(), FS * (1 + rng.uniform(-30, 30, n_rx) * 1e-6)
    rows, ptr = [], [0]
    for t, tx in sorted((t, tx) for tx, ts in times.items() for t in ts):
        for r in (heard or {}).get(tx, range(n_rx)):
            delay = float(np.linalg.norm(rx_pos[r] - tx_pos[tx])) / LIGHT
            rows.append((r, tx, round(1.7e9 + t + delay, 6), offset[r] + (t + delay) * rate[r] + rng.normal(0, noise),
                         rng.uniform(50, 200), rng.uniform(1, 3)))
        ptr.append(len(rows))
    cols = {name: np.array([row[k] for row in rows], kind) for k, (name, kind) in enumerate(_native.TDMAT_COLUMNS)}
    return cols, np.array(ptr, np.int64), np.arange(len(rows), dtype=np.int64)


def run_and_check(cols, ptr, idx, what="", **kw):
    want_counts, want = tdoa_matrix_ref(cols, ptr, idx, **kw)
    native = dict(kw, model=_native.TDOA_MODELS[kw.get("model", "poly")])
    native.pop("rx_pos", None), native.pop("beacon_pos", None)
    counts, out = _native.tdoamatrix(cols, ptr, idx, **native)
    assert {k: counts[k] for k in want_counts} == want_counts, what
    G.check_structure(out, want, what)
    ok = want["status"] == G.OK
    assert np.all(np.isnan(out["tdoa"][~ok])) and np.all(np.isnan(out["model_quality"][~ok])), what
    bound = 16 * want["cond"][ok] ** 2 * 2.0 ** -52 * want["spread"][ok] / FS
    assert np.all(np.abs(out["tdoa"][ok] - want["tdoa"][ok]) <= bound), what
    np.testing.assert_allclose(out["snr"], want["snr"], rtol=1e-14, atol=0)
    np.testing.assert_allclose(out["model_quality"][ok], want["model_quality"][ok], rtol=1e-12, atol=0)
    G.check_own_mask_and_stats(out, what)
    extra = 2 * float(np.max(bound)) * LIGHT if ok.any() else 0.0
    for c in range(counts["cells"]):
        n = int(want["cell_counts"][c, 4])
        if n:
            mabs = abs(want["cell_stats"][c, 0]) + want["cell_stats"][c, 1]      # >= mean |x| of the kept rows
            assert abs(out["cell_stats"][c, 0] - want["cell_stats"][c, 0]) <= (n + 2) * G.U * mabs + extra, (what, c)
            G.assert_std_within(out["cell_stats"][c, 1], want["cell_stats"][c, 1], mabs, n, extra=extra, what=(what, c))
    return counts, out


def beacon_times(stop, period=0.5):
    return np.arange(0.0, stop, period).tolist()


@pytest.mark.parametrize("tasks", [1, 4, 5])
def test_task_counts_around_a_workgroup(tasks):
    """One cell of `tasks` tasks: one wavefront in a workgroup of four, a full workgroup, one task in a second one.
    (A transmitter heard once is a TOO_FEW cell: its one task is skipped, by a wavefront all the same.)"""
    assert _native.tdoamatrix_geometry()[2] == 4 == _native.TDOA_TASKS_PER_WORKGROUP
    times = {0: beacon_times(20), 7: np.linspace(5.2, 14.7, tasks).tolist()}
    cols, ptr, idx = scene(10 + tasks, 2, times)
    counts, out = run_and_check(cols, ptr, idx, "tasks %d" % tasks, beacons=[0], targets=[7])
    assert counts["tasks"] == tasks and counts["cells"] == 1
    assert counts["tdoas"] == (0 if tasks < 3 else tasks) and out["cell_flags"][0] == (tasks < 3)
    assert out["status"].tolist() == [G.OK if tasks >= 3 else 3] * tasks


def test_cell_boundaries_on_and_past_a_tile_boundary_with_more_tiles_than_workgroups():
    tile, workgroup, _ = _native.tdoamatrix_geometry()
    assert tile == workgroup == 256
    sizes = {1: tile, 2: tile + 1, 3: 2 * tile + 3}             # TDOA positions: [0, T) | [T, 2T + 1) | [2T + 1, 4T + 4)
    stop = 120.0
    rng = np.random.default_rng(3)
    times = {0: beacon_times(stop + 4, 1.0)}
    times.update({tx: np.sort(rng.uniform(4.0, stop, n)).tolist() for tx, n in sizes.items()})
    cols, ptr, idx = scene(31, 2, times)
    try:
        base = None
        for cap in (0, 2, 1):
            _native.seg_tile_grid(cap)
            counts, out = run_and_check(cols, ptr, idx, "cap %d" % cap, beacons=[0], targets=[1, 2, 3]) if cap != 1 else \
                _native.tdoamatrix(cols, ptr, idx, beacons=[0], targets=[1, 2, 3])
            launches, trips = _native.seg_tile_stats()
            n_tiles = (counts["tdoas"] + tile - 1) // tile
            assert out["cell_counts"][:, 2].tolist() == [sizes[1], sizes[2], sizes[3]] and n_tiles == 5    # every task gave a TDOA
            assert launches > 0 and trips == (1 if cap == 0 else (n_tiles + cap - 1) // cap)
            if base is None:
                base = out
            assert all(base[k].tobytes() == out[k].tobytes() for k in _native.TDMAT_OUTPUTS), cap
    finally:
        _native.seg_tile_grid(0)


def test_a_beacon_that_is_also_a_target_and_a_target_absent_at_one_receiver():
    times = {0: beacon_times(30), 1: beacon_times(30, 0.7), 5: np.arange(3.3, 27, 1.1).tolist(), 6: np.arange(2.9, 27, 1.3).tolist()}
    cols, ptr, idx = scene(41, 3, times, heard={6: [0, 2]})
    counts, out = run_and_check(cols, ptr, idx, "beacon as target", beacons=[1, 0])
    keys = [tuple(k) for k in out["cell_key"].tolist()]
    assert (0, 1, 0, 1) in keys and (0, 1, 1, 0) in keys and (0, 2, 0, 6) in keys      # each beacon against the other
    assert not any(k[3] == 6 and 1 in k[:2] for k in keys)                                # transmitter 6 is not heard at receiver 1
    assert keys == sorted(keys) and counts["cells"] == 3 * 2 * 3 - 4
    # the listed targets alone, a receiver list, another window, degree and model
    for kw in (dict(beacons=[0, 1], targets=[5]), dict(beacons=[0], targets=[1, 6], receivers=[2, 0]),
               dict(beacons=[0, 1], window=1.5, deg=1), dict(beacons=[1], deg=3, window=6.0), dict(beacons=[0], model="nearest")):
        if kw.get("model") == "nearest":
            want = tdoa_matrix_ref(cols, ptr, idx, **kw)[1]
            got = _native.tdoamatrix(cols, ptr, idx, **dict(kw, model=_native.TDOA_MODELS["nearest"]))[1]
            G.check_structure(got, want, "nearest")
            assert got["tdoa"].tobytes() == want["tdoa"].tobytes()
            G.check_own_mask_and_stats(got, "nearest")
        else:
            run_and_check(cols, ptr, idx, str(kw), **kw)


def test_real_geometry_against_the_statement():
    times = {0: beacon_times(20), 1: beacon_times(20, 0.8), 5: np.arange(3.3, 17, 0.9).tolist()}
    cols, ptr, idx = scene(43, 3, times)
    rng = np.random.default_rng(7)
    rx_pos = {r: rng.uniform(-900, 900, 2) for r in (2, 0, 1)}
    beacon_pos = {b: rng.uniform(-900, 900, 2) for b in (1, 0)}
    receivers, beacons = [2, 0, 1], [1, 0]             # the table's rows and columns follow the lists as given
    dist = np.array([[np.sqrt(np.sum((rx_pos[r] - beacon_pos[b]) ** 2)) for b in beacons] for r in receivers])
    want = tdoa_matrix_ref(cols, ptr, idx, beacons=beacons, receivers=receivers, rx_pos=rx_pos, beacon_pos=beacon_pos)[1]
    counts, out = _native.tdoamatrix(cols, ptr, idx, beacons=beacons, receivers=receivers, dist=dist)
    G.check_structure(out, want, "geometry")
    ok = want["status"] == G.OK
    assert ok.sum() > 50
    bound = 16 * want["cond"][ok] ** 2 * 2.0 ** -52 * want["spread"][ok] / FS
    assert np.all(np.abs(out["tdoa"][ok] - want["tdoa"][ok]) <= bound)
    zero = _native.tdoamatrix(cols, ptr, idx, beacons=beacons, receivers=receivers)[1]
    assert np.max(np.abs(out["tdoa"][ok] - zero["tdoa"][ok])) > 1e-8        # the geometry is read


def test_the_beacon_list_at_its_cap():
    cap = _native.TDMAT_MAX_BEACONS
    times = {b: [k + 0.01 * b for k in range(1, 7)] for b in range(cap)}
    times[100] = [3.45, 3.55, 3.65]
    cols, ptr, idx = scene(51, 2, times)
    counts, out = run_and_check(cols, ptr, idx, "cap", beacons=list(range(cap))[::-1], targets=[100])
    assert counts["cells"] == cap and counts["tasks"] == 3 * cap and counts["tdoas"] > 2 * cap
    assert out["cell_key"][:, 2].tolist() == list(range(cap)) and np.all(out["cell_counts"][:, 0] == 6)
    with pytest.raises(ValueError, match="at most %d beacons" % cap):
        _native.tdoamatrix(cols, ptr, idx, beacons=list(range(cap + 1)))


def test_zero_cells():
    cols, ptr, idx = scene(61, 2, {0: beacon_times(5), 7: [1.1, 2.2, 3.3]})
    empty = {name: np.zeros(0, kind) for name, kind in _native.TDMAT_COLUMNS}
    for what, args, kw in (("no match", (empty, np.zeros(1, np.int64), np.zeros(0, np.int64)), dict(beacons=[0])),
                           ("no beacon", (cols, ptr, idx), dict(beacons=[])),
                           ("no such target", (cols, ptr, idx), dict(beacons=[0], targets=[9])),
                           ("the beacon alone", (cols, ptr, idx), dict(beacons=[0], targets=[0])),
                           ("one receiver", (cols, ptr, idx), dict(beacons=[0], receivers=[1])),
                           ("matches of one detection", (cols, np.arange(len(idx) + 1, dtype=np.int64), idx), dict(beacons=[0]))):
        counts, out = _native.tdoamatrix(*args, **kw)
        assert counts == {"tasks": 0, "cells": 0, "rows": 0, "tdoas": 0}, what
        assert out["cell_ptr"].tolist() == [0] and all(out[k].size == 0 for k in _native.TDMAT_OUTPUTS if k != "cell_ptr"), what
        want = tdoa_matrix_ref(*args, **kw)[1]
        assert len(want["cell_key"]) == 0, what


def test_argument_errors():
    cols, ptr, idx = scene(71, 3, {0: beacon_times(5), 7: [1.1, 2.2, 3.3]})
    run = lambda **kw: _native.tdoamatrix(cols, ptr, idx, **kw)  # noqa: E731
    before = _native.live_resources()
    for kw, words in ((dict(beacons=[0, 1, 0]), "a beacon is listed twice"), (dict(beacons=[0], receivers=[0, 1, 1]), "a receiver is listed twice"),
                      (dict(beacons=[0], model=4), "model must be"), (dict(beacons=[0], model=-1), "model must be"),
                      (dict(beacons=[0], deg=0), "deg must be"), (dict(beacons=[0], deg=4), "deg must be"),
                      (dict(beacons=[0], window=-1.0), "window"), (dict(beacons=[0], window=float("nan")), "window"),
                      (dict(beacons=[0], sample_rate=0.0), "sample_rate"),
                      (dict(beacons=[0], dist=np.zeros((3, 1))), "dist needs the list of receivers"),
                      (dict(beacons=[0], receivers=[0, 1], dist=np.zeros((3, 1))), "dist must be")):
        with pytest.raises(ValueError, match=words):
            run(**kw)
    _native.tdoamatrix(cols, ptr, idx, beacons=[0], model=2, deg=0)            # the degree is not read by `nearest`
    twice = idx.copy()
    twice[1] = twice[0]                                 # the first match holds one detection twice: one receiver twice
    with pytest.raises(ValueError, match="two detections of one receiver"):
        _native.tdoamatrix(cols, ptr, twice, beacons=[0])
    with pytest.raises(ValueError, match="holds detection"):
        _native.tdoamatrix(cols, ptr, idx + 1, beacons=[0])
    with pytest.raises(ValueError, match="match_ptr decreases"):
        _native.tdoamatrix(cols, np.r_[ptr[:2], ptr[1] - 1, ptr[3:]], idx, beacons=[0])
    with pytest.raises(ValueError, match="not a CSR pair"):
        _native.tdoamatrix(cols, ptr[:-1], idx, beacons=[0])
    with pytest.raises(ValueError, match="a list of beacons is needed"):
        _native.tdoamatrix(cols, ptr, idx, beacons=None)
    assert _native.live_resources() == before            # a refused call leaves nothing behind
