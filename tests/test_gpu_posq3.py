"""`thr_posq3` on the device (thrifty_amd/csrc/posq3.hip, csrc/pos3_lm.hpp).

Exact, no tolerance: `thr_pos3` and `thr_posg3` against the digests taken at the parent commit (the iteration learnt
weights and a row subset behind defaulted template parameters; the unweighted all-rows instantiation must return the
bits it returned before); ungated and unweighted output against `thr_pos3` in both modes; an all-ones weight column
against no weights; every candidate against one `thr_pos3` call on the groups rebuilt without that receiver's rows;
the known-height mode with every antenna at the height against `thr_posq` on the flat table; flags, eligibility,
choice, `excluded`, `used` and n_rows against the rule stated in NumPy on the device's own rms values; the gate's
strictness; the planted receivers.

Derived bounds, each stage from the device's previous output (u = 2^-53):
 * rms from the returned residuals: F is m (weighted) squares summed in a tree, then a division and a square
   root, on both sides: (m + 8) u relative;
 * a residual at the returned position: tc - (da - db) with two square roots of sums of THREE squares, on both
   sides.  test_gpu_posq.py's bound for two squares is 8 u (|tc| + da + db); the third square puts one more
   addition under each root, one more rounding u on the radicand, which the root halves: 0.5 u relative on da and
   on db, on either side, hence 9 u (|tc| + da + db);
 * q = inv(A), A taken from the NumPy statement at the returned position: 8 cond(A) m u relative to max |q|;
 * positions within kStepTol (|x*| + 1) + 4 ref_err_max of the fixture's exact minimiser: the first term is the
   project's stopping rule, the second the statement's own error with a margin of 4 for sums taken in team order
   instead of NumPy's.
"""
import hashlib

import numpy as np
import pytest

import pos3_golden
import posg3_golden
import posq3_golden
import posq3_ref
import posq_golden
import posq_ref
from thrifty_amd import _native, pos_3d, pos_3d_quality, pos_est, pos_quality, tdoa_est, track

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
STEP_TOL = 1e-13        # kStepTol of csrc/pos_lm.hpp
_runs = {}


def run(name, weighted=True, gated=True):
    """One device call per (fixture, weights, gate), shared by the tests and left unchanged."""
    key = (name, weighted, gated)
    if key not in _runs:
        g = posq3_golden.load(name)
        counts, out = _native.posq3(*posq3_golden.columns(g), **posq3_golden.options(g, weighted, gated))
        for value in out.values():
            value.setflags(write=False)
        _runs[key] = (counts, out)
    return _runs[key]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("name", pos3_golden.SETS)
def test_thr_pos3_returns_the_parents_bits(name):
    g = pos3_golden.load(name)
    out = pos_3d.pos3_columns(g["group_ptr"], g["rx0"], g["rx1"], g["tdoa"], g["snr"], pos3_golden.rx_pos(g), **pos3_golden.mode_args(g))
    want = posq3_golden.parent_digests()["thr_pos3"][name]
    assert set(want) == set(_native.POS3_OUTPUTS)
    for key in _native.POS3_OUTPUTS:
        assert sha(out[key]) == want[key], key


@pytest.mark.parametrize("name", posg3_golden.SETS)
def test_thr_posg3_returns_the_parents_bits(name):
    g = posg3_golden.load(name)
    _, out = _native.posg3(*posg3_golden.columns(g), posg3_golden.mode_of(g), map_first=0, map_count=len(g["group_id"]),
                           **posg3_golden.options(g))
    want = posq3_golden.parent_digests()["thr_posg3"][name]
    assert set(want) == set(_native.POSG3_OUTPUTS)
    for key in _native.POSG3_OUTPUTS:
        assert sha(out[key]) == want[key], key


def pos3_call(g):
    """(the columns and the mode, the keyword arguments both thr_pos3 and thr_posq3 take) of a pos3 fixture."""
    free_z = pos3_golden.free_z(g)
    cols = (g["group_ptr"], pos3_golden.dense(g, g["rx0"]), pos3_golden.dense(g, g["rx1"]), g["tdoa"], g["snr"], g["rx_xyz"],
            _native.POS3_FREE_Z if free_z else _native.POS3_KNOWN_HEIGHT)
    shared = dict(group_h=None if free_z else g["group_h"], x0=(0.1, 0.1, float(g["z0"]) if free_z else 0.0),
                  z_range=tuple(g["z_range"].tolist()) if free_z and len(g["z_range"]) else None)
    return cols, shared


@pytest.mark.parametrize("name", pos3_golden.SETS)
def test_ungated_unweighted_equals_thr_pos3(name):
    cols, shared = pos3_call(pos3_golden.load(name))
    want = _native.pos3(*cols, **shared)
    counts, out = _native.posq3(*cols, **shared)
    for key in ("pos", "dop", "hdop", "vdop", "snr", "status", "iters"):
        assert out[key].tobytes() == want[key].tobytes(), key
    assert np.ascontiguousarray(out["rms"][:, 0]).tobytes() == want["rms"].tobytes()
    assert out["full_pos"].tobytes() == want["pos"].tobytes() and out["full_status"].tobytes() == want["status"].tobytes()
    assert counts == {"groups": len(cols[0]) - 1, "rows": len(cols[1]), "flagged": 0, "tasks": 0}
    assert not out["flags"].any() and np.all(out["counts"][:, 2] == -1) and np.all(out["used"] == 1)
    assert not out["task_ptr"].any() and np.all(out["counts"][:, 1] == np.diff(cols[0]))
    assert np.array_equal(out["rms"][:, 0], out["rms"][:, 1], equal_nan=True)
    assert np.all(np.isnan(out["q"][out["dop"] == -1][:, :3])) and np.all(np.isfinite(out["q"][out["dop"] != -1]))
    if cols[6] == _native.POS3_KNOWN_HEIGHT:
        assert np.all(out["q"][:, 3:] == 0.0)


@pytest.mark.parametrize("name", posq3_golden.SETS)
def test_a_column_of_ones_is_the_unweighted_solve(name):
    g = posq3_golden.load(name)
    cols = posq3_golden.columns(g)
    _, want = run(name, weighted=False)
    opts = posq3_golden.options(g, weighted=False)
    opts["row_weight"] = np.ones(len(cols[1]))
    _, out = _native.posq3(*cols, **opts)
    assert set(out) == set(want) == set(_native.POSQ3_OUTPUTS)
    for key in want:
        assert out[key].tobytes() == want[key].tobytes(), key


@pytest.mark.parametrize("name", posq3_golden.SETS)
def test_every_candidate_is_thr_pos3_without_that_receivers_rows(name):
    g = posq3_golden.load(name)
    counts, out = run(name, weighted=False)
    opts = posq3_golden.options(g)
    n = posq3_golden.assert_candidates_equal_thr_pos3(out, *posq3_golden.columns(g), group_h=opts["group_h"], x0=opts["x0"],
                                                      z_range=opts["z_range"])
    assert n == counts["tasks"] > 0


@pytest.mark.parametrize("name", posq_golden.SETS)
def test_antennas_at_the_known_height_give_thr_posqs_bytes(name):
    """posq's fixtures lifted to z = 12.5 m with group_h = 12.5 m, weighted where the fixture is, gated: vz is 0
    everywhere, and every output thr_posq has equals thr_posq's on the flat table byte for byte."""
    g = posq_golden.load(name)
    ptr, rx0, rx1 = g["group_ptr"], posq_golden.dense(g, g["rx0"]), posq_golden.dense(g, g["rx1"])
    opts = dict(row_weight=posq_golden.weights_of(g), gate_m=float(g["gate_m"]), ratio=float(g["ratio"]), min_rx=int(g["min_rx"]))
    flat_counts, want = _native.posq(ptr, rx0, rx1, g["tdoa"], g["snr"], g["rx_xy"], **opts)
    lifted = np.c_[g["rx_xy"], np.full(len(g["rx_xy"]), 12.5)]
    counts, out = _native.posq3(ptr, rx0, rx1, g["tdoa"], g["snr"], lifted, _native.POS3_KNOWN_HEIGHT,
                                group_h=np.full(len(ptr) - 1, 12.5), **opts)
    assert counts == flat_counts and counts["tasks"] > 0 and set(_native.POSQ_OUTPUTS) <= set(_native.POSQ3_OUTPUTS)
    for key in _native.POSQ_OUTPUTS:
        ours = out[key]
        if key in ("pos", "full_pos", "task_pos"):
            assert np.all(ours[:, 2] == 12.5), key
            ours = np.ascontiguousarray(ours[:, :2])
        if key == "q":
            assert np.all(ours[:, 3:] == 0.0)
            ours = np.ascontiguousarray(ours[:, :3])
        assert ours.tobytes() == want[key].tobytes(), key
    assert out["hdop"].tobytes() == out["dop"].tobytes() and np.all(out["vdop"] == 0.0)
    for key in _native.POSQ_OUTPUTS:       # the same index and element type
        assert _native.POSQ3_OUTPUTS[key][:2] == _native.POSQ_OUTPUTS[key][:2], key


@pytest.mark.parametrize("name,weighted", [("h_fault6", False), ("h_five", False), ("z_fault7", False), ("z_weighted7", False),
                                           ("z_weighted7", True)])
def test_flags_and_choice_follow_the_rule(name, weighted):
    g = posq3_golden.load(name)
    counts, out = run(name, weighted)
    ptr, rx0, rx1 = posq3_golden.columns(g)[:3]
    posq3_golden.assert_choice_follows_the_rule(out, ptr, rx0, rx1, float(g["gate_m"]), float(g["ratio"]), int(g["min_rx"]))
    assert counts["flagged"] == int(np.count_nonzero(out["flags"] & _native.POSQ3_INCONSISTENT)) > 0
    assert np.count_nonzero(out["flags"] & _native.POSQ3_EXCLUDED) > 0
    # the chosen task's dops and q are the dops of a solve on the used rows: hdop / vdop against q
    ok = out["dop"] != -1
    q = out["q"][ok]
    if bool(g["free_z"]):
        assert np.allclose(out["hdop"][ok], np.sqrt(q[:, 0] + q[:, 2]), rtol=1e-14, atol=0)
        assert np.allclose(out["vdop"][ok], np.sqrt(q[:, 5]), rtol=1e-14, atol=0)
    else:
        assert out["hdop"].tobytes() == out["dop"].tobytes() and np.all(out["vdop"] == 0.0)
        np.testing.assert_array_equal(out["pos"][:, 2], g["group_h"])


@pytest.mark.parametrize("name,n_rx", [("h_fault6", 6), ("z_fault7", 7)])
def test_the_gate_is_strict(name, n_rx):
    g = posq3_golden.load(name)
    ptr, rx0, rx1, tdoa, snr, table, mode = posq3_golden.columns(g)
    k = int(np.flatnonzero(g["planted"] >= 0)[0])
    rows = slice(int(ptr[k]), int(ptr[k + 1]))
    opts = posq3_golden.options(g, weighted=False, gated=False)
    if opts["group_h"] is not None:
        opts["group_h"] = opts["group_h"][k:k + 1]
    one = ([0, rows.stop - rows.start], rx0[rows], rx1[rows], tdoa[rows], snr[rows], table, mode)
    rms = float(_native.posq3(*one, **opts)[1]["rms"][0, 0])
    assert rms > 3.0
    at, _ = _native.posq3(*one, **dict(opts, gate_m=rms))
    below, out = _native.posq3(*one, **dict(opts, gate_m=float(np.nextafter(rms, 0.0))))
    assert (at["flagged"], at["tasks"]) == (0, 0) and (below["flagged"], below["tasks"]) == (1, n_rx)
    assert out["flags"][0] & _native.POSQ3_INCONSISTENT


def _task_rows(g, out, weighted):
    """Per group: the rows of the chosen task, their normalised weights (None: unweighted)."""
    ptr = g["group_ptr"].tolist()
    weights = posq3_golden.weights_of(g) if weighted else None
    for k, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
        use = out["used"][a:b] != 0
        w = None if weights is None else posq_ref.task_weights(weights[a:b], use)[use]
        yield k, np.arange(a, b)[use], w


@pytest.mark.parametrize("name,weighted", [("h_fault6", False), ("z_fault7", False), ("z_weighted7", True), ("h_five", False)])
def test_rms_residuals_and_q_within_their_bounds(name, weighted):
    g = posq3_golden.load(name)
    ptr, rx0, rx1, tdoa, snr, table, mode = posq3_golden.columns(g)
    _, out = run(name, weighted)
    worst = {"rms": 0.0, "residual": 0.0, "q": 0.0}
    for k, rows, w in _task_rows(g, out, weighted):
        p, m = out["pos"][k], len(rows)
        h = 0.0 if mode == posq3_golden.FREE_Z else float(g["group_h"][k])
        # residuals at the returned position
        da = np.sqrt(np.sum((table[rx0[rows]] - p) ** 2, axis=1))
        db = np.sqrt(np.sum((table[rx1[rows]] - p) ** 2, axis=1))
        want = posq3_ref.residuals(p, rx0[rows], rx1[rows], tdoa[rows], table)
        got = out["residual"][rows]
        bound = 9 * U * (np.abs(tdoa[rows] * posq3_golden.C) + da + db)
        worst["residual"] = max(worst["residual"], float(np.max(np.abs(got - want) / bound)))
        assert np.all(np.abs(got - want) <= bound), k
        # rms from the returned residuals
        rms = np.sqrt(np.sum(got * got if w is None else w * (got * got)) / m)
        worst["rms"] = max(worst["rms"], abs(out["rms"][k, 1] - rms) / rms / ((m + 8) * U))
        assert abs(out["rms"][k, 1] - rms) <= (m + 8) * U * rms, k
        # q against the inverse of the statement's A at the returned position
        a = posq3_ref.normal_at(p, rx0[rows], rx1[rows], tdoa[rows], table, mode, h, w)
        q = np.linalg.inv(a)
        want_q = [q[0, 0], q[0, 1], q[1, 1]] + ([q[0, 2], q[1, 2], q[2, 2]] if mode == posq3_golden.FREE_Z else [0.0, 0.0, 0.0])
        bound = 8 * np.linalg.cond(a) * m * U * np.max(np.abs(q))
        err = np.max(np.abs(out["q"][k] - want_q))
        worst["q"] = max(worst["q"], float(err / bound))
        assert err <= bound, k
    print("largest share of the bound used:", worst)


@pytest.mark.parametrize("name,weighted", [("h_fault6", False), ("z_fault7", False), ("z_weighted7", True), ("h_five", False)])
def test_positions_sit_on_the_exact_minimisers(name, weighted):
    g = posq3_golden.load(name)
    if not weighted:        # the fixture's minimisers are those of its own weights
        assert posq3_golden.weights_of(g) is None
    _, out = run(name, weighted)
    np.testing.assert_array_equal(out["task_ptr"], g["ref_task_ptr"])
    worst = 0.0
    for pos, status, star in ((out["full_pos"], out["full_status"], g["full_x_star"]),
                              (out["task_pos"], out["task_status"], g["task_x_star"])):
        ok = (status == _native.POS_OK) & np.all(np.isfinite(star), axis=1)
        # with z free most candidates still hold the late receiver and end UNCONVERGED or AT_BOUND: the excluded ones are OK
        assert ok.sum() >= np.count_nonzero(out["flags"] & _native.POSQ3_EXCLUDED) > 0
        bound = STEP_TOL * (np.sqrt(np.sum(star[ok] ** 2, axis=1)) + 1.0) + 4.0 * float(g["ref_err_max"])
        err = np.max(np.abs(pos[ok] - star[ok]), axis=1)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound)
    print("max |x - x_star| / bound = %.3g (ref_err_max %.3g m)" % (worst, float(g["ref_err_max"])))


@pytest.mark.parametrize("name", posq3_golden.SETS)
def test_the_planted_receiver_is_excluded_and_no_other(name):
    g = posq3_golden.load(name)
    out = pos_3d_quality.quality3_columns(g["group_ptr"], g["rx0"], g["rx1"], g["tdoa"], g["snr"], posq3_golden.rx_pos(g),
                                          weights=posq3_golden.weights_of(g), exclude_gate_m=float(g["gate_m"]),
                                          ratio=float(g["ratio"]), min_rx=int(g["min_rx"]), **posq3_golden.mode_args(g))
    np.testing.assert_array_equal(out["excluded"], g["planted"])
    affected = g["planted"] >= 0
    assert affected.sum() >= 6
    np.testing.assert_array_equal(out["flags"], np.where(affected, pos_3d_quality.INCONSISTENT | pos_3d_quality.EXCLUDED, 0))
    assert np.all(out["rms"][affected] <= float(g["ratio"]) * out["rms_full"][affected])
    np.testing.assert_array_equal(out["flags"], g["ref_flags"])
    assert set(out["task_rx"].tolist()) <= set(g["rx_ids"].tolist())


def _groups(g):
    rows = np.zeros(len(g["tdoa"]), dtype=tdoa_est.TDOA_DTYPE)
    for name in ("rx0", "rx1", "tdoa", "snr"):
        rows[name] = g[name]
    ptr = g["group_ptr"].tolist()
    return [tdoa_est.TdoaGroup(int(i), float(t), int(tx), rows[a:b]) for i, t, tx, a, b in
            zip(g["group_id"], g["group_timestamp"], g["group_tx"], ptr[:-1], ptr[1:])]


@pytest.mark.parametrize("name", ["h_fault6", "z_weighted7"])
def test_solve_and_the_command_line(name, tmp_path, capsys):
    g = posq3_golden.load(name)
    free_z = bool(g["free_z"])
    _, dev = run(name)
    res = pos_3d_quality.solve(_groups(g), posq3_golden.rx_pos(g), weights=posq3_golden.weights_of(g), exclude_gate_m=float(g["gate_m"]),
                               **posq3_golden.mode_args(g))
    assert capsys.readouterr().out == "" and res.dtype.names == pos_3d_quality.QUALITY3_DTYPE["names"] and len(res) == len(g["group_id"])
    np.testing.assert_array_equal(res["group_id"], g["group_id"])
    np.testing.assert_array_equal(np.stack([res["x"], res["y"], res["z"]], axis=1), dev["pos"])
    np.testing.assert_array_equal(res["rms"], dev["rms"][:, 1])
    np.testing.assert_array_equal(res["flags"], dev["flags"])
    for key in ("dop", "hdop", "vdop"):
        np.testing.assert_array_equal(res[key], dev[key])
    np.testing.assert_array_equal(res["excluded"], np.where(dev["counts"][:, 2] >= 0, g["rx_ids"][np.maximum(dev["counts"][:, 2], 0)], -1))
    np.testing.assert_array_equal(res["zdop"], np.sqrt(dev["q"][:, 5]))
    for k in range(len(res)):
        want = posq_ref.ellipse(dev["q"][k, :3])
        got = [res[key][k] for key in ("xdop", "ydop", "major", "minor", "angle")]
        assert np.allclose(got, want, rtol=1e-12, atol=1e-12)      # the host's closed form against numpy's eigvalsh
        assert abs(res["hdop"][k] - np.hypot(res["xdop"][k], res["ydop"][k])) <= 1e-12 * res["hdop"][k]
    # the command line, every option
    tdoa, cfg, posq3, pos, posq = (tmp_path / n for n in ("data.tdoa", "pos-rx.cfg", "data.posq3", "data.pos", "data.posq"))
    tdoa_est.save_tdoa_groups(str(tdoa), _groups(g))
    cfg.write_text("".join("%d: %s\n" % (r, " ".join(repr(float(v)) for v in xyz)) for r, xyz in posq3_golden.rx_pos(g).items()))
    if free_z:
        mode = ["--free-z", "--z0", repr(float(g["z0"])), "--z-range"] + [repr(float(v)) for v in g["z_range"]]
        kwargs = dict(free_z=True, z0=float(g["z0"]), z_range=tuple(g["z_range"].tolist()))
    else:
        mode = ["--height", "0.0", "--height-tx", "7=%r" % float(g["group_h"][0])]
        kwargs = dict(height={7: float(g["group_h"][0])})
    argv = [str(tdoa), "-r", str(cfg), "-o", str(posq3), "--weights", "snr", "--exclude", "3", "--ratio", "0.6", "--min-rx",
            str(int(g["min_rx"])), "--pos", str(pos), "--posq", str(posq)] + mode
    assert pos_3d_quality._main(argv) == 0
    text = capsys.readouterr().out
    back, held, flat = pos_3d_quality.load_quality3(str(posq3)), pos_est.load_positions(str(pos)), pos_quality.load_quality(str(posq))
    want = pos_3d_quality.solve(tdoa_est.load_tdoa_groups(str(tdoa)), posq3_golden.rx_pos(g), weights="snr", exclude_gate_m=3.0,
                                ratio=0.6, min_rx=int(g["min_rx"]), **kwargs)
    assert back.tolist() == want.tolist() and text == pos_3d_quality.format_summary(want)
    axes = ("x", "y", "z") if free_z else ("x", "y")
    assert held.dtype.names == ("group_id", "timestamp", "tx", "dop", "snr") + axes
    assert held.tolist() == [tuple(r[key].item() for key in held.dtype.names) for r in want]
    assert flat.tolist() == pos_3d_quality.horizontal(want).tolist()
    np.testing.assert_array_equal(flat["dop"], want["hdop"])
    assert np.count_nonzero(back["flags"] & pos_3d_quality.EXCLUDED) > 0
    # what thrifty_amd.track makes of the .posq file: per-axis variances from xdop / ydop, every row valid
    var_x, var_y, valid = track.measurement_columns(flat, 2.0)
    np.testing.assert_array_equal(valid, (flat["flags"] & pos_quality.NO_CANDIDATE) == 0)
    assert valid.any() and np.array_equal(var_x, (2.0 * flat["xdop"]) ** 2) and np.array_equal(var_y, (2.0 * flat["ydop"]) ** 2)


def test_times_are_reported():
    g = posq3_golden.load("z_fault7")
    _native.posq3(*posq3_golden.columns(g), **posq3_golden.options(g))
    times = _native.posq3_times()
    assert len(times) == 6 and all(t > 0 for t in times)
