"""`thr_posq` on the device (thrifty_amd/csrc/posq.hip, csrc/pos_lm.hpp).

Exact, no tolerance: `thr_pos` against the digests taken at the parent commit (the iteration moved into a header
template; with no weights it must return the bits it returned before); ungated and unweighted output against
`thr_pos`; an all-ones weight column against no weights; every candidate against one `thr_pos` call on the groups
rebuilt without that receiver's rows; flags, eligibility, choice and `excluded` against the rule stated in NumPy
on the device's own rms values; the gate's strictness.

Derived bounds, each stage from the device's previous output (u = 2^-53):
 * rms from the returned residuals: F is m (weighted) squares summed in a tree, then a division and a square
   root, on both sides: (m + 8) u relative;
 * a residual at the returned position: tc - (da - db) with two square roots of sums of two squares, on both
   sides: 8 u (|tc| + da + db);
 * q = inv(A), A taken from the NumPy statement at the returned position: 8 cond(A) m u relative to max |q|;
 * positions within kStepTol (|x*| + 1) + 4 ref_err_max of the fixture's exact minimiser: the first term is the
   project's stopping rule, the second the statement's own error with a margin of 4 for sums taken in team order
   instead of NumPy's.
"""
import hashlib

import numpy as np
import pytest

import pos_golden
import posq_golden
import posq_ref
from thrifty_amd import _native, pos_est, pos_quality, tdoa_est

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
STEP_TOL = 1e-13        # kStepTol of csrc/pos_lm.hpp
_runs = {}


def columns(g):
    """(group_ptr, dense rx0, dense rx1, tdoa, snr, table) of a pos or posq fixture."""
    if "rx_xy" in g:
        return g["group_ptr"], posq_golden.dense(g, g["rx0"]), posq_golden.dense(g, g["rx1"]), g["tdoa"], g["snr"], g["rx_xy"]
    return g["group_ptr"], pos_golden.dense(g, g["rx0"]), pos_golden.dense(g, g["rx1"]), g["tdoa"], g["snr"], g["rx_xyz"]


def run(name, weighted=False, gated=True):
    """One device call per (fixture, weights, gate), shared by the tests and left unchanged."""
    key = (name, weighted, gated)
    if key not in _runs:
        g = posq_golden.load(name)
        counts, out = _native.posq(*columns(g), row_weight=posq_golden.weights_of(g) if weighted else None,
                                   gate_m=float(g["gate_m"]) if gated else 0.0, ratio=float(g["ratio"]), min_rx=int(g["min_rx"]))
        for value in out.values():
            value.setflags(write=False)
        _runs[key] = (counts, out)
    return _runs[key]


@pytest.mark.parametrize("name", pos_golden.SETS_2D)
def test_thr_pos_returns_the_parents_bits(name):
    g = pos_golden.load(name)
    out = pos_est.pos_columns(g["group_ptr"], g["rx0"], g["rx1"], g["tdoa"], g["snr"], pos_golden.rx_pos(g))
    want = posq_golden.parent_digests()[name]
    for key in ("pos", "dop", "snr", "status", "iters"):
        assert hashlib.sha256(np.ascontiguousarray(out[key]).tobytes()).hexdigest() == want[key], key


@pytest.mark.parametrize("name", pos_golden.SETS_2D)
def test_ungated_unweighted_equals_thr_pos(name):
    cols = columns(pos_golden.load(name))
    want = _native.pos(*cols)
    counts, out = _native.posq(*cols)
    for key in ("pos", "dop", "snr", "status", "iters"):
        assert out[key].tobytes() == want[key].tobytes(), key
    assert out["full_pos"].tobytes() == want["pos"].tobytes() and out["full_status"].tobytes() == want["status"].tobytes()
    assert counts == {"groups": len(cols[0]) - 1, "rows": len(cols[1]), "flagged": 0, "tasks": 0}
    assert not out["flags"].any() and np.all(out["counts"][:, 2] == -1) and np.all(out["used"] == 1)
    assert not out["task_ptr"].any() and np.all(out["counts"][:, 1] == np.diff(cols[0]))
    assert np.array_equal(out["rms"][:, 0], out["rms"][:, 1], equal_nan=True)
    assert np.all(np.isnan(out["q"][out["dop"] == -1])) and np.all(np.isfinite(out["q"][out["dop"] != -1]))


@pytest.mark.parametrize("name", posq_golden.SETS)
def test_a_column_of_ones_is_the_unweighted_solve(name):
    g = posq_golden.load(name)
    cols = columns(g)
    _, want = run(name)
    _, out = _native.posq(*cols, row_weight=np.ones(len(cols[1])), gate_m=float(g["gate_m"]))
    assert set(out) == set(want) == set(_native.POSQ_OUTPUTS)
    for key in want:
        assert out[key].tobytes() == want[key].tobytes(), key


@pytest.mark.parametrize("name", posq_golden.SETS)
def test_every_candidate_is_thr_pos_without_that_receivers_rows(name):
    counts, out = run(name)
    assert posq_golden.assert_candidates_equal_thr_pos(out, *columns(posq_golden.load(name))) == counts["tasks"] > 0


@pytest.mark.parametrize("name,weighted", [("posq_fault6", False), ("posq_weighted7", False), ("posq_weighted7", True)])
def test_flags_and_choice_follow_the_rule(name, weighted):
    g = posq_golden.load(name)
    counts, out = run(name, weighted)
    ptr, rx0, rx1 = columns(g)[:3]
    posq_golden.assert_choice_follows_the_rule(out, ptr, rx0, rx1, float(g["gate_m"]), float(g["ratio"]), int(g["min_rx"]))
    assert counts["flagged"] == int(np.count_nonzero(out["flags"] & _native.POSQ_INCONSISTENT)) > 0
    assert np.count_nonzero(out["flags"] & _native.POSQ_EXCLUDED) > 0


def test_the_gate_is_strict():
    g = posq_golden.load("posq_fault6")
    ptr, rx0, rx1, tdoa, snr, table = columns(g)
    k = int(np.flatnonzero(g["planted"] >= 0)[0])
    rows = slice(int(ptr[k]), int(ptr[k + 1]))
    one = ([0, rows.stop - rows.start], rx0[rows], rx1[rows], tdoa[rows], snr[rows], table)
    rms = float(_native.posq(*one)[1]["rms"][0, 0])
    assert rms > 3.0
    at, _ = _native.posq(*one, gate_m=rms)
    below, out = _native.posq(*one, gate_m=float(np.nextafter(rms, 0.0)))
    assert (at["flagged"], at["tasks"]) == (0, 0) and (below["flagged"], below["tasks"]) == (1, 6)
    assert out["flags"][0] & _native.POSQ_INCONSISTENT


def _task_rows(g, out, weighted):
    """Per group: the rows of the chosen task, their normalised weights (None: unweighted)."""
    ptr = g["group_ptr"].tolist()
    weights = posq_golden.weights_of(g) if weighted else None
    for k, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
        use = out["used"][a:b] != 0
        w = None if weights is None else posq_ref.task_weights(weights[a:b], use)[use]
        yield k, np.arange(a, b)[use], w


@pytest.mark.parametrize("name,weighted", [("posq_fault6", False), ("posq_weighted7", True)])
def test_rms_residuals_and_q_within_their_bounds(name, weighted):
    g = posq_golden.load(name)
    ptr, rx0, rx1, tdoa, snr, table = columns(g)
    _, out = run(name, weighted)
    worst = {"rms": 0.0, "residual": 0.0, "q": 0.0}
    for k, rows, w in _task_rows(g, out, weighted):
        p, m = out["pos"][k], len(rows)
        # residuals at the returned position
        va, vb = table[rx0[rows]] - p, table[rx1[rows]] - p
        da, db = np.hypot(va[:, 0], va[:, 1]), np.hypot(vb[:, 0], vb[:, 1])
        want = posq_ref.residuals(p, rx0[rows], rx1[rows], tdoa[rows], table)
        got = out["residual"][rows]
        bound = 8 * U * (np.abs(tdoa[rows] * posq_golden.C) + da + db)
        worst["residual"] = max(worst["residual"], float(np.max(np.abs(got - want) / bound)))
        assert np.all(np.abs(got - want) <= bound), k
        # rms from the returned residuals
        rms = np.sqrt(np.sum(got * got if w is None else w * (got * got)) / m)
        worst["rms"] = max(worst["rms"], abs(out["rms"][k, 1] - rms) / rms / ((m + 8) * U))
        assert abs(out["rms"][k, 1] - rms) <= (m + 8) * U * rms, k
        # q against the inverse of the statement's A at the returned position
        s = posq_ref.evaluate(p, table[rx0[rows]], table[rx1[rows]], tdoa[rows] * posq_golden.C, w)
        a = np.array([[s[1], s[2]], [s[2], s[3]]])
        q = np.linalg.inv(a)
        bound = 8 * np.linalg.cond(a) * m * U * np.max(np.abs(q))
        err = np.max(np.abs(out["q"][k] - [q[0, 0], q[0, 1], q[1, 1]]))
        worst["q"] = max(worst["q"], float(err / bound))
        assert err <= bound, k
    print("largest share of the bound used:", worst)


@pytest.mark.parametrize("name,weighted", [("posq_fault6", False), ("posq_weighted7", True)])
def test_positions_sit_on_the_exact_minimisers(name, weighted):
    g = posq_golden.load(name)
    if not weighted:        # the fixture's minimisers are those of its own weights: posq_fault6 has none
        assert posq_golden.weights_of(g) is None
    _, out = run(name, weighted)
    np.testing.assert_array_equal(out["task_ptr"], g["ref_task_ptr"])
    worst = 0.0
    for pos, status, star in ((out["full_pos"], out["full_status"], g["full_x_star"]),
                              (out["task_pos"], out["task_status"], g["task_x_star"])):
        ok = (status == _native.POS_OK) & np.all(np.isfinite(star), axis=1)
        assert ok.sum() >= len(ok) // 2
        bound = STEP_TOL * (np.hypot(star[ok, 0], star[ok, 1]) + 1.0) + 4.0 * float(g["ref_err_max"])
        err = np.max(np.abs(pos[ok] - star[ok]), axis=1)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound)
    print("max |x - x_star| / bound = %.3g (ref_err_max %.3g m)" % (worst, float(g["ref_err_max"])))


def test_the_planted_receiver_is_excluded_and_no_other():
    g = posq_golden.load("posq_fault6")
    out = pos_quality.quality_columns(g["group_ptr"], g["rx0"], g["rx1"], g["tdoa"], g["snr"], posq_golden.rx_pos(g),
                                      exclude_gate_m=float(g["gate_m"]), ratio=float(g["ratio"]), min_rx=int(g["min_rx"]))
    np.testing.assert_array_equal(out["excluded"], g["planted"])
    affected = g["planted"] >= 0
    assert affected.sum() == 16
    np.testing.assert_array_equal(out["flags"], np.where(affected, pos_quality.INCONSISTENT | pos_quality.EXCLUDED, 0))
    assert np.all(out["rms"][affected] <= 0.5 * out["rms_full"][affected]) and out["rms"].max() < 0.9
    np.testing.assert_array_equal(out["n_rx"], np.where(affected, 5, 6))
    np.testing.assert_array_equal(out["n_rows"], np.where(affected, 10, 15))
    assert set(out["task_rx"].tolist()) == set(g["rx_ids"].tolist()) and out["counts"]["tasks"] == 96


def _groups(g):
    rows = np.zeros(len(g["tdoa"]), dtype=tdoa_est.TDOA_DTYPE)
    for name in ("rx0", "rx1", "tdoa", "snr"):
        rows[name] = g[name]
    ptr = g["group_ptr"].tolist()
    return [tdoa_est.TdoaGroup(int(i), float(t), int(tx), rows[a:b]) for i, t, tx, a, b in
            zip(g["group_id"], g["group_timestamp"], g["group_tx"], ptr[:-1], ptr[1:])]


def test_solve_and_the_command_line(tmp_path, capsys):
    g = posq_golden.load("posq_weighted7")
    _, dev = run("posq_weighted7", weighted=True)
    res = pos_quality.solve(_groups(g), posq_golden.rx_pos(g), weights=g["weights"], exclude_gate_m=float(g["gate_m"]))
    assert capsys.readouterr().out == "" and res.dtype.names == pos_quality.QUALITY_DTYPE["names"] and len(res) == 24
    np.testing.assert_array_equal(res["group_id"], g["group_id"])
    np.testing.assert_array_equal(np.stack([res["x"], res["y"]], axis=1), dev["pos"])
    np.testing.assert_array_equal(res["rms"], dev["rms"][:, 1])
    np.testing.assert_array_equal(res["flags"], dev["flags"])
    np.testing.assert_array_equal(res["excluded"], np.where(dev["counts"][:, 2] >= 0, g["rx_ids"][np.maximum(dev["counts"][:, 2], 0)], -1))
    for k in range(len(res)):
        want = posq_ref.ellipse(dev["q"][k])
        got = [res[name][k] for name in ("xdop", "ydop", "major", "minor", "angle")]
        assert np.allclose(got, want, rtol=1e-12, atol=1e-12)      # the host's closed form against numpy's eigvalsh
        assert abs(res["dop"][k] - np.hypot(res["xdop"][k], res["ydop"][k])) <= 1e-12 * res["dop"][k]
    # the command line with --weights snr: the fixture's weights are its snr column with some zeros, so not the same run
    tdoa, cfg, posq, pos = (tmp_path / n for n in ("data.tdoa", "pos-rx.cfg", "data.posq", "data.pos"))
    tdoa_est.save_tdoa_groups(str(tdoa), _groups(g))
    cfg.write_text("".join("%d: %s\n" % (r, " ".join(repr(float(v)) for v in xy)) for r, xy in posq_golden.rx_pos(g).items()))
    assert pos_quality._main([str(tdoa), "-r", str(cfg), "-o", str(posq), "--weights", "snr", "--exclude", "3", "--pos", str(pos)]) == 0
    text = capsys.readouterr().out
    back, held = pos_quality.load_quality(str(posq)), pos_est.load_positions(str(pos))
    want = pos_quality.solve(tdoa_est.load_tdoa_groups(str(tdoa)), posq_golden.rx_pos(g), weights="snr", exclude_gate_m=3.0)
    assert back.tolist() == want.tolist() and text == pos_quality.format_summary(want)
    assert held.dtype.names == ("group_id", "timestamp", "tx", "dop", "snr", "x", "y")
    assert held.tolist() == [tuple(r)[:7] for r in want.tolist()]
    assert np.count_nonzero(back["flags"] & pos_quality.EXCLUDED) > 0


def test_times_are_reported():
    g = posq_golden.load("posq_fault6")
    _native.posq(*columns(g), gate_m=3.0)
    times = _native.posq_times()
    assert len(times) == 6 and all(t > 0 for t in times)
