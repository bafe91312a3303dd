"""`thr_coverage` on the device against the fixtures (tests/golden/make_golden_coverage.py) and the NumPy statement
(tests/coverage_ref.py): cells, hearing and rows exactly, the noise and the tdoas within their derived bounds, every kept
trial byte for byte `thr_pos` on the kept columns, the reduction against the rule on the device's own trials, the analytic
columns within the bound the host test validates, the whole map's discrete outputs where the statement's margin allows
it, the end-to-end claims on `far4` and `ring5`, and repeatability."""
import numpy as np
import pytest

import coverage_golden as G
import coverage_ref
from pos_ref import OK
from thrifty_amd import _native, coverage

pytestmark = pytest.mark.gpu
_runs = {}


def keep_range(g):
    """As many cells as one call keeps, ending on the last cell."""
    n = int(g["nx"]) * int(g["ny"])
    count = min(n, _native.COVERAGE_MAX_KEEP)
    return n - count, count


def run(name):
    """(fixture, counts, outputs) of one device call with the kept cells -- computed once per fixture."""
    if name not in _runs:
        g = G.load(name)
        first, count = keep_range(g)
        counts, out = G.native_call(g, keep_first=first, keep_count=count)
        _runs[name] = (g, counts, out)
    return _runs[name]


def kept_cells(g):
    """[(cell, receivers, first kept task)] of the covered kept cells."""
    first, count = keep_range(g)
    cells, task = [], 0
    for c in range(first, first + count):
        receivers = [r for r in range(len(g["table"])) if (int(g["ref_heard_mask"][c]) >> r) & 1]
        if len(receivers) >= 3:
            cells.append((c, receivers, task))
            task += int(g["trials"])
    return cells


def centre_of(g, c):
    return float(g["ref_cx"][c % int(g["nx"])]), float(g["ref_cy"][c // int(g["nx"])])


@pytest.mark.parametrize("name", G.SETS)
def test_cells_hearing_and_rows_equal_the_statements(name):
    g, counts, out = run(name)
    T, cells = int(g["trials"]), kept_cells(g)
    covered = g["ref_n_heard"] >= 3
    assert counts["cells"] == len(covered) and counts["covered"] == covered.sum() and counts["tasks"] == covered.sum() * T
    assert counts["keep_tasks"] == len(cells) * T and counts["slabs"] == 1 and counts["n_rx"] == len(g["table"])
    assert out["cx"].tobytes() == g["ref_cx"].tobytes() and out["cy"].tobytes() == g["ref_cy"].tobytes()
    np.testing.assert_array_equal(out["n_heard"], g["ref_n_heard"])
    np.testing.assert_array_equal(out["heard_mask"], g["ref_heard_mask"])
    np.testing.assert_array_equal(out["flags"] & 3, g["ref_flags"] & 3)
    want = [coverage_ref.pairs(receivers) for _, receivers, _ in cells for _ in range(T)]
    np.testing.assert_array_equal(out["keep_ptr"], np.cumsum([0] + [len(p[0]) for p in want]))
    np.testing.assert_array_equal(out["keep_rx0"], np.concatenate([p[0] for p in want]))
    np.testing.assert_array_equal(out["keep_rx1"], np.concatenate([p[1] for p in want]))
    assert counts["keep_rows"] == len(out["keep_rx0"]) and counts["rows"] == sum(
        int(h) * (int(h) - 1) // 2 for h in g["ref_n_heard"][covered]) * T


@pytest.mark.parametrize("name", G.SETS)
def test_noise_and_tdoas_are_within_their_derived_bounds(name):
    """The noise: coverage_golden.noise_bound -- 8 * 2^-52 * sigma_r * sqrt(-2 ln 2^-32) from the documented errors of
    log (1 ulp), cos (2 ulp) and sqrt (correctly rounded) on both sides; u1, u2 and the argument of cos are the same
    bits.  The tdoas: coverage_golden.tdoa_bound, the two noises' bounds over c plus four roundings of the row."""
    g, _, out = run(name)
    T, bound = int(g["trials"]), G.noise_bound(g["sigma"])
    worst = 0.0
    for c, receivers, task in kept_cells(g):
        got = out["keep_noise"][task:task + T]
        diff = np.abs(got - g["ref_noise"][c])
        assert np.all(diff <= bound), c
        worst = max(worst, float(np.max(diff[:, bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0)
        assert np.all(got[:, g["sigma"] == 0.0] == 0.0)
        for t in range(T):
            a, b = out["keep_ptr"][task + t], out["keep_ptr"][task + t + 1]
            rx0, rx1, tdoa = coverage_ref.synth(g["table"], centre_of(g, c), receivers, g["ref_noise"][c, t])
            assert np.all(np.abs(out["keep_tdoa"][a:b] - tdoa) <= G.tdoa_bound(g["sigma"], rx0, rx1, tdoa)), (c, t)
            # and exactly the statement's expression on the device's own noise
            own = coverage_ref.synth(g["table"], centre_of(g, c), receivers, got[t])[2]
            assert out["keep_tdoa"][a:b].tobytes() == own.tobytes(), (c, t)
    print("%s: largest noise difference / bound: %.3g" % (name, worst))


@pytest.mark.parametrize("name", G.SETS)
def test_every_kept_trial_is_thr_pos_to_the_bit(name):
    g, _, out = run(name)
    want = _native.pos(out["keep_ptr"], out["keep_rx0"], out["keep_rx1"], out["keep_tdoa"], np.ones(len(out["keep_tdoa"])),
                       g["table"], x0=tuple(g["x0"].tolist()), max_iter=100)
    assert len(out["keep_status"]) > 0
    assert out["keep_pos"].tobytes() == want["pos"].tobytes()
    assert out["keep_status"].tobytes() == want["status"].tobytes()
    assert out["keep_iters"].tobytes() == want["iters"].tobytes()


@pytest.mark.parametrize("name", G.SETS)
def test_the_reduction_follows_the_rule_on_the_devices_own_trials(name):
    """Counts, iters_sum, the LOSSY flag, q50 and q95 exactly; the means within (m - 1) 2^-53 sum|v| / m of the exact mean
    of the same float64 terms (coverage_golden.mean_bound)."""
    g, _, out = run(name)
    T, gross = int(g["trials"]), float(g["gross_m"])
    for c, _, task in kept_cells(g):
        pos, status, err = out["keep_pos"][task:task + T], out["keep_status"][task:task + T], out["keep_err"][task:task + T]
        px, py = centre_of(g, c)
        dx, dy = pos[:, 0] - px, pos[:, 1] - py
        want_err = np.array([coverage_ref.error_of(p, s, (px, py))[2] for p, s in zip(pos, status)])
        assert err.tobytes() == want_err.tobytes(), c
        counts, iters_sum, stats, lossy = coverage_ref.reduce_cell(dx, dy, err, status, out["keep_iters"][task:task + T], gross)
        np.testing.assert_array_equal(out["counts"][c], counts)
        assert out["iters_sum"][c] == iters_sum and bool(out["flags"][c] & 4) == lossy
        assert out["stats"][c, 6:].tobytes() == stats[6:].tobytes(), c
        good = (status == OK) & (err <= gross)
        if not good.any():
            assert np.all(np.isnan(out["stats"][c, :6]))
            continue
        for k, v in enumerate((dx, dy, dx * dx, dx * dy, dy * dy)):
            assert abs(out["stats"][c, k] - G.exact_mean(v[good])) <= G.mean_bound(v[good]), (c, k)
        assert out["stats"][c, 5] == np.sqrt(out["stats"][c, 2] + out["stats"][c, 4])
        assert out["stats"][c, :6].tobytes() == stats[:6].tobytes(), c       # the stated order, restated: the same bits
    uncovered = np.flatnonzero(g["ref_n_heard"] < 3)
    assert np.all(np.isnan(out["stats"][uncovered])) and np.all(np.isnan(out["pred"][uncovered]))
    assert not out["counts"][uncovered].any() and not out["iters_sum"][uncovered].any()


@pytest.mark.parametrize("name", G.SETS)
def test_analytic_columns_are_within_the_forward_bound(name):
    """Against the same formulas in np.longdouble, within the bound tests/test_coverage_host.py validates."""
    g, _, out = run(name)
    n_rx, checked = len(g["table"]), 0
    for c in np.flatnonzero((g["ref_flags"] & 3) == 0).tolist():
        receivers = [r for r in range(n_rx) if (int(g["ref_heard_mask"][c]) >> r) & 1]
        exact = coverage_ref.analytic(g["table"], g["sigma"], centre_of(g, c), receivers, dtype=np.longdouble)
        bound = G.pred_bound(g["ref_pred"][c], float(g["ref_cond"][c]), len(receivers) * (len(receivers) - 1) // 2, n_rx)
        diff = np.abs(out["pred"][c].astype(np.longdouble) - np.array(exact[:5]))
        assert np.all(diff <= bound), (c, diff, bound)
        checked += 1
    assert checked > 0


@pytest.mark.parametrize("name", G.SETS)
def test_the_whole_map_against_the_statement_where_its_margin_allows(name):
    g, _, out = run(name)
    covered, safe = g["ref_n_heard"] >= 3, g["safe"]
    assert np.count_nonzero(covered & ~safe) <= 0.05 * np.count_nonzero(covered)
    rows = covered & safe
    np.testing.assert_array_equal(out["counts"][rows, 4:], g["ref_counts"][rows, 4:])
    np.testing.assert_array_equal(out["flags"][rows], g["ref_flags"][rows])
    np.testing.assert_array_equal(out["flags"][~covered], g["ref_flags"][~covered])
    assert np.all(out["counts"][covered, :4].sum(axis=1) == int(g["trials"]))


def test_the_fixed_start_loses_cells_far_from_the_origin_and_a_start_at_the_array_does_not():
    g = G.load("far4")
    rx_pos = {10 + 3 * k: xy for k, xy in enumerate(g["table"])}
    options = dict(area=tuple(g["lo"].tolist()) + tuple(g["hi"].tolist()), grid=(int(g["nx"]), int(g["ny"])),
                   trials=int(g["trials"]), seed=int(g["seed"]))
    fixed = coverage.coverage_map(rx_pos, 0.3, float(g["gross_m"]), **options)
    assert fixed.shape == (6, 6) and np.any(fixed.flags & coverage.LOSSY)
    np.testing.assert_array_equal(fixed.flags.ravel()[g["safe"]], g["ref_flags"][g["safe"]])
    centred = coverage.coverage_map(rx_pos, 0.3, float(g["gross_m"]), x0=tuple(g["x0_centre"].tolist()), **options)
    assert not np.any(centred.flags & coverage.LOSSY)
    np.testing.assert_array_equal(centred.n_good.ravel()[g["safe_centre"]], g["ref_counts_centre"][g["safe_centre"], 4])
    assert "lossy" in fixed.format_summary() and len(fixed.format_raster("gross").splitlines()) == 7
    cell = fixed.cell(2, 3)
    assert cell["n_heard"] == 4 and cell["x"] == fixed.cx[2] and cell["y"] == fixed.cy[3] and cell["n_good"] == fixed.n_good[3, 2]


def test_without_noise_one_trial_per_cell_is_the_convergence_map():
    g = G.load("ring5")
    counts, out = G.native_call(g, sigma=np.zeros(5), trials=1, keep_first=0, keep_count=30)
    assert counts["tasks"] == 30 and np.all(out["keep_status"] == OK) and np.all(out["keep_noise"] == 0.0)
    assert np.all(out["keep_err"] <= float(g["pos_tolerance"])), out["keep_err"].max()
    assert out["stats"][:, 6].tobytes() == out["keep_err"].tobytes() == out["stats"][:, 7].tobytes()
    assert np.all(out["pred"][:, 1:] == 0.0) and np.all(out["counts"][:, 4] == 1)


def test_a_repeated_call_gives_the_same_bytes_and_each_seed_word_changes_the_noise():
    g, _, out = run("mixed5")
    again = G.native_call(g, keep_first=0, keep_count=6)[1]
    for key in _native.COVERAGE_OUTPUTS:
        assert again[key].tobytes() == out[key].tobytes(), key
    seed = int(g["seed"])
    for other in (seed ^ 1, seed ^ (1 << 32)):
        noise = G.native_call(g, seed=other, keep_first=0, keep_count=6, outputs=("keep_noise",))[1]["keep_noise"]
        moved = noise != out["keep_noise"]
        assert np.all(moved[:, g["sigma"] > 0]) and not np.any(moved[:, g["sigma"] == 0])
