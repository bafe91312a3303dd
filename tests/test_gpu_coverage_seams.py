"""The seams of `thr_coverage`: trial counts around the lane stride of the sums and the power-of-two padding of the sort,
the rank indices where ceil(0.95 T) steps, grids of one row or one cell, slab sizes that cut cells (every output must
keep its bytes), a map without a covered cell, a cell whose every trial is NONFINITE, the keep range's limits, and every
argument error.  No input here makes the device fault: every refused one is refused on the host."""
import numpy as np
import pytest

import coverage_golden as G
import coverage_ref
from pos_ref import NONFINITE
from thrifty_amd import _native

pytestmark = pytest.mark.gpu
TABLE = G.ring(3, 5)
BASE = dict(sigma_rx=np.full(5, 0.05), lo=(-40.0, -35.0), hi=(40.0, 35.0), gross_m=1.0)


def call(nx=1, ny=1, table=TABLE, **changes):
    a = dict(BASE, **changes)
    return _native.coverage(table, a.pop("sigma_rx"), a.pop("lo"), a.pop("hi"), nx, ny, a.pop("gross_m"), **a)


def check_reduction(out, cells, T, gross_m, cx, cy):
    """The kept cells' rows of counts / stats against the rule on the device's own trials, to the bit."""
    for k, c in enumerate(cells):
        s = slice(k * T, (k + 1) * T)
        px, py = cx[c % len(cx)], cy[c // len(cx)]
        dx, dy = out["keep_pos"][s, 0] - px, out["keep_pos"][s, 1] - py
        counts, iters_sum, stats, lossy = coverage_ref.reduce_cell(dx, dy, out["keep_err"][s], out["keep_status"][s],
                                                                   out["keep_iters"][s], gross_m)
        np.testing.assert_array_equal(out["counts"][c], counts)
        assert out["stats"][c].tobytes() == stats.tobytes(), (c, out["stats"][c], stats)
        assert out["iters_sum"][c] == iters_sum and bool(out["flags"][c] & 4) == lossy


@pytest.mark.parametrize("T", [1, 2, 19, 20, 21, 63, 64, 65, 127, 128, 129, 4096])
def test_trial_counts_at_the_lane_stride_the_padding_and_the_rank_steps(T):
    counts, out = call(trials=T, seed=T, keep_count=1, gross_m=0.08)     # 0.08 m: some trials are gross
    assert counts["tasks"] == counts["keep_tasks"] == T and counts["cells"] == 1
    check_reduction(out, [0], T, 0.08, out["cx"], out["cy"])
    order = np.sort(out["keep_err"])
    i50, i95 = {1: (0, 0), 19: (9, 18), 20: (9, 18), 21: (10, 19)}.get(T, coverage_ref.rank_indices(T))
    assert out["stats"][0, 6] == order[i50] and out["stats"][0, 7] == order[i95]
    assert out["counts"][0, 4] + out["counts"][0, 5] == T and (T < 63 or 0 < out["counts"][0, 5] < T)


@pytest.mark.parametrize("nx,ny", [(1, 1), (7, 3), (1, 33)])
def test_grids_of_one_cell_one_row_and_odd_sizes(nx, ny):
    counts, out = call(nx, ny, trials=5, keep_count=nx * ny)
    cx, cy = coverage_ref.cell_centres(BASE["lo"], BASE["hi"], nx, ny)
    assert out["cx"].tobytes() == cx.tobytes() and out["cy"].tobytes() == cy.tobytes()
    assert counts["covered"] == nx * ny and np.all(out["n_heard"] == 5) and np.all(out["heard_mask"] == 31)
    check_reduction(out, range(nx * ny), 5, 1.0, cx, cy)
    want = _native.pos(out["keep_ptr"], out["keep_rx0"], out["keep_rx1"], out["keep_tdoa"], np.ones(len(out["keep_tdoa"])), TABLE)
    assert out["keep_pos"].tobytes() == want["pos"].tobytes() and out["keep_iters"].tobytes() == want["iters"].tobytes()


def test_slab_sizes_that_cut_cells_move_no_byte():
    g = G.load("range6")                    # first and last cells UNCOVERED, 10 covered cells among 72
    T = int(g["trials"])
    assert g["ref_n_heard"][0] < 3 and g["ref_n_heard"][-1] < 3
    whole_counts, whole = G.native_call(g, keep_first=8, keep_count=64)
    tasks = whole_counts["tasks"]
    assert whole_counts["slabs"] == 1 and tasks == 10 * T and whole_counts["slab_groups"] > tasks
    for groups in (1, T - 1, T, T + 1, 3 * T + 5):
        counts, out = G.native_call(g, keep_first=8, keep_count=64, slab_groups=groups)
        assert counts["slab_groups"] == groups and counts["slabs"] == -(-tasks // groups)       # no empty slab is run
        assert counts["slab_bytes"] < whole_counts["slab_bytes"]
        for key in _native.COVERAGE_OUTPUTS:
            assert out[key].tobytes() == whole[key].tobytes(), (groups, key)


def test_a_map_without_a_covered_cell_launches_no_solve():
    counts, out = call(4, 3, range_m=1.0, trials=7, keep_count=12)
    assert counts["covered"] == counts["tasks"] == counts["slabs"] == counts["rows"] == counts["keep_tasks"] == 0
    assert np.all(out["flags"] == 1) and np.all(out["n_heard"] == 0) and not out["counts"].any() and not out["iters_sum"].any()
    assert np.all(np.isnan(out["stats"])) and np.all(np.isnan(out["pred"]))
    assert out["keep_ptr"].tolist() == [0] and len(out["keep_pos"]) == 0 and _native.coverage_times()[3] == 0.0


def test_a_receiver_on_the_cell_centre_makes_every_trial_nonfinite():
    table = np.vstack([TABLE, [[8.0, 4.0]]])           # the centre of the one cell of (0, 0) .. (16, 8), exactly
    counts, out = call(table=table, sigma_rx=np.full(6, 0.05), lo=(0.0, 0.0), hi=(16.0, 8.0), trials=6, x0=(8.0, 4.0),
                       keep_count=1)
    assert out["cx"][0] == 8.0 and out["cy"][0] == 4.0 and counts["tasks"] == 6
    assert np.all(out["keep_status"] == NONFINITE) and np.all(np.isinf(out["keep_err"]))
    assert out["counts"][0].tolist() == [0, 0, 0, 6, 0, 6] and out["flags"][0] == 2 | 4 and out["pred"][0, 0] == -1.0
    assert np.all(np.isnan(out["stats"][0, :6])) and np.all(np.isinf(out["stats"][0, 6:])) and np.all(np.isnan(out["pred"][0, 1:]))


def test_keep_count_zero_and_the_most_ending_on_the_last_cell():
    kept_counts, kept = call(11, 6, trials=1, keep_first=2, keep_count=64)
    assert kept_counts["keep_tasks"] == 64 and kept_counts["keep_rows"] == 640 and kept["keep_noise"].shape == (64, 5)
    assert kept["stats"][2:, 6].tobytes() == kept["keep_err"].tobytes()
    counts, out = call(11, 6, trials=1)
    assert counts["keep_tasks"] == counts["keep_rows"] == 0 and out["keep_ptr"].tolist() == [0]
    for key, value in out.items():
        assert (len(value) == 0 or key == "keep_ptr") if key.startswith("keep_") else value.tobytes() == kept[key].tobytes(), key


@pytest.mark.parametrize("changes,sentence", [
    (dict(table=np.array([[0.0, 0.0], [np.nan, 1.0], [5.0, 5.0]]), sigma_rx=np.ones(3)), "coordinate 2 is not finite"),
    (dict(sigma_rx=np.array([0.1, 0.1, np.inf, 0.1, 0.1])), "sigma of receiver 2"),
    (dict(sigma_rx=np.array([0.1, -0.1, 0.1, 0.1, 0.1])), "sigma of receiver 1"),
    (dict(lo=(40.0, -35.0)), "lo < hi"), (dict(hi=(40.0, np.inf)), "corners must be finite"),
    (dict(nx=0), "nx and ny"), (dict(nx=1025, ny=1024), "nx and ny"), (dict(nx=1024, ny=1024, trials=4096), "cells x trials"),
    (dict(trials=0), "trials must lie in 1 .. 4096"), (dict(trials=4097), "trials must lie in 1 .. 4096"),
    (dict(gross_m=0.0), "gross_m"), (dict(gross_m=np.inf), "gross_m"), (dict(gross_m=np.nan), "gross_m"),
    (dict(range_m=np.nan), "range_m"), (dict(max_iter=-1), "max_iter"), (dict(slab_groups=-1), "slab_groups"),
    (dict(nx=4, ny=4, keep_first=10, keep_count=7), "keep range 10 \\+ 7 passes the 16 cells"),
    (dict(nx=9, ny=9, keep_count=65), "keep_count must lie in 0 .. 64"), (dict(keep_first=-1), "keep range"),
    (dict(x0=(np.nan, 0.0)), "x0 must be finite"),
    (dict(lo=(-20000.0, -35.0)), "inside the solver's box"), (dict(hi=(40.0, 10200.0)), "inside the solver's box"),
])
def test_argument_errors(changes, sentence):
    with pytest.raises(ValueError, match=sentence):
        call(**changes)


def test_the_area_may_reach_the_solvers_box_and_sigma_may_be_zero():
    lo, hi = TABLE.min(axis=0) - 10e3, TABLE.max(axis=0) + 10e3
    counts, out = call(2, 2, lo=tuple(lo), hi=tuple(hi), sigma_rx=np.zeros(5), trials=1)
    assert counts["tasks"] == 4 and np.all(out["pred"][:, 1:] == 0.0)
