"""thr_reldist at its seams, on the smallest shapes that can go wrong (tests/reldist_scenes.py builds them; T is
the reductions' tile length, from reldist_geometry()).  Every scene is compared with the NumPy statement over all
rows of all cells (reldist_ref.assert_same: exact, but for mean and std within their rounding bounds and the smoothed
values within the measured SMOOTH_RTOL); each test then says what its scene is there for.

One shape of the issue cannot exist: "2 rows, one masked".  Two values lie equally far from their median, so
is_outlier masks both or neither.  `thresh_half` masks both (no kept row, no speed); `mad_zero` has the cell
that loses one row of five to the mask; a one-row cell has no speed either."""
import numpy as np
import pytest

import reldist_ref as R
import reldist_scenes as SC
from thrifty_amd import _native

pytestmark = pytest.mark.gpu

SEAMS = ("sizes_nearest", "sizes_linpol", "thresh_half", "nb_1", "nb_2", "outside_nearest", "outside_linpol", "mad_zero",
         "unsorted_frac_0", "unsorted_frac_0.25", "nan_row", "smooth_frac_1", "smooth_frac_0.5", "smooth_frac_0.025",
         "ties_frac_0.2", "ties_frac_0.25", "equal_abscissae_frac_0.2", "equal_abscissae_frac_0.25")


@pytest.fixture(scope="module")
def tile():
    return _native.reldist_geometry()[0]


@pytest.fixture(scope="module")
def runs(tile):
    """name -> (device result, statement's result), each computed once."""
    out = {}
    for name, (args, kwargs) in SC.seam_inputs(tile).items():
        out[name] = (_native.reldist(*args, **kwargs), R.reldist_ref(*args, **kwargs), kwargs)
    return out


def test_the_list_of_scenes_is_complete(runs):
    assert set(runs) == set(SEAMS)


@pytest.mark.parametrize("name", SEAMS)
def test_scene_equals_the_statement(runs, name):
    got, want, _ = runs[name]
    R.assert_same(got, want, what=name)


def test_cell_sizes_around_the_tile(runs, tile):
    for method in ("nearest", "linpol"):
        out = runs["sizes_" + method][0][1]
        assert np.diff(out["cell_ptr"]).tolist() == [tile - 1, tile + 1, 1, 2, 3, tile, 2 * tile + 1]
        assert out["cell_ptr"][1] == tile - 1 and out["cell_ptr"][2] // tile == out["cell_ptr"][5] // tile       # three cells, one tile
        assert out["cell_counts"][2].tolist()[:3] == [1, 40, 1] and np.diff(out["speed_ptr"])[2] == 0          # one row: no speed
        assert not out["cell_flags"].any() and np.all(np.isfinite(out["cell_stats"]))


def test_both_rows_masked_leaves_nothing(runs):
    out = runs["thresh_half"][0][1]
    assert out["mask1"][:2].tolist() == [1, 1] and out["cell_counts"][0, 2] == 0 and np.diff(out["speed_ptr"])[0] == 0
    assert out["cell_stats"][0, 0] == 0 and np.isnan(out["cell_stats"][0, 1]) and np.isnan(out["medians"][0, 2])
    assert out["cell_stats"][0, 3] == np.inf and out["cell_stats"][0, 4] == -np.inf
    assert out["cell_counts"][2, 2] < 9 and np.isfinite(out["cell_stats"][2, 1])          # the other cells are untouched


def test_one_and_two_beacon_rows(runs):
    for nb in (1, 2):
        out = runs["nb_%d" % nb][0][1]
        assert np.all(out["cell_counts"][:, 1] == nb) and set(out["hi"].tolist()) <= set(range(nb + 1))
        assert np.all(out["nearest_idx"] < nb) and np.all(np.isfinite(out["raw"]))
        held = out["row_flags"] == R.ROW_HELD
        assert np.array_equal(held, (out["hi"] == 0) | (out["hi"] == nb)) and (nb == 2 or held.all())


def test_rows_outside_the_beacons_span(runs):
    for method in ("nearest", "linpol"):
        out = runs["outside_" + method][0][1]
        assert np.diff(out["cell_ptr"]).tolist() == [6, 7]
        assert out["hi"].tolist() == [0] * 6 + [5] * 7 and out["nearest_idx"].tolist() == [0] * 6 + [4] * 7
        assert out["row_flags"].tolist() == ([R.ROW_HELD] * 13 if method == "linpol" else [0] * 13)
        assert np.all(np.isfinite(out["x"]))


def test_mad_of_zero_follows_numpy(runs):
    out = runs["mad_zero"][0][1]
    assert out["x"].tolist() == [5.0, 5.0, 5.0, 5.0, 37.0] and out["medians"][0, :2].tolist() == [5.0, 0.0]
    assert out["mask1"].tolist() == [0, 0, 0, 0, 1] and out["cell_counts"][0, 2] == 4 and len(out["speed"]) == 3
    assert out["speed"].tolist() == [0.0] * 3 and not out["mask2"].any()


def test_unsorted_rows_are_flagged_not_searched(runs):
    for frac, flags in ((0.0, [R.CELL_UNSORTED, 0, R.CELL_UNSORTED, 0]), (0.25, [R.CELL_UNSORTED, 0, R.CELL_UNSORTED, R.CELL_UNSORTED])):
        out = runs["unsorted_frac_%g" % frac][0][1]
        assert out["cell_key"].tolist() == [[1, 0, 0, 1], [1, 5, 0, 1], [2, 0, 0, 1], [2, 5, 0, 1]]
        assert out["cell_flags"].tolist() == flags
        for ci, fl in enumerate(flags):
            a, b = out["cell_ptr"][ci:ci + 2]
            assert np.all(np.isnan(out["x"][a:b])) == bool(fl) and np.all(out["hi"][a:b] == -1) == bool(fl)
            assert np.all(np.isfinite(out["dop"][a:b])) == (not fl)


def test_a_nan_row_stays_in_its_cell(runs):
    out = runs["nan_row"][0][1]
    a, b = out["cell_ptr"][:2]
    assert np.count_nonzero(np.isnan(out["x"][a:b])) == 1 and np.isnan(out["x"][a + 7])
    assert np.all(np.isnan(out["medians"][0, :4])) and not out["mask1"][a:b].any()           # numpy: median of a NaN is NaN
    assert np.isnan(out["cell_stats"][0, 1:5]).all() and out["cell_stats"][0, 0] == b - a
    assert np.all(np.isfinite(out["medians"][1])) and np.all(np.isfinite(out["cell_stats"][1]))
    assert np.all(np.isfinite(out["speed_smooth"][out["speed_smooth_ptr"][1]:]))


def test_smoother_windows_around_a_wave(runs):
    lanes = _native.reldist_geometry()[2]
    assert lanes == 64
    lengths = [1, 2, 3, 4, 63, 64, 65, 66, 126, 127, 128, 129, 130, 131]
    for frac, ks in ((1.0, lengths), (0.5, [max(2, m // 2) for m in lengths]), (0.025, [max(2, int(0.025 * m + 1e-10)) for m in lengths])):
        out = runs["smooth_frac_%g" % frac][0][1]
        m = np.diff(out["dop_smooth_ptr"])
        assert not out["mask3"].any() and m.tolist() == lengths              # the doppler series ARE those lengths
        assert [R.window_len(int(v), frac) for v in m[1:]] == ks[1:]
        assert out["dop_smooth"][0] == out["dop"][0]                         # m = 1: the value itself
    assert {63, 64, 65} <= set(R.window_len(m, 0.5) for m in lengths) and {63, 64, 65} <= set(lengths)
    out = runs["smooth_frac_0.025"][0][1]
    a, b = out["dop_smooth_ptr"][4:6]
    assert np.array_equal(out["dop_smooth"][a:b], out["dop"][out["cell_ptr"][4]:out["cell_ptr"][5]])      # k = 2: the point itself
    out = runs["smooth_frac_0.5"][0][1]
    a, b = out["dop_smooth_ptr"][12:14]
    x = out["dop_smooth_x"][a:b]
    starts = [R.window_start(x, i, 65) for i in range(len(x))]
    assert starts[0] == 0 and starts[-1] == len(x) - 65 and len(set(starts)) > 20           # pinned at each end, moving between


def test_ties_and_equal_abscissae(runs):
    for frac in (0.2, 0.25):
        out = runs["ties_frac_%g" % frac][0][1]
        x = out["dop_smooth_x"][:out["dop_smooth_ptr"][1]]
        k = R.window_len(len(x), frac)
        tied = [i for i in range(len(x)) for L in [R.window_start(x, i, k)] if L + k < len(x) and x[L + k] - x[i] == x[i] - x[L]]
        assert k % 2 == 0 and len(tied) > 10, (frac, k)           # an even window over evenly spaced points: the lowest wins
        out = runs["equal_abscissae_frac_%g" % frac][0][1]
        for stem in ("speed", "dop"):
            for ci, xs, ys in R.series_of(out, stem):
                assert len(set(xs.tolist())) == 1 and len(xs) > 10
                k = R.window_len(len(xs), frac)
                y = R.kept_values(out, stem, ci)
                assert np.allclose(ys, np.mean(y[:k]), rtol=1e-13, atol=0)           # h = 0: the mean of the lowest window
