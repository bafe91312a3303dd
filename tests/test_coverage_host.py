"""The coverage map, the part that needs no GPU: the generator against its known answers, the uniforms' range, the float64
analytic columns against np.longdouble within a derived bound, the prediction against the statement's own trials
(chi-square), the fixtures, the Python interface's refusals, the .npz round trip, the raster text and the plumbing
(header, export list, build lists, the hash)."""
import json
import os
import re

import numpy as np
import pytest

import coverage_golden as G
import coverage_ref
from thrifty_amd import _native, build, coverage

ROOT = G.ROOT


def words(values):
    return " ".join("%08x" % int(v) for v in values)


def test_philox_known_answers():
    philox = lambda counter, key: words(coverage_ref.philox4x32_10(np.array(counter, dtype=np.uint64), key))     # noqa: E731
    assert philox([0, 0, 0, 0], (0, 0)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert philox([0xFFFFFFFF] * 4, (0xFFFFFFFF, 0xFFFFFFFF)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert philox([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], (0xA4093822, 0x299F31D0)) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    batch = coverage_ref.philox4x32_10(np.array([[0, 0, 0, 0], [0xFFFFFFFF] * 4], dtype=np.uint64), (0, 0))
    assert words(batch[0]) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8" and batch.shape == (2, 4)


def test_the_uniforms_keep_the_logarithm_away_from_zero():
    u1, u2 = coverage_ref.uniforms(np.arange(40), 64, 6, seed=99)
    assert u1.min() > 0.0 and u1.max() <= 1.0 and u2.min() >= 0.0 and u2.max() < 1.0
    # the extreme words: w0 = 2^32 - 1 gives u1 = 1 (log 0 = 0, a zero normal), w0 = 0 gives 2^-32 (the largest normal)
    assert (float(0xFFFFFFFF) + 1.0) * 2.0 ** -32 == 1.0 and (0.0 + 1.0) * 2.0 ** -32 == 2.0 ** -32
    assert np.isclose(np.sqrt(-2.0 * np.log(2.0 ** -32)), G.R_MAX, rtol=1e-15)
    n = coverage_ref.noise(np.arange(40), 64, np.array([1.0, 0.0, 2.0]), seed=5)
    assert np.all(np.isfinite(n)) and np.all(n[..., 1] == 0.0) and np.all(np.abs(n[..., 0]) <= G.R_MAX)
    assert abs(n[..., 0].mean()) < 0.1 and abs(n[..., 0].std() - 1.0) < 0.05 and abs(n[..., 2].std() - 2.0) < 0.1
    # another cell, trial, receiver or seed word: another normal
    a = coverage_ref.noise([3], 4, np.ones(3), seed=1)[0]
    assert len(set(a.ravel().tolist())) == 12
    assert np.all(coverage_ref.noise([3], 4, np.ones(3), seed=1 + (1 << 32))[0] != a) and np.all(coverage_ref.noise([4], 4, np.ones(3), seed=1)[0] != a)


@pytest.mark.parametrize("name", G.SETS)
def test_pred_within_the_forward_bound(name):
    """The float64 statement of dop and Cov = inv(N) M inv(N) against the same formulas in np.longdouble (64-bit
    mantissa: its own error is 2^-11 of the float64 one).  The bound, with u = 2^-53, m rows, h hearing receivers:

    * a unit vector e_r = (rx_r - p) / |rx_r - p| carries 4u per component (a subtraction, the rounded sum of two rounded
      squares, a correctly rounded root, a division); g = e_a - e_b at most 10u absolute (|g| <= 2);
    * an entry of N = sum g g' is m products of 44u absolute each and m - 1 additions of u sum|terms| <= u tr N / 2 each:
      |dN| <= u (44 m + (m - 1) tr N) <= u (88 m / tr N + 2 (m - 1)) lambda_max(N) =: eps_N lambda_max (lambda_max >= tr N / 2);
    * u_r is a sum of h - 1 differences and M = sum sigma_r^2 u_r u_r' has n_rx terms at most: the same count gives
      eps_M of the order (2 h + n_rx + 20) u relative to tr M, as long as |u_r| is of the order h (it is h e_r - sum e_b);
    * Cov' - Cov = -inv(N) dN Cov - Cov dN inv(N) + inv(N) dM inv(N) to first order, so |dCov| <= (2 eps_N cond(N) + eps_M c) |Cov|
      in norm, c = |inv(N)|^2 |M| / |Cov| <= cond(N) when M and N share their principal axes (they do up to the sigmas'
      spread: M = 2 sigma^2 N for independent pairs); the closed form (three divisions by one determinant, two 2 x 2
      products) adds some 30 u cond(N).
    With tr N of the order m, eps_N <= (2 m + 88) u; twice that, eps_M and the closed form's 30 u stay below
    k u = (4 (m + n_rx) + 200) u, to be multiplied by cond(N).  The covariance entries are bounded in NORM, |value| = sxx + syy; dop = sqrt(tr inv(N)) and rms = sqrt(tr Cov) carry half
    the relative error of their squares.  This test holds the statement to k 2^-53 cond(N) |value| on every covered,
    non-degenerate fixture cell and prints how much of the bound is used."""
    g = G.load(name)
    n_rx, used, checked = len(g["table"]), 0.0, 0
    for c in np.flatnonzero((g["ref_flags"] & 3) == 0).tolist():
        receivers = [r for r in range(n_rx) if (int(g["ref_heard_mask"][c]) >> r) & 1]
        p = (g["ref_cx"][c % int(g["nx"])], g["ref_cy"][c // int(g["nx"])])
        double = coverage_ref.analytic(g["table"], g["sigma"], p, receivers)
        exact = coverage_ref.analytic(g["table"], g["sigma"], p, receivers, dtype=np.longdouble)
        assert np.array(double[:5]).tobytes() == g["ref_pred"][c].tobytes() and 1.0 <= double[5] < 1e8
        assert np.isclose(double[5], float(exact[5]), rtol=1e-6)
        bound = G.pred_bound(double[:5], double[5], len(receivers) * (len(receivers) - 1) // 2, n_rx)
        diff = np.abs(np.array(double[:5], dtype=np.longdouble) - np.array(exact[:5]))
        assert np.all(diff <= bound), (c, diff, bound)
        used, checked = max(used, float(np.max(diff / bound))), checked + 1
    assert checked > 0 and np.finfo(np.longdouble).nmant >= 63
    print("%s: %d cells, largest |float64 - longdouble| / bound: %.3g" % (name, checked, used))


def pooled_chi_square(g, cov_of):
    """sum over the good trials of e' inv(Cov) e / (2 n) and n, Cov per cell from cov_of(cell) -> (sxx, sxy, syy)."""
    total, n = 0.0, 0
    for c in range(len(g["ref_flags"])):
        sxx, sxy, syy = cov_of(c)
        good = (g["ref_trial_status"][c] == 0) & (g["ref_trial_err"][c] <= float(g["gross_m"]))
        dx, dy = g["ref_trial_dx"][c][good], g["ref_trial_dy"][c][good]
        det = sxx * syy - sxy * sxy
        total += float(np.sum((syy * dx * dx - 2.0 * sxy * dx * dy + sxx * dy * dy) / det))
        n += int(good.sum())
    return total / (2.0 * n), n


def test_the_prediction_describes_the_trials_and_independent_pair_noise_does_not():
    """ring5: sigma = 0.05 m on a ring of 100 m, cells inside it, 2100 pooled trials of the statement.  With the right
    covariance sum e' inv(Cov) e is chi-square with 2 n degrees of freedom: mean 2 n, standard deviation 2 sqrt(n), so
    the pooled ratio lies within 6 / sqrt(n) of 1 (six standard deviations are 2 / sqrt(n) * 3; the first-order
    covariance is exact to (sigma / 100 m)^2).  The seed is fixed.  A prediction from independent pair noise, M = 2
    sigma^2 N, i.e. Cov = 2 sigma^2 inv(N), understates the covariance by about h / 2 (on a ring sum e_r is small, u_r is
    about h e_r and M about h sigma^2 N) and must fail the same test."""
    g = G.load("ring5")
    assert np.all(g["sigma"] == 0.05) and int(g["trials"]) * len(g["ref_flags"]) == 2100
    ratio, n = pooled_chi_square(g, lambda c: g["ref_pred"][c, 1:4])
    assert n >= 2000 and abs(ratio - 1.0) <= 6.0 / np.sqrt(n), (ratio, n)
    receivers = list(range(5))

    def independent(c):
        p = (g["ref_cx"][c % int(g["nx"])], g["ref_cy"][c // int(g["nx"])])
        return coverage_ref.analytic(g["table"], g["sigma"], p, receivers, independent=True)[1:4]
    wrong, _ = pooled_chi_square(g, independent)
    assert abs(wrong - 1.0) > 6.0 / np.sqrt(n), wrong
    print("pooled chi-square / (2 n): %.4f with the estimator's covariance, %.4f with independent pairs (n = %d)" % (ratio, wrong, n))
    # and the simulated rms is the predicted one, cell by cell, within the spread of 70 trials
    assert np.all(np.abs(g["ref_stats"][:, 5] / g["ref_pred"][:, 4] - 1.0) < 0.35)


def test_the_statement_reproduces_the_fixtures_and_they_hold_what_they_are_for():
    for name in G.SETS:
        g = G.load(name)
        assert os.path.getsize(os.path.join(G.GOLDEN, name + ".npz")) < 256 * 1024
        covered = g["ref_n_heard"] >= 3
        assert np.count_nonzero(covered & ~g["safe"]) <= 0.05 * np.count_nonzero(covered)
        assert 1e-8 < float(g["pos_tolerance"]) == G.pos_tolerance() < 1e-6
    g = G.load("mixed5")
    ref = coverage_ref.coverage_ref(**G.arguments(g))
    for key in ("cx", "cy", "n_heard", "heard_mask", "flags", "noise", "counts"):
        assert ref[key].tobytes() == g["ref_" + key].tobytes(), key
    np.testing.assert_allclose(ref["stats"], g["ref_stats"], rtol=1e-9)          # NumPy's sums may differ between builds
    assert {0, 2, 3, 4, 6} <= set(G.load("range6")["ref_n_heard"].tolist())
    far = G.load("far4")
    assert np.any(far["ref_flags"] & 4) and not np.any(far["ref_flags_centre"] & 4)
    assert np.linalg.norm(far["table"].mean(axis=0) - (5000.0, -3000.0)) < 20.0


def test_the_reduction_rule_on_small_cases():
    assert [coverage_ref.rank_indices(t) for t in (1, 2, 19, 20, 21, 100, 4096)] == [
        (0, 0), (0, 1), (9, 18), (9, 18), (10, 19), (49, 94), (2047, 3891)]
    for t in (1, 3, 19, 20, 21, 64, 100, 255, 4096):
        assert coverage_ref.rank_indices(t) == (int(np.ceil(t / 2)) - 1, -(-95 * t // 100) - 1)
    err = np.array([0.5, np.inf, 0.25, 3.0])
    counts, iters, stats, lossy = coverage_ref.reduce_cell([0.5, np.nan, 0.0, 3.0], [0.0, np.nan, 0.25, 0.0], err, [0, 4, 0, 0],
                                                           [3, 0, 5, 7], gross_m=1.0)
    assert counts.tolist() == [3, 0, 0, 1, 2, 2] and iters == 15 and not lossy
    assert stats.tolist() == [0.25, 0.125, 0.125, 0.0, 0.03125, np.sqrt(0.15625), 0.5, np.inf]
    counts, _, stats, lossy = coverage_ref.reduce_cell([9.0], [0.0], [9.0], [0], [1], gross_m=1.0)
    assert counts.tolist() == [1, 0, 0, 0, 0, 1] and lossy and np.all(np.isnan(stats[:6])) and stats[6] == stats[7] == 9.0
    values = np.random.default_rng(0).normal(size=200)
    assert abs(coverage_ref.lane_sum(values) - G.exact_mean(values) * 200) <= 199 * G.U * np.abs(values).sum()


RX = {7: (0.0, 0.0), 3: (100.0, 0.0), 9: (0.0, 80.0), 4: (90.0, 95.0)}


@pytest.mark.parametrize("changes,sentence", [
    (dict(rx_pos={}), "rx_pos is empty"), (dict(rx_pos={1: (0.0, 1.0, 2.0)}), "2 dimensions"),
    (dict(rx_pos={1: (0.0, np.nan), 2: (1.0, 1.0)}), "not finite"), (dict(rx_pos={k: (k, 1.0) for k in range(65)}), "at most 64"),
    (dict(sigma_m=-1.0), "sigma_m"), (dict(sigma_m={7: 0.1, 3: 0.1, 9: 0.1}), "one entry per receiver"), (dict(sigma_m=np.inf), "sigma_m"),
    (dict(gross_m=0.0), "gross_m"), (dict(gross_m=np.nan), "gross_m"),
    (dict(area=(0.0, 0.0, 0.0, 5.0)), "lo < hi"), (dict(area=(0.0, 0.0, 5.0)), "area holds"),
    (dict(area=(-20000.0, 0.0, 5.0, 5.0)), "solver's box"), (dict(margin_m=-1.0), "margin_m"), (dict(margin_m=20e3), "solver's box"),
    (dict(grid=(0, 4)), "grid"), (dict(grid=(2048, 1024)), "grid"), (dict(grid=(2.5, 4)), "grid"),
    (dict(trials=0), "trials"), (dict(trials=4097), "trials"), (dict(grid=(1024, 1024), trials=4096), "cells x trials"),
    (dict(range_m=np.inf), "range_m"), (dict(seed=-1), "seed"), (dict(seed=1 << 64), "seed"),
    (dict(x0=(0.0, np.inf)), "x0"), (dict(max_iter=-1), "max_iter"), (dict(keep=(0, 65)), "keep"), (dict(keep=(4090, 10)), "keep"),
])
def test_argument_errors_that_need_no_device(changes, sentence):
    arguments = dict(rx_pos=RX, sigma_m=0.3, gross_m=5.0)
    arguments.update(changes)
    with pytest.raises(ValueError, match=sentence):
        coverage.coverage_map(**arguments)
    with pytest.raises(TypeError):
        coverage.coverage_map(RX)               # sigma_m and gross_m have no default


def fixture_map(name):
    """A CoverageMap from a fixture's statement outputs (no device)."""
    g = G.load(name)
    ny, nx = int(g["ny"]), int(g["nx"])
    arrays = {key: g["ref_" + key].reshape(ny, nx) for key in ("n_heard", "heard_mask", "flags", "iters_sum")}
    for table, names in (("pred", _native.COVERAGE_PRED), ("counts", _native.COVERAGE_CELL_COUNTS), ("stats", _native.COVERAGE_STATS)):
        arrays.update({key: np.ascontiguousarray(g["ref_" + table][:, k]).reshape(ny, nx) for k, key in enumerate(names)})
    params = dict(lo=g["lo"], hi=g["hi"], gross_m=float(g["gross_m"]), range_m=float(g["range_m"]), trials=int(g["trials"]),
                  seed=int(g["seed"]), x0=g["x0"], max_iter=100)
    return g, coverage.CoverageMap(arrays, g["ref_cx"], g["ref_cy"], list(range(len(g["table"]))), g["table"], g["sigma"], params)


def test_npz_round_trip_cell_and_summary(tmp_path):
    g, result = fixture_map("range6")
    assert result.shape == (8, 9) and result.rms.shape == (8, 9) and result.dop.dtype == np.float64
    result.save(str(tmp_path / "c.npz"))
    again = coverage.CoverageMap.load(str(tmp_path / "c.npz"))
    assert sorted(again.arrays) == sorted(result.arrays) and len(result.arrays) == 23
    for key, value in result.arrays.items():
        assert again.arrays[key].tobytes() == value.tobytes() and again.arrays[key].dtype == value.dtype, key
    assert again.cx.tobytes() == result.cx.tobytes() and again.params["trials"] == 8 and again.params["seed"] == 7
    assert again.rx_ids == list(range(6)) and again.sigma.tolist() == [0.3] * 6
    j, i = np.argwhere(result.n_heard == 6)[0]
    cell = result.cell(i, j)
    assert cell["n_heard"] == 6 and cell["x"] == g["ref_cx"][i] and cell["y"] == g["ref_cy"][j] and cell["rms"] == result.rms[j, i]
    assert cell["n_good"] + cell["n_gross"] == 8 and cell["heard_mask"] == 63
    text = result.format_summary()
    assert text.startswith("72 cells, 10 covered, 0 degenerate, 3 lossy; rms median ") and text.endswith("\n")
    assert re.search(r"worst \d+\.\d{3} m; median rms / pred_rms \d+\.\d{3}\n$", text)
    with pytest.raises(AttributeError):
        result.nothing


def test_raster_text():
    g, result = fixture_map("range6")
    text = result.format_raster("pred_rms")
    lines = text.splitlines()
    assert len(lines) == 9 and all(len(line) == 9 for line in lines[:8])
    covered = (result.flags & coverage.UNCOVERED) == 0
    for j in range(8):                        # the top line is the largest y
        assert [ch != " " for ch in lines[7 - j]] == covered[j].tolist()
    used = set("".join(lines[:8])) - {" "}
    assert used <= set(coverage.LADDER) and coverage.LADDER[0] in used and coverage.LADDER[-1] in used
    values = result.pred_rms[covered]
    assert lines[8] == "pred_rms: '.' = %.6g .. '@' = %.6g (' ' uncovered, '?' no value)" % (values.min(), values.max())
    j, i = np.unravel_index(np.nanargmax(np.where(covered, result.pred_rms, np.nan)), covered.shape)
    assert lines[7 - j][i] == "@"
    assert result.format_raster("gross").splitlines()[8].startswith("gross: '.' = 0 .. '@' = ")
    for name in coverage.RASTERS:
        assert len(result.format_raster(name).splitlines()) == 9
    with pytest.raises(ValueError, match="raster must be one of"):
        result.format_raster("snr")
    lossy = fixture_map("far4")[1]
    assert "@" in lossy.format_raster("gross") and ("?" in lossy.format_raster("rms")) == bool(np.any(lossy.n_good == 0))


def test_command_line_parsing(tmp_path):
    cfg = tmp_path / "pos-rx.cfg"
    cfg.write_text("0: 0.0 0.0\n1: 100.0 0.0\n2: 0.0 100.0\n")
    p = coverage._parser()
    a = p.parse_args(["-r", str(cfg), "--sigma", "0.5", "--gross", "10"])
    a.rx_pos.close()
    assert a.sigma_m == 0.5 and a.gross_m == 10.0 and a.sigma_rx == [] and a.area is None and tuple(a.grid) == (64, 64)
    assert a.margin_m is None and a.range_m is None and a.trials == 256 and a.seed == 0 and a.output is None and a.raster is None
    a = p.parse_args(["-r", str(cfg), "--sigma", "1", "--gross", "5", "--sigma-rx", "2=0.25", "--sigma-rx", "0=3", "--area", "0", "1", "2", "3",
                      "--grid", "8", "4", "--margin", "7", "--range", "50", "--trials", "16", "--seed", "9", "-o", "c.npz", "--raster", "q95"])
    a.rx_pos.close()
    assert a.sigma_rx == [(2, 0.25), (0, 3.0)] and a.area == [0.0, 1.0, 2.0, 3.0] and a.grid == [8, 4] and a.margin_m == 7.0
    assert a.range_m == 50.0 and a.trials == 16 and a.seed == 9 and a.output == "c.npz" and a.raster == "q95"
    for bad in (["--gross", "5"], ["--sigma", "1"], ["--sigma", "1", "--gross", "5", "--raster", "snr"],
                ["--sigma", "1", "--gross", "5", "--sigma-rx", "x"]):
        with pytest.raises(SystemExit):
            p.parse_args(["-r", str(cfg)] + bad)
    assert coverage._main(["-r", str(cfg), "--sigma", "1", "--gross", "5", "--sigma-rx", "8=1"]) == 1       # an unknown receiver
    assert coverage._main(["-r", str(cfg), "--sigma", "1", "--gross", "0"]) == 1                           # refused before the device


def test_thr_coverage_is_declared_listed_and_built():
    header = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
    assert "#define THR_ABI_VERSION 11" in header and _native.ABI_VERSION == 11
    assert re.search(r"\+ thr_coverage / thr_coverage_fetch / thr_coverage_free / thr_debug_coverage_times", header)
    assert header.index("within 11, a pure addition") < header.index("+ thr_coverage /") < header.index("#define THR_ABI_VERSION")
    assert re.search(r"\bint thr_coverage\(int device_id, int n_rx,", header)
    for name in ("thr_coverage", "thr_coverage_fetch", "thr_coverage_free", "thr_debug_coverage_times"):
        assert name in _native.EXPORTS and re.search(r"\b%s\(" % name, header), name
    for name, (which, _, _) in _native.COVERAGE_OUTPUTS.items():
        assert re.search(r"#define THR_COV_%s %d\b" % (name.upper(), which), header), name
    assert re.search(r"#define THR_COV_N_OUTPUTS %d\b" % len(_native.COVERAGE_OUTPUTS), header)
    for name, value in (("UNCOVERED", coverage.UNCOVERED), ("DEGENERATE", coverage.DEGENERATE), ("LOSSY", coverage.LOSSY),
                        ("MAX_TRIALS", _native.COVERAGE_MAX_TRIALS), ("MAX_KEEP", _native.COVERAGE_MAX_KEEP)):
        assert re.search(r"#define THR_COV_%s %d\b" % (name, value), header), name
    assert re.search(r"#define THR_COV_SLAB_BYTES \(512u << 20\)", header) and _native.COVERAGE_SLAB_BYTES == 512 << 20
    fields = re.search(r"typedef struct thr_coverage_counts \{(.*?)\} thr_coverage_counts;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S).replace("size_t", "")
    assert tuple(w.strip() for w in fields.strip(" ;\n").split(",")) == _native.COVERAGE_COUNTS
    assert _native.ThrCoverageOpts.lo.offset == 0 and _native.ThrCoverageOpts.nx.offset == 32
    assert _native.ThrCoverageOpts.range_m.offset == 48 and _native.ThrCoverageOpts.seed_lo.offset == 80
    assert _native.ThrCoverageOpts.slab_groups.offset == 88 and _native.ThrCoverageOpts.keep_count.offset == 100
    if os.path.exists(_native.LIB_PATH):
        lib = _native.load_library()
        assert lib.thr_coverage and lib.thr_coverage_fetch and lib.thr_debug_coverage_times


def test_build_lists_and_no_atomics():
    assert "coverage.hip" in build.SOURCES and build.UNPROFILED_COVERAGE == ("coverage.hip",)
    assert build.PER_FILE_FLAGS["coverage.hip"] == ["-ffp-contract=off"] == build.PER_FILE_FLAGS["posg.hip"]
    source = open(os.path.join(build.CSRC, "coverage.hip")).read()
    assert "#pragma clang fp contract(off)" in source and '#include "post_stages.hpp"' in source and "thr::pos_core(" in source
    assert "atomic" not in source.replace("no atomic:", "")
    for constant in ("0xD2511F53u", "0xCD9E8D57u", "0x9E3779B9u", "0xBB67AE85u", "6.283185307179586"):
        assert constant in source, constant


def test_csrc_hash_does_not_see_the_new_file(monkeypatch):
    before = build.csrc_hash()
    monkeypatch.setattr(build, "UNPROFILED_COVERAGE", ())
    assert build.csrc_hash() != before                  # it does see it once the list is emptied
    monkeypatch.undo()
    assert build.csrc_hash() == before
    with open(os.path.join(ROOT, "profiles", "hbm_traffic.json")) as f:
        recorded = json.load(f)
    assert before in json.dumps(recorded)               # the recorded hash still holds
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "coverage.hip"])
    assert build.csrc_hash() == before                  # and is the one of a tree without the file
