"""Receiver numbers at bits 31, 32 and 63 of the 64-bit receiver mask, across the position stages, and 1023 of
`thr_tdoa`'s 1024 (tests/receiver_scenes.py holds the scenes and the checks; tests/test_receiver_seams_host.py shows
that the checks raise on what a 32-bit mask would leave).

1. `thr_pos`, `thr_pos3` (both modes): one group per named set, status exactly and position / dops within the fixtures'
   tolerances of tests/pos_ref.py / pos3_ref.py; `thr_posg`, `thr_posg3`: every task byte for byte `thr_pos` / `thr_pos3`.
2. `thr_posq`, `thr_posq3` (both modes): the candidate list of groups whose late receiver is 31, 32 or 63 -- the list
   itself, every candidate byte for byte `thr_pos` / `thr_pos3` on the group rebuilt without that receiver, the choice
   by the rule on the device's own rms; 64 candidates per group for the full table.
3. `thr_coverage` at 33 and 64 receivers, with and without a hearing range: everything tests/test_gpu_coverage.py holds
   its fixtures to.
4. `thr_tdoa` with a table of 1024 receivers: tests/test_gpu_tdoa_seams.py's check, both entry points' models.
5. `thr_postdetect` with a 64-entry table whose hearing receivers are the dense indices 0, 31, 32 and 63.

No tolerance is this file's own: each is imported, or copied with its source named."""
import numpy as np
import pytest

import coverage_golden
import coverage_ref
import posg3_golden
import posg3_ref
import posg_golden
import posg_ref
import posq3_golden
import posq_golden
import postdetect_scene
import receiver_scenes as S
from pos_ref import OK, UNDERDETERMINED
from tdoa_models_ref import tdoa_models_ref
from tdoa_ref import tdoa_ref
from thrifty_amd import _native, kitchen_sink, tdoa_est

pytestmark = pytest.mark.gpu

TABLE65 = S.table65()
TABLE = TABLE65[:64]
MODES = (None, S.KNOWN_HEIGHT, S.FREE_Z)        # thr_pos / thr_posq; thr_pos3 / thr_posq3 with the height known and with z free


def cols_of(scene):
    return scene["group_ptr"], scene["rx0"], scene["rx1"], scene["tdoa"], scene["snr"]


def same_bytes(got, want, keys=None):
    for key in (want if keys is None else keys):
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key


# ---------------------------------------------------------------- 1. thr_pos, thr_pos3, thr_posg, thr_posg3
def solve(scene, mode, table=None):
    if mode is None:
        return _native.pos(*cols_of(scene), TABLE[:, :2] if table is None else table)
    return _native.pos3(*cols_of(scene), TABLE if table is None else table, mode, scene["group_h"], x0=S.START3)


@pytest.mark.parametrize("mode", MODES)
def test_groups_on_either_side_of_bit_32_have_their_status_and_position(mode):
    scene, want = S.planted_reference(mode)
    out = solve(scene, mode)
    print(dict(zip(scene["names"], out["status"].tolist())), "iters", out["iters"].tolist())
    S.assert_solves_equal(out, want, scene["names"], *S.tolerances(mode), dop_keys=S.dop_keys(mode))
    np.testing.assert_array_equal(out["iters"][scene["names"].index("HIGH2")], 0)
    with pytest.raises(ValueError, match="1 to 64 receivers, not 65"):
        solve(scene, mode, TABLE65[:, :2] if mode is None else TABLE65)


def test_thr_posg_solves_the_same_groups_from_every_start():
    scene, _ = S.planted_reference(None)
    table = scene["table"]
    margin = posg_golden.margin_of(table)
    flat = solve(scene, None)
    counts, out = _native.posg(*cols_of(scene), table, margin)
    cx, cy = posg_ref.centres(table, margin, 32)
    assert counts["groups"] == len(scene["names"])
    assert out["task_status"][:, 0].tobytes() == flat["status"].tobytes()               # the fixed start is thr_pos
    posg_golden.assert_tasks_equal_thr_pos(out, *cols_of(scene), table, cx, cy)
    under = {name for name, st in zip(scene["names"], out["task_status"][:, 0]) if st == UNDERDETERMINED}
    assert under == {"HIGH2"}
    assert np.all(out["status"][[k for k, name in enumerate(scene["names"]) if name != "HIGH2"]] != UNDERDETERMINED)


@pytest.mark.parametrize("mode", [S.KNOWN_HEIGHT, S.FREE_Z])
def test_thr_posg3_solves_the_same_groups_from_every_start(mode):
    scene, _ = S.planted_reference(mode)
    margin = posg_golden.margin_of(TABLE[:, :2])
    free_z = mode == S.FREE_Z
    kw = dict(z_grid=posg3_golden.default_z_grid(TABLE)) if free_z else dict(grid_z=1, group_h=scene["group_h"])
    flat = solve(scene, mode)
    counts, out = _native.posg3(*cols_of(scene), TABLE, mode, margin, x0=S.START3, **kw)
    out["cx"], out["cy"], out["cz"] = posg3_ref.centres(TABLE, margin, 32, kw.get("z_grid"), 8 if free_z else 1)
    assert counts["groups"] == len(scene["names"])
    assert out["task_status"][:, 0].tobytes() == flat["status"].tobytes()               # the fixed start is thr_pos3
    posg3_golden.assert_tasks_equal_thr_pos3(out, *cols_of(scene), TABLE, mode, scene["group_h"], S.START3)
    under = {name for name, st in zip(scene["names"], out["task_status"][:, 0]) if st == UNDERDETERMINED}
    assert under == {"HIGH2"}
    assert np.all(out["status"][[k for k, name in enumerate(scene["names"]) if name != "HIGH2"]] != UNDERDETERMINED)


# ---------------------------------------------------------------- 2. thr_posq, thr_posq3
def quality(scene, mode, **kw):
    if mode is None:
        return _native.posq(*cols_of(scene), scene["table"], **kw)
    return _native.posq3(*cols_of(scene), scene["table"], mode, scene["group_h"] if mode == S.KNOWN_HEIGHT else None, x0=S.START3, **kw)


def min_rx_of(mode):
    return _native.POSQ_MIN_RX if mode is None else _native.POSQ3_MIN_RX[1 if mode == S.FREE_Z else 0]


def check_candidates(scene, mode, **kw):
    """The gated call -> (counts, outputs): the candidates against thr_pos / thr_pos3 on the rebuilt groups (to the
    bit) and the choice against the rule on the device's own rms (the helpers of tests/posq_golden.py, posq3_golden.py)."""
    counts, out = quality(scene, mode, gate_m=S.GATE_M, **kw)
    min_rx = kw.get("min_rx", min_rx_of(mode))
    if mode is None:
        n = posq_golden.assert_candidates_equal_thr_pos(out, *cols_of(scene), scene["table"])
        posq_golden.assert_choice_follows_the_rule(out, scene["group_ptr"], scene["rx0"], scene["rx1"], S.GATE_M, 0.5, min_rx)
    else:
        n = posq3_golden.assert_candidates_equal_thr_pos3(out, *cols_of(scene), scene["table"], mode,
                                                          scene["group_h"] if mode == S.KNOWN_HEIGHT else None, S.START3)
        posq3_golden.assert_choice_follows_the_rule(out, scene["group_ptr"], scene["rx0"], scene["rx1"], S.GATE_M, 0.5, min_rx)
    assert n == counts["tasks"]
    return counts, out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,late,seed", S.late_cases())
def test_the_candidate_list_names_every_receiver_of_the_set(name, late, seed, mode):
    scene = S.late_case(name, late, seed, mode)
    size = len(S.SETS[name])
    # without the gate: counts[:, 0] is the receiver count of the full solve, the mask's population
    _, plain = quality(scene, mode)
    np.testing.assert_array_equal(plain["counts"][:, 0], size)
    np.testing.assert_array_equal(plain["counts"][:, 2], -1)
    counts, out = check_candidates(scene, mode)
    assert counts["flagged"] == 3 and counts["tasks"] == 3 * size
    S.assert_candidate_list(out, scene)          # task_ptr, task_rx, counts[:, 2], counts[:, 0] == size - 1, used
    assert np.all(out["flags"] == _native.POSQ_INCONSISTENT | _native.POSQ_EXCLUDED)
    rows = size * (size - 1) // 2
    np.testing.assert_array_equal(out["counts"][:, 1], rows - (size - 1))
    np.testing.assert_array_equal(out["task_nrx"], size - 1)
    again = quality(scene, mode, gate_m=S.GATE_M)
    assert again[0] == counts
    same_bytes(again[1], out)


@pytest.mark.parametrize("mode", MODES)
def test_sixty_four_candidates_and_the_limits_of_min_rx_and_of_the_table(mode):
    scene = S.late_case("ALL", 32, 100, mode)
    counts, out = check_candidates(scene, mode, min_rx=64)          # 64 receivers are still enough to flag
    assert counts["flagged"] == 3 and counts["tasks"] == 192 and counts["rows"] == 3 * 2016
    S.assert_candidate_list(out, scene)
    np.testing.assert_array_equal(out["counts"][:, 1], 1953)        # every candidate walks 1953 used rows of 2016
    with pytest.raises(ValueError, match="min_rx must lie in"):
        quality(scene, mode, gate_m=S.GATE_M, min_rx=65)
    wide = dict(scene, table=TABLE65[:, :2] if mode is None else TABLE65)
    with pytest.raises(ValueError, match="1 to 64 receivers, not 65"):
        quality(wide, mode, gate_m=S.GATE_M)


@pytest.mark.parametrize("mode", MODES)
def test_the_weighted_solves_list_and_choose_the_same_way(mode):
    scene = S.late_case("ENDS", 63, 100, mode)
    counts, out = quality(scene, mode, gate_m=S.GATE_M, row_weight=scene["snr"])
    assert counts["flagged"] == 3 and counts["tasks"] == 18
    S.assert_candidate_list(out, scene)
    rule = posq_golden if mode is None else posq3_golden
    rule.assert_choice_follows_the_rule(out, scene["group_ptr"], scene["rx0"], scene["rx1"], S.GATE_M, 0.5, min_rx_of(mode))
    _, plain = quality(scene, mode, gate_m=S.GATE_M)
    assert out["task_pos"].tobytes() != plain["task_pos"].tobytes()          # the weights were read
    same_bytes(quality(scene, mode, gate_m=S.GATE_M, row_weight=scene["snr"])[1], out)


# ---------------------------------------------------------------- 3. thr_coverage
COVERAGE_CASES = [(64, 130.0), (64, 0.0), (33, 130.0), (33, 0.0)]
_maps = {}


def coverage_run(n_rx, range_m):
    """(arguments, the statement's cells, counts, outputs) of one device call that keeps every cell -- once per case."""
    if (n_rx, range_m) not in _maps:
        a = S.coverage_scene(n_rx, range_m, trials=5 if range_m else 3)
        _maps[n_rx, range_m] = (a, S.coverage_cells(a)) + coverage_call(a)
    return _maps[n_rx, range_m]


def coverage_call(a, **changes):
    a = dict(a, keep_first=0, keep_count=a["nx"] * a["ny"], **changes)
    return _native.coverage(a.pop("table"), a.pop("sigma"), a.pop("lo"), a.pop("hi"), a.pop("nx"), a.pop("ny"), a.pop("gross_m"), **a)


def kept(a, cells):
    """[(cell, receivers, first kept task, centre)] of the covered cells."""
    out, task = [], 0
    for c, receivers in enumerate(cells["receivers"]):
        if len(receivers) >= 3:
            out.append((c, receivers, task, (float(cells["cx"][c % a["nx"]]), float(cells["cy"][c // a["nx"]]))))
            task += a["trials"]
    return out


@pytest.mark.parametrize("n_rx,range_m", COVERAGE_CASES)
def test_coverage_cells_hearing_and_rows(n_rx, range_m):
    a, cells, counts, out = coverage_run(n_rx, range_m)
    T, covered = a["trials"], cells["n_heard"] >= 3
    S.assert_cells_and_rows(out, cells, T)
    assert out["cx"].tobytes() == cells["cx"].tobytes() and out["cy"].tobytes() == cells["cy"].tobytes()
    assert counts["cells"] == 12 and counts["covered"] == covered.sum() and counts["tasks"] == covered.sum() * T
    assert counts["keep_tasks"] == covered.sum() * T and counts["n_rx"] == n_rx
    assert counts["keep_rows"] == len(out["keep_rx0"]) == counts["rows"] == sum(int(h) * (int(h) - 1) // 2 for h in cells["n_heard"][covered]) * T
    if range_m == 0.0:
        assert np.all(out["heard_mask"] == np.uint64((1 << n_rx) - 1)) and np.all(np.diff(out["keep_ptr"]) == n_rx * (n_rx - 1) // 2)
    elif n_rx == 64:
        assert {31, 32, 63} in [set(S.receivers_of_mask(m)) for m in out["heard_mask"]]


@pytest.mark.parametrize("n_rx,range_m", COVERAGE_CASES)
def test_coverage_noise_and_tdoas(n_rx, range_m):
    """tests/test_gpu_coverage.py: test_noise_and_tdoas_are_within_their_derived_bounds -- the noise within
    coverage_golden.noise_bound of the statement's (the third counter word is the receiver number), the tdoas byte for
    byte the statement's expression on the device's own noise."""
    a, cells, _, out = coverage_run(n_rx, range_m)
    T, bound = a["trials"], coverage_golden.noise_bound(a["sigma"])
    cells_kept = kept(a, cells)
    want = coverage_ref.noise([c for c, _, _, _ in cells_kept], T, a["sigma"], a["seed"])
    assert out["keep_noise"].shape == (len(cells_kept) * T, n_rx)
    for k, (c, receivers, task, centre) in enumerate(cells_kept):
        got = out["keep_noise"][task:task + T]
        assert np.all(np.abs(got - want[k]) <= bound), c
        assert np.all(got != 0.0)
        for t in range(T):
            lo, hi = out["keep_ptr"][task + t], out["keep_ptr"][task + t + 1]
            rx0, rx1, tdoa = coverage_ref.synth(a["table"], centre, receivers, want[k, t])
            assert np.all(np.abs(out["keep_tdoa"][lo:hi] - tdoa) <= coverage_golden.tdoa_bound(a["sigma"], rx0, rx1, tdoa)), (c, t)
            own = coverage_ref.synth(a["table"], centre, receivers, got[t])[2]
            assert out["keep_tdoa"][lo:hi].tobytes() == own.tobytes(), (c, t)


@pytest.mark.parametrize("n_rx,range_m", COVERAGE_CASES)
def test_coverage_trials_are_thr_pos_and_the_reduction_follows_the_rule(n_rx, range_m):
    """tests/test_gpu_coverage.py: test_every_kept_trial_is_thr_pos_to_the_bit and
    test_the_reduction_follows_the_rule_on_the_devices_own_trials."""
    a, cells, _, out = coverage_run(n_rx, range_m)
    T, gross = a["trials"], a["gross_m"]
    want = _native.pos(out["keep_ptr"], out["keep_rx0"], out["keep_rx1"], out["keep_tdoa"], np.ones(len(out["keep_tdoa"])), a["table"],
                       x0=a["x0"], max_iter=100)
    assert len(out["keep_status"]) > 0
    same_bytes({"pos": out["keep_pos"], "status": out["keep_status"], "iters": out["keep_iters"]}, want, ("pos", "status", "iters"))
    for c, _, task, (px, py) in kept(a, cells):
        pos, status, err = out["keep_pos"][task:task + T], out["keep_status"][task:task + T], out["keep_err"][task:task + T]
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
        # the means: the statement's bits (its order of additions is the device's).  That file's looser check against
        # the exact mean is left out: its bound has no term for the division, which shows with three to five trials
        assert out["stats"][c, :6].tobytes() == stats[:6].tobytes(), c
    uncovered = np.flatnonzero(cells["n_heard"] < 3)
    assert np.all(np.isnan(out["stats"][uncovered])) and np.all(np.isnan(out["pred"][uncovered]))
    assert not out["counts"][uncovered].any() and not out["iters_sum"][uncovered].any()


@pytest.mark.parametrize("n_rx,range_m", COVERAGE_CASES)
def test_coverage_analytic_columns(n_rx, range_m):
    """tests/test_gpu_coverage.py: test_analytic_columns_are_within_the_forward_bound -- against the same formulas in
    np.longdouble, within coverage_golden.pred_bound."""
    a, cells, _, out = coverage_run(n_rx, range_m)
    checked = 0
    for c, receivers, _, centre in kept(a, cells):
        exact = coverage_ref.analytic(a["table"], a["sigma"], centre, receivers, dtype=np.longdouble)
        bound = coverage_golden.pred_bound(cells["pred"][c], float(cells["cond"][c]), len(receivers) * (len(receivers) - 1) // 2, n_rx)
        diff = np.abs(out["pred"][c].astype(np.longdouble) - np.array(exact[:5]))
        assert np.all(diff <= bound), (c, diff, bound)
        checked += 1
    assert checked > 0


@pytest.mark.parametrize("n_rx,range_m", [(64, 130.0), (64, 0.0)])
def test_coverage_slabs_give_the_bytes_of_one_slab(n_rx, range_m):
    a, _, counts, out = coverage_run(n_rx, range_m)
    assert counts["slabs"] == 1
    for slab_groups in (1, a["trials"] + 1):
        more, again = coverage_call(a, slab_groups=slab_groups)
        assert more["slabs"] == -(-counts["tasks"] // slab_groups)
        same_bytes(again, out, _native.COVERAGE_OUTPUTS)


def test_coverage_refuses_sixty_five_receivers():
    a = S.coverage_scene(64)
    table = np.concatenate([a["table"], [[0.0, 200.0]]])
    with pytest.raises(ValueError, match="1 to 64 receivers, not 65"):
        coverage_call(dict(a, table=table, sigma=np.full(65, 0.1)))


# ---------------------------------------------------------------- 4. thr_tdoa
@pytest.mark.parametrize("model", ["poly", "nearest"])
def test_tdoa_with_a_table_of_1024_receivers(model):
    """tests/test_gpu_tdoa_seams.py: check(), on thr_tdoa_model's own columns (the dense index IS the receiver number
    here): discrete outputs exact; `tdoa` of the polynomial within that file's derived bound 16 cond^2 2^-52 spread / fs,
    of the nearest pair the statement's bits (tests/test_gpu_tdoa_models.py); snr relative 1e-14, model_quality 1e-12."""
    scene = S.tdoa_scene()
    cols = scene.cols()
    ref_args = (cols["rxid"], cols["txid"], cols["timestamp"], cols["soa"], cols["energy"], cols["noise"], scene.matches, 8.0,
                S.TDOA_BEACON_POS, S.TDOA_RX_POS, S.FS)
    want = tdoa_ref(*ref_args) if model == "poly" else tdoa_models_ref(*(ref_args + (model,)))
    args = S.tdoa_native_args(scene)
    assert args[8].shape == (1024, 2)
    got = _native.tdoa(*args, deg=2, model=_native.TDOA_MODELS[model])
    assert got["n_window"].tolist() == want["n_window"]
    assert got["n_kept"].tolist() == want["n_kept"]
    assert [tuple(p) for p in got["failures"].tolist()] == want["failures"] == []
    assert got["group_id"].tolist() == [g[0] for g in want["groups"]]
    assert got["group_ptr"].tolist() == np.cumsum([0] + [len(g[3]) for g in want["groups"]]).tolist() == [0, 28, 56, 57, 58]
    rows = [row for g in want["groups"] for row in g[3]]
    assert got["row_rx"][:, 0].tolist() == [row[0] for row in rows] and got["row_rx"][:, 1].tolist() == [row[1] for row in rows]
    assert got["row_det"][:, 0].tolist() == [row[5] for row in rows] and got["row_det"][:, 1].tolist() == [row[6] for row in rows]
    assert got["row_rx"].max() == 1023 and [tuple(p) for p in got["row_rx"][56:].tolist()] == [(0, 1023), (1022, 1023)]
    ref_tdoa = np.array([row[2] for row in rows], dtype=float)
    if model == "poly":
        bound = np.array([16 * c * c * 2.0 ** -52 * s / S.FS for c, s in zip(want["cond"], want["spread"])])
        diff = np.abs(got["tdoa"] - ref_tdoa)
        print("max |tdoa - tdoa_ref| = %.3g s, bound %.3g s" % (diff.max(), bound.min()))
        assert len(bound) == len(rows) and np.all(diff <= bound)
        assert np.all(got["picks"] == -1)
        same_bytes(_native.tdoa(*args, deg=2, model=None), {k: v for k, v in got.items() if k != "picks"})     # thr_tdoa itself
    else:
        assert got["tdoa"].tobytes() == ref_tdoa.tobytes()
        assert [tuple(p) for p in got["picks"].tolist()] == want["picks"]
    np.testing.assert_allclose(got["snr"], [row[3] for row in rows], rtol=1e-14, atol=0)
    np.testing.assert_allclose(got["model_quality"], [row[4] for row in rows], rtol=1e-12, atol=0)
    # the public columns number the receivers of the matches densely: the same rows under the receivers' own numbers
    ptr, idx = args[5], args[6]
    public = tdoa_est.tdoa_columns(cols, ptr, idx, 8.0, S.TDOA_BEACON_POS, S.TDOA_RX_POS, S.FS, model=model)
    assert public["tdoas"]["rx0"].tolist() == got["row_rx"][:, 0].tolist() and public["tdoas"]["rx1"].tolist() == got["row_rx"][:, 1].tolist()
    assert public["tdoas"]["tdoa"].tobytes() == got["tdoa"].tobytes()


def test_tdoa_refuses_1025_receivers():
    args = S.tdoa_native_args(S.tdoa_scene(), n_rx=1025)
    for model in (None, _native.TDOA_MODELS["poly"]):
        with pytest.raises(ValueError, match="1 to 1024 receivers, not 1025"):
            _native.tdoa(*args, model=model)


# ---------------------------------------------------------------- 5. thr_postdetect
def test_postdetect_with_a_full_table_equals_the_staged_calls():
    st = postdetect_scene.settings(rx_ids=S.POST_HEARING)
    st = st._replace(rx_pos=S.post_rx_pos(st))
    assert len(st.rx_pos) == 64 and [sorted(st.rx_pos).index(rx) for rx in S.POST_HEARING] == [0, 31, 32, 63]
    cols = postdetect_scene.columns(100, rx_ids=S.POST_HEARING)
    got = kitchen_sink.postdetect_columns(cols, st)
    postdetect_scene.assert_identical(got, postdetect_scene.staged(cols, st))       # test_gpu_postdetect_seams.py: fused_is_staged
    rows = got["tdoas"]
    assert got["counts"]["groups"] > 0 and set(np.unique(rows["rx0"])) | set(np.unique(rows["rx1"])) == set(S.POST_HEARING)
    assert np.any(got["status"] == OK)
    # 65 entries: the library's own refusal
    with pytest.raises(ValueError, match="thr_postdetect: 1 to 64 receivers, not 65"):
        kitchen_sink.postdetect_columns(cols, st._replace(rx_pos=S.post_rx_pos(st, 65)))
