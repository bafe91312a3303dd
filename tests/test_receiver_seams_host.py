"""The scenes of tests/receiver_scenes.py are what they claim, by the NumPy references alone, and the checks that
tests/test_gpu_receiver_seams.py applies to the device raise on outputs doctored the way a 32-bit receiver mask would
leave them: a receiver count over the low word only (or the high word only), a candidate list without its receivers
from 32 on, a hearing mask without its high word and the pair rows decoded from it.  No GPU."""
import numpy as np
import pytest

import coverage_ref
import receiver_scenes as S
from pos_ref import OK, UNDERDETERMINED
from tdoa_models_ref import tdoa_models_ref
from tdoa_ref import tdoa_ref

TABLE = S.table65()[:64]
MODES = (None, S.KNOWN_HEIGHT, S.FREE_Z)        # thr_pos; thr_pos3 with the height known and with z free


def mask_of(receivers):
    return sum(1 << r for r in receivers)


def planted(mode):
    return S.planted_reference(mode)


def late_reference(name, late, seed, mode, weighted=False):
    scene = S.late_case(name, late, seed, mode)
    return scene, S.late_reference(scene, mode, weighted)


# ---------------------------------------------------------------- (a) the scenes are what they claim
def test_every_named_set_holds_the_bits_its_name_says():
    low, high = (1 << 32) - 1, ((1 << 32) - 1) << 32
    m = {name: mask_of(rx) for name, rx in S.SETS.items()}
    count = lambda v: bin(v).count("1")     # noqa: E731
    assert m["LOW3"] & high == 0 and count(m["LOW3"]) == 3
    assert m["HIGH3"] & low == 0 and count(m["HIGH3"]) == 3 and m["HIGH3"] >> 63 == 1 and (m["HIGH3"] >> 32) & 1
    assert m["STRADDLE"] == 0b111 << 31
    assert (count(m["SPLIT12"] & low), count(m["SPLIT12"] & high)) == (1, 2)
    assert (count(m["SPLIT21"] & low), count(m["SPLIT21"] & high)) == (2, 1)
    assert m["HIGH2"] & low == 0 and count(m["HIGH2"]) == 2
    assert m["TOP"] == ((1 << 10) - 1) << 54 and m["ACROSS"] == ((1 << 10) - 1) << 27
    assert (count(m["ACROSS"] & low), count(m["ACROSS"] & high)) == (5, 5)
    assert m["ENDS"] == 0b11 | (0b11 << 31) | (0b11 << 62)
    assert m["ALL"] == (1 << 64) - 1
    # with z free: four receivers, fewer than four in either half alone (but for the sets of one half)
    for name in ("LOW3", "HIGH3", "STRADDLE", "SPLIT12", "SPLIT21"):
        rx = S.SETS_FREE_Z[name]
        assert len(rx) == 4 and set(S.SETS[name]) < set(rx)
        halves = (len([r for r in rx if r < 32]), len([r for r in rx if r >= 32]))
        assert halves in ((4, 0), (0, 4)) or max(halves) < 4
    scene = S.planted_groups(S.SETS, TABLE[:, :2])
    assert np.diff(scene["group_ptr"]).tolist() == [3, 3, 3, 3, 3, 1, 45, 45, 15, 2016]
    assert scene["rx0"].max() == 62 and scene["rx1"].max() == 63 and np.all(scene["rx0"] < scene["rx1"])
    assert S.table65().shape == (65, 3)


@pytest.mark.parametrize("mode", MODES)
def test_the_references_solve_every_solvable_group_at_the_planted_point(mode):
    scene, want = planted(mode)
    tol = S.tolerances(mode)[0]
    axes = 2 if mode is None else 3
    for k, name in enumerate(scene["names"]):
        if name == "HIGH2":
            assert want["status"][k] == UNDERDETERMINED
            continue
        assert want["status"][k] == OK, name
        assert np.max(np.abs(want["pos"][k] - S.MOBILE[:axes])) <= tol, (name, want["pos"][k])
    S.assert_solves_equal(want, want, scene["names"], *S.tolerances(mode), dop_keys=S.dop_keys(mode))     # the check takes its own reference


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,late,seed", S.late_cases())
def test_the_references_exclude_the_late_receiver_with_a_margin(name, late, seed, mode):
    scene, out = late_reference(name, late, seed, mode)
    assert np.all(out["flags"] == 3)                     # INCONSISTENT | EXCLUDED
    assert np.all(out["rms"][:, 0] > 3.0) and np.all(out["rms"][:, 1] <= 0.5 * out["rms"][:, 0])
    S.assert_candidate_list(out, scene)
    assert S.late_margin(out, scene) > 3.0
    if name == "ALL":
        assert len(out["task_rx"]) == 3 * 64 and np.all(out["counts"][:, 1] == 2016 - 63)


def test_the_weighted_scene_excludes_the_late_receiver_too():
    for mode in MODES:
        scene, out = late_reference("ENDS", 63, 100, mode, weighted=True)
        S.assert_candidate_list(out, scene)
        assert S.late_margin(out, scene) > 3.0


def test_the_coverage_raster_holds_the_four_kinds_of_cells():
    a = S.coverage_scene(64)
    assert a["nx"] * a["ny"] <= 12 and 3 <= a["trials"] <= 5
    cx, cy = coverage_ref.cell_centres(a["lo"], a["hi"], a["nx"], a["ny"])
    heard = coverage_ref.hearing(a["table"], cx, cy, a["range_m"])
    sets = [set(np.flatnonzero(row).tolist()) for row in heard]
    assert any(len(s) >= 3 and min(s) >= 32 for s in sets)                       # only the high word
    assert any(len(s) >= 3 and {31, 32, 63} <= s for s in sets)                  # across the words, up to the top bit
    assert {31, 32, 63} in sets                                                  # ... with bit 63 the last one left
    assert any(len(s) >= 3 and max(s) <= 31 for s in sets)                       # only the low word
    assert any(len(s) < 3 for s in sets)
    cells = S.coverage_cells(a)
    assert set(cells["flags"].tolist()) == {0, coverage_ref.UNCOVERED}           # no covered cell is DEGENERATE
    # 33 receivers: bit 32 is the table's last; without a range every cell hears every receiver
    assert S.coverage_table(33).shape == (33, 2) and np.array_equal(S.coverage_table(33), a["table"][:33])
    for n_rx in (33, 64):
        everyone = S.coverage_cells(S.coverage_scene(n_rx, range_m=0.0))
        assert np.all(everyone["heard_mask"] == np.uint64((1 << n_rx) - 1)) and not everyone["flags"].any()
        assert len(coverage_ref.pairs(everyone["receivers"][0])[0]) == n_rx * (n_rx - 1) // 2
    # no cluster is collinear: the rank of each centred cluster is 2
    table = a["table"]
    for part in (table[:31], table[31:34], table[34:]):
        assert np.linalg.matrix_rank(part - part.mean(axis=0), tol=1.0) == 2


@pytest.mark.parametrize("model", ["poly", "nearest"])
def test_the_1024_receiver_tdoa_scene_has_no_failure(model):
    scene = S.tdoa_scene()
    cols = scene.cols()
    args = (cols["rxid"], cols["txid"], cols["timestamp"], cols["soa"], cols["energy"], cols["noise"], scene.matches, 8.0,
            S.TDOA_BEACON_POS, S.TDOA_RX_POS, S.FS)
    want = tdoa_ref(*args) if model == "poly" else tdoa_models_ref(*(args + (model,)))
    assert len(S.TDOA_RX_POS) == 1024 and sorted(S.TDOA_RX_POS) == list(range(1024))
    assert want["failures"] == [] and [len(g[3]) for g in want["groups"]] == [28, 28, 1, 1]
    assert min(want["n_kept"]) >= 3
    assert [row[:2] for row in want["groups"][2][3]] == [(0, 1023)] and [row[:2] for row in want["groups"][3][3]] == [(1022, 1023)]
    assert [row[:2] for row in want["groups"][1][3]][0] == (1022, 1023)         # the descending match: the lower receiver first
    rx, dist = S.tdoa_native_args(scene)[0], S.tdoa_native_args(scene)[8]
    assert rx.max() == 1023 and dist.shape == (1024, 2) and S.tdoa_native_args(scene, 1025)[8].shape == (1025, 2)


def test_the_postdetect_table_puts_the_hearing_receivers_on_0_31_32_and_63():
    ids = S.POST_IDS[:64]
    assert list(ids) == sorted(set(ids)) and ids[-1] - ids[0] > 63
    assert [ids.index(rx) for rx in S.POST_HEARING] == [0, 31, 32, 63]


# ---------------------------------------------------------------- (b) the checks discriminate
@pytest.mark.parametrize("mode", MODES)
def test_a_receiver_count_over_one_word_fails_the_status_check(mode):
    scene, want = planted(mode)
    names, needed = scene["names"], 4 if mode == S.FREE_Z else 3
    tol = S.tolerances(mode)
    lost = {"low": S.low_half_statuses(scene, want["status"], needed), "high": S.high_half_statuses(scene, want["status"], needed)}
    under = {half: {n for n, s in zip(names, st) if s == UNDERDETERMINED} for half, st in lost.items()}
    # the five small sets tell the slips apart: each half alone loses its own set and every mixed one
    assert under["low"] >= {"HIGH3", "STRADDLE", "SPLIT12", "SPLIT21", "HIGH2", "TOP"} and "LOW3" not in under["low"]
    assert under["high"] >= {"LOW3", "STRADDLE", "SPLIT12", "SPLIT21", "HIGH2"} and "HIGH3" not in under["high"]
    for status in lost.values():
        with pytest.raises(AssertionError):
            S.assert_solves_equal(dict(want, status=status), want, names, *tol)
    # a receiver counted in both words: HIGH2 would pass for three receivers
    double = np.array(want["status"])
    double[names.index("HIGH2")] = OK
    with pytest.raises(AssertionError):
        S.assert_solves_equal(dict(want, status=double), want, names, *tol)


@pytest.mark.parametrize("name,late,seed", [case for case in S.late_cases() if case[0] != "ALL" or case[1] == 32])
def test_a_candidate_list_without_the_high_receivers_fails_the_list_check(name, late, seed):
    scene, out = late_reference(name, late, seed, None)
    doctored = S.without_high_candidates(out)
    assert len(doctored["task_rx"]) == 3 * len([r for r in S.SETS[name] if r < 32]) < len(out["task_rx"])
    with pytest.raises(AssertionError):
        S.assert_candidate_list(doctored, scene)
    # a list that is complete but whose choice is a low receiver fails too
    wrong = dict(out, counts=out["counts"].copy())
    wrong["counts"][:, 2] = min(S.SETS[name])
    with pytest.raises(AssertionError):
        S.assert_candidate_list(wrong, scene)


@pytest.mark.parametrize("n_rx,range_m", [(64, 130.0), (64, 0.0), (33, 0.0)])
def test_a_hearing_mask_without_its_high_word_fails_the_cell_check(n_rx, range_m):
    a = S.coverage_scene(n_rx, range_m)
    cells = S.coverage_cells(a)
    S.assert_cells_and_rows(S.statement_rows(cells, a["trials"]), cells, a["trials"])       # the statement passes its own check
    doctored = S.low_word_cells(cells, a["trials"])
    with pytest.raises(AssertionError):
        S.assert_cells_and_rows(doctored, cells, a["trials"])
    # each part of the check alone: the mask, the count, and the rows decoded from the low word
    good = S.statement_rows(cells, a["trials"])
    for key in ("heard_mask", "n_heard", "keep_rx1", "keep_ptr"):
        with pytest.raises(AssertionError):
            S.assert_cells_and_rows(dict(good, **{key: doctored[key]}), cells, a["trials"])
