"""What every post-detect entry point takes from the HIP runtime it gives back: thr_debug_live_resources (device buffers,
pinned buffers, streams, events) around a success, a held result handle, a host refusal, the two device_id refusals, the
refusals decided on the device and every early stop, for the calls of tests/post_contract_cases.py.  A repeated call
returns the same bytes and leaves its inputs alone.  Exact: bytes and counts, no tolerance."""
import gc

import numpy as np
import pytest

import post_contract_cases as P
import postdetect_scene
from thrifty_amd import _native, identify, kitchen_sink

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize("case", P.CASES, ids=repr)
FAMILIES = pytest.mark.parametrize("case", P.FAMILIES, ids=repr)


def baseline(case):
    """The count after one warm-up call of the same entry point (the runtime's own first-call state is not ours)."""
    case.run()
    gc.collect()
    return _native.live_resources()


def unchanged(before, what=""):
    gc.collect()
    now = _native.live_resources()
    assert now == before, "%s: %s" % (what, ", ".join("%s %d -> %d" % (k, a, b) for k, a, b in zip(P.KINDS, before, now) if a != b))


@CASES
def test_success_twice(case):
    before = baseline(case)
    snapshot = [a.tobytes() for a in case.inputs()]
    first = P.flatten(case.run())
    second = P.flatten(case.run())
    assert P.same_bytes(second, first) == []
    assert [a.tobytes() for a in case.inputs()] == snapshot and not any(a.flags.writeable for a in case.inputs())
    assert any(v.size for v in first.values())
    if case.times is not None:
        times = case.times()
        assert len(times) == case.n_times and all(t >= 0 for t in times) and sum(times) > 0
    del first, second
    unchanged(before, "two calls")


@FAMILIES
def test_a_held_handle(case):
    lib = _native.load_library()
    before = baseline(case)
    raw = P.raw_call(case)
    assert raw.rc == 0 and raw.handle.value
    held = _native.live_resources()
    assert held[0] > before[0], "a result that holds no device buffer"
    assert held[1] == before[1] and held[2] == before[2]
    assert held[3] == before[3] + P.RESULT_EVENTS
    free = getattr(lib, "thr_%s_free" % case.family.stem)
    free(None)                                  # a no-op
    assert _native.live_resources() == held
    raw.free()
    unchanged(before, "after the free")


@CASES
def test_the_host_refusal(case):
    before = baseline(case)
    r = case.refusal
    raw = P.raw_call(case, args=r.args, mutate=r.mutate, hold=False, **(r.kwargs or {}))
    assert raw.rc == _native.ERR_ARG, (raw.rc, raw.error)
    assert isinstance(raw.exception, ValueError) and r.match in str(raw.exception), repr(raw.exception)
    assert r.match in raw.error
    if case.family:
        assert raw.handle.value is None
    unchanged(before, "refusal")


@pytest.fixture(scope="module")
def device_count():
    import torch
    return torch.cuda.device_count()


@CASES
@pytest.mark.parametrize("where", ["below", "above"])
def test_a_device_that_does_not_exist(case, where, device_count):
    """Reached in pick_device, after every argument check has passed."""
    device_id = -1 if where == "below" else device_count
    assert device_count >= 1
    before = baseline(case)
    raw = P.raw_call(case, hold=False, device_id=device_id)
    assert raw.rc == _native.ERR_ARG, (raw.rc, raw.error)
    assert isinstance(raw.exception, ValueError) and "bad device_id %d" % device_id in str(raw.exception), repr(raw.exception)
    if case.family:
        assert raw.handle.value is None
    unchanged(before, "device_id %d" % device_id)


# ------------------------------------------------------------------ refusals decided on the device
W = _native.MATCH_WORKGROUP


def late_columns():
    """Two and a bit workgroups of detections in order."""
    return tuple(c.copy() for c in P.match_columns(n=2 * W + 37, seed=3))


@pytest.mark.parametrize("what", ["NaN", "earlier"])
def test_match_refuses_on_the_device_and_returns_everything(what):
    case = P.BY_NAME["match"]
    before = baseline(case)
    rx, tx, ts, en = late_columns()
    bad = W + 11                        # past the first workgroup
    ts[bad] = np.nan if what == "NaN" else ts[bad - 1] - 0.25
    with pytest.raises(ValueError) as err:
        _native.match(rx, tx, ts, en, 0.5)
    want = "thr_match: timestamps must be non-decreasing without NaN: detection %d is %s" % (
        bad, "NaN" if what == "NaN" else "earlier than the one before it")
    assert want in str(err.value)
    assert want in _native.load_library().thr_last_error().decode()
    unchanged(before, what)
    assert P.same_bytes(P.flatten(case.run()), P.flatten(case.run())) == []        # and the next call is a whole one


def test_postdetect_refuses_a_nan_among_the_kept_after_identify_has_run():
    case = P.BY_NAME["postdetect"]
    before = baseline(case)
    counts, out = case.run()
    assert counts["kept"] > 40
    cols = [c.copy() for c in case.args]
    victim = int(out["kept_order"][40])
    cols[2][victim] = np.nan
    raw = P.raw_call(case, args=tuple(cols), hold=False)
    assert raw.rc == _native.ERR_ARG and raw.handle.value is None
    assert isinstance(raw.exception, ValueError)
    # the refusal names the detection by its place among the kept, which thr_identify alone gives for the same columns
    rxid, block, ts, cbin, coff, _, energy, _ = cols
    _, keep, order = _native.identify(rxid, block, ts, cbin, coff, energy, identify._flatten(postdetect_scene.settings().tx_freqs))
    assert keep[victim] and list(order).count(victim) == 1
    place = list(order).index(victim)
    assert "thr_match: timestamps must be non-decreasing without NaN: detection %d is NaN" % place in raw.error
    assert all(getattr(raw.counts, name) == 0 for name in _native.POST_COUNTS)
    unchanged(before, "NaN among the kept")


# ------------------------------------------------------------------ early stops
@pytest.mark.parametrize("case,stop", P.stops_of(), ids=lambda v: v if isinstance(v, str) else repr(v))
def test_an_early_stop_gives_everything_back(case, stop):
    before = baseline(case)
    args, changes = P.stop_call(case, stop)
    if stop == "zero" and case.zero_refused:
        raw = P.raw_call(case, args=args, hold=False, **changes)
        assert raw.rc == _native.ERR_ARG and case.zero_refused in raw.error and isinstance(raw.exception, ValueError)
        assert raw.handle.value is None
        unchanged(before, stop)
        return
    snapshot = [a.tobytes() for a in case.inputs(args, changes)]
    first = P.flatten(case.run(args, **changes))
    assert P.same_bytes(P.flatten(case.run(args, **changes)), first) == []
    assert [a.tobytes() for a in case.inputs(args, changes)] == snapshot
    EXPECT[stop](case, first)
    if case.family:
        raw = P.raw_call(case, args=args, **changes)
        assert raw.rc == 0 and raw.handle.value
        fetched = P.fetch_all(case, raw, args)      # every size is what the shape table says for the counts, the empty ones too
        raw.free()
        assert P.same_bytes(fetched, {k: v for k, v in first.items() if k != "(counts)"}) == []
        if stop == "zero":
            assert getattr(raw.counts, raw.counts._fields_[0][0]) == 0
    del first
    unchanged(before, stop)


def counts_of(names, out):
    """The counts a wrapper returned, by name (P.flatten keeps them sorted by name)."""
    return dict(zip(sorted(names), out["(counts)"].astype(np.int64).tolist()))


def _zero(case, out):
    for name, v in out.items():
        if name == "(counts)":
            continue
        assert v.size <= 1 and not v.any(), (name, v)         # nothing, or the one zero of a CSR pointer


def _no_task(case, out):
    assert len(out["n_window"]) == 0 and len(out["tdoa"]) == 0 and out["group_ptr"].tolist() == [0] and len(out["failures"]) == 0


def _gate_0(case, out):
    c = counts_of(_native.POSQ_COUNTS, out)
    assert c["flagged"] == 0 and c["tasks"] == 0 and c["groups"] > 0
    assert not out["task_ptr"].any() and out["task_pos"].size == 0 and out["task_rx"].size == 0


def _tiny_gate(case, out):
    c = counts_of(_native.POSQ_COUNTS, out)
    assert c["flagged"] == c["groups"] > 0 and np.all(np.diff(out["task_ptr"]) > 0)
    assert out["task_pos"].shape[0] == out["task_ptr"][-1] == c["tasks"] > c["groups"]


def _post(**want):
    def check(case, out):
        c = counts_of(_native.POST_COUNTS, out)
        for key, positive in want.items():
            assert (c[key] > 0) == positive, (key, c)
        if c["groups"]:
            assert (out["status"] == _native.POS_UNDERDETERMINED).all()
        else:
            assert out["group_ptr"].tolist() == [0] and out["pos"].shape == (0, 2)
        if not c["matches"]:
            assert out["match_ptr"].tolist() == [0]
    return check


def _no_grid(case, out):
    assert (out["task_status"][:, 0] == _native.POS_UNDERDETERMINED).all() and (out["task_status"][:, 1:] == -1).all()
    assert not out["n_local"].any() and (out["start_cell"] == -1).all() and np.isnan(out["map"]).all() and not out["map_min"].any()


def _no_covered_cell(case, out):
    assert (out["flags"] & _native.COVERAGE_UNCOVERED).all() and not out["counts"].any()
    assert counts_of(_native.COVERAGE_COUNTS, out)["covered"] == 0


def _invalid(case, out):
    assert not out["used"].any() and len(out["used"]) == len(case.args[0])


EXPECT = {
    "zero": _zero, "no_task": _no_task, "gate_0": _gate_0, "tiny_gate": _tiny_gate,
    "nothing_kept": _post(kept=False, matches=False), "all_misses": _post(kept=True, matches=False, misses=True, tasks=False),
    "beacon_matches_only": _post(matches=True, tasks=False, groups=False),
    "every_group_underdetermined": lambda case, out: (_post(groups=True) if case.name == "postdetect" else _no_grid)(case, out),
    "no_covered_cell": _no_covered_cell, "every_row_invalid": _invalid,
}


def test_every_entry_point_has_its_stops():
    """The stops the table must hold (so that a row cannot lose one silently)."""
    want = {"tdoa": {"no_task"}, "tdoa_nearest": {"no_task"}, "tdoa_linear": {"no_task"}, "tdoa_weighted": {"no_task"},
            "postdetect": {"nothing_kept", "all_misses", "beacon_matches_only", "every_group_underdetermined"},
            "posq": {"gate_0", "tiny_gate"}, "posq3_known_height": {"gate_0", "tiny_gate"}, "posq3_free_z": {"gate_0", "tiny_gate"},
            "coverage": {"no_covered_cell"}, "posg": {"every_group_underdetermined"},
            "posg3_free_z": {"every_group_underdetermined"}, "posg3_known_height": {"every_group_underdetermined"},
            "track": {"every_row_invalid"}}
    for case in P.CASES:
        assert set(case.stops) == want.get(case.name, set()), case
        assert case.zero is not None or case.name == "coverage", case
        assert case.refusal is not None, case
    assert kitchen_sink.COLUMNS[2] == "timestamp"       # the column the NaN test above writes into
