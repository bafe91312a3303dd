"""The fetch contract of the twelve result-handle families (thr_post, thr_tstats, thr_bsync, thr_tdstats, thr_reldist,
thr_tdmat, thr_posq, thr_track, thr_posg, thr_coverage, thr_posg3, thr_posq3) on a live handle from a raw call
(tests/post_contract_cases.py): the exact size and nothing else, the output index, NULL handles and destinations, empty
outputs, thr_post_fetch's host-side answer for a stage that did not run, repeated and reversed fetches, the wrapper's
`outputs=` selection and the copy-out time.  Exact: bytes and status codes."""
import numpy as np
import pytest

import post_contract_cases as P
from thrifty_amd import _native

pytestmark = pytest.mark.gpu

FAMILIES = pytest.mark.parametrize("case", P.FAMILIES, ids=repr)
FILL = 0xA5


def last_error():
    return _native.load_library().thr_last_error().decode()


class Held(object):
    """A raw call's live handle with the sizes its counts give; freed on the way out."""

    def __init__(self, case, args=None, **changes):
        self.case, self.args, self.changes = case, args, changes

    def __enter__(self):
        self.raw = P.raw_call(self.case, args=self.args, **self.changes)
        assert self.raw.rc == 0 and self.raw.handle.value
        self.specs = P.output_specs(self.case, self.raw.counts_dict(), self.args)
        return self

    def __exit__(self, *exc):
        self.raw.free()

    def nbytes(self, name):
        which, kind, shape = self.specs[name]
        return int(np.prod(shape, dtype=np.int64)) * kind.itemsize

    def fetch(self, name):
        which, kind, shape = self.specs[name]
        out = np.zeros(shape, dtype=kind)
        assert P.fetch(self.case, self.raw.handle, which, out, out.nbytes) == 0, (name, last_error())
        return out


def test_the_twelve_families_are_here():
    assert sorted({case.family.stem for case in P.FAMILIES}) == sorted(
        ["post", "tstats", "bsync", "tdstats", "reldist", "tdmat", "posq", "track", "posg", "coverage", "posg3", "posq3"])


@FAMILIES
def test_every_output_fetches_with_its_exact_size_any_number_of_times(case):
    want = P.flatten(case.run())
    want.pop("(counts)")
    with Held(case) as h:
        names = sorted(h.specs, key=lambda name: h.specs[name][0])
        assert [h.specs[name][0] for name in names] == list(range(len(names)))
        copied = [case.times()[-1]]
        assert copied[0] == 0.0                 # the call itself has fetched nothing yet
        first = {}
        for name in names:
            first[name] = h.fetch(name)
            if h.nbytes(name):
                copied.append(case.times()[-1])
        assert P.same_bytes(first, want) == []
        assert any(h.nbytes(name) for name in names)
        again = {name: h.fetch(name) for name in names}
        name = next(n for n in names if h.nbytes(n))
        assert P.fetch(case, h.raw.handle, h.specs[name][0], first[name], h.nbytes(name) + 1) == _native.ERR_ARG     # a refused fetch
        assert P.fetch(case, h.raw.handle, len(names), first[name], h.nbytes(name)) == _native.ERR_ARG                # in between
        backwards = {name: h.fetch(name) for name in reversed(names)}
        copied.append(case.times()[-1])
        assert P.same_bytes(again, want) == [] and P.same_bytes(backwards, want) == [] and P.same_bytes(first, want) == []
        assert all(b >= a for a, b in zip(copied, copied[1:])), copied
        assert all(t >= 0 for t in case.times())


@FAMILIES
def test_a_wrong_size_is_refused_and_nothing_is_written(case):
    who = "thr_%s_fetch" % case.family.stem
    with Held(case) as h:
        per_kind = {}
        for name in sorted(h.specs, key=lambda name: h.specs[name][0]):
            if h.nbytes(name):
                per_kind.setdefault(h.specs[name][1], name)
        assert per_kind
        for kind, name in per_kind.items():
            which, exact = h.specs[name][0], h.nbytes(name)
            for wrong in (exact - 1, exact + 1, exact + kind.itemsize):
                dst = np.full(exact + kind.itemsize + 8, FILL, dtype=np.uint8)
                assert P.fetch(case, h.raw.handle, which, dst, wrong) == _native.ERR_ARG, (name, wrong)
                said = last_error()
                assert who in said and "%d bytes, not %d" % (exact, wrong) in said, said
                assert np.all(dst == FILL), name
            assert h.fetch(name).nbytes == exact        # and the exact size still goes through


@FAMILIES
def test_a_wrong_index_a_null_handle_and_a_null_destination(case):
    who = "thr_%s_fetch" % case.family.stem
    with Held(case) as h:
        n_out = len(h.specs)
        name = next(n for n in sorted(h.specs, key=lambda n: h.specs[n][0]) if h.nbytes(n))
        which, exact = h.specs[name][0], h.nbytes(name)
        dst = np.full(exact, FILL, dtype=np.uint8)
        for bad in (-1, n_out):
            assert P.fetch(case, h.raw.handle, bad, dst, exact) == _native.ERR_ARG
            assert who in last_error() and "(%d)" % bad in last_error()
        assert P.fetch(case, None, which, dst, exact) == _native.ERR_ARG and who in last_error()
        assert P.fetch(case, h.raw.handle, which, None, exact) == _native.ERR_ARG
        assert who in last_error() and "null" in last_error()
        assert np.all(dst == FILL)
        assert P.fetch(case, h.raw.handle, which, dst, exact) == 0
        assert dst.tobytes() == h.fetch(name).tobytes()


EMPTY = [(case, stop) for case, stop in P.stops_of(P.FAMILIES) if not (stop == "zero" and case.zero_refused)]
SURELY_EMPTY = ("zero", "gate_0", "nothing_kept", "all_misses", "beacon_matches_only")      # stops that leave an output without a byte


@pytest.mark.parametrize("case,stop", EMPTY, ids=lambda v: v if isinstance(v, str) else repr(v))
def test_an_empty_output_takes_a_null_destination_and_no_bytes(case, stop):
    args, changes = P.stop_call(case, stop)
    with Held(case, args, **changes) as h:
        empty = [name for name in h.specs if h.nbytes(name) == 0]
        assert empty or stop not in SURELY_EMPTY, "%s / %s has no empty output" % (case, stop)
        if (case.name, stop) == ("posq", "gate_0"):
            assert "task_pos" in empty
        somewhere = np.full(16, FILL, dtype=np.uint8)
        for name in empty:
            which = h.specs[name][0]
            assert P.fetch(case, h.raw.handle, which, None, 0) == 0, (name, last_error())
            assert P.fetch(case, h.raw.handle, which, somewhere, 0) == 0
            assert P.fetch(case, h.raw.handle, which, somewhere, 8) == _native.ERR_ARG and "0 bytes, not 8" in last_error()
            assert P.fetch(case, h.raw.handle, which, None, 8) == _native.ERR_ARG
        assert np.all(somewhere == FILL)


@pytest.mark.parametrize("stop,host_side,device_side", [
    ("zero", ["match_ptr", "group_ptr"], []),
    ("nothing_kept", ["match_ptr", "group_ptr"], ["txid", "keep"]),
    ("all_misses", ["group_ptr"], ["match_ptr", "misses"]),
    ("beacon_matches_only", ["group_ptr"], ["match_ptr", "match_idx"]),
])
def test_post_fetch_answers_for_a_stage_that_did_not_run_without_a_copy(stop, host_side, device_side):
    """The CSR pointers of a stage that did not run are the single zero the header documents, written on the host: the
    copy-out time of thr_debug_post_times does not move."""
    case = P.BY_NAME["postdetect"]
    args, changes = P.stop_call(case, stop)
    with Held(case, args, **changes) as h:
        for name in device_side:
            assert h.nbytes(name) > 0
            h.fetch(name)
        before = _native.post_times()[5]
        for name in host_side:
            which = h.specs[name][0]
            assert h.nbytes(name) == 8
            dst = np.full(1, -1, dtype=np.int64)
            assert P.fetch(case, h.raw.handle, which, dst, 8) == 0
            assert dst.tolist() == [0]
            assert _native.post_times()[5] == before, name
            assert P.fetch(case, h.raw.handle, which, None, 8) == _native.ERR_ARG        # the same checks come first
            assert P.fetch(case, h.raw.handle, which, dst, 16) == _native.ERR_ARG


@FAMILIES
def test_the_wrappers_outputs_argument_selects_exactly(case):
    counts, full = case.run()
    names = sorted(case.family.outputs, key=lambda name: case.family.outputs[name][0])
    for name in (names[0], names[len(names) // 2], names[-1]):
        got_counts, got = case.run(outputs=[name])
        assert list(got) == [name] and got_counts == counts
        assert got[name].dtype == full[name].dtype and got[name].shape == full[name].shape
        assert got[name].tobytes() == full[name].tobytes(), name
