"""The post-detect entry points from several threads at once.  `_native` loads the library with ctypes.CDLL, so the GIL is
released inside every call and the threads really are inside the library together: four workers walk the whole table of
tests/post_contract_cases.py three times from different rows and hold every output to the bytes a lone call returned;
the times and the last error are the calling thread's; a result handle made on one thread is fetched and freed on
another.  Exact: bytes, counts and strings.

Measured on an MI355X: the serial pass over the 28 rows 0.018 s; four workers times three walks 0.246 s, about twelve
serial passes, against a limit of 60 s."""
import threading
import time

import pytest

import post_contract_cases as P
from thrifty_amd import _native

pytestmark = pytest.mark.gpu

WORKERS, WALKS, OFFSETS = 4, 3, (0, 4, 8, 12)


def in_thread(fn, limit=60.0):
    """fn() on a fresh daemon thread -> its result; its exception is raised here."""
    box = {}

    def body():
        try:
            box["result"] = fn()
        except BaseException as exc:      # noqa: BLE001 -- handed to the caller
            box["error"] = exc
    t = threading.Thread(target=body, daemon=True)
    t.start()
    t.join(limit)
    assert not t.is_alive(), "the thread did not come back within %g s" % limit
    if "error" in box:
        raise box["error"]
    return box["result"]


@pytest.fixture(scope="module")
def serial():
    """Every row once on the main thread -> ({name: outputs}, seconds of the pass)."""
    for case in P.CASES:
        case.run()                   # warm: module loading and first-call state are not part of the pass
    t0 = time.perf_counter()
    answers = {case.name: P.flatten(case.run()) for case in P.CASES}
    return answers, time.perf_counter() - t0


def test_four_threads_walk_the_table_and_get_the_serial_bytes(serial):
    answers, serial_s = serial
    assert len(P.CASES) > max(OFFSETS)
    before = _native.live_resources()
    barrier = threading.Barrier(WORKERS)
    problems = []

    def worker(offset):
        try:
            barrier.wait()
            for walk in range(WALKS):
                for k in range(len(P.CASES)):
                    case = P.CASES[(offset + k) % len(P.CASES)]
                    bad = P.same_bytes(P.flatten(case.run()), answers[case.name])
                    if bad:
                        problems.append("worker %d, walk %d, %s: %s differ" % (offset, walk, case, ", ".join(bad)))
        except BaseException as exc:      # noqa: BLE001 -- reported by the main thread
            problems.append("worker %d: %r" % (offset, exc))

    threads = [threading.Thread(target=worker, args=(offset,), daemon=True) for offset in OFFSETS]
    limit = max(60.0, 20.0 * serial_s * WALKS)
    t0 = time.perf_counter()
    for t in threads:
        t.start()
    deadline = t0 + limit
    for t in threads:
        t.join(max(0.0, deadline - time.perf_counter()))
    threaded_s = time.perf_counter() - t0
    print("serial pass %.3f s; %d workers x %d walks %.3f s (limit %.1f s)" % (serial_s, WORKERS, WALKS, threaded_s, limit))
    alive = [t for t in threads if t.is_alive()]
    assert not alive, "%d workers still running after %.1f s" % (len(alive), limit)
    assert problems == []
    assert _native.live_resources() == before


@pytest.mark.parametrize("name,other", [("z_four", "posq3_free_z"), ("match", "posq3_free_z"), ("reldist", "posq3_free_z")])
def test_times_are_the_calling_threads(name, other):
    mine, theirs = P.BY_NAME[name], P.BY_NAME[other]
    theirs.run()
    theirs_before = theirs.times()
    mine.run()
    kept = mine.times()
    assert len(kept) == mine.n_times and sum(kept) > 0

    def fresh():
        seen = [mine.times(), theirs.times()]
        theirs.run()
        return seen + [theirs.times(), mine.times()]
    nothing_mine, nothing_theirs, after, still_nothing = in_thread(fresh)
    assert nothing_mine == (0.0,) * mine.n_times and nothing_theirs == (0.0,) * theirs.n_times
    assert len(after) == theirs.n_times and all(t >= 0 for t in after) and sum(after) > 0 and after[1] > 0
    assert still_nothing == (0.0,) * mine.n_times
    assert mine.times() == kept and theirs.times() == theirs_before


def test_the_last_error_is_the_calling_threads():
    a, b = P.BY_NAME["posg3_free_z"], P.BY_NAME["track"]
    barrier = threading.Barrier(2)
    said = {"a": [], "b": []}

    def provoke(key, case, **bad):
        barrier.wait()
        for _ in range(50):
            try:
                case.run(**bad)
                said[key].append("no error")
            except ValueError as exc:
                said[key].append("%s | %s" % (exc, _native.load_library().thr_last_error().decode()))
    threads = [threading.Thread(target=provoke, args=("a", a), kwargs=dict(grid=64), daemon=True),
               threading.Thread(target=provoke, args=("b", b), kwargs=dict(q=-1.0), daemon=True)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60.0)
    assert not any(t.is_alive() for t in threads)
    assert len(said["a"]) == len(said["b"]) == 50
    assert all(text.count("thr_posg3: grid must be 16 or 32, not 64") == 2 and "thr_track" not in text for text in said["a"]), said["a"][:3]
    assert all(text.count("thr_track: q must be finite and not negative") == 2 and "thr_posg3" not in text for text in said["b"]), said["b"][:3]


def test_a_handle_made_here_is_fetched_and_freed_over_there(serial):
    answers, _ = serial
    case = P.BY_NAME["posq3_free_z"]
    case.run()
    before = _native.live_resources()
    raw = P.raw_call(case)                  # on this thread
    assert raw.rc == 0 and raw.handle.value

    def elsewhere():
        out = P.fetch_all(case, raw)
        copied = case.times()
        raw.free()
        return out, copied
    out, copied = in_thread(elsewhere)
    want = dict(answers[case.name])
    want.pop("(counts)")
    assert P.same_bytes(out, want) == []
    assert copied[:-1] == (0.0,) * (case.n_times - 1) and copied[-1] >= 0      # that thread made no call: only its own copies out
    assert _native.live_resources() == before
