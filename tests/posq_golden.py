"""The posq fixtures (tests/golden/posq/*.npz, made by tests/golden/make_golden_posq.py) and the small synthetic
scenes the host and GPU tests of `thr_posq` share: a jittered ring of receivers, arrivals with noise, one
receiver's arrival delayed in some groups (one multipath detection), TDOA rows for chosen receiver pairs."""
import itertools
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "posq")
SETS = ("posq_fault6", "posq_weighted7")
C = 2.997e8
_cache = {}


def load(name):
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, name + ".npz")) as g:
            _cache[name] = {key: g[key] for key in g.files}
        for value in _cache[name].values():
            value.setflags(write=False)
    return _cache[name]


def parent_digests():
    with open(os.path.join(GOLDEN, "thr_pos_digests.json")) as f:
        return json.load(f)


def rx_pos(g):
    """The receivers as the dict the public interface takes, in the fixture's order."""
    return {int(r): np.array(xy) for r, xy in zip(g["rx_ids"], g["rx_xy"])}


def dense(g, column):
    index = {int(r): k for k, r in enumerate(g["rx_ids"])}
    return np.array([index[int(v)] for v in column], dtype=np.int32)


def weights_of(g):
    return g["weights"] if len(g["weights"]) else None


def ring(rng, n_rx, radius=100.0):
    ang = np.linspace(0, 2 * np.pi, n_rx, endpoint=False) + 0.3
    return np.c_[np.cos(ang), np.sin(ang)] * radius + rng.normal(0, radius * 0.05, (n_rx, 2))


def scene(seed, n_rx, n_groups, noise=0.3, delay=150.0, every=3, keep=1.0, radius=100.0, pairs=None, late_rx=None):
    """-> dict(table, group_ptr, rx0, rx1 (dense), tdoa, snr, planted (dense index or -1 per group)).  Every
    group is a mobile inside the ring; receiver arrivals carry `noise` metres; in every `every`-th group (0: in
    none) one receiver's arrival is `delay` metres late (`late_rx`, or each in turn).  Rows: the pairs i < j, each kept with probability `keep`
    (or the list `pairs`, the same for every group)."""
    rng = np.random.default_rng(seed)
    table = ring(rng, n_rx, radius)
    every_pair = list(itertools.combinations(range(n_rx), 2))
    ptr, rx0, rx1, tdoa, snr, planted = [0], [], [], [], [], []
    for g in range(n_groups):
        ang, rad = rng.uniform(0, 2 * np.pi), 0.6 * radius * np.sqrt(rng.uniform())
        mobile = np.array([np.cos(ang), np.sin(ang)]) * rad
        arrival = np.linalg.norm(table - mobile, axis=1) + rng.normal(0, noise, n_rx)
        bad = -1
        if every and g % every == every - 1:
            bad = (g // every) % n_rx if late_rx is None else late_rx
            arrival[bad] += delay
        rows = list(pairs) if pairs is not None else [pr for pr in every_pair if keep >= 1.0 or rng.random() < keep]
        for i, j in rows:
            rx0.append(i), rx1.append(j), tdoa.append((arrival[i] - arrival[j]) / C), snr.append(rng.uniform(5.0, 500.0))
        ptr.append(len(rx0))
        planted.append(bad)
    return {"table": table, "group_ptr": np.array(ptr, dtype=np.int64), "rx0": np.array(rx0, dtype=np.int32),
            "rx1": np.array(rx1, dtype=np.int32), "tdoa": np.array(tdoa, dtype=np.float64),
            "snr": np.array(snr, dtype=np.float64), "planted": np.array(planted, dtype=np.int32)}


def without_receiver(group_ptr, rx0, rx1, columns, groups, receivers):
    """The rows of `groups[k]` that do not name `receivers[k]`, as new CSR columns: what a candidate solves."""
    ptr, keep = [0], []
    for g, r in zip(groups, receivers):
        rows = np.arange(group_ptr[g], group_ptr[g + 1])
        rows = rows[(rx0[rows] != r) & (rx1[rows] != r)]
        keep.append(rows)
        ptr.append(ptr[-1] + len(rows))
    keep = np.concatenate(keep) if keep else np.zeros(0, dtype=np.int64)
    return np.array(ptr, dtype=np.int64), rx0[keep], rx1[keep], [np.asarray(c)[keep] for c in columns]


# ---------------------------------------------------------------- checks the GPU tests share (they load the library)
def assert_candidates_equal_thr_pos(out, group_ptr, rx0, rx1, tdoa, snr, table, x0=(0.1, 0.1), max_iter=100):
    """Every candidate's pos / status / iters equal ONE thr_pos call on the groups rebuilt without that receiver's
    rows, to the bit; task_nrx is the count of the receivers those rows name.  -> the number of candidates."""
    from thrifty_amd import _native
    tptr = out["task_ptr"]
    groups = np.repeat(np.arange(len(tptr) - 1), np.diff(tptr))
    ptr, r0, r1, (t, s) = without_receiver(group_ptr, rx0, rx1, (tdoa, snr), groups, out["task_rx"])
    want = _native.pos(ptr, r0, r1, t, s, table, x0=x0, max_iter=max_iter)
    assert out["task_pos"].tobytes() == want["pos"].tobytes()
    assert out["task_status"].tobytes() == want["status"].tobytes()
    assert out["task_iters"].tobytes() == want["iters"].tobytes()
    nrx = [len(set(r0[a:b].tolist()) | set(r1[a:b].tolist())) for a, b in zip(ptr[:-1], ptr[1:])]
    np.testing.assert_array_equal(out["task_nrx"], nrx)
    return len(groups)


def assert_choice_follows_the_rule(out, group_ptr, rx0, rx1, gate_m, ratio, min_rx):
    """Flags, the candidates' list, eligibility, the choice and `excluded` against the rule stated in NumPy
    (posq_ref.is_flagged / choose) on the device's OWN rms values; the chosen task's numbers are copies."""
    import posq_ref
    ptr = np.asarray(group_ptr).tolist()
    tptr = out["task_ptr"].tolist()
    assert tptr[0] == 0 and tptr[-1] == len(out["task_rx"])
    for g, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
        names = sorted(set(rx0[a:b].tolist()) | set(rx1[a:b].tolist()))
        flagged = posq_ref.is_flagged(int(out["full_status"][g]), len(names), out["rms"][g, 0], gate_m, min_rx)
        ta, tb = tptr[g], tptr[g + 1]
        assert out["task_rx"][ta:tb].tolist() == (names if flagged else []), g
        flags, best = posq_ref.choose(out["rms"][g, 0], flagged, names, out["task_rms"][ta:tb], out["task_status"][ta:tb],
                                      out["task_nrx"][ta:tb], ratio, min_rx)
        assert int(out["flags"][g]) == flags, (g, int(out["flags"][g]), flags)
        excluded = names[best] if best >= 0 else -1
        assert int(out["counts"][g, 2]) == excluded, g
        np.testing.assert_array_equal(out["used"][a:b], (rx0[a:b] != excluded) & (rx1[a:b] != excluded))
        assert int(out["counts"][g, 1]) == int(out["used"][a:b].sum())
        if best >= 0:
            t = ta + best
            assert out["pos"][g].tobytes() == out["task_pos"][t].tobytes() and out["rms"][g, 1].tobytes() == out["task_rms"][t].tobytes()
            assert (int(out["status"][g]), int(out["iters"][g]), int(out["counts"][g, 0])) == (
                int(out["task_status"][t]), int(out["task_iters"][t]), int(out["task_nrx"][t]))
        else:
            assert out["pos"][g].tobytes() == out["full_pos"][g].tobytes() and out["rms"][g, 1].tobytes() == out["rms"][g, 0].tobytes()
            assert int(out["status"][g]) == int(out["full_status"][g]) and int(out["counts"][g, 0]) == len(names)
