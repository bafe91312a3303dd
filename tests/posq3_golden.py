"""The posq3 fixtures (tests/golden/posq3/*.npz, made by tests/golden/make_golden_posq3.py) and the small synthetic
scenes the host and GPU tests of `thr_posq3` share: tests/posq_golden.py's scene with a height per receiver and a tag
height -- a jittered ring of antennas, arrivals with noise, one receiver's arrival delayed in some groups (one
multipath detection), TDOA rows for chosen receiver pairs."""
import itertools
import json
import os

import numpy as np

import posq_golden

ROOT = posq_golden.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "posq3")
SETS_H = ("h_fault6", "h_five")
SETS_Z = ("z_fault7", "z_weighted7")
SETS = SETS_H + SETS_Z
C = posq_golden.C
KNOWN_HEIGHT, FREE_Z = 0, 1
_cache = {}

without_receiver = posq_golden.without_receiver


def load(name):
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, name + ".npz")) as g:
            _cache[name] = {key: g[key] for key in g.files}
        for value in _cache[name].values():
            value.setflags(write=False)
    return _cache[name]


def parent_digests():
    """sha256 of thr_pos3's outputs per pos3 fixture and thr_posg3's per posg3 fixture, taken on the device at the parent commit."""
    with open(os.path.join(GOLDEN, "parent_digests.json")) as f:
        return json.load(f)


def rx_pos(g):
    """The receivers as the dict the public interface takes, in the fixture's order."""
    return {int(r): np.array(xyz) for r, xyz in zip(g["rx_ids"], g["rx_xyz"])}


def dense(g, column):
    index = {int(r): k for k, r in enumerate(g["rx_ids"])}
    return np.array([index[int(v)] for v in column], dtype=np.int32)


def weights_of(g):
    return g["weights"] if len(g["weights"]) else None


def mode_of(g):
    return FREE_Z if bool(g["free_z"]) else KNOWN_HEIGHT


def columns(g):
    """(group_ptr, rx0, rx1 (dense), tdoa, snr, table, mode) of a fixture."""
    return g["group_ptr"], dense(g, g["rx0"]), dense(g, g["rx1"]), g["tdoa"], g["snr"], g["rx_xyz"], mode_of(g)


def options(g, weighted=True, gated=True, weights_key="row_weight"):
    """The keyword arguments of `_native.posq3` after the columns and the mode (of `posq3_ref.posq3_ref` with
    weights_key="weights")."""
    free_z = bool(g["free_z"])
    return dict(group_h=None if free_z else g["group_h"], **{weights_key: weights_of(g) if weighted else None},
                gate_m=float(g["gate_m"]) if gated else 0.0, ratio=float(g["ratio"]), min_rx=int(g["min_rx"]),
                x0=(0.1, 0.1, float(g["z0"]) if free_z else 0.0), z_range=tuple(g["z_range"].tolist()) if len(g["z_range"]) else None)


def mode_args(g):
    """The keyword arguments of `pos_3d_quality.quality3_columns` / `solve` that say how the set is solved."""
    if bool(g["free_z"]):
        return {"free_z": True, "z0": float(g["z0"]), "z_range": tuple(g["z_range"].tolist()) if len(g["z_range"]) else None}
    return {"height": g["group_h"]}


def ring3(rng, n_rx, radius, z_lo, z_hi):
    """posq_golden.ring with the stated height spread in no order around the ring."""
    return np.c_[posq_golden.ring(rng, n_rx, radius), rng.permutation(np.linspace(z_lo, z_hi, n_rx))]


def scene(seed, n_rx, n_groups, z_span=(3.0, 40.0), tag_z=1.0, noise=0.3, delay=150.0, every=3, keep=1.0, radius=100.0, pairs=None,
          late_rx=None, table=None):
    """-> dict(table[n_rx, 3], group_ptr, rx0, rx1 (dense), tdoa, snr, planted (dense index or -1 per group), mobile[g, 3]).
    `posq_golden.scene` with the antennas at heights z_span[0] .. z_span[1] and every mobile at the height `tag_z`
    (a number or one per group): receiver arrivals carry `noise` metres; in every `every`-th group (0: in none) one
    receiver's arrival is `delay` metres late (`late_rx`, or each in turn).  Rows: the pairs i < j, each kept with
    probability `keep` (or the list `pairs`, the same for every group; or one list per group)."""
    rng = np.random.default_rng(seed)
    table = ring3(rng, n_rx, radius, *z_span) if table is None else np.asarray(table, dtype=np.float64)
    n_rx = len(table)
    every_pair = list(itertools.combinations(range(n_rx), 2))
    heights = np.broadcast_to(np.asarray(tag_z, dtype=np.float64), (n_groups,))
    per_group = pairs is not None and len(pairs) == n_groups and len(pairs[0]) and not np.isscalar(pairs[0][0])
    ptr, rx0, rx1, tdoa, snr, planted, mobiles = [0], [], [], [], [], [], []
    for g in range(n_groups):
        ang, rad = rng.uniform(0, 2 * np.pi), 0.6 * radius * np.sqrt(rng.uniform())
        mobile = np.array([np.cos(ang) * rad, np.sin(ang) * rad, heights[g]])
        arrival = np.linalg.norm(table - mobile, axis=1) + rng.normal(0, noise, n_rx)
        bad = -1
        if every and g % every == every - 1:
            bad = (g // every) % n_rx if late_rx is None else late_rx
            arrival[bad] += delay
        if pairs is not None:
            rows = list(pairs[g] if per_group else pairs)
        else:
            rows = [pr for pr in every_pair if keep >= 1.0 or rng.random() < keep]
        for i, j in rows:
            rx0.append(i), rx1.append(j), tdoa.append((arrival[i] - arrival[j]) / C), snr.append(rng.uniform(5.0, 500.0))
        ptr.append(len(rx0))
        planted.append(bad)
        mobiles.append(mobile)
    return {"table": table, "group_ptr": np.array(ptr, dtype=np.int64), "rx0": np.array(rx0, dtype=np.int32),
            "rx1": np.array(rx1, dtype=np.int32), "tdoa": np.array(tdoa, dtype=np.float64),
            "snr": np.array(snr, dtype=np.float64), "planted": np.array(planted, dtype=np.int32),
            "mobile": np.array(mobiles, dtype=np.float64).reshape(n_groups, 3)}


# ---------------------------------------------------------------- checks the GPU tests share (they load the library)
def assert_candidates_equal_thr_pos3(out, group_ptr, rx0, rx1, tdoa, snr, table, mode, group_h=None, x0=(0.1, 0.1, 0.0), z_range=None,
                                     max_iter=100):
    """Every candidate's pos / status / iters equal ONE thr_pos3 call on the groups rebuilt without that receiver's
    rows, to the bit (and its rms, unweighted: sqrt(F / rows) is thr_pos3's rms_out); task_nrx is the count of the
    receivers those rows name.  -> the number of candidates."""
    from thrifty_amd import _native
    tptr = out["task_ptr"]
    groups = np.repeat(np.arange(len(tptr) - 1), np.diff(tptr))
    ptr, r0, r1, (t, s) = without_receiver(group_ptr, rx0, rx1, (tdoa, snr), groups, out["task_rx"])
    want = _native.pos3(ptr, r0, r1, t, s, table, mode, None if group_h is None else np.asarray(group_h)[groups], x0, z_range, max_iter)
    assert out["task_pos"].tobytes() == want["pos"].tobytes()
    assert out["task_status"].tobytes() == want["status"].tobytes()
    assert out["task_iters"].tobytes() == want["iters"].tobytes()
    assert out["task_rms"].tobytes() == want["rms"].tobytes()
    nrx = [len(set(r0[a:b].tolist()) | set(r1[a:b].tolist())) for a, b in zip(ptr[:-1], ptr[1:])]
    np.testing.assert_array_equal(out["task_nrx"], nrx)
    return len(groups)


def assert_choice_follows_the_rule(out, group_ptr, rx0, rx1, gate_m, ratio, min_rx):
    """`posq_golden.assert_choice_follows_the_rule` (flags, the candidates' list, eligibility, the choice, `excluded`,
    `used`, n_rows against posq_ref.is_flagged / choose on the device's OWN rms values; the chosen task's numbers are
    copies) -- it reads no shape -- and an unflagged group has no candidate and excludes nothing."""
    posq_golden.assert_choice_follows_the_rule(out, group_ptr, rx0, rx1, gate_m, ratio, min_rx)
    unflagged = (out["flags"] & 1) == 0
    assert np.all(out["counts"][unflagged, 2] == -1) and np.all(np.diff(out["task_ptr"])[unflagged] == 0)
