#!/usr/bin/env python
"""Fixtures of `thr_posq3` (tests/golden/posq3/*.npz): small scenes with antenna heights, what the NumPy statement
(tests/posq3_ref.py) makes of them, and per task the exact (weighted) minimiser by Newton's method in 50-digit
arithmetic.  Needs mpmath; nothing of the reference is read.

    python tests/golden/make_golden_posq3.py

h_fault6     known height: a jittered ring of six antennas at 3 .. 40 m, radius 100 m, the tag at 1 m, all pairs, 0.3 m
             of noise per arrival, one receiver's arrival 150 m late in every third group; gate 3 m, ratio 0.5, min_rx 5.
z_fault7     free z: seven antennas at 3 .. 80 m, z_range -20 .. 100 m, the same noise and fault; min_rx 6.
z_weighted7  free z: the same ring, about 85 % of the pairs, weights = the snr column.
h_five       known height: five antennas, the floor of min_rx; a height per group.

For EVERY fixture the generator asserts that the statement alone excludes the planted receiver in every affected group
and none in a clean group.  ref_err_max is the statement's own distance from the exact minimisers over the tasks that
ended THR_POS_OK (the bound the device is held to is built from it, tests/test_gpu_posq3.py).  parent_digests.json in
the same folder is not made here: it was taken on the device before csrc/pos3_lm.hpp learnt weights and row subsets."""
import os
import sys

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import posq3_golden  # noqa: E402
import posq3_ref  # noqa: E402

mpmath.mp.dps = 50
OK = 0


def exact_minimum(start, a, b, tdoa, w, n):
    """Newton on the gradient of sum w r^2 in the first n coordinates from `start`[3] -> x_star[3] (the others stay),
    or NaNs when it does not converge to a point with a positive definite Hessian."""
    mp = mpmath.mp
    a = [mp.matrix(row.tolist()) for row in a]
    b = [mp.matrix(row.tolist()) for row in b]
    tc = [mp.mpf(float(t)) * mp.mpf(posq3_golden.C) for t in tdoa]
    w = [mp.mpf(float(v)) for v in w]
    p = mp.matrix([float(v) for v in start])
    eye = mp.eye(3)

    def parts(p):
        grad, hess = mp.zeros(3, 1), mp.zeros(3, 3)
        for ai, bi, ti, wi in zip(a, b, tc, w):
            va, vb = ai - p, bi - p
            da, db = mp.norm(va), mp.norm(vb)
            ua, ub = va / da, vb / db
            res, row = ti - (da - db), ua - ub
            grad += wi * row * res
            hess += wi * (row * row.T + res * ((eye - ub * ub.T) / db - (eye - ua * ua.T) / da))
        return grad[:n, 0], hess[:n, :n]

    for _ in range(60):
        grad, hess = parts(p)
        step = mp.lu_solve(hess, grad)
        for k in range(n):
            p[k] -= step[k]
        if mp.norm(step) < mp.mpf(10) ** -30:
            break
    else:
        return np.full(3, np.nan)
    if min(mp.eigsy(parts(p)[1], eigvals_only=True)) <= 0:
        return np.full(3, np.nan)
    return np.array([float(p[0]), float(p[1]), float(p[2])])


def star_of(s, weights, rows, use, start, status, n):
    if status != OK:
        return np.full(3, np.nan)
    rows = rows[use]
    w = np.ones(len(rows)) if weights is None else weights[rows]
    return exact_minimum(start, s["table"][s["rx0"][rows]], s["table"][s["rx1"][rows]], s["tdoa"][rows], w, n)


def make(name, s, ids, free_z, group_h, z0, z_range, weights, gate_m, ratio, min_rx, planted_count):
    mode = posq3_golden.FREE_Z if free_z else posq3_golden.KNOWN_HEIGHT
    x0 = (0.1, 0.1, z0 if free_z else 0.0)
    ref = posq3_ref.posq3_ref(s["group_ptr"], s["rx0"], s["rx1"], s["tdoa"], s["snr"], s["table"], mode, group_h, weights, gate_m,
                              ratio, min_rx, x0, z_range)
    # the condition on the inputs: the statement alone names the planted receiver in every affected group and touches
    # no clean group
    np.testing.assert_array_equal(ref["counts"][:, 2], s["planted"], err_msg=name)
    np.testing.assert_array_equal((ref["flags"] & 1) != 0, s["planted"] >= 0, err_msg=name)
    np.testing.assert_array_equal((ref["flags"] & 2) != 0, s["planted"] >= 0, err_msg=name)
    assert int((s["planted"] >= 0).sum()) == planted_count
    ptr = s["group_ptr"]
    n, axes = len(ptr) - 1, 3 if free_z else 2
    full_star, task_star = np.full((n, 3), np.nan), np.full((len(ref["task_rx"]), 3), np.nan)
    for g in range(n):
        rows = np.arange(ptr[g], ptr[g + 1])
        full_star[g] = star_of(s, weights, rows, np.ones(len(rows), bool), ref["full_pos"][g], ref["full_status"][g], axes)
        for t in range(ref["task_ptr"][g], ref["task_ptr"][g + 1]):
            r = ref["task_rx"][t]
            use = (s["rx0"][rows] != r) & (s["rx1"][rows] != r)
            task_star[t] = star_of(s, weights, rows, use, ref["task_pos"][t], ref["task_status"][t], axes)
    err = np.concatenate([np.abs(ref["full_pos"] - full_star).max(axis=1), np.abs(ref["task_pos"] - task_star).max(axis=1)])
    assert np.isfinite(err).sum() >= n, "most tasks have an exact minimiser"
    ref_err_max = float(np.nanmax(err))
    assert ref_err_max < 1e-9, ref_err_max
    chosen_err = np.sqrt(np.sum((ref["pos"] - s["mobile"]) ** 2, axis=1))
    ids = np.asarray(ids, dtype=np.int32)
    path = os.path.join(posq3_golden.GOLDEN, name + ".npz")
    np.savez_compressed(
        path, rx_ids=ids, rx_xyz=s["table"], free_z=free_z, group_h=np.zeros(0) if free_z else group_h, z0=z0,
        z_range=np.zeros(0) if z_range is None else np.asarray(z_range, dtype=np.float64), group_ptr=ptr, rx0=ids[s["rx0"]],
        rx1=ids[s["rx1"]], tdoa=s["tdoa"], snr=s["snr"], weights=np.zeros(0) if weights is None else weights,
        planted=np.where(s["planted"] >= 0, ids[np.maximum(s["planted"], 0)], -1), mobile=s["mobile"],
        group_id=np.arange(n, dtype=np.int32) * 3 + 100, group_timestamp=1.7e9 + 0.25 * np.arange(n), group_tx=np.full(n, 7, np.int32),
        gate_m=gate_m, ratio=ratio, min_rx=min_rx, full_x_star=full_star, task_x_star=task_star, ref_err_max=ref_err_max,
        ref_flags=ref["flags"], ref_excluded=ref["counts"][:, 2], ref_task_ptr=ref["task_ptr"], ref_pos=ref["pos"], ref_rms=ref["rms"])
    print("%s: %d groups, %d rows, %d flagged, %d tasks, ref_err_max %.3g m, worst error after exclusion %.3g m, %d bytes" % (
        name, n, ptr[-1], int((ref["flags"] & 1).sum()), len(ref["task_rx"]), ref_err_max, chosen_err.max(), os.path.getsize(path)))
    return ref


def main():
    os.makedirs(posq3_golden.GOLDEN, exist_ok=True)
    s = posq3_golden.scene(seed=2, n_rx=6, n_groups=30, z_span=(3.0, 40.0), tag_z=1.0)
    make("h_fault6", s, [3, 5, 8, 13, 21, 34], False, np.full(30, 1.0), 0.0, None, None, 3.0, 0.5, 5, 10)
    s = posq3_golden.scene(seed=3, n_rx=7, n_groups=30, z_span=(3.0, 80.0), tag_z=1.0)
    make("z_fault7", s, [2, 4, 6, 9, 12, 40, 41], True, None, 40.0, (-20.0, 100.0), None, 3.0, 0.5, 6, 10)
    s = posq3_golden.scene(seed=5, n_rx=7, n_groups=24, z_span=(3.0, 80.0), tag_z=1.0, every=4, keep=0.85)
    make("z_weighted7", s, [2, 4, 6, 9, 12, 40, 41], True, None, 40.0, (-20.0, 100.0), s["snr"].copy(), 3.0, 0.5, 6, 6)
    heights = np.linspace(0.5, 2.0, 24)
    s = posq3_golden.scene(seed=7, n_rx=5, n_groups=24, z_span=(3.0, 40.0), tag_z=heights)
    make("h_five", s, [1, 2, 3, 4, 5], False, heights, 0.0, None, None, 3.0, 0.5, 5, 8)


if __name__ == "__main__":
    main()
