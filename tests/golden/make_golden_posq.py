#!/usr/bin/env python
"""Fixtures of `thr_posq` (tests/golden/posq/*.npz): small scenes, what the NumPy statement (tests/posq_ref.py)
makes of them, and per task the exact (weighted) minimiser by Newton's method in 50-digit arithmetic.  Needs
mpmath; nothing of the reference is read.

    python tests/golden/make_golden_posq.py

posq_fault6     the scene of the issue: a jittered ring of six receivers, radius 100 m, all pairs, 0.3 m of noise
                per arrival, one receiver's arrival 150 m late in every third group; gate 3 m, ratio 0.5.  The
                generator ASSERTS that the statement alone excludes the planted receiver in every affected group
                and none elsewhere, and that the repaired positions are as good as the clean ones.
posq_weighted7  seven receivers, about 80 % of the pairs, weights = the snr column with some zeros, a late arrival
                in every fourth group; gate 3 m.

ref_err_max is the statement's own distance from the exact minimisers over the tasks that ended THR_POS_OK inside
the box (the bound the device is held to is built from it, tests/test_gpu_posq.py)."""
import os
import sys

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import posq_golden  # noqa: E402
import posq_ref  # noqa: E402

mpmath.mp.dps = 50
OK = 0


def exact_minimum(start, a, b, tdoa, w):
    """Newton on the gradient of sum w r^2 from `start` -> x_star, or NaNs when it does not converge to a point
    with a positive definite Hessian."""
    mp = mpmath.mp
    a = [mp.matrix(row.tolist()) for row in a]
    b = [mp.matrix(row.tolist()) for row in b]
    tc = [mp.mpf(float(t)) * mp.mpf(posq_golden.C) for t in tdoa]
    w = [mp.mpf(float(v)) for v in w]
    p = mp.matrix([float(v) for v in start])
    eye = mp.eye(2)

    def parts(p):
        grad, hess = mp.zeros(2, 1), mp.zeros(2, 2)
        for ai, bi, ti, wi in zip(a, b, tc, w):
            va, vb = ai - p, bi - p
            da, db = mp.norm(va), mp.norm(vb)
            ua, ub = va / da, vb / db
            res, row = ti - (da - db), ua - ub
            grad += wi * row * res
            hess += wi * (row * row.T + res * ((eye - ub * ub.T) / db - (eye - ua * ua.T) / da))
        return grad, hess

    for _ in range(60):
        grad, hess = parts(p)
        step = mp.lu_solve(hess, grad)
        p = p - step
        if mp.norm(step) < mp.mpf(10) ** -30:
            break
    else:
        return np.full(2, np.nan)
    if min(mp.eigsy(parts(p)[1], eigvals_only=True)) <= 0:
        return np.full(2, np.nan)
    return np.array([float(p[0]), float(p[1])])


def star_of(s, weights, rows, use, start, status):
    if status != OK:
        return np.full(2, np.nan)
    rows = rows[use]
    w = np.ones(len(rows)) if weights is None else weights[rows]
    return exact_minimum(start, s["table"][s["rx0"][rows]], s["table"][s["rx1"][rows]], s["tdoa"][rows], w)


def make(name, s, ids, weights, gate_m, ratio, min_rx):
    ref = posq_ref.posq_ref(s["group_ptr"], s["rx0"], s["rx1"], s["tdoa"], s["snr"], s["table"], weights, gate_m, ratio, min_rx)
    ptr = s["group_ptr"]
    n = len(ptr) - 1
    full_star, task_star = np.full((n, 2), np.nan), np.full((len(ref["task_rx"]), 2), np.nan)
    for g in range(n):
        rows = np.arange(ptr[g], ptr[g + 1])
        full_star[g] = star_of(s, weights, rows, np.ones(len(rows), bool), ref["full_pos"][g], ref["full_status"][g])
        for t in range(ref["task_ptr"][g], ref["task_ptr"][g + 1]):
            r = ref["task_rx"][t]
            use = (s["rx0"][rows] != r) & (s["rx1"][rows] != r)
            task_star[t] = star_of(s, weights, rows, use, ref["task_pos"][t], ref["task_status"][t])
    err = np.concatenate([np.abs(ref["full_pos"] - full_star).max(axis=1), np.abs(ref["task_pos"] - task_star).max(axis=1)])
    assert np.isfinite(err).sum() >= n, "most tasks have an exact minimiser"
    ref_err_max = float(np.nanmax(err))
    assert ref_err_max < 1e-9, ref_err_max
    ids = np.asarray(ids, dtype=np.int32)
    path = os.path.join(posq_golden.GOLDEN, name + ".npz")
    np.savez_compressed(
        path, rx_ids=ids, rx_xy=s["table"], group_ptr=ptr, rx0=ids[s["rx0"]], rx1=ids[s["rx1"]], tdoa=s["tdoa"], snr=s["snr"],
        weights=np.zeros(0) if weights is None else weights, planted=np.where(s["planted"] >= 0, ids[np.maximum(s["planted"], 0)], -1),
        group_id=np.arange(n, dtype=np.int32) * 3 + 100, group_timestamp=1.7e9 + 0.25 * np.arange(n), group_tx=np.full(n, 7, np.int32),
        gate_m=gate_m, ratio=ratio, min_rx=min_rx, full_x_star=full_star, task_x_star=task_star, ref_err_max=ref_err_max,
        ref_flags=ref["flags"], ref_excluded=ref["counts"][:, 2], ref_task_ptr=ref["task_ptr"], ref_pos=ref["pos"], ref_rms=ref["rms"])
    print("%s: %d groups, %d rows, %d flagged, %d tasks, ref_err_max %.3g m, %d bytes" % (
        name, n, ptr[-1], int((ref["flags"] & 1).sum()), len(ref["task_rx"]), ref_err_max, os.path.getsize(path)))
    return ref


def fault6():
    s = posq_golden.scene(seed=2, n_rx=6, n_groups=48, noise=0.3, delay=150.0, every=3)
    ref = make("posq_fault6", s, [3, 5, 8, 13, 21, 34], None, 3.0, 0.5, 5)
    # the condition on the inputs: the statement alone names the planted receiver in every affected group, touches
    # no clean group, and repairs the positions
    np.testing.assert_array_equal(ref["counts"][:, 2], s["planted"])
    np.testing.assert_array_equal((ref["flags"] & 1) != 0, s["planted"] >= 0)
    np.testing.assert_array_equal((ref["flags"] & 2) != 0, s["planted"] >= 0)
    assert int((s["planted"] >= 0).sum()) == 16 and ref["rms"][:, 1].max() < 0.9, ref["rms"][:, 1].max()


def weighted7():
    s = posq_golden.scene(seed=5, n_rx=7, n_groups=24, noise=0.3, delay=150.0, every=4, keep=0.8)
    weights = s["snr"].copy()
    weights[::11] = 0.0
    make("posq_weighted7", s, [2, 4, 6, 9, 12, 40, 41], weights, 3.0, 0.5, 5)


if __name__ == "__main__":
    os.makedirs(posq_golden.GOLDEN, exist_ok=True)
    fault6()
    weighted7()
