"""The device's solver for receivers with three coordinates (thrifty_amd/csrc/pos3_lm.hpp) restated in plain
NumPy, one group at a time: the same iteration, the same decisions, the same stopping rule and statuses as
tests/pos_ref.py, with the transmitter's height known (unknowns x, y) or free (unknowns x, y, z).  Sums over rows
are NumPy's here and 8-lane trees on the device, and the step on the free axes is numpy.linalg.solve here and a
cofactor expansion there, so iterates agree to rounding, not to the bit -- except the snr mean, whose order of
operations is the device's."""
import numpy as np

from pos_ref import (AT_BOUND, C, GAUSS_NEWTON_GATE, MAX_DIST, MU_MAX, MU_START, NONFINITE, OK, STEP_TOL, UNCONVERGED,
                     UNDERDETERMINED, team_sum)

KNOWN_HEIGHT, FREE_Z = 0, 1


def evaluate(p, a, b, tc, n):
    """(F, A[n, n], g[n]) at p (three entries; the first n are unknowns)."""
    with np.errstate(all="ignore"):
        va, vb = a - p, b - p
        da = np.sqrt((va[:, 0] * va[:, 0] + va[:, 1] * va[:, 1]) + va[:, 2] * va[:, 2])
        db = np.sqrt((vb[:, 0] * vb[:, 0] + vb[:, 1] * vb[:, 1]) + vb[:, 2] * vb[:, 2])
        res = tc - (da - db)
        grad = (va / da[:, None] - vb / db[:, None])[:, :n]
        return float(np.sum(res * res)), grad.T @ grad, grad.T @ res


def dops_of(normal):
    """(dop, hdop, vdop) of a 2 x 2 (the height is known: vdop = 0) or 3 x 3 normal matrix, the device's
    closed forms; -1 where the determinant is 0 or not finite."""
    with np.errstate(all="ignore"):
        s = np.asarray(normal, dtype=np.float64)
        if s.shape == (2, 2):
            det = s[0, 0] * s[1, 1] - s[0, 1] * s[0, 1]
            if det == 0.0 or not np.isfinite(det):
                return -1.0, -1.0, 0.0
            dop = float(np.sqrt((s[0, 0] + s[1, 1]) / det))
            return dop, dop, 0.0
        c00 = s[1, 1] * s[2, 2] - s[1, 2] * s[1, 2]
        c01 = s[0, 2] * s[1, 2] - s[0, 1] * s[2, 2]
        c02 = s[0, 1] * s[1, 2] - s[0, 2] * s[1, 1]
        c11 = s[0, 0] * s[2, 2] - s[0, 2] * s[0, 2]
        c22 = s[0, 0] * s[1, 1] - s[0, 1] * s[0, 1]
        det = (s[0, 0] * c00 + s[0, 1] * c01) + s[0, 2] * c02
        if det == 0.0 or not np.isfinite(det):
            return -1.0, -1.0, -1.0
        i00, i11, i22 = c00 / det, c11 / det, c22 / det
        return float(np.sqrt((i00 + i11) + i22)), float(np.sqrt(i00 + i11)), float(np.sqrt(i22))


def box_of(table, mode, z_range=None):
    lo, hi = table.min(axis=0) - MAX_DIST, table.max(axis=0) + MAX_DIST
    if mode == FREE_Z and z_range is not None:
        lo[2], hi[2] = z_range
    return lo, hi


def pos3_ref(rx0, rx1, tdoa, snr, table, mode, height=0.0, x0=(0.1, 0.1, 0.0), z_range=None, max_iter=100):
    """One group: dense receiver indices rx0 / rx1 into table[n_rx, 3] ->
    (pos[3], dop, hdop, vdop, rms, snr, status, iters)."""
    table = np.asarray(table, dtype=np.float64)
    rx0, rx1 = np.asarray(rx0, dtype=np.int64), np.asarray(rx1, dtype=np.int64)
    m, n = len(rx0), (3 if mode == FREE_Z else 2)
    shift = np.array([0.0, 0.0, 0.0 if mode == FREE_Z else height])     # the device: az = rz - h, a constant
    a, b = table[rx0].reshape(m, 3) - shift, table[rx1].reshape(m, 3) - shift
    with np.errstate(all="ignore"):
        tc = np.asarray(tdoa, dtype=np.float64) * C
        snr_mean = float(np.float64(team_sum(snr)) / np.float64(m))
    lo, hi = box_of(table, mode, z_range)
    lo, hi = lo[:n], hi[:n]
    p = np.array([x0[0], x0[1], x0[2] if mode == FREE_Z else 0.0], dtype=np.float64)
    cur = evaluate(p, a, b, tc, n)

    def result(status, iters):
        with np.errstate(all="ignore"):
            rms = float(np.sqrt(np.float64(cur[0]) / np.float64(m)))
        return (p + shift,) + dops_of(cur[1]) + (rms, snr_mean, status, iters)

    if len(set(rx0.tolist()) | set(rx1.tolist())) < n + 1:
        return result(UNDERDETERMINED, 0)
    if not (np.isfinite(cur[0]) and np.all(np.isfinite(cur[1])) and np.all(np.isfinite(cur[2]))):
        return result(NONFINITE, 0)
    status, iters = UNCONVERGED, 0
    mu, nu = MU_START * float(np.max(np.diag(cur[1]))), 2.0
    with np.errstate(all="ignore"):
        for it in range(max_iter):
            F, A, g = cur
            iters = it + 1
            q = p[:n]
            zero_grad = float(np.max(np.abs(g))) == 0.0
            hold = np.array([(q[k] <= lo[k] and g[k] > 0.0) or (q[k] >= hi[k] and g[k] < 0.0) for k in range(n)])
            scale = float(np.sqrt(np.sum(q * q))) + 1.0
            free = np.flatnonzero(~hold)

            def step(damp):
                h = np.zeros(n)
                if len(free):
                    try:
                        h[free] = np.linalg.solve((A + damp * np.eye(n))[np.ix_(free, free)], -g[free])
                    except np.linalg.LinAlgError:
                        h[free] = np.nan
                h = np.minimum(np.maximum(q + h, lo), hi) - q       # fmax / fmin: a NaN gives the bound
                return h, float(np.sqrt(np.sum(h * h)))

            h, length = step(0.0)
            gauss_newton = length <= GAUSS_NEWTON_GATE * scale
            if not gauss_newton:
                h, length = step(mu)
            trial_p = p.copy()
            trial_p[:n] = q + h
            trial = evaluate(trial_p, a, b, tc, n)
            if zero_grad or hold.all():
                status = OK
                break
            if not (np.isfinite(trial[0]) and np.all(np.isfinite(trial[1])) and np.all(np.isfinite(trial[2]))) or not np.isfinite(length):
                status = NONFINITE
                break
            if gauss_newton or trial[0] < F:
                if not gauss_newton:
                    pred = -(2.0 * float(h @ g) + float(h @ A @ h))
                    ratio = 2.0 * (np.float64(F - trial[0]) / np.float64(pred)) - 1.0
                    shrink = 1.0 - ratio * ratio * ratio
                    mu *= 1.0 / 3.0 if np.isnan(shrink) else min(max(1.0 / 3.0, float(shrink)), 2.0)
                    nu = 2.0
                p, cur = trial_p, trial
                if length <= STEP_TOL * scale:
                    status = OK
                    break
            else:
                mu, nu = min(mu * nu, MU_MAX), min(nu * 2.0, MU_MAX)
    if status == OK and (np.any(p[:n] <= lo) or np.any(p[:n] >= hi)):
        status = AT_BOUND
    return result(status, iters)


def pos3_ref_groups(group_ptr, rx0, rx1, tdoa, snr, table, mode, group_h=None, x0=(0.1, 0.1, 0.0), z_range=None, max_iter=100):
    """All groups -> dict of the columns `thrifty_amd._native.pos3` returns."""
    ptr = np.asarray(group_ptr).tolist()
    res = [pos3_ref(rx0[s:e], rx1[s:e], tdoa[s:e], snr[s:e], table, mode, 0.0 if group_h is None else float(group_h[k]),
                    x0, z_range, max_iter) for k, (s, e) in enumerate(zip(ptr[:-1], ptr[1:]))]
    out = {"pos": np.array([r[0] for r in res], dtype=np.float64).reshape(len(res), 3)}
    for col, key in enumerate(("dop", "hdop", "vdop", "rms", "snr"), start=1):
        out[key] = np.array([r[col] for r in res], dtype=np.float64)
    out["status"] = np.array([r[6] for r in res], dtype=np.int32)
    out["iters"] = np.array([r[7] for r in res], dtype=np.int32)
    return out
