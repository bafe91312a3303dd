"""thr_posq (thrifty_amd/csrc/posq.hip) stated in plain NumPy: pos_ref's iteration with weights and a row
subset (a TASK), then flag, candidates, choice, residuals, q and the ellipse.  Sums over rows are NumPy's here
and 8-lane trees on the device, so iterates agree to rounding, not to the bit -- except the weights' factor
m_used / sum w, whose order of operations is the device's (pos_ref.team_sum over the task's rows)."""
import numpy as np

from pos_ref import (AT_BOUND, C, GAUSS_NEWTON_GATE, MAX_DIST, MU_MAX, MU_START, NONFINITE, OK, STEP_TOL, UNCONVERGED,
                     UNDERDETERMINED, dop_of, team_sum)

INCONSISTENT, EXCLUDED, NO_CANDIDATE = 1, 2, 4


def task_weights(weights, use):
    """w_i * (m_used / sum of the used w), the sum in team order, then one division; None without weights."""
    if weights is None:
        return None
    with np.errstate(all="ignore"):
        w = np.asarray(weights, dtype=np.float64)
        return np.where(use, w * (np.float64(int(np.sum(use))) / np.float64(team_sum(w[use]))), 0.0)


def evaluate(p, a, b, tc, w=None):
    """(F, A00, A01, A11, g0, g1) at p; every term times w_i where weights are given."""
    with np.errstate(all="ignore"):
        da_v, db_v = a - p, b - p
        da, db = np.sqrt(np.sum(da_v * da_v, axis=1)), np.sqrt(np.sum(db_v * db_v, axis=1))
        res = tc - (da - db)
        gx, gy = (da_v / da[:, None] - db_v / db[:, None]).T
        terms = (res * res, gx * gx, gx * gy, gy * gy, gx * res, gy * res)
        return tuple(float(np.sum(t if w is None else w * t)) for t in terms)


def residuals(p, rx0, rx1, tdoa, table):
    """tdoa c - (|rx0 - p| - |rx1 - p|) per row: add_row's expression."""
    table = np.asarray(table, dtype=np.float64)
    with np.errstate(all="ignore"):
        va, vb = table[rx0] - p, table[rx1] - p
        da = np.sqrt(va[:, 0] * va[:, 0] + va[:, 1] * va[:, 1])
        db = np.sqrt(vb[:, 0] * vb[:, 0] + vb[:, 1] * vb[:, 1])
        return np.asarray(tdoa, dtype=np.float64) * C - (da - db)


def q_of(s):
    """inv(A) as (a11 / det, -a01 / det, a00 / det); NaN under dop_of's determinant rule."""
    with np.errstate(all="ignore"):
        det = np.float64(s[1] * s[3] - s[2] * s[2])
        if det == 0.0 or not np.isfinite(det):
            return np.full(3, np.nan)
        return np.array([s[3] / det, -s[2] / det, s[1] / det])


def solve_task(rx0, rx1, tdoa, table, weights=None, use=None, x0=(0.1, 0.1), max_iter=100):
    """One task: the rows of a group where `use` holds -> dict(pos, dop, q, rms, status, iters, nrx, rows, sums)."""
    table = np.asarray(table, dtype=np.float64)
    rx0, rx1 = np.asarray(rx0, dtype=np.int64), np.asarray(rx1, dtype=np.int64)
    use = np.ones(len(rx0), dtype=bool) if use is None else np.asarray(use, dtype=bool)
    w = task_weights(weights, use)
    w = None if w is None else w[use]
    m = int(use.sum())
    a, b = table[rx0[use]].reshape(m, 2), table[rx1[use]].reshape(m, 2)
    with np.errstate(all="ignore"):
        tc = np.asarray(tdoa, dtype=np.float64)[use] * C
    lo, hi = table.min(axis=0) - MAX_DIST, table.max(axis=0) + MAX_DIST
    p = np.array(x0, dtype=np.float64)
    cur = evaluate(p, a, b, tc, w)
    nrx = len(set(rx0[use].tolist()) | set(rx1[use].tolist()))
    status, iters = UNCONVERGED, 0
    if nrx < 3:
        status, max_iter = UNDERDETERMINED, 0
    elif not np.all(np.isfinite(cur)):
        status, max_iter = NONFINITE, 0
    mu, nu = MU_START * max(cur[1], cur[3]), 2.0
    with np.errstate(all="ignore"):
        for it in range(max_iter):
            F, a00, a01, a11, g0, g1 = cur
            iters = it + 1
            zero_grad = max(abs(g0), abs(g1)) == 0.0
            hold = [(p[k] <= lo[k] and g > 0.0) or (p[k] >= hi[k] and g < 0.0) for k, g in ((0, g0), (1, g1))]
            scale = float(np.sqrt(p[0] * p[0] + p[1] * p[1])) + 1.0

            def step(damp):
                aa, dd = a00 + damp, a11 + damp
                if hold[0] or hold[1]:
                    h = np.array([0.0 if hold[0] else -g0 / np.float64(aa), 0.0 if hold[1] else -g1 / np.float64(dd)])
                else:
                    det = np.float64(aa * dd - a01 * a01)
                    h = np.array([(a01 * g1 - dd * g0) / det, (a01 * g0 - aa * g1) / det])
                h = np.minimum(np.maximum(p + h, lo), hi) - p       # fmax / fmin: a NaN gives the bound
                return h, float(np.sqrt(h[0] * h[0] + h[1] * h[1]))

            h, length = step(0.0)
            gauss_newton = length <= GAUSS_NEWTON_GATE * scale
            if not gauss_newton:
                h, length = step(mu)
            trial_p = p + h
            trial = evaluate(trial_p, a, b, tc, w)
            if zero_grad or (hold[0] and hold[1]):
                status = OK
                break
            if not np.all(np.isfinite(trial)) or not np.isfinite(length):
                status = NONFINITE
                break
            if gauss_newton or trial[0] < F:
                if not gauss_newton:
                    pred = -(2.0 * (h[0] * g0 + h[1] * g1) + (h[0] * (a00 * h[0] + a01 * h[1]) + h[1] * (a01 * h[0] + a11 * h[1])))
                    q = 2.0 * (np.float64(F - trial[0]) / np.float64(pred)) - 1.0
                    shrink = 1.0 - q * q * q
                    mu *= 1.0 / 3.0 if np.isnan(shrink) else min(max(1.0 / 3.0, float(shrink)), 2.0)
                    nu = 2.0
                p, cur = trial_p, trial
                if length <= STEP_TOL * scale:
                    status = OK
                    break
            else:
                mu, nu = min(mu * nu, MU_MAX), min(nu * 2.0, MU_MAX)
        if status == OK and (np.any(p <= lo) or np.any(p >= hi)):
            status = AT_BOUND
        rms = float(np.sqrt(np.float64(cur[0]) / np.float64(m)))
    return {"pos": p, "dop": dop_of(cur), "q": q_of(cur), "rms": rms, "status": status, "iters": iters, "nrx": nrx,
            "rows": m, "sums": cur}


def choose(rms_full, flagged, task_rx, task_rms, task_status, task_nrx, ratio, min_rx):
    """The rule of kernel E for one group -> (flags, position of the chosen candidate or -1)."""
    if not flagged:
        return 0, -1
    best = -1
    for t in range(len(task_rx)):
        if task_status[t] == OK and task_nrx[t] >= min_rx - 1 and (best < 0 or task_rms[t] < task_rms[best]):
            best = t
    if best >= 0 and task_rms[best] <= np.float64(ratio) * np.float64(rms_full):
        return INCONSISTENT | EXCLUDED, best
    return INCONSISTENT | NO_CANDIDATE, -1


def is_flagged(status, nrx, rms_full, gate_m, min_rx):
    return bool(gate_m > 0.0 and status not in (UNDERDETERMINED, NONFINITE) and nrx >= min_rx and rms_full > gate_m)


def posq_ref(group_ptr, rx0, rx1, tdoa, snr, table, weights=None, gate_m=0.0, ratio=0.5, min_rx=5, x0=(0.1, 0.1),
             max_iter=100):
    """All groups -> dict with the names of `thrifty_amd._native.POSQ_OUTPUTS` (dense receiver indices)."""
    ptr = np.asarray(group_ptr).tolist()
    rx0, rx1 = np.asarray(rx0, dtype=np.int64), np.asarray(rx1, dtype=np.int64)
    tdoa, snr = np.asarray(tdoa, dtype=np.float64), np.asarray(snr, dtype=np.float64)
    n = len(ptr) - 1
    out = {"pos": np.zeros((n, 2)), "dop": np.zeros(n), "status": np.zeros(n, np.int32), "iters": np.zeros(n, np.int32),
           "q": np.zeros((n, 3)), "rms": np.zeros((n, 2)), "counts": np.zeros((n, 3), np.int32), "flags": np.zeros(n, np.int32),
           "full_pos": np.zeros((n, 2)), "full_status": np.zeros(n, np.int32), "snr": np.zeros(n),
           "residual": np.zeros(len(rx0)), "used": np.zeros(len(rx0), np.uint8), "task_ptr": np.zeros(n + 1, np.int64)}
    tasks = {"task_rx": [], "task_pos": [], "task_rms": [], "task_status": [], "task_nrx": [], "task_iters": []}
    for g, (s, e) in enumerate(zip(ptr[:-1], ptr[1:])):
        cols = (rx0[s:e], rx1[s:e], tdoa[s:e], table)
        w = None if weights is None else np.asarray(weights, dtype=np.float64)[s:e]
        full = solve_task(*cols, weights=w, x0=x0, max_iter=max_iter)
        with np.errstate(all="ignore"):
            out["snr"][g] = np.float64(team_sum(snr[s:e])) / np.float64(e - s)
        out["full_pos"][g], out["full_status"][g] = full["pos"], full["status"]
        cands, names = [], []
        if is_flagged(full["status"], full["nrx"], full["rms"], gate_m, min_rx):
            names = sorted(set(rx0[s:e].tolist()) | set(rx1[s:e].tolist()))
            cands = [solve_task(*cols, weights=w, use=(rx0[s:e] != r) & (rx1[s:e] != r), x0=x0, max_iter=max_iter) for r in names]
        flags, best = choose(full["rms"], bool(names), names, [c["rms"] for c in cands], [c["status"] for c in cands],
                             [c["nrx"] for c in cands], ratio, min_rx)
        chosen, excluded = (cands[best], names[best]) if best >= 0 else (full, -1)
        out["pos"][g], out["dop"][g], out["q"][g] = chosen["pos"], chosen["dop"], chosen["q"]
        out["status"][g], out["iters"][g] = chosen["status"], chosen["iters"]
        out["rms"][g] = full["rms"], chosen["rms"]
        out["counts"][g] = chosen["nrx"], chosen["rows"], excluded
        out["flags"][g] = flags
        out["residual"][s:e] = residuals(chosen["pos"], rx0[s:e], rx1[s:e], tdoa[s:e], table)
        out["used"][s:e] = (rx0[s:e] != excluded) & (rx1[s:e] != excluded)
        out["task_ptr"][g + 1] = out["task_ptr"][g] + len(cands)
        tasks["task_rx"] += names
        for c in cands:
            tasks["task_pos"].append(c["pos"]), tasks["task_rms"].append(c["rms"]), tasks["task_status"].append(c["status"])
            tasks["task_nrx"].append(c["nrx"]), tasks["task_iters"].append(c["iters"])
    out["task_rx"] = np.array(tasks["task_rx"], dtype=np.int32)
    out["task_pos"] = np.array(tasks["task_pos"], dtype=np.float64).reshape(len(tasks["task_rx"]), 2)
    out["task_rms"] = np.array(tasks["task_rms"], dtype=np.float64)
    for name in ("task_status", "task_nrx", "task_iters"):
        out[name] = np.array(tasks[name], dtype=np.int32)
    return out


def ellipse(q):
    """(q00, q01, q11) -> (xdop, ydop, major, minor, angle in degrees) through numpy's symmetric eigenvalues."""
    q00, q01, q11 = (float(v) for v in q)
    if not np.all(np.isfinite([q00, q01, q11])):
        return (np.nan,) * 5
    low, high = np.linalg.eigvalsh(np.array([[q00, q01], [q01, q11]]))
    return (np.sqrt(q00), np.sqrt(q11), np.sqrt(high), np.sqrt(max(low, 0.0)),
            float(np.degrees(0.5 * np.arctan2(2.0 * q01, q00 - q11))))
