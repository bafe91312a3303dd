"""The device's position solver (thrifty_amd/csrc/pos.hip) restated in plain NumPy, one group at a time:
the same iteration, the same decisions, the same stopping rule and statuses.  Sums over rows are
NumPy's here and 8-lane trees on the device, so iterates agree to rounding, not to the bit -- except the
1-D formula and the snr mean, whose order of operations is the device's."""
import numpy as np

C = 2.997e8
MAX_DIST = 10e3
STEP_TOL = 1e-13
GAUSS_NEWTON_GATE = 1e-4
MU_START = 1e-3
MU_MAX = 1e100
OK, UNDERDETERMINED, UNCONVERGED, AT_BOUND, NONFINITE = range(5)


def team_sum(values):
    """Lane j adds rows j, j + 8, ... in order; the eight lanes are added as xor 1, xor 2, mirror."""
    lanes = np.zeros(8)
    for i, v in enumerate(np.asarray(values, dtype=np.float64).tolist()):
        lanes[i % 8] += v
    pairs = lanes[0::2] + lanes[1::2]
    quads = pairs[0::2] + pairs[1::2]
    return float(quads[0] + quads[1])


def evaluate(p, a, b, tc):
    """(F, A00, A01, A11, g0, g1) at p."""
    with np.errstate(all="ignore"):
        da_v, db_v = a - p, b - p
        da, db = np.sqrt(np.sum(da_v * da_v, axis=1)), np.sqrt(np.sum(db_v * db_v, axis=1))
        res = tc - (da - db)
        gx, gy = (da_v / da[:, None] - db_v / db[:, None]).T
        return tuple(float(np.sum(t)) for t in (res * res, gx * gx, gx * gy, gy * gy, gx * res, gy * res))


def dop_of(s):
    with np.errstate(all="ignore"):
        det = s[1] * s[3] - s[2] * s[2]
        return -1.0 if det == 0.0 or not np.isfinite(det) else float(np.sqrt(np.float64(s[1] + s[3]) / det))


def pos_ref_1d(rx0, rx1, tdoa, snr, table, first_two=(0, 1)):
    x = np.asarray(table, dtype=np.float64)[:, 0]
    with np.errstate(all="ignore"):
        tdoa_pos = np.float64(tdoa[0]) * C
        both = x[first_two[0]] + x[first_two[1]]
        p = (both - tdoa_pos) / 2 if x[first_two[0]] > x[first_two[1]] else (both + tdoa_pos) / 2
        a, b = x[rx0[0]] - p, x[rx1[0]] - p
        s = (a / abs(a) - b / abs(b)) ** 2
        dop = -1.0 if s == 0.0 else float(np.sqrt(1.0 / s))
    return np.array([p]), dop, float(snr[0]), OK if np.isfinite(p) and np.isfinite(s) else NONFINITE, 0


def pos_ref(rx0, rx1, tdoa, snr, table, x0=(0.1, 0.1), max_iter=100, trace=None):
    """One group: dense receiver indices rx0 / rx1 into table[n_rx, 2] -> (pos, dop, snr, status, iters)."""
    table = np.asarray(table, dtype=np.float64)
    rx0, rx1 = np.asarray(rx0, dtype=np.int64), np.asarray(rx1, dtype=np.int64)
    if table.shape[1] == 1:
        return pos_ref_1d(rx0, rx1, tdoa, snr, table)
    m = len(rx0)
    a, b = table[rx0].reshape(m, 2), table[rx1].reshape(m, 2)
    with np.errstate(all="ignore"):
        tc = np.asarray(tdoa, dtype=np.float64) * C
        snr_mean = float(np.float64(team_sum(snr)) / np.float64(m))
    lo, hi = table.min(axis=0) - MAX_DIST, table.max(axis=0) + MAX_DIST
    p = np.array(x0, dtype=np.float64)
    cur = evaluate(p, a, b, tc)
    if len(set(rx0.tolist()) | set(rx1.tolist())) < 3:
        return p, dop_of(cur), snr_mean, UNDERDETERMINED, 0
    if not np.all(np.isfinite(cur)):
        return p, dop_of(cur), snr_mean, NONFINITE, 0
    status, iters = UNCONVERGED, 0
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
            trial = evaluate(trial_p, a, b, tc)
            if trace is not None:
                trace.append((it, gauss_newton, length, trial[0] < F))
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
    return p, dop_of(cur), snr_mean, status, iters


def pos_ref_groups(group_ptr, rx0, rx1, tdoa, snr, table, x0=(0.1, 0.1), max_iter=100):
    """All groups -> dict of the columns `thrifty_amd._native.pos` returns."""
    ptr = np.asarray(group_ptr).tolist()
    table = np.asarray(table, dtype=np.float64)
    res = [pos_ref(rx0[s:e], rx1[s:e], tdoa[s:e], snr[s:e], table, x0, max_iter) for s, e in zip(ptr[:-1], ptr[1:])]
    return {"pos": np.array([r[0] for r in res], dtype=np.float64).reshape(len(res), table.shape[1]),
            "dop": np.array([r[1] for r in res], dtype=np.float64), "snr": np.array([r[2] for r in res], dtype=np.float64),
            "status": np.array([r[3] for r in res], dtype=np.int32), "iters": np.array([r[4] for r in res], dtype=np.int32)}
