"""The coverage map (thrifty_amd/csrc/coverage.hip, include/thrifty_hip.h) restated in plain NumPy: the Philox4x32-10
generator in uint64 arithmetic, the normal, who hears a cell, the analytic columns, the synthesis of a trial's rows and
the per-cell reduction.  A trial's solve is tests/pos_ref.py's `pos_ref`, the statement of thr_pos.

What agrees to the bit with the device: the cell centres, the hearing masks, the rows' receivers, the distances
(the same float64 operations one by one), the generator's words and uniforms.  What agrees to rounding: the normal
(log and cos are library functions on both sides), hence the tdoas; the solve (pos_ref sums with NumPy, the device
with 8-lane trees); the analytic columns (`analytic` takes a dtype so that a test can evaluate the same formulas in
np.longdouble)."""
import numpy as np

from pos_ref import NONFINITE, OK, AT_BOUND, UNCONVERGED, pos_ref

C = 2.997e8
UNCOVERED, DEGENERATE, LOSSY = 1, 2, 4
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
TWO_PI = 6.283185307179586


def philox4x32_10(counter, key):
    """counter: uint array [..., 4], key: (k0, k1) -> uint64 array [..., 4] of 32-bit words."""
    c = [np.asarray(counter, dtype=np.uint64)[..., k] & MASK32 for k in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]        # 32 x 32 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1)


def uniforms(cells, trials, n_rx, seed):
    """(u1, u2)[len(cells), trials, n_rx] of the counters (c, t, r, 0); seed is the 64-bit key."""
    cells = np.asarray(cells, dtype=np.uint64)
    counter = np.zeros((len(cells), trials, n_rx, 4), dtype=np.uint64)
    counter[..., 0] = cells[:, None, None]
    counter[..., 1] = np.arange(trials, dtype=np.uint64)[None, :, None]
    counter[..., 2] = np.arange(n_rx, dtype=np.uint64)[None, None, :]
    w = philox4x32_10(counter, (seed & 0xFFFFFFFF, seed >> 32))
    return (w[..., 0].astype(np.float64) + 1.0) * 2.0 ** -32, w[..., 1].astype(np.float64) * 2.0 ** -32


def noise(cells, trials, sigma, seed):
    """n[len(cells), trials, n_rx] in metres."""
    sigma = np.asarray(sigma, dtype=np.float64)
    u1, u2 = uniforms(cells, trials, len(sigma), seed)
    return sigma * (np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI * u2))


def cell_centres(lo, hi, nx, ny):
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    return (lo[0] + (np.arange(nx) + 0.5) * ((hi[0] - lo[0]) / nx), lo[1] + (np.arange(ny) + 0.5) * ((hi[1] - lo[1]) / ny))


def hearing(table, cx, cy, range_m):
    """bool[cells, n_rx], cell c = j * nx + i."""
    table = np.asarray(table, dtype=np.float64)
    px, py = np.tile(cx, len(cy)), np.repeat(cy, len(cx))
    dx, dy = table[None, :, 0] - px[:, None], table[None, :, 1] - py[:, None]
    if range_m <= 0.0:
        return np.ones(dx.shape, dtype=bool)
    return np.sqrt(dx * dx + dy * dy) <= range_m


def mask_of(heard):
    return np.array([sum(1 << r for r in np.flatnonzero(row).tolist()) for row in heard], dtype=np.uint64)


def pairs(receivers):
    """The rows of a cell: all pairs a < b of its hearing receivers, a-major."""
    rx = list(receivers)
    return (np.array([a for i, a in enumerate(rx) for _ in rx[i + 1:]], dtype=np.int32),
            np.array([b for i, _ in enumerate(rx) for b in rx[i + 1:]], dtype=np.int32))


def analytic(table, sigma, p, receivers, dtype=np.float64, independent=False):
    """(dop, sxx, sxy, syy, rms, cond N) at p for the hearing `receivers`, every operation in `dtype`.
    independent=True is the WRONG prediction that treats the pairs' noises as independent (M = 2 sigma^2 N, one sigma)."""
    f = dtype
    xy, s, p = np.asarray(table, dtype=f), np.asarray(sigma, dtype=f), np.asarray(p, dtype=f)
    rx0, rx1 = pairs(receivers)
    nan = f(np.nan)
    with np.errstate(all="ignore"):
        d = xy - p
        e = d / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])[:, None]
        g = e[rx0] - e[rx1]
        n00, n01, n11 = f(0), f(0), f(0)
        for gx, gy in g:
            n00, n01, n11 = n00 + gx * gx, n01 + gx * gy, n11 + gy * gy
        det = n00 * n11 - n01 * n01
        if det == 0 or not np.isfinite(det):
            return f(-1), nan, nan, nan, nan, f(np.inf)
        dop = np.sqrt((n00 + n11) / det)
        m00, m01, m11 = f(0), f(0), f(0)
        for r in receivers:
            ux, uy = f(0), f(0)
            for b in receivers:
                if b != r:
                    ux, uy = ux + (e[r, 0] - e[b, 0]), uy + (e[r, 1] - e[b, 1])
            s2 = s[r] * s[r]
            m00, m01, m11 = m00 + s2 * (ux * ux), m01 + s2 * (ux * uy), m11 + s2 * (uy * uy)
        if independent:
            s2 = f(2) * s[receivers[0]] * s[receivers[0]]
            m00, m01, m11 = s2 * n00, s2 * n01, s2 * n11
        i00, i01, i11 = n11 / det, -n01 / det, n00 / det
        t00, t01 = i00 * m00 + i01 * m01, i00 * m01 + i01 * m11
        t10, t11 = i01 * m00 + i11 * m01, i01 * m01 + i11 * m11
        sxx, sxy, syy = t00 * i00 + t01 * i01, t00 * i01 + t01 * i11, t10 * i01 + t11 * i11
        half, root = (n00 + n11) / f(2), np.sqrt(((n00 - n11) / f(2)) ** 2 + n01 * n01)
        cond = (half + root) / (half - root)
    return dop, sxx, sxy, syy, np.sqrt(sxx + syy), cond


def synth(table, p, receivers, n):
    """One trial: (rx0, rx1, tdoa) for the noise n[n_rx] -- the device's operations one by one."""
    table = np.asarray(table, dtype=np.float64)
    rx0, rx1 = pairs(receivers)
    d = table - np.asarray(p, dtype=np.float64)
    dist = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    return rx0, rx1, ((dist[rx0] - dist[rx1]) + (n[rx0] - n[rx1])) / C


def error_of(pos, status, p):
    """(dx, dy, e) of one trial."""
    dx, dy = float(pos[0]) - float(p[0]), float(pos[1]) - float(p[1])
    if status == NONFINITE or not (np.isfinite(pos[0]) and np.isfinite(pos[1])):
        return dx, dy, np.inf
    return dx, dy, float(np.sqrt(np.float64(dx * dx + dy * dy)))


def lane_sum(values):
    """Lane l adds values l, l + 64, ... in order from 0.0; then lane[l] += lane[l + d] for d = 32, 16, .. 1."""
    lanes = np.zeros(64)
    for i, v in enumerate(np.asarray(values, dtype=np.float64).tolist()):
        lanes[i % 64] += v
    d = 32
    while d >= 1:
        lanes[:d] = lanes[:d] + lanes[d:2 * d]
        d //= 2
    return float(lanes[0])


def rank_indices(trials):
    """The positions of q50 and q95 in the sorted errors: ceil(p T) - 1 in integers."""
    return (trials + 1) // 2 - 1, (95 * trials + 99) // 100 - 1


def reduce_cell(dx, dy, err, status, iters, gross_m):
    """One covered cell's trials -> (counts[6], iters_sum, stats[8], lossy).  The sums add the GOOD trials in the lanes
    their trial number puts them in."""
    dx, dy, err = (np.asarray(v, dtype=np.float64) for v in (dx, dy, err))
    status = np.asarray(status)
    trials = len(err)
    good = (status == OK) & (err <= gross_m)
    n_good = int(good.sum())
    counts = np.array([np.sum(status == OK), np.sum(status == AT_BOUND), np.sum(status == UNCONVERGED),
                       np.sum(status == NONFINITE), n_good, trials - n_good], dtype=np.int32)
    stats = np.full(8, np.nan)
    if n_good:
        zero = lambda v: np.where(good, v, 0.0)     # noqa: E731  adding 0.0 to a lane changes nothing
        with np.errstate(all="ignore"):
            sums = [lane_sum(zero(v)) for v in (dx, dy, dx * dx, dx * dy, dy * dy)]
        stats[:5] = np.array(sums) / np.float64(n_good)
        stats[5] = np.sqrt(stats[2] + stats[4])
    order = np.sort(err)
    i50, i95 = rank_indices(trials)
    stats[6], stats[7] = order[i50], order[i95]
    return counts, int(np.sum(np.asarray(iters, dtype=np.int64))), stats, bool((trials - n_good) * 2 > trials)


def coverage_ref(table, sigma, lo, hi, nx, ny, gross_m, trials, range_m=0.0, seed=0, x0=(0.1, 0.1), max_iter=100):
    """The whole map -> dict of the device's per-cell outputs (flat, cell c = j * nx + i) plus the per-trial columns
    trial_pos[cells, T, 2], trial_status, trial_iters, trial_dx, trial_dy, trial_err (NaN / -1 for uncovered cells) and
    noise[cells, T, n_rx]."""
    table, sigma = np.asarray(table, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    cx, cy = cell_centres(lo, hi, nx, ny)
    heard = hearing(table, cx, cy, range_m)
    n_cells, n_rx = nx * ny, len(table)
    out = {"cx": cx, "cy": cy, "n_heard": heard.sum(axis=1).astype(np.int32), "heard_mask": mask_of(heard),
           "flags": np.zeros(n_cells, dtype=np.int32), "pred": np.full((n_cells, 5), np.nan),
           "cond": np.full(n_cells, np.nan), "counts": np.zeros((n_cells, 6), dtype=np.int32),
           "iters_sum": np.zeros(n_cells, dtype=np.int64), "stats": np.full((n_cells, 8), np.nan),
           "noise": noise(np.arange(n_cells), trials, sigma, seed),
           "trial_pos": np.full((n_cells, trials, 2), np.nan), "trial_status": np.full((n_cells, trials), -1, dtype=np.int32),
           "trial_iters": np.zeros((n_cells, trials), dtype=np.int32), "trial_dx": np.full((n_cells, trials), np.nan),
           "trial_dy": np.full((n_cells, trials), np.nan), "trial_err": np.full((n_cells, trials), np.nan)}
    for c in range(n_cells):
        receivers = np.flatnonzero(heard[c]).tolist()
        if len(receivers) < 3:
            out["flags"][c] = UNCOVERED
            continue
        p = (cx[c % nx], cy[c // nx])
        res = analytic(table, sigma, p, receivers)
        out["pred"][c], out["cond"][c] = res[:5], res[5]
        if res[0] == -1:
            out["flags"][c] |= DEGENERATE
        for t in range(trials):
            rx0, rx1, tdoa = synth(table, p, receivers, out["noise"][c, t])
            pos, _, _, status, iters = pos_ref(rx0, rx1, tdoa, np.ones(len(rx0)), table, x0, max_iter)
            out["trial_pos"][c, t], out["trial_status"][c, t], out["trial_iters"][c, t] = pos, status, iters
            out["trial_dx"][c, t], out["trial_dy"][c, t], out["trial_err"][c, t] = error_of(pos, status, p)
        counts, iters_sum, stats, lossy = reduce_cell(out["trial_dx"][c], out["trial_dy"][c], out["trial_err"][c],
                                                      out["trial_status"][c], out["trial_iters"][c], gross_m)
        out["counts"][c], out["iters_sum"][c], out["stats"][c] = counts, iters_sum, stats
        if lossy:
            out["flags"][c] |= LOSSY
    return out
