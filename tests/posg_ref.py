"""The global position solve (thrifty_amd/csrc/posg.hip, `thr_posg`) stated in NumPy: the definitions of
include/thrifty_hip.h on top of `pos_ref.pos_ref(x0=start)`.  The surface, its local minima and the starts are the
device's operations one by one (the same bits, as far as NumPy's sqrt and the device's agree); a task's iterates agree
with the device's to rounding only (pos_ref's sums are NumPy's), so the discrete outputs are comparable where the
fixtures keep their margins (tests/golden/make_golden_posg.py).  `pick` is the choice rule alone, on any task outputs."""
import numpy as np

import pos_ref

MOVED, AMBIGUOUS, NO_MINIMUM = 1, 2, 4
NO_TASK = -1
NEIGHBOURS = [(dj, di) for dj in (-1, 0, 1) for di in (-1, 0, 1) if (dj, di) != (0, 0)]


def centres(table, margin_m, grid):
    """(cx, cy): the cell centres of the search area, in exactly the header's form."""
    table = np.asarray(table, dtype=np.float64)
    lo, hi = table.min(axis=0) - np.float64(margin_m), table.max(axis=0) + np.float64(margin_m)
    return tuple(lo[k] + (np.arange(grid) + 0.5) * ((hi[k] - lo[k]) / grid) for k in (0, 1))


def surface(rx0, rx1, tdoa, table, cx, cy):
    """F[j, i]: one accumulator per cell over the rows in order."""
    table = np.asarray(table, dtype=np.float64)
    px, py = np.meshgrid(cx, cy)                # px[j, i] = cx[i]
    acc = np.zeros(px.shape)
    with np.errstate(all="ignore"):
        for r0, r1, t in zip(np.asarray(rx0).tolist(), np.asarray(rx1).tolist(), np.asarray(tdoa, dtype=np.float64)):
            ax, ay, bx, by = table[r0, 0] - px, table[r0, 1] - py, table[r1, 0] - px, table[r1, 1] - py
            res = t * pos_ref.C - (np.sqrt(ax * ax + ay * ay) - np.sqrt(bx * bx + by * by))
            acc = acc + res * res
    return acc


def local_minima(F):
    """bool[j, i]: F[c] < F[n], or F[c] == F[n] and n > c, for every neighbour; outside the grid: F[c] < +inf."""
    G = F.shape[0]
    cell = np.arange(G * G).reshape(G, G)
    padded = np.full((G + 2, G + 2), np.inf)
    padded[1:-1, 1:-1] = F
    number = np.full((G + 2, G + 2), -1)
    number[1:-1, 1:-1] = cell
    ok = np.ones((G, G), dtype=bool)
    with np.errstate(invalid="ignore"):
        for dj, di in NEIGHBOURS:
            fn, n = padded[1 + dj:G + 1 + dj, 1 + di:G + 1 + di], number[1 + dj:G + 1 + dj, 1 + di:G + 1 + di]
            ok &= (F < fn) | ((F == fn) & (n > cell))
    return ok


def lowest(F, minima, starts):
    """(cells int32[starts], F float64[starts]): the local minima with the smallest (F, c); -1 and NaN in unused slots."""
    cells = np.flatnonzero(minima.ravel())
    order = cells[np.lexsort((cells, F.ravel()[cells]))][:starts]
    out_c, out_f = np.full(starts, -1, dtype=np.int32), np.full(starts, np.nan)
    out_c[:len(order)], out_f[:len(order)] = order, F.ravel()[order]
    return out_c, out_f


def pick(task_pos, task_rms, task_status, merge_m, ratio, floor_m):
    """The choice of one group from its tasks' pos[T, 2], rms[T], status[T] -> dict(task, pos, rms, pos2, rms2, n_minima,
    flags, duplicate[T])."""
    T = len(task_rms)
    elig = np.asarray(task_status) == pos_ref.OK
    with np.errstate(invalid="ignore"):
        before = np.array([[bool(elig[u]) and u != t and (task_rms[u] < task_rms[t] or (task_rms[u] == task_rms[t] and u < t))
                            for u in range(T)] for t in range(T)])
        d = task_pos[:, None, :] - task_pos[None, :, :]
        near = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) <= merge_m
        dup = np.any(before & near, axis=1)
        first = elig & ~np.any(before, axis=1)
        best = int(np.flatnonzero(first)[0]) if first.any() else -1
        rest = [t for t in range(T) if elig[t] and not dup[t] and not first[t]]
        second = min(rest, key=lambda t: (task_rms[t], t)) if rest else -1
        chosen = max(best, 0)
        flags = NO_MINIMUM if best < 0 else 0
        d0 = task_pos[chosen] - task_pos[0]
        if not elig[0] or not (np.sqrt(d0[0] * d0[0] + d0[1] * d0[1]) <= merge_m):
            flags |= MOVED
        if second >= 0 and task_rms[second] <= np.fmax(np.float64(ratio) * task_rms[chosen], np.float64(floor_m)):
            flags |= AMBIGUOUS
    return {"task": chosen, "pos": task_pos[chosen].copy(), "rms": task_rms[chosen],
            "pos2": task_pos[second].copy() if second >= 0 else np.full(2, np.nan),
            "rms2": task_rms[second] if second >= 0 else np.nan, "n_minima": int(np.count_nonzero(elig & ~dup)),
            "flags": flags, "duplicate": dup & elig}


def pick_groups(task_pos, task_rms, task_status, merge_m, ratio, floor_m):
    """`pick` over task arrays [groups, T(, 2)] -> dict of arrays."""
    res = [pick(p, r, s, merge_m, ratio, floor_m) for p, r, s in zip(task_pos, task_rms, task_status)]
    n = len(res)
    return {"task": np.array([r["task"] for r in res], dtype=np.int32), "pos": np.array([r["pos"] for r in res]).reshape(n, 2),
            "rms": np.array([r["rms"] for r in res], dtype=np.float64), "pos2": np.array([r["pos2"] for r in res]).reshape(n, 2),
            "rms2": np.array([r["rms2"] for r in res], dtype=np.float64),
            "n_minima": np.array([r["n_minima"] for r in res], dtype=np.int32),
            "flags": np.array([r["flags"] for r in res], dtype=np.int32)}


def solve_task(rx0, rx1, tdoa, snr, table, start, max_iter):
    """One task: pos_ref from `start` -> (pos, dop, rms, status, iters, snr)."""
    p, dop, snr_mean, status, iters = pos_ref.pos_ref(rx0, rx1, tdoa, snr, table, x0=start, max_iter=max_iter)
    m = len(rx0)
    table = np.asarray(table, dtype=np.float64)
    with np.errstate(all="ignore"):
        F = pos_ref.evaluate(p, table[np.asarray(rx0, dtype=np.int64)].reshape(m, 2), table[np.asarray(rx1, dtype=np.int64)].reshape(m, 2),
                             np.asarray(tdoa, dtype=np.float64) * pos_ref.C)[0]
        rms = float(np.sqrt(np.float64(F) / np.float64(m)))
    return p, dop, rms, status, iters, snr_mean


def posg_ref(group_ptr, rx0, rx1, tdoa, snr, table, margin_m, grid=32, starts=4, merge_m=1.0, ratio=2.0, floor_m=0.0,
             x0=(0.1, 0.1), max_iter=100, maps=True):
    """All groups -> dict of the outputs of `thrifty_amd._native.posg` (`map` / `map_min` for every group when `maps`)."""
    ptr = np.asarray(group_ptr).tolist()
    table = np.asarray(table, dtype=np.float64)
    n, T = len(ptr) - 1, starts + 1
    cx, cy = centres(table, margin_m, grid)
    out = {"task_pos": np.full((n, T, 2), np.nan), "task_dop": np.full((n, T), np.nan), "task_rms": np.full((n, T), np.nan),
           "task_status": np.full((n, T), NO_TASK, dtype=np.int32), "task_iters": np.zeros((n, T), dtype=np.int32),
           "start_cell": np.full((n, starts), -1, dtype=np.int32), "start_f": np.full((n, starts), np.nan),
           "n_local": np.zeros(n, dtype=np.int32), "snr": np.zeros(n), "map": np.full((n, grid, grid), np.nan),
           "map_min": np.zeros((n, grid, grid), dtype=np.uint8)}
    for g, (s, e) in enumerate(zip(ptr[:-1], ptr[1:])):
        cols = (rx0[s:e], rx1[s:e], tdoa[s:e], snr[s:e], table)

        def run(t, start):
            p, dop, rms, status, iters, snr_mean = solve_task(*cols, start, max_iter)
            out["task_pos"][g, t], out["task_dop"][g, t], out["task_rms"][g, t] = p, dop, rms
            out["task_status"][g, t], out["task_iters"][g, t] = status, iters
            return snr_mean

        if e == s:
            out["task_pos"][g, 0], out["task_dop"][g, 0], out["task_status"][g, 0] = x0, -1.0, pos_ref.UNDERDETERMINED
            out["snr"][g] = np.nan
            continue
        out["snr"][g] = run(0, x0)
        if out["task_status"][g, 0] in (pos_ref.UNDERDETERMINED, pos_ref.NONFINITE):
            continue
        F = surface(*cols[:3], table, cx, cy)
        minima = local_minima(F)
        out["n_local"][g] = int(minima.sum())
        out["start_cell"][g], out["start_f"][g] = lowest(F, minima, starts)
        if maps:
            out["map"][g], out["map_min"][g] = F, minima
        for k, cell in enumerate(out["start_cell"][g].tolist()):
            if cell >= 0:
                run(k + 1, (cx[cell % grid], cy[cell // grid]))
    out.update(pick_groups(out["task_pos"], out["task_rms"], out["task_status"], merge_m, ratio, floor_m))
    rows = np.arange(n)
    out["dop"], out["status"] = out["task_dop"][rows, out["task"]], out["task_status"][rows, out["task"]]
    out["cx"], out["cy"] = cx, cy
    if not maps:
        del out["map"], out["map_min"]
    return out
