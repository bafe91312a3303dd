"""The global solve for receivers with three coordinates (thrifty_amd/csrc/posg3.hip, `thr_posg3`) stated in NumPy: the
definitions of include/thrifty_hip.h on top of `pos3_ref.pos3_ref(x0=start)`.  The volume, its local minima and the
starts are the device's operations one by one (the same bits, as far as NumPy's sqrt and the device's agree); a task's
iterates agree with the device's to rounding only (pos3_ref's sums are NumPy's), so the discrete outputs are comparable
where the fixtures keep their margins (tests/golden/make_golden_posg3.py).  `pick` is the choice rule alone, on any task
outputs."""
import numpy as np

import pos3_ref
from pos_ref import C, NONFINITE, OK, UNDERDETERMINED

MOVED, AMBIGUOUS, NO_MINIMUM, MIRROR = 1, 2, 4, 8
NO_TASK = -1
KNOWN_HEIGHT, FREE_Z = pos3_ref.KNOWN_HEIGHT, pos3_ref.FREE_Z
NEIGHBOURS = [(dk, dj, di) for dk in (-1, 0, 1) for dj in (-1, 0, 1) for di in (-1, 0, 1) if (dk, dj, di) != (0, 0, 0)]


def centres(table, margin_m, grid, z_grid=None, grid_z=1):
    """(cx, cy, cz): the cell centres of the search volume, in exactly the header's form; cz is None without `z_grid`."""
    table = np.asarray(table, dtype=np.float64)
    lo, hi = table[:, :2].min(axis=0) - np.float64(margin_m), table[:, :2].max(axis=0) + np.float64(margin_m)
    cx, cy = (lo[k] + (np.arange(grid) + 0.5) * ((hi[k] - lo[k]) / grid) for k in (0, 1))
    if z_grid is None:
        return cx, cy, None
    zlo, zhi = np.float64(z_grid[0]), np.float64(z_grid[1])
    return cx, cy, zlo + (np.arange(grid_z) + 0.5) * ((zhi - zlo) / grid_z)


def volume(rx0, rx1, tdoa, table, cx, cy, cz):
    """F[k, j, i]: one accumulator per cell over the rows in order; cz holds the planes' heights."""
    table = np.asarray(table, dtype=np.float64)
    pz, py, px = np.meshgrid(np.asarray(cz, dtype=np.float64), cy, cx, indexing="ij")       # px[k, j, i] = cx[i]
    acc = np.zeros(px.shape)
    with np.errstate(all="ignore"):
        for r0, r1, t in zip(np.asarray(rx0).tolist(), np.asarray(rx1).tolist(), np.asarray(tdoa, dtype=np.float64)):
            ax, ay, az = table[r0, 0] - px, table[r0, 1] - py, table[r0, 2] - pz
            bx, by, bz = table[r1, 0] - px, table[r1, 1] - py, table[r1, 2] - pz
            res = t * C - (np.sqrt((ax * ax + ay * ay) + az * az) - np.sqrt((bx * bx + by * by) + bz * bz))
            acc = acc + res * res
    return acc


def local_minima(F):
    """bool[k, j, i]: F[c] < F[n], or F[c] == F[n] and n > c, for every neighbour; outside the volume: F[c] < +inf."""
    gz, G = F.shape[0], F.shape[1]
    cell = np.arange(gz * G * G).reshape(gz, G, G)
    padded = np.full((gz + 2, G + 2, G + 2), np.inf)
    padded[1:-1, 1:-1, 1:-1] = F
    number = np.full((gz + 2, G + 2, G + 2), -1)
    number[1:-1, 1:-1, 1:-1] = cell
    ok = np.ones(F.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        for dk, dj, di in NEIGHBOURS:
            window = (slice(1 + dk, gz + 1 + dk), slice(1 + dj, G + 1 + dj), slice(1 + di, G + 1 + di))
            fn, n = padded[window], number[window]
            ok &= (F < fn) | ((F == fn) & (n > cell))
    return ok


def lowest(F, minima, starts):
    """(cells int32[starts], F float64[starts]): the local minima with the smallest (F, c); -1 and NaN in unused slots."""
    cells = np.flatnonzero(minima.ravel())
    order = cells[np.lexsort((cells, F.ravel()[cells]))][:starts]
    out_c, out_f = np.full(starts, -1, dtype=np.int32), np.full(starts, np.nan)
    out_c[:len(order)], out_f[:len(order)] = order, F.ravel()[order]
    return out_c, out_f


def pick(task_pos, task_rms, task_status, merge_m, ratio, floor_m, free_z):
    """The choice of one group from its tasks' pos[T, 3], rms[T], status[T] -> dict(task, pos, rms, pos2, rms2, n_minima,
    flags, duplicate[T])."""
    T = len(task_rms)
    elig = np.asarray(task_status) == OK
    with np.errstate(invalid="ignore"):
        before = np.array([[bool(elig[u]) and u != t and (task_rms[u] < task_rms[t] or (task_rms[u] == task_rms[t] and u < t))
                            for u in range(T)] for t in range(T)])
        d = task_pos[:, None, :] - task_pos[None, :, :]
        flat = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        apart = np.sqrt(flat + d[..., 2] * d[..., 2]) if free_z else np.sqrt(flat)
        near = apart <= merge_m
        dup = np.any(before & near, axis=1)
        first = elig & ~np.any(before, axis=1)
        best = int(np.flatnonzero(first)[0]) if first.any() else -1
        rest = [t for t in range(T) if elig[t] and not dup[t] and not first[t]]
        second = min(rest, key=lambda t: (task_rms[t], t)) if rest else -1
        chosen = max(best, 0)
        flags = NO_MINIMUM if best < 0 else 0
        if not elig[0] or not (apart[chosen, 0] <= merge_m):
            flags |= MOVED
        if second >= 0 and task_rms[second] <= np.fmax(np.float64(ratio) * task_rms[chosen], np.float64(floor_m)):
            flags |= AMBIGUOUS
            if free_z and np.sqrt(flat[second, chosen]) <= merge_m:
                flags |= MIRROR
    return {"task": chosen, "pos": task_pos[chosen].copy(), "rms": task_rms[chosen],
            "pos2": task_pos[second].copy() if second >= 0 else np.full(3, np.nan),
            "rms2": task_rms[second] if second >= 0 else np.nan, "n_minima": int(np.count_nonzero(elig & ~dup)),
            "flags": flags, "duplicate": dup & elig}


def pick_groups(task_pos, task_rms, task_status, merge_m, ratio, floor_m, free_z):
    """`pick` over task arrays [groups, T(, 3)] -> dict of arrays."""
    res = [pick(p, r, s, merge_m, ratio, floor_m, free_z) for p, r, s in zip(task_pos, task_rms, task_status)]
    n = len(res)
    return {"task": np.array([r["task"] for r in res], dtype=np.int32), "pos": np.array([r["pos"] for r in res]).reshape(n, 3),
            "rms": np.array([r["rms"] for r in res], dtype=np.float64), "pos2": np.array([r["pos2"] for r in res]).reshape(n, 3),
            "rms2": np.array([r["rms2"] for r in res], dtype=np.float64),
            "n_minima": np.array([r["n_minima"] for r in res], dtype=np.int32),
            "flags": np.array([r["flags"] for r in res], dtype=np.int32)}


def posg3_ref(group_ptr, rx0, rx1, tdoa, snr, table, mode, margin_m, group_h=None, x0=(0.1, 0.1, 0.0), z_range=None, z_grid=None,
              grid=32, grid_z=8, starts=4, merge_m=1.0, ratio=2.0, floor_m=0.0, max_iter=100, maps=True):
    """All groups -> dict of the outputs of `thrifty_amd._native.posg3` (`map` / `map_min` for every group when `maps`)."""
    ptr = np.asarray(group_ptr).tolist()
    table = np.asarray(table, dtype=np.float64)
    free_z = mode == FREE_Z
    n, T = len(ptr) - 1, starts + 1
    cx, cy, cz = centres(table, margin_m, grid, z_grid if free_z else None, grid_z)
    out = {"task_pos": np.full((n, T, 3), np.nan), "task_status": np.full((n, T), NO_TASK, dtype=np.int32),
           "task_iters": np.zeros((n, T), dtype=np.int32), "start_cell": np.full((n, starts), -1, dtype=np.int32),
           "start_f": np.full((n, starts), np.nan), "n_local": np.zeros(n, dtype=np.int32), "snr": np.zeros(n),
           "map": np.full((n, grid_z, grid, grid), np.nan), "map_min": np.zeros((n, grid_z, grid, grid), dtype=np.uint8)}
    for key in ("task_dop", "task_hdop", "task_vdop", "task_rms"):
        out[key] = np.full((n, T), np.nan)
    for g, (s, e) in enumerate(zip(ptr[:-1], ptr[1:])):
        cols = (rx0[s:e], rx1[s:e], tdoa[s:e], snr[s:e], table)
        h = 0.0 if free_z else float(group_h[g])

        def run(t, start):
            p, dop, hdop, vdop, rms, snr_mean, status, iters = pos3_ref.pos3_ref(*cols, mode, h, start, z_range, max_iter)
            out["task_pos"][g, t], out["task_dop"][g, t], out["task_hdop"][g, t], out["task_vdop"][g, t] = p, dop, hdop, vdop
            out["task_rms"][g, t], out["task_status"][g, t], out["task_iters"][g, t] = rms, status, iters
            return snr_mean

        out["snr"][g] = run(0, x0)
        if out["task_status"][g, 0] in (UNDERDETERMINED, NONFINITE):
            continue
        F = volume(*cols[:3], table, cx, cy, cz if free_z else [h])
        minima = local_minima(F)
        out["n_local"][g] = int(minima.sum())
        out["start_cell"][g], out["start_f"][g] = lowest(F, minima, starts)
        if maps:
            out["map"][g], out["map_min"][g] = F, minima
        for k, cell in enumerate(out["start_cell"][g].tolist()):
            if cell >= 0:
                run(k + 1, (cx[cell % grid], cy[(cell // grid) % grid], cz[cell // (grid * grid)] if free_z else 0.0))
    out.update(pick_groups(out["task_pos"], out["task_rms"], out["task_status"], merge_m, ratio, floor_m, free_z))
    rows = np.arange(n)
    for key in ("dop", "hdop", "vdop", "status"):
        out[key] = out["task_" + key][rows, out["task"]]
    out["cx"], out["cy"], out["cz"] = cx, cy, cz
    if not maps:
        del out["map"], out["map_min"]
    return out
