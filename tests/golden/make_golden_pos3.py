#!/usr/bin/env python3
"""Golden fixtures for `thrifty_amd.pos_3d` (receivers with three coordinates), made on the CPU.  Needs a checkout of
the reference, SciPy and mpmath; THRIFTY_REFERENCE names the checkout:

    THRIFTY_REFERENCE=<checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pos3.py

The reference's `solve_numerically` cannot be called with three coordinates: its start `x0 = [0.1, 0.1]` has two
entries and SciPy raises on the shapes.  Its residual and Jacobian are written for any number of coordinates, so this
generator STATES those two expressions itself (`residuals`, `jacobian` below: tdoa c - (|rx0 - p| - |rx1 - p|) and
the difference of the unit vectors), for three coordinates and for two with the height substituted, and hands them to
the same SciPy call: `least_squares` (TRF) from (0.1, 0.1, z0) -- or (0.1, 0.1) -- inside the reference's bounds
(the receivers' extent -+ MAX_DIST per axis; `z_range` on z where a set has one).  The reference's own `dop()` does
run in three dimensions and gives `dop_ref` of the free-z sets (imported as in make_golden_pos.py); with the height
known `dop_ref` is the same expression on the two horizontal columns.

Each file under tests/golden/pos3/ holds the receivers (rx_ids, rx_xyz), the groups as CSR (group_id,
group_timestamp, group_tx, group_ptr; rows rx0, rx1, tdoa, snr), the mode (`free_z`, `group_h`, `z0`, `z_range`) and
per group: solved, x_ref (SciPy's answer; z = the height where it is known), x_star (the EXACT minimiser: Newton on
the gradient with the analytic Hessian in 50-digit arithmetic from x_ref -- on the free coordinates only, so for a
group of z_box whose minimum lies outside `z_range` it is the constrained minimiser on the bound, `on_bound`, whose
z gradient is checked to point outwards), dop_star / hdop_star / vdop_star there in 50 digits, dop_ref, snr_ref, the
condition number of G'G, and ref_err_max = max |x_ref - x_star|, dop_ref_err_max = max |dop_ref - dop_star| /
dop_star.  No group is omitted from any set; every set's ref_err_max reaches FLOOR (another seed otherwise).  The
device's iteration takes longer first steps than SciPy's trust region, and on the nearly coplanar ring of z_ring6
(cond(G'G) of several hundred) it can end in ANOTHER local minimum than SciPy from the same start: seed 35 sends 4
of 44 groups 140 to 220 m up, to minima with twice the r.m.s. residual.  Which basin a start belongs to is not what
these fixtures pin (README, "Receivers at different heights?" says what to do about it), so such a draw is printed and
drawn again as a whole, never thinned.  Within the basin the NumPy restatement of the device algorithm
(tests/pos3_ref.py) is asserted to be within ref_err_max of x_star and dop_ref_err_max of the three dops: whether the
yardstick can be met is decided here, before any GPU run.
"""
import itertools
import os
import sys

import mpmath
import numpy as np
import scipy.optimize

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ["THRIFTY_REFERENCE"])
sys.path.insert(0, os.path.dirname(HERE))

from thrifty import pos_est, tdoa_est  # noqa: E402

import pos3_ref  # noqa: E402  (tests/pos3_ref.py: the device algorithm in NumPy)

pos_est.zip = lambda *args: list(zip(*args))
mpmath.mp.dps = 50
C = pos_est.SPEED_OF_LIGHT
MAX_DIST = pos_est.MAX_DIST
OUT = os.path.join(HERE, "pos3")
FLOOR = 1e-9          # a set's ref_err_max must reach this (make_golden_pos.py's)


def residuals(p, a, b, tc):
    return tc - (np.linalg.norm(a - p, axis=1) - np.linalg.norm(b - p, axis=1))


def jacobian(p, a, b):
    va, vb = a - p, b - p
    return va / np.linalg.norm(va, axis=1)[:, None] - vb / np.linalg.norm(vb, axis=1)[:, None]


def scipy_answer(a, b, tdoa, table, free_z, height, z0, z_range):
    """x_ref[3]: the reference's call on the expressions above."""
    tc = tdoa * C
    lo, hi = table.min(axis=0) - MAX_DIST, table.max(axis=0) + MAX_DIST
    if free_z:
        if z_range is not None:
            lo[2], hi[2] = z_range
        res = scipy.optimize.least_squares(lambda p: residuals(p, a, b, tc), [0.1, 0.1, z0], jac=lambda p: jacobian(p, a, b),
                                           bounds=(lo, hi))
        return res.x
    full = lambda q: np.array([q[0], q[1], height])      # noqa: E731
    res = scipy.optimize.least_squares(lambda q: residuals(full(q), a, b, tc), [0.1, 0.1],
                                       jac=lambda q: jacobian(full(q), a, b)[:, :2], bounds=(lo[:2], hi[:2]))
    return full(res.x)


def exact_minimum(start, free, a, b, tdoa):
    """Newton on the gradient over the coordinates `free` from `start` (three entries; the others stay) ->
    (x_star[3], the full 3-D gradient, the Hessian over `free`, the full G'G) in 50 digits, or None."""
    mp = mpmath.mp
    a = [mp.matrix(row.tolist()) for row in a]
    b = [mp.matrix(row.tolist()) for row in b]
    tc = [mp.mpf(float(t)) * mp.mpf(C) for t in tdoa]
    p = mp.matrix([float(v) for v in start])
    eye = mp.eye(3)

    def parts(p):
        grad, hess, gtg = mp.zeros(3, 1), mp.zeros(3, 3), mp.zeros(3, 3)
        for ai, bi, ti in zip(a, b, tc):
            va, vb = ai - p, bi - p
            da, db = mp.norm(va), mp.norm(vb)
            ua, ub = va / da, vb / db
            res, row = ti - (da - db), ua - ub
            grad += row * res
            gtg += row * row.T
            hess += row * row.T + res * ((eye - ub * ub.T) / db - (eye - ua * ua.T) / da)
        return grad, hess, gtg

    def cut(matrix, cols=None):
        rows = list(free)
        return mp.matrix([[matrix[r, c] for c in (rows if cols is None else cols)] for r in rows])

    for _ in range(60):
        grad, hess, gtg = parts(p)
        step = mp.lu_solve(cut(hess), cut(grad, [0]))
        for k, axis in enumerate(free):
            p[axis] -= step[k]
        if mp.norm(step) < mp.mpf(10) ** -30:
            break
    else:
        return None
    grad, hess, gtg = parts(p)
    return p, grad, cut(hess), gtg


def dops_exact(gtg, axes):
    """(dop, hdop, vdop, cond) of G'G cut to `axes` in 50 digits; vdop = 0 where z is not among them."""
    mp = mpmath.mp
    sub = mp.matrix([[gtg[r, c] for c in axes] for r in axes])
    eig = mp.eigsy(sub, eigvals_only=True)
    assert min(eig) > 0
    inv = sub ** -1
    hdop = mp.sqrt(inv[0, 0] + inv[1, 1])
    vdop = mp.sqrt(inv[2, 2]) if len(axes) == 3 else mp.mpf(0)
    dop = mp.sqrt(sum(inv[k, k] for k in range(len(axes))))
    return float(dop), float(hdop), float(vdop), float(max(eig) / min(eig))


def ring(rng, n_rx, radius, z_lo, z_hi):
    ang = np.linspace(0, 2 * np.pi, n_rx, endpoint=False) + 0.3
    xy = np.c_[np.cos(ang), np.sin(ang)] * radius + rng.normal(0, radius * 0.05, (n_rx, 2))
    z = rng.permutation(np.linspace(z_lo, z_hi, n_rx))       # the stated spread, in no order around the ring
    return np.c_[xy, z]


def make_rows(rng, table, ids, mobile, noise, needed, keep=0.8, pairs=None):
    if pairs is None:
        every = list(itertools.combinations(range(len(ids)), 2))
        while True:
            pairs = [pr for pr in every if rng.random() < keep]
            if len({i for pr in pairs for i in pr}) >= needed and len(pairs) >= needed:
                break
    rows = np.zeros(len(pairs), dtype=tdoa_est.TDOA_DTYPE)
    for k, (i, j) in enumerate(pairs):
        true = (np.linalg.norm(table[i] - mobile) - np.linalg.norm(table[j] - mobile)) / C
        rows[k] = (ids[i], ids[j], true + rng.normal(0, noise), rng.uniform(5.0, 500.0), 1.0, 2 * k, 2 * k + 1)
    return rows


def header(n, rng):
    return 100 + 3 * n, round(1.7e9 + 0.75 * n + float(rng.integers(0, 1000)) * 1e-6, 6), int(rng.integers(2, 6))


class ListDict(dict):
    def keys(self):
        return list(dict.keys(self))

    def values(self):
        return list(dict.values(self))


def solve_set(groups, ids, table, free_z, group_h, z0, z_range):
    """Per group (x_ref, x_star, dops_star, dop_ref, cond, on_bound) or None where the group is underdetermined."""
    needed = 4 if free_z else 3
    index = {r: k for k, r in enumerate(ids)}
    rx_pos = ListDict((int(i), np.array(xyz)) for i, xyz in zip(ids, table))
    out = []
    for n, group in enumerate(groups):
        rows = group[3]
        if len(set(rows["rx0"].tolist()) | set(rows["rx1"].tolist())) < needed:
            out.append(None)
            continue
        i0, i1 = [index[r] for r in rows["rx0"]], [index[r] for r in rows["rx1"]]
        a, b = table[i0], table[i1]
        h = 0.0 if free_z else float(group_h[n])
        x_ref = scipy_answer(a, b, rows["tdoa"], table, free_z, h, z0, z_range)
        free, on_bound = ((0, 1, 2) if free_z else (0, 1)), False
        start = x_ref.copy()
        star = exact_minimum(start, free, a, b, rows["tdoa"])
        if free_z and z_range is not None and not (star is not None and z_range[0] < float(star[0][2]) < z_range[1]):
            on_bound, free = True, (0, 1)         # the free minimum lies outside: the constrained one, z on the bound
            start[2] = z_range[0] if abs(x_ref[2] - z_range[0]) < abs(x_ref[2] - z_range[1]) else z_range[1]
            star = exact_minimum(start, free, a, b, rows["tdoa"])
        assert star is not None, (n, "no convergent Newton from SciPy's answer")
        p, grad, hess, gtg = star
        assert min(mpmath.mp.eigsy(hess, eigvals_only=True)) > 0, (n, "not a minimum")
        x_star = np.array([float(p[k]) for k in range(3)])
        if on_bound:      # descent (-grad) must point out of the box on z
            assert (grad[2] > 0) == (start[2] == z_range[0]) and grad[2] != 0, (n, "the bound is not active")
        elif free_z and z_range is not None:
            assert z_range[0] < x_star[2] < z_range[1], (n, "a free minimum outside the range")
        assert np.max(np.abs(x_ref - x_star)) < 1e-2, (n, "SciPy ends more than 1 cm from the minimum", x_ref, x_star)
        dops = dops_exact(gtg, (0, 1, 2) if free_z else (0, 1))
        if free_z:
            dop_ref = float(pos_est.dop(x_ref, rx_pos, list(zip(rows["rx0"].tolist(), rows["rx1"].tolist()))))
        else:
            G = jacobian(x_ref, a, b)[:, :2]
            dop_ref = float(np.sqrt(np.trace(np.linalg.inv(G.T.dot(G)))))
        out.append((x_ref, x_star, dops[:3], dop_ref, dops[3], on_bound))
    return out


def save(name, ids, table, groups, free_z, group_h, z0, z_range, tx_height=None):
    sol = solve_set(groups, ids, table, free_z, group_h, z0, z_range)
    solved = np.array([s is not None for s in sol])
    nan3 = np.full(3, np.nan)
    pick = lambda f, empty: np.array([f(s) if s is not None else empty for s in sol], dtype=np.float64)      # noqa: E731
    x_ref, x_star = pick(lambda s: s[0], nan3), pick(lambda s: s[1], nan3)
    dop_star, hdop_star, vdop_star = (pick(lambda s, k=k: s[2][k], np.nan) for k in range(3))
    dop_ref, cond = pick(lambda s: s[3], np.nan), pick(lambda s: s[4], np.nan)
    on_bound = np.array([bool(s is not None and s[5]) for s in sol])
    ref_err = float(np.max(np.abs(x_ref - x_star)[solved]))
    dop_err = float(np.max((np.abs(dop_ref - dop_star) / dop_star)[solved]))
    rows = np.concatenate([g[3] for g in groups])
    ptr = np.cumsum([0] + [len(g[3]) for g in groups]).astype(np.int64)
    snr_ref = np.array([np.mean(g[3]["snr"]) if ok else np.nan for g, ok in zip(groups, solved)], dtype=np.float64)

    # the device algorithm's restatement must meet the yardstick on the CPU
    index = {r: k for k, r in enumerate(ids)}
    d0 = np.array([index[r] for r in rows["rx0"]]), np.array([index[r] for r in rows["rx1"]])
    ours = pos3_ref.pos3_ref_groups(ptr, d0[0], d0[1], rows["tdoa"], rows["snr"], table,
                                    pos3_ref.FREE_Z if free_z else pos3_ref.KNOWN_HEIGHT, group_h,
                                    (0.1, 0.1, z0 if free_z else 0.0), z_range)
    per_group = np.max(np.abs(ours["pos"] - x_star), axis=1)
    elsewhere = np.flatnonzero(solved & ~(per_group <= 1e-3))
    if len(elsewhere):      # another local minimum than SciPy's: the start decides the basin, not the arithmetic
        print("   %s: the device algorithm ends in another local minimum than SciPy in groups %s (%.3g m away at most): "
              "another seed" % (name, elsewhere.tolist(), np.nanmax(per_group[elsewhere])))
        return None
    assert np.array_equal(ours["status"] == pos3_ref.UNDERDETERMINED, ~solved)
    assert np.array_equal(ours["status"][solved] == pos3_ref.AT_BOUND, on_bound[solved]), ours["status"]
    assert set(ours["status"][solved & ~on_bound].tolist()) == {pos3_ref.OK}, ours["status"]
    our_err = float(np.max(per_group[solved]))
    our_dop = max(float(np.max((np.abs(ours[key] - star) / star)[solved])) for key, star in
                  (("dop", dop_star), ("hdop", hdop_star)) + ((("vdop", vdop_star),) if free_z else ()))
    assert our_err <= ref_err and our_dop <= dop_err, (name, our_err, ref_err, our_dop, dop_err)

    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(
        path, rx_ids=np.array(ids, dtype=np.int64), rx_xyz=table,
        group_id=np.array([g[0] for g in groups], dtype=np.int64),
        group_timestamp=np.array([g[1] for g in groups], dtype=np.float64),
        group_tx=np.array([g[2] for g in groups], dtype=np.int64), group_ptr=ptr,
        rx0=rows["rx0"].astype(np.int64), rx1=rows["rx1"].astype(np.int64), tdoa=rows["tdoa"], snr=rows["snr"],
        free_z=np.bool_(free_z), group_h=np.zeros(0) if group_h is None else np.asarray(group_h, dtype=np.float64),
        tx_height=np.zeros((0, 2)) if tx_height is None else np.array(sorted(tx_height.items()), dtype=np.float64),
        z0=np.float64(z0 if free_z else np.nan), z_range=np.zeros(0) if z_range is None else np.asarray(z_range, dtype=np.float64),
        solved=solved, on_bound=on_bound, x_ref=x_ref, dop_ref=dop_ref, snr_ref=snr_ref, x_star=x_star, dop_star=dop_star,
        hdop_star=hdop_star, vdop_star=vdop_star, cond=cond, ref_err_max=ref_err, dop_ref_err_max=dop_err)
    size = os.path.getsize(path)
    print("%-8s %2d groups (%d solved, %d on the bound) %4d rows  cond <= %.3g  ref_err_max %.3g m (restatement %.3g)  "
          "dop_ref_err_max %.3g (restatement %.3g)  iters <= %d  %d bytes"
          % (name, len(groups), int(solved.sum()), int(on_bound.sum()), len(rows), np.nanmax(cond), ref_err, our_err, dop_err,
             our_dop, ours["iters"].max(), size))
    assert len(groups) <= 64 and size <= 64 * 1024
    return ref_err


def ring_set(name, seed, n_rx, radius, z_span, noise, free_z, n_groups=48, cut=(5, 6, 20, 33), heights="group", z_range=None,
             all_pairs=False, table_of=None):
    needed = 4 if free_z else 3
    for attempt in range(20):
        rng = np.random.default_rng(seed + 1000 * attempt)
        ids = [0] + sorted(rng.choice(np.arange(1, 40), n_rx - 1, replace=False).tolist())
        table = ring(rng, n_rx, radius, *z_span)
        if table_of is not None:
            ids, table = table_of
        z0 = 0.5 * (z_range[0] + z_range[1]) if z_range is not None else float(table[:, 2].min()) - 1.0
        groups, group_h, tx_height = [], [], {tx: 0.5 + 0.6 * tx for tx in range(2, 6)}
        for n in range(n_groups):
            head = header(n, rng)
            tag_z = tx_height[head[2]] if heights == "tx" else rng.uniform(0.0, 3.0)
            mobile = np.append(rng.uniform(-1, 1, 2) * radius * 0.6, tag_z)
            pairs = list(itertools.combinations(range(n_rx), 2)) if all_pairs else None
            if n in cut:      # one receiver too few: the pairs of needed - 1 receivers (once, or the first of them twice)
                few = sorted(rng.choice(n_rx, needed - 1, replace=False).tolist())
                pairs = list(itertools.combinations(few, 2))
                pairs = pairs + pairs[:1] if n % 2 else pairs
            groups.append(head + (make_rows(rng, table, ids, mobile, noise, needed, pairs=pairs),))
            group_h.append(tag_z)
        err = save(name, ids, table, groups, free_z, None if free_z else np.array(group_h), z0, z_range,
                   tx_height if heights == "tx" and not free_z else None)
        if err is not None and err >= FLOOR:
            return ids, table
        if err is not None:
            print("   below the floor: another seed")
    raise AssertionError(name)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    ring_set("h_ring4", 31, 4, 100.0, (2.0, 32.0), 1e-9, False)
    ring_set("h_ring6", 32, 6, 300.0, (2.0, 42.0), 3e-9, False, heights="tx")
    tall6 = ring_set("z_tall6", 33, 6, 100.0, (2.0, 82.0), 1e-9, True)
    ring_set("z_tall5", 34, 5, 100.0, (2.0, 102.0), 1e-9, True)
    ring_set("z_ring6", 35, 6, 300.0, (2.0, 42.0), 3e-9, True)
    ring_set("z_four", 36, 4, 100.0, (2.0, 102.0), 1e-9, True, all_pairs=True)
    # z_tall6's receivers; the tags sit at 0 .. 3 m and the range starts at 1.5 m: about half of the free minima lie below it
    ring_set("z_box", 37, 6, 100.0, (2.0, 82.0), 1e-9, True, cut=(), z_range=(1.5, 60.0), table_of=tall6)
