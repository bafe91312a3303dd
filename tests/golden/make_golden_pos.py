#!/usr/bin/env python3
"""Golden fixtures for the `pos` step, made by RUNNING THE REFERENCE's thrifty/pos_est.py (`solve`) on
synthetic TDOA groups.  Needs a checkout of the reference, SciPy and mpmath; THRIFTY_REFERENCE names
the checkout:

    THRIFTY_REFERENCE=<checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pos.py

The reference's module is Python 2.  It is imported as it is and two things are put in its way: a `zip`
in its namespace that returns a list (it walks the receiver pairs twice), and `rx_pos` is a dict whose
`keys()` and `values()` return lists (it indexes them).

Each file under tests/golden/pos/ holds the receivers (rx_ids, rx_xyz, in the order of the dict), the
groups as CSR (group_id, group_timestamp, group_tx, group_ptr; rows rx0, rx1, tdoa, snr), and per group
the reference's answer (solved, x_ref, dop_ref, snr_ref) next to the EXACT one: x_star, the minimiser
of the sum of squares found by Newton's method on the gradient with the analytic Hessian in 50-digit
arithmetic from x_ref, and dop_star, the DOP there.  ref_err_max = max |x_ref - x_star| and
dop_ref_err_max = max |dop_ref - dop_star| / dop_star say how far the reference is from it.  `omitted`
/ `omitted_reason` list the generated groups of pos_outside that were left out (see `solve_all`: the
reference, or the device algorithm's NumPy restatement, did not reach the minimum).  The 1-D set is two files, pos_line and pos_line_rising: the order of the two
receivers' coordinates belongs to `rx_pos`, so each order is a fixture of its own.
"""
import itertools
import os
import sys

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ["THRIFTY_REFERENCE"])
sys.path.insert(0, os.path.dirname(HERE))

from thrifty import pos_est, tdoa_est  # noqa: E402

import pos_ref  # noqa: E402  (tests/pos_ref.py: the device algorithm in NumPy)

pos_est.zip = lambda *args: list(zip(*args))
mpmath.mp.dps = 50
C = pos_est.SPEED_OF_LIGHT
OUT = os.path.join(HERE, "pos")
FLOOR = 1e-9          # a set's ref_err_max must reach this (three decades over a float64 solver's floor)


class ListDict(dict):
    def keys(self):
        return list(dict.keys(self))

    def values(self):
        return list(dict.values(self))


def exact_minimum(start, a, b, tdoa):
    """Newton on the gradient from `start` -> (x_star, dop_star, cond(G'G)) or None when it does not
    converge to a point with a positive definite Hessian."""
    mp = mpmath.mp
    a = [mp.matrix(row.tolist()) for row in a]
    b = [mp.matrix(row.tolist()) for row in b]
    tc = [mp.mpf(float(t)) * mp.mpf(C) for t in tdoa]
    p = mp.matrix([float(v) for v in start])
    eye = mp.eye(2)

    def parts(p):
        grad, hess, gtg = mp.zeros(2, 1), mp.zeros(2, 2), mp.zeros(2, 2)
        for ai, bi, ti in zip(a, b, tc):
            va, vb = ai - p, bi - p
            da, db = mp.norm(va), mp.norm(vb)
            ua, ub = va / da, vb / db
            res, row = ti - (da - db), ua - ub
            grad += row * res
            gtg += row * row.T
            hess += row * row.T + res * ((eye - ub * ub.T) / db - (eye - ua * ua.T) / da)
        return grad, hess, gtg

    for _ in range(60):
        grad, hess, gtg = parts(p)
        step = mp.lu_solve(hess, grad)
        p = p - step
        if mp.norm(step) < mp.mpf(10) ** -30:
            break
    else:
        return None
    grad, hess, gtg = parts(p)
    eig_h, eig_g = mp.eigsy(hess, eigvals_only=True), mp.eigsy(gtg, eigvals_only=True)
    if min(eig_h) <= 0 or min(eig_g) <= 0:
        return None
    inv = gtg ** -1
    return (np.array([float(p[0]), float(p[1])]), float(mp.sqrt(inv[0, 0] + inv[1, 1])), float(max(eig_g) / min(eig_g)),
            p)


def ring(rng, n_rx, radius):
    ang = np.linspace(0, 2 * np.pi, n_rx, endpoint=False) + 0.3
    return np.c_[np.cos(ang), np.sin(ang)] * radius + rng.normal(0, radius * 0.05, (n_rx, 2))


def make_rows(rng, table, ids, mobile, noise, keep=0.8, pairs=None):
    if pairs is None:
        every = list(itertools.combinations(range(len(ids)), 2))
        while True:
            pairs = [pr for pr in every if rng.random() < keep]
            if len({i for pr in pairs for i in pr}) >= 3:
                break
    rows = np.zeros(len(pairs), dtype=tdoa_est.TDOA_DTYPE)
    for k, (i, j) in enumerate(pairs):
        true = (np.linalg.norm(table[i] - mobile) - np.linalg.norm(table[j] - mobile)) / C
        rows[k] = (ids[i], ids[j], true + rng.normal(0, noise), rng.uniform(5.0, 500.0), 1.0, 2 * k, 2 * k + 1)
    return rows


def run_reference(groups, ids, table):
    """The reference's `solve`, group by group so that a dropped group is known by its place."""
    rx_pos = ListDict((int(i), np.array(xyz)) for i, xyz in zip(ids, table))
    out = []
    for group in groups:
        res = pos_est.solve([group], rx_pos)
        out.append(res[0] if len(res) else None)
    return out


def save(name, ids, table, groups, ref, star, omitted=(), reasons=()):
    solved = np.array([r is not None for r in ref])
    dims = table.shape[1]
    nan = np.full(dims, np.nan)
    axes = ("x", "y")[:dims]
    x_ref = np.array([[r[k] for k in axes] if r is not None else nan for r in ref], dtype=np.float64).reshape(len(ref), dims)
    x_star = np.array([s[0] if s is not None else nan for s in star], dtype=np.float64).reshape(len(ref), dims)
    dop_ref = np.array([r["dop"] if r is not None else np.nan for r in ref], dtype=np.float64)
    dop_star = np.array([s[1] if s is not None else np.nan for s in star], dtype=np.float64)
    ref_err = float(np.max(np.abs(x_ref - x_star)[solved])) if solved.any() else 0.0
    dop_err = float(np.max((np.abs(dop_ref - dop_star) / np.abs(dop_star))[solved])) if solved.any() else 0.0
    rows = np.concatenate([g[3] for g in groups])
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(
        path, rx_ids=np.array(ids, dtype=np.int64), rx_xyz=table,
        group_id=np.array([g[0] for g in groups], dtype=np.int64),
        group_timestamp=np.array([g[1] for g in groups], dtype=np.float64),
        group_tx=np.array([g[2] for g in groups], dtype=np.int64),
        group_ptr=np.cumsum([0] + [len(g[3]) for g in groups]).astype(np.int64),
        rx0=rows["rx0"].astype(np.int64), rx1=rows["rx1"].astype(np.int64), tdoa=rows["tdoa"], snr=rows["snr"],
        solved=solved, x_ref=x_ref, dop_ref=dop_ref,
        snr_ref=np.array([r["snr"] if r is not None else np.nan for r in ref], dtype=np.float64),
        x_star=x_star, dop_star=dop_star, ref_err_max=ref_err, dop_ref_err_max=dop_err,
        omitted=np.array(omitted, dtype=np.int64), omitted_reason=np.array(list(reasons), dtype="U64"))
    size = os.path.getsize(path)
    print("%-12s %2d groups (%d solved) %4d rows  ref_err_max %.3g m  dop_ref_err_max %.3g  %d bytes  omitted %s"
          % (name, len(groups), int(solved.sum()), len(rows), ref_err, dop_err, size, list(omitted)))
    assert len(groups) <= 64 and size <= 64 * 1024
    return ref_err


def dense(ids, column):
    return np.searchsorted(np.array(ids), column) if list(ids) == sorted(ids) else np.array([list(ids).index(v) for v in column])


def solve_all(groups, ids, table, may_omit=False):
    """(kept groups, reference answers, exact answers, omitted indices, reasons)."""
    ref = run_reference(groups, ids, table)
    kept, refs, stars, omitted, reasons = [], [], [], [], []
    for n, (group, r) in enumerate(zip(groups, ref)):
        if r is None:
            kept.append(group), refs.append(None), stars.append(None)
            continue
        rows = group[3]
        i0, i1 = dense(ids, rows["rx0"]), dense(ids, rows["rx1"])
        star = exact_minimum([r["x"], r["y"]], table[i0], table[i1], rows["tdoa"])
        why = None
        if star is None:
            why = "no convergent Newton from the reference's answer"
        elif max(abs(r["x"] - star[0][0]), abs(r["y"] - star[0][1])) > 1e-3:
            why = "the reference ends more than 1 mm from a minimum"
        else:
            ours = pos_ref.pos_ref(i0, i1, rows["tdoa"], rows["snr"], table)
            if np.max(np.abs(ours[0] - star[0])) > 1e-3:
                why = "the device algorithm goes to another minimum"
        if why is not None:
            assert may_omit, (n, why)
            omitted.append(n), reasons.append(why)
            continue
        assert star[2] < 1e6, (n, star[2])
        kept.append(group), refs.append(r), stars.append(star)
    return kept, refs, stars, omitted, reasons


def header(n, rng):
    return 100 + 3 * n, round(1.7e9 + 0.75 * n + float(rng.integers(0, 1000)) * 1e-6, 6), int(rng.integers(2, 6))


def ring_set(name, seed, n_rx, radius, noise, n_groups=48, cut=(5, 6, 20, 33), reach=0.6, keep=0.8, may_omit=False):
    for attempt in range(20):
        rng = np.random.default_rng(seed + 1000 * attempt)
        ids = [0] + sorted(rng.choice(np.arange(1, 40), n_rx - 1, replace=False).tolist())   # the reference reads rx_pos[0]
        table = ring(rng, n_rx, radius)
        groups = []
        for n in range(n_groups):
            mobile = rng.uniform(-1, 1, 2) * radius * reach
            pairs = None
            if n in cut:      # fewer than three receivers: one pair, once or twice
                i, j = sorted(rng.choice(n_rx, 2, replace=False).tolist())
                pairs = [(i, j)] * (1 + n % 2)
            groups.append(header(n, rng) + (make_rows(rng, table, ids, mobile, noise, keep, pairs),))
        kept, refs, stars, omitted, reasons = solve_all(groups, ids, table, may_omit)
        assert len(omitted) <= 0.05 * len(groups), omitted
        err = save(name, ids, table, kept, refs, stars, omitted, reasons)
        if err >= FLOOR:
            return
        print("   below the floor: another seed")
    raise AssertionError(name)


def three(seed):
    """Three receivers, two or three rows: nearly exactly determined."""
    for attempt in range(20):
        rng = np.random.default_rng(seed + 1000 * attempt)
        ids, table = [0, 8, 21], ring(rng, 3, 200.0)
        groups = []
        for n in range(40):
            mobile = rng.uniform(-1, 1, 2) * 200.0 * 0.5
            every = [(0, 1), (0, 2), (1, 2)]
            pairs = every if n % 2 else [every[k] for k in sorted(rng.choice(3, 2, replace=False).tolist())]
            groups.append(header(n, rng) + (make_rows(rng, table, ids, mobile, 3e-9, pairs=pairs),))
        kept, refs, stars, omitted, reasons = solve_all(groups, ids, table)
        if save("pos_three", ids, table, kept, refs, stars) >= FLOOR:
            return
    raise AssertionError("pos_three")


def line(seed):
    """Two receivers on a line, once per coordinate order (pos_line: the first receiver of `rx_pos` has
    the larger coordinate, pos_line_rising: the smaller; the order decides the formula's sign).  Each
    file has rows that name the receivers in either order, tdoas of both signs, and mobiles between the
    two and outside them (outside: dop == -1)."""
    rng = np.random.default_rng(seed)
    for name, xs in (("pos_line", [35.0, -12.5]), ("pos_line_rising", [-12.5, 35.0])):
        ids, table = [7, 4], np.array(xs).reshape(2, 1)
        groups = []
        for n in range(24):
            mobile = rng.uniform(-40.0, 70.0)        # outside the two about half of the time
            a, b = (0, 1) if n % 3 else (1, 0)
            true = (abs(table[a, 0] - mobile) - abs(table[b, 0] - mobile)) / C
            rows = np.zeros(1, dtype=tdoa_est.TDOA_DTYPE)
            rows[0] = (ids[a], ids[b], true * (1 if n % 5 else 1.5) + rng.normal(0, 3e-9), rng.uniform(5.0, 500.0), 1.0, 0, 1)
            groups.append(header(n, rng) + (rows,))
        ref = run_reference(groups, ids, table)
        assert all(r is not None for r in ref)
        dops = np.array([r["dop"] for r in ref])
        assert np.any(dops == -1) and np.any(dops == 0.5)
        tdoas = np.array([g[3]["tdoa"][0] for g in groups])
        assert np.any(tdoas > 0) and np.any(tdoas < 0)
        star = [(np.array([r["x"]]), float(r["dop"]), 1.0) for r in ref]      # the formula IS the exact answer
        save(name, ids, table, groups, ref, star)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    ring_set("pos_ring4", 11, 4, 100.0, 1e-9)
    ring_set("pos_ring6", 12, 6, 300.0, 3e-9)
    ring_set("pos_ring8", 13, 8, 1000.0, 10e-9)
    three(14)
    # five receivers, the mobile up to 2.5 radii away: groups the reference (or the device algorithm)
    # does not bring to the minimum are left out, 5 % of the generated ones at most, and listed
    ring_set("pos_outside", 15, 5, 100.0, 3e-9, n_groups=60, cut=(), reach=2.5, may_omit=True)
    line(16)
