"""The NumPy statement of thr_track (include/thrifty_hip.h): the plain sequential recursion, in float64 and in
np.longdouble, and the same filter and smoother as scans whose elements are combined in a balanced tree over the whole
track ("scan") or as track.hip combines them ("tiles": fragments cut where the sorted position crosses a multiple of
the tile length, a doubling-step scan inside each, a sequential walk of five-double carries between them).

    run(scene-like columns, q, v0, gate, max_rounds, kind=np.float64, form="sequential" | "scan" | "tiles") -> dict

Every array is in input row order except track_tx / track_ptr / track_stats / track_flags (per track) and order."""
import numpy as np

GATE_999 = 13.815510557964274
LOST = 1


def sort_rows(tx, timestamp):
    """Stable sort on (tx, timestamp) -> order (sorted position -> input row), track_tx, track_ptr."""
    tx, timestamp = np.asarray(tx, dtype=np.int64), np.asarray(timestamp, dtype=np.float64)
    order = np.lexsort((timestamp, tx)).astype(np.int64)          # lexsort is stable; the last key is the primary one
    track_tx, first = np.unique(tx[order], return_index=True)
    return order, track_tx.astype(np.int32), np.append(first, len(tx)).astype(np.int64)


def _q(dt, q, kind):
    return q * (dt * dt * dt / kind(3)), q * (dt * dt / kind(2)), q * dt


# ------------------------------------------------------------------ the sequential recursion, one track, one axis
def filter_axis(t, z, r, mask, q, v0, kind):
    """t, z, r, mask from the track's start row on -> m[n, 2], P[n, 3] (pp, pv, vv), nu[n], S[n] of the predictions."""
    n = len(t)
    m, P, nu, S = np.zeros((n, 2), kind), np.zeros((n, 3), kind), np.zeros(n, kind), np.ones(n, kind)
    m0, m1, p00, p01, p11 = z[0], kind(0), r[0], kind(0), v0 * v0
    m[0], P[0] = (m0, m1), (p00, p01, p11)
    for k in range(1, n):
        dt = t[k] - t[k - 1]
        q00, q01, q11 = _q(dt, q, kind)
        # F m, F P F' + Q
        m0 = m0 + dt * m1
        f00, f01 = p00 + dt * p01, p01 + dt * p11
        p00, p01, p11 = (f00 + dt * f01) + q00, f01 + q01, p11 + q11
        nu[k], S[k] = z[k] - m0, p00 + r[k]
        if mask[k]:
            k0, k1 = p00 / S[k], p01 / S[k]
            m0, m1 = m0 + k0 * nu[k], m1 + k1 * nu[k]
            p00, p01, p11 = p00 - k0 * p00, p01 - k0 * p01, p11 - k1 * p01
        m[k], P[k] = (m0, m1), (p00, p01, p11)
    return m, P, nu, S


def smooth_axis(t, m, P, q, kind):
    """Rauch-Tung-Striebel over filter_axis' output: G_k = P_k F' inv(F P_k F' + Q)."""
    n = len(t)
    ms, Ps = m.copy(), P.copy()
    for k in range(n - 2, -1, -1):
        dt = t[k + 1] - t[k]
        q00, q01, q11 = _q(dt, q, kind)
        p00, p01, p11 = P[k]
        f00, f01 = p00 + dt * p01, p01 + dt * p11
        a00, a01, a11 = (f00 + dt * f01) + q00, f01 + q01, p11 + q11
        det = a00 * a11 - a01 * a01
        i00, i01, i11 = a11 / det, -a01 / det, a00 / det
        g00, g01 = f00 * i00 + p01 * i01, f00 * i01 + p01 * i11
        g10, g11 = f01 * i00 + p11 * i01, f01 * i01 + p11 * i11
        d0, d1 = ms[k + 1, 0] - (m[k, 0] + dt * m[k, 1]), ms[k + 1, 1] - m[k, 1]
        ms[k] = (m[k, 0] + (g00 * d0 + g01 * d1), m[k, 1] + (g10 * d0 + g11 * d1))
        e00, e01, e11 = Ps[k + 1, 0] - a00, Ps[k + 1, 1] - a01, Ps[k + 1, 2] - a11
        # P + G (Ps - PP) G'
        y00, y01, y10, y11 = g00 * e00 + g01 * e01, g00 * e01 + g01 * e11, g10 * e00 + g11 * e01, g10 * e01 + g11 * e11
        Ps[k] = (p00 + (y00 * g00 + y01 * g01), p01 + (y00 * g10 + y01 * g11), p11 + (y10 * g10 + y11 * g11))
    return ms, Ps


# ------------------------------------------------------------------ the same as scans
def filter_elements(t, z, r, mask, q, v0, kind):
    """e[n, 14] = A00 A01 A10 A11 | b0 b1 | C00 C01 C11 | eta0 eta1 | J00 J01 J11 of the rows from the start row on."""
    n = len(t)
    e = np.zeros((n, 14), kind)
    dt = np.diff(t, prepend=t[:1])
    q00, q01, q11 = _q(dt, q, kind)
    on = np.asarray(mask, dtype=bool)
    s = q00 + r
    k0, k1 = q00 / s, q01 / s
    one = kind(1)
    meas = np.stack([one - k0, (one - k0) * dt, -k1, one - k1 * dt, k0 * z, k1 * z, (one - k0) * q00, (one - k0) * q01,
                     q11 - k1 * q01, z / s, dt * z / s, one / s, dt / s, dt * dt / s], axis=1)
    zero = np.zeros(n, kind)
    pred = np.stack([zero + one, dt, zero, zero + one, zero, zero, q00, q01, q11, zero, zero, zero, zero, zero], axis=1)
    e[:] = np.where(on[:, None], meas, pred)
    e[0] = 0
    e[0, 4], e[0, 6], e[0, 8] = z[0], r[0], v0 * v0
    return e


def filter_combine(i, j):
    """i (x) j on rows of elements: i the earlier rows, j the later ones.  With M = inv(I + C_i J_j):
    A = A_j M A_i, b = A_j M (b_i + C_i eta_j) + b_j, C = A_j M C_i A_j' + C_j, eta = A_i' N (eta_j - J_j b_i) + eta_i,
    J = A_i' N J_j A_i + J_i; N = inv(I + J_j C_i) is M transposed.  b in the form A_j (b_i + M C_i (eta_j - J_j b_i)) + b_j,
    the same number with the error of a badly conditioned M on the innovation, not on the position."""
    o = np.empty_like(i)
    I = [i[:, k] for k in range(14)]
    J = [j[:, k] for k in range(14)]
    t00, t01 = 1 + (I[6] * J[11] + I[7] * J[12]), I[6] * J[12] + I[7] * J[13]
    t10, t11 = I[7] * J[11] + I[8] * J[12], 1 + (I[7] * J[12] + I[8] * J[13])
    det = t00 * t11 - t01 * t10
    m00, m01, m10, m11 = t11 / det, -t01 / det, -t10 / det, t00 / det
    # MC = M C_i
    c00, c01, c10, c11 = m00 * I[6] + m01 * I[7], m00 * I[7] + m01 * I[8], m10 * I[6] + m11 * I[7], m10 * I[7] + m11 * I[8]
    d0, d1 = J[9] - (J[11] * I[4] + J[12] * I[5]), J[10] - (J[12] * I[4] + J[13] * I[5])
    u0, u1 = I[4] + (c00 * d0 + c01 * d1), I[5] + (c10 * d0 + c11 * d1)
    x00, x01, x10, x11 = J[0] * m00 + J[1] * m10, J[0] * m01 + J[1] * m11, J[2] * m00 + J[3] * m10, J[2] * m01 + J[3] * m11
    y00, y01, y10, y11 = J[0] * c00 + J[1] * c10, J[0] * c01 + J[1] * c11, J[2] * c00 + J[3] * c10, J[2] * c01 + J[3] * c11
    w00, w10 = m00 * I[0] + m01 * I[2], m00 * I[1] + m01 * I[3]
    w01, w11 = m10 * I[0] + m11 * I[2], m10 * I[1] + m11 * I[3]
    z00, z01, z10, z11 = w00 * J[11] + w01 * J[12], w00 * J[12] + w01 * J[13], w10 * J[11] + w11 * J[12], w10 * J[12] + w11 * J[13]
    o[:, 0], o[:, 1] = x00 * I[0] + x01 * I[2], x00 * I[1] + x01 * I[3]
    o[:, 2], o[:, 3] = x10 * I[0] + x11 * I[2], x10 * I[1] + x11 * I[3]
    o[:, 4], o[:, 5] = (J[0] * u0 + J[1] * u1) + J[4], (J[2] * u0 + J[3] * u1) + J[5]
    o[:, 6], o[:, 7], o[:, 8] = (y00 * J[0] + y01 * J[1]) + J[6], (y00 * J[2] + y01 * J[3]) + J[7], (y10 * J[2] + y11 * J[3]) + J[8]
    o[:, 9], o[:, 10] = (w00 * d0 + w01 * d1) + I[9], (w10 * d0 + w11 * d1) + I[10]
    o[:, 11], o[:, 12], o[:, 13] = (z00 * I[0] + z01 * I[2]) + I[11], (z00 * I[1] + z01 * I[3]) + I[12], (z10 * I[1] + z11 * I[3]) + I[13]
    return o


def smooth_elements(t, m, P, q, kind):
    """e[n, 9] = E00 E01 E10 E11 | g0 g1 | L00 L01 L11: E = G, g = m - G F m, L = P - G F P; the last row (0, m, P)."""
    n = len(t)
    e = np.zeros((n, 9), kind)
    if n > 1:
        dt = np.diff(t)
        q00, q01, q11 = _q(dt, q, kind)
        m0, m1, p00, p01, p11 = m[:-1, 0], m[:-1, 1], P[:-1, 0], P[:-1, 1], P[:-1, 2]
        f00, f01 = p00 + dt * p01, p01 + dt * p11
        a00, a01, a11 = (f00 + dt * f01) + q00, f01 + q01, p11 + q11
        det = a00 * a11 - a01 * a01
        i00, i01, i11 = a11 / det, -a01 / det, a00 / det
        g00, g01 = f00 * i00 + p01 * i01, f00 * i01 + p01 * i11
        g10, g11 = f01 * i00 + p11 * i01, f01 * i01 + p11 * i11
        fm0 = m0 + dt * m1
        e[:-1] = np.stack([g00, g01, g10, g11, m0 - (g00 * fm0 + g01 * m1), m1 - (g10 * fm0 + g11 * m1),
                           p00 - (g00 * f00 + g01 * p01), p01 - (g00 * f01 + g01 * p11), p11 - (g10 * f01 + g11 * p11)], axis=1)
    e[-1, 4:6], e[-1, 6:9] = m[-1], P[-1]
    return e


def smooth_combine(i, j):
    """i (x) j: i the rows nearer the start, j the ones after them."""
    o = np.empty_like(i)
    I = [i[:, k] for k in range(9)]
    J = [j[:, k] for k in range(9)]
    y00, y01, y10, y11 = I[0] * J[6] + I[1] * J[7], I[0] * J[7] + I[1] * J[8], I[2] * J[6] + I[3] * J[7], I[2] * J[7] + I[3] * J[8]
    o[:, 0], o[:, 1], o[:, 2], o[:, 3] = I[0] * J[0] + I[1] * J[2], I[0] * J[1] + I[1] * J[3], I[2] * J[0] + I[3] * J[2], I[2] * J[1] + I[3] * J[3]
    o[:, 4], o[:, 5] = (I[0] * J[4] + I[1] * J[5]) + I[4], (I[2] * J[4] + I[3] * J[5]) + I[5]
    o[:, 6], o[:, 7], o[:, 8] = (y00 * I[0] + y01 * I[1]) + I[6], (y00 * I[2] + y01 * I[3]) + I[7], (y10 * I[2] + y11 * I[3]) + I[8]
    return o


def tree_scan(e, combine, backward=False):
    """Inclusive scan of the rows of e in a balanced tree (doubling steps: row k takes the combination of up to d
    rows before it, d = 1, 2, 4, ...); backward: of the rows after it."""
    e = e[::-1].copy() if backward else e.copy()
    d = 1
    while d < len(e):
        e[d:] = combine(e[d:], e[:-d]) if backward else combine(e[:-d], e[d:])
        d *= 2
    return e[::-1] if backward else e


def _innovations(t, z, r, pre, q, kind):
    m, P = pre[:, 4:6].copy(), pre[:, 6:9].copy()
    nu, S = np.zeros(len(t), kind), np.ones(len(t), kind)
    if len(t) > 1:     # the gate kernel's step: the prediction from the state of the row before
        dt = np.diff(t)
        q00 = _q(dt, q, kind)[0]
        s = np.concatenate([m[:-1], P[:-1]], axis=1)
        nu[1:] = z[1:] - (s[:, 0] + dt * s[:, 1])
        S[1:] = (((s[:, 2] + dt * s[:, 3]) + dt * (s[:, 3] + dt * s[:, 4])) + q00) + r[1:]
    return m, P, nu, S


def filter_axis_scan(t, z, r, mask, q, v0, kind):
    return _innovations(t, z, r, tree_scan(filter_elements(t, z, r, mask, q, v0, kind), filter_combine), q, kind)


def smooth_axis_scan(t, m, P, q, kind):
    suf = tree_scan(smooth_elements(t, m, P, q, kind), smooth_combine, backward=True)
    return suf[:, 4:6].copy(), suf[:, 6:9].copy()


# ------------------------------------------------------------------ the same as track.hip's tiles and carries
TILE = 256


def fragments(first, n, tile=TILE):
    """The n rows of a track whose first row has sorted position `first` in the whole call -> [(a, e), ...]: the
    ranges of its rows between the multiples of the tile length."""
    cuts = [0] + [p - first for p in range((first // tile + 1) * tile, first + n, tile)] + [n]
    return [(a, e) for a, e in zip(cuts[:-1], cuts[1:]) if e > a]


def _state(o):
    """(0, state, 0): what k_filter_carry and k_smooth_carry keep of a combination, slots 4 .. 8 in both operators."""
    c = np.zeros_like(o)
    c[4:9] = o[4:9]
    return c


def filter_axis_tiles(t, z, r, mask, q, v0, kind, first=0, tile=TILE):
    """k_filter<false>, k_filter_carry, k_filter<true>: every fragment's total without a carry, the walk over the
    fragments in order (carry (x) total), the carry combined into the fragment's first element, and the scan again.
    One departure: the fragments here are cut from the START row (`first` is its sorted position) and the first of them
    reads no carry, while track.hip cuts from the track's first row and, where the start row lies beyond the first
    tile boundary (invalid rows at a track's head, the `invalid_tile` kind of scene), combines a zero carry into the
    fragments of identity rows before it and into the one that holds the start row.  The start row's A = 0 annihilates
    whatever stands before it, so the state is the same; the path is not, and no scene of clauses() takes it."""
    e = filter_elements(t, z, r, mask, q, v0, kind)
    frags = fragments(first, len(t), tile)
    carry, carries = np.zeros(14, kind), []
    for a, b in frags:
        carries.append(carry)
        total = tree_scan(e[a:b], filter_combine)[-1]
        carry = _state(filter_combine(carry[None], total[None])[0])
    pre = np.zeros_like(e)
    for f, (a, b) in enumerate(frags):
        el = e[a:b].copy()
        if f:       # a track's first fragment reads no carry
            el[0] = filter_combine(carries[f][None], el[:1])[0]
        pre[a:b] = tree_scan(el, filter_combine)
    return _innovations(t, z, r, pre, q, kind)


def smooth_axis_tiles(t, m, P, q, kind, first=0, tile=TILE):
    """k_smooth<false>, k_smooth_carry, k_smooth<true>: the same backwards (total (x) carry, last element (x) carry)."""
    e = smooth_elements(t, m, P, q, kind)
    frags = fragments(first, len(t), tile)
    carry, carries = np.zeros(9, kind), [None] * len(frags)
    for f in range(len(frags) - 1, -1, -1):
        a, b = frags[f]
        carries[f] = carry
        total = tree_scan(e[a:b], smooth_combine, backward=True)[0]
        carry = _state(smooth_combine(total[None], carry[None])[0])
    suf = np.zeros_like(e)
    for f, (a, b) in enumerate(frags):
        el = e[a:b].copy()
        if f + 1 < len(frags):       # a track's last fragment reads no carry
            el[-1] = smooth_combine(el[-1:], carries[f][None])[0]
        suf[a:b] = tree_scan(el, smooth_combine, backward=True)
    return suf[:, 4:6].copy(), suf[:, 6:9].copy()


# ------------------------------------------------------------------ the whole call
def run(tx, timestamp, x, y, rx, ry, valid=None, q=None, v0=10.0, gate=GATE_999, max_rounds=4, kind=np.float64,
        form="sequential", smoother=True, tile=TILE):
    """thr_track.  `nis_rounds`: the nis of every filter run (for the gate's margin); `masks`: the mask every filter
    run was made with.  `tile` matters to form="tiles" alone."""
    n = len(tx)
    order, track_tx, track_ptr = sort_rows(tx, timestamp)
    valid = np.ones(n, dtype=bool) if valid is None else np.asarray(valid).astype(bool)
    cols = [np.asarray(v, dtype=np.float64).astype(kind) for v in (timestamp, x, y, rx, ry)]
    q, v0 = kind(q), kind(v0)
    filt_fn = {"sequential": filter_axis, "scan": filter_axis_scan, "tiles": filter_axis_tiles}[form]
    smooth_fn = {"sequential": smooth_axis, "scan": smooth_axis_scan, "tiles": smooth_axis_tiles}[form]
    nt = len(track_tx)
    out = {"order": order, "track_tx": track_tx, "track_ptr": track_ptr, "used": np.zeros(n, np.uint8),
           "nis": np.full(n, np.nan, kind), "filt": np.full((n, 4), np.nan, kind), "filt_var": np.full((n, 6), np.nan, kind),
           "smooth": np.full((n, 4), np.nan, kind), "smooth_var": np.full((n, 6), np.nan, kind),
           "track_stats": np.zeros((nt, 8), kind), "track_flags": np.zeros(nt, np.int32)}
    tracks, where = [], []      # a track's rows from the start row on; form="tiles": the sorted position of the first
    for c in range(nt):
        rows = order[track_ptr[c]:track_ptr[c + 1]]
        ok = np.flatnonzero(valid[rows])
        rows = rows[ok[0]:] if len(ok) else rows[:0]       # from the start row on
        tracks.append(rows)
        where.append(dict(first=int(track_ptr[c] + (ok[0] if len(ok) else 0)), tile=tile) if form == "tiles" else {})
    mask = valid.copy()
    rounds, converged, nis_rounds, masks = 0, 0, [], []

    def one_run():
        nis = np.full(n, np.nan, kind)
        masks.append(mask.copy())
        for rows, at in zip(tracks, where):
            if not len(rows):
                continue
            t = cols[0][rows]
            value = np.zeros(len(rows), kind)
            for axis in range(2):
                m, P, nu, S = filt_fn(t, cols[1 + axis][rows], cols[3 + axis][rows], mask[rows], q, v0, kind, **at)
                out["filt"][rows, 2 * axis:2 * axis + 2], out["filt_var"][rows, 3 * axis:3 * axis + 3] = m, P
                value = value + nu * nu / S
            value[0] = 0
            nis[rows] = np.where(valid[rows], value, np.nan)
        nis_rounds.append(nis)
        return nis

    for _ in range(int(max_rounds)):
        nis = one_run()
        rounds += 1
        new = valid & np.isfinite(nis)
        if gate > 0:
            with np.errstate(invalid="ignore"):
                new &= nis <= kind(gate)
        if np.array_equal(new, mask):
            converged = 1
            break
        mask = new
    if not converged:
        nis = one_run()
        rounds += 1
    tracked = np.zeros(n, dtype=bool)
    for rows in tracks:
        tracked[rows] = True
    out["nis"] = nis
    out["used"] = (mask & tracked).astype(np.uint8)
    for c, rows in enumerate(tracks):
        all_rows = order[track_ptr[c]:track_ptr[c + 1]]
        stats = out["track_stats"][c]
        stats[0], stats[1] = len(all_rows), np.count_nonzero(valid[all_rows])
        stats[2] = np.count_nonzero(out["used"][all_rows])
        stats[3] = stats[1] - stats[2]
        stats[4:] = np.nan
        if not len(rows):
            continue
        t = cols[0][rows]
        if smoother:
            for axis in range(2):
                ms, Ps = smooth_fn(t, out["filt"][rows, 2 * axis:2 * axis + 2], out["filt_var"][rows, 3 * axis:3 * axis + 3], q, kind,
                                       **where[c])
                out["smooth"][rows, 2 * axis:2 * axis + 2], out["smooth_var"][rows, 3 * axis:3 * axis + 3] = ms, Ps
        used = out["used"][rows].astype(bool)
        sm = out["smooth"][rows]
        dx, dy = np.diff(sm[:, 0]), np.diff(sm[:, 2])
        stats[4] = nis[rows][used].sum() / kind(used.sum()) if used.any() else np.nan
        stats[5] = t[-1] - t[0]
        stats[6] = np.sqrt(dx * dx + dy * dy).sum()
        stats[7] = np.sqrt(sm[:, 1] * sm[:, 1] + sm[:, 3] * sm[:, 3]).sum() / kind(len(rows))
        out["track_flags"][c] = LOST if 2 * stats[2] < stats[1] else 0
    out["counts"] = {"rows": n, "tracks": nt, "used": int(out["used"].sum()),
                     "rejected": int(np.count_nonzero(valid & tracked) - out["used"].sum()), "rounds": rounds, "converged": converged}
    out["nis_rounds"] = nis_rounds
    out["masks"] = masks
    out["tracked"] = tracked
    return out
