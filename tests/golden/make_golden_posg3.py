#!/usr/bin/env python
"""Fixtures of `thr_posg3` (tests/golden/posg3/*.npz): small scenes, the planted positions, and what the NumPy
statement (tests/posg3_ref.py) makes of them.  Nothing of the reference is read; z_tall6g takes its receivers from
tests/golden/pos3/z_tall6.npz.

    python tests/golden/make_golden_posg3.py

z_lost6    z_ring6's scene (tests/golden/make_golden_pos3.py): six antennas at 2 .. 42 m on a ring of 300 m, a random
           share of the pairs, 3 ns (0.9 m) of noise per TDOA, 44 groups and 4 that name one receiver too few; z free,
           the default options.  The fixed start loses a share of the groups to minima far above or below the antennas.
z_mirror6  six antennas all at 30 m on a ring of 100 m, 1 ns of noise, tags at 0 .. 3 m, z_grid = (-10, 70), 32 groups:
           the cost is exactly even about z = 30 m, both mirror minima fit equally.
h_far4     the height is known: posg's far4 scene (4 receivers on a ring of 100 m centred on (5000, -3000) m, every pair,
           0.3 m of noise per arrival) with antenna heights of 2 .. 32 m and a height per group.
z_tall6g   z_tall6's receivers (2 .. 82 m on 100 m), 1 ns of noise: nothing moves, nothing is ambiguous.

The generator ASSERTS, on the statement alone, every condition listed in `check`.  A draw that fails is printed and the
WHOLE set is drawn again with another seed (at most 20 attempts); it is never thinned.

One condition needs a word.  Neighbouring cells, and the local minima among each other, must differ by at least 1e-9
relative, so that no rounding decides a comparison.  In z_mirror6 the planes lie symmetrically about the antennas' plane
and vz enters only as vz * vz: mirrored cells hold EQUAL bits in any arithmetic, here and on the device, and the order of
such a pair is decided by the cell number on both sides.  Cells of neighbouring planes and pairs of local minima that are
equal to the bit are therefore let through in that set (and only there); every other pair keeps the margin."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import pos3_ref  # noqa: E402
import pos_ref  # noqa: E402
import posg3_golden  # noqa: E402
import posg3_ref  # noqa: E402
import posg_golden  # noqa: E402

FREE_Z, KNOWN_HEIGHT = posg3_ref.FREE_Z, posg3_ref.KNOWN_HEIGHT


class Redraw(Exception):
    pass


def need(condition, *what):
    if not condition:
        raise Redraw(" ".join(str(w) for w in what))


def planted_solves(s, mode, group_h, z_range):
    """Per group, pos3_ref started AT the planted position: (pos[3], rms, status)."""
    ptr = s["group_ptr"].tolist()
    res = []
    for g, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
        h = 0.0 if mode == FREE_Z else float(group_h[g])
        r = pos3_ref.pos3_ref(s["rx0"][a:b], s["rx1"][a:b], s["tdoa"][a:b], s["snr"][a:b], s["table"], mode, h,
                              tuple(s["planted"][g]), z_range, 100)
        res.append((r[0], r[4], r[6]))
    return res


def lost_by_task0(s, ref, truth, uncut):
    """Groups whose task 0 is not OK or ends more than 10 m (3-D) from the solve started at the planted position."""
    far = np.array([np.sqrt(np.sum((ref["task_pos"][g, 0] - truth[g][0]) ** 2)) > 10.0 for g in range(len(truth))])
    return uncut & ((ref["task_status"][:, 0] != pos_ref.OK) | far)


def check(name, s, ref, opts, mode, truth, uncut):
    n = len(s["planted"])
    ptr = s["group_ptr"].tolist()
    free_z = mode == FREE_Z
    elig = ref["task_status"] == pos_ref.OK
    lost = lost_by_task0(s, ref, truth, uncut)
    # 1. what the fixed start loses
    if name in ("z_lost6", "h_far4"):
        need(lost.sum() >= 5, name, "the fixed start loses only", int(lost.sum()))
    # 2. for EVERY uncut group the chosen task is eligible and its cost is at most that of the solve started at the
    # planted position x (1 + 1e-9), plus posg's rounding term sum_r (4 2^-53 (|tc_r| + da_r + db_r))^2
    if name in ("z_lost6", "h_far4"):
        for g in np.flatnonzero(uncut).tolist():
            a, b = ptr[g], ptr[g + 1]
            need(elig[g, ref["task"][g]], name, "group", g, "has no eligible task")
            da = np.sqrt(np.sum((s["table"][s["rx0"][a:b]] - s["planted"][g]) ** 2, axis=1))
            db = np.sqrt(np.sum((s["table"][s["rx1"][a:b]] - s["planted"][g]) ** 2, axis=1))
            floor = float(np.sum((4.0 * 2.0 ** -53 * (np.abs(s["tdoa"][a:b] * pos_ref.C) + da + db)) ** 2))
            need(ref["rms"][g] ** 2 * (b - a) <= truth[g][1] ** 2 * (b - a) * (1 + 1e-9) + floor,
                 name, "group", g, "stays above the planted-start cost:", ref["rms"][g], truth[g][1])
    # 3. the mirror
    if name == "z_mirror6":
        both = posg3_ref.AMBIGUOUS | posg3_ref.MIRROR
        marked = (ref["flags"] & both) == both
        need(marked.sum() >= 16, name, "only", int(marked.sum()), "groups are AMBIGUOUS | MIRROR")
        plane = float(s["table"][0, 2])
        mirrored = ref["pos"] * np.array([1.0, 1.0, -1.0]) + np.array([0.0, 0.0, 2.0 * plane])
        need(np.all(np.sqrt(np.sum((ref["pos2"] - mirrored)[marked] ** 2, axis=1)) <= 1e-6), name, "pos2 is not the mirrored best")
    # 4. nothing moves
    if name == "z_tall6g":
        need(not np.any(ref["flags"] & (posg3_ref.AMBIGUOUS | posg3_ref.MOVED)), name, "flags", ref["flags"].tolist())
    # 5. neighbouring cells, and the local minima among each other, differ by at least 1e-9 relative (equal bits of a
    # mirrored pair in z_mirror6: the module docstring)
    for g in range(n):
        F = ref["map"][g]
        if np.all(np.isnan(F)):
            continue
        gz, G = F.shape[0], F.shape[1]
        for dk, dj, di in [d for d in posg3_ref.NEIGHBOURS if d > (0, 0, 0)]:
            k0, k1 = max(0, -dk), gz - max(0, dk)
            j0, j1, i0, i1 = max(0, -dj), G - max(0, dj), max(0, -di), G - max(0, di)
            x, y = F[k0:k1, j0:j1, i0:i1], F[k0 + dk:k1 + dk, j0 + dj:j1 + dj, i0 + di:i1 + di]
            apart = (np.abs(x - y) >= 1e-9 * np.maximum(x, y)) | ((x == y) if name == "z_mirror6" and dk else False)
            need(np.all(apart), name, "group", g, "neighbouring cells too close", (dk, dj, di))
        low = np.sort(F[ref["map_min"][g].astype(bool)])
        gaps = np.diff(low)
        fine = (gaps >= 1e-9 * low[1:]) | ((gaps == 0.0) if name == "z_mirror6" else False)
        need(np.all(fine), name, "group", g, "local minima too close")
    # 6. no pair of eligible tasks within 1e-6 m of merge_m (both distances), no rms2 within 1e-6 relative of the threshold
    d = ref["task_pos"][:, :, None, :] - ref["task_pos"][:, None, :, :]
    flat = np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2)
    dist = np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2 + d[..., 2] ** 2)
    both = elig[:, :, None] & elig[:, None, :]
    with np.errstate(invalid="ignore"):
        need(not np.any(both & (np.abs(dist - opts["merge_m"]) <= 1e-6)), name, "a task pair at merge_m")
        need(not np.any(both & (np.abs(flat - opts["merge_m"]) <= 1e-6)), name, "a task pair at merge_m horizontally")
    has2 = ~np.isnan(ref["rms2"])
    limit = np.fmax(opts["ratio"] * ref["rms"][has2], opts["floor_m"])
    need(not np.any(np.abs(ref["rms2"][has2] - limit) <= 1e-6 * limit), name, "an rms2 at its threshold")
    # is the ORDER of a group's distinct minima safe?  Their rms differ by far more than the iteration's rounding --
    # except between the two mirror minima of z_mirror6, whose costs are equal: which is "best" is rounding noise there,
    # and with it task, the MOVED flag and which of the two positions is the second (three_out's case in posg)
    merge = dist if free_z else flat
    safe = np.ones(n, dtype=bool)
    for g in range(n):
        reps = [t for t in range(elig.shape[1]) if elig[g, t] and not any(elig[g, u] and merge[g, t, u] <= 0.5 for u in range(t))]
        r = np.sort(ref["task_rms"][g, reps])
        safe[g] = bool(np.all(np.diff(r) >= 1e-6 * r[1:]))
        need(safe[g] or name == "z_mirror6", name, "group", g, "two minima of equal cost", r)
    ref["order_safe"] = safe
    return int(lost.sum())


def draw(name, seed):
    """-> (scene, mode, group_h, z0, z_grid, cut groups, rx ids)"""
    if name == "z_lost6":
        cut = (5, 6, 20, 33)
        s = posg3_golden.ring_scene(seed, 6, 300.0, (2.0, 42.0), 3e-9, 48, cut=cut)
        return s, FREE_Z, None, cut
    if name == "z_mirror6":
        s = posg3_golden.ring_scene(seed, 6, 100.0, (30.0, 30.0), 1e-9, 32)
        return s, FREE_Z, None, ()
    if name == "z_tall6g":
        with np.load(os.path.join(HERE, "pos3", "z_tall6.npz")) as tall:
            table = tall["rx_xyz"]
        s = posg3_golden.ring_scene(seed, 6, 100.0, None, 1e-9, 24, table=table)
        return s, FREE_Z, None, ()
    if name == "h_far4":
        flat = posg_golden.scene(seed, 4, 32, 0.3, offset=posg_golden.OFFSET)
        rng = np.random.default_rng(seed + 77)
        table = np.c_[flat["table"], rng.permutation(np.linspace(2.0, 32.0, 4))]
        heights = rng.uniform(0.0, 3.0, 32)
        planted = np.c_[flat["planted"], heights]
        # the arrivals again, in three coordinates, with the same noise level
        ptr = flat["group_ptr"].tolist()
        tdoa = np.zeros(len(flat["rx0"]))
        for g in range(32):
            arrival = np.linalg.norm(table - planted[g], axis=1) + rng.normal(0, 0.3, 4)
            rows = slice(ptr[g], ptr[g + 1])
            tdoa[rows] = (arrival[flat["rx0"][rows]] - arrival[flat["rx1"][rows]]) / posg3_golden.C
        s = dict(flat, table=table, planted=planted, tdoa=tdoa)
        return s, KNOWN_HEIGHT, heights, ()
    raise KeyError(name)


def make(name, seed0):
    for attempt in range(20):
        seed = seed0 + 1000 * attempt
        s, mode, group_h, cut = draw(name, seed)
        n = len(s["planted"])
        free_z = mode == FREE_Z
        uncut = np.array([g not in cut for g in range(n)])
        z0 = float(s["table"][:, 2].min()) - 1.0
        z_grid = (-10.0, 70.0) if name == "z_mirror6" else posg3_golden.default_z_grid(s["table"])
        opts = dict(posg3_golden.OPTIONS, margin_m=posg_golden.margin_of(s["table"][:, :2]))
        if not free_z:
            opts["grid_z"] = 1
        try:
            truth = planted_solves(s, mode, group_h, None)
            if name in ("z_lost6", "h_far4"):      # the cheap condition first: task 0 alone
                zero = posg3_ref.posg3_ref(s["group_ptr"], s["rx0"], s["rx1"], s["tdoa"], s["snr"], s["table"], mode, group_h=group_h,
                                           x0=(0.1, 0.1, z0 if free_z else 0.0), z_grid=z_grid if free_z else None,
                                           **dict(opts, grid=2, grid_z=2 if free_z else 1, starts=1))
                need(lost_by_task0(s, zero, truth, uncut).sum() >= 5, name, "the fixed start loses only",
                     int(lost_by_task0(s, zero, truth, uncut).sum()))
            ref = posg3_ref.posg3_ref(s["group_ptr"], s["rx0"], s["rx1"], s["tdoa"], s["snr"], s["table"], mode, group_h=group_h,
                                      x0=(0.1, 0.1, z0 if free_z else 0.0), z_grid=z_grid if free_z else None, **opts)
            lost = check(name, s, ref, opts, mode, truth, uncut)
        except Redraw as why:
            print("   seed %d: %s: the whole set again" % (seed, why))
            continue
        n_rx = len(s["table"])
        rx_ids = np.arange(n_rx, dtype=np.int32) * 3 + 11         # receiver ids that are no dense indices
        data = {"rx_ids": rx_ids, "rx_xyz": s["table"], "group_ptr": s["group_ptr"], "rx0": rx_ids[s["rx0"]], "rx1": rx_ids[s["rx1"]],
                "tdoa": s["tdoa"], "snr": s["snr"], "planted": s["planted"], "group_id": np.arange(n, dtype=np.int32) + 100,
                "timestamp": 1700000000.0 + 0.25 * np.arange(n), "group_tx": np.full(n, 7, dtype=np.int32),
                "free_z": np.bool_(free_z), "group_h": np.zeros(0) if free_z else group_h, "z0": np.float64(z0 if free_z else np.nan),
                "z_grid": np.array(z_grid if free_z else (), dtype=np.float64), "uncut": uncut, "seed": np.int64(seed),
                "lost_by_the_fixed_start": np.int64(lost),
                "planted_pos": np.array([t[0] for t in truth]), "planted_rms": np.array([t[1] for t in truth])}
        data.update({key: np.array(value) for key, value in opts.items()})
        data.update({"ref_" + key: ref[key] for key in posg3_golden.RECORDED})
        path = os.path.join(posg3_golden.GOLDEN, name + ".npz")
        np.savez_compressed(path, **data)
        flags = ref["flags"]
        print("%-10s seed %5d: %2d groups, %2d lost by the fixed start, %2d moved, %2d ambiguous, %2d mirror, %2d without a minimum, "
              "local minima %.2f in the mean and %d at most, %6d bytes" % (
                  name, seed, n, lost, np.count_nonzero(flags & 1), np.count_nonzero(flags & 2), np.count_nonzero(flags & 8),
                  np.count_nonzero(flags & 4), ref["n_local"][uncut].mean(), ref["n_local"].max(), os.path.getsize(path)))
        assert n <= 64 and os.path.getsize(path) <= 64 * 1024
        return
    raise AssertionError(name)


if __name__ == "__main__":
    os.makedirs(posg3_golden.GOLDEN, exist_ok=True)
    for set_name, first_seed in (("z_lost6", 35), ("z_mirror6", 41), ("h_far4", 0), ("z_tall6g", 43)):
        if len(sys.argv) < 2 or set_name in sys.argv[1:]:
            make(set_name, first_seed)
