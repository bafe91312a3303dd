#!/usr/bin/env python
"""Fixtures of `thr_posg` (tests/golden/posg/*.npz): small scenes, the planted positions, and what the NumPy
statement (tests/posg_ref.py) makes of them.  Nothing of the reference is read.

    python tests/golden/make_golden_posg.py

far4       4 receivers on a jittered ring of 100 m centred on (5000, -3000) m, every pair, 0.3 m of noise per arrival,
           the tag inside the ring: the fixed start (0.1, 0.1) loses a share of the groups.
far8       8 receivers, 3 m of noise, the same offset.
three_out  3 receivers at the origin, the tag outside the ring: the two intersections of the hyperbolae fit equally
           (floor_m = 1 m).
clean6     6 receivers at the origin, the tag inside: nothing moves, nothing is ambiguous.

The generator ASSERTS, on the statement alone, the six properties listed in `check` -- among them the margins that
make the discrete outputs (cells, task, n_minima, flags) safe to compare exactly with the device's."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import pos_ref  # noqa: E402
import posg_golden  # noqa: E402
import posg_ref  # noqa: E402


def check(name, s, ref, opts):
    n = len(s["planted"])
    ptr = s["group_ptr"].tolist()
    elig = ref["task_status"] == pos_ref.OK
    # 1. the fixed start loses groups in the far scenes
    lost = np.hypot(*(ref["task_pos"][:, 0] - s["planted"]).T) > 10.0
    if name in ("far4", "far8"):
        assert lost.sum() >= 4, (name, int(lost.sum()))
    # 2. the chosen cost is at most that of a solve started AT the planted position.  With three receivers both
    # intersections fit EXACTLY (two independent TDOAs, two unknowns): both costs are rounding noise of some 1e-27 m^2
    # and a purely relative bound says nothing there, so the squared rounding error of the residuals themselves is
    # allowed on top: sum_r (4 2^-53 (|tc_r| + da_r + db_r))^2, some 1e-25 m^2 -- nothing beside a real cost.
    for g in range(n):
        if not elig[g].any():
            continue
        a, b = ptr[g], ptr[g + 1]
        truth = posg_ref.solve_task(s["rx0"][a:b], s["rx1"][a:b], s["tdoa"][a:b], s["snr"][a:b], s["table"], s["planted"][g], 100)
        da = np.hypot(*(s["table"][s["rx0"][a:b]] - s["planted"][g]).T)
        db = np.hypot(*(s["table"][s["rx1"][a:b]] - s["planted"][g]).T)
        floor = float(np.sum((4.0 * 2.0 ** -53 * (np.abs(s["tdoa"][a:b] * pos_ref.C) + da + db)) ** 2))
        assert ref["rms"][g] ** 2 * (b - a) <= truth[2] ** 2 * (b - a) * (1 + 1e-9) + floor, (name, g, ref["rms"][g], truth[2])
    # 3., 4.
    if name == "three_out":
        assert np.count_nonzero(ref["flags"] & posg_ref.AMBIGUOUS) >= 5
    if name == "clean6":
        assert not np.any(ref["flags"] & (posg_ref.AMBIGUOUS | posg_ref.MOVED))
    # 5. neighbouring cells, and the local minima among each other, differ by at least 1e-9 relative
    for g in range(n):
        F = ref["map"][g]
        if np.all(np.isnan(F)):
            continue
        G = F.shape[0]
        for dj, di in ((0, 1), (1, 0), (1, 1), (1, -1)):
            j0, j1, i0, i1 = max(0, -dj), G - max(0, dj), max(0, -di), G - max(0, di)
            x, y = F[j0:j1, i0:i1], F[j0 + dj:j1 + dj, i0 + di:i1 + di]
            assert np.all(np.abs(x - y) >= 1e-9 * np.maximum(x, y)), (name, g, dj, di)
        low = np.sort(F[ref["map_min"][g].astype(bool)])
        assert np.all(np.diff(low) >= 1e-9 * low[1:]), (name, g)
    # 6. no pair of eligible tasks within 1e-6 m of merge_m, no rms2 within 1e-6 relative of the threshold
    d = ref["task_pos"][:, :, None, :] - ref["task_pos"][:, None, :, :]
    dist = np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2)
    both = elig[:, :, None] & elig[:, None, :]
    assert not np.any(both & (np.abs(dist - opts["merge_m"]) <= 1e-6)), name
    # (pairs of tasks that ended in one minimum lie some 1e-9 m apart, pairs in two minima metres: the rms order of a
    # pair in one minimum is not safe, but it changes neither n_minima nor the second nor the flags)
    has2 = ~np.isnan(ref["rms2"])
    limit = np.fmax(opts["ratio"] * ref["rms"][has2], opts["floor_m"])
    assert not np.any(np.abs(ref["rms2"][has2] - limit) <= 1e-6 * limit), name
    # is the ORDER of a group's distinct minima safe?  Their rms differ by far more than the iteration's rounding --
    # except where two minima both fit exactly (three receivers): which of two residuals of 1e-14 m is the smaller is
    # decided by rounding, and with it task, the MOVED flag and which of the two positions is the second
    safe = np.ones(n, dtype=bool)
    for g in range(n):
        reps = [t for t in range(elig.shape[1]) if elig[g, t] and not any(elig[g, u] and dist[g, t, u] <= 0.5 for u in range(t))]
        r = np.sort(ref["task_rms"][g, reps])
        safe[g] = bool(np.all(np.diff(r) >= 1e-6 * r[1:]))
        assert safe[g] or (name == "three_out" and np.all(r < 1e-9)), (name, g, r)
    ref["order_safe"] = safe
    return int(lost.sum())


def main():
    os.makedirs(posg_golden.GOLDEN, exist_ok=True)
    for name in posg_golden.SETS:
        seed, n_rx, n_groups, noise, outside, offset, floor_m = posg_golden.SCENES[name]
        s = posg_golden.scene(seed, n_rx, n_groups, noise, outside=outside, offset=offset)
        opts = dict(posg_golden.OPTIONS, margin_m=posg_golden.margin_of(s["table"]), floor_m=floor_m)
        ref = posg_ref.posg_ref(s["group_ptr"], s["rx0"], s["rx1"], s["tdoa"], s["snr"], s["table"], **opts)
        lost = check(name, s, ref, opts)
        rx_ids = np.arange(n_rx, dtype=np.int32) * 3 + 11         # receiver ids that are no dense indices
        data = {"rx_ids": rx_ids, "rx_xy": s["table"], "group_ptr": s["group_ptr"], "rx0": rx_ids[s["rx0"]], "rx1": rx_ids[s["rx1"]],
                "tdoa": s["tdoa"], "snr": s["snr"], "planted": s["planted"], "group_id": np.arange(n_groups, dtype=np.int32) + 100,
                "timestamp": 1700000000.0 + 0.25 * np.arange(n_groups), "lost_by_the_fixed_start": np.int64(lost)}
        data.update({key: np.array(value) for key, value in opts.items()})
        data.update({"ref_" + key: ref[key] for key in posg_golden.RECORDED})
        path = os.path.join(posg_golden.GOLDEN, name + ".npz")
        np.savez_compressed(path, **data)
        flags = ref["flags"]
        print("%-10s %2d groups, %2d lost by the fixed start, %2d moved, %2d ambiguous, %2d without a minimum, %6d bytes" % (
            name, n_groups, lost, np.count_nonzero(flags & 1), np.count_nonzero(flags & 2), np.count_nonzero(flags & 4),
            os.path.getsize(path)))


if __name__ == "__main__":
    main()
