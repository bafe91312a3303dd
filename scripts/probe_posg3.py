"""A CPU count, not a device measurement: what the grid starts of `thr_posg3` recover on z_lost6's scene, by the NumPy
statement (tests/posg3_ref.py) alone.  --draws draws of 44 groups (six antennas at 2 .. 42 m on a ring of 300 m, 0.9 m
of noise, z free, the default options; tests/posg3_golden.py's ring scene without the cut groups).  A group is LOST when
the chosen solve is not OK, or its cost lies above that of a solve started AT the planted position (x (1 + 1e-9), plus
the rounding term of the residuals).  Prints the counts README.md quotes."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import pos3_ref  # noqa: E402
import pos_ref  # noqa: E402
import posg3_golden  # noqa: E402
import posg3_ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--draws", type=int, default=20)
    ap.add_argument("--seed", type=int, default=9000)
    args = ap.parse_args()
    total = dict(groups=0, lost_fixed=0, lost_global=0, unconverged_everywhere=0, neighbouring_minimum=0, other=0, local_minima=0.0)
    most_minima, farthest = 0, 0.0
    for draw in range(args.draws):
        s = posg3_golden.ring_scene(args.seed + draw, 6, 300.0, (2.0, 42.0), 3e-9, 44)
        table, ptr = s["table"], s["group_ptr"].tolist()
        margin = float(np.max(table[:, :2].max(axis=0) - table[:, :2].min(axis=0)))
        ref = posg3_ref.posg3_ref(s["group_ptr"], s["rx0"], s["rx1"], s["tdoa"], s["snr"], table, posg3_ref.FREE_Z, margin,
                                  x0=(0.1, 0.1, float(table[:, 2].min()) - 1.0), z_grid=posg3_golden.default_z_grid(table),
                                  maps=False, **posg3_golden.OPTIONS)
        total["local_minima"] += float(ref["n_local"].sum())
        most_minima = max(most_minima, int(ref["n_local"].max()))
        for g, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
            cols = (s["rx0"][a:b], s["rx1"][a:b], s["tdoa"][a:b], s["snr"][a:b], table)
            truth = pos3_ref.pos3_ref(*cols, posg3_ref.FREE_Z, 0.0, tuple(s["planted"][g]), None, 100)
            da = np.sqrt(np.sum((table[cols[0]] - s["planted"][g]) ** 2, axis=1))
            db = np.sqrt(np.sum((table[cols[1]] - s["planted"][g]) ** 2, axis=1))
            floor = float(np.sum((4.0 * 2.0 ** -53 * (np.abs(cols[2] * pos_ref.C) + da + db)) ** 2))
            limit = truth[4] ** 2 * (b - a) * (1 + 1e-9) + floor

            def lost(status, rms):
                return status != pos_ref.OK or not rms ** 2 * (b - a) <= limit

            total["groups"] += 1
            if lost(ref["task_status"][g, 0], ref["task_rms"][g, 0]):
                total["lost_fixed"] += 1
                farthest = max(farthest, float(np.sqrt(np.sum((ref["task_pos"][g, 0] - truth[0]) ** 2))))
            if lost(ref["status"][g], ref["rms"][g]):
                total["lost_global"] += 1
                exists = ref["task_status"][g] != posg3_ref.NO_TASK
                if truth[6] == pos_ref.UNCONVERGED and np.all(ref["task_status"][g][exists] == pos_ref.UNCONVERGED):
                    total["unconverged_everywhere"] += 1
                elif ref["status"][g] == pos_ref.OK:
                    total["neighbouring_minimum"] += 1
                else:
                    total["other"] += 1
    total["local_minima"] /= total["groups"]
    print("CPU counts over %d draws: %s; at most %d local-minimum cells; the fixed start's lost groups end up to %.0f m away" % (
        args.draws, total, most_minima, farthest))


if __name__ == "__main__":
    main()
