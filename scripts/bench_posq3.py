"""Measurement: `thr_posq3` beside `thr_pos3` on scripts/bench_pos3.py's scene (8 antennas at 5 .. 200 m on a jittered
ring of 1000 m, transmitters at 0 .. 3 m, --groups groups of all 28 receiver pairs, 10 ns of TDOA noise), in both modes.
Six legs, alternated inside every repeat so that they share the box's state, one warm-up round first:

  pos3_known / pos3_free_z            thr_pos3: the yardstick (kernel = `thr_debug_pos3_times`' middle entry);
  posq3_known / posq3_free_z          thr_posq3 without a gate: its full solves are thr_pos3's solve;
  posq3_known_gate / posq3_free_z_gate  thr_posq3 at a gate of --gate metres with one receiver's arrival --delay metres
                                      late in --share of the groups: the flagged groups, the candidates, how many planted
                                      receivers were excluded and how many others.

Per leg: median and range over --repeats of every part `thr_debug_posq3_times` reports and of the wall time.

--parent-lib FILE adds the comparison the header change is accepted by: thr_pos3's kernel (both modes) and thr_posg3's
two solve stages (task 0 + refinement, both modes, --groups-posg3 groups) with the library of this tree and with FILE
(a build of the parent commit), each in a fresh process, five rounds of --repeats calls each, the builds alternated.
Per build the five medians; `spread_parent` is max - min of the parent's five, `diff` the difference of the two
medians of medians, `within_spread` whether |diff| <= spread_parent.  Writes one JSON record (default
profiles/r29_posq3.json); no figure is asserted anywhere."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402

import bench_pos  # noqa: E402
import bench_pos3  # noqa: E402
from thrifty_amd import _native, build, pos_3d_global, pos_est  # noqa: E402

POSQ3_PARTS = ("copies_in_ms", "full_solves_ms", "flags_and_expansion_ms", "candidates_ms", "choice_and_residuals_ms", "copies_out_ms")
ROUNDS = 5


def solve_stage_child(groups, groups_posg3, repeats):
    """One process, one library: the medians of thr_pos3's kernel and of thr_posg3's solve stages -> one JSON line."""
    rec = {}
    ptr, rx0, rx1, _, snr, table = bench_pos.scene(groups)
    xyz, tdoa, group_h = bench_pos3.tall_scene(groups, table, rx0, rx1)
    z0 = float(xyz[:, 2].min()) - 1.0
    calls = {"pos3_known": lambda: _native.pos3(ptr, rx0, rx1, tdoa, snr, xyz, _native.POS3_KNOWN_HEIGHT, group_h),
             "pos3_free_z": lambda: _native.pos3(ptr, rx0, rx1, tdoa, snr, xyz, _native.POS3_FREE_Z, None, (0.1, 0.1, z0))}
    n = groups_posg3
    sub = (ptr[:n + 1], rx0[:28 * n], rx1[:28 * n], tdoa[:28 * n], snr[:28 * n], xyz)
    margin = float(np.max(table.max(axis=0) - table.min(axis=0)))
    z_grid = pos_3d_global.default_z_grid(xyz)
    calls["posg3_known"] = lambda: _native.posg3(*sub, _native.POS3_KNOWN_HEIGHT, margin, group_h=group_h[:n], grid_z=1)
    calls["posg3_free_z"] = lambda: _native.posg3(*sub, _native.POS3_FREE_Z, margin, x0=(0.1, 0.1, z0), z_grid=z_grid)
    times = {name: [] for name in calls}
    for name, call in calls.items():
        call()                                                          # warm-up
    for _ in range(repeats):
        for name, call in calls.items():
            call()
            if name.startswith("posg3"):
                ms = _native.posg3_times()
                times[name].append(ms[1] + ms[4])                       # task 0 and the refinement: the team solves
            else:
                times[name].append(_native.pos3_times()[1])
    rec = {name: statistics.median(values) for name, values in times.items()}
    print(json.dumps(rec), flush=True)


def header_comparison(parent_lib, args):
    """Five fresh processes per build, alternated -> the record described in the module docstring."""
    builds = {"parent": os.path.abspath(parent_lib), "this": _native.LIB_PATH}
    medians = {name: {} for name in builds}
    for _ in range(ROUNDS):
        for name, lib in builds.items():
            env = dict(os.environ, THRIFTY_HIP_LIB=lib)
            line = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--solve-stage-child", "--groups", str(args.groups),
                                            "--groups-posg3", str(args.groups_posg3), "--repeats", str(args.repeats)], env=env)
            for leg, value in json.loads(line.decode().strip().splitlines()[-1]).items():
                medians[name].setdefault(leg, []).append(value)
    rec = {"rounds": ROUNDS, "repeats_per_round": args.repeats, "groups": args.groups, "groups_posg3": args.groups_posg3, "legs": {}}
    for leg in medians["this"]:
        parent, this = medians["parent"][leg], medians["this"][leg]
        spread, diff = max(parent) - min(parent), statistics.median(this) - statistics.median(parent)
        rec["legs"][leg] = {"parent_medians_ms": parent, "this_medians_ms": this, "spread_parent_ms": spread, "diff_ms": diff,
                            "within_spread": bool(abs(diff) <= spread)}
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--groups-posg3", type=int, default=1 << 14, help="groups of the thr_posg3 legs of --parent-lib")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--share", type=float, default=0.01, help="share of the groups with a late arrival")
    ap.add_argument("--delay", type=float, default=150.0, help="metres")
    ap.add_argument("--gate", type=float, default=10.0, help="metres; the scene's TDOA noise is 3 m")
    ap.add_argument("--parent-lib", help="a build of the parent commit to compare thr_pos3's and thr_posg3's solves with")
    ap.add_argument("--solve-stage-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "r29_posq3.json"))
    args = ap.parse_args()
    if args.solve_stage_child:
        return solve_stage_child(args.groups, args.groups_posg3, args.repeats)
    # the children first: this process has not opened the device yet
    comparison = header_comparison(args.parent_lib, args) if args.parent_lib else None
    ptr, rx0, rx1, _, snr, table = bench_pos.scene(args.groups)
    xyz, tdoa, group_h = bench_pos3.tall_scene(args.groups, table, rx0, rx1)
    z0 = float(xyz[:, 2].min()) - 1.0
    rng = np.random.default_rng(12)
    late = rng.random(args.groups) < args.share
    which = rng.integers(0, bench_pos.N_RX, args.groups)
    row_late, row_which = np.repeat(late, 28), np.repeat(which, 28)
    shift = args.delay / pos_est.SPEED_OF_LIGHT
    planted = tdoa + shift * (row_late & (rx0 == row_which)) - shift * (row_late & (rx1 == row_which))
    known = dict(mode=_native.POS3_KNOWN_HEIGHT, group_h=group_h)
    free = dict(mode=_native.POS3_FREE_Z, x0=(0.1, 0.1, z0))
    cols = (ptr, rx0, rx1, tdoa, snr, xyz)
    late_cols = (ptr, rx0, rx1, planted, snr, xyz)
    legs = {
        "pos3_known": lambda: _native.pos3(*cols, _native.POS3_KNOWN_HEIGHT, group_h),
        "pos3_free_z": lambda: _native.pos3(*cols, _native.POS3_FREE_Z, None, (0.1, 0.1, z0)),
        "posq3_known": lambda: _native.posq3(*cols, **known),
        "posq3_free_z": lambda: _native.posq3(*cols, **free),
        "posq3_known_gate": lambda: _native.posq3(*late_cols, gate_m=args.gate, **known),
        "posq3_free_z_gate": lambda: _native.posq3(*late_cols, gate_m=args.gate, **free),
    }
    out = {name: call() for name, call in legs.items()}                # warm-up, every leg
    wall, parts = {name: [] for name in legs}, {name: [] for name in legs}
    for _ in range(args.repeats):
        for name, call in legs.items():                                # alternated: a drift of the box reaches all six
            t0 = time.perf_counter()
            out[name] = call()
            wall[name].append(time.perf_counter() - t0)
            parts[name].append(_native.pos3_times() if name.startswith("pos3") else _native.posq3_times())
    hashes = {}
    for name in ("pos3.hip", "posq3.hip", "pos3_lm.hpp"):            # (csrc_hash() leaves all three out)
        with open(os.path.join(build.CSRC, name), "rb") as f:
            hashes[name] = hashlib.sha256(f.read()).hexdigest()[:16]
    rec = {"csrc_hash": build.csrc_hash(), "sha256": hashes, "receivers": bench_pos.N_RX, "rows_per_group": 28,
           "radius_m": bench_pos.RADIUS, "noise_s": bench_pos.NOISE, "antenna_heights_m": [bench_pos3.Z_LO, bench_pos3.Z_HI],
           "tag_heights_m": [0.0, bench_pos3.TAG_Z], "z0_m": z0, "repeats": args.repeats, "groups": args.groups, "legs": {}}
    for name in legs:
        names = ("copies_in_ms", "kernel_ms", "copies_out_ms") if name.startswith("pos3") else POSQ3_PARTS
        leg = {"wall_ms": bench_pos.spread([1e3 * w for w in wall[name]])}
        leg.update({part: bench_pos.spread([p[k] for p in parts[name]]) for k, part in enumerate(names)})
        rec["legs"][name] = leg
    for mode in ("known", "free_z"):
        fixed, (counts, plain), (gated_counts, gated) = out["pos3_" + mode], out["posq3_" + mode], out["posq3_%s_gate" % mode]
        leg = rec["legs"]["posq3_" + mode]
        leg["same_bytes_as_thr_pos3"] = bool(all(plain[k].tobytes() == fixed[k].tobytes() for k in ("pos", "dop", "hdop", "vdop", "snr", "status", "iters"))
                                             and np.ascontiguousarray(plain["rms"][:, 0]).tobytes() == fixed["rms"].tobytes())
        leg["full_solves_over_thr_pos3_kernel"] = leg["full_solves_ms"]["median"] / rec["legs"]["pos3_" + mode]["kernel_ms"]["median"]
        excluded = gated["counts"][:, 2]
        rec["legs"]["posq3_%s_gate" % mode].update({
            "gate_m": args.gate, "delay_m": args.delay, "groups_with_a_late_arrival": int(late.sum()),
            "flagged": gated_counts["flagged"], "tasks": gated_counts["tasks"],
            "excluded_the_planted_receiver": int(np.count_nonzero(late & (excluded == which))),
            "excluded_another_receiver": int(np.count_nonzero((excluded >= 0) & ~(late & (excluded == which)))),
            "flag_counts": {str(k): int(v) for k, v in zip(*np.unique(gated["flags"], return_counts=True))}})
    del out
    if comparison is not None:
        rec["header_change_against_parent"] = comparison
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
