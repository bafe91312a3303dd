"""The posg3 fixtures (tests/golden/posg3/*.npz, made by tests/golden/make_golden_posg3.py) and the scenes the host and
GPU tests of `thr_posg3` share: the ring scenes of tests/golden/make_golden_pos3.py (a jittered ring of antennas at
stated heights, a random share of the receiver pairs, Gaussian noise on each TDOA, tags at 0 .. 3 m inside 0.6 of the
ring); the generator lifts tests/posg_golden.py's far scene to three coordinates itself."""
import itertools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "posg3")
SETS = ("z_lost6", "z_mirror6", "h_far4", "z_tall6g")
C = 2.997e8
KNOWN_HEIGHT, FREE_Z = 0, 1
OPTIONS = dict(grid=32, grid_z=8, starts=4, merge_m=1.0, ratio=2.0, floor_m=0.0)
# the statement's outputs a fixture records ("ref_" + name)
RECORDED = ("task_pos", "task_rms", "task_status", "start_cell", "start_f", "n_local", "task", "pos", "rms", "pos2", "rms2",
            "n_minima", "flags", "map_min", "order_safe")
_cache = {}


def load(name):
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, name + ".npz")) as g:
            _cache[name] = {key: g[key] for key in g.files}
        for value in _cache[name].values():
            value.setflags(write=False)
    return _cache[name]


def rx_pos(g):
    """The receivers as the dict the public interface takes, in the fixture's order."""
    return {int(r): np.array(xyz) for r, xyz in zip(g["rx_ids"], g["rx_xyz"])}


def dense(g, column):
    index = {int(r): k for k, r in enumerate(g["rx_ids"])}
    return np.array([index[int(v)] for v in column], dtype=np.int32)


def columns(g):
    """(group_ptr, rx0, rx1 (dense), tdoa, snr, table) of a fixture."""
    return g["group_ptr"], dense(g, g["rx0"]), dense(g, g["rx1"]), g["tdoa"], g["snr"], g["rx_xyz"]


def mode_of(g):
    return FREE_Z if bool(g["free_z"]) else KNOWN_HEIGHT


def options(g):
    """The keyword arguments of `posg3_ref.posg3_ref` and `_native.posg3` after the columns and the mode."""
    free_z = bool(g["free_z"])
    return dict(margin_m=float(g["margin_m"]), group_h=None if free_z else g["group_h"],
                x0=(0.1, 0.1, float(g["z0"]) if free_z else 0.0), z_range=None, z_grid=tuple(g["z_grid"].tolist()) if free_z else None,
                grid=int(g["grid"]), grid_z=int(g["grid_z"]), starts=int(g["starts"]), merge_m=float(g["merge_m"]),
                ratio=float(g["ratio"]), floor_m=float(g["floor_m"]))


def default_z_grid(table):
    """The Python interface's default: the antennas' heights grown by s = max(their spread, 10 m) on either side."""
    z = np.asarray(table, dtype=np.float64)[:, 2]
    s = max(float(z.max() - z.min()), 10.0)
    return float(z.min()) - s, float(z.max()) + s


def ring3(rng, n_rx, radius, z_lo, z_hi, offset=(0.0, 0.0)):
    """make_golden_pos3.py's ring: jittered positions, the stated height spread in no order around the ring."""
    ang = np.linspace(0, 2 * np.pi, n_rx, endpoint=False) + 0.3
    xy = np.c_[np.cos(ang), np.sin(ang)] * radius + rng.normal(0, radius * 0.05, (n_rx, 2)) + np.asarray(offset)
    return np.c_[xy, rng.permutation(np.linspace(z_lo, z_hi, n_rx))]


def ring_scene(seed, n_rx, radius, z_span, noise_s, n_groups, cut=(), needed=4, keep=0.8, table=None, tag_z=(0.0, 3.0), offset=(0.0, 0.0),
               all_pairs=False, rows=None):
    """-> dict(table, group_ptr, rx0, rx1 (dense), tdoa, snr, planted[g, 3]).  Every group keeps a random share `keep` of
    the receiver pairs that still names `needed` receivers (or every pair); the groups in `cut` name one receiver too
    few; `rows` (one number per group) takes that many rows from every pair in turn instead.  The noise is drawn per
    TDOA, in seconds."""
    rng = np.random.default_rng(seed)
    if table is None:
        table = ring3(rng, n_rx, radius, *z_span, offset=offset)
    table = np.asarray(table, dtype=np.float64)
    n_rx = len(table)
    every = list(itertools.combinations(range(n_rx), 2))
    ptr, rx0, rx1, tdoa, snr, planted = [0], [], [], [], [], []
    for g in range(n_groups):
        mobile = np.append(rng.uniform(-1, 1, 2) * radius * 0.6 + np.asarray(offset), rng.uniform(*tag_z))
        if rows is not None:
            pairs = [every[k % len(every)] for k in range(rows[g])]
        elif g in cut:
            few = sorted(rng.choice(n_rx, needed - 1, replace=False).tolist())
            pairs = list(itertools.combinations(few, 2))
        elif all_pairs:
            pairs = every
        else:
            while True:
                pairs = [pr for pr in every if rng.random() < keep]
                if len({i for pr in pairs for i in pr}) >= needed and len(pairs) >= needed:
                    break
        for i, j in pairs:
            true = (np.linalg.norm(table[i] - mobile) - np.linalg.norm(table[j] - mobile)) / C
            rx0.append(i), rx1.append(j), tdoa.append(true + rng.normal(0, noise_s)), snr.append(rng.uniform(5.0, 500.0))
        ptr.append(len(rx0))
        planted.append(mobile)
    return {"table": table, "group_ptr": np.array(ptr, dtype=np.int64), "rx0": np.array(rx0, dtype=np.int32),
            "rx1": np.array(rx1, dtype=np.int32), "tdoa": np.array(tdoa, dtype=np.float64),
            "snr": np.array(snr, dtype=np.float64), "planted": np.array(planted, dtype=np.float64).reshape(n_groups, 3)}


def volume_bound(rx0, rx1, tdoa, table, cx, cy, cz):
    """Per cell, `posg_golden.surface_bound`'s derived bound with three coordinates: 4 m 2^-53 sum_r (|tc_r| + da_r + db_r)^2
    on the difference of two float64 evaluations of F that add the rows in the same order."""
    table = np.asarray(table, dtype=np.float64)
    pz, py, px = np.meshgrid(np.asarray(cz, dtype=np.float64), cy, cx, indexing="ij")
    total = np.zeros(px.shape)
    for r0, r1, t in zip(np.asarray(rx0).tolist(), np.asarray(rx1).tolist(), np.asarray(tdoa, dtype=np.float64)):
        da = np.sqrt((table[r0, 0] - px) ** 2 + (table[r0, 1] - py) ** 2 + (table[r0, 2] - pz) ** 2)
        db = np.sqrt((table[r1, 0] - px) ** 2 + (table[r1, 1] - py) ** 2 + (table[r1, 2] - pz) ** 2)
        total += (abs(t * C) + da + db) ** 2
    return 4.0 * len(rx0) * 2.0 ** -53 * total


def assert_same_discrete_outputs(out, ref, safe=None):
    """`posg_golden.assert_same_discrete_outputs` with three coordinates: local-minimum cells (where `out` holds a map),
    start cells with their -1 slots, n_local, the tasks' statuses, n_minima and the flags; the chosen task must lie in the
    statement's chosen minimum.  Groups outside `safe` (two fits whose order is rounding noise) are compared without
    `task` and the MOVED flag."""
    n = len(ref["flags"])
    safe = np.ones(n, dtype=bool) if safe is None else np.asarray(safe, dtype=bool)
    for key in ("start_cell", "n_local", "task_status", "n_minima"):
        np.testing.assert_array_equal(out[key], ref[key], err_msg=key)
    np.testing.assert_array_equal(out["start_cell"] < 0, np.isnan(out["start_f"]))
    if "map_min" in out and len(out["map_min"]) == n:
        np.testing.assert_array_equal(out["map_min"], ref["map_min"])
        np.testing.assert_array_equal(out["map_min"].reshape(n, -1).sum(axis=1), out["n_local"])
    np.testing.assert_array_equal(out["flags"][safe], ref["flags"][safe])
    np.testing.assert_array_equal(out["flags"] & ~1, ref["flags"] & ~1)
    rows = np.flatnonzero(safe & ((ref["flags"] & 4) == 0))
    d = ref["task_pos"][rows, out["task"][rows]] - ref["pos"][rows]
    assert np.all(np.sqrt(np.sum(d * d, axis=1)) <= 1e-6), "the chosen task lies in another minimum than the statement's"
    np.testing.assert_array_equal(out["task"][(ref["flags"] & 4) != 0], 0)


# ---------------------------------------------------------------- checks the GPU tests share (they load the library)
def start_of(out_or_centres, cell, grid, free_z, x0):
    cx, cy, cz = out_or_centres
    if cell < 0:
        return x0
    return cx[cell % grid], cy[(cell // grid) % grid], cz[cell // (grid * grid)] if free_z else 0.0


def assert_tasks_equal_thr_pos3(out, group_ptr, rx0, rx1, tdoa, snr, table, mode, group_h=None, x0=(0.1, 0.1, 0.0), z_range=None,
                                max_iter=100):
    """Every task's pos, dop, hdop, vdop, rms, status and iters are byte for byte those of ONE thr_pos3 call per distinct
    start on the groups that have that start (grouped by task number, then by start cell); a task that does not exist
    holds the fill.  `out` holds cx, cy, cz.  -> the number of existing tasks."""
    from thrifty_amd import _native
    ptr = np.asarray(group_ptr, dtype=np.int64)
    free_z = mode == FREE_Z
    grid, T, n_tasks = len(out["cx"]), out["task_status"].shape[1], 0
    for t in range(T):
        cells = np.full(len(ptr) - 1, -2, dtype=np.int64) if t == 0 else out["start_cell"][:, t - 1].astype(np.int64)
        missing = cells == -1
        assert np.all(out["task_status"][missing, t] == _native.POSG3_NO_TASK) and np.all(out["task_iters"][missing, t] == 0)
        for key in ("task_pos", "task_rms", "task_dop", "task_hdop", "task_vdop"):
            assert np.all(np.isnan(out[key][missing, t])), key
        for cell in np.unique(cells[~missing]).tolist():
            groups = np.flatnonzero(cells == cell)
            rows = np.concatenate([np.arange(ptr[g], ptr[g + 1]) for g in groups])
            sub = np.concatenate([[0], np.cumsum(ptr[groups + 1] - ptr[groups])])
            start = start_of((out["cx"], out["cy"], out["cz"]), -1 if t == 0 else cell, grid, free_z, x0)
            want = _native.pos3(sub, rx0[rows], rx1[rows], tdoa[rows], snr[rows], table, mode,
                                None if free_z else np.asarray(group_h)[groups], start, z_range, max_iter)
            for key in ("pos", "dop", "hdop", "vdop", "rms", "status", "iters"):
                assert out["task_" + key][groups, t].tobytes() == want[key].tobytes(), (key, t, cell)
            if t == 0:
                assert out["snr"][groups].tobytes() == want["snr"].tobytes()
            n_tasks += len(groups)
    return n_tasks


def assert_choice_follows_the_rule(out, merge_m, ratio, floor_m, free_z):
    """task, pos, rms, dops, status, pos2, rms2, n_minima and flags against the rule in NumPy (posg3_ref.pick) on the
    device's OWN task outputs."""
    import posg3_ref
    want = posg3_ref.pick_groups(out["task_pos"], out["task_rms"], out["task_status"], merge_m, ratio, floor_m, free_z)
    for key in ("task", "n_minima", "flags"):
        np.testing.assert_array_equal(out[key], want[key], err_msg=key)
    for key in ("pos", "rms", "pos2", "rms2"):
        assert out[key].tobytes() == want[key].tobytes(), key
    rows = np.arange(len(out["task"]))
    for key in ("dop", "hdop", "vdop", "status"):
        assert out[key].tobytes() == out["task_" + key][rows, out["task"]].tobytes(), key

