"""The posg fixtures (tests/golden/posg/*.npz, made by tests/golden/make_golden_posg.py) and the scenes the host and
GPU tests of `thr_posg` share: a jittered ring of receivers of radius 100 m, every receiver pair, Gaussian noise on
each arrival, the tag inside the ring or outside it, the array at the origin or far from it."""
import itertools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "posg")
SETS = ("far4", "far8", "three_out", "clean6")
C = 2.997e8
RADIUS = 100.0
OFFSET = (5000.0, -3000.0)
# name -> (seed, receivers, groups, noise [m], tag outside the ring, array offset, floor_m)
SCENES = {"far4": (0, 4, 32, 0.3, False, OFFSET, 0.0), "far8": (9, 8, 32, 3.0, False, OFFSET, 0.0),
          "three_out": (1, 3, 40, 0.3, True, (0.0, 0.0), 1.0), "clean6": (0, 6, 24, 0.3, False, (0.0, 0.0), 0.0)}
OPTIONS = dict(grid=32, starts=4, merge_m=1.0, ratio=2.0)
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
    return {int(r): np.array(xy) for r, xy in zip(g["rx_ids"], g["rx_xy"])}


def dense(g, column):
    index = {int(r): k for k, r in enumerate(g["rx_ids"])}
    return np.array([index[int(v)] for v in column], dtype=np.int32)


def columns(g):
    """(group_ptr, rx0, rx1 (dense), tdoa, snr, table) of a fixture."""
    return g["group_ptr"], dense(g, g["rx0"]), dense(g, g["rx1"]), g["tdoa"], g["snr"], g["rx_xy"]


def options(g):
    return dict(margin_m=float(g["margin_m"]), grid=int(g["grid"]), starts=int(g["starts"]), merge_m=float(g["merge_m"]),
                ratio=float(g["ratio"]), floor_m=float(g["floor_m"]))


def ring(rng, n_rx, radius=RADIUS, offset=(0.0, 0.0)):
    ang = np.linspace(0, 2 * np.pi, n_rx, endpoint=False) + 0.3
    return np.c_[np.cos(ang), np.sin(ang)] * radius + rng.normal(0, radius * 0.05, (n_rx, 2)) + np.asarray(offset)


def margin_of(table):
    """The Python interface's default: the longer side of the receivers' bounding box."""
    table = np.asarray(table, dtype=np.float64)
    return float(np.max(table.max(axis=0) - table.min(axis=0)))


def scene(seed, n_rx, n_groups, noise, outside=False, offset=(0.0, 0.0), pairs=None, rows=None):
    """-> dict(table, group_ptr, rx0, rx1 (dense), tdoa, snr, planted[g, 2]).  The tag lies inside 0.6 of the ring, or
    (`outside`) between 1.2 and 3 radii from its centre; rows: every receiver pair (or `pairs`), or `rows` rows drawn
    from them in turn (one number, or one per group)."""
    rng = np.random.default_rng(seed)
    table = ring(rng, n_rx, offset=offset)
    every_pair = list(itertools.combinations(range(n_rx), 2)) if pairs is None else list(pairs)
    ptr, rx0, rx1, tdoa, snr, planted = [0], [], [], [], [], []
    for g in range(n_groups):
        ang = rng.uniform(0, 2 * np.pi)
        rad = RADIUS * rng.uniform(1.2, 3.0) if outside else 0.6 * RADIUS * np.sqrt(rng.uniform())
        tag = np.array([np.cos(ang), np.sin(ang)]) * rad + np.asarray(offset)
        arrival = np.linalg.norm(table - tag, axis=1) + rng.normal(0, noise, n_rx)
        n_rows = rows if rows is None or np.isscalar(rows) else rows[g]
        chosen = every_pair if n_rows is None else [every_pair[k % len(every_pair)] for k in range(n_rows)]
        for i, j in chosen:
            rx0.append(i), rx1.append(j), tdoa.append((arrival[i] - arrival[j]) / C), snr.append(rng.uniform(5.0, 500.0))
        ptr.append(len(rx0))
        planted.append(tag)
    return {"table": table, "group_ptr": np.array(ptr, dtype=np.int64), "rx0": np.array(rx0, dtype=np.int32),
            "rx1": np.array(rx1, dtype=np.int32), "tdoa": np.array(tdoa, dtype=np.float64),
            "snr": np.array(snr, dtype=np.float64), "planted": np.array(planted, dtype=np.float64).reshape(n_groups, 2)}


def surface_bound(rx0, rx1, tdoa, table, cx, cy):
    """Per cell, the derived bound on the difference of two float64 evaluations of F that add the rows in the same
    order: 4 m 2^-53 sum_r (|tc_r| + da_r + db_r)^2.  Each residual is three roundings of quantities bounded by
    |tc| + da + db (relative 2^-53 each, the sqrt's and the differences' included in the factor), its square doubles
    the relative error, and m additions of non-negative terms add m 2^-53 of the sum."""
    table = np.asarray(table, dtype=np.float64)
    px, py = np.meshgrid(cx, cy)
    total = np.zeros(px.shape)
    for r0, r1, t in zip(np.asarray(rx0).tolist(), np.asarray(rx1).tolist(), np.asarray(tdoa, dtype=np.float64)):
        da = np.sqrt((table[r0, 0] - px) ** 2 + (table[r0, 1] - py) ** 2)
        db = np.sqrt((table[r1, 0] - px) ** 2 + (table[r1, 1] - py) ** 2)
        total += (abs(t * C) + da + db) ** 2
    return 4.0 * len(rx0) * 2.0 ** -53 * total


def assert_same_discrete_outputs(out, ref, safe=None):
    """The device's (or another build's) discrete outputs against the statement's: local-minimum cells (where `out`
    holds a map), start cells with their -1 slots, n_local, the tasks' statuses, n_minima and the flags; the chosen task
    must lie in the statement's chosen minimum (two tasks that end in ONE minimum have the same rms up to rounding, so
    the task NUMBER is not comparable).  Groups outside `safe` (two exact fits, tests/golden/make_golden_posg.py) are
    compared without `task` and the MOVED flag."""
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
    assert np.all(np.hypot(d[:, 0], d[:, 1]) <= 1e-6), "the chosen task lies in another minimum than the statement's"
    np.testing.assert_array_equal(out["task"][(ref["flags"] & 4) != 0], 0)


# ---------------------------------------------------------------- checks the GPU tests share (they load the library)
def assert_tasks_equal_thr_pos(out, group_ptr, rx0, rx1, tdoa, snr, table, cx, cy, x0=(0.1, 0.1), max_iter=100):
    """Every task's pos, dop, status and iters are byte for byte those of ONE thr_pos call per distinct start on the
    groups that have that start (grouped by task number, then by start cell); a task that does not exist holds the
    fill.  -> the number of existing tasks."""
    from thrifty_amd import _native
    ptr = np.asarray(group_ptr, dtype=np.int64)
    grid, T, n_tasks = len(cx), out["task_status"].shape[1], 0
    for t in range(T):
        cells = np.zeros(len(ptr) - 1, dtype=np.int64) if t == 0 else out["start_cell"][:, t - 1].astype(np.int64)
        missing = cells < 0
        assert np.all(out["task_status"][missing, t] == _native.POSG_NO_TASK) and np.all(out["task_iters"][missing, t] == 0)
        assert np.all(np.isnan(out["task_pos"][missing, t])) and np.all(np.isnan(out["task_rms"][missing, t]))
        assert np.all(np.isnan(out["task_dop"][missing, t]))
        for cell in np.unique(cells[~missing]).tolist():
            groups = np.flatnonzero(cells == cell)
            rows = np.concatenate([np.arange(ptr[g], ptr[g + 1]) for g in groups])
            sub = np.concatenate([[0], np.cumsum(ptr[groups + 1] - ptr[groups])])
            start = x0 if t == 0 else (cx[cell % grid], cy[cell // grid])
            want = _native.pos(sub, rx0[rows], rx1[rows], tdoa[rows], snr[rows], table, x0=start, max_iter=max_iter)
            assert out["task_pos"][groups, t].tobytes() == want["pos"].tobytes(), (t, cell)
            assert out["task_dop"][groups, t].tobytes() == want["dop"].tobytes(), (t, cell)
            assert out["task_status"][groups, t].tobytes() == want["status"].tobytes(), (t, cell)
            assert out["task_iters"][groups, t].tobytes() == want["iters"].tobytes(), (t, cell)
            if t == 0:
                assert out["snr"][groups].tobytes() == want["snr"].tobytes()
            n_tasks += len(groups)
    return n_tasks


def assert_choice_follows_the_rule(out, merge_m, ratio, floor_m):
    """task, pos, rms, dop, status, pos2, rms2, n_minima and flags against the rule in NumPy (posg_ref.pick) on the
    device's OWN task outputs."""
    import posg_ref
    want = posg_ref.pick_groups(out["task_pos"], out["task_rms"], out["task_status"], merge_m, ratio, floor_m)
    for key in ("task", "n_minima", "flags"):
        np.testing.assert_array_equal(out[key], want[key], err_msg=key)
    for key in ("pos", "rms", "pos2", "rms2"):
        assert out[key].tobytes() == want[key].tobytes(), key
    rows = np.arange(len(out["task"]))
    assert out["dop"].tobytes() == out["task_dop"][rows, out["task"]].tobytes()
    assert out["status"].tobytes() == out["task_status"][rows, out["task"]].tobytes()
