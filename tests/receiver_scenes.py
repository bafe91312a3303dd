"""Scenes with high receiver numbers, and the checks the host and the GPU tests of the receiver seams share
(tests/test_receiver_seams_host.py, tests/test_gpu_receiver_seams.py).  Every stage after `thr_tdoa` keeps the
receivers a group names as a 64-bit mask, so the receiver number is what changes the code path: the scenes here name
receivers on both sides of bit 32 and up to bit 63 (1023 for `thr_tdoa`, whose limit is 1024).  Plain NumPy; nothing
here loads the library.

The checks take the device's outputs and a reference's (tests/pos_ref.py, pos3_ref.py, posq_ref.py, coverage_ref.py)
and raise AssertionError; the host test feeds them references doctored the way a 32-bit mask would leave them."""
import itertools

import numpy as np

import coverage_ref
import pos3_golden
import pos_golden
from pos_ref import OK, UNDERDETERMINED

C = 2.997e8
KNOWN_HEIGHT, FREE_Z = 0, 1

# ---------------------------------------------------------------- the table and the named sets
SETS = {
    "LOW3": (3, 17, 30),                    # bits of the low word only
    "HIGH3": (32, 45, 63),                  # bits of the high word only: lost with the high half
    "STRADDLE": (31, 32, 33),               # the last bit of the low word and the first two of the high one
    "SPLIT12": (5, 40, 50),                 # one low, two high: underdetermined if either half is lost
    "SPLIT21": (5, 9, 40),                  # two low, one high
    "HIGH2": (40, 50),                      # two receivers, one row: UNDERDETERMINED (OK only if one is counted twice)
    "TOP": tuple(range(54, 64)),
    "ACROSS": tuple(range(27, 37)),
    "ENDS": (0, 1, 31, 32, 62, 63),
    "ALL": tuple(range(64)),                # every pair: 2016 rows, all but 32 of them past the register rows
}
# with z free three receivers are underdetermined (tests/test_gpu_pos3_seams.py: resized): the 3-receiver sets get a
# fourth receiver of the half that holds most of theirs, so that losing either half still leaves fewer than four
SETS_FREE_Z = dict(SETS, LOW3=(3, 12, 17, 30), HIGH3=(32, 45, 54, 63), STRADDLE=(31, 32, 33, 34), SPLIT12=(5, 40, 50, 59),
                   SPLIT21=(5, 9, 22, 40))


def table65():
    """tests/test_gpu_pos3_seams.py: ring64 -- a ring of 65 receivers of 500 m with four heights in turn; the first 64
    are the table, the 65th is there for the refusals."""
    ang = np.linspace(0, 2 * np.pi, 65, endpoint=False)
    return np.c_[np.cos(ang) * 500.0, np.sin(ang) * 500.0, 5.0 + 60.0 * (np.arange(65) % 4)]


MOBILE = np.array([-180.0, 95.0, 1.5])     # the planted position; z is the known height
START3 = (0.1, 0.1, 4.0)                    # the free-z start of tests/test_gpu_pos3_seams.py's 64-receiver case


def pairs_of(receivers):
    """Every pair a < b of the receivers, a-major -> (rx0, rx1) int32."""
    rows = list(itertools.combinations(sorted(receivers), 2))
    return np.array([a for a, _ in rows], dtype=np.int32), np.array([b for _, b in rows], dtype=np.int32)


def planted_groups(sets, table, mobile=MOBILE):
    """One noise-free group per named set, every pair of the set as rows -> dict(names, sets, table, group_ptr, rx0,
    rx1, tdoa, snr).  `table` has two or three columns; the mobile's first columns are used."""
    table = np.asarray(table, dtype=np.float64)
    p = np.asarray(mobile, dtype=np.float64)[:table.shape[1]]
    dist = np.linalg.norm(table - p, axis=1)
    rx0, rx1 = zip(*[pairs_of(sets[name]) for name in sets])
    ptr = np.cumsum([0] + [len(a) for a in rx0])
    rx0, rx1 = np.concatenate(rx0), np.concatenate(rx1)
    return {"names": list(sets), "sets": dict(sets), "table": table, "group_ptr": ptr.astype(np.int64), "rx0": rx0, "rx1": rx1,
            "tdoa": (dist[rx0] - dist[rx1]) / C, "snr": 5.0 + (np.arange(len(rx0)) * 37 % 101).astype(np.float64)}


def tolerances(mode=None):
    """(position [m], dop relative) -- no tolerance of this file's own: ref_err_max and dop_ref_err_max of the fixture
    that tests/test_gpu_pos.py (pos_golden.check_positions) and tests/test_gpu_pos_seams.py hold thr_pos to against
    tests/pos_ref.py, the largest ring, pos_ring8; for thr_pos3 those of tests/test_gpu_pos3.py and
    tests/test_gpu_pos3_seams.py (MODES): h_ring6 with the height known, z_tall6 with z free."""
    g = pos_golden.load("pos_ring8") if mode is None else pos3_golden.load("h_ring6" if mode == KNOWN_HEIGHT else "z_tall6")
    return float(g["ref_err_max"]), float(g["dop_ref_err_max"])


_planted = {}


def planted_reference(mode):
    """(scene, the reference's columns) of the noise-free groups, one per named set -- computed once per mode (None:
    thr_pos on the flat table; KNOWN_HEIGHT / FREE_Z: thr_pos3).  Nobody changes them."""
    if mode not in _planted:
        from pos3_ref import pos3_ref_groups
        from pos_ref import pos_ref_groups
        table = table65()[:64]
        if mode is None:
            scene = planted_groups(SETS, table[:, :2])
            want = pos_ref_groups(scene["group_ptr"], scene["rx0"], scene["rx1"], scene["tdoa"], scene["snr"], scene["table"])
        else:
            scene = planted_groups(SETS_FREE_Z if mode == FREE_Z else SETS, table)
            scene["group_h"] = np.full(len(scene["names"]), MOBILE[2]) if mode == KNOWN_HEIGHT else None
            want = pos3_ref_groups(scene["group_ptr"], scene["rx0"], scene["rx1"], scene["tdoa"], scene["snr"], table, mode,
                                   scene["group_h"], START3)
        _planted[mode] = (scene, want)
    return _planted[mode]


def dop_keys(mode):
    return ("dop",) if mode is None else ("dop", "hdop") + (("vdop",) if mode == FREE_Z else ())


# ---------------------------------------------------------------- checks: thr_pos, thr_pos3
def assert_solves_equal(out, want, names, pos_tol, dop_rtol, dop_keys=("dop",)):
    """`out` (the device's columns) against `want` (pos_ref_groups / pos3_ref_groups on the same rows): the status
    exactly -- HIGH2 UNDERDETERMINED and every other named set OK --, the snr exactly (the references add in the
    device's order), position and dops of the solved groups within the tolerances."""
    np.testing.assert_array_equal(out["status"], want["status"])
    expected = [UNDERDETERMINED if name == "HIGH2" else OK for name in names]
    assert out["status"].tolist() == expected, dict(zip(names, out["status"].tolist()))
    solved = np.asarray(want["status"]) == OK
    err = np.max(np.abs(out["pos"][solved] - want["pos"][solved]), axis=1)
    print("max |x_dev - x_ref| = %.3g m (%s)" % (err.max(), names[int(np.flatnonzero(solved)[np.argmax(err)])]))
    assert np.all(err <= pos_tol), dict(zip(np.array(names)[solved], err))
    for key in dop_keys:
        np.testing.assert_allclose(out[key][solved], want[key][solved], rtol=dop_rtol, atol=0, err_msg=key)
    np.testing.assert_array_equal(out["snr"], want["snr"])


def low_half_statuses(scene, status, needed):
    """What a solver would answer that counted the receivers of the low word only: UNDERDETERMINED wherever fewer than
    `needed` receivers of the group are below 32."""
    ptr = scene["group_ptr"].tolist()
    out = np.array(status, dtype=np.int32)
    for g, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
        names = set(scene["rx0"][a:b].tolist()) | set(scene["rx1"][a:b].tolist())
        if len([r for r in names if r < 32]) < needed:
            out[g] = UNDERDETERMINED
    return out


def high_half_statuses(scene, status, needed):
    """The same for a solver that lost the low word."""
    ptr = scene["group_ptr"].tolist()
    out = np.array(status, dtype=np.int32)
    for g, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
        names = set(scene["rx0"][a:b].tolist()) | set(scene["rx1"][a:b].tolist())
        if len([r for r in names if r >= 32]) < needed:
            out[g] = UNDERDETERMINED
    return out


# ---------------------------------------------------------------- thr_posq, thr_posq3: one receiver late
def late_scene(receivers, late_rx, seed, table, n_groups=3, noise=0.01, delay=150.0, tag_z=1.5):
    """posq_golden.scene / posq3_golden.scene on a given table and receiver subset: `n_groups` mobiles inside the ring,
    arrivals with `noise` metres, the arrival at `late_rx` `delay` metres late in EVERY group, every pair of
    `receivers` as rows -> dict(table, group_ptr, rx0, rx1, tdoa, snr, planted, group_h, receivers)."""
    rng = np.random.default_rng(seed)
    table = np.asarray(table, dtype=np.float64)
    receivers = sorted(receivers)
    assert late_rx in receivers
    radius = float(np.max(np.linalg.norm(table[:, :2], axis=1)))
    r0, r1 = pairs_of(receivers)
    tdoa, snr = [], []
    for _ in range(n_groups):
        ang, rad = rng.uniform(0, 2 * np.pi), 0.6 * radius * np.sqrt(rng.uniform())
        mobile = np.array([np.cos(ang) * rad, np.sin(ang) * rad, tag_z])[:table.shape[1]]
        arrival = np.linalg.norm(table - mobile, axis=1) + rng.normal(0, noise, len(table))
        arrival[late_rx] += delay
        tdoa.append((arrival[r0] - arrival[r1]) / C)
        snr.append(rng.uniform(5.0, 500.0, len(r0)))
    return {"table": table, "group_ptr": (len(r0) * np.arange(n_groups + 1)).astype(np.int64), "rx0": np.tile(r0, n_groups),
            "rx1": np.tile(r1, n_groups), "tdoa": np.concatenate(tdoa), "snr": np.concatenate(snr),
            "planted": np.full(n_groups, late_rx, dtype=np.int32), "group_h": np.full(n_groups, float(tag_z)),
            "receivers": receivers}


LATE = (31, 32, 63)
GATE_M = 3.0        # tests/test_gpu_posq_seams.py's gate: far above the noise, far below what 150 m of delay leave


def late_case(name, late, seed, mode):
    """The late scene of a named set for thr_posq (mode None, the flat table) or thr_posq3."""
    table = table65()[:64]
    return late_scene(SETS[name], late, seed, table[:, :2] if mode is None else table)


def late_reference(scene, mode, weighted=False, **kw):
    """posq_ref / posq3_ref on a late scene with the gate GATE_M."""
    import posq3_ref
    import posq_ref
    cols = (scene["group_ptr"], scene["rx0"], scene["rx1"], scene["tdoa"], scene["snr"], scene["table"])
    weights = scene["snr"] if weighted else None
    if mode is None:
        return posq_ref.posq_ref(*cols, weights=weights, gate_m=GATE_M, **kw)
    return posq3_ref.posq3_ref(*cols, mode, scene["group_h"] if mode == KNOWN_HEIGHT else None, weights=weights, gate_m=GATE_M,
                               x0=START3, **kw)


# ENDS is three pairs of neighbours: without one receiver of a pair its neighbour still marks the site, and with z free
# a start far from the mobile then converges for few mobiles; these seeds' mobiles do (the host test holds every case
# to a margin: the planted candidate's rms is less than a third of any other's, by the references alone)
LATE_SEEDS = {("ENDS", 31): 104, ("ENDS", 32): 106}


def late_cases():
    """[(set name, late receiver, seed)]: 31, 32 and 63 in turn where the set holds it."""
    return [(name, late, LATE_SEEDS.get((name, late), 100)) for name in ("TOP", "ACROSS", "ENDS", "ALL") for late in LATE
            if late in SETS[name]]


def late_margin(out, scene):
    """The smallest ratio, over the groups, of any other candidate's rms to the planted receiver's candidate's; 0 where
    the planted receiver is not the one excluded."""
    n, worst = len(scene["receivers"]), np.inf
    for g, planted in enumerate(scene["planted"].tolist()):
        if int(out["counts"][g, 2]) != planted:
            return 0.0
        rx, rms = np.asarray(out["task_rx"][g * n:(g + 1) * n]), np.asarray(out["task_rms"][g * n:(g + 1) * n])
        worst = min(worst, float(rms[rx != planted].min() / rms[rx == planted][0]))
    return worst


def assert_candidate_list(out, scene):
    """The candidate list of a call in which every group is flagged: task_ptr steps by the size of the set, task_rx
    of every group is the sorted set; the planted receiver is the one excluded, and `used` is 0 exactly on the rows that
    name it.  (counts[:, 0] is the receiver count of the CHOSEN solve: the set without the excluded receiver.)"""
    receivers, n = scene["receivers"], len(scene["group_ptr"]) - 1
    np.testing.assert_array_equal(out["task_ptr"], len(receivers) * np.arange(n + 1))
    assert len(out["task_rx"]) == n * len(receivers)
    np.testing.assert_array_equal(np.asarray(out["task_rx"]).reshape(n, len(receivers)), np.tile(receivers, (n, 1)))
    np.testing.assert_array_equal(out["counts"][:, 2], scene["planted"])
    np.testing.assert_array_equal(out["counts"][:, 0], len(receivers) - 1)
    late = np.repeat(scene["planted"], np.diff(scene["group_ptr"]))
    np.testing.assert_array_equal(np.asarray(out["used"]).astype(bool), (scene["rx0"] != late) & (scene["rx1"] != late))


def without_high_candidates(out):
    """A reference's outputs as a 32-bit candidate list would leave them: no candidate of a receiver >= 32."""
    keep = np.asarray(out["task_rx"]) < 32
    groups = np.repeat(np.arange(len(out["task_ptr"]) - 1), np.diff(out["task_ptr"]))
    doctored = dict(out)
    doctored["task_ptr"] = np.concatenate([[0], np.cumsum(np.bincount(groups[keep], minlength=len(out["task_ptr"]) - 1))])
    for key in out:
        if key.startswith("task_") and key != "task_ptr":
            doctored[key] = np.asarray(out[key])[keep]
    return doctored


# ---------------------------------------------------------------- thr_coverage: three clusters
def cluster(centre, first, count, radius, turn=0.4):
    """`count` receivers on two rings around `centre` (never collinear for count >= 3)."""
    k = np.arange(count)
    ang = turn + 2 * np.pi * k / count + 0.37 * first
    rad = radius * np.where(k % 2 == 0, 1.0, 0.55)
    return np.asarray(centre, dtype=np.float64) + np.c_[np.cos(ang) * rad, np.sin(ang) * rad]


def coverage_table(n_rx=64):
    """Receivers 0..30 in the west, 31..33 in the middle, 34..63 in the east with 63 on the cluster's western edge (so
    that a cell between the middle and the east hears 31, 32, 33 and 63 and no other); 33 receivers: 0..30 and 31..32."""
    east = cluster((300.0, 0.0), 34, 30, 40.0)
    east[-1] = (195.0, 20.0)
    table = np.concatenate([cluster((-300.0, 0.0), 0, 31, 40.0), cluster((40.0, 10.0), 31, 3, 30.0), east])
    return table[:n_rx]


def coverage_scene(n_rx=64, range_m=130.0, trials=4):
    """The arguments of _native.coverage / coverage_ref: a 4 x 3 raster over the three clusters."""
    return dict(table=coverage_table(n_rx), sigma=0.05 + 0.01 * (np.arange(n_rx) % 7), lo=(-400.0, -150.0), hi=(400.0, 150.0), nx=4,
                ny=3, gross_m=5.0, trials=trials, range_m=range_m, seed=0x9E3779B97F4A7C15, x0=(0.1, 0.1))


def coverage_cells(a):
    """The cells of a coverage scene by coverage_ref alone (no trial is solved) -> dict(cx, cy, heard, n_heard,
    heard_mask, flags (UNCOVERED and DEGENERATE), pred, cond, receivers [per cell])."""
    cx, cy = coverage_ref.cell_centres(a["lo"], a["hi"], a["nx"], a["ny"])
    heard = coverage_ref.hearing(a["table"], cx, cy, a["range_m"])
    n = a["nx"] * a["ny"]
    out = {"cx": cx, "cy": cy, "heard": heard, "n_heard": heard.sum(axis=1).astype(np.int32), "heard_mask": coverage_ref.mask_of(heard),
           "flags": np.zeros(n, dtype=np.int32), "pred": np.full((n, 5), np.nan), "cond": np.full(n, np.nan),
           "receivers": [np.flatnonzero(row).tolist() for row in heard]}
    for c, receivers in enumerate(out["receivers"]):
        if len(receivers) < 3:
            out["flags"][c] = coverage_ref.UNCOVERED
            continue
        res = coverage_ref.analytic(a["table"], a["sigma"], (cx[c % a["nx"]], cy[c // a["nx"]]), receivers)
        out["pred"][c], out["cond"][c] = res[:5], res[5]
        if res[0] == -1:
            out["flags"][c] |= coverage_ref.DEGENERATE
    return out


def receivers_of_mask(mask):
    return [r for r in range(64) if (int(mask) >> r) & 1]


def assert_cells_and_rows(out, cells, trials):
    """n_heard, heard_mask and flags & 3 equal the statement's; the kept rows are coverage_ref.pairs of each covered
    cell's receivers, once per trial (tests/test_gpu_coverage.py: test_cells_hearing_and_rows_equal_the_statements)."""
    np.testing.assert_array_equal(out["n_heard"], cells["n_heard"])
    np.testing.assert_array_equal(np.asarray(out["heard_mask"], dtype=np.uint64), cells["heard_mask"])
    np.testing.assert_array_equal(np.asarray(out["flags"]) & 3, cells["flags"] & 3)
    want = [coverage_ref.pairs(receivers) for receivers in cells["receivers"] if len(receivers) >= 3 for _ in range(trials)]
    np.testing.assert_array_equal(out["keep_ptr"], np.cumsum([0] + [len(p[0]) for p in want]))
    np.testing.assert_array_equal(out["keep_rx0"], np.concatenate([p[0] for p in want]))
    np.testing.assert_array_equal(out["keep_rx1"], np.concatenate([p[1] for p in want]))


def low_word_cells(cells, trials):
    """The discrete outputs of a map whose hearing mask lost its high word, rows decoded from that mask: the `out` of
    assert_cells_and_rows."""
    mask = cells["heard_mask"] & np.uint64(0xFFFFFFFF)
    receivers = [receivers_of_mask(m) for m in mask]
    rows = [coverage_ref.pairs(rx) for rx in receivers if len(rx) >= 3 for _ in range(trials)]
    return {"n_heard": np.array([len(rx) for rx in receivers], dtype=np.int32), "heard_mask": mask,
            "flags": np.where(np.array([len(rx) for rx in receivers]) < 3, coverage_ref.UNCOVERED, cells["flags"] & 2),
            "keep_ptr": np.cumsum([0] + [len(p[0]) for p in rows]),
            "keep_rx0": np.concatenate([p[0] for p in rows]) if rows else np.zeros(0, dtype=np.int32),
            "keep_rx1": np.concatenate([p[1] for p in rows]) if rows else np.zeros(0, dtype=np.int32)}


def statement_rows(cells, trials):
    """The `out` of assert_cells_and_rows that the statement itself gives."""
    rows = [coverage_ref.pairs(rx) for rx in cells["receivers"] if len(rx) >= 3 for _ in range(trials)]
    return {"n_heard": cells["n_heard"], "heard_mask": cells["heard_mask"], "flags": cells["flags"],
            "keep_ptr": np.cumsum([0] + [len(p[0]) for p in rows]), "keep_rx0": np.concatenate([p[0] for p in rows]),
            "keep_rx1": np.concatenate([p[1] for p in rows])}


# ---------------------------------------------------------------- thr_tdoa: 1024 receivers
FS = 2.4e6
TDOA_RX = 1024
TDOA_RX_POS = {r: np.array([45.0 * (r % 32) - 700.0, 38.0 * (r // 32) - 600.0]) for r in range(TDOA_RX)}
TDOA_BEACON_POS = {0: np.array([300.0, 400.0]), 1: np.array([-200.0, 650.0])}      # tests/test_gpu_tdoa_seams.py
HEARD = [0, 1, 31, 32, 512, 513, 1022, 1023]


def clock_offset(r):
    """tests/test_gpu_tdoa_seams.py: OFFSET as a function of the receiver number (samples)."""
    return 3e9 + 2e6 * ((r * 7919) % 4099)


def clock_ppm(r):
    """tests/test_gpu_tdoa_seams.py: PPM as a function of the receiver number: slow drifts within +-0.25e-6."""
    return 0.025e-6 * ((r * 37) % 21 - 10)


class TdoaScene(object):
    """tests/test_gpu_tdoa_seams.py: Scene with the per-receiver offset and drift as functions of r."""

    def __init__(self, seed=1):
        self.rng = np.random.default_rng(seed)
        self.rows, self.matches = [], []

    def send(self, tx, t, receivers):
        match = []
        for r in receivers:
            soa = clock_offset(r) + FS * (1 + clock_ppm(r)) * t + 2e-3 * (r % 5 + 1) * t * t + float(self.rng.normal(0, 0.05))
            match.append(len(self.rows))
            self.rows.append((r, tx, 1000.0 + t, soa, float(self.rng.uniform(50, 200)), float(self.rng.uniform(1, 3))))
        self.matches.append(match)

    def cols(self):
        names = ("rxid", "txid", "timestamp", "soa", "energy", "noise")
        return {name: np.array([row[k] for row in self.rows], dtype=(np.int64 if k < 2 else np.float64))
                for k, name in enumerate(names)}


def tdoa_scene():
    """40 beacon transmissions (tests/test_gpu_tdoa_seams.py: test_match_sizes_and_task_counts) heard by HEARD, then four
    mobile matches: the whole list (28 tasks), the list in descending order, [1023, 0] and [1022, 1023]."""
    scene = TdoaScene(1024)
    for k in range(40):
        scene.send(k % 2, -10.0 + 0.5 * k, HEARD)
    scene.send(5, -3.0, HEARD)
    scene.send(6, -2.3, HEARD[::-1])
    scene.send(5, -1.6, [1023, 0])
    scene.send(6, -0.9, [1022, 1023])
    return scene


def tdoa_native_args(scene, n_rx=TDOA_RX, window=8.0):
    """The arguments of _native.tdoa for a table of n_rx receivers whose dense index is the receiver number."""
    cols = scene.cols()
    beacons = sorted(TDOA_BEACON_POS)
    first_tx = [int(cols["txid"][m[0]]) for m in scene.matches]
    match_beacon = np.array([beacons.index(tx) if tx in beacons else -1 for tx in first_tx], dtype=np.int32)
    rx_pos = [TDOA_RX_POS[r] if r < TDOA_RX else np.array([900.0, 900.0]) for r in range(n_rx)]
    dist = np.array([[np.sqrt(np.sum((np.asarray(p, dtype=float) - np.asarray(TDOA_BEACON_POS[b], dtype=float)) ** 2)) for b in beacons]
                     for p in rx_pos])
    ptr = np.cumsum([0] + [len(m) for m in scene.matches])
    idx = np.array([i for m in scene.matches for i in m], dtype=np.int64)
    return (cols["rxid"].astype(np.int32), cols["timestamp"], cols["soa"], cols["energy"], cols["noise"], ptr, idx, match_beacon, dist,
            window, FS)


# ---------------------------------------------------------------- thr_postdetect: a full table
POST_IDS = tuple(3 * k + 2 for k in range(65))       # ascending, not dense; the 65th is there for the refusal
POST_HEARING = tuple(POST_IDS[k] for k in (0, 31, 32, 63))


def post_rx_pos(settings, n_rx=64):
    """The receiver table of postdetect_scene's settings (made for rx_ids=POST_HEARING) grown to n_rx entries: the scene's
    four receivers land on the dense indices 0, 31, 32 and 63; the others, on a ring of 1.6 km, are never heard."""
    rx_pos = {}
    for k, rx in enumerate(POST_IDS[:n_rx]):
        ang = 0.2 + 2 * np.pi * k / 65
        rx_pos[rx] = np.asarray(settings.rx_pos[rx]) if rx in settings.rx_pos else np.array([np.cos(ang), np.sin(ang)]) * 1600.0
    return rx_pos
