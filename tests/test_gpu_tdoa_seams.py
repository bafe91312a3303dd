"""`thr_tdoa` at the seams of its kernels.  Every expectation is tests/tdoa_ref.py's (itself held to the
reference's fixtures by tests/test_tdoa_host.py): groups, rows, failures, n_window and n_kept exact.

Tolerance of `tdoa` against tdoa_ref: both fit the same centred and scaled problem.  The device sums
each moment as at most a few terms per lane and a six-level tree (about 10 roundings, relative to sums
of terms of one sign or of size <= spread = max |y - mean y|), and solves the Gram system, whose
condition is cond(V)^2, with partial pivoting: coefficients, and with them the fitted value at |u| <= 1,
off by about 10 eps cond(V)^2 spread; tdoa_ref's SVD adds cond(V) eps, the final subtractions a few eps
spread.  Bound: 16 * cond(V)^2 * 2^-52 * spread / sample_rate, cond(V) and spread per pair from tdoa_ref
-- 3e-13 to 4e-13 s for a 16 s parabola, against TDOAs of 1e-6 s.  snr relative
1e-14, model_quality relative 1e-12 (summation order)."""
import numpy as np
import pytest

from tdoa_ref import tdoa_ref
from thrifty_amd import _native, tdoa_est

pytestmark = pytest.mark.gpu

FS = 2.4e6
WAVES = _native.TDOA_TASKS_PER_WORKGROUP
LDS = _native.TDOA_LDS_WINDOW
RX_POS = {r: np.array(p) for r, p in enumerate([(0.0, 0.0), (900.0, 0.0), (0.0, 700.0), (800.0, 900.0), (-500.0, 300.0)])}
BEACON_POS = {0: np.array([300.0, 400.0]), 1: np.array([-200.0, 650.0])}
OFFSET = [3e9, 7e9, 1.1e10, 5e9, 9e9]
PPM = [0.0, 0.2e-6, -0.12e-6, 0.07e-6, -0.25e-6]       # slow drifts: a gross SoA error stands out of a window


class Scene(object):
    """Detections appended one transmission at a time; a match per transmission."""

    def __init__(self, seed=1):
        self.rng = np.random.default_rng(seed)
        self.rows, self.matches = [], []

    def send(self, tx, t, receivers, soa_error=0.0, stamp=None):
        match = []
        for r in receivers:
            soa = OFFSET[r] + FS * (1 + PPM[r]) * t + 2e-3 * (r + 1) * t * t + float(self.rng.normal(0, 0.05))
            match.append(len(self.rows))
            self.rows.append((r, tx, 1000.0 + (t if stamp is None else stamp), soa + (soa_error if r == receivers[-1] else 0.0),
                              float(self.rng.uniform(50, 200)), float(self.rng.uniform(1, 3))))
        self.matches.append(match)

    def cols(self):
        names = ("rxid", "txid", "timestamp", "soa", "energy", "noise")
        return {name: np.array([row[k] for row in self.rows], dtype=(np.int64 if k < 2 else np.float64))
                for k, name in enumerate(names)}


def check(scene, window=8.0, deg=2, beacon_pos=BEACON_POS):
    """Device == sequential statement; -> tdoa_ref's dict."""
    cols = scene.cols()
    want = tdoa_ref(cols["rxid"], cols["txid"], cols["timestamp"], cols["soa"], cols["energy"], cols["noise"],
                    scene.matches, window, beacon_pos, RX_POS, FS, deg)
    ptr = np.cumsum([0] + [len(m) for m in scene.matches])
    idx = np.array([i for m in scene.matches for i in m], dtype=np.int64)
    got = tdoa_est.tdoa_columns(cols, ptr, idx, window, beacon_pos, RX_POS, FS, deg)
    assert got["n_window"].tolist() == want["n_window"]
    assert got["n_kept"].tolist() == want["n_kept"]
    assert [tuple(p) for p in got["failures"].tolist()] == want["failures"]
    assert got["group_id"].tolist() == [g[0] for g in want["groups"]]
    assert got["timestamp"].tolist() == [g[1] for g in want["groups"]]
    assert got["tx"].tolist() == [g[2] for g in want["groups"]]
    assert got["group_ptr"].tolist() == np.cumsum([0] + [len(g[3]) for g in want["groups"]]).tolist()
    rows = [row for g in want["groups"] for row in g[3]]
    ours = got["tdoas"]
    for k, key in ((0, "rx0"), (1, "rx1"), (5, "det0_idx"), (6, "det1_idx")):
        assert ours[key].tolist() == [row[k] for row in rows], key
    # the pairs that produced a row, in order: their cond and spread bound the tdoa difference
    failed = set(want["failures"])
    tasks = [(d0, d1) if cols["rxid"][d0] < cols["rxid"][d1] else (d1, d0)
             for m in scene.matches if cols["txid"][m[0]] not in beacon_pos
             for i, d0 in enumerate(m) for d1 in m[i + 1:]]
    bound = [16 * c * c * 2.0 ** -52 * s / FS for t, c, s in zip(tasks, want["cond"], want["spread"]) if t not in failed]
    assert len(bound) == len(rows)
    diff = np.abs(ours["tdoa"] - np.array([row[2] for row in rows], dtype=float))
    print("max |tdoa - tdoa_ref| = %.3g s, bound %.3g s" % (diff.max() if len(diff) else 0, min(bound) if bound else 0))
    assert np.all(diff <= np.array(bound, dtype=float))
    np.testing.assert_allclose(ours["snr"], [row[3] for row in rows], rtol=1e-14, atol=0)
    np.testing.assert_allclose(ours["model_quality"], [row[4] for row in rows], rtol=1e-12, atol=0)
    return want


def windowed(length, seed=1, receivers=(0, 1), outlier_every=17):
    """`length` beacon transmissions inside [-8, 8] (the first and the last ON the edges), three on
    either side outside, every 17th with a gross SoA error, then one mobile transmission at 0."""
    scene = Scene(seed)
    inside = np.linspace(-8.0, 8.0, length).tolist() if length > 1 else [-8.0] * length
    for k, t in enumerate([-20.0, -15.0, -8.5] + inside + [8.5, 12.0, 30.0]):
        scene.send(k % 2, t, receivers, soa_error=40.0 if k % outlier_every == 5 else 0.0)
    scene.send(7, 0.0, receivers)
    return scene


@pytest.mark.parametrize("length", [0, 1, 2, 3, 4, 63, 64, 65, 128, 129, LDS - 1, LDS, LDS + 1, 2 * LDS + 3])
def test_window_lengths(length):
    want = check(windowed(length))
    assert want["n_window"] == [length]
    assert len(want["failures"]) == (1 if want["n_kept"][0] < 3 else 0) and (length >= 3 or want["failures"])
    if length >= 63:
        assert want["n_kept"][0] < length                           # gross errors were masked


@pytest.mark.parametrize("deg", [1, 3])
def test_other_degrees(deg):
    for length in (deg, deg + 1, 40, 70):
        want = check(windowed(length, seed=deg, outlier_every=1000), deg=deg)
        assert len(want["failures"]) == (1 if want["n_kept"][0] <= deg else 0) and (length > deg or want["failures"])
        assert length < 40 or want["failures"] == []


@pytest.mark.parametrize("sizes", [(2,), (3,), (5,), (2, 2, 2, 2, 2), (5, 3, 2, 5, 3), (2,) * (2 * WAVES + 1)])
def test_match_sizes_and_task_counts(sizes):
    """1, 3 and 10 pairs per match; task lists that are not a multiple of the wavefronts per workgroup."""
    scene = Scene(len(sizes))
    for k in range(40):
        scene.send(k % 2, -10.0 + 0.5 * k, [0, 1, 2, 3, 4])
    order = [4, 1, 3, 0, 2]                      # matches list their receivers in any order
    for k, size in enumerate(sizes):
        scene.send(5 + k % 2, -3.0 + 0.7 * k, order[k % 3:][:size] if size < 5 else order)
    want = check(scene)
    n_tasks = sum(s * (s - 1) // 2 for s in sizes)
    assert len(want["n_window"]) == n_tasks and want["failures"] == []
    assert len(want["groups"]) == len(sizes)
    if len(sizes) > 1:
        assert n_tasks % WAVES != 0


def test_no_beacon_match_and_no_mobile_match():
    scene = Scene()
    for k in range(5):
        scene.send(7, float(k), [0, 1, 2])
    want = check(scene)                          # every list is missing: empty windows, failures
    assert want["groups"] == [] and len(want["failures"]) == 15 and set(want["n_window"]) == {0}
    scene = Scene()
    for k in range(5):
        scene.send(0, float(k), [0, 1, 2])
    want = check(scene)
    assert want["groups"] == [] and want["failures"] == [] and want["n_window"] == []
    empty = Scene()
    got = tdoa_est.tdoa_columns(empty.cols(), [0], [], 8.0, BEACON_POS, RX_POS, FS)
    assert len(got["tdoas"]) == 0 and len(got["group_id"]) == 0 and got["group_ptr"].tolist() == [0]
    assert tdoa_est.estimate_tdoas([], [], 8.0, BEACON_POS, RX_POS, FS) == ([], [])


def test_one_receiver_pair_holds_every_beacon_pair():
    """The other receiver pairs have no list (the reference: KeyError; here: failures)."""
    scene = Scene(4)
    for k in range(30):
        scene.send(k % 2, -7.0 + 0.5 * k, [0, 1])
    scene.send(7, 0.0, [2, 0, 1])
    scene.send(7, 1.0, [1, 2])
    want = check(scene)
    assert [g[0] for g in want["groups"]] == [30] and [row[:2] for row in want["groups"][0][3]] == [(0, 1)]
    assert want["n_window"] == [0, 0, 30, 0] and len(want["failures"]) == 3


def test_unsorted_lists_give_what_pythons_bisection_gives():
    rng = np.random.default_rng(8)
    for trial in range(4):
        scene = Scene(trial)
        stamps = rng.permutation(np.arange(-12.0, 12.0, 0.5)) if trial else np.arange(12.0, -12.0, -0.5)
        for k, t in enumerate(np.sort(stamps)):
            scene.send(k % 2, float(t), [0, 1], stamp=float(stamps[k]))
        for t in (-6.0, 0.0, 5.5):
            scene.send(7, t, [1, 0])
        want = check(scene)
        assert len(set(want["n_window"])) > 1 or trial == 0


def test_ties_and_a_zero_mad():
    """SoA differences on a grid: medians of equal values, mad == 0 (0 / 0 is kept, x / 0 is dropped)."""
    for length in (5, 6, 64, 65):
        scene = Scene(length)
        step = np.array([0, 0, 0, 1, 0, 0, -2, 0])
        for k, t in enumerate(np.linspace(-8.0, 8.0, length)):
            scene.send(0, float(t), [0, 1])
        scene.send(7, 0.0, [0, 1])
        for i, row in enumerate(scene.rows):           # receiver 0: 1000 t exactly, receiver 1: 1000 t + 5e9 + a step
            t = row[2] - 1000.0
            soa = np.round(1000.0 * t) + (5e9 + step[(i // 2) % 8] if row[0] == 1 else 0.0)
            scene.rows[i] = row[:3] + (float(soa),) + row[4:]
        want = check(scene)
        assert want["n_window"] == [length] and 3 <= want["n_kept"][0] < length
    # mad == 0 and every diff == 0: all kept
    scene = Scene(2)
    for k in range(6):
        scene.send(0, float(k), [0, 1])
    scene.send(7, 2.5, [0, 1])
    scene.rows = [row[:3] + (float(np.round(800.0 * (row[2] - 1000.0)) + (4e9 if row[0] else 0.0)),) + row[4:]
                  for row in scene.rows]
    assert check(scene)["n_kept"] == [6]


def test_repeated_abscissae_and_too_large_tdoas_are_failures():
    scene = Scene(6)
    for k in range(8):
        scene.send(0, float(k), [0, 1])
    scene.send(7, 3.0, [0, 1])
    first = {0: scene.rows[0][3], 1: scene.rows[1][3]}
    for i in range(4, 16):                      # pairs 2..7 repeat pair 0's SoAs: two distinct abscissae in all
        scene.rows[i] = scene.rows[i][:3] + (first[scene.rows[i][0]] + (0.01 * i if scene.rows[i][0] == 0 else 0.0),) + scene.rows[i][4:]
    want = check(scene)
    assert want["n_kept"][0] >= 3 and want["failures"] == [(16, 17)]
    check(scene, deg=1)                         # two distinct abscissae carry a line (wherever it leads)
    scene = Scene(7)
    for k in range(20):
        scene.send(k % 2, -5.0 + 0.5 * k, [0, 1])
    scene.send(7, 0.0, [0, 1], soa_error=600.0)
    scene.send(7, 1.0, [0, 1])
    want = check(scene)
    assert want["failures"] == [(40, 41)] and [g[0] for g in want["groups"]] == [21]
