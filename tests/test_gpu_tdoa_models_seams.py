"""`thr_tdoa_model` at the seams of the three added models.  Every expectation is tests/tdoa_models_ref.py's
(itself held to the reference's fixtures by tests/test_tdoa_models_host.py): groups, rows, failures,
n_window, n_kept and the picks -- positions in the KEPT list -- exact; `tdoa` of nearest and linear equal
to the statement's bits.

Tolerance of the weighted `tdoa` against the statement: the bound tests/test_gpu_tdoa_seams.py derives for
the plain fit, 16 * cond(V)^2 * 2^-52 * spread / sample_rate, with V the WEIGHTED scaled Vandermonde
diag(w) V(u): the weights lie in [2/3, 1] and are the same float64 numbers on both sides, so they change
the Gram system's entries and its condition, not the count of roundings.  snr relative 1e-14,
model_quality relative 1e-12 (summation order)."""
import numpy as np
import pytest

from tdoa_models_ref import tdoa_models_ref
from test_gpu_tdoa_seams import BEACON_POS, FS, LDS, RX_POS, WAVES, Scene, windowed
from thrifty_amd import tdoa_est

pytestmark = pytest.mark.gpu

MODELS = ("weighted_poly", "nearest", "linear")
MINIMUM = {"weighted_poly": 3, "nearest": 1, "linear": 2}     # kept pairs a model needs (deg 2)


def check(scene, model, window=8.0, deg=2):
    """Device == sequential statement; -> the statement's dict."""
    cols = scene.cols()
    want = tdoa_models_ref(cols["rxid"], cols["txid"], cols["timestamp"], cols["soa"], cols["energy"], cols["noise"],
                           scene.matches, window, BEACON_POS, RX_POS, FS, model, deg)
    ptr = np.cumsum([0] + [len(m) for m in scene.matches])
    idx = np.array([i for m in scene.matches for i in m], dtype=np.int64)
    got = tdoa_est.tdoa_columns(cols, ptr, idx, window, BEACON_POS, RX_POS, FS, deg, model=model)
    assert got["n_window"].tolist() == want["n_window"]
    assert got["n_kept"].tolist() == want["n_kept"]
    assert [tuple(p) for p in got["picks"].tolist()] == want["picks"]
    assert [tuple(p) for p in got["failures"].tolist()] == want["failures"]
    assert got["group_id"].tolist() == [g[0] for g in want["groups"]]
    assert got["timestamp"].tolist() == [g[1] for g in want["groups"]]
    assert got["tx"].tolist() == [g[2] for g in want["groups"]]
    assert got["group_ptr"].tolist() == np.cumsum([0] + [len(g[3]) for g in want["groups"]]).tolist()
    rows = [row for g in want["groups"] for row in g[3]]
    ours = got["tdoas"]
    for k, key in ((0, "rx0"), (1, "rx1"), (5, "det0_idx"), (6, "det1_idx")):
        assert ours[key].tolist() == [row[k] for row in rows], key
    theirs = np.array([row[2] for row in rows], dtype=np.float64)
    mine = np.ascontiguousarray(ours["tdoa"], dtype=np.float64)
    if model == "weighted_poly":
        failed = set(want["failures"])
        tasks = [(d0, d1) if cols["rxid"][d0] < cols["rxid"][d1] else (d1, d0)
                 for m in scene.matches if cols["txid"][m[0]] not in BEACON_POS
                 for i, d0 in enumerate(m) for d1 in m[i + 1:]]
        bound = [16 * c * c * 2.0 ** -52 * s / FS for t, c, s in zip(tasks, want["cond"], want["spread"]) if t not in failed]
        assert len(bound) == len(rows)
        diff = np.abs(mine - theirs)
        print("max |tdoa - statement| = %.3g s, bound %.3g s" % (diff.max() if len(diff) else 0, min(bound) if bound else 0))
        assert np.all(diff <= np.array(bound, dtype=float))
    else:
        assert mine.tobytes() == theirs.tobytes(), np.flatnonzero(mine != theirs)[:5]
    np.testing.assert_allclose(ours["snr"], [row[3] for row in rows], rtol=1e-14, atol=0)
    np.testing.assert_allclose(ours["model_quality"], [row[4] for row in rows], rtol=1e-12, atol=0)
    return want


def line(times, mobiles, beacons=None, errors=(), seed=3, receivers=(0, 1), mobile_error=0.0):
    """Beacon transmissions at `times` (beacon 0, or beacons[k]), those listed in `errors` with a gross SoA
    error (the mask drops them), then mobile transmissions at `mobiles`."""
    scene = Scene(seed)
    for k, t in enumerate(times):
        scene.send(0 if beacons is None else beacons[k], float(t), list(receivers), soa_error=40.0 if k in errors else 0.0)
    for t in mobiles:
        scene.send(7, float(t), list(receivers), soa_error=mobile_error)
    return scene


@pytest.mark.parametrize("model", MODELS)
def test_kept_pairs_around_each_models_minimum(model):
    kept = set()
    for length in (0, 1, 2, 3, 4, 5):
        want = check(windowed(length, seed=length + 1, outlier_every=1000), model)
        assert want["n_window"] == [length]
        assert (want["n_kept"][0] < MINIMUM[model]) <= (len(want["failures"]) == 1)
        kept.add(want["n_kept"][0])
    assert {0, 1, 2, 3} <= kept
    # one beacon only: the linear model finds its earlier pair whenever two are kept
    for length in (1, 2, 3):
        want = check(line(np.linspace(-2.0, 2.0, length), [0.5]), model)
        assert want["n_kept"] == [length] and (len(want["failures"]) == 1) == (length < MINIMUM[model])
    check(windowed(4, seed=9, outlier_every=1000), "weighted_poly", deg=3)
    check(windowed(3, seed=9, outlier_every=1000), "weighted_poly", deg=3)
    check(windowed(2, seed=9, outlier_every=1000), "weighted_poly", deg=1)
    check(windowed(40, seed=9), "weighted_poly", deg=1)
    check(windowed(70, seed=9), "weighted_poly", deg=3)


def test_ties_of_the_bisection_and_of_the_distances():
    on_a_beacon = line([-2.0, -1.0, 0.0, 1.0, 2.0], [0.0])                  # t0 equals a kept timestamp: bisect_left stops ON it
    assert check(on_a_beacon, "nearest")["picks"] == [(2, -1)]
    assert check(on_a_beacon, "linear")["picks"] == [(1, 2)]
    halfway = line([-3.0, -1.0, 1.0, 3.0], [0.0])                           # 999 and 1001 around 1000: |d| equal, strict <
    assert check(halfway, "nearest")["picks"] == [(2, -1)]
    nearer_before = line([-3.0, -1.0, 1.5, 3.0], [0.0])
    assert check(nearer_before, "nearest")["picks"] == [(1, -1)]
    assert check(nearer_before, "linear")["picks"] == [(1, 2)]


def test_before_every_kept_pair_and_after_every_one():
    before = line([1.0, 2.0, 3.0, 4.0], [0.0])
    assert check(before, "nearest")["picks"] == [(0, -1)]
    want = check(before, "linear")
    assert want["picks"] == [(-1, 0)] and want["failures"] == [(8, 9)] and want["n_kept"] == [4]
    after = line([-4.0, -3.0, -2.0, -1.0], [0.0], beacons=[0, 1, 0, 1])
    assert check(after, "nearest")["picks"] == [(3, -1)]                    # idx == n_kept: the last pair
    assert check(after, "linear")["picks"] == [(1, 3)]                      # high clamped; the pair before is beacon 0's
    check(before, "weighted_poly")
    check(after, "weighted_poly")


def test_a_masked_pair_where_the_bisection_probes():
    """Seven pairs in the window, those at -2 and 0 dropped by the mask: kept = (-3, -1, 1, 2, 3).  The probe
    at kept rank 2 is the pair at 1 (window position 4); window position 2 is the pair at -1, on the other
    side of t0 = 0.5 -- a bisection in window coordinates ends elsewhere."""
    scene = line([-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0], [0.5, -1.5, 2.5], errors=(1, 3))
    want = check(scene, "nearest")
    assert want["n_window"] == [7, 7, 7] and want["n_kept"] == [5, 5, 5]
    assert want["picks"] == [(2, -1), (1, -1), (4, -1)]                     # window positions 4, 2, 6
    want = check(scene, "linear")
    assert want["picks"] == [(1, 2), (0, 1), (3, 4)]
    check(scene, "weighted_poly")
    # the dropped pair between `high` and the pair the walk ends on, other beacons' pairs before it
    scene = line([-5.0, -4.0, -3.0, -2.0, -1.0, 1.0, 2.0], [0.0], beacons=[1, 1, 0, 1, 0, 1, 0], errors=(3,))
    want = check(scene, "linear")
    assert want["n_kept"] == [6] and want["picks"] == [(1, 4)]             # kept: 1 1 0 (x) 0 | 1 0 -> high 4, low over two 0s


def test_a_list_that_is_not_monotone():
    rng = np.random.default_rng(8)
    differ = 0
    for trial in range(4):
        scene = Scene(trial)
        stamps = rng.permutation(np.arange(-12.0, 12.0, 0.5)) if trial else np.arange(12.0, -12.0, -0.5)
        for k, t in enumerate(np.sort(stamps)):
            scene.send(k % 2, float(t), [0, 1], stamp=float(stamps[k]), soa_error=40.0 if k % 11 == 4 else 0.0)
        for t in (-6.0, 0.0, 5.5):
            scene.send(7, t, [1, 0])
        for model in MODELS:
            want = check(scene, model)
        differ += len(set(want["picks"]))
    assert differ > 4


def test_the_walk_down_crosses_other_beacons_pairs_and_runs_out():
    far = line([-5.0, -4.0, -3.0, -2.0, -1.0, 1.0], [0.0], beacons=[1, 0, 0, 0, 0, 1])
    want = check(far, "linear")
    assert want["picks"] == [(0, 5)] and want["failures"] == []
    out = line([-4.0, -3.0, -2.0, -1.0, 1.0], [0.0], beacons=[0, 0, 0, 0, 1])
    want = check(out, "linear")
    assert want["picks"] == [(-1, 4)] and want["failures"] == [(10, 11)] and want["groups"] == []
    assert check(out, "nearest")["failures"] == []
    # a long walk: the only earlier pair of beacon 1 is the window's first, more than two trips of 64 below
    n = 150
    long_walk = line(np.linspace(-7.5, -0.1, n).tolist() + [0.2], [0.0], beacons=[1] + [0] * (n - 1) + [1], errors=(40, 90))
    want = check(long_walk, "linear")
    assert want["picks"] == [(0, want["n_kept"][0] - 1)] and want["n_kept"][0] < n + 1


@pytest.mark.parametrize("length", [63, 64, 65, 128, LDS - 1, LDS, LDS + 1, 2 * LDS + 3])
def test_kept_lists_at_the_trip_and_staging_seams(length):
    """Kept lists of exactly `length` pairs (nothing masked), and windows of `length` with every 17th pair
    masked.  The beacon transmissions thin out over the window, so the mobiles' picks lie past the window's
    middle, among its first and among its last pairs: every trip of 64 is picked from."""
    for outlier_every in (0, 17):
        scene = Scene(length)
        inside = (-8.0 + 16.0 * np.linspace(0.0, 1.0, length) ** 2).tolist()      # dense early, sparse late
        for k, t in enumerate([-20.0, -15.0, -8.5] + inside + [8.5, 12.0, 30.0]):
            scene.send(k % 2, t, (0, 1), soa_error=40.0 if outlier_every and k % outlier_every == 5 else 0.0)
        for t in (0.0, 0.03, -7.97, 7.97, 3.1):
            scene.send(7, t, (0, 1))
        for model in MODELS:
            want = check(scene, model)
            assert want["n_window"][0] == length
            assert (want["n_kept"][0] == length) == (outlier_every == 0)
            assert want["failures"] == []
        assert len(set(want["picks"])) >= 3


@pytest.mark.parametrize("n_mobile", [3 * WAVES - 4, 3 * WAVES - 3, 3 * WAVES - 2, 1])
def test_task_counts_around_the_workgroup(n_mobile):
    """One task per two-receiver match and three of a last match: 3 * WAVES - 1 / + 0 / + 1 tasks, and WAVES."""
    scene = Scene(n_mobile)
    for k in range(40):
        scene.send(k % 2, -10.0 + 0.5 * k, [0, 1, 2])
    for k in range(n_mobile):
        scene.send(5 + k % 2, -3.0 + 0.7 * k, [1, 0])
    scene.send(6, 2.2, [2, 0, 1])                          # three more tasks
    for model in MODELS:
        want = check(scene, model)
        assert len(want["n_window"]) == n_mobile + 3 and want["failures"] == []


@pytest.mark.parametrize("model", MODELS)
def test_a_gross_error_is_beyond_max_tdoa(model):
    scene = Scene(7)
    for k in range(20):
        scene.send(k % 2, -5.0 + 0.5 * k, [0, 1])
    scene.send(7, 0.1, [0, 1], soa_error=600.0)
    scene.send(7, 1.1, [0, 1])
    want = check(scene, model)
    assert want["failures"] == [(40, 41)] and [g[0] for g in want["groups"]] == [21]
    assert want["picks"][0] != (-1, -1) or model == "weighted_poly"         # it failed AFTER it picked


def shift_pair(scene, match, soa0):
    """Beacon pair `match` moved so that its det0 SoA is `soa0`, its SoA difference (what the mask sees) kept."""
    a, b = scene.matches[match]
    delta = soa0 - scene.rows[a][3]
    for i in (a, b):
        scene.rows[i] = scene.rows[i][:3] + (scene.rows[i][3] + delta,) + scene.rows[i][4:]


def test_equal_soas_are_failures_where_the_reference_divides_by_zero():
    scene = line([-3.0, -2.0, -1.0, 1.0, 2.0], [0.0, 0.4])
    shift_pair(scene, 3, scene.rows[scene.matches[2][0]][3])          # S0[high] == S0[low] for the pairs at -1 and 1
    want = check(scene, "linear")
    assert want["n_kept"] == [5, 5] and want["picks"] == [(2, 3), (2, 3)] and len(want["failures"]) == 2
    assert check(scene, "nearest")["failures"] == []
    scene = line([-3.0, -2.0, -1.0, 1.0, 2.0], [0.0, 0.4])
    shift_pair(scene, 1, scene.rows[scene.matches[5][0]][3])          # a kept pair AT the first mobile's soa0
    want = check(scene, "weighted_poly")
    assert want["n_kept"] == [5, 5] and want["failures"] == [(10, 11)] and len(want["groups"]) == 1
    assert check(scene, "linear")["failures"] == []
