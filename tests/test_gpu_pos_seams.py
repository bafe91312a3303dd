"""The seams of k_pos2d (thrifty_amd/csrc/pos.hip): group sizes around one trip of the 8-lane team and
around the register-resident rows, group counts around one wave's eight teams and around a workgroup,
waves that mix short and long iterations and failed groups, max_iter, non-finite inputs, the box and the
receiver count.  Inputs are fixture groups, repeated and truncated.  Expected positions are the
fixture's x_star for unchanged groups and tests/pos_ref.py for derived rows, both held to the fixture's
ref_err_max.  No input here makes the device fault: every refused one is refused on the host."""
import itertools

import numpy as np
import pytest

import pos_golden
from pos_ref import pos_ref, pos_ref_groups
from thrifty_amd import _native

pytestmark = pytest.mark.gpu

OK, UNDER, UNCONV, AT_BOUND, NONFINITE = (_native.POS_OK, _native.POS_UNDERDETERMINED, _native.POS_UNCONVERGED,
                                          _native.POS_AT_BOUND, _native.POS_NONFINITE)


def dense_groups(name):
    """[(rx0, rx1, tdoa, snr, x_star or None)] of a fixture, receivers as dense indices."""
    g = pos_golden.load(name)
    rx0, rx1, ptr = pos_golden.dense(g, g["rx0"]), pos_golden.dense(g, g["rx1"]), g["group_ptr"].tolist()
    return [(rx0[a:b], rx1[a:b], g["tdoa"][a:b], g["snr"][a:b], g["x_star"][k] if g["solved"][k] else None)
            for k, (a, b) in enumerate(zip(ptr[:-1], ptr[1:]))]


def run(groups, table, **kw):
    ptr = np.cumsum([0] + [len(grp[0]) for grp in groups])
    cat = [np.concatenate([grp[k] for grp in groups]) if groups else np.zeros(0) for k in range(4)]
    return _native.pos(ptr, cat[0], cat[1], cat[2], cat[3], table, **kw), (ptr, cat)


def resized(group, m):
    pick = np.arange(m) % len(group[0])
    return tuple(col[pick] for col in group[:4]) + (None,)


def test_group_sizes_around_the_team_and_the_register_rows():
    g = pos_golden.load("pos_ring8")
    base = [grp for grp in dense_groups("pos_ring8") if grp[4] is not None and len(grp[0]) >= 20][:3]
    sizes = (1, 2, 3, 7, 8, 9, 16, 17, 28, 32, 33, 45)
    groups = [resized(grp, m) if m > 2 else resized((grp[0][:1], grp[1][:1], grp[2][:1], grp[3][:1]), m)
              for grp in base for m in sizes]
    out, (ptr, cat) = run(groups, g["rx_xyz"])
    want = pos_ref_groups(ptr, cat[0].astype(int), cat[1].astype(int), cat[2], cat[3], g["rx_xyz"])
    np.testing.assert_array_equal(out["status"], want["status"])
    np.testing.assert_array_equal(out["status"], np.tile(np.where(np.array(sizes) <= 2, UNDER, OK), len(base)))
    solved = out["status"] == OK
    err = np.max(np.abs(out["pos"][solved] - want["pos"][solved]))
    print("max |x_dev - x_pos_ref| = %.3g m" % err)
    assert err <= float(g["ref_err_max"])
    np.testing.assert_allclose(out["dop"][solved], want["dop"][solved], rtol=float(g["dop_ref_err_max"]), atol=0)
    np.testing.assert_array_equal(out["snr"], want["snr"])      # pos_ref adds in the device's order


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 2 * _native.POS_GROUPS_PER_WORKGROUP - 1,
                               2 * _native.POS_GROUPS_PER_WORKGROUP, 2 * _native.POS_GROUPS_PER_WORKGROUP + 1])
def test_group_counts_around_a_wave_and_a_workgroup(n):
    g = pos_golden.load("pos_ring4")
    base = dense_groups("pos_ring4")
    groups = [base[k % len(base)] for k in range(n)]
    out, _ = run(groups, g["rx_xyz"])
    assert all(len(out[key]) == n for key in ("pos", "dop", "snr", "status", "iters"))
    solved = np.array([grp[4] is not None for grp in groups], dtype=bool)
    np.testing.assert_array_equal(out["status"], np.where(solved, OK, UNDER))
    if solved.any():
        star = np.array([grp[4] for grp in groups if grp[4] is not None])
        assert np.max(np.abs(out["pos"][solved] - star)) <= float(g["ref_err_max"])


def test_waves_that_mix_short_and_long_iterations_and_failures():
    three, outside = pos_golden.load("pos_three"), pos_golden.load("pos_outside")
    table = np.concatenate([three["rx_xyz"], outside["rx_xyz"]])
    shift = len(three["rx_xyz"])
    quick = dense_groups("pos_three")
    slow = [(a + shift, b + shift, t, s, star) for a, b, t, s, star in dense_groups("pos_outside")]
    failed = (quick[0][0][:1], quick[0][1][:1], quick[0][2][:1], quick[0][3][:1], None)
    groups, bound = [], []
    for wave in range(8):
        for lane in range(8):
            k = 8 * wave + lane
            if lane == wave:
                groups.append(failed), bound.append(0.0)
            elif lane % 2:
                groups.append(quick[k % len(quick)]), bound.append(float(three["ref_err_max"]))
            else:
                groups.append(slow[k % len(slow)]), bound.append(float(outside["ref_err_max"]))
    out, _ = run(groups, table)
    solved = np.array([grp[4] is not None for grp in groups], dtype=bool)
    np.testing.assert_array_equal(out["status"], np.where(solved, OK, UNDER))
    star = np.array([grp[4] for grp in groups if grp[4] is not None])
    assert np.all(np.max(np.abs(out["pos"][solved] - star), axis=1) <= np.array(bound)[solved])
    iters = out["iters"][solved]
    print("iterations in the mixed waves: %d .. %d" % (iters.min(), iters.max()))
    assert iters.max() >= 2 * iters.min()


@pytest.mark.parametrize("max_iter", [0, 1, 3])
def test_max_iter_stops_where_pos_ref_does(max_iter):
    g = pos_golden.load("pos_ring6")
    group = next(grp for grp in dense_groups("pos_ring6") if grp[4] is not None)
    out, _ = run([group], g["rx_xyz"], max_iter=max_iter)
    want = pos_ref(group[0], group[1], group[2], group[3], g["rx_xyz"], max_iter=max_iter)
    assert out["status"][0] == UNCONV == want[3] and out["iters"][0] == max_iter == want[4]
    np.testing.assert_allclose(out["pos"][0], want[0], rtol=1e-9, atol=0)
    np.testing.assert_allclose(out["dop"][0], want[1], rtol=1e-9, atol=0)
    if max_iter == 0:
        np.testing.assert_array_equal(out["pos"][0], [0.1, 0.1])


def test_dop_on_the_line_of_three_collinear_receivers_is_minus_one():
    table = np.array([[0.0, 0.0], [10.0, 0.0], [25.0, 0.0]])
    out = _native.pos([0, 3], [0, 0, 1], [1, 2, 2], [1e-9, 2e-9, 3e-9], [4.0, 5.0, 9.0], table, x0=(5.0, 0.0), max_iter=0)
    assert out["dop"][0] == -1.0 and out["status"][0] == UNCONV and out["snr"][0] == 6.0
    np.testing.assert_array_equal(out["pos"][0], [5.0, 0.0])


def test_a_nan_tdoa_fails_its_group_only():
    g = pos_golden.load("pos_ring6")
    groups = [grp for grp in dense_groups("pos_ring6") if grp[4] is not None][:9]
    clean, _ = run(groups, g["rx_xyz"])
    for value in (np.nan, np.inf):
        tdoa = groups[4][2].copy()
        tdoa[1] = value
        dirty, _ = run(groups[:4] + [(groups[4][0], groups[4][1], tdoa, groups[4][3], None)] + groups[5:], g["rx_xyz"])
        assert dirty["status"][4] == NONFINITE and dirty["iters"][4] == 0
        others = np.arange(9) != 4
        for key in ("pos", "dop", "snr", "status", "iters"):
            np.testing.assert_array_equal(dirty[key][others], clean[key][others], err_msg=key)


def test_x0_on_a_receiver_is_nonfinite_at_iteration_zero():
    g = pos_golden.load("pos_ring6")
    group = next(grp for grp in dense_groups("pos_ring6") if grp[4] is not None and 0 in grp[0])
    out, _ = run([group], g["rx_xyz"], x0=tuple(g["rx_xyz"][0]))
    assert out["status"][0] == NONFINITE and out["iters"][0] == 0


def test_a_minimum_beyond_the_box_ends_on_the_box():
    ang = np.linspace(0, 2 * np.pi, 5, endpoint=False) + 0.3
    table = np.c_[np.cos(ang), np.sin(ang)] * 100.0
    pairs = list(itertools.combinations(range(5), 2))
    rx0, rx1 = np.array([a for a, _ in pairs]), np.array([b for _, b in pairs])
    mobile = np.array([50e3, 2e3])
    tdoa = (np.linalg.norm(table[rx0] - mobile, axis=1) - np.linalg.norm(table[rx1] - mobile, axis=1)) / 2.997e8
    out = _native.pos([0, len(pairs)], rx0, rx1, tdoa, np.ones(len(pairs)), table)
    want = pos_ref(rx0, rx1, tdoa, np.ones(len(pairs)), table)
    assert want[3] == AT_BOUND and out["status"][0] == AT_BOUND
    assert out["pos"][0, 0] == table[:, 0].max() + 10e3
    # along the box the problem is 1-D and well conditioned: the two agree as the fixtures' solvers do
    assert abs(out["pos"][0, 1] - want[0][1]) <= 1e-6


def test_sixty_four_receivers_pass_and_sixty_five_are_refused():
    ang = np.linspace(0, 2 * np.pi, 65, endpoint=False)
    table = np.c_[np.cos(ang), np.sin(ang)] * 500.0
    mobile = np.array([120.0, -75.0])
    rx0, rx1 = np.array([0, 20, 41, 63, 63]), np.array([20, 41, 63, 0, 31])
    tdoa = (np.linalg.norm(table[rx0] - mobile, axis=1) - np.linalg.norm(table[rx1] - mobile, axis=1)) / 2.997e8
    out = _native.pos([0, 5], rx0, rx1, tdoa, np.ones(5), table[:64])
    assert out["status"][0] == OK and np.max(np.abs(out["pos"][0] - mobile)) <= 1e-6      # exact tdoas: c * 2^-53 * |t| of noise
    with pytest.raises(ValueError, match="1 to 64 receivers, not 65"):
        _native.pos([0, 5], rx0, rx1, tdoa, np.ones(5), table)
