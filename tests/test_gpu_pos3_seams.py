"""The seams of k_pos_h and k_pos_z (thrifty_amd/csrc/pos3.hip): group sizes around one trip of the 8-lane team and
around the register-resident rows, group counts around a workgroup's 32 teams, no group at all, the receiver count,
non-finite inputs, max_iter, and the independence of a group's bytes from its place and from the call.  Inputs are
fixture groups, repeated and truncated.  Expected positions are the fixture's x_star for unchanged groups and
tests/pos3_ref.py for derived rows, both held to the fixture's ref_err_max.  No input here makes the device fault:
every refused one is refused on the host."""
import numpy as np
import pytest

import pos3_golden
from pos3_ref import FREE_Z, KNOWN_HEIGHT, pos3_ref, pos3_ref_groups
from thrifty_amd import _native

pytestmark = pytest.mark.gpu

OK, UNDER, UNCONV, AT_BOUND, NONFINITE = (_native.POS_OK, _native.POS_UNDERDETERMINED, _native.POS_UNCONVERGED,
                                          _native.POS_AT_BOUND, _native.POS_NONFINITE)
MODES = (("h_ring6", KNOWN_HEIGHT), ("z_tall6", FREE_Z))


def dense_groups(name):
    """[(rx0, rx1, tdoa, snr, height, x_star or None)] of a fixture, receivers as dense indices."""
    g = pos3_golden.load(name)
    rx0, rx1, ptr = pos3_golden.dense(g, g["rx0"]), pos3_golden.dense(g, g["rx1"]), g["group_ptr"].tolist()
    h = g["group_h"] if len(g["group_h"]) else np.zeros(len(ptr) - 1)
    return [(rx0[a:b], rx1[a:b], g["tdoa"][a:b], g["snr"][a:b], float(h[k]), g["x_star"][k] if g["solved"][k] else None)
            for k, (a, b) in enumerate(zip(ptr[:-1], ptr[1:]))]


def start_of(g):
    return (0.1, 0.1, float(g["z0"]) if pos3_golden.free_z(g) else 0.0)


def run(groups, g, mode, **kw):
    ptr = np.cumsum([0] + [len(grp[0]) for grp in groups])
    cat = [np.concatenate([grp[k] for grp in groups]) if groups else np.zeros(0) for k in range(4)]
    heights = np.array([grp[4] for grp in groups], dtype=np.float64) if mode == KNOWN_HEIGHT else None
    kw.setdefault("x0", start_of(g))
    return _native.pos3(ptr, cat[0], cat[1], cat[2], cat[3], g["rx_xyz"], mode, heights, **kw), (ptr, cat, heights)


def resized(group, m):
    """m rows of the group, cyclically -- but one row twice for m = 2 (one pair of receivers: underdetermined in both
    modes) and a triangle for m = 3 (three receivers: solvable with the height known, underdetermined with z free)."""
    pick = np.arange(m) % len(group[0])
    if m == 2:
        pick = np.array([0, 0])
    if m == 3:
        pairs = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(group[0], group[1]))}
        pick = next(np.array([pairs[a, b], pairs[a, c], pairs[b, c]]) for (a, b) in pairs for c in range(64)
                    if (a, c) in pairs and (b, c) in pairs)
    return tuple(col[pick] for col in group[:4]) + (group[4], None)


def same_bytes(got, want, err_msg=""):
    for key in _native.POS3_OUTPUTS:
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg="%s %s" % (key, err_msg))


@pytest.mark.parametrize("name,mode", MODES)
def test_group_lengths_around_the_team_and_the_register_rows(name, mode):
    g = pos3_golden.load(name)
    base = [grp for grp in dense_groups(name) if grp[5] is not None and len(grp[0]) >= 12][:3]
    sizes = (1, 2, 3, 6, 28, 32, 33, 40)      # 32: exactly the registers; 33, 40: the re-read path
    groups = [resized(grp, m) for grp in base for m in sizes]
    out, (ptr, cat, heights) = run(groups, g, mode)
    want = pos3_ref_groups(ptr, cat[0].astype(int), cat[1].astype(int), cat[2], cat[3], g["rx_xyz"], mode, heights, start_of(g))
    np.testing.assert_array_equal(out["status"], want["status"])
    np.testing.assert_array_equal(out["status"], np.tile(np.where(np.array(sizes) <= (3 if mode == FREE_Z else 2), UNDER, OK), len(base)))
    solved = out["status"] == OK
    assert solved[np.tile(np.array(sizes) >= 28, len(base))].all()
    err = np.max(np.abs(out["pos"][solved] - want["pos"][solved]))
    print("max |x_dev - x_pos3_ref| = %.3g m" % err)
    assert err <= float(g["ref_err_max"])
    for key in ("dop", "hdop") + (("vdop",) if mode == FREE_Z else ()):
        np.testing.assert_allclose(out[key][solved], want[key][solved], rtol=float(g["dop_ref_err_max"]), atol=0, err_msg=key)
    np.testing.assert_array_equal(out["snr"], want["snr"])      # pos3_ref adds in the device's order


@pytest.mark.parametrize("name,mode", MODES)
@pytest.mark.parametrize("n", [0, _native.POS3_GROUPS_PER_WORKGROUP - 1, _native.POS3_GROUPS_PER_WORKGROUP,
                               _native.POS3_GROUPS_PER_WORKGROUP + 1, 2 * _native.POS3_GROUPS_PER_WORKGROUP + 1])
def test_group_counts_around_a_workgroup(name, mode, n):
    g = pos3_golden.load(name)
    base = dense_groups(name)
    groups = [base[k % len(base)] for k in range(n)]
    out, _ = run(groups, g, mode)
    assert all(len(out[key]) == n for key in _native.POS3_OUTPUTS) and out["pos"].shape == (n, 3)
    solved = np.array([grp[5] is not None for grp in groups], dtype=bool)
    np.testing.assert_array_equal(out["status"], np.where(solved, OK, UNDER))
    if solved.any():
        axes = 3 if mode == FREE_Z else 2
        star = np.array([grp[5] for grp in groups if grp[5] is not None])
        assert np.max(np.abs(out["pos"][solved] - star)[:, :axes]) <= float(g["ref_err_max"])


@pytest.mark.parametrize("name,mode", MODES)
def test_a_groups_bytes_do_not_depend_on_its_place_or_the_call(name, mode):
    g = pos3_golden.load(name)
    groups = dense_groups(name)
    first, _ = run(groups, g, mode)
    again, _ = run(groups, g, mode)
    same_bytes(again, first, "(a repeated call)")
    order = np.random.default_rng(5).permutation(len(groups))
    assert not np.array_equal(order, np.arange(len(groups)))
    shuffled, _ = run([groups[k] for k in order], g, mode)
    same_bytes(shuffled, {key: first[key][order] for key in first}, "(permuted groups)")


def ring64():
    ang = np.linspace(0, 2 * np.pi, 65, endpoint=False)
    table = np.c_[np.cos(ang) * 500.0, np.sin(ang) * 500.0, 5.0 + 60.0 * (np.arange(65) % 4)]
    mobile = np.array([120.0, -75.0, 1.5])
    rx0, rx1 = np.array([0, 21, 42, 63, 63, 10]), np.array([21, 42, 63, 0, 31, 53])
    tdoa = (np.linalg.norm(table[rx0] - mobile, axis=1) - np.linalg.norm(table[rx1] - mobile, axis=1)) / 2.997e8
    return table, mobile, rx0, rx1, tdoa


@pytest.mark.parametrize("mode", [KNOWN_HEIGHT, FREE_Z])
def test_sixty_four_receivers_pass_and_sixty_five_are_refused(mode):
    table, mobile, rx0, rx1, tdoa = ring64()
    heights = [mobile[2]] if mode == KNOWN_HEIGHT else None
    out = _native.pos3([0, 6], rx0, rx1, tdoa, np.ones(6), table[:64], mode, heights, x0=(0.1, 0.1, 4.0))
    want = pos3_ref(rx0, rx1, tdoa, np.ones(6), table[:64], mode, mobile[2], (0.1, 0.1, 4.0))
    assert out["status"][0] == OK == want[6]
    # exact tdoas (c 2^-53 |t| of noise, amplified by the dop of the geometry, below 10): the mobile itself
    assert np.max(np.abs(out["pos"][0] - mobile)) <= 1e-6 and np.max(np.abs(want[0] - mobile)) <= 1e-6
    with pytest.raises(ValueError, match="1 to 64 receivers, not 65"):
        _native.pos3([0, 6], rx0, rx1, tdoa, np.ones(6), table, mode, heights, x0=(0.1, 0.1, 4.0))


@pytest.mark.parametrize("name,mode", MODES)
def test_a_nan_tdoa_fails_its_group_only(name, mode):
    g = pos3_golden.load(name)
    groups = [grp for grp in dense_groups(name) if grp[5] is not None][:9]
    clean, _ = run(groups, g, mode)
    for value in (np.nan, np.inf):
        tdoa = groups[4][2].copy()
        tdoa[1] = value
        dirty, _ = run(groups[:4] + [(groups[4][0], groups[4][1], tdoa) + groups[4][3:]] + groups[5:], g, mode)
        assert dirty["status"][4] == NONFINITE and dirty["iters"][4] == 0
        others = np.arange(9) != 4
        same_bytes({key: dirty[key][others] for key in dirty}, {key: clean[key][others] for key in clean}, "(the other groups)")


@pytest.mark.parametrize("name,mode", MODES)
def test_a_start_on_a_receiver_is_nonfinite_for_the_groups_that_name_it(name, mode):
    g = pos3_golden.load(name)
    groups = [grp for grp in dense_groups(name) if grp[5] is not None][:8]
    rx = g["rx_xyz"][0]
    if mode == KNOWN_HEIGHT:      # the iterate meets the receiver where the height is the receiver's own
        groups = [grp[:4] + (float(rx[2]), None) for grp in groups]
    out, _ = run(groups, g, mode, x0=tuple(rx))
    names = np.array([bool(np.any(grp[0] == 0) or np.any(grp[1] == 0)) for grp in groups])
    assert names.any()
    np.testing.assert_array_equal(out["status"][names], NONFINITE)
    np.testing.assert_array_equal(out["iters"][names], 0)
    assert not np.any(out["status"][~names] == NONFINITE)


@pytest.mark.parametrize("name,mode", MODES)
@pytest.mark.parametrize("max_iter", [0, 1, 3])
def test_max_iter_stops_where_pos3_ref_does(name, mode, max_iter):
    g = pos3_golden.load(name)
    group = next(grp for grp in dense_groups(name) if grp[5] is not None)
    out, _ = run([group], g, mode, max_iter=max_iter)
    want = pos3_ref(group[0], group[1], group[2], group[3], g["rx_xyz"], mode, group[4], start_of(g), max_iter=max_iter)
    assert out["status"][0] == UNCONV == want[6] and out["iters"][0] == max_iter == want[7]
    np.testing.assert_allclose(out["pos"][0], want[0], rtol=1e-9, atol=0)
    for col, key in ((1, "dop"), (2, "hdop"), (4, "rms")):
        np.testing.assert_allclose(out[key][0], want[col], rtol=1e-9, atol=0, err_msg=key)
    if max_iter == 0:      # evaluated at the start
        np.testing.assert_array_equal(out["pos"][0], [0.1, 0.1, float(g["z0"]) if mode == FREE_Z else group[4]])


def test_a_singular_normal_matrix_gives_minus_one_three_times():
    # four receivers and the start in one plane (z = 3): no row has a z component, det(G'G) is exactly 0
    table = np.array([[0.0, 0.0, 3.0], [10.0, 0.0, 3.0], [25.0, 40.0, 3.0], [-30.0, 15.0, 3.0]])
    out = _native.pos3([0, 4], [0, 0, 1, 2], [1, 2, 3, 3], [1e-9, 2e-9, 3e-9, 4e-9], [4.0, 5.0, 9.0, 2.0], table, FREE_Z,
                       x0=(5.0, 7.0, 3.0), max_iter=0)
    assert out["dop"][0] == out["hdop"][0] == out["vdop"][0] == -1.0
    assert out["status"][0] == UNCONV and out["snr"][0] == 5.0
    np.testing.assert_array_equal(out["pos"][0], [5.0, 7.0, 3.0])


def test_what_the_host_refuses():
    table, mobile, rx0, rx1, tdoa = ring64()
    args = ([0, 6], rx0, rx1, tdoa, np.ones(6), table[:64])
    for kw, text in ((dict(mode=FREE_Z, x0=(0.1, 0.1, 4.0), z_range=(5.0, 5.0)), "z_lo < z_hi"),
                     (dict(mode=FREE_Z, x0=(0.1, 0.1, 4.0), z_range=(5.0, 50.0)), "outside the z range"),
                     (dict(mode=FREE_Z, x0=(0.1, np.nan, 4.0)), "x0 must be finite"),
                     (dict(mode=KNOWN_HEIGHT, group_h=[np.inf]), "height of group 0"),
                     (dict(mode=KNOWN_HEIGHT), "needs group_h"),
                     (dict(mode=2), "mode must be"),
                     (dict(mode=FREE_Z, max_iter=-1), "max_iter")):
        with pytest.raises(ValueError, match=text):
            _native.pos3(*args, **kw)
    with pytest.raises(ValueError, match="names receivers"):
        _native.pos3([0, 6], rx0, rx1 + 1, tdoa, np.ones(6), table[:64], FREE_Z)
    with pytest.raises(ValueError, match="decreases"):
        _native.pos3([0, 6, 5, 6], rx0, rx1, tdoa, np.ones(6), table[:64], FREE_Z)
