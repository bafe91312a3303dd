"""`pos_3d` on the device against the fixtures of tests/golden/make_golden_pos3.py, through `pos3_columns`, `solve`
and the command line.  Exact: which groups are solved and in what order, group_id, timestamp, tx, the statuses and
the printed failure lines.  The position must be as close to the EXACT minimiser (x_star, 50-digit Newton, stored in
the fixture; the constrained one on the bound for z_box) as SciPy is (ref_err_max, 1x); dop, hdop and vdop within
dop_ref_err_max (relative) of the exact values; snr within (m - 1) 2^-53 sum|snr_i| / m.

Bit identity with `thr_pos`: the 2-D fixtures of tests/golden/pos with every receiver lifted to z = 12.5, solved with
the height 12.5 known, give position, dop, snr, status and iters of `pos_est.pos_columns` on the flat table byte for
byte.

The NumPy restatement (tests/pos3_ref.py) measures, max |x - x_star| restatement / SciPy: h_ring4 3.6e-14 / 1.1e-7 m,
h_ring6 5.7e-14 / 3.2e-8 m, z_tall6 6.5e-14 / 2.7e-7 m, z_tall5 8.1e-14 / 2.2e-7 m, z_ring6 1.3e-12 / 5.2e-5 m,
z_four 1.0e-13 / 3.6e-9 m, z_box 4.9e-14 / 1.9e-7 m; the dops within 1.8e-14 relative.  On an MI355X the device
measures 3.6e-14, 5.7e-14, 8.5e-14, 6.8e-14, 1.4e-12, 7.6e-14 and 5.6e-14 m on the same sets, the dops within 1.9e-14
relative."""
import sys

import numpy as np
import pytest

import pos3_golden
import pos_golden
from thrifty_amd import _native, pos_3d, pos_est, tdoa_est

pytestmark = pytest.mark.gpu

DROPPED = (_native.POS_UNDERDETERMINED, _native.POS_NONFINITE)


@pytest.mark.parametrize("name", pos3_golden.SETS)
def test_columns_equal_the_exact_minimiser(name):
    g = pos3_golden.load(name)
    out = pos_3d.pos3_columns(g["group_ptr"], g["rx0"], g["rx1"], g["tdoa"], g["snr"], pos3_golden.rx_pos(g),
                              **pos3_golden.mode_args(g))
    dropped = np.isin(out["status"], DROPPED)
    np.testing.assert_array_equal(~dropped, g["solved"])
    np.testing.assert_array_equal(out["status"][dropped], _native.POS_UNDERDETERMINED)
    np.testing.assert_array_equal(out["status"][~dropped], np.where(g["on_bound"][~dropped], _native.POS_AT_BOUND, _native.POS_OK))
    print("iterations: max %d; rms %.3g .. %.3g m" % (out["iters"].max(), out["rms"][~dropped].min(), out["rms"][~dropped].max()))
    keep = ~dropped
    pos3_golden.check_positions(g, g["group_id"][keep], g["group_timestamp"][keep], g["group_tx"][keep], out["pos"][keep],
                                out["dop"][keep], out["snr"][keep], out["hdop"][keep], out["vdop"][keep])
    if pos3_golden.free_z(g):
        if g["on_bound"].any():
            lo = float(g["z_range"][0])
            np.testing.assert_array_equal(out["pos"][g["on_bound"], 2], lo)
            assert np.all(out["pos"][keep & ~g["on_bound"], 2] > lo)
    else:       # the height is given back, the dilution is horizontal
        np.testing.assert_array_equal(out["pos"][:, 2], g["group_h"])
        np.testing.assert_array_equal(out["hdop"], out["dop"])
        np.testing.assert_array_equal(out["vdop"], 0.0)
    # the r.m.s. residual is the cost at the answer: against NumPy on the device's own position
    ptr, table = g["group_ptr"].tolist(), g["rx_xyz"]
    a, b = table[pos3_golden.dense(g, g["rx0"])], table[pos3_golden.dense(g, g["rx1"])]
    for k in np.flatnonzero(keep).tolist():
        rows = slice(ptr[k], ptr[k + 1])
        p = out["pos"][k]
        res = g["tdoa"][rows] * 2.997e8 - (np.linalg.norm(a[rows] - p, axis=1) - np.linalg.norm(b[rows] - p, axis=1))
        # each residual carries a few ulp of the ranges (up to some hundred metres): 1e-12 m is generous and tiny
        assert abs(out["rms"][k] - np.sqrt(np.mean(res * res))) <= 1e-12 + 1e-12 * out["rms"][k]


def test_the_height_forms_agree_to_the_byte():
    g = pos3_golden.load("h_ring6")
    args = (g["group_ptr"], g["rx0"], g["rx1"], g["tdoa"], g["snr"], pos3_golden.rx_pos(g))
    column = pos_3d.pos3_columns(*args, height=g["group_h"])
    by_tx = pos_3d.pos3_columns(*args, group_tx=g["group_tx"], **pos3_golden.mode_args(g, by_tx=True))
    for key in _native.POS3_OUTPUTS:
        np.testing.assert_array_equal(column[key], by_tx[key], err_msg=key)
    one = pos_3d.pos3_columns(*args, height=float(g["group_h"][0]))
    same = g["group_h"] == g["group_h"][0]
    assert same.any() and not same.all()
    for key in _native.POS3_OUTPUTS:
        np.testing.assert_array_equal(column[key][same], one[key][same], err_msg=key)


@pytest.mark.parametrize("name", pos3_golden.SETS)
def test_solve_equals_the_exact_minimiser(name, capsys):
    g = pos3_golden.load(name)
    details = {}
    res = pos_3d.solve(pos3_golden.groups(g), pos3_golden.rx_pos(g), details=details, **pos3_golden.mode_args(g, by_tx=True))
    assert capsys.readouterr().out.splitlines() == pos3_golden.failure_lines(g)
    axes = ("x", "y", "z") if pos3_golden.free_z(g) else ("x", "y")
    assert res.dtype.names == pos_est.POSITION_INFO_DTYPE["names"][:5 + len(axes)]
    pos3_golden.check_positions(g, res["group_id"], res["timestamp"], res["tx"], np.stack([res[axis] for axis in axes], axis=1),
                                res["dop"], res["snr"])
    np.testing.assert_array_equal(details["group_id"], g["group_id"])
    assert all(len(details[key]) == len(g["group_id"]) for key in _native.POS3_OUTPUTS)


@pytest.mark.parametrize("name", pos3_golden.SETS)
def test_command_line_writes_the_pos_file(name, tmp_path, capsys):
    g = pos3_golden.load(name)
    tdoa, out, cfg, npz = tmp_path / "data.tdoa", tmp_path / "data.pos", tmp_path / "pos-rx.cfg", tmp_path / "more.npz"
    tdoa_est.save_tdoa_groups(str(tdoa), pos3_golden.groups(g))
    cfg.write_text("".join("%d: %s\n" % (r, " ".join(repr(float(v)) for v in xyz)) for r, xyz in pos3_golden.rx_pos(g).items()))
    if pos3_golden.free_z(g):
        mode = ["--free-z", "--z0", repr(float(g["z0"]))]
        if len(g["z_range"]):
            mode += ["--z-range"] + [repr(float(v)) for v in g["z_range"]]
    elif len(g["tx_height"]):
        mode = ["--height", "0.0", "--height-tx"] + ["%d=%r" % (int(tx), float(h)) for tx, h in g["tx_height"]]
    else:
        # one height on the command line: the groups that have it (a set with per-group heights is not a deployment's)
        mode = ["--height", repr(float(g["group_h"][0]))]
    pos_3d._main([str(tdoa), "-o", str(out), "-r", str(cfg), "--npz", str(npz)] + mode)
    printed = capsys.readouterr().out.splitlines()
    assert printed == pos3_golden.failure_lines(g)
    assert not sys.stdout.closed
    got = pos_est.load_positions(str(out))
    axes = ("x", "y", "z") if pos3_golden.free_z(g) else ("x", "y")
    assert got.dtype.names == pos_est.POSITION_INFO_DTYPE["names"][:5 + len(axes)]
    held = tdoa_est.load_tdoa_matrix(str(tdoa))
    np.testing.assert_array_equal(held["snr"], g["snr"])
    assert np.all(np.abs(held["tdoa"] - g["tdoa"]) <= 2.0 ** -52 * np.abs(g["tdoa"]))
    with np.load(str(npz)) as more:
        assert set(more.files) == set(_native.POS3_OUTPUTS) | {"group_id"}
        np.testing.assert_array_equal(more["group_id"], g["group_id"])
        keep = ~np.isin(more["status"], DROPPED)
        np.testing.assert_array_equal(more["pos"][keep][:, :len(axes)], np.stack([got[axis] for axis in axes], axis=1))
        np.testing.assert_array_equal(more["dop"][keep], got["dop"])
    # test_gpu_pos.py's slack for the .tdoa round trip: a residual off by e moves the minimiser by at most
    # |(G'G)^-1 G'| |e| <= dop sqrt(m) max|e|, m <= 28 rows, e = c 2^-52 |t|
    slack = float(np.nanmax(g["dop_star"])) * np.sqrt(28.0) * 2.997e8 * 2.0 ** -52 * float(np.max(np.abs(g["tdoa"])))
    assert np.diff(g["group_ptr"]).max() <= 28 and slack < 1e-3 * float(g["ref_err_max"])
    if name == "h_ring4":      # only the groups whose height the command line gave are the fixture's problem
        same = (g["group_h"] == g["group_h"][0])[g["solved"]]
        assert same.any()
        ok = g["solved"]
        np.testing.assert_array_equal(got["group_id"], g["group_id"][ok])
        err = np.abs(np.stack([got["x"], got["y"]], axis=1) - g["x_star"][ok][:, :2])[same]
        assert np.max(err) <= float(g["ref_err_max"]) + slack
        return
    pos3_golden.check_positions(g, got["group_id"], got["timestamp"], got["tx"], np.stack([got[axis] for axis in axes], axis=1),
                                got["dop"], got["snr"], slack=slack)


@pytest.mark.parametrize("name", pos_golden.SETS_2D)
def test_receivers_at_the_known_height_give_thr_pos_to_the_byte(name):
    g = pos_golden.load(name)
    args = (g["group_ptr"], g["rx0"], g["rx1"], g["tdoa"], g["snr"])
    flat = pos_est.pos_columns(*args, pos_golden.rx_pos(g))
    lifted = {r: np.append(xy, 12.5) for r, xy in pos_golden.rx_pos(g).items()}
    out = pos_3d.pos3_columns(*args, lifted, height=12.5)
    assert set(flat["status"].tolist()) >= {_native.POS_OK} and flat["iters"].max() > 3
    np.testing.assert_array_equal(out["pos"][:, :2].view(np.uint64), flat["pos"].view(np.uint64))
    np.testing.assert_array_equal(out["pos"][:, 2], 12.5)
    for key in ("dop", "snr"):
        np.testing.assert_array_equal(out[key].view(np.uint64), flat[key].view(np.uint64), err_msg=key)
    for key in ("status", "iters"):
        np.testing.assert_array_equal(out[key], flat[key], err_msg=key)


def test_times_are_reported():
    g = pos3_golden.load("z_four")
    pos_3d.pos3_columns(g["group_ptr"], g["rx0"], g["rx1"], g["tdoa"], g["snr"], pos3_golden.rx_pos(g), **pos3_golden.mode_args(g))
    times = _native.pos3_times()
    assert len(times) == 3 and all(t > 0 for t in times)
