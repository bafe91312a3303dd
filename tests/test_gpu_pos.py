"""`pos` on the device against the fixtures the reference's `solve` produced
(tests/golden/make_golden_pos.py), through `pos_columns`, `solve` and the command line.  Exact: which
groups are solved and in what order, group_id, timestamp, tx, the printed failure lines, and every
output of the 1-D sets.  The position must be as close to the EXACT minimiser (x_star, 50-digit Newton,
stored in the fixture) as the reference is (ref_err_max, 1x), hence within 2 ref_err_max of the
reference; dop within dop_ref_err_max of the exact one; snr within (m - 1) 2^-53 sum|snr_i| / m.

The NumPy restatement (tests/pos_ref.py) measures, max |x - x_star| restatement / reference:
pos_ring4 3.6e-14 / 5.3e-8 m, pos_ring6 4.3e-14 / 9.3e-8 m, pos_ring8 1.1e-13 / 1.4e-7 m,
pos_three 5.7e-14 / 3.2e-8 m, pos_outside 2.9e-12 / 1.6e-4 m.  On an MI355X the device measures 3.6e-14, 3.6e-14,
1.1e-13, 5.7e-14 and 2.4e-12 m on the same sets, dop within 2.1e-14 relative."""
import sys

import numpy as np
import pytest

import pos_golden
from pos_ref import pos_ref_1d
from thrifty_amd import _native, pos_est, tdoa_est

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", pos_golden.SETS)
def test_columns_equal_the_reference(name):
    g = pos_golden.load(name)
    out = pos_est.pos_columns(g["group_ptr"], g["rx0"], g["rx1"], g["tdoa"], g["snr"], pos_golden.rx_pos(g))
    dropped = np.isin(out["status"], (_native.POS_UNDERDETERMINED, _native.POS_NONFINITE))
    np.testing.assert_array_equal(~dropped, g["solved"])
    np.testing.assert_array_equal(out["status"][dropped], _native.POS_UNDERDETERMINED)
    assert set(out["status"][~dropped].tolist()) == {_native.POS_OK}
    print("iterations: max %d" % out["iters"].max())
    keep = ~dropped
    pos_golden.check_positions(g, g["group_id"][keep], g["group_timestamp"][keep], g["group_tx"][keep],
                               out["pos"][keep], out["dop"][keep], out["snr"][keep])


@pytest.mark.parametrize("name", pos_golden.SETS)
def test_solve_equals_the_reference(name, capsys):
    g = pos_golden.load(name)
    res = pos_est.solve(pos_golden.groups(g), pos_golden.rx_pos(g))
    assert capsys.readouterr().out.splitlines() == pos_golden.failure_lines(g)
    dims = g["rx_xyz"].shape[1]
    assert res.dtype.names == pos_est.POSITION_INFO_DTYPE["names"][:5 + dims]
    pos_golden.check_positions(g, res["group_id"], res["timestamp"], res["tx"],
                               np.stack([res[axis] for axis in ("x", "y")[:dims]], axis=1), res["dop"], res["snr"])


@pytest.mark.parametrize("name", pos_golden.SETS)
def test_command_line_writes_the_pos_file(name, tmp_path, capsys):
    g = pos_golden.load(name)
    tdoa, out, cfg = tmp_path / "data.tdoa", tmp_path / "data.pos", tmp_path / "pos-rx.cfg"
    tdoa_est.save_tdoa_groups(str(tdoa), pos_golden.groups(g))
    cfg.write_text("".join("%d: %s\n" % (r, " ".join(repr(float(v)) for v in xyz)) for r, xyz in pos_golden.rx_pos(g).items()))
    pos_est._main([str(tdoa), "-o", str(out), "-r", str(cfg)])
    assert capsys.readouterr().out.splitlines() == pos_golden.failure_lines(g)
    assert not sys.stdout.closed
    got = pos_est.load_positions(str(out))
    dims = g["rx_xyz"].shape[1]
    assert got.dtype.names == pos_est.POSITION_INFO_DTYPE["names"][:5 + dims]
    # a .tdoa line holds tdoa * 1e9 and its loader divides by 1e9, so the solver sees every tdoa with up to
    # two roundings, 2^-52 |t| -- everything else in the two files is a round-trip repr
    held = tdoa_est.load_tdoa_matrix(str(tdoa))
    np.testing.assert_array_equal(held["snr"], g["snr"])
    assert np.all(np.abs(held["tdoa"] - g["tdoa"]) <= 2.0 ** -52 * np.abs(g["tdoa"]))
    if dims == 1:
        # exact: the reference's three operations (tests/pos_ref.py) on the tdoas the file holds
        ok, rx0, rx1 = g["solved"], pos_golden.dense(g, g["rx0"]), pos_golden.dense(g, g["rx1"])
        want = [pos_ref_1d(rx0[k:k + 1], rx1[k:k + 1], held["tdoa"][k:k + 1], held["snr"][k:k + 1], g["rx_xyz"])
                for k in range(len(ok))]
        np.testing.assert_array_equal(got["group_id"], g["group_id"][ok])
        np.testing.assert_array_equal(got["timestamp"], g["group_timestamp"][ok])
        np.testing.assert_array_equal(got["tx"], g["group_tx"][ok])
        np.testing.assert_array_equal(got["x"], [w[0][0] for w in want])
        np.testing.assert_array_equal(got["dop"], [w[1] for w in want])
        np.testing.assert_array_equal(got["snr"], g["snr_ref"][ok])
        assert np.all(np.abs(got["x"] - g["x_ref"][ok, 0]) <= 2.997e8 * 2.0 ** -52 * np.abs(g["tdoa"]) / 2 + 2.0 ** -52 * np.abs(got["x"]))
        return
    # a residual off by e moves the minimiser by at most |(G'G)^-1 G'| |e| <= dop sqrt(m) max|e|, m <= 28 rows,
    # e = c 2^-52 |t|: some 1e-13 m here, beside a ref_err_max of 3e-8 m and more
    slack = float(np.nanmax(g["dop_star"])) * np.sqrt(28.0) * 2.997e8 * 2.0 ** -52 * float(np.max(np.abs(g["tdoa"])))
    assert slack < 1e-3 * float(g["ref_err_max"])
    pos_golden.check_positions(g, got["group_id"], got["timestamp"], got["tx"], np.stack([got["x"], got["y"]], axis=1),
                               got["dop"], got["snr"], slack=slack)


def test_times_are_reported():
    g = pos_golden.load("pos_ring4")
    pos_est.pos_columns(g["group_ptr"], g["rx0"], g["rx1"], g["tdoa"], g["snr"], pos_golden.rx_pos(g))
    times = _native.pos_times()
    assert len(times) == 3 and all(t > 0 for t in times)
