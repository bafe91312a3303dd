"""`thr_track` on the device against the NumPy statement (tests/track_ref.py): three scenes of at most 4096 rows with
1, 3 and 8 interleaved tracks, duplicate timestamps, planted outliers and a block of invalid rows.  Floats within
the tolerance recorded for the scene (tests/golden/make_golden_track.py: measured on the CPU, times 16), integers
exact.  The condition for an exact mask is asserted on the reference first: in no round a nis lies within a
relative 1e-6 of the gate."""
import numpy as np
import pytest

import track_check
import track_ref
import track_scenes
from thrifty_amd import _native, pos_est, pos_quality, track

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", [0, 1, 2])
def test_every_array_against_the_reference(k):
    s, ref = track_check.gating(k)
    track_check.assert_margin(ref)
    assert len(s["tx"]) <= 4096 and ref["counts"]["tracks"] == (1, 3, 8)[k] and ref["counts"]["rounds"] == 3
    counts, out = track_check.device(s)
    track_check.compare("gating_%d" % k, counts, out, ref)
    assert counts["converged"] == 1 and not np.any(out["used"].astype(bool) & s["outlier"])
    times, geometry = _native.track_times(), _native.track_geometry()
    assert len(times) == 6 and all(t >= 0.0 for t in times) and times[2] > 0.0 and geometry == (256, 256, 14)


def test_without_a_gate_every_valid_row_is_used_in_one_run():
    s, _ = track_check.gating(1)
    ref = track_check.reference(s, gate=0.0)
    counts, out = track_check.device(s, gate=0.0)
    assert counts["rounds"] == 1 and counts["converged"] == 1 and counts["rejected"] == 0
    assert np.array_equal(out["used"], (s["valid"].astype(bool) & ref["tracked"]).astype(np.uint8))
    assert counts == ref["counts"] and np.array_equal(out["used"], ref["used"])
    track_check.compare("gating_1_no_gate", counts, out, ref)
    # the outliers pull the track: the states are not the gated ones
    assert np.nanmax(np.abs(out["filt"] - track_check.gating(1)[1]["filt"])) > 1.0


def test_one_round_on_a_scene_that_needs_three():
    s, full = track_check.gating(0)
    assert full["counts"]["rounds"] == 3
    ref = track_check.gating_0_one_round()
    track_check.assert_margin(ref)
    counts, out = track_check.device(s, max_rounds=1)
    assert counts["converged"] == 0 and counts["rounds"] == 2
    assert counts == ref["counts"] and np.array_equal(out["used"], ref["used"]) and not np.array_equal(out["used"], full["used"])
    track_check.compare("gating_0_one_round", counts, out, ref)


def test_the_interface_refuses_what_the_header_lists():
    s = track_scenes.scene(5, rows=8)
    cols = list(track_scenes.columns(s)[:6])
    for k, bad in ((1, np.nan), (1, np.inf), (2, np.nan), (4, 0.0), (5, -1.0), (4, np.inf)):
        broken = [c.copy() for c in cols]
        broken[k][3] = bad
        with pytest.raises(ValueError, match="thr_track"):
            _native.track(*broken, q=1.0)
        if k != 1:      # the same row marked invalid is taken
            valid = np.ones(8, np.uint8)
            valid[3] = 0
            assert _native.track(*broken, valid=valid, q=1.0)[0]["used"] <= 7
    for kw in (dict(q=-1.0), dict(q=1.0, v0=0.0), dict(q=1.0, gate=-1.0), dict(q=1.0, max_rounds=0), dict(q=1.0, max_rounds=17),
               dict(q=np.nan)):
        with pytest.raises(ValueError, match="thr_track"):
            _native.track(*cols, **kw)


def _written_inputs(tmp_path):
    s = track_scenes.scene(9, tracks=3, rows=120, outliers=0.03)
    n = len(s["tx"])
    posq = np.zeros(n, dtype=pos_quality.QUALITY_DTYPE)
    posq["group_id"], posq["timestamp"], posq["tx"] = np.arange(n), s["timestamp"], s["tx"]
    posq["x"], posq["y"] = s["x"], s["y"]
    posq["xdop"], posq["ydop"] = np.sqrt(s["rx"]) / 3.0, np.sqrt(s["ry"]) / 3.0
    posq["dop"] = np.sqrt(posq["xdop"] ** 2 + posq["ydop"] ** 2)
    posq["flags"][::17] = pos_quality.NO_CANDIDATE | pos_quality.INCONSISTENT
    posq["dop"][5] = -1.0
    pos = np.zeros(n, dtype=pos_est._result_dtype(2))
    for name in pos.dtype.names:
        pos[name] = posq[name]
    paths = str(tmp_path / "data.pos"), str(tmp_path / "data.posq")
    pos_est.save_positions(paths[0], pos)
    pos_quality.save_quality(paths[1], posq)
    return paths


@pytest.mark.parametrize("kind", [0, 1])
def test_the_command_line_writes_what_track_returns(tmp_path, kind, capsys):
    path = _written_inputs(tmp_path)[kind]
    out_path = str(tmp_path / "data.track")
    assert track._main([path, "-o", out_path, "--sigma", "3", "--accel", "0.5"]) == 0
    loaded = (pos_est.load_positions, pos_quality.load_quality)[kind](path)
    records, out = track.track(loaded, 3.0, 0.5)
    written = track.load_tracks(out_path)
    assert len(written) == len(records) > 300
    for name in track.TRACK_DTYPE["names"]:
        assert np.array_equal(written[name], records[name], equal_nan=True), name
    assert capsys.readouterr().out == track.format_summary(out)
    rx, ry, valid = track.measurement_columns(loaded, 3.0)
    assert not np.any(out["used"][~valid]) and np.count_nonzero(~valid) >= (1, 22)[kind]
    ref = track_ref.run(loaded["tx"], loaded["timestamp"], loaded["x"], loaded["y"], rx, ry, valid, q=0.25, v0=10.0)
    track_check.assert_margin(ref)
    assert out["counts"] == ref["counts"] and np.array_equal(out["used"], ref["used"])
