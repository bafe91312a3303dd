"""The weighted, nearest and linear TDOA models on the device against the fixtures the reference's own
builders produced (tests/golden/make_golden_tdoa_models.py).  Exact: groups, receivers, detection indices,
the row order, the failures, n_window and n_kept.  `tdoa` of nearest and linear: the reference's bits.
`tdoa` of the weighted polynomial: as close to the EXACT weighted least-squares answer (stored in the
fixture) as the reference is (ref_err_max, 1x) and within 2 ref_err_max of the reference -- the rule
tests/test_gpu_tdoa.py applies to the plain polynomial.  snr relative 1e-14, model_quality 1e-12.

Beside it: the command line with --model, the fused post-detect call against the staged calls for every
model (byte for byte), thr_tdoa_model(THR_TDOA_POLY) against thr_tdoa (bit for bit), and a bad model code.

Measured on an MI355X (max |tdoa - exact|, device / reference, weighted model): see DESIGN.md 3.8."""
import numpy as np
import pytest

import postdetect_scene as scene
import tdoa_golden
import tdoa_models_golden
from tdoa_models_ref import tdoa_models_ref
from thrifty_amd import _native, cli, identify, kitchen_sink, matchmaker, pos_est, tdoa_est, toads_data

pytestmark = pytest.mark.gpu

ALL_MODELS = ("poly", "weighted_poly", "nearest", "linear")


def cols_of(g):
    return {key: g[key] for key in ("rxid", "txid", "timestamp", "soa", "energy", "noise")}


@pytest.mark.parametrize("name", tdoa_models_golden.SETS)
def test_columns_equal_the_reference(name):
    g = tdoa_models_golden.load(name)
    rx_pos, beacon_pos = tdoa_golden.positions(g)
    res = tdoa_est.tdoa_columns(cols_of(g), g["match_ptr"], g["match_idx"], float(g["window"]), beacon_pos, rx_pos,
                                float(g["sample_rate"]), int(g["deg"]), model=g["model"])
    rows = res["tdoas"]
    assert rows.dtype == np.dtype(tdoa_est.TDOA_DTYPE)
    tdoa_models_golden.check_against_fixture(
        g, res["group_id"], res["timestamp"], res["tx"], res["group_ptr"],
        {"rx0": rows["rx0"], "rx1": rows["rx1"], "tdoa": rows["tdoa"], "snr": rows["snr"],
         "model_quality": rows["model_quality"], "det0": rows["det0_idx"], "det1": rows["det1_idx"]},
        res["failures"], res["n_window"], res["n_kept"])
    # the picks are the sequential statement's (which the host tests hold to the same fixtures)
    want = tdoa_models_ref(g["rxid"], g["txid"], g["timestamp"], g["soa"], g["energy"], g["noise"],
                           tdoa_golden.matches(g), float(g["window"]), beacon_pos, rx_pos, float(g["sample_rate"]),
                           g["model"], int(g["deg"]))
    assert res["picks"].dtype == np.int32 and res["picks"].shape == (len(g["n_window"]), 2)
    assert [tuple(p) for p in res["picks"].tolist()] == want["picks"]


@pytest.mark.parametrize("name", tdoa_models_golden.SETS)
def test_estimate_tdoas_equals_the_reference(name):
    g = tdoa_models_golden.load(name)
    rx_pos, beacon_pos = tdoa_golden.positions(g)
    builder = getattr(tdoa_est, "build_model_" + g["model"])
    params = {"deg": int(g["deg"])} if g["model"] == "weighted_poly" else None
    groups, failures = tdoa_est.estimate_tdoas(tdoa_golden.detections(g), tdoa_golden.matches(g), float(g["window"]),
                                               beacon_pos, rx_pos, float(g["sample_rate"]), deg=3,
                                               model_builder=builder, model_params=params)
    assert all(isinstance(grp, tdoa_est.TdoaGroup) and isinstance(grp.group_id, int) for grp in groups)
    table = tdoa_est.groups_to_matrix(groups)
    tdoa_models_golden.check_against_fixture(
        g, [grp.group_id for grp in groups], [grp.timestamp for grp in groups], [grp.tx for grp in groups],
        np.cumsum([0] + [len(grp.tdoas) for grp in groups]),
        {"rx0": table["rx0"], "rx1": table["rx1"], "tdoa": table["tdoa"], "snr": table["snr"],
         "model_quality": table["model_quality"], "det0": table["det0_idx"], "det1": table["det1_idx"]}, failures)


def test_command_line_writes_the_nearest_models_tdoa_file(tmp_path, capsys):
    g = tdoa_models_golden.load("tdoa_failures_nearest")
    rx_pos, beacon_pos = tdoa_golden.positions(g)
    toads, match, out = tmp_path / "data.toads", tmp_path / "data.match", tmp_path / "data.tdoa"
    rx_cfg, beacon_cfg = tmp_path / "pos-rx.cfg", tmp_path / "pos-beacon.cfg"
    dets = tdoa_golden.detections(g)
    toads.write_text("".join(d.serialize() + "\n" for d in dets))
    with open(str(match), "w") as handle:
        matchmaker.save_matches(tdoa_golden.matches(g), handle)
    rx_cfg.write_text("".join("%d: %r %r\n" % (r, float(p[0]), float(p[1])) for r, p in rx_pos.items()))
    beacon_cfg.write_text("".join("%d: %r %r\n" % (b, float(p[0]), float(p[1])) for b, p in beacon_pos.items()))
    argv = [str(toads), str(match), "-o", str(out), "-r", str(rx_cfg), "-b", str(beacon_cfg), "--model", "nearest"]
    assert cli.main(["tdoa"] + argv) == 0
    printed = capsys.readouterr().out.splitlines()
    back = tdoa_est.load_tdoa_groups(str(out))
    # a .toads line keeps eight decimals of the SoA: the expectation is the in-process call on what the file holds
    with open(str(toads)) as handle:
        reread = toads_data.load_toads(handle)
    groups, failures = tdoa_est.estimate_tdoas(reread, tdoa_golden.matches(g), 8.0, beacon_pos, rx_pos, 2.4e6,
                                               model_builder=tdoa_est.build_model_nearest)
    assert printed == ["Number of TDOA estimations: %d" % len(groups), "Number of TDOA estimation failures: %d" % len(failures)]
    assert len(failures) == len(g["failures"]) and [grp.group_id for grp in back] == g["group_id"].tolist()
    want, got = tdoa_est.groups_to_matrix(groups), tdoa_est.groups_to_matrix(back)
    for key in ("group_id", "timestamp", "tx", "rx0", "rx1", "snr", "model_quality", "det0_idx", "det1_idx"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    np.testing.assert_array_equal(got["tdoa"], want["tdoa"] * 1e9 / 1e9)       # through the text's nanoseconds
    np.testing.assert_array_equal(got["det0_idx"], g["det0"])
    # the polynomial needs three kept pairs where nearest needs one: the same file without --model has fewer rows
    assert cli.main(["tdoa"] + argv[:-2]) == 0
    capsys.readouterr()
    assert len(tdoa_est.load_tdoa_matrix(str(out))) < len(got)


@pytest.fixture(scope="module")
def front():
    """identify and match of the post-detect scene, once: the models share them."""
    cols, st = scene.columns(140), scene.settings()
    txid, keep, order = identify.integrate_columns(cols, st.tx_freqs)
    toads = {name: np.asarray(cols[name])[order] for name in ("rxid", "timestamp", "soa", "energy", "noise")}
    toads["txid"] = txid[order]
    ptr, idx, misses, collisions = matchmaker.match_columns(toads, st.match_window, 2)
    return cols, st, toads, {"txid": txid, "keep": keep, "kept_order": order, "match_ptr": ptr, "match_idx": idx,
                             "misses": misses, "collisions": collisions}


@pytest.mark.parametrize("model", ALL_MODELS)
def test_fused_call_equals_the_staged_calls(front, model):
    cols, st, toads, want = front
    want = dict(want)
    td = tdoa_est.tdoa_columns(toads, want["match_ptr"], want["match_idx"], st.tdoa_est_window, st.beacon_pos, st.rx_pos,
                               st.sample_rate, model=model)
    rows = td["tdoas"]
    want.update(td)
    want.update(pos_est.pos_columns(td["group_ptr"], rows["rx0"], rows["rx1"], rows["tdoa"], rows["snr"], st.rx_pos))
    got = kitchen_sink.postdetect_columns(cols, st, tdoa_model=getattr(tdoa_est, "build_model_" + model))
    scene.assert_identical(got, want)
    assert got["counts"]["rows"] > 50
    if model == "poly":
        scene.assert_identical(kitchen_sink.postdetect_columns(cols, st), want)           # the default is the polynomial
    else:
        assert scene.staged(cols, st)["tdoas"].tobytes() != want["tdoas"].tobytes()


def test_postdetect_takes_the_model_through_patch_module(front):
    cols, st, toads, want = front
    objects = [toads_data.DetectionResult(float(cols["timestamp"][i]), int(cols["block"][i]), float(cols["soa"][i]),
                                          toads_data.CarrierSyncInfo(int(cols["carrier_bin"][i]), float(cols["carrier_offset"][i]), 9.0, 1.0),
                                          toads_data.CorrDetectionInfo(100, 0.25, float(cols["energy"][i]), float(cols["noise"][i])),
                                          rxid=int(cols["rxid"][i])) for i in range(len(cols["rxid"]))]
    estimator = kitchen_sink.patch_module(tdoa_est.estimate_tdoas, model_builder=tdoa_est.build_model_linear)
    assert kitchen_sink._fused_tdoa_options(estimator) == {"tdoa_model": tdoa_est.build_model_linear, "deg": 2}
    result = kitchen_sink.postdetect(objects, st, tdoa_estimator=estimator)
    td = tdoa_est.tdoa_columns(toads, want["match_ptr"], want["match_idx"], st.tdoa_est_window, st.beacon_pos, st.rx_pos,
                               st.sample_rate, model="linear")
    assert [g.group_id for g in result.tdoas] == td["group_id"].tolist()
    assert np.concatenate([g.tdoas for g in result.tdoas]).tobytes() == td["tdoas"].tobytes()


def test_locate_with_a_model_writes_the_files_of_the_four_commands(front, tmp_path, monkeypatch, capsys):
    cols, st, _, _ = front
    monkeypatch.chdir(tmp_path)
    lines = [toads_data.DetectionResult(float(cols["timestamp"][i]), int(cols["block"][i]), float(cols["soa"][i]),
                                        toads_data.CarrierSyncInfo(int(cols["carrier_bin"][i]), float(cols["carrier_offset"][i]), 9.0, 1.0),
                                        toads_data.CorrDetectionInfo(100, 0.25, float(cols["energy"][i]), float(cols["noise"][i])),
                                        rxid=int(cols["rxid"][i])) for i in range(len(cols["rxid"]))]
    for rx in sorted(st.rx_pos):
        with open("rx%d.toad" % rx, "w") as out:
            out.write("".join(d.serialize() + "\n" for d in lines if d.rxid == rx))
    with open("freqmap.cfg", "w") as out:
        out.write("".join("%d: %r - %r\n" % (tx, scene.BIN_OF_TX[tx] - 3.0, scene.BIN_OF_TX[tx] + 3.0) for tx in sorted(scene.TX_POS)))
        out.write("".join("@%d: %d\n" % (rx, scene.BIN_OF_RX[k]) for k, rx in enumerate(sorted(st.rx_pos))))
    for name, table in (("pos-rx.cfg", st.rx_pos), ("pos-beacon.cfg", st.beacon_pos)):
        with open(name, "w") as out:
            out.write("".join("%d: %s\n" % (key, " ".join(repr(float(v)) for v in table[key])) for key in table))
    files = ["rx%d.toad" % rx for rx in sorted(st.rx_pos)]
    assert cli.main(["identify"] + files + ["-m", "freqmap.cfg", "-o", "staged.toads"]) == 0
    assert cli.main(["match", "staged.toads", "-o", "staged.match"]) == 0
    assert cli.main(["tdoa", "staged.toads", "staged.match", "-o", "staged.tdoa", "--model", "nearest"]) == 0
    assert cli.main(["pos", "staged.tdoa", "-o", "staged.pos"]) == 0
    assert cli.main(["locate"] + files + ["-m", "freqmap.cfg", "--prefix", "fused", "--tdoa-model", "nearest"]) == 0
    capsys.readouterr()
    for ext in ("toads", "match", "tdoa", "pos"):
        with open("staged." + ext, "rb") as a, open("fused." + ext, "rb") as b:
            want, got = a.read(), b.read()
        assert len(want) > 1000 and got == want, ext


def _native_args(g):
    rx_pos, beacon_pos = tdoa_golden.positions(g)
    receivers, beacons = sorted(rx_pos), sorted(beacon_pos)
    first_tx = g["txid"][g["match_idx"][g["match_ptr"][:-1]]]
    match_beacon = np.array([beacons.index(tx) if tx in beacons else -1 for tx in first_tx.tolist()], dtype=np.int32)
    dist = np.array([[tdoa_est._distance(rx_pos[r], beacon_pos[b]) for b in beacons] for r in receivers])
    dense = np.searchsorted(receivers, g["rxid"]).astype(np.int32)
    return (dense, g["timestamp"], g["soa"], g["energy"], g["noise"], g["match_ptr"], g["match_idx"], match_beacon, dist,
            8.0, 2.4e6)


@pytest.mark.parametrize("deg", [1, 2, 3])
def test_the_polynomial_through_thr_tdoa_model_is_thr_tdoa(deg):
    args = _native_args(tdoa_golden.load("tdoa_failures" if deg == 2 else "tdoa_ties"))
    old, new = _native.tdoa(*args, deg=deg, model=None), _native.tdoa(*args, deg=deg, model=_native.TDOA_MODELS["poly"])
    assert len(old["tdoa"]) > 0 and len(old["failures"]) + len(old["tdoa"]) == len(old["n_kept"])
    for key in old:
        assert old[key].dtype == new[key].dtype and old[key].shape == new[key].shape, key
        assert old[key].tobytes() == new[key].tobytes(), key
    assert np.all(new["picks"] == -1)


def test_a_bad_model_code_is_the_argument_error():
    args = _native_args(tdoa_golden.load("tdoa_failures"))
    for code in (-1, 4, 99):
        with pytest.raises(ValueError, match="model must be"):
            _native.tdoa(*args, model=code)
    with pytest.raises(ValueError, match="deg must be"):
        _native.tdoa(*args, deg=4, model=_native.TDOA_MODELS["weighted_poly"])
    assert len(_native.tdoa(*args, deg=0, model=_native.TDOA_MODELS["nearest"])["tdoa"]) > 0     # deg is not read
    cols, st = scene.columns(20), scene.settings()
    native, _ = kitchen_sink._native_settings(st, 2, 2, (0.1, 0.1), 100, False)
    native[0].tdoa_model = 7
    with pytest.raises(ValueError, match="tdoa_model must be"):
        _native.postdetect(*[cols[name] for name in kitchen_sink.COLUMNS], settings=native)
