"""`thr_postdetect` (kitchen_sink.postdetect_columns) against the staged device path on the same inputs,
and through its front ends.

Fused against staged is EXACT, every output bit for bit: the fused call runs the same kernels in the same
order, its dense receiver numbering preserves the order of the ids (so every receiver-pair list holds the
same pairs in the same order), and no stage accumulates floating-point values with atomics.  A
difference is a bug in the chain, not noise.

The scene (tests/postdetect_scene.py) is about 560 raw detections of 4 receivers: duplicates, unmapped
bins, misses, collisions, underdetermined groups, mobile transmissions before the first beacon; one
fixture with a frequency map, one in automatic mode, one 1-D with two receivers."""
import os

import numpy as np
import pytest

import postdetect_scene as scene
from thrifty_amd import _native, cli, kitchen_sink, pos_est, toads_data

pytestmark = pytest.mark.gpu

N_EVENTS = 140


@pytest.fixture(scope="module")
def mapped():
    cols, st = scene.columns(N_EVENTS), scene.settings()
    return cols, st, scene.staged(cols, st)


def test_fused_equals_staged_with_a_frequency_map(mapped):
    cols, st, want = mapped
    got = kitchen_sink.postdetect_columns(cols, st)
    scene.assert_identical(got, want)
    c = got["counts"]
    # the scene holds every category (figures of the sequential statements: 497 kept of 561, 132 matches,
    # 8 misses, 22 collisions, 79 groups, 23 failures)
    assert 0 < c["kept"] < len(cols["rxid"]) and (got["txid"] == -1).any()
    assert c["matches"] > 100 and c["misses"] > 0 and c["collisions"] > 0 and c["failures"] > 0
    assert c["groups"] >= 20 and c["rows"] > c["groups"] and c["tasks"] == c["rows"] + c["failures"]
    assert c["match_entries"] == int(got["match_ptr"][-1]) and c["rows"] == int(got["group_ptr"][-1])
    assert (got["status"] == _native.POS_UNDERDETERMINED).any() and (got["status"] == _native.POS_OK).sum() >= 20
    # sensible positions: the solved mobiles lie within a few metres of where the scene put them
    ok = got["status"] == _native.POS_OK
    truth = np.array([scene.TX_POS[int(tx)] for tx in got["tx"][ok]])
    assert np.abs(got["pos"][ok] - truth).max() < 50.0


def test_fused_equals_staged_in_automatic_mode():
    cols, st = scene.columns(N_EVENTS, seed=6), scene.settings(automatic=True)
    got = kitchen_sink.postdetect_columns(cols, st)
    scene.assert_identical(got, scene.staged(cols, st))
    assert got["counts"]["matches"] > 0


def test_fused_equals_staged_on_a_line():
    cols, st = scene.columns(N_EVENTS, seed=7, rx_ids=(0, 1), line=True), scene.settings(rx_ids=(0, 1), line=True)
    got = kitchen_sink.postdetect_columns(cols, st)
    scene.assert_identical(got, scene.staged(cols, st))
    assert got["pos"].shape[1] == 1 and got["counts"]["groups"] >= 20
    assert np.array_equal(np.diff(got["group_ptr"]), np.ones(got["counts"]["groups"], dtype=np.int64))
    # the order of the receiver table's first two entries decides the formula's sign: the other order too
    flipped = st._replace(rx_pos={1: st.rx_pos[1], 0: st.rx_pos[0]})
    scene.assert_identical(kitchen_sink.postdetect_columns(cols, flipped), scene.staged(cols, flipped))


def test_times_are_reported_per_stage(mapped):
    cols, st, _ = mapped
    kitchen_sink.postdetect_columns(cols, st)
    times = _native.post_times()
    assert len(times) == 6 and all(t > 0 for t in times)


def _objects(cols):
    return [toads_data.DetectionResult(float(cols["timestamp"][i]), int(cols["block"][i]), float(cols["soa"][i]),
                                       toads_data.CarrierSyncInfo(int(cols["carrier_bin"][i]), float(cols["carrier_offset"][i]), 9.0, 1.0),
                                       toads_data.CorrDetectionInfo(100, 0.25, float(cols["energy"][i]), float(cols["noise"][i])),
                                       rxid=int(cols["rxid"][i]))
            for i in range(len(cols["rxid"]))]


def test_postdetect_on_result_objects_equals_the_column_path(mapped, capsys):
    cols, st, want = mapped
    toad = _objects(cols)
    result = kitchen_sink.postdetect(toad, st)
    announced = capsys.readouterr().out
    assert [d.txid for d in toad] == want["txid"].tolist()                     # set in place
    assert [id(d) for d in result.toads] == [id(toad[i]) for i in want["kept_order"].tolist()]
    ptr, idx = want["match_ptr"].tolist(), want["match_idx"].tolist()
    assert result.matches == [idx[a:b] for a, b in zip(ptr[:-1], ptr[1:])]
    assert [g.group_id for g in result.tdoas] == want["group_id"].tolist()
    assert [g.timestamp for g in result.tdoas] == want["timestamp"].tolist()
    assert [g.tx for g in result.tdoas] == want["tx"].tolist()
    assert np.concatenate([g.tdoas for g in result.tdoas]).tobytes() == want["tdoas"].tobytes()
    keep = ~np.isin(want["status"], list(pos_est._DROPPED))
    assert result.pos.dtype.names == ("group_id", "timestamp", "tx", "dop", "snr", "x", "y")
    assert result.pos["group_id"].tolist() == want["group_id"][keep].tolist()
    for name, column in (("x", want["pos"][keep, 0]), ("y", want["pos"][keep, 1]), ("dop", want["dop"][keep]),
                         ("snr", want["snr"][keep]), ("timestamp", want["timestamp"][keep])):
        assert result.pos[name].tobytes() == np.ascontiguousarray(column).tobytes(), name
    dropped = want["group_id"][~keep].tolist()
    assert dropped and announced.splitlines() == ["Failed to estimate group #%d: Underdetermined" % g for g in dropped]


def test_locate_writes_the_files_of_the_four_commands(mapped, tmp_path, monkeypatch, capsys):
    cols, st, _ = mapped
    monkeypatch.chdir(tmp_path)
    toad = _objects(cols)
    for rx in sorted(st.rx_pos):
        with open("rx%d.toad" % rx, "w") as out:
            out.write("".join(d.serialize() + "\n" for d in toad if d.rxid == rx))
    with open("freqmap.cfg", "w") as out:
        out.write("".join("%d: %r - %r\n" % (tx, scene.BIN_OF_TX[tx] - 3.0, scene.BIN_OF_TX[tx] + 3.0) for tx in sorted(scene.TX_POS)))
        out.write("".join("@%d: %d\n" % (rx, scene.BIN_OF_RX[k]) for k, rx in enumerate(sorted(st.rx_pos))))
    for name, table in (("pos-rx.cfg", st.rx_pos), ("pos-beacon.cfg", st.beacon_pos)):
        with open(name, "w") as out:
            out.write("".join("%d: %s\n" % (key, " ".join(repr(float(v)) for v in table[key])) for key in table))
    files = ["rx%d.toad" % rx for rx in sorted(st.rx_pos)]
    assert cli.main(["identify"] + files + ["-m", "freqmap.cfg", "-o", "staged.toads"]) == 0
    assert cli.main(["match", "staged.toads", "-o", "staged.match"]) == 0
    assert cli.main(["tdoa", "staged.toads", "staged.match", "-o", "staged.tdoa"]) == 0
    assert cli.main(["pos", "staged.tdoa", "-o", "staged.pos"]) == 0
    assert cli.main(["locate"] + files + ["-m", "freqmap.cfg", "--prefix", "fused"]) == 0
    capsys.readouterr()
    for ext in ("toads", "match", "tdoa", "pos"):
        with open("staged." + ext, "rb") as a, open("fused." + ext, "rb") as b:
            want, got = a.read(), b.read()
        assert len(want) > 1000 and got == want, ext
    assert len(open("fused.pos").read().splitlines()) >= 20
    assert os.path.getsize("fused.tdoa") > os.path.getsize("fused.pos")


# ---------------------------------------------------------------- against the reference's own kitchen_sink.postdetect
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "postdetect")


@pytest.mark.parametrize("name", ["map", "auto", "line"])
def test_fused_equals_the_reference(name):
    """tests/golden/make_golden_postdetect.py ran the reference's `kitchen_sink.postdetect` on the scene.  Every
    discrete output is equal.  The fixture stores how far the reference is from the NumPy statements of the
    device algorithms (d_tdoa, d_pos, d_dop: 2.2e-12 .. 4.7e-12 s, 3.3e-4 .. 6.8e-4 m, 0 .. 1.0e-6); the device
    may be that far from them on its other side, so it is held to the reference within TWICE those distances
    (tests/test_gpu_tdoa.py's rule): tdoa absolute, snr and model_quality by the same figure relative,
    positions and dop absolute.  Measured on an MI355X (printed below): the device is 3.5e-15 .. 4.7e-15 s,
    5.2e-7 .. 7.2e-7 m and <= 1.1e-9 from the NumPy statements, so one d_* from the reference."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    cols = {c: g["col_" + c] for c in kitchen_sink.COLUMNS}
    freqmap = None
    if len(g["freqmap"]):
        freqmap = {}
        for rx, tx, lo, hi in g["freqmap"].tolist():
            freqmap.setdefault(int(rx), {})[int(tx)] = (lo, hi)
    st = kitchen_sink.PostdetectSettings(
        tx_freqs=freqmap, match_window=float(g["match_window"]), tdoa_est_window=float(g["tdoa_window"]),
        rx_pos={int(rx): xyz for rx, xyz in zip(g["rx_ids"].tolist(), g["rx_xyz"])},
        beacon_pos={int(tx): xyz for tx, xyz in zip(g["beacon_ids"].tolist(), g["beacon_xyz"])}, sample_rate=float(g["sample_rate"]))
    got = kitchen_sink.postdetect_columns(cols, st)
    for ours, theirs in (("txid", "txid"), ("kept_order", "kept_order"), ("match_ptr", "match_ptr"), ("match_idx", "match_idx"),
                         ("misses", "misses"), ("collisions", "collisions"), ("group_id", "group_id"), ("group_ptr", "group_ptr"),
                         ("timestamp", "group_timestamp"), ("tx", "group_tx")):
        assert np.array_equal(got[ours], g[theirs]), ours
    rows = got["tdoas"]
    for field, theirs in (("rx0", "rx0"), ("rx1", "rx1"), ("det0_idx", "det0"), ("det1_idx", "det1")):
        assert np.array_equal(rows[field], g[theirs]), field
    solved = ~np.isin(got["status"], list(pos_est._DROPPED))
    assert np.array_equal(got["group_id"][solved], g["pos_group_id"]) and solved.sum() >= 20
    d_tdoa, d_pos, d_dop = float(g["d_tdoa"]), float(g["d_pos"]), float(g["d_dop"])
    seen = {"tdoa": np.abs(rows["tdoa"] - g["tdoa"]).max(), "snr": np.abs(rows["snr"] / g["snr"] - 1).max(),
            "model_quality": np.abs(rows["model_quality"] / g["model_quality"] - 1).max(),
            "pos": np.abs(got["pos"][solved] - g["pos"]).max(), "dop": np.abs(got["dop"][solved] - g["dop"]).max(),
            "pos_snr": np.abs(got["snr"][solved] / g["pos_snr"] - 1).max(),
            "tdoa_np": np.abs(rows["tdoa"] - g["tdoa_np"]).max(), "pos_np": np.abs(got["pos"][solved] - g["pos_np"]).max(),
            "dop_np": np.abs(got["dop"][solved] - g["dop_np"]).max()}
    print("%s: device against the reference %s; bounds 2 x (%.3g s, %.3g m, %.3g)" % (
        name, ", ".join("%s %.3g" % item for item in seen.items()), d_tdoa, d_pos, d_dop))
    assert seen["tdoa"] <= 2 * d_tdoa
    assert seen["snr"] <= 2 * d_tdoa and seen["model_quality"] <= 2 * d_tdoa and seen["pos_snr"] <= 2 * d_tdoa
    assert seen["pos"] <= 2 * d_pos
    assert seen["dop"] <= 2 * d_dop
