"""`thr_postdetect` at its seams: sizes around the wavefront and the workgroup of its own kernels, every
stage producing nothing, its errors, a beacon nobody heard, a receiver table whose dense numbering differs
from the staged path's, and `detect_all`.  Every case is held to the staged device path
(tests/postdetect_scene.py: staged), exactly."""
import io

import numpy as np
import pytest

import postdetect_scene as scene
from thrifty_amd import _native, block_data, kitchen_sink
from thrifty_amd.detect import Detector, DetectorSettings

pytestmark = pytest.mark.gpu

W = _native.POST_WORKGROUP


@pytest.fixture(scope="module")
def cols():
    return scene.columns(140)


def fused_is_staged(cols, st, **options):
    got = kitchen_sink.postdetect_columns(cols, st, **options)
    scene.assert_identical(got, scene.staged(cols, st, **options))
    return got


# 400 raw detections keep about 355: the gather and the dense-index kernels run a second workgroup
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, W - 1, W, W + 1, 400])
def test_sizes(cols, n):
    got = fused_is_staged(scene.head(cols, n), scene.settings())
    assert len(got["txid"]) == n
    if n == 400:
        assert got["counts"]["kept"] > W
    if n == 0:
        assert got["match_ptr"].tolist() == [0] and got["group_ptr"].tolist() == [0]
        assert got["pos"].shape == (0, 2) and all(v == 0 for v in got["counts"].values())


def test_nothing_kept(cols):
    stray = dict(cols, carrier_bin=np.full_like(cols["carrier_bin"], 5))
    got = fused_is_staged(stray, scene.settings())
    assert got["counts"]["kept"] == 0 and not got["keep"].any() and got["match_ptr"].tolist() == [0]


def test_all_misses():
    got = fused_is_staged(scene.columns(60, only=[0], extras=False), scene.settings())
    c = got["counts"]
    assert c["kept"] > 0 and c["matches"] == 0 and c["misses"] > 0 and c["tasks"] == 0 and got["group_ptr"].tolist() == [0]


def test_beacon_matches_only():
    got = fused_is_staged(scene.columns(60, tx_order=(0, 1)), scene.settings())
    c = got["counts"]
    assert c["matches"] > 0 and c["tasks"] == 0 and c["groups"] == 0 and got["group_ptr"].tolist() == [0]


def test_no_beacon_in_any_window():
    got = fused_is_staged(scene.columns(60, tx_order=(2, 3, 4)), scene.settings())
    c = got["counts"]
    assert c["tasks"] > 0 and c["failures"] == c["tasks"] and c["rows"] == 0 and c["groups"] == 0
    assert got["group_ptr"].tolist() == [0] and got["pos"].shape == (0, 2)


def test_every_group_underdetermined():
    got = fused_is_staged(scene.columns(80, only=[0, 1], extras=False), scene.settings())
    assert got["counts"]["groups"] > 0 and (got["status"] == _native.POS_UNDERDETERMINED).all()


def test_other_settings(cols):
    fused_is_staged(cols, scene.settings(), min_match=3)
    fused_is_staged(cols, scene.settings(), deg=1)
    fused_is_staged(cols, scene.settings(), min_match=1, deg=3)


def test_a_matched_receiver_that_the_table_lacks(cols):
    st = scene.settings()
    lacking = st._replace(rx_pos={rx: p for rx, p in st.rx_pos.items() if rx != 3})
    with pytest.raises(KeyError) as staged_err:
        scene.staged(cols, lacking)
    with pytest.raises(KeyError) as fused_err:
        kitchen_sink.postdetect_columns(cols, lacking)
    assert fused_err.value.args == staged_err.value.args == (3,)
    # the library's own words: THR_ERR_ARG naming the detection and its receiver
    native, _ = kitchen_sink._native_settings(lacking, 2, 2, (0.1, 0.1), 100, False)
    with pytest.raises(ValueError, match=r"thr_postdetect: detection \d+ is of receiver 3, which rx_ids lacks"):
        _native.postdetect(*[cols[name] for name in kitchen_sink.COLUMNS], settings=native)


def test_a_nan_timestamp_is_thr_match_s_refusal(cols):
    st = scene.settings()
    kept = scene.staged(cols, st)["kept_order"]
    bad = dict(cols, timestamp=cols["timestamp"].copy())
    bad["timestamp"][kept[40]] = np.nan
    with pytest.raises(ValueError) as staged_err:
        scene.staged(bad, st)
    with pytest.raises(ValueError) as fused_err:
        kitchen_sink.postdetect_columns(bad, st)
    assert str(fused_err.value) == str(staged_err.value)
    assert "thr_match: timestamps must be non-decreasing without NaN" in str(fused_err.value) and "is NaN" in str(fused_err.value)


def test_a_beacon_no_detection_names(cols):
    got = fused_is_staged(cols, scene.settings(extra_beacons=(7, -4)))
    assert got["counts"]["groups"] > 0


def test_an_unused_receiver_in_the_middle_of_the_table():
    """rx_pos holds receiver 3, which detected nothing: the fused numbering (0, 1, 3 -> 2, 5 -> 3, 7 -> 4)
    differs from the staged one (the receivers of the matches: 0, 1, 5 -> 2, 7 -> 3)."""
    ids = (0, 1, 5, 7)
    st = scene.settings(rx_ids=ids)
    rx_pos = dict(st.rx_pos)
    rx_pos[3] = np.array([40.0, -60.0])
    st = st._replace(rx_pos={rx: rx_pos[rx] for rx in (7, 0, 3, 5, 1)})
    got = fused_is_staged(scene.columns(100, rx_ids=ids), st)
    assert got["counts"]["groups"] > 0 and set(np.unique(got["tdoas"]["rx0"])) | set(np.unique(got["tdoas"]["rx1"])) == set(ids)


def test_detect_all_is_the_detector_runs_in_dict_order(golden, tmp_path):
    g = golden("small")
    tpl = g["template"]
    settings = DetectorSettings(int(g["block_len"]), int(g["history_len"]), int(np.asarray(tpl).shape[-1]),
                                tuple(g["carrier_thresh"]), tuple(int(v) for v in g["carrier_window"]), tpl,
                                tuple(g["corr_thresh"]))
    count = len(g["blocks"])
    cards = {}
    for rxid, picked in ((4, range(count)), (2, range(count - 1, -1, -1))):        # the second capture: blocks reversed
        cards[rxid] = str(tmp_path / ("rx%d.card" % rxid))
        with open(cards[rxid], "w") as out:
            out.write("# synthetic\n" + "".join(block_data.card_line(1000.0 + i, int(g["block_idx"][i]), g["blocks"][i])
                                                for i in picked))
    got = kitchen_sink.detect_all(cards, settings)
    want = []
    for rxid, name in cards.items():
        with open(name, "r") as capture:
            want += [r for hit, r in Detector(settings, block_data.card_reader(io.StringIO(capture.read())), rxid=rxid) if hit]
    assert [r.serialize() for r in got] == [r.serialize() for r in want]
    assert [r.rxid for r in got] == [4] * (len(got) // 2) + [2] * (len(got) // 2)
    assert len(got) == 2 * int(np.asarray(g["det"]).astype(bool).sum())
