"""`thr_track` at the smallest shapes at which its scans can go wrong (tests/track_scenes.py: seams()): row counts
around the tile of 256, tracks that meet inside a tile and at its edges, hundreds of one-row tracks, invalid rows at
a track's start, at a tile's last and first position and across a whole tile, a row that the gate rejects at a tile's
last and first position, equal timestamps, epoch timestamps with
millisecond steps -- against tests/track_ref.py within the tolerance recorded per scene, integers exact -- and the
equalities of bytes the header promises."""
import numpy as np
import pytest

import track_check
import track_scenes
from thrifty_amd import _native

pytestmark = pytest.mark.gpu

SCENES = sorted(track_scenes.seams())


@pytest.mark.parametrize("name", SCENES)
def test_a_seam_against_the_reference(name):
    s, ref = track_check.seam(name)
    track_check.assert_margin(ref)
    counts, out = track_check.device(s)
    track_check.compare(name, counts, out, ref)


def test_what_the_scenes_hold():
    seams = track_check.seams()
    assert [len(seams["single_%d" % n]["tx"]) for n in (0, 1, 2, 255, 256, 257, 512, 513, 769)] == [0, 1, 2, 255, 256, 257, 512, 513, 769]
    for name, first in (("meet_inside", 100), ("meet_at_last", 255), ("meet_at_first", 256)):
        assert track_check.seam(name)[1]["track_ptr"].tolist() == [0, first, first + 300]
    assert track_check.seam("singles_300")[1]["counts"]["tracks"] == 300
    assert track_check.seam("long_between")[1]["track_ptr"].tolist() == [0, 1, 601, 602]
    s, ref = track_check.seam("invalid_first3")
    assert not ref["tracked"][ref["order"][:3]].any() and ref["tracked"][ref["order"][3:]].all()
    s, ref = track_check.seam("no_valid_row")
    assert np.isnan(ref["track_stats"][1, 4:]).all() and ref["track_stats"][1, :4].tolist() == [30, 0, 0, 0]
    for name, at in (("invalid_255", [255]), ("invalid_256", [256]), ("invalid_tile", list(range(200, 521)))):
        s, ref = track_check.seam(name)
        assert np.flatnonzero(s["valid"][ref["order"]] == 0).tolist() == at
    for name, at in (("reject_255", 255), ("reject_256", 256)):      # a row the gate rejects: valid, not used, its nis reported
        s, ref = track_check.seam(name)
        assert len(s["tx"]) == 600 and s["valid"].all() and ref["counts"]["tracks"] == 1
        assert np.flatnonzero(s["outlier"][ref["order"]]).tolist() == [at]
        row = int(ref["order"][at])
        assert ref["used"][row] == 0 and ref["counts"]["rounds"] >= 2 and ref["counts"]["converged"] == 1
        assert np.isfinite(ref["nis"][row]) and ref["nis"][row] > track_check.track_ref.GATE_999
    s = seams["equal_times"]
    assert all(len(set(s["timestamp"][s["tx"] == tx])) == 1 for tx in set(s["tx"].tolist()))
    s = seams["epoch_ms"]
    assert s["timestamp"].min() >= 1.5e9 and np.allclose(np.diff(np.sort(s["timestamp"][s["tx"] == 3])), 1e-3, atol=1e-6)


@pytest.mark.parametrize("name", ["single_513", "meet_at_last", "no_valid_row"])
def test_a_repeated_call_returns_the_same_bytes(name):
    s = track_check.seams()[name]
    track_check.same_bytes(track_check.device(s), track_check.device(s))


@pytest.mark.parametrize("name", ["single_769", "long_between", "invalid_tile"])
def test_shuffled_rows_return_the_same_bytes_per_row(name):
    s = track_check.seams()[name]
    assert all(len(set(s["timestamp"][s["tx"] == tx])) == np.count_nonzero(s["tx"] == tx) for tx in set(s["tx"].tolist()))
    perm = np.random.default_rng(1).permutation(len(s["tx"]))
    shuffled = {key: (value[perm] if isinstance(value, np.ndarray) else value) for key, value in s.items()}
    (ca, a), (cb, b) = track_check.device(s), track_check.device(shuffled)
    assert ca == cb
    for key in ("used", "nis", "filt", "filt_var", "smooth", "smooth_var"):
        assert a[key][perm].tobytes() == b[key].tobytes(), key
    for key in ("track_tx", "track_ptr", "track_stats", "track_flags"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert np.array_equal(perm[b["order"]], a["order"])


def test_a_track_alone_and_with_other_transmitters_after_it_returns_the_same_bytes():
    alone = track_scenes.scene(401, rows=700, outliers=0.02, first_tx=2)
    others = track_scenes.scene(402, tracks=3, rows=(90, 400, 1), first_tx=10)      # every tx above 2: sorted after it
    both = {key: np.concatenate([others[key], alone[key]]) for key in track_scenes.COLUMNS}
    both["q"], both["v0"] = alone["q"], alone["v0"]
    (ca, a), (cb, b) = track_check.device(alone), track_check.device(both)
    assert ca["tracks"] == 1 and cb["tracks"] == 4 and cb["rounds"] >= ca["rounds"]
    n_other = len(others["tx"])
    for key in ("used", "nis", "filt", "filt_var", "smooth", "smooth_var"):
        assert a[key].tobytes() == b[key][n_other:].tobytes(), key
    assert a["track_stats"].tobytes() == b["track_stats"][:1].tobytes() and a["track_flags"][0] == b["track_flags"][0]
    assert np.array_equal(b["order"][:700] - n_other, a["order"])
