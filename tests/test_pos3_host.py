"""Host side of `pos_3d` (no GPU): the NumPy restatement tests/pos3_ref.py against the fixtures of
tests/golden/make_golden_pos3.py under the rules the device is held to, the forms of the height, the records and the
.pos text of both modes, the argument parser, the inputs refused before the library is loaded, and the wiring of
`thr_pos3` into the header, the symbol list and the build."""
import io
import json
import os
import re

import numpy as np
import pytest

import pos3_golden
from pos3_ref import FREE_Z, KNOWN_HEIGHT, pos3_ref_groups
from thrifty_amd import _native, build, pos_3d, pos_est, tdoa_est

ROOT = pos3_golden.ROOT


def test_fixtures_are_what_the_issue_asks_for():
    shape = {"h_ring4": (4, False), "h_ring6": (6, False), "z_tall6": (6, True), "z_tall5": (5, True), "z_ring6": (6, True),
             "z_four": (4, True), "z_box": (6, True)}
    assert set(shape) == set(pos3_golden.SETS)
    for name, (n_rx, free) in shape.items():
        assert os.path.getsize(os.path.join(pos3_golden.GOLDEN, name + ".npz")) <= 64 * 1024
        g = pos3_golden.load(name)
        assert 0 < len(g["group_id"]) <= 64 and len(g["x_star"]) == len(g["x_ref"]) == len(g["solved"])
        assert g["rx_xyz"].shape == (n_rx, 3) and pos3_golden.free_z(g) == free and float(g["ref_err_max"]) >= 1e-9
        assert np.ptp(g["rx_xyz"][:, 2]) >= 30.0
        inner = np.flatnonzero(~g["solved"])
        if name == "z_box":
            assert len(inner) == 0 and 5 <= g["on_bound"].sum() <= len(g["solved"]) - 5
            np.testing.assert_array_equal(g["rx_xyz"], pos3_golden.load("z_tall6")["rx_xyz"])
            np.testing.assert_array_equal(g["x_star"][g["on_bound"], 2], g["z_range"][0])
        else:       # failures sit between solved groups
            assert len(inner) == 4 and inner.min() > 0 and inner.max() < len(g["solved"]) - 1 and not g["on_bound"].any()
            needed = 4 if free else 3
            ptr = g["group_ptr"].tolist()
            for k in inner.tolist():
                assert len(set(g["rx0"][ptr[k]:ptr[k + 1]].tolist()) | set(g["rx1"][ptr[k]:ptr[k + 1]].tolist())) == needed - 1
    assert set(np.diff(pos3_golden.load("z_four")["group_ptr"])[pos3_golden.load("z_four")["solved"]].tolist()) == {6}
    assert np.nanmax(pos3_golden.load("z_ring6")["cond"]) > 300 > np.nanmax(pos3_golden.load("z_tall5")["cond"])
    h4, h6 = pos3_golden.load("h_ring4"), pos3_golden.load("h_ring6")
    assert h4["group_h"].min() >= 0.0 and h4["group_h"].max() <= 3.0 and len(set(h4["group_h"].tolist())) == len(h4["group_h"])
    heights = {int(tx): h for tx, h in h6["tx_height"]}
    np.testing.assert_array_equal(h6["group_h"], [heights[int(tx)] for tx in h6["group_tx"]])


@pytest.mark.parametrize("name", pos3_golden.SETS)
def test_pos3_ref_meets_the_devices_rules(name):
    g = pos3_golden.load(name)
    free = pos3_golden.free_z(g)
    out = pos3_ref_groups(g["group_ptr"], pos3_golden.dense(g, g["rx0"]), pos3_golden.dense(g, g["rx1"]), g["tdoa"], g["snr"],
                          g["rx_xyz"], FREE_Z if free else KNOWN_HEIGHT, None if free else g["group_h"],
                          (0.1, 0.1, float(g["z0"]) if free else 0.0), tuple(g["z_range"]) if len(g["z_range"]) else None)
    keep = ~np.isin(out["status"], (_native.POS_UNDERDETERMINED, _native.POS_NONFINITE))
    np.testing.assert_array_equal(keep, g["solved"])
    np.testing.assert_array_equal(out["status"][keep], np.where(g["on_bound"][keep], _native.POS_AT_BOUND, _native.POS_OK))
    assert out["iters"].max() < 50
    pos3_golden.check_positions(g, g["group_id"][keep], g["group_timestamp"][keep], g["group_tx"][keep], out["pos"][keep],
                                out["dop"][keep], out["snr"][keep], out["hdop"][keep], out["vdop"][keep])


def test_the_forms_of_the_height():
    np.testing.assert_array_equal(pos_3d.group_heights(1.5, 3), [1.5, 1.5, 1.5])
    np.testing.assert_array_equal(pos_3d.group_heights(np.float32(2.0), 2), [2.0, 2.0])
    np.testing.assert_array_equal(pos_3d.group_heights({2: 0.5, 7: 3.0}, 3, group_tx=np.array([7, 2, 7])), [3.0, 0.5, 3.0])
    np.testing.assert_array_equal(pos_3d.group_heights([1.0, 2.0], 2), [1.0, 2.0])
    assert pos_3d.group_heights(1.0, 0).shape == (0,)
    for bad, text in (((np.nan, 2), "finite"), (([1.0, np.inf], 2), "finite"), (([1.0, 2.0], 3), "one value per group"),
                      (({2: 1.0}, 2, [2, 5]), "no height for tx 5"), (({2: 1.0}, 2), "needs group_tx"),
                      (({2: 1.0}, 2, [2]), "one transmitter per group")):
        with pytest.raises(ValueError, match=text):
            pos_3d.group_heights(*bad)


def test_the_start_height_and_its_refusals():
    table = np.array([[0.0, 0.0, 4.0], [100.0, 0.0, 31.0], [0.0, 100.0, 12.0], [90.0, 80.0, 20.0]])
    assert pos_3d.start_height(table) == (3.0, None)                    # 1 m below the lowest receiver
    z0, box = pos_3d.start_height(table, z_range=(-2.0, 10.0))
    assert z0 == 4.0 and box.tolist() == [-2.0, 10.0]                   # the middle of the range
    assert pos_3d.start_height(table, 7.5, (-2.0, 10.0))[0] == 7.5
    assert pos_3d.start_height(table, 31.0 + 10e3)[0] == 10031.0        # the reference's box on z
    for args, text in (((None, (5.0, 5.0)), "z_lo < z_hi"), ((None, (6.0, 5.0)), "z_lo < z_hi"), ((None, (0.0, np.inf)), "z_lo < z_hi"),
                       ((11.0, (-2.0, 10.0)), "outside the z range"), ((31.0 + 10e3 + 1.0, None), "outside the z range"),
                       ((np.nan, None), "outside the z range")):
        with pytest.raises(ValueError, match=text):
            pos_3d.start_height(table, *args)
    level = table.copy()
    level[:, 2] = 6.0
    assert pos_3d.start_height(level) == (5.0, None)
    with pytest.raises(ValueError, match="mirror plane"):
        pos_3d.start_height(level, 6.0)
    with pytest.raises(ValueError, match="mirror plane"):
        pos_3d.start_height(level, z_range=(2.0, 10.0))                 # the middle of the range is the plane


def test_bad_inputs_are_refused_before_the_library_is_loaded(monkeypatch):
    def no_library():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_native, "load_library", no_library)
    tall = {0: np.array([0.0, 0.0, 4.0]), 1: np.array([100.0, 0.0, 31.0]), 2: np.array([0.0, 100.0, 12.0]), 5: np.array([90.0, 80.0, 20.0])}
    args = ([0, 4], [0, 0, 1, 2], [1, 2, 2, 5], [1e-9, 2e-9, 3e-9, 4e-9], [1.0, 1.0, 1.0, 1.0])
    for rx_pos in ({k: v[:2] for k, v in tall.items()}, {k: v[:1] for k, v in list(tall.items())[:2]},
                   {0: tall[0], 1: tall[1], 2: tall[2][:2], 5: tall[5]}):
        with pytest.raises(ValueError, match="three coordinates.*pos_est"):
            pos_3d.pos3_columns(*args, rx_pos, height=1.0)
    with pytest.raises(ValueError, match="no default mode"):
        pos_3d.pos3_columns(*args, tall)
    with pytest.raises(ValueError, match="no default mode"):
        pos_3d.pos3_columns(*args, tall, height=1.0, free_z=True)
    with pytest.raises(ValueError, match="z_lo < z_hi"):
        pos_3d.pos3_columns(*args, tall, free_z=True, z_range=(3.0, 3.0))
    with pytest.raises(ValueError, match="outside the z range"):
        pos_3d.pos3_columns(*args, tall, free_z=True, z0=-1.0, z_range=(0.0, 3.0))
    with pytest.raises(ValueError, match="z0 must be finite"):
        pos_3d.pos3_columns(*args, tall, free_z=True, z0=np.inf)
    with pytest.raises(ValueError, match="mirror plane"):
        pos_3d.pos3_columns(*args, {k: np.append(v[:2], 7.0) for k, v in tall.items()}, free_z=True, z0=7.0)
    with pytest.raises(ValueError, match="belong to free_z"):
        pos_3d.pos3_columns(*args, tall, height=1.0, z0=0.0)
    for height in (np.nan, [np.inf], {3: np.nan}):
        with pytest.raises(ValueError, match="finite"):
            pos_3d.pos3_columns(*args, tall, height=height, group_tx=[3])
    with pytest.raises(ValueError, match="no height for tx 4"):
        pos_3d.pos3_columns(*args, tall, height={3: 1.0}, group_tx=[4])
    with pytest.raises(KeyError):
        pos_3d.pos3_columns(*args, {k: v for k, v in tall.items() if k != 5}, height=1.0)
    with pytest.raises(ValueError, match="group_ptr"):
        pos_3d.pos3_columns([0, 3], *args[1:], tall, height=1.0)
    with pytest.raises(ValueError, match="x0"):
        pos_3d.pos3_columns(*args, tall, height=1.0, x0=(0.1, np.nan))
    many = {k: np.array([float(k), 1.0, 2.0 + k]) for k in range(65)}
    with pytest.raises(ValueError, match="at most 64 receivers, not 65"):
        pos_3d.pos3_columns(*args, many, free_z=True)
    with pytest.raises(ValueError, match="not finite"):
        pos_3d.pos3_columns(*args, {**tall, 5: np.array([1.0, np.nan, 2.0])}, height=1.0)
    rows = np.zeros(4, dtype=tdoa_est.TDOA_DTYPE)
    rows["rx0"], rows["rx1"] = args[1], args[2]
    group = tdoa_est.TdoaGroup(1, 2.0, 3, rows)
    with pytest.raises(ValueError, match="three coordinates"):
        pos_3d.solve([group], {k: v[:2] for k, v in tall.items()}, height=1.0)
    with pytest.raises(ValueError, match="no height for tx 3"):
        pos_3d.solve([group], tall, height={2: 1.0})
    with pytest.raises(KeyError):
        pos_3d.solve([group], {k: v for k, v in tall.items() if k != 5}, free_z=True)
    with pytest.raises(ValueError, match="no default mode"):
        pos_3d.solve([group], tall)


def fake_columns(g):
    """What `_native.pos3` would return if the device gave SciPy's answers."""
    n = len(g["solved"])
    out = {"pos": np.where(g["solved"][:, None], g["x_ref"], 0.0), "dop": np.where(g["solved"], g["dop_ref"], -1.0),
           "hdop": np.full(n, 1.5), "vdop": np.full(n, 2.5), "rms": np.full(n, 0.25), "snr": np.where(g["solved"], g["snr_ref"], 0.0),
           "status": np.where(g["solved"], _native.POS_OK, _native.POS_UNDERDETERMINED).astype(np.int32),
           "iters": np.full(n, 7, dtype=np.int32)}
    out["status"][np.flatnonzero(~g["solved"])[-1:]] = _native.POS_NONFINITE
    return out


@pytest.mark.parametrize("name", ["h_ring6", "z_tall5"])
def test_records_and_pos_text_of_both_modes(name, monkeypatch, capsys, tmp_path):
    g = pos3_golden.load(name)
    seen = {}

    def pos3(ptr, rx0, rx1, tdoa, snr, table, mode, heights, x0, z_range, max_iter, device_id):
        seen.update(mode=mode, heights=heights, x0=x0, z_range=z_range, rx0=rx0, table=table)
        return fake_columns(g)
    monkeypatch.setattr(_native, "pos3", pos3)
    free = pos3_golden.free_z(g)
    details = {}
    res = pos_3d.solve(pos3_golden.groups(g), pos3_golden.rx_pos(g), details=details, **pos3_golden.mode_args(g, by_tx=True))
    lost = g["group_id"][~g["solved"]]
    assert capsys.readouterr().out.splitlines() == ["Failed to estimate group #%d: Underdetermined" % i for i in lost[:-1]] + \
        ["Failed to estimate group #%d: Nonfinite" % lost[-1]]
    np.testing.assert_array_equal(seen["table"], g["rx_xyz"])
    np.testing.assert_array_equal(seen["rx0"], pos3_golden.dense(g, g["rx0"]))
    if free:
        assert seen["mode"] == _native.POS3_FREE_Z and seen["heights"] is None and seen["z_range"] is None
        assert seen["x0"] == (0.1, 0.1, float(g["rx_xyz"][:, 2].min()) - 1.0) and seen["x0"][2] == float(g["z0"])
        assert res.dtype.names == ("group_id", "timestamp", "tx", "dop", "snr", "x", "y", "z")
        np.testing.assert_array_equal(res["z"], g["x_ref"][g["solved"], 2])
    else:
        assert seen["mode"] == _native.POS3_KNOWN_HEIGHT and seen["x0"] == (0.1, 0.1, 0.0)
        np.testing.assert_array_equal(seen["heights"], g["group_h"])        # the {tx: height} dict, looked up per group
        assert res.dtype.names == ("group_id", "timestamp", "tx", "dop", "snr", "x", "y")      # `thrifty pos`' own 2-D record
    assert res.dtype == np.dtype({"names": pos_est.POSITION_INFO_DTYPE["names"][:len(res.dtype.names)],
                                  "formats": pos_est.POSITION_INFO_DTYPE["formats"][:len(res.dtype.names)]})
    ok = g["solved"]
    np.testing.assert_array_equal(res["group_id"], g["group_id"][ok])
    np.testing.assert_array_equal(res["timestamp"], g["group_timestamp"][ok])
    np.testing.assert_array_equal(res["tx"], g["group_tx"][ok])
    np.testing.assert_array_equal(res["x"], g["x_ref"][ok, 0])
    np.testing.assert_array_equal(res["y"], g["x_ref"][ok, 1])
    np.testing.assert_array_equal(res["dop"], g["dop_ref"][ok])
    assert set(details) == set(_native.POS3_OUTPUTS) | {"group_id"} and len(details["hdop"]) == len(ok)
    text = io.StringIO()
    pos_est.save_positions(text, res)
    lines = text.getvalue().splitlines()
    assert len(lines) == len(res) and all(len(line.split()) == (8 if free else 7) for line in lines)
    first = res[0]
    assert lines[0] == " ".join(["%d %.6f %d" % (first["group_id"], first["timestamp"], first["tx"])] +
                                [repr(float(first[key])) for key in res.dtype.names[3:]])
    path = tmp_path / "data.pos"
    pos_est.save_positions(str(path), res)
    back = pos_est.load_positions(str(path))
    assert back.dtype == res.dtype and back.tolist() == res.tolist()


def test_the_argument_parser():
    parser = pos_3d._parser()
    assert parser.get_default("tdoa") == "data.tdoa" and parser.get_default("output") == "data.pos"
    assert parser.get_default("rx_pos") == "pos-rx.cfg"
    flags = {s for a in parser._actions for s in a.option_strings}
    assert flags >= {"-o", "--output", "-r", "--rx-coordinates", "--height", "--height-tx", "--free-z", "--z0", "--z-range", "--npz"}
    parse = lambda *words: parser.parse_args(["-r", os.devnull, "-o", os.devnull, os.devnull] + list(words))     # noqa: E731
    for words in ((), ("--height", "1.0", "--free-z")):      # no default mode, and not both
        with pytest.raises(SystemExit):
            parse(*words)
    capsys_free = parse("--free-z", "--z0", "-2.5", "--z-range", "-10", "40", "--npz", "more.npz")
    assert capsys_free.free_z and capsys_free.height is None and capsys_free.z0 == -2.5 and capsys_free.z_range == [-10.0, 40.0]
    assert capsys_free.npz == "more.npz"
    known = parse("--height", "1.2", "--height-tx", "3=0.5", "4=2", "--height-tx", "9=7.25")
    assert known.height == 1.2 and not known.free_z and known.z0 is None and known.z_range is None
    assert dict(pair for given in known.height_tx for pair in given) == {3: 0.5, 4: 2.0, 9: 7.25}
    with pytest.raises(SystemExit):
        parse("--height", "1.2", "--height-tx", "3:0.5")
    for args in (capsys_free, known):
        for stream in (args.tdoa, args.rx_pos, args.output):
            stream.close()
    for words in (("--free-z", "--height-tx", "3=1"), ("--height", "1", "--z0", "2"), ("--height", "1", "--z-range", "0", "2")):
        with pytest.raises(SystemExit):
            pos_3d._main(["-r", os.devnull, "-o", os.devnull, os.devnull] + list(words))


def test_thr_pos3_is_declared_listed_and_built():
    header = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
    assert re.search(r"\bint thr_pos3\(int device_id, size_t n_groups, const int64_t\* group_ptr,", header)
    assert re.search(r"\bint thr_debug_pos3_times\(double\* ms_out", header)
    assert "#define THR_ABI_VERSION 11" in header and _native.ABI_VERSION == 11
    listed = header[header.index("within 11, a pure addition"):header.index("#define THR_ABI_VERSION")]
    assert re.search(r"\+ thr_pos3 / thr_debug_pos3_times", listed)
    assert "#define THR_POS3_KNOWN_HEIGHT %d" % _native.POS3_KNOWN_HEIGHT in header
    assert "#define THR_POS3_FREE_Z %d" % _native.POS3_FREE_Z in header
    assert {"thr_pos3", "thr_debug_pos3_times"} <= set(_native.EXPORTS) and callable(_native.pos3) and callable(_native.pos3_times)
    assert "pos3.hip" in build.SOURCES and "pos3_lm.hpp" in build.HEADERS
    assert set(build.UNPROFILED_POS3) == {"pos3.hip", "pos3_lm.hpp"}
    assert "-ffp-contract=off" in build.PER_FILE_FLAGS["pos3.hip"]
    source = open(os.path.join(build.CSRC, "pos3.hip")).read()
    shared = open(os.path.join(build.CSRC, "pos3_lm.hpp")).read()
    for text in (source, shared):
        assert "#pragma clang fp contract(off)" in text and not re.search(r"atomic[A-Z_(]", text)
    assert '#include "pos3_lm.hpp"' in source and '#include "pos_lm.hpp"' in shared
    assert "k_pos_h" in source and "k_pos_z" in source
    assert "sqrt((ax * ax + ay * ay) + az * az)" in shared
    assert int(re.search(r"constexpr int kBlock = (\d+);", source).group(1)) // 8 == _native.POS3_GROUPS_PER_WORKGROUP
    assert int(re.search(r"constexpr int kRegRows = (\d+);", source).group(1)) == _native.POS3_REGISTER_ROWS
    assert int(re.search(r"constexpr int kMaxReceivers = (\d+);", source).group(1)) == _native.POS_MAX_RECEIVERS


def test_the_built_library_exports_thr_pos3():
    assert os.path.exists(_native.LIB_PATH), "the library is not built: python -m thrifty_amd.build"
    lib = _native.load_library()
    assert lib.thr_pos3 and lib.thr_debug_pos3_times


def test_csrc_hash_does_not_see_the_new_files(monkeypatch):
    with_pos3 = build.csrc_hash()
    recorded = json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json")))
    hashes = {workload["_source"]["csrc_sha16"] for workload in recorded.values()}
    assert hashes == {with_pos3}                     # the recorded hash still holds
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "pos3.hip"])
    monkeypatch.setattr(build, "HEADERS", [h for h in build.HEADERS if h != "pos3_lm.hpp"])
    assert build.csrc_hash() == with_pos3            # unchanged by this addition
    monkeypatch.undo()
    monkeypatch.setattr(build, "UNPROFILED_POS3", ())
    assert build.csrc_hash() != with_pos3
