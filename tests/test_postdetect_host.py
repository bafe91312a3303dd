"""Host side of the post-detect chain: the additions are named where the siblings are, every argument
check of `thr_postdetect` answers THR_ERR_ARG before a device is looked for (this file runs without one),
an empty input is a result without a device, `kitchen_sink.postdetect` chains replaced stages like the
reference, `patch_module`, and the `thrifty_amd.cli` front end."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_not_transcribed
from thrifty_amd import _native, build, cli, identify, kitchen_sink, matchmaker, pos_est, tdoa_est

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_additions_are_named_and_the_abi_stays_11():
    header = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
    assert re.search(r"#define THR_ABI_VERSION 11\b", header) and _native.ABI_VERSION == 11
    for name in ("thr_postdetect", "thr_post_fetch", "thr_post_free", "thr_debug_post_times"):
        assert re.search(r"\b%s\(" % name, header) and name in _native.EXPORTS
    assert "postdetect.hip" in build.SOURCES and "post_stages.hpp" in build.HEADERS
    assert set(build.UNPROFILED_POST) == {"postdetect.hip", "post_stages.hpp"}
    assert build.PER_FILE_FLAGS["tdoa.hip"] == ["-ffp-contract=off"] == build.PER_FILE_FLAGS["pos.hip"]
    # THR_POST_* and _native.POST_OUTPUTS agree
    defined = dict((name.lower(), int(value)) for name, value in re.findall(r"#define THR_POST_([A-Z_]+) (\d+)", header))
    assert defined.pop("n_outputs") == len(_native.POST_OUTPUTS) == len(defined)
    renamed = {"group_timestamp": "group_ts"}
    assert {renamed.get(name, name): spec[0] for name, spec in _native.POST_OUTPUTS.items()} == defined
    # the struct layouts: field names in the header's order
    for struct, kind in (("thr_post_settings", _native.ThrPostSettings), ("thr_post_counts", _native.ThrPostCounts)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
        assert names == [f[0] for f in kind._fields_], struct


def valid(**changes):
    spec = dict(freq_ranges=[(0, 0, 1.0, 2.0)], match_window=0.2, min_match=2, rx_ids=[0, 1, 2],
                rx_coords=[[0.0, 0.0], [100.0, 0.0], [0.0, 100.0]], first_two_rx=(0, 1), beacon_ids=[0, 1],
                dist=np.ones((3, 2)), tdoa_window=8.0, sample_rate=2.4e6, deg=2, x0=(0.1, 0.1), max_iter=100)
    spec.update(changes)
    return _native.post_settings(**spec)


def call(settings, n=4, null_column=None, null_settings=False, null_result=False):
    lib = _native.load_library()
    st, _alive = settings
    cols = [np.zeros(n, dtype=kind) for kind in (np.int32, np.int32, np.float64, np.int32, np.float64, np.float64,
                                                 np.float64, np.float64)]
    ptrs = [col.ctypes.data for col in cols]
    if null_column is not None:
        ptrs[null_column] = None
    handle, counts = C.c_void_p(), _native.ThrPostCounts()
    rc = lib.thr_postdetect(0, n, *ptrs, None if null_settings else C.byref(st), None if null_result else C.byref(handle),
                            C.byref(counts))
    assert handle.value is None or rc == 0
    if handle.value is not None:
        lib.thr_post_free(handle)
    return rc, lib.thr_last_error().decode()


BAD = {
    "rx_ids descending": dict(rx_ids=[0, 2, 1]),
    "rx_ids repeated": dict(rx_ids=[0, 1, 1]),
    "65 receivers": dict(rx_ids=list(range(65)), rx_coords=np.zeros((65, 2)), dist=np.ones((65, 2))),
    "beacon_ids descending": dict(beacon_ids=[1, 0]),
    "beacon_ids repeated": dict(beacon_ids=[1, 1]),
    "three dimensions": dict(rx_coords=np.zeros((3, 3))),
    "deg 0": dict(deg=0),
    "deg 4": dict(deg=4),
    "a NaN coordinate": dict(rx_coords=[[0.0, 0.0], [np.nan, 0.0], [0.0, 100.0]]),
    "an infinite coordinate": dict(rx_coords=[[0.0, 0.0], [100.0, 0.0], [0.0, np.inf]]),
    "a NaN x0": dict(x0=(np.nan, 0.1)),
    "an infinite x0": dict(x0=(0.1, -np.inf)),
    "a negative max_iter": dict(max_iter=-1),
    "1-D with three receivers": dict(rx_coords=[[0.0], [100.0], [200.0]]),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_argument_checks_answer_before_a_device_is_looked_for(what):
    rc, said = call(valid(**BAD[what]))
    assert rc == _native.ERR_ARG and said.startswith("thr_postdetect:"), (rc, said)


def test_null_pointers_are_refused():
    for kwargs in (dict(null_settings=True), dict(null_result=True)) + tuple(dict(null_column=k) for k in range(8)):
        rc, said = call(valid(), **kwargs)
        assert rc == _native.ERR_ARG and "null" in said, (kwargs, rc, said)
    for field in ("rx_ids", "rx_coords", "beacon_ids", "dist", "map"):
        settings = valid()
        setattr(settings[0], field, None)
        rc, said = call(settings)
        assert rc == _native.ERR_ARG and said.startswith("thr_postdetect:"), (field, rc, said)
    rc, said = call(valid(first_two_rx=(0, 2), rx_ids=[0, 1], rx_coords=[[0.0], [9.0]], dist=np.ones((2, 2))))
    assert rc == _native.ERR_ARG and "first_two_rx" in said


def test_an_empty_input_is_a_result_without_a_device():
    empty = [np.zeros(0)] * 8
    counts, out = _native.postdetect(*empty, settings=valid())
    assert set(counts) == set(_native.POST_COUNTS) and all(v == 0 for v in counts.values())
    assert out["match_ptr"].tolist() == [0] and out["group_ptr"].tolist() == [0]
    assert out["pos"].shape == (0, 2) and out["collisions"].shape == (0, 2) and out["row_val"].shape == (0, 3)
    assert all(len(out[name]) == 0 for name in out if name not in ("match_ptr", "group_ptr"))
    assert _native.post_times() == (0.0,) * 6
    settings = kitchen_sink.PostdetectSettings(None, 0.2, 8.0, {0: (0.0, 0.0), 1: (5.0, 0.0), 2: (0.0, 5.0)}, {4: (1.0, 1.0)}, 2.4e6)
    res = kitchen_sink.postdetect_columns({name: np.zeros(0) for name in kitchen_sink.COLUMNS}, settings)
    assert len(res["tdoas"]) == 0 and res["tdoas"].dtype == np.dtype(tdoa_est.TDOA_DTYPE) and res["counts"]["kept"] == 0
    done = kitchen_sink.postdetect([], settings)
    assert done.toads == [] and done.matches == [] and done.tdoas == [] and len(done.pos) == 0


def test_the_reference_s_names():
    assert kitchen_sink.PostdetectSettings._fields == ("tx_freqs", "match_window", "tdoa_est_window", "rx_pos",
                                                       "beacon_pos", "sample_rate")
    assert kitchen_sink.PostdetectResult._fields == ("toads", "matches", "tdoas", "pos")
    import inspect
    spec = inspect.signature(kitchen_sink.postdetect)
    assert list(spec.parameters) == ["toad", "settings", "integrator", "matcher", "tdoa_estimator", "pos_estimator"]
    defaults = [spec.parameters[name].default for name in list(spec.parameters)[2:]]
    assert defaults == [identify.integrate, matchmaker.match_toads, tdoa_est.estimate_tdoas, pos_est.solve]
    assert list(inspect.signature(kitchen_sink.detect_all).parameters) == ["cards", "settings", "detector"]


def test_replaced_stages_are_chained_like_the_reference():
    calls = []
    settings = kitchen_sink.PostdetectSettings(tx_freqs={"map": 1}, match_window=0.3, tdoa_est_window=5.0,
                                               rx_pos={0: (1.0, 2.0), 1: [3.0, 4.0]}, beacon_pos={9: (5.0, 6.0)},
                                               sample_rate=2e6)

    def integrator(toad, freqmap=None):
        calls.append(("integrate", toad, freqmap))
        return "TOADS"

    def matcher(toads, window):
        calls.append(("match", toads, window))
        return "MATCHES", "MISSES", "COLLISIONS"

    def tdoa_estimator(**kwargs):
        calls.append(("tdoa", kwargs))
        return "TDOAS", "FAILURES"

    def pos_estimator(tdoas, rx_pos):
        calls.append(("pos", tdoas, rx_pos))
        return "POS"

    result = kitchen_sink.postdetect("RAW", settings, integrator=integrator, matcher=matcher,
                                     tdoa_estimator=tdoa_estimator, pos_estimator=pos_estimator)
    assert result == kitchen_sink.PostdetectResult(toads="TOADS", matches="MATCHES", tdoas="TDOAS", pos="POS")
    assert [c[0] for c in calls] == ["integrate", "match", "tdoa", "pos"]
    assert calls[0][1:] == ("RAW", {"map": 1}) and calls[1][1:] == ("TOADS", 0.3)
    kwargs = calls[2][1]
    assert sorted(kwargs) == ["beacon_pos", "detections", "matches", "rx_pos", "sample_rate", "window_size"]
    assert kwargs["detections"] == "TOADS" and kwargs["matches"] == "MATCHES" and kwargs["window_size"] == 5.0
    assert kwargs["sample_rate"] == 2e6
    for table, want in ((kwargs["rx_pos"], settings.rx_pos), (kwargs["beacon_pos"], settings.beacon_pos), (calls[3][2], settings.rx_pos)):
        assert list(table) == list(want) and all(isinstance(v, np.ndarray) and v.tolist() == list(want[k]) for k, v in table.items())
    assert calls[3][1] == "TDOAS"
    # one replaced stage is enough to leave the fused call (no device is touched here)
    kitchen_sink.postdetect("RAW", settings, integrator=integrator, matcher=matcher, tdoa_estimator=tdoa_estimator,
                            pos_estimator=kitchen_sink.patch_module(pos_estimator))


def test_patch_module():
    seen = []

    def module(a, b=1, c=2):
        seen.append((a, b, c))
        return a + b + c

    patched = kitchen_sink.patch_module(module, c=10)
    assert patched(1) == 12 and patched(1, b=5) == 16 and patched(1, 2, c=3) == 13       # the override wins
    assert seen == [(1, 1, 10), (1, 5, 10), (1, 2, 10)]
    assert kitchen_sink.patch_module(module)(1) == 4


def test_the_front_end_maps_every_command(capsys):
    wanted = {"detect", "identify", "match", "tdoa", "pos", "template_generate", "template_extract", "locate"}
    assert set(cli.COMMANDS) == wanted
    for command in wanted:
        assert callable(cli.resolve(command))
    assert cli.resolve("locate") is kitchen_sink._main and cli.resolve("match") is matchmaker._main
    assert cli.resolve("tdoa") is tdoa_est._main and cli.resolve("pos") is pos_est._main and cli.resolve("identify") is identify._main
    assert cli.main(["help"]) == 0
    text = capsys.readouterr().out
    assert all(command in text for command in wanted)
    assert cli.main([]) == 1
    capsys.readouterr()
    assert cli.main(["frobnicate"]) == 1
    assert "frobnicate" in capsys.readouterr().err
    for command in ("capture", "scope", "analyze_toads", "analyze_detect", "analyze_beacon", "analyze_tdoa"):
        assert cli.main([command, "--anything"]) == 1
        said = capsys.readouterr().err
        assert command in said and "not part of this port" in said and said.count("\n") == 1
    for command in sorted(wanted):
        with pytest.raises(SystemExit) as done:
            cli.main(["help", command])
        assert done.value.code == 0
        assert "usage:" in capsys.readouterr().out


@pytest.mark.skipif(not os.path.isdir(os.path.join(test_not_transcribed.REF, "thrifty")), reason="no reference checkout here")
@pytest.mark.parametrize("name", ["kitchen_sink.py", "cli.py"])
def test_kitchen_sink_and_cli_are_not_transcribed(name):
    """tests/test_not_transcribed.py's measure on the two new mirrors alone (the whole-package run is that file's)."""
    import difflib
    t = test_not_transcribed
    ours, theirs = t._parse(os.path.join(ROOT, "thrifty_amd", name)), t._parse(os.path.join(t.REF, "thrifty", name))
    mine = [(fn.name, t._dump(fn)) for fn in t._functions(ours) if t._statements(fn) > t.MIN_STATEMENTS]
    assert mine and theirs is not None
    worst = max((difflib.SequenceMatcher(None, d, t._dump(ref), autojunk=False).ratio(), fn, ref.name)
                for fn, d in mine for ref in t._functions(theirs))
    assert worst[0] < t.LIMIT, worst
