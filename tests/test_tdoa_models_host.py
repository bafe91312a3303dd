"""Host side of the weighted, nearest and linear TDOA models (no GPU): the sequential statement
tests/tdoa_models_ref.py against the fixtures the reference's own builders produced
(tests/golden/make_golden_tdoa_models.py) -- nearest and linear to the last bit --, the selector objects
that stand where the reference has model builders, the TypeErrors of `estimate_tdoas`, the command
lines, and the wiring of `thr_tdoa_model` into the header, the symbol list and the settings struct."""
import os
import re

import numpy as np
import pytest

import tdoa_golden
import tdoa_models_golden
from tdoa_models_ref import nearest_position, tdoa_models_ref, weights_of
from thrifty_amd import _native, kitchen_sink, tdoa_est

ROOT = tdoa_golden.ROOT
_ref = {}


def ref_of(name):
    """tdoa_models_ref's answer for a fixture, computed once."""
    if name not in _ref:
        g = tdoa_models_golden.load(name)
        rx_pos, beacon_pos = tdoa_golden.positions(g)
        _ref[name] = tdoa_models_ref(g["rxid"], g["txid"], g["timestamp"], g["soa"], g["energy"], g["noise"],
                                     tdoa_golden.matches(g), float(g["window"]), beacon_pos, rx_pos,
                                     float(g["sample_rate"]), g["model"], int(g["deg"]))
    return _ref[name]


def test_fixtures_are_what_the_issue_asks_for():
    seen = {model: set() for model in tdoa_models_golden.MODELS}
    for name in tdoa_models_golden.SETS:
        assert os.path.getsize(os.path.join(tdoa_models_golden.GOLDEN, name + ".npz")) < 100 * 1024
        g = tdoa_models_golden.load(name)
        scene = tdoa_golden.load(name[:name.index("_" + g["model"])])
        for key in ("rxid", "txid", "timestamp", "soa", "energy", "noise", "match_ptr", "match_idx", "rx_xyz",
                    "beacon_xyz", "n_window", "n_kept", "uncovered_matches"):
            np.testing.assert_array_equal(g[key], scene[key], err_msg=key)       # the polynomial's scenes, its front
        assert len(g["n_window"]) == len(g["tdoa"]) + len(g["failures"]) and np.all(np.isfinite(g["tdoa"]))
        assert int(g["deg"]) == (1 if name.endswith("_deg1") else 2)
        if g["model"] == "weighted_poly":
            assert 0 < float(g["ref_err_max"]) < 1e-9 and len(g["exact_tdoa"]) == len(g["tdoa"]) > 0
        seen[g["model"]] |= {"row"} if len(g["tdoa"]) else set()
        seen[g["model"]] |= {"failure"} if len(g["failures"]) else set()
        # what the models went through, read off the statement's picks (which the fixtures' bits confirm below)
        out = ref_of(name)
        failed = set(out["failures"])
        tasks = [pair for m in tdoa_golden.matches(g) if g["txid"][m[0]] not in g["beacon_ids"]
                 for pair in tdoa_models_golden_pairs(g, m)]
        for pair, (a, b), kept in zip(tasks, out["picks"], out["n_kept"]):
            if g["model"] == "nearest" and a >= 0:
                seen["nearest"] |= {"n_kept == 1"} if kept == 1 else set()
                seen["nearest"] |= {"the last pair"} if a == kept - 1 else set()
            if g["model"] == "linear" and b >= 0:
                seen["linear"] |= {"low < 0"} if a < 0 and pair in failed else set()
                seen["linear"] |= {"skipped"} if 0 <= a < b - 1 else set()
                seen["linear"] |= {"the last pair"} if b == kept - 1 else set()
    assert seen["weighted_poly"] == {"row", "failure"}
    assert seen["nearest"] == {"row", "failure", "n_kept == 1", "the last pair"}
    assert seen["linear"] == {"row", "failure", "low < 0", "skipped", "the last pair"}


def tdoa_models_golden_pairs(g, match):
    rx = g["rxid"]
    return [(a, b) if rx[a] < rx[b] else (b, a) for i, a in enumerate(match) for b in match[i + 1:]]


@pytest.mark.parametrize("name", tdoa_models_golden.SETS)
def test_the_statement_equals_the_reference(name):
    g, out = tdoa_models_golden.load(name), ref_of(name)
    rows = [row for group in out["groups"] for row in group[3]]
    cols = {key: np.array([row[k] for row in rows]) for k, key in
            enumerate(("rx0", "rx1", "tdoa", "snr", "model_quality", "det0", "det1"))}
    tdoa_models_golden.check_against_fixture(
        g, [grp[0] for grp in out["groups"]], [grp[1] for grp in out["groups"]], [grp[2] for grp in out["groups"]],
        np.cumsum([0] + [len(grp[3]) for grp in out["groups"]]), cols, out["failures"], out["n_window"], out["n_kept"])
    assert len(out["picks"]) == len(out["n_kept"])
    if g["model"] == "weighted_poly":
        assert set(out["picks"]) == {(-1, -1)}
        assert np.isfinite(out["cond"]).sum() >= len(rows)


def test_nearest_position_and_weights():
    stamps = [5.0, 10.0, 15.0]
    assert [nearest_position(stamps, v) for v in (4.0, 5.0, 6.0, 7.5, 9.0, 10.0, 11.0, 12.5, 14.0, 16.0)] == \
        [0, 0, 0, 1, 1, 1, 1, 2, 2, 2]                             # 7.5 and 12.5: a tie stays on the later pair
    assert nearest_position([], 1.0) == 0 and nearest_position([3.0], 9.0) == 0
    assert nearest_position([9.0, 1.0, 5.0], 4.0) == 2 and nearest_position([9.0, 3.5, 5.0], 4.0) == 1    # unsorted: Python's probes, then one comparison
    w = weights_of(np.array([10.0, 12.0, 19.0, 3.0]), 11.0)
    assert w.max() == 1.0 and w[0] == w[1] == 1.0 and np.all(w > 2.0 / 3.0)
    assert w[2] == w[3] == (np.sqrt(np.sqrt(1.0 / 8.0) / 1.0) + 2) / 3


def test_selectors_stand_where_the_reference_has_builders():
    names = {"build_model_poly": "poly", "build_model_weighted_poly": "weighted_poly",
             "build_model_nearest": "nearest", "build_model_linear": "linear"}
    for attr, name in names.items():
        sel = getattr(tdoa_est, attr)
        assert (sel.name, sel.code) == (name, _native.TDOA_MODELS[name]) and tdoa_est.MODELS[name] is sel
        assert name in repr(sel)
        with pytest.raises(NotImplementedError, match="inside the device call"):
            sel([], np.zeros(0), 2.4e6)
    assert tdoa_est.default_model is tdoa_est.build_model_poly
    assert tdoa_est._model("linear") is tdoa_est.build_model_linear


def test_model_arguments_are_refused_like_the_references():
    args = ([], [], 8.0, {}, {}, 2.4e6)
    with pytest.raises(TypeError, match="unexpected keyword argument 'deg'"):
        tdoa_est.estimate_tdoas(*args, model_builder=tdoa_est.build_model_nearest, model_params={"deg": 1})
    with pytest.raises(TypeError, match="unexpected keyword argument 'deg'"):
        tdoa_est.estimate_tdoas(*args, model_builder=tdoa_est.build_model_linear, model_params={"deg": 2})
    with pytest.raises(TypeError, match="unexpected keyword argument 'order'"):
        tdoa_est.estimate_tdoas(*args, model_builder=tdoa_est.build_model_weighted_poly, model_params={"deg": 1, "order": 3})
    with pytest.raises(TypeError, match="unexpected keyword argument 'rcond'"):
        tdoa_est.estimate_tdoas(*args, model_params={"rcond": 0.1})
    for builder in (lambda pairs, sdoa, fs: None, "cubic", 2):
        with pytest.raises(TypeError) as err:
            tdoa_est.estimate_tdoas(*args, model_builder=builder)
        for word in ("build_model_poly", "build_model_weighted_poly", "build_model_nearest", "build_model_linear",
                     "host callables cannot run inside the device call"):
            assert word in str(err.value)
    with pytest.raises(TypeError, match="host callables cannot run inside the device call"):
        tdoa_est.tdoa_columns({}, [0], [], 8.0, {}, {}, 2.4e6, model="spline")
    with pytest.raises(TypeError, match="host callables cannot run inside the device call"):
        kitchen_sink._native_settings(None, 2, 2, (0.1, 0.1), 100, False, "spline")
    assert tdoa_est._model_and_degree(None, None, 3) == (tdoa_est.build_model_poly, 3)
    assert tdoa_est._model_and_degree(tdoa_est.build_model_weighted_poly, {"deg": 1}, 3) == (tdoa_est.build_model_weighted_poly, 1)
    assert tdoa_est._model_and_degree(tdoa_est.build_model_nearest, {}, 2)[0] is tdoa_est.build_model_nearest


def test_command_lines_take_the_model():
    parser = tdoa_est._parser()
    assert parser.get_default("model") == "poly" and parser.get_default("deg") == 2
    choices = {a.dest: a.choices for a in parser._actions}
    assert tuple(choices["model"]) == ("poly", "weighted_poly", "nearest", "linear")
    assert parser._option_string_actions["--deg"].type is int
    locate = kitchen_sink._parser()
    assert locate.get_default("tdoa_model") == "poly"
    assert tuple({a.dest: a.choices for a in locate._actions}["tdoa_model"]) == ("poly", "weighted_poly", "nearest", "linear")


def test_thr_tdoa_model_is_declared_listed_and_the_abi_is_still_11():
    header = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
    assert "#define THR_ABI_VERSION 11" in header and _native.ABI_VERSION == 11
    codes = {name.lower(): int(code) for name, code in re.findall(r"#define THR_TDOA_(\w+) (\d+)\n", header)}
    assert codes == _native.TDOA_MODELS == {"poly": 0, "weighted_poly": 1, "nearest": 2, "linear": 3}
    assert re.search(r"\bint thr_tdoa_model\(int device_id, size_t n_det,", header)
    assert re.search(r"int32_t\* n_kept_out,\s+int model, int32_t\* pick_out\);", header)
    assert re.search(r"\bint thr_tdoa\(int device_id, size_t n_det,", header)          # (unchanged beside it)
    assert "thr_tdoa_model" in _native.EXPORTS
    assert re.search(r"int32_t tdoa_model;\s+/\* THR_TDOA_\*; 0 = the polynomial \*/\n} thr_post_settings;", header)
    assert "int32_t reserved;            /* 0 */" not in header
    fields = [name for name, _ in _native.ThrPostSettings._fields_]
    assert fields[-2:] == ["tdoa_as_text", "tdoa_model"] and "reserved" not in fields
    assert _native.ThrPostSettings.tdoa_model.offset == _native.ThrPostSettings.tdoa_as_text.offset + 4
    assert _native.ThrPostSettings.tdoa_model.size == 4
    source = open(os.path.join(ROOT, "thrifty_amd", "csrc", "tdoa.hip")).read()
    assert "template <int DEG, int MODEL>" in source and "#pragma clang fp contract(off)" in source
    if os.path.exists(_native.LIB_PATH):
        assert _native.load_library().thr_tdoa_model
