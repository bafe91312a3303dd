"""Host side of the detection statistics (no GPU): the wiring of thr_toadstats into the header, the symbol list
and the build; the NumPy restatement (tests/toadstats_ref.py) against the reference's recorded run
(tests/golden/toadstats): discrete outputs and the report's text exactly, floats within the bounds the device
is held to; the restated offset histogram against np.histogram; the argument errors that need no device; the
command line's parser; the tables; and the transcription measure on thrifty_amd/toads_analysis.py alone."""
import json
import os
import re

import numpy as np
import pytest

import toadstats_golden as G
import toadstats_ref as R
from thrifty_amd import _native, build, cli, toads_analysis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["thr_toadstats", "thr_tstats_fetch", "thr_tstats_free", "thr_debug_toadstats_times",
           "thr_debug_toadstats_geometry"]


def test_thr_toadstats_is_declared_listed_and_built():
    header = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
    assert "#define THR_ABI_VERSION 11" in header and _native.ABI_VERSION == 11
    assert re.search(r"\+ thr_toadstats / thr_tstats_fetch / thr_tstats_free", header)
    assert re.search(r"typedef struct thr_tstats_counts \{\s*size_t rows, cells, receivers, minute_bins, carrier_bins, "
                     r"offset_bins;\s*double time0;\s*\} thr_tstats_counts;", header)
    for sym in SYMBOLS:
        assert re.search(r"\b%s\(" % sym, header) and sym in _native.EXPORTS
    for name, (which, _, _) in _native.TSTATS_OUTPUTS.items():
        assert re.search(r"#define THR_TSTATS_%s %d\b" % (name.upper(), which), header), name
    assert "#define THR_TSTATS_N_OUTPUTS %d" % len(_native.TSTATS_OUTPUTS) in header
    assert [name for name, _ in _native.TSTATS_COLUMNS] == [name for name, _ in R.COLUMNS]
    assert "toadstats.hip" in build.SOURCES and build.UNPROFILED_TOADSTATS == ("toadstats.hip",)
    assert build.PER_FILE_FLAGS["toadstats.hip"] == ["-ffp-contract=off"]
    source = open(os.path.join(build.CSRC, "toadstats.hip")).read()
    assert "#pragma clang fp contract(off)" in source and '#include "post_stages.hpp"' in source
    assert len(re.findall(r"\blog10\(", source)) == 2 and "atomicAdd(&" in source
    assert not re.search(r"atomicAdd\([^;]*(double|float)", source) and "hipMalloc(" not in source
    assert '#include "seg_reduce.hpp"' in source        # the reduction: the same properties hold of its text
    shared = open(os.path.join(build.CSRC, "seg_reduce.hpp")).read()
    assert "#pragma clang fp contract(off)" in shared and "atomic" not in shared.split("#include", 1)[1]
    assert "hipMalloc(" not in shared and not re.search(r"\blog10\(", shared)
    assert "analyze_toads" not in cli.COMMANDS


def test_the_tile_grid_cap_is_declared_listed_and_bound():
    header = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
    within = header[header.index("within 11, a pure addition"):header.index("#define THR_ABI_VERSION")]
    assert "+ thr_debug_seg_tile_grid / thr_debug_seg_tile_stats" in within
    assert re.search(r"\bint thr_debug_seg_tile_grid\(int workgroups\);", header)
    assert re.search(r"\bint thr_debug_seg_tile_stats\(int\* launches, int\* max_trips\);", header)
    assert {"thr_debug_seg_tile_grid", "thr_debug_seg_tile_stats"} <= set(_native.EXPORTS)
    assert callable(_native.seg_tile_grid) and callable(_native.seg_tile_stats)
    # one place sizes a tile grid, and so one place counts: the header declares it, toadstats.hip defines it with
    # the two entry points, and no stage works the grid out for itself
    shared = open(os.path.join(build.CSRC, "seg_reduce.hpp")).read()
    assert "dim3 tile_grid(int n_tiles);" in shared and "constexpr int kMaxTileGrid = 2048;" in shared
    for name in ("toadstats.hip", "syncstats.hip", "reldist.hip", "track.hip", "seg_cells.hpp", "track_scan.hpp"):
        text = open(os.path.join(build.CSRC, name)).read()
        assert ("kMaxTileGrid" in text) == (name == "toadstats.hip"), name
        assert len(re.findall(r"\bdim3 thr::seg::tile_grid\(int n_tiles\) \{", text)) == (name == "toadstats.hip"), name
    assert os.path.exists(_native.LIB_PATH), "the library is not built: python -m thrifty_amd.build"
    lib = _native.load_library()
    assert lib.thr_debug_seg_tile_grid and lib.thr_debug_seg_tile_stats
    for bad in (-1, 65537):      # refused before any device is looked for
        with pytest.raises(ValueError, match="thr_debug_seg_tile_grid"):
            _native.seg_tile_grid(bad)
    for ok in (1, 65536, 0):
        _native.seg_tile_grid(ok)
        assert _native.seg_tile_stats() == (0, 0)


def test_the_built_library_exports_thr_toadstats():
    assert os.path.exists(_native.LIB_PATH), "the library is not built: python -m thrifty_amd.build"
    lib = _native.load_library()
    assert all(getattr(lib, sym) for sym in SYMBOLS)
    tile, workgroup = _native.toadstats_geometry()
    assert tile >= 64 and workgroup % 64 == 0


def test_csrc_hash_is_the_recorded_one_and_does_not_see_toadstats(monkeypatch):
    recorded = set(re.findall(r'"csrc_sha16": "([0-9a-f]{16})"', open(os.path.join(ROOT, "profiles", "hbm_traffic.json")).read()))
    assert recorded == {build.csrc_hash()}
    with_stats = build.csrc_hash()
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "toadstats.hip"])
    assert build.csrc_hash() == with_stats
    monkeypatch.undo()
    monkeypatch.setattr(build, "UNPROFILED_TOADSTATS", ())
    assert build.csrc_hash() != with_stats


def test_csrc_hash_does_not_see_the_shared_reduction(monkeypatch):
    assert "seg_reduce.hpp" in build.HEADERS and build.UNPROFILED_SEGREDUCE == ("seg_reduce.hpp",)
    with_header = build.csrc_hash()
    monkeypatch.setattr(build, "HEADERS", [h for h in build.HEADERS if h != "seg_reduce.hpp"])
    assert build.csrc_hash() == with_header
    monkeypatch.undo()
    monkeypatch.setattr(build, "UNPROFILED_SEGREDUCE", ())
    assert build.csrc_hash() != with_header


# ------------------------------------------------------------------ the restatement against the reference
@pytest.fixture(scope="module")
def golden():
    return {name: G.load(name) for name in G.NAMES}


CASES = [(name, "") for name in G.NAMES] + [("realistic", "m_")]


@pytest.fixture(scope="module")
def restated(golden):
    return {(name, prefix): R.toad_stats_ref(G.columns(golden[name]), G.selection(golden[name], prefix))
            for name, prefix in CASES}


def test_the_fixtures_are_the_scenes_of_the_issue(golden):
    g = golden["realistic"]
    assert 500 <= len(g["rxid"]) <= 700 and len(g["cell_rx"]) == 12 and g["cell_tx"].min() == -1
    assert np.ptp(g["timestamp"]) > 3000 and len(g["m_cell_rx"]) > 0
    a = g["exact_rx_fit"][:, 0]
    assert 10e-6 < np.ptp(1 / a) / np.mean(1 / a) < 200e-6        # clocks some tens of ppm apart
    g = golden["ties"]
    on_grid = np.abs(g["offset"] / 0.05 - np.round(g["offset"] / 0.05)) < 1e-9
    assert on_grid.all() and np.all((g["timestamp"] - g["time0"]) % 60 == 0) and np.ptp(g["carrier_noise"]) == 0
    on_edge = [np.isin(g["offset"][(g["rxid"] == rx) & (g["txid"] == tx)], e).sum()
               for rx, tx, e in zip(g["cell_rx"], g["cell_tx"], g["offset_edges"])]
    assert sum(on_edge) > 40
    g = golden["sparse"]
    assert set(np.diff(g["cell_ptr"]).tolist()) == {1, 2} and 1 in [int(np.sum(g["rxid"] == r)) for r in g["rx_id"]]
    assert sum(os.path.getsize(os.path.join(G.GOLDEN, f)) for f in os.listdir(G.GOLDEN)) < 200 << 10


@pytest.mark.parametrize("name,prefix", CASES)
def test_restatement_equals_the_reference(golden, restated, name, prefix):
    counts, out = restated[name, prefix]
    ulps = G.check(counts, out, golden[name], prefix, name + prefix)
    assert ulps == 0.0      # the restatement's dB columns ARE NumPy's
    g = golden[name]
    assert np.array_equal(out["stats"][:, :, 2:], g[prefix + "np_stats"][:, :, 2:])


@pytest.mark.parametrize("name,prefix", CASES)
def test_report_text_of_the_restatement_is_the_references(golden, restated, name, prefix):
    g = golden[name]
    stats = toads_analysis.ToadStats(*restated[name, prefix])
    text = toads_analysis.format_stats(stats)
    want = "Timestamps relative to {:.6f}\n".format(float(g[prefix + "time0"]))
    for rx, tx, body in zip(g[prefix + "cell_rx"], g[prefix + "cell_tx"], g[prefix + "text"]):
        want += "# Stats for RX #{}'s detections of TX #{}'s transmissions:\n\n".format(rx, tx) + str(body) + "\n\n"
    assert text == want
    for c in range(len(stats)):
        assert toads_analysis.format_cell(stats, c) == str(g[prefix + "text"][c])


@pytest.mark.parametrize("name,prefix", CASES)
def test_tables_are_the_references(golden, restated, name, prefix):
    g = golden[name]
    stats = toads_analysis.ToadStats(*restated[name, prefix])
    txids, rxids, counts = toads_analysis.count_table(stats)
    assert np.array_equal(txids, g[prefix + "table_txids"]) and np.array_equal(rxids, g[prefix + "rx_id"])
    assert np.array_equal(counts, g[prefix + "count_table"])
    assert np.array_equal(toads_analysis.mean_energy_table(stats)[2], g[prefix + "mean_energy_table"])
    text = toads_analysis.format_table("# Detection count table:", txids, rxids, counts)
    lines = text.splitlines()
    assert lines[0] == "# Detection count table:" and len(lines) == 3 + len(txids) and len({len(l) for l in lines[1:]}) == 1
    assert lines[1].split() == ["v", "TX", "/", "RX", ">"] + [str(r) for r in rxids]
    assert [l.split() for l in lines[3:]] == [[str(t)] + [str(v) for v in row] for t, row in zip(txids, counts)]


def test_match_length_histogram(golden):
    m = G.matches(golden["realistic"])
    hist = toads_analysis.match_length_histogram(m)
    assert hist == {k: sum(len(x) == k for x in m) for k in (2, 3)} and list(hist) == sorted(hist)


def test_cell_lookup(golden, restated):
    stats = toads_analysis.ToadStats(*restated["realistic", ""])
    g = golden["realistic"]
    cell = stats.cell(1, -1)
    rows = np.flatnonzero((g["rxid"] == 1) & (g["txid"] == -1))
    assert np.array_equal(cell["rows"], rows) and cell["count"] == len(rows)
    assert cell["energy"]["max"] == g["energy"][rows].max() and cell["minute_hist"].sum() == len(rows)
    assert cell["bin_hist"].sum() == len(rows) == cell["offset_hist"].sum()
    with pytest.raises(KeyError):
        stats.cell(9, 9)


# ------------------------------------------------------------------ the offset histogram is np.histogram(x, 10)
def test_offset_histogram_is_numpys():
    rng = np.random.default_rng(7)
    arrays = [rng.uniform(-0.5, 0.5, int(rng.integers(1, 400))) for _ in range(400)]
    arrays += [np.round(rng.uniform(-0.5, 0.5, int(rng.integers(1, 200))), int(rng.integers(1, 3))) for _ in range(300)]
    arrays += [0.05 * rng.integers(-10, 11, int(rng.integers(1, 200))) for _ in range(160)]
    arrays += [rng.integers(-3, 4, int(rng.integers(1, 50))) * 10.0 ** int(rng.integers(-300, 15)) for _ in range(100)]
    arrays += [np.linspace(a, b, 11) for a, b in rng.uniform(-1e3, 1e3, (40, 2))]       # values ON every edge
    arrays += [np.array([0.3]), np.array([0.0, 0.0]), np.array([-0.5, 0.5, 0.5, 0.5]), np.array([-1e300, 1e300]),
               np.array([0.1 * k for k in range(11)]), np.array([0.0, 1e-300]), np.array([-7.0, -7.0, -6.0]),
               np.array([-0.45, 0.45, 0.0]), np.array([0.05 * k for k in range(-10, 11)])]
    assert len(arrays) >= 1000
    for x in arrays:
        edges, counts, flag = R.offset_histogram(x)
        want, want_edges = np.histogram(x, 10)
        assert flag == 0 and np.array_equal(counts, want) and edges.tobytes() == want_edges.tobytes(), x
    for bad in (np.array([0.1, np.nan]), np.array([np.inf, 0.0]), np.array([-np.inf])):
        edges, counts, flag = R.offset_histogram(bad)
        assert flag == 1 and np.isnan(edges).all() and not counts.any()
        with pytest.raises(ValueError):
            np.histogram(bad, 10)


# ------------------------------------------------------------------ errors without a device, the command line
def _columns(n):
    rng = np.random.default_rng(n)
    cols = {name: rng.integers(0, 3, n).astype(kind) for name, kind in R.COLUMNS}
    cols["noise"] += 1
    cols["carrier_noise"] += 1
    return cols


@pytest.mark.parametrize("change,sel,words", [
    (None, [], "selection is empty"), (None, [0, 9], "out of range"), (None, [-1, 2], "out of range"),
    (None, [2, 1], "strictly ascending"), (None, [1, 1], "strictly ascending"),
    (("timestamp", 3, np.nan), None, "not finite"), (("timestamp", 3, np.inf), [2, 3], "not finite"),
    (("timestamp", 3, 1e12), None, r"exceed 2\^26 bins"),
])
def test_what_the_host_pass_refuses(change, sel, words):
    cols = _columns(9)
    if change:
        cols[change[0]][change[1]] = change[2]
    with pytest.raises(ValueError, match=words):
        _native.toadstats(cols, sel)
    with pytest.raises(ValueError):
        R.toad_stats_ref(cols, sel)


def test_no_detections_at_all_is_an_empty_selection():
    with pytest.raises(ValueError, match="selection is empty"):
        _native.toadstats(_columns(0))
    with pytest.raises(ValueError, match="selection is empty"):
        toads_analysis.toad_stats([], matches=None)
    with pytest.raises(ValueError, match="differ in length"):
        _native.toadstats(dict(_columns(4), soa=np.zeros(3)))
    cols = _columns(5)
    cols["timestamp"][4] = np.nan       # outside the selection: not looked at
    if _has_gpu():
        assert _native.toadstats(cols, [0, 1])[0]["rows"] == 2
    else:       # past the host pass: no device, and no fallback
        with pytest.raises(_native.NativeError, match="no HIP device"):
            _native.toadstats(cols, [0, 1])


def _has_gpu():
    try:
        import torch
        return bool(torch.cuda.is_available())
    except ImportError:
        return False


def test_parser_takes_the_references_arguments(tmp_path):
    parser = toads_analysis._parser()
    toads = tmp_path / "x.toads"
    toads.write_text("")
    match = tmp_path / "x.match"
    match.write_text("")
    args = parser.parse_args(["--toad", "-i", str(toads), "-m", str(match), "-o", "stats.npz"])
    assert args.toad and args.input.name == str(toads) and args.match.name == str(match) and args.output == "stats.npz"
    args.input.close()
    args.match.close()
    args = parser.parse_args(["--input", str(toads), "--match", str(match)])
    assert not args.toad and args.output is None
    args.input.close()
    args.match.close()
    actions = {a.dest: a for a in parser._actions}
    assert actions["input"].default == "data.toads" and actions["match"].default is None
    assert "matplotlib" not in open(toads_analysis.__file__).read().replace("No plots", "")


def test_module_docstring_names_every_deviation():
    doc = toads_analysis.__doc__
    for words in ("--toad", "(-1, -1)", "empty selection", "non-finite `offset`", "fewer than two distinct `soa`",
                  "non-finite timestamp", "out of range", "2^26"):
        assert words in doc, words


def test_toads_analysis_is_not_transcribed():
    import test_not_transcribed as T
    if not os.path.isdir(os.path.join(T.REF, "thrifty")):
        pytest.skip("no reference checkout here")
    import difflib
    ours = T._parse(toads_analysis.__file__)
    mine = [(fn.name, T._dump(fn)) for fn in T._functions(ours) if T._statements(fn) > T.MIN_STATEMENTS]
    theirs = [path for path in T._reference_files()["toads_analysis.py"]]
    assert mine and theirs
    for path in theirs:
        for ref_name, ref_dump in [(fn.name, T._dump(fn)) for fn in T._functions(T._parse(path))]:
            for name, dump in mine:
                ratio = difflib.SequenceMatcher(None, dump, ref_dump, autojunk=False).ratio()
                assert ratio < T.LIMIT, (name, ref_name, ratio)
