"""The host contract of the post-detect API as far as the sources and tables can show it without a device: every time
record and the last error are per thread, every fetch / free pair is exported and described by a gapless output table of
the header's length, and tests/post_contract_cases.py has a row for every entry point the header declares."""
import glob
import os
import re

import post_contract_cases as P
from thrifty_amd import _native, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
# `outputs` tables whose name is not the fetch function's stem in capitals
TABLES = {"coverage": "COVERAGE_OUTPUTS"}


def test_every_time_record_and_the_last_error_are_thread_local():
    seen = []
    for path in sorted(glob.glob(os.path.join(build.CSRC, "*.hip")) + glob.glob(os.path.join(build.CSRC, "*.hpp"))):
        for line in open(path).read().splitlines():
            m = re.match(r"\s*((?:static |thread_local |inline |constexpr )*)(?:double|float)\s+(g_\w*ms)\s*\[", line)
            if m:
                assert "thread_local" in m.group(1), "%s: %s" % (os.path.basename(path), line.strip())
                seen.append((os.path.basename(path), m.group(2)))
            m = re.match(r"\s*((?:static |thread_local |inline )*)std::string\s+g_last_error\b", line)
            if m:
                assert "thread_local" in m.group(1), "%s: %s" % (os.path.basename(path), line.strip())
                seen.append((os.path.basename(path), "g_last_error"))
    names = [name for _, name in seen]
    assert names.count("g_last_error") == 1
    # one record per entry point that reports times: thr_identify has none, thr_tdoa and thr_tdoa_model share one
    assert len(names) - 1 == 16, seen
    files = {f for f, _ in seen}
    assert {"match.hip", "tdoa.hip", "pos.hip", "postdetect.hip", "toadstats.hip", "syncstats.hip", "reldist.hip", "posq.hip",
            "track.hip", "posg.hip", "tdoamatrix.hip", "coverage.hip", "pos3.hip", "posg3.hip", "posq3.hip", "handle.hip"} <= files


def fetch_stems():
    return re.findall(r"^int thr_(\w+)_fetch\(", HEADER, flags=re.M)


def test_every_fetch_has_its_free_its_exports_and_a_gapless_table_of_the_headers_length():
    stems = fetch_stems()
    assert len(stems) == 12 and len(set(stems)) == 12
    for stem in stems:
        assert "thr_%s_fetch" % stem in _native.EXPORTS and "thr_%s_free" % stem in _native.EXPORTS, stem
        assert re.search(r"^void thr_%s_free\(" % stem, HEADER, flags=re.M), stem
        table = getattr(_native, TABLES.get(stem, "%s_OUTPUTS" % stem.upper()))
        # the N_OUTPUTS the header defines last before the fetch function
        n = int(re.findall(r"#define THR_\w+_N_OUTPUTS (\d+)", HEADER[:HEADER.index("int thr_%s_fetch(" % stem)])[-1])
        assert sorted(which for which, _, _ in table.values()) == list(range(n)), stem
        if stem != "coverage":
            assert re.search(r"#define THR_%s_N_OUTPUTS %d\b" % (stem.upper(), n), HEADER), stem
        else:
            assert "#define THR_COV_N_OUTPUTS %d" % n in HEADER
    assert {case.family.stem for case in P.FAMILIES} == set(stems)
    for case in P.FAMILIES:
        assert case.family.outputs is getattr(_native, TABLES.get(case.family.stem, "%s_OUTPUTS" % case.family.stem.upper()))


def test_the_table_names_every_entry_point_that_takes_a_device_id():
    declared = re.findall(r"^int (thr_\w+)\(int device_id\b", HEADER, flags=re.M)
    assert len(declared) == len(set(declared)) >= 18
    assert set(P.ENTRIES) == set(declared)
    for case in P.CASES:
        assert case.entry in _native.EXPORTS and callable(case.fn) and case.refusal is not None and case.refusal.match
        assert not any(a.flags.writeable for a in case.inputs()), case
    # the modes the issue names: both identify modes, the four TDOA models, 1-D and 2-D, and both 3-D modes of each solver
    for name in ("identify_map", "identify_auto", "tdoa", "tdoa_nearest", "tdoa_linear", "tdoa_weighted", "pos_three", "pos_line",
                 "z_four", "h_ring4", "posg3_free_z", "posg3_known_height", "posq3_free_z", "posq3_known_height"):
        assert name in P.BY_NAME
