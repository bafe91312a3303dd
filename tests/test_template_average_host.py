"""Host side of the averaged templates (thr_extract_average*, thrifty_amd.template_extract --average): no GPU.

The statement of include/thrifty_hip.h as tests/average_ref.py restates it: how well the fixed-point envelope
represents the float64 one, how far the statement with ONE record is from the extraction's own template, the
class rule, what averaging is for, and the wiring (header, exports, build lists, the recorded hash, the command
line and its refusals).
"""
import json
import os
import re

import numpy as np
import pytest

import average_ref
import conftest
import extract_ref
from thrifty_amd import _native, build, template_extract

ROOT = conftest.ROOT
FIXTURES = ["extract_16384", "extract_1024", "extract_2048"]      # N / H / W: 16384/4096/1023, 1024/512/127, 2048/1024/510


def load_golden(name):
    return conftest.load_golden("template_extract/" + name)


HEADER = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()


def stated(*phrases):
    """The header's "Averaged templates" block states these, word for word: average_ref restates the HEADER, so a
    test of the restatement is a test of what the library is held to."""
    block = HEADER[HEADER.index(" * Averaged templates --"):HEADER.index("#define THR_AVERAGE_MAX_CLASSES")]
    text = " ".join(re.sub(r"(?m)^ \*", "", block).split())
    for phrase in phrases:
        assert " ".join(phrase.split()) in text, phrase
    return True


def one_record(sample, bin_=10, offset=0.25, flags=_native.FLAG_CORR | _native.FLAG_CARRIER, corr_offset=0.0):
    rec = np.zeros(1, dtype=_native.RECORD_DTYPE)
    rec["flags"], rec["corr_sample"], rec["carrier_bin"], rec["carrier_offset"] = flags, sample, bin_, offset
    rec["corr_offset"] = corr_offset
    return rec


# ------------------------------------------------------------------ the envelope's representation
def test_fixed_point_envelope_represents_the_float64_one():
    """All 65536 byte pairs: e / (2^20 * 640) against hypot of the float64 quantiser values (b - 127.4) / 128.
    q / 640^2 IS the squared magnitude ((5 b - 637) / 640 = (b - 127.4) / 128, exactly, in the rationals), and
    e = floor(sqrt(q) 2^20), so 0 <= sqrt(q) / 640 - e / (2^20 640) < 2^-20 / 640.  The comparison itself is
    float64: 127.4 is off by at most 2^-47 (2^-54 after the division by 128), hypot by one ulp of a value below
    2 (2^-52), e / 671088640 by 2^-53: one rounding, 2^-51 for all of it."""
    assert stated("q = (5 bI - 637)^2 + (5 bQ - 637)^2", "e = floor(sqrt(q * 2^40))", "671088640 = 2^20 * 640")
    assert average_ref.E_UNIT == 2.0 ** 20 * 640 and average_ref.Q_UNIT == 640.0 ** 2
    q, e = average_ref.tables()
    b = (np.arange(256, dtype=np.float64) - 127.4) / 128.0
    exact = np.hypot(b[:, None], b[None, :])
    diff = exact - e.astype(np.float64) / average_ref.E_UNIT
    bound = 2.0 ** -20 / 640
    print("floor error: %.4g .. %.4g of a bound of %.4g; largest q %d" % (diff.min(), diff.max(), bound, q.max()))
    assert q.max() == q[255, 255] == 2 * 638 ** 2 < 2 ** 20 and q.min() == 2 * 2 ** 2 and q[0, 0] == 2 * 637 ** 2
    assert diff.min() >= -2.0 ** -51 and diff.max() < bound + 2.0 ** -51
    for v in (int(q.min()), int(q.max()), 409600, 12345):               # the integer square root, by its definition
        r = average_ref.e_of_q(v)
        assert r * r <= (v << 40) < (r + 1) * (r + 1)


# ------------------------------------------------------------------ one record: the extraction's own template
@pytest.mark.parametrize("name", FIXTURES)
def test_statement_with_one_record_is_the_extractions_template(name):
    """With exactly one qualifying record the averaged template is the extraction's template of that block, but
    for what the two quantiser forms differ by.  extract_ref.expected_template takes float32 samples
    (v - 127.4f) / 128; the statement takes the exact rational (v - 127.4) / 128, floored to 2^-20 / 640.

    Per component, in byte units:
      127.4f = 127.40000152587890625: its representation error is 1.52587890625e-6;
      v - 127.4f is rounded to float32 once, and |v - 127.4f| < 128 has an ulp of 2^-17 at most: 2^-18;
      the division by 128 is exact.  So a component is off by d <= (1.52587890625e-6 + 2^-18) / 128 = 4.17e-8,
      and a magnitude by sqrt(2) d at most (both components move it the same way at worst).
    The fixed-point floor adds 2^-20 / 640 = 1.49e-9:   eps = sqrt(2) d + 2^-20 / 640 = 6.05e-8 per magnitude.
    Through the template's arithmetic t = m s - mean(m s), s = 2 / (mean + std):  the mean moves by eps at most
    and the population std by eps at most (it is 1-Lipschitz in the largest deviation), so
    |ds| = 2 |d(mean + std)| / (mean + std)^2 <= s^2 eps, |d(m s)| <= eps s + max(m) s^2 eps, and the recentring
    at most doubles that:   bound = 2 eps s (1 + max(m) s), first order; the second-order terms are of size
    eps^2 s^3 ~ 1e-13 and are covered by a factor 1.001."""
    assert stated("m[n] = double(acc_e[k][n]) / (double(count) * 671088640.0)",
                  "var[n] = max(double(acc_q[k][n]) / (double(count) * 409600.0) - m[n] * m[n], 0)",
                  "sem[n] = sqrt(var[n] / double(count)) * scale")
    g = load_golden(name)
    w = len(g["template"])
    d = (1.52587890625e-6 + 2.0 ** -18) / 128
    eps = np.sqrt(2.0) * d + 2.0 ** -20 / 640
    for pick in ("", "2"):
        k = int(g["chosen" + pick])
        sample = int(g["sample"][k])
        acc_e, acc_q, count, n_uncl = average_ref.accumulate(g["blocks"][k:k + 1], one_record(sample), w, 0.2)
        assert count == [1] and n_uncl == 0
        tpl, sem, scale = average_ref.finish(acc_e[0], acc_q[0], 1)
        m = acc_e[0].astype(np.float64) / average_ref.E_UNIT
        bound = 1.001 * 2 * eps * scale * (1 + m.max() * scale)
        err = float(np.max(np.abs(tpl - extract_ref.expected_template(g["blocks"][k], sample, w))))
        print("%s pick%s: max |statement - expected_template| = %.3g, %.0f %% of the bound %.3g"
              % (name, pick or "1", err, 100 * err / bound, bound))
        assert err <= bound
        # one record has no spread but the floor's: var = q / 640^2 - m^2 lies in [0, 2 m 2^-20 / 640)
        assert np.all(sem >= 0) and np.max(sem) <= np.sqrt(2 * m.max() * 2.0 ** -20 / 640) * scale


# ------------------------------------------------------------------ the class rule
def test_class_rule_is_identifys():
    assert stated("the class is the LAST k with lo[k] <= v <= hi[k]", "v = double(carrier_bin) + carrier_offset",
                  "counted in n_unclassified and accumulated nowhere")
    assert average_ref.class_of(3.5, ()) == 0                               # no ranges: one class
    ranges = [(1.0, 5.0), (4.0, 9.0), (4.5, 4.5), (20.0, 30.0)]
    assert average_ref.class_of(2.0, ranges) == 0
    assert average_ref.class_of(4.2, ranges) == 1                           # overlap: the LAST match
    assert average_ref.class_of(4.5, ranges) == 2                           # lo == hi == the value
    assert average_ref.class_of(1.0, ranges) == 0 and average_ref.class_of(9.0, ranges) == 1     # both edges inclusive
    assert average_ref.class_of(np.nextafter(1.0, 0), ranges) == -1 and average_ref.class_of(9.5, ranges) == -1
    assert average_ref.class_of(30.0, ranges) == 3 and average_ref.class_of(np.nextafter(30.0, 31), ranges) == -1
    # through accumulate(): the value is double(carrier_bin) + carrier_offset, an unmatched record counts apart
    g = load_golden("extract_1024")
    k, w = int(g["chosen"]), len(g["template"])
    recs = np.concatenate([one_record(int(g["sample"][k]), 4, 0.5), one_record(int(g["sample"][k]), 4, 0.2),
                           one_record(int(g["sample"][k]), 12, -0.25), one_record(int(g["sample"][k]), 4, 0.5, corr_offset=0.3),
                           one_record(int(g["sample"][k]), 4, 0.5, flags=_native.FLAG_CARRIER)])
    blocks = np.repeat(g["blocks"][k:k + 1], 5, axis=0)
    acc_e, acc_q, count, n_uncl = average_ref.accumulate(blocks, recs, w, 0.2, ranges)
    assert count == [0, 1, 1, 0] and n_uncl == 1                            # 4.5 -> 2, 4.2 -> 1, 11.75 -> none
    assert np.array_equal(acc_e[1], acc_e[2]) and not acc_e[0].any() and acc_q[1].any()


# ------------------------------------------------------------------ what it is for
def test_averaged_template_is_closer_to_the_waveform_than_the_single_best():
    """A synthetic capture (average_ref.benefit_capture: a seeded, low-pass-filtered OOK Gold waveform sent 64
    times, each with fresh noise): the r.m.s. error of the averaged template against the noise-free waveform,
    after the best scalar fit, is SMALLER than the single best block's.  No factor is asserted: the envelope of
    a noisy sample is biased upwards where the signal is off (a Rayleigh floor), and that does not average out."""
    assert stated("the result depends on the SET of qualifying records only") and _native.AVERAGE_MAX_CLASSES == 16
    cap = average_ref.benefit_capture()
    w, n_tx = cap["w"], len(cap["blocks"])
    recs = np.concatenate([one_record(int(p)) for p in cap["position"]])
    # the single best block: the largest correlation of the cut's envelope with the base template
    cuts = [template_extract.direct_template(b, int(p), w) for b, p in zip(cap["blocks"], cap["position"])]
    best = int(np.argmax([np.dot(c, cap["base"]) / np.sqrt(np.dot(c, c)) for c in cuts]))
    acc_e, acc_q, count, _ = average_ref.accumulate(cap["blocks"], recs, w, 0.2)
    assert count == [n_tx] and n_tx == 64
    tpl, sem, _ = average_ref.finish(acc_e[0], acc_q[0], n_tx)
    err_avg, err_one = average_ref.fit_error(tpl, cap["clean"]), average_ref.fit_error(cuts[best], cap["clean"])
    every = [average_ref.fit_error(c, cap["clean"]) for c in cuts]
    print("averaged over %d: rms error %.4g; single best (block %d): %.4g; ratio %.3f; best / median / worst single "
          "block %.4g / %.4g / %.4g; mean sem %.4g" % (n_tx, err_avg, best, err_one, err_avg / err_one, min(every),
                                                      float(np.median(every)), max(every), float(np.mean(sem))))
    assert err_avg < err_one
    assert err_avg < min(every)                 # ... and than ANY single block's


# ------------------------------------------------------------------ wiring
def test_header_lists_the_additions_within_abi_11():
    header = open(os.path.join(ROOT, "include", "thrifty_hip.h")).read()
    block = header[header.index("within 11, a pure addition"):header.index("#define THR_ABI_VERSION 11")]
    for sym in ("thr_extract_average", "thr_extract_average_counts", "thr_extract_average_result", "thr_average_opts"):
        assert sym in block and sym in header[header.index("#define THR_ABI_VERSION 11"):]
        if sym != "thr_average_opts":
            assert sym in _native.EXPORTS
    assert _native.ABI_VERSION == 11 and "#define THR_AVERAGE_MAX_CLASSES 16" in header
    assert _native.AVERAGE_MAX_CLASSES == 16 == average_ref.MAX_CLASSES
    import ctypes as C
    assert C.sizeof(_native.ThrAverageOpts) == 8 + 2 * 16 * 8
    # nothing of what tests/test_post_contract_host.py counts
    new = open(os.path.join(ROOT, "thrifty_amd", "csrc", "template_average.hip")).read()
    assert "int device_id" not in new and not re.search(r"g_\w*ms\[", new) and "_fetch" not in new


def test_library_exports_the_three_calls():
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libthriftyhip.so not built")
    lib = _native.load_library()
    for sym in ("thr_extract_average", "thr_extract_average_counts", "thr_extract_average_result"):
        assert getattr(lib, sym)
    assert lib.thr_extract_average(None, None) == _native.ERR_ARG and b"null" in lib.thr_last_error()
    assert lib.thr_extract_average_counts(None, None, None) == _native.ERR_ARG
    assert lib.thr_extract_average_result(None, 0, None, None, 0, None, None) == _native.ERR_ARG


def test_build_lists_and_the_recorded_hash(monkeypatch):
    assert "template_average.hip" in build.SOURCES and build.UNPROFILED_AVERAGE == ("template_average.hip",)
    assert set(build.UNPROFILED_EXTRACT) == {"template_extract.hip", "template_extract.hpp"}
    assert "template_average.hip" not in build.HOST_ONLY and "template_average.hip" not in build.PER_FILE_FLAGS
    recorded = json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json")))
    shas = set(re.findall(r'"csrc_sha16": "([0-9a-f]+)"', json.dumps(recorded)))
    assert shas and shas == {build.csrc_hash()}
    # blind to the new file: the hash without it is the same, and only because it is listed as unprofiled
    with_file = build.csrc_hash()
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "template_average.hip"])
    assert build.csrc_hash() == with_file
    monkeypatch.undo()
    monkeypatch.setattr(build, "UNPROFILED_AVERAGE", ())
    assert build.csrc_hash() != with_file


# ------------------------------------------------------------------ the command line
def test_arguments(tmp_path):
    card = tmp_path / "rx.card"
    card.write_bytes(b"")
    fmap = tmp_path / "freqmap.cfg"
    fmap.write_text("0: 10 - 20\n@3: 0.5\n")
    p = template_extract.build_parser()
    a = p.parse_args([str(card)])
    assert (a.average, a.min_count, a.freq_map, a.rxid, a.npz) == (False, 1, None, None, None)
    a.input.close()
    a = p.parse_args([str(card), "--average", "--min-count", "5", "--freq-map", str(fmap), "--rxid", "3", "--npz", "s.npz"])
    assert (a.average, a.min_count, a.rxid, a.npz) == (True, 5, 3, "s.npz")
    assert template_extract.average_classes(a) == {0: (10.5, 20.5)}
    a.input.close()


def test_class_ranges_of_extract():
    assert template_extract.class_ranges(None) == ([0], [])
    assert template_extract.class_ranges([(1, 2), (3.5, 4)]) == ([0, 1], [(1.0, 2.0), (3.5, 4.0)])
    assert template_extract.class_ranges({7: (1, 2), 2: (0, 9)}) == ([7, 2], [(1.0, 2.0), (0.0, 9.0)])
    with pytest.raises(ValueError, match="at most 16"):
        template_extract.class_ranges([(0, 1)] * 17)


@pytest.mark.parametrize("extra, sentence", [
    (["--average", "--freq-map", "MAP"], "--freq-map needs --rxid"),
    (["--average", "--freq-map", "MAP", "--rxid", "9"], "receiver 9 is not in the frequency map"),
    (["--average", "--freq-map", "MAP17", "--rxid", "0"], "at most 16 ranges"),
    (["--average", "--raw"], "--average takes .card input"),
    (["--average", "--min-count", "0"], "--min-count must be at least 1"),
    (["--freq-map", "MAP", "--rxid", "0"], "--freq-map belongs to --average"),
    (["--npz", "sums.npz"], "--npz belongs to --average"),
    (["--rxid", "0"], "--rxid belongs to --average"),
    (["--min-count", "3"], "--min-count belongs to --average"),
    (["--average", "--rxid", "0"], "--rxid belongs to --freq-map"),
])
def test_refusals_come_before_the_library_is_loaded(tmp_path, monkeypatch, extra, sentence):
    monkeypatch.chdir(tmp_path)

    def no_library(*args, **kwargs):
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_native, "load_library", no_library)
    (tmp_path / "rx.card").write_bytes(b"")
    (tmp_path / "MAP").write_text("1: 10 - 20\n2: 30 - 40\n@0: 0\n@1: 0.25\n")
    (tmp_path / "MAP17").write_text("".join("%d: %d - %d\n" % (t, 3 * t, 3 * t + 2) for t in range(17)) + "@0: 0\n")
    np.save("base.npy", np.ones(127))
    argv = ["rx.card", "-z", "base.npy", "-b", "1024", "-y", "512", "-w", "2-60", "-t", "15*snr", "-u", "15*snr"]
    with pytest.raises(SystemExit, match=re.escape(sentence)):
        template_extract.main(argv + extra)
    # ... and what is not refused does get as far as the library
    with pytest.raises(AssertionError, match="the library was loaded"):
        template_extract.main(argv + ["--average", "--freq-map", "MAP", "--rxid", "1", "--min-count", "2"])
