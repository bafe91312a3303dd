"""Build the gfx950 shared library in-tree (no torch involved).

    python -m thrifty_amd.build            # hipcc -> thrifty_amd/libthriftyhip.so
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libthriftyhip.so")
SOURCES = ["handle.hip", "window.hip", "pipeline.hip", "entry.hip", "text.hip", "detect16k.hip", "detect16k_geom0.hip", "detect16k_geom1.hip", "detect16k_geom2.hip", "detect16k_carrier.hip", "detect16k_preshift.hip", "detect16k_sec.hip", "detect_seg.hip", "detect_long.hip", "detect_small.hip", "generic.hip", "card_ingest.hip", "identify.hip", "run_file.hip", "card_gate.hip", "run_gate.hip", "template_extract.hip", "template_average.hip", "run_extract.hip", "match.hip", "tdoa.hip", "pos.hip", "postdetect.hip", "survey.hip", "chipscan.hip", "toadstats.hip", "syncstats.hip", "dossier.hip", "reldist.hip", "posq.hip", "track.hip", "posg.hip", "tdoamatrix.hip", "coverage.hip", "pos3.hip", "posg3.hip", "posq3.hip"]
HEADERS = ["host_internal.hpp", "correlate16k.hpp", "correlate16k_geom.hpp", "detect_common.hpp", "fft_regs.hpp", "kernel_util.hpp", "lmdif8.hpp", "passes_w8.hpp", "card_gate.hpp", "template_extract.hpp", "post_stages.hpp", "run_loop.hpp", "hip_own.hpp", "input_window.hpp", "survey.hpp", "chipscan.hpp", "dossier.hpp", "seg_reduce.hpp", "seg_cells.hpp", "pos_lm.hpp", "track_scan.hpp", "tdoa_task.hpp", "pos3_lm.hpp", os.path.join("..", "..", "include", "thrifty_hip.h")]
HOST_ONLY = ("handle.hip", "window.hip", "pipeline.hip", "entry.hip", "text.hip", "run_file.hip", "run_gate.hip", "run_extract.hip",
             "host_internal.hpp", "run_loop.hpp", "hip_own.hpp", "input_window.hpp")     # no kernels: csrc_hash() leaves these out
# kernels that none of the workloads of profiles/hbm_traffic.json launches (the carrier gate's verdict and
# base64 encode): editing them cannot make the recorded counters stale, so csrc_hash() skips them too
UNPROFILED = ("card_gate.hip", "card_gate.hpp")
# the same for template extraction's fold, keep and cut kernels (a list of its own: tests/test_gate_host.py
# pins UNPROFILED to the gate's two files)
UNPROFILED_EXTRACT = ("template_extract.hip", "template_extract.hpp")
# and for the averaged templates' classify, accumulate and finish kernels (a list of its own again:
# tests/test_template_extract_host.py pins UNPROFILED_EXTRACT to the extraction's two files)
UNPROFILED_AVERAGE = ("template_average.hip",)
# and for the matcher (thr_match), which no workload of bench.py reaches
UNPROFILED_MATCH = ("match.hip",)
# and for the TDOA estimator (thr_tdoa)
UNPROFILED_TDOA = ("tdoa.hip",)
# and for the position solver (thr_pos)
UNPROFILED_POS = ("pos.hip",)
# and for the post-detect chain (thr_postdetect) and the header its four stage cores are declared in
UNPROFILED_POST = ("postdetect.hip", "post_stages.hpp")
# and for the capture survey (thr_survey_*)
UNPROFILED_SURVEY = ("survey.hip", "survey.hpp")
# and for the chip-rate scan (thr_chipscan)
UNPROFILED_CHIPSCAN = ("chipscan.hip", "chipscan.hpp")
# and for the detection statistics (thr_toadstats)
UNPROFILED_TOADSTATS = ("toadstats.hip",)
# and for the clock-sync and TDOA statistics (thr_beaconsync, thr_tdoastats)
UNPROFILED_SYNCSTATS = ("syncstats.hip",)
# and for the segmented reduction those two stages share
UNPROFILED_SEGREDUCE = ("seg_reduce.hpp",)
# and for the detection dossiers (thr_dossier_*)
UNPROFILED_DOSSIER = ("dossier.hip", "dossier.hpp")
# and for the relative distance, speed and Doppler (thr_reldist) and the row / cell builders it shares with syncstats.hip
UNPROFILED_RELDIST = ("reldist.hip", "seg_cells.hpp")
# and for the position quality (thr_posq) and the iteration it shares with pos.hip
UNPROFILED_POSQ = ("posq.hip", "pos_lm.hpp")
# and for the tracks (thr_track) and the scan of a non-commutative operator they are built on
UNPROFILED_TRACK = ("track.hip", "track_scan.hpp")
# and for the global position solve (thr_posg)
UNPROFILED_POSG = ("posg.hip",)
# and for the per-beacon TDOA matrices (thr_tdoamatrix) and the per-task estimator they share with tdoa.hip
UNPROFILED_TDMAT = ("tdoamatrix.hip", "tdoa_task.hpp")
# and for the coverage map (thr_coverage)
UNPROFILED_COVERAGE = ("coverage.hip",)
# and for the positions from receivers with three coordinates (thr_pos3) and the iteration of its two modes
UNPROFILED_POS3 = ("pos3.hip", "pos3_lm.hpp")
# and for the global solve on receivers with three coordinates (thr_posg3)
UNPROFILED_POSG3 = ("posg3.hip",)
# and for the position quality on receivers with three coordinates (thr_posq3)
UNPROFILED_POSQ3 = ("posq3.hip",)
# per-file code-generation flags (measured on MI355X, see csrc/detect16k_carrier.hip)
PER_FILE_FLAGS = {"detect16k_carrier.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"],
                  # the work cursor's atomicAdd stays ONE lane's atomic whose result is waited for where it is
                  # used (the wave-aggregation pass puts a v_readfirstlane, and with it the wait, right behind it)
                  "detect16k_sec.hip": ["-mllvm", "-amdgpu-atomic-optimizer-strategy=None"],
                  # the outlier mask repeats numpy's float64 operations one by one: no fused multiply-add
                  "tdoa.hip": ["-ffp-contract=off"],
                  # the team's eight lanes must agree bit for bit, and the 1-D result must equal numpy's
                  "pos.hip": ["-ffp-contract=off"],
                  # the histogram edges and bin indices are numpy's float64 operations one by one
                  "toadstats.hip": ["-ffp-contract=off"],
                  # the discontinuity threshold and the outlier mask are numpy's float64 operations one by one
                  "syncstats.hip": ["-ffp-contract=off"],
                  # searchsorted, the interpolation, the masks and the speeds are numpy's float64 operations one by one
                  "reldist.hip": ["-ffp-contract=off"],
                  # the team's eight lanes must agree bit for bit, and a column of ones must give the unweighted bits
                  "posq.hip": ["-ffp-contract=off"],
                  # a shuffled input must give the same bytes per row, and the statistics are summed as numpy sums them
                  "track.hip": ["-ffp-contract=off"],
                  # a task must return thr_pos's bits, and a cell's sum over the rows NumPy's
                  "posg.hip": ["-ffp-contract=off"],
                  # a task must return thr_tdoa_model's bits, and the cell mask numpy's
                  "tdoamatrix.hip": ["-ffp-contract=off"],
                  # a row's distances are thr_pos's expressions and a cell's sums are added in one stated order
                  "coverage.hip": ["-ffp-contract=off"],
                  # the team's eight lanes must agree bit for bit, and the known-height mode on a flat table gives thr_pos's bits
                  "pos3.hip": ["-ffp-contract=off"],
                  # a task must return thr_pos3's bits, and a cell's sum the statement's (thr_posg's on a flat table)
                  "posg3.hip": ["-ffp-contract=off"],
                  # a task must return thr_pos3's bits, a column of ones the unweighted bits, a flat table thr_posq's
                  "posq3.hip": ["-ffp-contract=off"]}


# host glue in C (CPython API, no device code): the batch constructor of the per-block result objects
FAST_SRC = os.path.join(CSRC, "fastresults.c")
FAST_LIB = os.path.join(HERE, "_fastresults.so")


def build_fastresults(force=False, verbose=False):
    """gcc -> thrifty_amd/_fastresults.so (imported as thrifty_amd._fastresults)."""
    import sysconfig
    if not force and os.path.exists(FAST_LIB) and os.path.getmtime(FAST_LIB) > max(
            os.path.getmtime(FAST_SRC), os.path.getmtime(os.path.abspath(__file__))):
        return FAST_LIB
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        raise RuntimeError("no C compiler: thrifty_amd._fastresults cannot be built")
    cmd = [cc, "-O2", "-fPIC", "-shared", "-Wall", "-I" + sysconfig.get_paths()["include"], FAST_SRC, "-o", FAST_LIB]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return FAST_LIB


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found; the MI355X engine cannot be built")
    return exe


def compile_cmd(src, path, obj, extra=()):
    """The compile line of one entry of SOURCES (scripts/device_code_digest.py runs the same line)."""
    return [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
            "-fno-slp-vectorize"] + PER_FILE_FLAGS.get(src, []) + list(extra) + ["-c", path, "-o", obj]


def csrc_hash():
    """sha256 (first 16 hex digits) over the kernel sources and headers (everything but the host
    side, HOST_ONLY, and the kernels no profiled workload launches, UNPROFILED / UNPROFILED_EXTRACT / UNPROFILED_AVERAGE / UNPROFILED_MATCH / UNPROFILED_TDOA / UNPROFILED_POS / UNPROFILED_POST / UNPROFILED_SURVEY / UNPROFILED_CHIPSCAN / UNPROFILED_TOADSTATS / UNPROFILED_SYNCSTATS / UNPROFILED_SEGREDUCE / UNPROFILED_DOSSIER / UNPROFILED_RELDIST / UNPROFILED_POSQ / UNPROFILED_TRACK / UNPROFILED_POSG / UNPROFILED_TDMAT / UNPROFILED_COVERAGE / UNPROFILED_POS3 / UNPROFILED_POSG3 / UNPROFILED_POSQ3): profiles/hbm_traffic.json records the hash its counter passes were taken on,
    bench.py flags a mismatch (`traffic_stale`)."""
    import hashlib
    h = hashlib.sha256()
    skipped = HOST_ONLY + UNPROFILED + UNPROFILED_EXTRACT + UNPROFILED_AVERAGE + UNPROFILED_MATCH + UNPROFILED_TDOA + UNPROFILED_POS + UNPROFILED_POST + UNPROFILED_SURVEY + UNPROFILED_CHIPSCAN + UNPROFILED_TOADSTATS + UNPROFILED_SYNCSTATS + UNPROFILED_SEGREDUCE + UNPROFILED_DOSSIER + UNPROFILED_RELDIST + UNPROFILED_POSQ + UNPROFILED_TRACK + UNPROFILED_POSG + UNPROFILED_TDMAT + UNPROFILED_COVERAGE + UNPROFILED_POS3 + UNPROFILED_POSG3 + UNPROFILED_POSQ3
    for name in sorted(x for x in SOURCES + HEADERS if not x.startswith("..") and x not in skipped):
        h.update(name.encode())
        with open(os.path.join(CSRC, name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def needs_build():
    if not os.path.exists(LIB):
        return True
    try:       # objects / library of another flag set (a dev variant): rebuild
        if open(os.path.join(CSRC, ".build_flags")).read() != " ".join(os.environ.get("THR_EXTRA_CFLAGS", "").split()):
            return True
    except OSError:
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps)


def build_native(force=False, verbose=False):
    """Compile every HIP source for gfx950 and link libthriftyhip.so (and the C result builder)."""
    build_fastresults(force=force, verbose=verbose)
    if not force and not needs_build():
        return LIB
    # -fno-slp-vectorize: the kernels are hand-vectorised with ext-vector float2;
    # the SLP vectorizer only adds v_mov shuffles (see csrc/fft_regs.hpp)
    extra = os.environ.get("THR_EXTRA_CFLAGS", "").split()
    jobs = []
    objs = []
    # an object is rebuilt when its source, any shared header or this file is newer than it (every
    # translation unit includes the shared headers) -- or when the objects on disk were compiled
    # with a different flag set: the stamp file names the THR_EXTRA_CFLAGS they belong to, so a
    # default build after a dev-variant build (scripts/build_variant.sh) never links leftovers
    common = [os.path.join(CSRC, hname) for hname in HEADERS] + [os.path.abspath(__file__)]
    newest_common = max(os.path.getmtime(d) for d in common)
    stamp = os.path.join(CSRC, ".build_flags")
    flags_now = " ".join(extra)
    try:
        flags_then = open(stamp).read()
    except OSError:
        flags_then = None
    if flags_then != flags_now:
        # objects of another flag set: none of them may survive, whatever interrupts this rebuild --
        # the library and every object go first, the stamp is written LAST (after the link), so an
        # interrupted rebuild is still seen as "flags differ" by the next one
        force = True
        for stale in [LIB, stamp] + [os.path.join(CSRC, src.replace(".hip", ".o")) for src in SOURCES]:
            if os.path.exists(stale):
                os.remove(stale)
    for src in SOURCES:
        obj = os.path.join(CSRC, src.replace(".hip", ".o"))
        objs.append(obj)
        if (not force and os.path.exists(obj) and
                os.path.getmtime(obj) > max(newest_common, os.path.getmtime(os.path.join(CSRC, src)))):
            continue
        cmd = compile_cmd(src, os.path.join(CSRC, src), obj, extra)
        if verbose:
            print(" ".join(cmd))
        jobs.append((subprocess.Popen(cmd), cmd, obj))   # the translation units build in parallel
    for proc, cmd, obj in jobs:
        if proc.wait() != 0:
            raise subprocess.CalledProcessError(proc.returncode, cmd)
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    with open(stamp, "w") as f:
        f.write(flags_now)
    return LIB


if __name__ == "__main__":
    print(build_native(force="--force" in sys.argv, verbose=True))
