"""ctypes binding of libthriftyhip.so (include/thrifty_hip.h).

There is deliberately no fallback: if the shared library is missing or no
MI355X is visible, constructing an :class:`Engine` raises.
"""
from __future__ import annotations

import atexit
import ctypes as C
import os
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("THRIFTY_HIP_LIB") or os.path.join(HERE, "libthriftyhip.so")  # env: A/B builds

THR_IN_U8 = 0
THR_IN_C64 = 1
FLAG_CARRIER = 1
FLAG_CORR = 2
FLAG_INDEX_ERROR = 4
FLAG_INT_OFFSET = 8
FLAG_FIT_UNCONVERGED = 16
N_KERNEL_SLOTS = 5

ABI_VERSION = 11    # THR_ABI_VERSION of include/thrifty_hip.h

EXPORTS = [
    "thr_abi_version", "thr_last_error", "thr_create", "thr_destroy", "thr_detect",
    "thr_create_preshift", "thr_create_fastdet", "thr_create_ex", "thr_plan_sections", "thr_host_register", "thr_host_unregister", "thr_input_window", "thr_detect_card", "thr_detect_stream", "thr_detect_stream_device", "thr_detect_device", "thr_sync", "thr_set_stream", "thr_compact_device",
    "thr_profile_enable", "thr_profile_read", "thr_kernel_name", "thr_debug_fft",
    "thr_debug_stage", "thr_debug_stage_offsets", "thr_identify", "thr_frame_card",
    "thr_submit", "thr_submit_card", "thr_submit_stream", "thr_collect", "thr_inputs_consumed", "thr_poll",
    "thr_set_stream_default", "thr_format_toad",
    "thr_run_card", "thr_run_stream", "thr_get_settings", "thr_input_window_ex", "thr_input_window_release", "thr_detect_offsets", "thr_set_wait_mode", "thr_debug_window", "thr_debug_window_times", "thr_debug_correlate_geom", "thr_debug_sections", "thr_debug_section_counts", "thr_debug_pipe_times", "thr_get_path_info",
    "thr_gate", "thr_gate_stream", "thr_gate_card", "thr_gate_slot_stride", "thr_format_card",
    "thr_run_gate_stream", "thr_run_gate_card",
    "thr_extract_create", "thr_extract_destroy", "thr_extract_reset", "thr_extract_feed", "thr_extract_feed_card",
    "thr_extract_feed_stream", "thr_extract_submit_card", "thr_extract_submit_stream", "thr_extract_result",
    "thr_run_extract_card", "thr_run_extract_stream",
    "thr_extract_average", "thr_extract_average_counts", "thr_extract_average_result",
    "thr_match", "thr_debug_match_times",
    "thr_tdoa", "thr_debug_tdoa_times", "thr_tdoa_model",
    "thr_pos", "thr_debug_pos_times",
    "thr_postdetect", "thr_post_fetch", "thr_post_free", "thr_debug_post_times",
    "thr_debug_live_resources",
    "thr_survey_create", "thr_survey_destroy", "thr_survey_reset", "thr_survey_shift", "thr_survey_pending",
    "thr_survey_feed", "thr_survey_feed_stream", "thr_debug_survey_geometry",
    "thr_chipscan", "thr_debug_chipscan_geometry", "thr_debug_chipscan_budget", "thr_debug_chipscan_times",
    "thr_debug_chipscan_fill", "thr_debug_chipscan_groups",
    "thr_toadstats", "thr_tstats_fetch", "thr_tstats_free", "thr_debug_toadstats_times", "thr_debug_toadstats_geometry",
    "thr_debug_seg_tile_grid", "thr_debug_seg_tile_stats",
    "thr_beaconsync", "thr_bsync_fetch", "thr_bsync_free", "thr_debug_beaconsync_times", "thr_debug_beaconsync_geometry",
    "thr_tdoastats", "thr_tdstats_fetch", "thr_tdstats_free", "thr_debug_tdoastats_times", "thr_debug_tdoastats_geometry",
    "thr_dossier_create", "thr_dossier_destroy", "thr_dossier_reset", "thr_dossier_feed", "thr_dossier_feed_card",
    "thr_dossier_feed_stream", "thr_dossier_result", "thr_dossier_geometry",
    "thr_reldist", "thr_reldist_fetch", "thr_reldist_free", "thr_debug_reldist_times", "thr_debug_reldist_geometry",
    "thr_posq", "thr_posq_fetch", "thr_posq_free", "thr_debug_posq_times",
    "thr_track", "thr_track_fetch", "thr_track_free", "thr_debug_track_times", "thr_debug_track_geometry",
    "thr_posg", "thr_posg_fetch", "thr_posg_free", "thr_debug_posg_times",
    "thr_tdoamatrix", "thr_tdmat_fetch", "thr_tdmat_free", "thr_debug_tdoamatrix_times", "thr_debug_tdoamatrix_geometry",
    "thr_coverage", "thr_coverage_fetch", "thr_coverage_free", "thr_debug_coverage_times",
    "thr_pos3", "thr_debug_pos3_times",
    "thr_posg3", "thr_posg3_fetch", "thr_posg3_free", "thr_debug_posg3_times",
    "thr_posq3", "thr_posq3_fetch", "thr_posq3_free", "thr_debug_posq3_times",
]
ERR_ARG, ERR_DEVICE, ERR_STATE, ERR_INDEX = -1, -2, -3, -4       # THR_ERR_*
VARIANT_DEFAULT, VARIANT_PRESHIFT, VARIANT_FASTDET, VARIANT_GATE = 0, 1, 2, 3      # THR_VARIANT_*
INTERPOLATORS = {"parabolic": 0, "none": 1, "gaussian": 2, "cosine": 3}      # THR_INTERP_*
PATHS = {"auto": 0, "multipass": 1, "unsectioned": 2, "generic_rows": 3, "unsectioned_generic_rows": 4}      # THR_PATH_*
MAX_IN_FLIGHT = 3       # THR_MAX_IN_FLIGHT
TOAD_LINE_MAX = 384     # THR_TOAD_LINE_MAX
CARD_HEADER_MAX = 48    # THR_CARD_HEADER_MAX


BSYNC_COUNTS = ("rows", "cells", "discontinuities", "cuts")
TDSTATS_COUNTS = ("rows", "cells", "robust")
RELDIST_COUNTS = ("rows", "cells", "speeds", "speed_points", "dop_points")
POSQ_COUNTS = ("groups", "rows", "flagged", "tasks")
TRACK_COUNTS = ("rows", "tracks", "used", "rejected", "rounds", "converged")
POSG_COUNTS = ("groups", "rows", "tasks", "starts", "grid", "map_groups")
POSG3_COUNTS = ("groups", "rows", "tasks", "starts", "grid", "grid_z", "map_groups")
TDMAT_COUNTS = ("tasks", "cells", "rows", "tdoas")
COVERAGE_COUNTS = ("cells", "nx", "ny", "n_rx", "trials", "covered", "tasks", "rows", "slabs", "slab_groups", "slab_bytes",
                   "keep_tasks", "keep_rows")


AVERAGE_MAX_CLASSES = 16      # THR_AVERAGE_MAX_CLASSES


class ThrAverageOpts(C.Structure):        # thr_average_opts
    _fields_ = [("n_classes", C.c_int32), ("lo", C.c_double * AVERAGE_MAX_CLASSES),
                ("hi", C.c_double * AVERAGE_MAX_CLASSES)]


class ThrBsyncCounts(C.Structure):        # thr_bsync_counts
    _fields_ = [(name, C.c_size_t) for name in BSYNC_COUNTS]


class ThrTdstatsCounts(C.Structure):      # thr_tdstats_counts
    _fields_ = [(name, C.c_size_t) for name in TDSTATS_COUNTS]


class ThrReldistCounts(C.Structure):      # thr_reldist_counts
    _fields_ = [(name, C.c_size_t) for name in RELDIST_COUNTS]


class ThrPosqCounts(C.Structure):         # thr_posq_counts
    _fields_ = [(name, C.c_size_t) for name in POSQ_COUNTS]


class ThrPosqOpts(C.Structure):           # thr_posq_opts
    _fields_ = [("max_iter", C.c_int32), ("min_rx", C.c_int32), ("x0", C.c_double * 2), ("gate_m", C.c_double),
                ("ratio", C.c_double)]


class ThrPosgCounts(C.Structure):         # thr_posg_counts
    _fields_ = [(name, C.c_size_t) for name in POSG_COUNTS]


class ThrPosgOpts(C.Structure):           # thr_posg_opts
    _fields_ = [("max_iter", C.c_int32), ("grid", C.c_int32), ("starts", C.c_int32), ("x0", C.c_double * 2),
                ("margin_m", C.c_double), ("merge_m", C.c_double), ("ratio", C.c_double), ("floor_m", C.c_double),
                ("map_first", C.c_int64), ("map_count", C.c_int32)]


class ThrPosg3Counts(C.Structure):        # thr_posg3_counts
    _fields_ = [(name, C.c_size_t) for name in POSG3_COUNTS]


class ThrPosg3Opts(C.Structure):          # thr_posg3_opts
    _fields_ = [("max_iter", C.c_int32), ("grid", C.c_int32), ("grid_z", C.c_int32), ("starts", C.c_int32),
                ("x0", C.c_double * 3), ("margin_m", C.c_double), ("merge_m", C.c_double), ("ratio", C.c_double),
                ("floor_m", C.c_double), ("map_first", C.c_int64), ("map_count", C.c_int32)]


class ThrPosq3Counts(C.Structure):        # thr_posq3_counts
    _fields_ = [(name, C.c_size_t) for name in POSQ_COUNTS]


class ThrPosq3Opts(C.Structure):          # thr_posq3_opts
    _fields_ = [("max_iter", C.c_int32), ("min_rx", C.c_int32), ("has_z_range", C.c_int32), ("x0", C.c_double * 3),
                ("z_range", C.c_double * 2), ("gate_m", C.c_double), ("ratio", C.c_double)]


class ThrTdmatCounts(C.Structure):        # thr_tdmat_counts
    _fields_ = [(name, C.c_size_t) for name in TDMAT_COUNTS]


class ThrCoverageCounts(C.Structure):     # thr_coverage_counts
    _fields_ = [(name, C.c_size_t) for name in COVERAGE_COUNTS]


class ThrCoverageOpts(C.Structure):       # thr_coverage_opts
    _fields_ = [("lo", C.c_double * 2), ("hi", C.c_double * 2), ("nx", C.c_int32), ("ny", C.c_int32), ("trials", C.c_int32),
                ("max_iter", C.c_int32), ("range_m", C.c_double), ("gross_m", C.c_double), ("x0", C.c_double * 2),
                ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("slab_groups", C.c_int64), ("keep_first", C.c_int32),
                ("keep_count", C.c_int32)]


class ThrTrackCounts(C.Structure):        # thr_track_counts
    _fields_ = [(name, C.c_size_t) for name in TRACK_COUNTS]


class ThrTrackOpts(C.Structure):          # thr_track_opts
    _fields_ = [("q", C.c_double), ("v0", C.c_double), ("gate", C.c_double), ("max_rounds", C.c_int32), ("reserved", C.c_int32)]


class ThrReldistGeom(C.Structure):        # thr_reldist_geom
    _fields_ = [("beacon", C.c_int32), ("rx0", C.c_int32), ("rx1", C.c_int32), ("reserved", C.c_int32),
                ("d_beacon", C.c_double), ("dist_rx", C.c_double), ("dist_beacon", C.c_double)]


class ThrReldistOpts(C.Structure):        # thr_reldist_opts
    _fields_ = [("method", C.c_int32), ("reserved", C.c_int32), ("sample_rate", C.c_double), ("block_len", C.c_double),
                ("carrier_hz", C.c_double), ("thresh", C.c_double), ("smooth_frac", C.c_double),
                ("geometry", C.POINTER(ThrReldistGeom)), ("n_geometry", C.c_size_t)]


class ThrSettings(C.Structure):
    _fields_ = [
        ("block_len", C.c_int32), ("history_len", C.c_int32),
        ("n_templates", C.c_int32), ("template_len", C.c_int32),
        ("templates", C.POINTER(C.c_double)),
        ("carrier_len", C.c_int32), ("carrier_window", C.c_int32 * 2),
        ("carrier_thresh", C.c_double * 3), ("corr_thresh", C.c_double * 3),
        ("device_id", C.c_int32), ("max_batch", C.c_int32),
    ]


class ThrPathInfo(C.Structure):
    _fields_ = [
        ("n_sections", C.c_int32), ("section_len", C.c_int32), ("rows_lo", C.c_int32), ("rows_hi", C.c_int32),
        ("why_unsectioned", C.c_int32), ("n_templates", C.c_int32),
        ("carrier_kernel", C.c_char * 48), ("correlate_kernel", C.c_char * 48), ("text", C.c_char * 256),
    ]


# THR_WHY_*
WHY_UNSECTIONED = ("sectioned", "path", "variant", "stddev", "geometry", "block_len")


class ThrRunOpts(C.Structure):
    _fields_ = [
        ("struct_bytes", C.c_uint32), ("batch_blocks", C.c_int32), ("out_fd", C.c_int32),
        ("with_rxid", C.c_int32), ("rxid", C.c_int64), ("with_txid", C.c_int32),
        ("carrier_offset_mode", C.c_int32), ("timestamp", C.c_double),
        ("rec_out", C.c_void_p), ("rec_capacity", C.c_size_t),
    ]


class ThrRunStats(C.Structure):
    _fields_ = [
        ("blocks", C.c_uint64), ("detections", C.c_uint64), ("batches", C.c_uint64),
        ("bytes_in", C.c_uint64), ("text_bytes", C.c_uint64), ("index_error_at", C.c_uint64),
        ("index_error_block", C.c_int64), ("index_error_bin", C.c_int32), ("reserved_", C.c_int32),
        ("total_s", C.c_double), ("frame_s", C.c_double), ("submit_s", C.c_double), ("wait_s", C.c_double),
        ("format_s", C.c_double), ("write_s", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved_"}


class ThrGateRunOpts(C.Structure):
    _fields_ = [
        ("struct_bytes", C.c_uint32), ("batch_blocks", C.c_int32), ("out_fd", C.c_int32), ("skip", C.c_int32),
        ("timestamp", C.c_double), ("rec_out", C.c_void_p), ("rec_capacity", C.c_size_t),
    ]


class ThrGateRunStats(C.Structure):
    _fields_ = [
        ("blocks", C.c_uint64), ("passed", C.c_uint64), ("batches", C.c_uint64), ("bytes_in", C.c_uint64),
        ("text_bytes", C.c_uint64), ("total_s", C.c_double), ("frame_s", C.c_double), ("gate_s", C.c_double),
        ("wait_s", C.c_double), ("format_s", C.c_double), ("write_s", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


# numpy mirror of thr_record (64 bytes)
RECORD_DTYPE = np.dtype([
    ("block_idx", "<i8"), ("flags", "<u4"), ("template_id", "<i4"),
    ("carrier_bin", "<i4"), ("corr_sample", "<i4"),
    ("carrier_offset", "<f8"), ("corr_offset", "<f8"),
    ("carrier_energy", "<f4"), ("carrier_noise", "<f4"),
    ("corr_energy", "<f4"), ("corr_noise", "<f4"), ("reserved", "<u8"),
])
assert RECORD_DTYPE.itemsize == 64

# numpy mirror of thr_chip_record (24 bytes)
CHIP_RECORD_DTYPE = np.dtype([("sample", "<i4"), ("flags", "<u4"), ("energy", "<f4"), ("noise", "<f4"),
                              ("offset", "<f8")])
assert CHIP_RECORD_DTYPE.itemsize == 24
CHIP_MAX_CHIPS = 2047       # kChipMaxChips of csrc/chipscan.hpp


class ThrPostSettings(C.Structure):       # thr_post_settings
    _fields_ = [("map", C.c_void_p), ("n_map", C.c_size_t), ("match_window", C.c_double), ("min_match", C.c_int32),
                ("n_rx", C.c_int32), ("rx_ids", C.c_void_p), ("dims", C.c_int32), ("n_beacons", C.c_int32),
                ("rx_coords", C.c_void_p), ("first_two_rx", C.c_int32 * 2), ("beacon_ids", C.c_void_p),
                ("dist", C.c_void_p), ("tdoa_window", C.c_double), ("sample_rate", C.c_double), ("deg", C.c_int32),
                ("max_iter", C.c_int32), ("x0", C.c_double * 2), ("tdoa_as_text", C.c_int32), ("tdoa_model", C.c_int32)]


POST_COUNTS = ("kept", "matches", "match_entries", "misses", "collisions", "tasks", "rows", "groups", "failures")


class ThrPostCounts(C.Structure):         # thr_post_counts
    _fields_ = [(name, C.c_size_t) for name in POST_COUNTS]


TSTATS_COUNTS = ("rows", "cells", "receivers", "minute_bins", "carrier_bins", "offset_bins")


class ThrTstatsCounts(C.Structure):       # thr_tstats_counts
    _fields_ = [(name, C.c_size_t) for name in TSTATS_COUNTS] + [("time0", C.c_double)]


class ThrDossierOut(C.Structure):          # thr_dossier_out
    _fields_ = [(name, C.c_void_p) for name in (
        "records", "timestamps", "positions", "hist", "fft_mag", "filtered", "synced", "synced_fft_mag", "corr",
        "scalars", "autocorr")]


DOSSIER_SCALARS_DTYPE = np.dtype([      # thr_dossier_scalars
    ("rms_unsynced", "<f8"), ("rms_synced", "<f8"), ("fft_std", "<f8"), ("corr_std", "<f8"),
    ("synced_fft_std", "<f8"), ("filtered_std", "<f8"),
    ("carrier_threshold", "<f8"), ("corr_threshold", "<f8"), ("fit_amplitude", "<f8"), ("fit_offset", "<f8"),
    ("fit_valid", "<i4"), ("peak_start", "<i4"), ("peak_len", "<i4"), ("reserved", "<i4"),
    ("corr_shifted", "<f8", (11,))])
DOSSIER_MAX_RANGES = 16
DOSSIER_ARRAYS = ("hist", "fft_mag", "filtered", "synced", "synced_fft_mag", "corr", "scalars")


class NativeError(RuntimeError):
    """An error status of the library: args = (message[, status code[, thr_run_* statistics]])."""

    def __str__(self):
        return str(self.args[0]) if self.args else ""

    @property
    def code(self):
        return self.args[1] if len(self.args) > 1 else None


_lib = None


def _share_hip_runtime_with_torch():
    """A process can hold only ONE HIP runtime.  PyTorch-ROCm wheels bundle their
    own libamdhip64 (SONAME libamdhip64.so.7, same as /opt/rocm's); if both copies
    get loaded, whichever initialises second sees "No HIP GPUs".  bench.py and the
    multi-GPU gather need torch in the same process, so when a torch wheel with a
    bundled runtime is installed we load *that* copy first (RTLD_GLOBAL); our
    DT_NEEDED libamdhip64.so.7 then resolves to it by SONAME.  Without torch the
    system ROCm runtime is used.  THRIFTY_HIP_RUNTIME=system skips this."""
    if os.environ.get("THRIFTY_HIP_RUNTIME", "") == "system":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            try:
                C.CDLL(path, mode=C.RTLD_GLOBAL)
            except OSError:
                return


def load_library():
    """dlopen the engine; raises NativeError (never falls back) if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(
            "%s not found: build it with `python -m thrifty_amd.build` (needs hipcc). "
            "thrifty_amd has no CPU fallback." % LIB_PATH)
    _share_hip_runtime_with_torch()
    lib = C.CDLL(LIB_PATH)
    vp, i64p = C.c_void_p, C.POINTER(C.c_int64)
    lib.thr_abi_version.restype = C.c_int
    if lib.thr_abi_version() != ABI_VERSION:
        raise NativeError("%s has ABI version %d, this package needs %d: rebuild it with "
                          "`python -m thrifty_amd.build --force`" % (LIB_PATH, lib.thr_abi_version(), ABI_VERSION))
    lib.thr_last_error.restype = C.c_char_p
    lib.thr_kernel_name.restype = C.c_char_p
    lib.thr_kernel_name.argtypes = [C.c_int]
    lib.thr_create.argtypes = [C.POINTER(ThrSettings), C.POINTER(vp)]
    lib.thr_create_preshift.argtypes = [C.POINTER(ThrSettings), C.c_int, C.POINTER(vp)]
    lib.thr_create_fastdet.argtypes = [C.POINTER(ThrSettings), C.POINTER(vp)]
    lib.thr_input_window.argtypes = [vp, vp, C.c_size_t]
    lib.thr_input_window_ex.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_size_t]
    lib.thr_run_card.argtypes = [vp, vp, C.c_size_t, C.POINTER(ThrRunOpts), C.POINTER(ThrRunStats)]
    lib.thr_run_stream.argtypes = [vp, vp, C.c_size_t, C.c_int64, C.POINTER(ThrRunOpts), C.POINTER(ThrRunStats)]
    lib.thr_get_settings.argtypes = [vp, C.POINTER(ThrSettings)]
    lib.thr_host_register.argtypes = [vp, C.c_size_t]
    lib.thr_host_unregister.argtypes = [vp]
    ip = C.POINTER(C.c_int)
    lib.thr_plan_sections.argtypes = [C.c_int, C.c_int, C.c_int, ip] + [C.c_int * 8] * 5
    lib.thr_create_ex.argtypes = [C.POINTER(ThrSettings), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    lib.thr_destroy.argtypes = [vp]
    lib.thr_destroy.restype = None
    lib.thr_detect.argtypes = [vp, vp, C.c_int, vp, C.c_size_t, vp]
    lib.thr_detect_card.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_size_t, vp]
    lib.thr_detect_offsets.argtypes = [vp, vp, C.c_int, vp, C.c_size_t, vp, vp]
    lib.thr_frame_card.argtypes = [vp, C.c_size_t, C.c_int, C.c_int, C.c_size_t, vp, vp, vp,
                                   C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    lib.thr_detect_device.argtypes = [vp, vp, C.c_int, vp, C.c_size_t, vp]
    lib.thr_detect_stream.argtypes = [vp, vp, C.c_size_t, C.c_int64, vp, C.c_size_t,
                                      C.POINTER(C.c_size_t)]
    lib.thr_detect_stream_device.argtypes = [vp, vp, vp, C.c_size_t, vp]
    u64p = C.POINTER(C.c_uint64)
    lib.thr_submit.argtypes = [vp, vp, C.c_int, vp, C.c_size_t, vp, u64p]
    lib.thr_submit_card.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_size_t, vp, u64p]
    lib.thr_submit_stream.argtypes = [vp, vp, C.c_size_t, C.c_int64, vp, C.c_size_t,
                                      C.POINTER(C.c_size_t), u64p]
    lib.thr_collect.argtypes = [vp, C.c_uint64]
    lib.thr_inputs_consumed.argtypes = [vp, C.c_uint64]
    lib.thr_poll.argtypes = [vp, C.c_uint64, C.POINTER(C.c_int)]
    lib.thr_set_stream_default.argtypes = [vp]
    lib.thr_format_toad.argtypes = [vp, vp, C.c_size_t, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int,
                                    vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.thr_sync.argtypes = [vp]
    lib.thr_set_stream.argtypes = [vp, vp]
    lib.thr_compact_device.argtypes = [vp, vp, C.c_size_t, vp, C.POINTER(C.c_size_t)]
    lib.thr_profile_enable.argtypes = [vp, C.c_int]
    lib.thr_profile_read.argtypes = [vp, C.POINTER(C.c_double), i64p]
    lib.thr_debug_fft.argtypes = [vp, vp, C.c_int, C.c_size_t, vp]
    lib.thr_debug_stage.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_int, vp, vp]
    lib.thr_debug_stage_offsets.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_int, vp, vp, vp]
    lib.thr_identify.argtypes = [C.c_int, C.c_size_t, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp, vp,
                                 vp, C.POINTER(C.c_size_t)]
    szp = C.POINTER(C.c_size_t)
    lib.thr_gate_slot_stride.argtypes = [vp, szp, szp]
    lib.thr_gate.argtypes = [vp, vp, vp, C.c_size_t, vp, szp, vp, C.c_size_t]
    lib.thr_gate_stream.argtypes = [vp, vp, C.c_size_t, C.c_int64, vp, C.c_size_t, szp, szp, vp, C.c_size_t]
    lib.thr_gate_card.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_size_t, vp, szp, vp, C.c_size_t]
    lib.thr_format_card.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, vp, C.c_size_t, szp]
    lib.thr_run_gate_stream.argtypes = [vp, vp, C.c_size_t, C.c_int64, C.POINTER(ThrGateRunOpts),
                                        C.POINTER(ThrGateRunStats)]
    lib.thr_run_gate_card.argtypes = [vp, vp, C.c_size_t, C.POINTER(ThrGateRunOpts), C.POINTER(ThrGateRunStats)]
    lib.thr_extract_create.argtypes = [vp, C.c_double, C.POINTER(vp)]
    lib.thr_extract_destroy.argtypes = [vp]
    lib.thr_extract_destroy.restype = None
    lib.thr_extract_reset.argtypes = [vp]
    lib.thr_extract_feed.argtypes = [vp, vp, C.c_int, vp, vp, C.c_size_t, vp]
    lib.thr_extract_feed_card.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, C.c_size_t, vp]
    lib.thr_extract_feed_stream.argtypes = [vp, vp, C.c_size_t, C.c_int64, vp, vp, C.c_size_t, szp]
    lib.thr_extract_submit_card.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, C.c_size_t, vp, u64p]
    lib.thr_extract_submit_stream.argtypes = [vp, vp, C.c_size_t, C.c_int64, C.c_double, vp, C.c_size_t, szp, u64p]
    lib.thr_extract_result.argtypes = [vp, vp, C.POINTER(C.c_double), vp, C.c_size_t, u64p]
    lib.thr_extract_average.argtypes = [vp, C.POINTER(ThrAverageOpts)]
    lib.thr_extract_average_counts.argtypes = [vp, vp, u64p]
    lib.thr_extract_average_result.argtypes = [vp, C.c_int, vp, vp, C.c_size_t, vp, vp]
    lib.thr_dossier_create.argtypes = [vp, vp, C.c_int, C.c_int64, C.POINTER(vp)]
    lib.thr_dossier_destroy.argtypes = [vp]
    lib.thr_dossier_destroy.restype = None
    lib.thr_dossier_reset.argtypes = [vp]
    lib.thr_dossier_feed.argtypes = [vp, vp, C.c_int, vp, vp, C.c_size_t, vp, szp, u64p, u64p]
    lib.thr_dossier_feed_card.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, C.c_size_t, vp, szp, u64p, u64p]
    lib.thr_dossier_feed_stream.argtypes = [vp, vp, C.c_size_t, C.c_int64, vp, vp, C.c_size_t, szp, szp, u64p, u64p]
    lib.thr_dossier_result.argtypes = [vp, C.c_size_t, C.c_size_t, C.POINTER(ThrDossierOut), szp]
    lib.thr_dossier_geometry.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.thr_run_extract_card.argtypes = [vp, vp, C.c_size_t, C.POINTER(ThrRunOpts), vp, C.POINTER(ThrRunStats)]
    lib.thr_run_extract_stream.argtypes = [vp, vp, C.c_size_t, C.c_int64, C.POINTER(ThrRunOpts), vp,
                                           C.POINTER(ThrRunStats)]
    lib.thr_match.argtypes = [C.c_int, C.c_size_t, vp, vp, vp, vp, C.c_double, C.c_int, vp, vp, szp, vp, szp, vp, szp]
    lib.thr_debug_match_times.argtypes = [C.POINTER(C.c_double)]
    lib.thr_tdoa.argtypes = ([C.c_int, C.c_size_t] + [vp] * 5 + [C.c_size_t, vp, vp, vp, C.c_int, C.c_int, vp,
                             C.c_double, C.c_double, C.c_int, C.c_size_t, vp, vp, vp, szp, vp, vp, szp, vp, szp, vp, vp])
    lib.thr_tdoa_model.argtypes = lib.thr_tdoa.argtypes + [C.c_int, vp]
    lib.thr_debug_tdoa_times.argtypes = [C.POINTER(C.c_double)]
    lib.thr_pos.argtypes = [C.c_int, C.c_size_t, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]
    lib.thr_debug_pos_times.argtypes = [C.POINTER(C.c_double)]
    lib.thr_postdetect.argtypes = ([C.c_int, C.c_size_t] + [vp] * 8 +
                                   [C.POINTER(ThrPostSettings), C.POINTER(vp), C.POINTER(ThrPostCounts)])
    lib.thr_post_fetch.argtypes = [vp, C.c_int, vp, C.c_size_t]
    lib.thr_post_free.argtypes = [vp]
    lib.thr_post_free.restype = None
    lib.thr_debug_post_times.argtypes = [C.POINTER(C.c_double)]
    lib.thr_debug_live_resources.argtypes = [C.POINTER(C.c_int64)]
    lib.thr_survey_create.argtypes = [vp, C.c_int, C.POINTER(vp)]
    lib.thr_survey_destroy.argtypes = [vp]
    lib.thr_survey_destroy.restype = None
    lib.thr_survey_reset.argtypes = [vp]
    lib.thr_survey_shift.argtypes = [vp, ip]
    lib.thr_survey_pending.argtypes = [vp, u64p, u64p]
    lib.thr_survey_feed.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, C.c_size_t, szp]
    lib.thr_survey_feed_stream.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, szp, vp, vp, C.c_size_t, szp]
    lib.thr_debug_survey_geometry.argtypes = [vp, ip, ip, ip]
    lib.thr_chipscan.argtypes = [vp, vp, C.c_int, C.c_size_t, vp, C.c_int, vp, C.c_size_t, vp, vp]
    lib.thr_debug_chipscan_geometry.argtypes = [vp, C.c_size_t, ip, ip]
    lib.thr_debug_chipscan_budget.argtypes = [vp, C.c_size_t]
    lib.thr_debug_chipscan_times.argtypes = [vp, C.POINTER(C.c_double)]
    lib.thr_debug_chipscan_fill.argtypes = [vp, C.c_size_t]
    lib.thr_debug_chipscan_groups.argtypes = [vp, C.c_size_t, C.c_size_t, ip, ip]
    lib.thr_toadstats.argtypes = ([C.c_int, C.c_size_t] + [vp] * 11 +
                                  [vp, C.c_size_t, C.POINTER(vp), C.POINTER(ThrTstatsCounts)])
    lib.thr_tstats_fetch.argtypes = [vp, C.c_int, vp, C.c_size_t]
    lib.thr_tstats_free.argtypes = [vp]
    lib.thr_tstats_free.restype = None
    lib.thr_debug_toadstats_times.argtypes = [C.POINTER(C.c_double)]
    lib.thr_debug_toadstats_geometry.argtypes = [ip, ip]
    lib.thr_debug_seg_tile_grid.argtypes = [C.c_int]
    lib.thr_debug_seg_tile_stats.argtypes = [ip, ip]
    lib.thr_beaconsync.argtypes = ([C.c_int, C.c_size_t] + [vp] * 6 + [C.c_size_t, vp, vp, C.c_int, vp, vp, C.c_size_t,
                                   vp, C.c_size_t, C.POINTER(vp), C.POINTER(ThrBsyncCounts)])
    lib.thr_tdoastats.argtypes = ([C.c_int, C.c_size_t] + [vp] * 7 + [vp, vp, C.c_int, C.POINTER(vp),
                                  C.POINTER(ThrTdstatsCounts)])
    lib.thr_reldist.argtypes = ([C.c_int, C.c_size_t] + [vp] * 7 + [C.c_size_t, vp, vp] + [vp, C.c_size_t] * 3 +
                                [C.POINTER(ThrReldistOpts), C.POINTER(vp), C.POINTER(ThrReldistCounts)])
    lib.thr_debug_reldist_times.argtypes = [C.POINTER(C.c_double)]
    lib.thr_debug_reldist_geometry.argtypes = [ip, ip, ip]
    lib.thr_posq.argtypes = ([C.c_int, C.c_size_t] + [vp] * 6 + [C.c_int, C.c_int, vp, C.POINTER(ThrPosqOpts), C.POINTER(vp),
                             C.POINTER(ThrPosqCounts)])
    lib.thr_debug_posq_times.argtypes = [C.POINTER(C.c_double)]
    lib.thr_track.argtypes = [C.c_int, C.c_size_t] + [vp] * 7 + [C.POINTER(ThrTrackOpts), C.POINTER(vp), C.POINTER(ThrTrackCounts)]
    lib.thr_debug_track_times.argtypes = [C.POINTER(C.c_double)]
    lib.thr_debug_track_geometry.argtypes = [ip, ip, ip]
    lib.thr_posg.argtypes = ([C.c_int, C.c_size_t] + [vp] * 5 + [C.c_int, C.c_int, vp, C.POINTER(ThrPosgOpts), C.POINTER(vp),
                             C.POINTER(ThrPosgCounts)])
    lib.thr_debug_posg_times.argtypes = [C.POINTER(C.c_double)]
    lib.thr_tdoamatrix.argtypes = ([C.c_int, C.c_size_t] + [vp] * 6 + [C.c_size_t, vp, vp] + [vp, C.c_size_t] * 3 +
                                   [vp, C.c_double, C.c_double, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(ThrTdmatCounts)])
    lib.thr_debug_tdoamatrix_times.argtypes = [C.POINTER(C.c_double)]
    lib.thr_debug_tdoamatrix_geometry.argtypes = [ip, ip, ip]
    lib.thr_coverage.argtypes = [C.c_int, C.c_int, vp, vp, C.POINTER(ThrCoverageOpts), C.POINTER(vp), C.POINTER(ThrCoverageCounts)]
    lib.thr_debug_coverage_times.argtypes = [C.POINTER(C.c_double)]
    lib.thr_pos3.argtypes = [C.c_int, C.c_size_t] + [vp] * 5 + [C.c_int, vp, C.c_int, vp, vp, vp, C.c_int] + [vp] * 8
    lib.thr_debug_pos3_times.argtypes = [C.POINTER(C.c_double)]
    lib.thr_posg3.argtypes = ([C.c_int, C.c_size_t] + [vp] * 5 + [C.c_int, vp, C.c_int, vp, vp, vp, C.POINTER(ThrPosg3Opts),
                              C.POINTER(vp), C.POINTER(ThrPosg3Counts)])
    lib.thr_debug_posg3_times.argtypes = [C.POINTER(C.c_double)]
    lib.thr_posg3_fetch.argtypes = [vp, C.c_int, vp, C.c_size_t]
    lib.thr_posg3_free.argtypes = [vp]
    lib.thr_posg3_free.restype = None
    if hasattr(lib, "thr_posq3"):       # a THRIFTY_HIP_LIB build from before thr_posq3 still loads for an A/B run; posq3() on it raises
        lib.thr_posq3.argtypes = ([C.c_int, C.c_size_t] + [vp] * 6 + [C.c_int, vp, C.c_int, vp, C.POINTER(ThrPosq3Opts), C.POINTER(vp),
                                  C.POINTER(ThrPosq3Counts)])
        lib.thr_debug_posq3_times.argtypes = [C.POINTER(C.c_double)]
        lib.thr_posq3_fetch.argtypes = [vp, C.c_int, vp, C.c_size_t]
        lib.thr_posq3_free.argtypes = [vp]
        lib.thr_posq3_free.restype = None
    for stem in ("bsync", "tdstats", "reldist", "posq", "track", "posg", "tdmat", "coverage"):
        getattr(lib, "thr_%s_fetch" % stem).argtypes = [vp, C.c_int, vp, C.c_size_t]
        getattr(lib, "thr_%s_free" % stem).argtypes = [vp]
        getattr(lib, "thr_%s_free" % stem).restype = None
    for stem in ("beaconsync", "tdoastats"):
        getattr(lib, "thr_debug_%s_times" % stem).argtypes = [C.POINTER(C.c_double)]
        getattr(lib, "thr_debug_%s_geometry" % stem).argtypes = [ip, ip]
    _lib = lib
    return lib


def _check(lib, rc):
    if rc != 0:
        raise NativeError("libthriftyhip: %s (code %d)" % (lib.thr_last_error().decode(), rc))


def frame_card(buf, start, stop, block_len, at_eof, max_records):
    """thr_frame_card over buf[start:stop] (bytes-like: bytearray, mmap, ...) ->
    (timestamps float64[n], block_idx int64[n], payload_off int64[n] relative to buf, next start)."""
    lib = load_library()
    arr = np.frombuffer(buf, dtype=np.uint8)
    cap = int(min(max_records, (stop - start) // 16 + 1))
    ts = np.empty(cap, dtype=np.float64)
    idx = np.empty(cap, dtype=np.int64)
    off = np.empty(cap, dtype=np.int64)
    n, used = C.c_size_t(0), C.c_size_t(0)
    _check(lib, lib.thr_frame_card(arr.ctypes.data + start, stop - start, int(block_len), int(bool(at_eof)),
                                   cap, ts.ctypes.data, idx.ctypes.data, off.ctypes.data,
                                   C.byref(n), C.byref(used)))
    del arr
    k = n.value
    return ts[:k], idx[:k], off[:k] + start, start + used.value


def format_toad(recs, timestamps, new_len, rxid=None, with_txid=False, carrier_offset_f32=False):
    """thr_format_toad: `.toad` text (bytes, one '\\n'-terminated line per record) for a batch of
    DETECTED records -- the text `DetectionResult.serialize()` produces, without per-record
    objects.  with_txid: prepend each record's template_id as the txid column."""
    lib = load_library()
    recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE).reshape(-1)
    ts = np.ascontiguousarray(timestamps, dtype=np.float64).reshape(-1)
    n = len(recs)
    assert len(ts) == n
    buf = np.empty(max(1, n * TOAD_LINE_MAX), dtype=np.uint8)
    used = C.c_size_t(0)
    _check(lib, lib.thr_format_toad(recs.ctypes.data, ts.ctypes.data, n, int(new_len),
                                    0 if rxid is None else 1, 0 if rxid is None else int(rxid),
                                    int(bool(with_txid)), int(carrier_offset_f32),
                                    buf.ctypes.data, buf.size, C.byref(used)))
    return buf[:used.value].tobytes()


def gate_payload_chars(block_len):
    """Base64 characters of one block's 2 * block_len raw bytes ('=' padding included)."""
    return (2 * int(block_len) + 2) // 3 * 4


def gate_slot_stride(block_len):
    """Bytes from one payload slot of the gate to the next: payload, newline, rounded up to 16."""
    return (gate_payload_chars(block_len) + 1 + 15) // 16 * 16


def format_card(timestamps, block_idx, slots, block_len):
    """thr_format_card: .card text (bytes, one line per slot) from the gate's payload slots
    (uint8 [n, slot_stride] or flat) -- the text `block_data.card_line` produces."""
    lib = load_library()
    ts = np.ascontiguousarray(timestamps, dtype=np.float64).reshape(-1)
    idx = np.ascontiguousarray(block_idx, dtype=np.int64).reshape(-1)
    n = len(ts)
    stride, chars = gate_slot_stride(block_len), gate_payload_chars(block_len)
    sl = np.ascontiguousarray(slots, dtype=np.uint8).reshape(-1)
    assert len(idx) == n and sl.size >= n * stride
    buf = np.empty(max(1, n * (CARD_HEADER_MAX + chars + 1)), dtype=np.uint8)
    used = C.c_size_t(0)
    _check(lib, lib.thr_format_card(ts.ctypes.data, idx.ctypes.data, sl.ctypes.data, stride, chars, n,
                                    buf.ctypes.data, buf.size, C.byref(used)))
    return buf[:used.value].tobytes()


def format_toad_address():
    """Address of thr_format_toad in the loaded library (0: no library) -- handed to
    thrifty_amd._fastresults, which links nothing, so that DetectionResult.serialize() of an engine
    record is the library's own text."""
    try:
        lib = load_library()
    except Exception:       # noqa: BLE001 -- host-only use without the library: Python formatting
        return 0
    return C.cast(lib.thr_format_toad, C.c_void_p).value or 0


class Ticket(object):
    """An open thr_submit*(): the records array the library will fill and the inputs it may
    still be reading (kept alive here)."""
    __slots__ = ("id", "out", "keep")

    def __init__(self, tid, out, keep):
        self.id, self.out, self.keep = tid, out, keep


FREQ_RANGE_DTYPE = np.dtype([("rxid", "<i4"), ("txid", "<i4"), ("lo", "<f8"), ("hi", "<f8")])


def identify(rxid, block, timestamp, carrier_bin, carrier_offset, energy, freq_ranges=None,
             device_id=0):
    """thr_identify on columns -> (txid int32[n], keep bool[n], kept_order int64[k]).
    freq_ranges: None (automatic windows) or rows (rxid, txid, lo, hi) in map order.  ValueError for what
    thr_identify refuses."""
    lib = load_library()
    n = len(rxid)
    cols = [np.ascontiguousarray(rxid, dtype=np.int32), np.ascontiguousarray(block, dtype=np.int32),
            np.ascontiguousarray(timestamp, dtype=np.float64),
            np.ascontiguousarray(carrier_bin, dtype=np.int32),
            np.ascontiguousarray(carrier_offset, dtype=np.float64),
            np.ascontiguousarray(energy, dtype=np.float64)]
    assert all(len(c) == n for c in cols)
    fmap = (np.zeros(0, dtype=FREQ_RANGE_DTYPE) if freq_ranges is None
            else np.ascontiguousarray(np.asarray(freq_ranges, dtype=FREQ_RANGE_DTYPE)))
    if freq_ranges is not None and len(fmap) == 0:
        raise ValueError("empty frequency map")
    txid = np.zeros(n, dtype=np.int32)
    keep = np.zeros(n, dtype=np.uint8)
    order = np.zeros(n, dtype=np.int64)
    n_kept = C.c_size_t(0)
    rc = lib.thr_identify(int(device_id), n, *[c.ctypes.data for c in cols],
                          fmap.ctypes.data if len(fmap) else None, len(fmap),
                          txid.ctypes.data, keep.ctypes.data, order.ctypes.data,
                          C.byref(n_kept))
    if rc == ERR_ARG:       # like every other post-detect wrapper: what the library refuses is a ValueError
        raise ValueError(lib.thr_last_error().decode())
    _check(lib, rc)
    return txid, keep.astype(bool), order[:n_kept.value]


MATCH_WORKGROUP = 256      # kBlock of csrc/match.hip: the workgroup size of every matcher kernel


def match(rxid, txid, timestamp, energy, window, min_match=2, device_id=0):
    """thr_match on columns of detections in timestamp order -> (match_ptr int64[m + 1],
    match_idx int64[match_ptr[-1]], misses int64[k], collisions int64[c, 2]): match m is
    match_idx[match_ptr[m]:match_ptr[m + 1]].  ValueError if the timestamps decrease or hold a NaN."""
    lib = load_library()
    n = len(rxid)
    cols = [np.ascontiguousarray(rxid, dtype=np.int32), np.ascontiguousarray(txid, dtype=np.int32),
            np.ascontiguousarray(timestamp, dtype=np.float64), np.ascontiguousarray(energy, dtype=np.float64)]
    assert all(c.ndim == 1 and len(c) == n for c in cols)
    ptr = np.zeros(n + 1, dtype=np.int64)
    idx = np.zeros(n, dtype=np.int64)
    miss = np.zeros(n, dtype=np.int64)
    coll = np.zeros((n, 2), dtype=np.int64)
    n_match, n_miss, n_coll = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    rc = lib.thr_match(int(device_id), n, *[c.ctypes.data for c in cols], float(window), int(min_match),
                       ptr.ctypes.data, idx.ctypes.data, C.byref(n_match), miss.ctypes.data, C.byref(n_miss),
                       coll.ctypes.data, C.byref(n_coll))
    if rc == ERR_ARG:
        raise ValueError(lib.thr_last_error().decode())
    _check(lib, rc)
    ptr = ptr[:n_match.value + 1]
    return ptr, idx[:int(ptr[-1])], miss[:n_miss.value], coll[:n_coll.value]


def match_times():
    """{copies in, kernels, copies out} of this thread's last match(), milliseconds (HIP events)."""
    lib = load_library()
    ms = (C.c_double * 3)()
    _check(lib, lib.thr_debug_match_times(ms))
    return tuple(ms)


class HostPin(object):
    """thr_host_register over a bytes-like object (an mmap of the input file): page-locks it so
    that the engine's chunk copies are asynchronous DMA out of the page cache.  Best effort:
    `.ok` False (and nothing locked) if the range is larger than `limit` bytes -- by default a
    quarter of the memory the kernel says is available -- or the runtime refuses; the engine
    works the same on unlocked memory.  close() (or garbage collection) unlocks."""

    def __init__(self, buf, limit=None):
        self._ptr, self.ok, self.why = None, False, ""
        arr = np.frombuffer(buf, dtype=np.uint8)
        if limit is None:
            limit = _available_memory() // 4
        if arr.size == 0 or arr.size > limit:
            self.why = "%d bytes against a limit of %d" % (arr.size, limit)
            return
        try:
            lib = load_library()
            rc = lib.thr_host_register(arr.ctypes.data, arr.size)
        except Exception as exc:       # no library / no device: the caller's engine will say so itself
            self.why = str(exc)
            return
        if rc != 0:
            self.why = lib.thr_last_error().decode()
            return
        self._lib, self._ptr, self.ok = lib, arr.ctypes.data, True

    def close(self):
        if self._ptr is not None:
            self._lib.thr_host_unregister(self._ptr)
            self._ptr, self.ok = None, False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _available_memory():
    try:
        for ln in open("/proc/meminfo"):
            if ln.startswith("MemAvailable:"):
                return int(ln.split()[1]) * 1024
    except (OSError, ValueError):
        pass
    return 1 << 33


def plan_sections(block_len, history_len, template_len):
    """thr_plan_sections: the overlap-save plan of a long block's correlate stage (host-only).
    Returns a list of dicts (start, win_lo, win_hi, sum_lo, sum_hi), block coordinates; [] when the
    geometry is not sectioned."""
    lib = load_library()
    n = C.c_int()
    arrs = [(C.c_int * 8)() for _ in range(5)]
    _check(lib, lib.thr_plan_sections(int(block_len), int(history_len), int(template_len), C.byref(n), *arrs))
    keys = ("start", "win_lo", "win_hi", "sum_lo", "sum_hi")
    return [dict((k, int(a[g])) for k, a in zip(keys, arrs)) for g in range(n.value)]


# Handles still open when the interpreter exits are destroyed by an atexit hook -- threads joined,
# pages unlocked, streams gone BEFORE the process runs the HIP runtime's own static destructors.  (A
# Detector's stage objects refer back to it, so a script that never calls close() keeps its engine,
# and its input window's threads inside the runtime, until then.)
_live_engines = weakref.WeakSet()


def _close_live_engines():
    for eng in list(_live_engines):
        try:
            eng.close()
        except Exception:       # noqa: BLE001 -- at exit: nothing to report to
            pass


atexit.register(_close_live_engines)


class Engine(object):
    """One detector handle == one (device, stream).  Not thread-safe per handle."""

    @classmethod
    def gate(cls, block_len, history_len, window=(0, -1), threshold=(100.0, 2.0), device_id=0, max_batch=2048,
             path="auto"):
        """The carrier gate (THR_VARIANT_GATE): fastcard's verdict `max > c + s * noise` (power domain,
        threshold = (c, s)) over the inclusive, non-wrapping bin window [min, max], and the passed
        blocks as base64.  No templates; only the gate_* methods and the queries apply."""
        lib = load_library()
        st = ThrSettings()
        st.block_len, st.history_len = int(block_len), int(history_len)
        st.n_templates, st.template_len, st.templates = 0, 0, None
        st.carrier_window[0], st.carrier_window[1] = int(window[0]), int(window[1])
        st.carrier_thresh[0], st.carrier_thresh[1], st.carrier_thresh[2] = float(threshold[0]), float(threshold[1]), 0.0
        st.device_id, st.max_batch = int(device_id), int(max_batch)
        handle = C.c_void_p()
        _check(lib, lib.thr_create_ex(C.byref(st), VARIANT_GATE, 0, PATHS[path], C.byref(handle)))
        self = cls.__new__(cls)
        self.path, self.preshift_num = path, 0
        self._lib, self._h = lib, handle
        _live_engines.add(self)
        self.block_len, self.history_len, self.n_templates = int(block_len), int(history_len), 0
        self.max_batch = int(max_batch)
        self.slot_stride, self.payload_chars = gate_slot_stride(block_len), gate_payload_chars(block_len)
        return self

    def _gate_out(self, nb, slots):
        if slots is None:
            slots = np.empty(max(1, nb) * self.slot_stride, dtype=np.uint8)
        assert slots.dtype == np.uint8 and slots.flags.c_contiguous
        return np.zeros(nb, dtype=RECORD_DTYPE), slots

    def gate_blocks(self, blocks, block_idx=None, slots=None):
        """thr_gate: u8 [B, 2N] -> (records [B], n_passed, slots uint8 -- slot k = the k-th passed
        block's base64 payload and newline at [k * slot_stride ...]).  `slots`: a caller buffer (uint8,
        at least B * slot_stride bytes; only the passed slots' payload + newline bytes are written)."""
        a = np.ascontiguousarray(np.asarray(blocks, dtype=np.uint8)).reshape(-1, 2 * self.block_len)
        nb = a.shape[0]
        out, slots = self._gate_out(nb, slots)
        idx, idx_p = self._idx_ptr(block_idx, nb)
        n = C.c_size_t(0)
        _check(self._lib, self._lib.thr_gate(self._h, a.ctypes.data, idx_p, nb, out.ctypes.data, C.byref(n),
                                             slots.ctypes.data, slots.size))
        return out, n.value, slots

    def gate_stream(self, stream, first_block_idx=0, slots=None):
        """thr_gate_stream: raw u8 I/Q bytes, overlapping blocks framed on the device (see
        detect_stream) -> (records [n_whole_blocks], n_passed, slots)."""
        buf = np.frombuffer(stream, dtype=np.uint8)
        stride = 2 * (self.block_len - self.history_len)
        nb = 0 if buf.size < 2 * self.block_len else (buf.size - 2 * self.block_len) // stride + 1
        out, slots = self._gate_out(nb, slots)
        got, n = C.c_size_t(0), C.c_size_t(0)
        _check(self._lib, self._lib.thr_gate_stream(self._h, buf.ctypes.data, buf.size, int(first_block_idx),
                                                    out.ctypes.data, nb, C.byref(got), C.byref(n),
                                                    slots.ctypes.data, slots.size))
        assert got.value == nb
        return out, n.value, slots

    def gate_card(self, text, payload_off, block_idx=None, slots=None):
        """thr_gate_card: .card text + payload offsets (see detect_card) -> (records, n_passed, slots)."""
        buf = np.frombuffer(text, dtype=np.uint8)
        off = np.ascontiguousarray(np.asarray(payload_off, dtype=np.int64))
        nb = off.shape[0]
        out, slots = self._gate_out(nb, slots)
        idx, idx_p = self._idx_ptr(block_idx, nb)
        n = C.c_size_t(0)
        _check(self._lib, self._lib.thr_gate_card(self._h, buf.ctypes.data, buf.size, off.ctypes.data, idx_p, nb,
                                                  out.ctypes.data, C.byref(n), slots.ctypes.data, slots.size))
        return out, n.value, slots

    def run_gate(self, data, card=False, out_fd=None, skip=0, timestamp=None, batch_blocks=0, rec_out=None,
                 first_block_idx=0):
        """thr_run_gate_stream / thr_run_gate_card: gate the whole input `data` (bytes-like: the mapped
        capture or .card file) inside the library; the .card lines go to the descriptor `out_fd`, every
        block's record into `rec_out` (a RECORD_DTYPE array) if given.  -> the statistics as a dict."""
        buf = np.frombuffer(data, dtype=np.uint8)
        o = ThrGateRunOpts()
        o.struct_bytes = C.sizeof(ThrGateRunOpts)
        o.batch_blocks, o.skip = int(batch_blocks or 0), int(skip)
        o.out_fd = -1 if out_fd is None else int(out_fd)
        o.timestamp = float("nan") if timestamp is None else float(timestamp)
        if rec_out is not None:
            assert rec_out.dtype == RECORD_DTYPE and rec_out.flags.c_contiguous
            o.rec_out, o.rec_capacity = rec_out.ctypes.data, rec_out.size
        st = ThrGateRunStats()
        ptr = buf.ctypes.data if buf.size else None
        if card:
            rc = self._lib.thr_run_gate_card(self._h, ptr, buf.size, C.byref(o), C.byref(st))
        else:
            rc = self._lib.thr_run_gate_stream(self._h, ptr, buf.size, int(first_block_idx), C.byref(o), C.byref(st))
        del buf
        _check(self._lib, rc)
        return st.as_dict()

    def __init__(self, block_len, history_len, templates, carrier_thresh, carrier_window,
                 corr_thresh, carrier_len=0, device_id=0, max_batch=256, preshift_num=0,
                 fastdet=False, path="auto", interpolator="parabolic"):
        """preshift_num > 0 selects the PreshiftDetector variant (thr_create_preshift);
        fastdet=True the fastdet-compatible one (thr_create_fastdet, power-domain thresholds).
        path: "auto" (the fastest kernels for the block length), "multipass" (the generic
        multi-pass pipeline whatever the length) or "unsectioned" (block_len 32768 / 65536: one
        long transform pair instead of overlap-save sections) -- thr_create_ex's THR_PATH_*; the
        non-default paths are independent implementations kept for cross-checks.
        interpolator (preshift variant): "parabolic" | "none" | "gaussian" | "cosine" (THR_INTERP_*)."""
        lib = load_library()
        tpl = np.ascontiguousarray(np.atleast_2d(np.asarray(templates, dtype=np.float64)))
        if tpl.ndim != 2:
            raise ValueError("templates must be 1-D or [n_templates, template_len]")
        st = ThrSettings()
        st.block_len, st.history_len = int(block_len), int(history_len)
        st.n_templates, st.template_len = tpl.shape
        st.templates = tpl.ctypes.data_as(C.POINTER(C.c_double))
        st.carrier_len = int(carrier_len)
        window = (0, -1) if carrier_window is None else carrier_window
        st.carrier_window[0], st.carrier_window[1] = int(window[0]), int(window[1])
        for i in range(3):
            st.carrier_thresh[i] = float(carrier_thresh[i])
            st.corr_thresh[i] = float(corr_thresh[i])
        st.device_id, st.max_batch = int(device_id), int(max_batch)
        handle = C.c_void_p()
        variant = VARIANT_FASTDET if fastdet else VARIANT_PRESHIFT if preshift_num else VARIANT_DEFAULT
        arg = int(preshift_num) | (INTERPOLATORS[interpolator] << 16 if preshift_num and not fastdet else 0)
        _check(lib, lib.thr_create_ex(C.byref(st), variant, arg, PATHS[path], C.byref(handle)))
        self.path = path
        self.preshift_num = int(preshift_num)
        self._lib, self._h = lib, handle
        _live_engines.add(self)
        self.block_len, self.n_templates = int(block_len), int(tpl.shape[0])
        self.history_len = int(history_len)
        self.max_batch = int(max_batch)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.thr_destroy(self._h)      # (closes an input window too)
            self._h = None
            self._window = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- host-buffer path -------------------------------------------------
    def _as_input(self, blocks):
        a = np.asarray(blocks)
        if a.dtype == np.uint8:
            a = np.ascontiguousarray(a).reshape(-1, 2 * self.block_len)
            return a, THR_IN_U8
        a = np.ascontiguousarray(a.astype(np.complex64, copy=False)).reshape(-1, self.block_len)
        return a, THR_IN_C64

    def detect(self, blocks, block_idx=None):
        """blocks: u8 [B, 2N] or complex64 [B, N] -> structured records [B, n_templates]."""
        a, fmt = self._as_input(blocks)
        nb = a.shape[0]
        out = np.zeros((nb, self.n_templates), dtype=RECORD_DTYPE)
        idx_p = None
        if block_idx is not None:
            idx = np.ascontiguousarray(np.asarray(block_idx, dtype=np.int64))
            assert idx.shape == (nb,)
            idx_p = idx.ctypes.data
        _check(self._lib, self._lib.thr_detect(self._h, a.ctypes.data, fmt, idx_p, nb,
                                               out.ctypes.data))
        return out

    def detect_offsets(self, blocks, carrier_offset, block_idx=None):
        """thr_detect_offsets: detect() with the sub-bin carrier offset of every block given (float64
        [B]) instead of fitted -- the slow path behind a replaced `Detector.sync.interpolator`."""
        a, fmt = self._as_input(blocks)
        nb = a.shape[0]
        off = np.ascontiguousarray(np.asarray(carrier_offset, dtype=np.float64))
        assert off.shape == (nb,)
        out = np.zeros((nb, self.n_templates), dtype=RECORD_DTYPE)
        idx, idx_p = self._idx_ptr(block_idx, nb)
        _check(self._lib, self._lib.thr_detect_offsets(self._h, a.ctypes.data, fmt, idx_p, nb, off.ctypes.data,
                                                       out.ctypes.data))
        return out

    def detect_card(self, text, payload_off, block_idx=None):
        """text: bytes-like holding .card records; payload_off: int64 offsets of each block's
        base64 payload.  Decoding happens on the device.  -> records [B, n_templates]."""
        buf = np.frombuffer(text, dtype=np.uint8)
        off = np.ascontiguousarray(np.asarray(payload_off, dtype=np.int64))
        nb = off.shape[0]
        out = self._records_out(nb)
        idx_p = None
        if block_idx is not None:
            idx = np.ascontiguousarray(np.asarray(block_idx, dtype=np.int64))
            assert idx.shape == (nb,)
            idx_p = idx.ctypes.data
        _check(self._lib, self._lib.thr_detect_card(self._h, buf.ctypes.data, buf.size,
                                                    off.ctypes.data, idx_p, nb, out.ctypes.data))
        return out

    def detect_stream(self, stream, first_block_idx=0):
        """stream: bytes-like raw interleaved u8 I/Q; the overlapping blocks
        (block_reader framing, stride block_len - history_len samples) are framed on the
        device.  -> records [n_whole_blocks, n_templates]."""
        buf = np.frombuffer(stream, dtype=np.uint8)
        stride = 2 * (self.block_len - self.history_len)
        nb = 0 if buf.size < 2 * self.block_len else (buf.size - 2 * self.block_len) // stride + 1
        out = self._records_out(nb)
        got = C.c_size_t(0)
        _check(self._lib, self._lib.thr_detect_stream(self._h, buf.ctypes.data, buf.size,
                                                      int(first_block_idx), out.ctypes.data, nb,
                                                      C.byref(got)))
        assert got.value == nb
        return out

    # ---- asynchronous host path: submit a batch, collect its records later --
    # Record arrays of the ticket interface.  A batch's array is 128 KiB and up -- glibc serves that by
    # mmap, and every mmap / munmap / first-touch fault of a process whose input window is page-locking
    # a file waits for the address-space lock the lockers hold for milliseconds at a time (the iteration
    # over a .card file ran anywhere between 0.66 and 1.05 M blocks/s).  A caller that is done with a
    # collected array hands it back (`recycle`) and the next submit reuses its pages.
    def _records_out(self, nb):
        pool = self.__dict__.setdefault("_out_pool", {})
        spare = pool.get(nb)
        if spare:
            return spare.pop()
        return np.zeros((nb, self.n_templates), dtype=RECORD_DTYPE)

    def recycle(self, records):
        """Hand a collected record array back for reuse by a later submit*() (the caller keeps no view of it)."""
        base = records
        while isinstance(getattr(base, "base", None), np.ndarray):
            base = base.base
        if (isinstance(base, np.ndarray) and base.dtype == RECORD_DTYPE and base.ndim == 2
                and base.shape[1] == self.n_templates and base.flags.c_contiguous and base.flags.owndata):
            spare = self.__dict__.setdefault("_out_pool", {}).setdefault(base.shape[0], [])
            if len(spare) < MAX_IN_FLIGHT + 2:
                spare.append(base)

    def _idx_ptr(self, block_idx, nb):
        if block_idx is None:
            return None, None
        idx = np.ascontiguousarray(np.asarray(block_idx, dtype=np.int64))
        assert idx.shape == (nb,)
        return idx, idx.ctypes.data

    def submit(self, blocks, block_idx=None):
        """thr_submit: like detect() for ONE batch (<= max_batch blocks), but returns a Ticket at
        once; `collect(ticket)` -> records [B, n_templates].  Up to MAX_IN_FLIGHT may be open."""
        a, fmt = self._as_input(blocks)
        nb = a.shape[0]
        out = self._records_out(nb)
        idx, idx_p = self._idx_ptr(block_idx, nb)
        t = C.c_uint64(0)
        _check(self._lib, self._lib.thr_submit(self._h, a.ctypes.data, fmt, idx_p, nb, out.ctypes.data,
                                               C.byref(t)))
        return Ticket(t.value, out, (a, idx))

    def submit_card(self, text, payload_off, block_idx=None):
        """thr_submit_card (see detect_card)."""
        buf = np.frombuffer(text, dtype=np.uint8)
        off = np.ascontiguousarray(np.asarray(payload_off, dtype=np.int64))
        nb = off.shape[0]
        out = self._records_out(nb)
        idx, idx_p = self._idx_ptr(block_idx, nb)
        t = C.c_uint64(0)
        _check(self._lib, self._lib.thr_submit_card(self._h, buf.ctypes.data, buf.size, off.ctypes.data,
                                                    idx_p, nb, out.ctypes.data, C.byref(t)))
        # (`text` itself is NOT kept: a reader's bytearray must stay resizable -- the caller keeps
        # it valid until inputs_consumed() / collect())
        return Ticket(t.value, out, (off, idx))

    def submit_stream(self, stream, first_block_idx=0):
        """thr_submit_stream (see detect_stream)."""
        buf = np.frombuffer(stream, dtype=np.uint8)
        stride = 2 * (self.block_len - self.history_len)
        nb = 0 if buf.size < 2 * self.block_len else (buf.size - 2 * self.block_len) // stride + 1
        out = self._records_out(nb)
        got, t = C.c_size_t(0), C.c_uint64(0)
        _check(self._lib, self._lib.thr_submit_stream(self._h, buf.ctypes.data, buf.size,
                                                      int(first_block_idx), out.ctypes.data, nb,
                                                      C.byref(got), C.byref(t)))
        assert got.value == nb
        return Ticket(t.value, out, None)

    def input_window(self, buf=None, populate_threads=0, segment_bytes=0):
        """thr_input_window[_ex]: declare `buf` (bytes-like: the mmap of the input file, or a slice of
        it) as the range the host entry points will read front to back -- a library thread
        page-locks it a bounded distance ahead of the copies, which then are asynchronous DMA.
        None closes the window.  The caller keeps `buf` alive until then.  populate_threads: the
        page-table populators ahead of the locking (0 = the library's default, 3; a rank of a sharded
        run passes its share of the host, parallel.populate_threads); segment_bytes: the locking
        granularity (0 = 128 MiB; tests)."""
        if buf is None:
            _check(self._lib, self._lib.thr_input_window(self._h, None, 0))
            self._window = None
            return
        if getattr(self, "_window", None) is not None:     # (waits for a released window's unlocking)
            _check(self._lib, self._lib.thr_input_window(self._h, None, 0))
            self._window = None
        arr = np.frombuffer(buf, dtype=np.uint8)
        _check(self._lib, self._lib.thr_input_window_ex(self._h, arr.ctypes.data, arr.size,
                                                        int(populate_threads), int(segment_bytes)))
        self._window = arr

    def input_window_release(self):
        """thr_input_window_release: the input has been read -- stop locking, unlock what is still
        locked in the background, return at once.  This object keeps the buffer alive until the
        window is really closed (input_window(None), a new window, or close())."""
        self._lib.thr_input_window_release.argtypes = [C.c_void_p]
        _check(self._lib, self._lib.thr_input_window_release(self._h))

    # ---- the whole file -> .toad loop inside the library (thr_run_card / thr_run_stream) -------
    def _run_opts(self, out_fd, rxid, with_txid, carrier_offset_mode, batch_blocks, rec_out, timestamp=None):
        o = ThrRunOpts()
        o.struct_bytes = C.sizeof(ThrRunOpts)
        o.batch_blocks = int(batch_blocks or 0)
        o.out_fd = -1 if out_fd is None else int(out_fd)
        o.with_rxid, o.rxid = (0, 0) if rxid is None else (1, int(rxid))
        o.with_txid = int(bool(with_txid))
        o.carrier_offset_mode = int(carrier_offset_mode)
        o.timestamp = float("nan") if timestamp is None else float(timestamp)
        if rec_out is not None:
            assert rec_out.dtype == RECORD_DTYPE and rec_out.flags.c_contiguous
            o.rec_out, o.rec_capacity = rec_out.ctypes.data, rec_out.size
        return o

    def _run_done(self, rc, stats):
        """-> stats dict; THR_ERR_INDEX is reported in it (`index_error`), everything else raises."""
        out = stats.as_dict()
        out["index_error"] = rc == ERR_INDEX
        if rc != 0 and rc != ERR_INDEX:
            raise NativeError("libthriftyhip: %s (code %d)" % (self._lib.thr_last_error().decode(), rc),
                              rc, out)
        return out

    def _run(self, data, call):
        """One whole-input call: `call(pointer, n_bytes, stats)` -> rc, over the bytes-like `data` -> _run_done."""
        buf = np.frombuffer(data, dtype=np.uint8)
        st = ThrRunStats()
        rc = call(buf.ctypes.data if buf.size else None, buf.size, C.byref(st))
        del buf
        return self._run_done(rc, st)

    def run_card(self, text, out_fd=None, rxid=None, with_txid=False, carrier_offset_mode=0,
                 batch_blocks=0, rec_out=None):
        """thr_run_card: frame, detect and format the .card text `text` (bytes-like: the mapped
        file) inside the library; the .toad text goes to the descriptor `out_fd`, the detected
        records (timestamp bits in `reserved`) into `rec_out` (a RECORD_DTYPE array) if given.
        -> stats dict (blocks, detections, seconds per stage, `index_error` ...)."""
        o = self._run_opts(out_fd, rxid, with_txid, carrier_offset_mode, batch_blocks, rec_out)
        return self._run(text, lambda ptr, n, st: self._lib.thr_run_card(self._h, ptr, n, C.byref(o), st))

    def run_stream(self, stream, first_block_idx=0, out_fd=None, rxid=None, with_txid=False,
                   carrier_offset_mode=0, batch_blocks=0, rec_out=None, timestamp=None):
        """thr_run_stream: the same for a raw u8 I/Q stream whose first 2 * block_len bytes are
        block `first_block_idx` (overlap framing on the device)."""
        o = self._run_opts(out_fd, rxid, with_txid, carrier_offset_mode, batch_blocks, rec_out, timestamp)
        return self._run(stream, lambda ptr, n, st: self._lib.thr_run_stream(self._h, ptr, n, int(first_block_idx),
                                                                             C.byref(o), st))

    def debug_window(self):
        """thr_debug_window -> (released_below, locked_lo, locked_hi, segment_bytes), byte offsets
        from the window's page-aligned start (test hook)."""
        out = (C.c_size_t * 4)()
        self._lib.thr_debug_window.argtypes = [C.c_void_p, C.c_size_t * 4]
        _check(self._lib, self._lib.thr_debug_window(self._h, out))
        return tuple(int(v) for v in out)

    def correlate_geom(self):
        """thr_debug_correlate_geom -> (rows_lo, rows_hi) of the window-row specialisation this
        handle's correlate launches take, or (-1, -1): the generic kernel."""
        lo, hi = C.c_int(-1), C.c_int(-1)
        self._lib.thr_debug_correlate_geom.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _check(self._lib, self._lib.thr_debug_correlate_geom(self._h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def path_info(self):
        """thr_get_path_info -> dict: which kernels this handle's plain launches take and why
        (`why_unsectioned` is one of WHY_UNSECTIONED; `text` says the same as one sentence)."""
        info = ThrPathInfo()
        self._lib.thr_get_path_info.argtypes = [C.c_void_p, C.POINTER(ThrPathInfo)]
        _check(self._lib, self._lib.thr_get_path_info(self._h, C.byref(info)))
        return {"n_sections": info.n_sections, "section_len": info.section_len,
                "rows": (info.rows_lo, info.rows_hi), "why_unsectioned": WHY_UNSECTIONED[info.why_unsectioned],
                "n_templates": info.n_templates, "carrier_kernel": info.carrier_kernel.decode(),
                "correlate_kernel": info.correlate_kernel.decode(), "text": info.text.decode()}

    def sections(self):
        """thr_debug_sections -> (n_sections, section_len) of this handle's plain correlate launches
        ((0, 0): unsectioned)."""
        n, ln = C.c_int(0), C.c_int(0)
        self._lib.thr_debug_sections.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _check(self._lib, self._lib.thr_debug_sections(self._h, C.byref(n), C.byref(ln)))
        return n.value, ln.value

    def section_counts(self):
        """thr_debug_section_counts -> (computed, skipped): the (block, section) items the one-template
        section kernel has searched / left out by its energy bound since the last call (reads and zeroes)."""
        done, skipped = C.c_longlong(0), C.c_longlong(0)
        self._lib.thr_debug_section_counts.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        _check(self._lib, self._lib.thr_debug_section_counts(self._h, C.byref(done), C.byref(skipped)))
        return done.value, skipped.value

    def debug_pipe_times(self):
        """thr_debug_pipe_times -> seconds per phase of the host entry points' chunks (reads and resets)."""
        out = (C.c_double * 16)()
        self._lib.thr_debug_pipe_times.argtypes = [C.c_void_p, C.c_double * 16]
        _check(self._lib, self._lib.thr_debug_pipe_times(self._h, out))
        keys = ("grow_s", "h2d_s", "meta_s", "launch_s", "d2h_s", "chunks", "event_s", "fill_s")
        res = dict(zip(keys, (float(v) for v in out[:8])))
        res.update(("max_" + k, float(v)) for k, v in zip(keys, out[8:]) if k != "chunks")
        return res

    def debug_window_times(self):
        """thr_debug_window_times -> dict of seconds per activity of the input window's threads."""
        out = (C.c_double * 6)()
        self._lib.thr_debug_window_times.argtypes = [C.c_void_p, C.c_double * 6]
        _check(self._lib, self._lib.thr_debug_window_times(self._h, out))
        keys = ("populate_s", "register_s", "unregister_s", "acquire_wait_s", "acquire_waits", "pageable_copies")
        return dict(zip(keys, (float(v) for v in out)))

    def set_wait_mode(self, sleeping):
        """thr_set_wait_mode: True = collect() naps between queries of the batch's event instead of
        polling it (a CPU per rank saved on hosts shared by several ranks)."""
        self._lib.thr_set_wait_mode.argtypes = [C.c_void_p, C.c_int]
        _check(self._lib, self._lib.thr_set_wait_mode(self._h, int(bool(sleeping))))

    def collect(self, ticket):
        """thr_collect: wait for the ticket's batch -> its records [B, n_templates]."""
        _check(self._lib, self._lib.thr_collect(self._h, ticket.id))
        ticket.keep = None
        return ticket.out

    def inputs_consumed(self, ticket):
        """thr_inputs_consumed: wait until the ticket's input arrays may be overwritten."""
        _check(self._lib, self._lib.thr_inputs_consumed(self._h, ticket.id))
        ticket.keep = None

    def poll(self, ticket):
        done = C.c_int(0)
        _check(self._lib, self._lib.thr_poll(self._h, ticket.id, C.byref(done)))
        return bool(done.value)

    # ---- device-resident path (pointers are plain integers) ---------------
    def detect_stream_device(self, d_stream, n_blocks, d_out, d_block_idx=None):
        _check(self._lib, self._lib.thr_detect_stream_device(self._h, d_stream, d_block_idx,
                                                             n_blocks, d_out))

    def detect_device(self, d_samples, fmt, n_blocks, d_out, d_block_idx=None):
        _check(self._lib, self._lib.thr_detect_device(self._h, d_samples, fmt, d_block_idx,
                                                      n_blocks, d_out))

    def compact_device(self, d_in, n_records, d_out):
        kept = C.c_size_t(0)
        _check(self._lib, self._lib.thr_compact_device(self._h, d_in, n_records, d_out,
                                                       C.byref(kept)))
        return kept.value

    def sync(self):
        _check(self._lib, self._lib.thr_sync(self._h))

    def set_stream(self, stream_ptr):
        """Run on the caller's HIP stream.  0 / None -- the handle value of torch's DEFAULT stream
        -- selects the device's legacy default stream (ordered with torch's fills and copies
        there); `use_own_stream()` goes back to the engine's private non-blocking stream."""
        if not stream_ptr:
            _check(self._lib, self._lib.thr_set_stream_default(self._h))
        else:
            _check(self._lib, self._lib.thr_set_stream(self._h, stream_ptr))

    def use_own_stream(self):
        _check(self._lib, self._lib.thr_set_stream(self._h, None))

    def profile_enable(self, every=1):
        """every = n > 0: time the kernels of every n-th batch; 0/False: off."""
        _check(self._lib, self._lib.thr_profile_enable(self._h, int(every)))

    def profile_read(self):
        ms = (C.c_double * N_KERNEL_SLOTS)()
        cnt = (C.c_int64 * N_KERNEL_SLOTS)()
        _check(self._lib, self._lib.thr_profile_read(self._h, ms, cnt))
        return {self._lib.thr_kernel_name(i).decode(): (ms[i], cnt[i])
                for i in range(N_KERNEL_SLOTS)}

    # ---- test hooks ------------------------------------------------------
    def debug_fft(self, blocks):
        a, fmt = self._as_input(blocks)
        out = np.zeros((a.shape[0], self.block_len), dtype=np.complex64)
        _check(self._lib, self._lib.thr_debug_fft(self._h, a.ctypes.data, fmt, a.shape[0],
                                                  out.ctypes.data))
        return out

    def debug_stage(self, blocks, template_id=0, carrier_offset=None):
        a, fmt = self._as_input(blocks)
        xhat = np.zeros((a.shape[0], self.block_len), dtype=np.complex64)
        corr = np.zeros((a.shape[0], self.block_len), dtype=np.complex64)
        off = None
        if carrier_offset is not None:
            off = np.ascontiguousarray(carrier_offset, dtype=np.float64)
            if off.shape != (a.shape[0],):
                raise ValueError("carrier_offset: one value per block")
        _check(self._lib, self._lib.thr_debug_stage_offsets(self._h, a.ctypes.data, fmt, a.shape[0],
                                                            template_id, off.ctypes.data if off is not None else None,
                                                            xhat.ctypes.data, corr.ctypes.data))
        return xhat, corr


class Extraction(object):
    """A template extraction riding on an Engine (thr_extract_*): feed it the blocks of a capture in any
    batching, through any of the engine's input forms, then take `result()`.  The engine must be the
    default single-template detector and must stay open while this object is."""

    def __init__(self, engine, max_offset=0.2):
        self._lib, self._eng = engine._lib, engine
        self.max_offset = float(max_offset)
        x = C.c_void_p()
        _check(self._lib, self._lib.thr_extract_create(engine._h, self.max_offset, C.byref(x)))
        self._x = x

    def close(self):
        if getattr(self, "_x", None):
            if getattr(self._eng, "_h", None):      # (an engine that is gone took the device state with it)
                self._lib.thr_extract_destroy(self._x)
            self._x = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def reset(self):
        _check(self._lib, self._lib.thr_extract_reset(self._x))

    @staticmethod
    def _stamps(timestamps, nb):
        if timestamps is None:
            return None, None
        ts = np.ascontiguousarray(np.asarray(timestamps, dtype=np.float64))
        assert ts.shape == (nb,)
        return ts, ts.ctypes.data

    def feed(self, blocks, timestamps=None, block_idx=None):
        """thr_extract_feed: u8 [B, 2N] or complex64 [B, N] blocks -> the batch's records [B]."""
        eng = self._eng
        a, fmt = eng._as_input(blocks)
        nb = a.shape[0]
        out = np.zeros(nb, dtype=RECORD_DTYPE)
        idx, idx_p = eng._idx_ptr(block_idx, nb)
        ts, ts_p = self._stamps(timestamps, nb)
        _check(self._lib, self._lib.thr_extract_feed(self._x, a.ctypes.data, fmt, idx_p, ts_p, nb, out.ctypes.data))
        return out

    def feed_card(self, text, payload_off, timestamps=None, block_idx=None):
        """thr_extract_feed_card: .card text + payload offsets (see Engine.detect_card) -> records [B]."""
        buf = np.frombuffer(text, dtype=np.uint8)
        off = np.ascontiguousarray(np.asarray(payload_off, dtype=np.int64))
        nb = off.shape[0]
        out = np.zeros(nb, dtype=RECORD_DTYPE)
        idx, idx_p = self._eng._idx_ptr(block_idx, nb)
        ts, ts_p = self._stamps(timestamps, nb)
        _check(self._lib, self._lib.thr_extract_feed_card(self._x, buf.ctypes.data, buf.size, off.ctypes.data, idx_p,
                                                          ts_p, nb, out.ctypes.data))
        return out

    def feed_stream(self, stream, first_block_idx=0, timestamps=None):
        """thr_extract_feed_stream: raw u8 I/Q bytes, overlapping blocks framed on the device (see
        Engine.detect_stream) -> records [n_whole_blocks]."""
        eng = self._eng
        buf = np.frombuffer(stream, dtype=np.uint8)
        stride = 2 * (eng.block_len - eng.history_len)
        nb = 0 if buf.size < 2 * eng.block_len else (buf.size - 2 * eng.block_len) // stride + 1
        out = np.zeros(nb, dtype=RECORD_DTYPE)
        ts, ts_p = self._stamps(timestamps, nb)
        got = C.c_size_t(0)
        _check(self._lib, self._lib.thr_extract_feed_stream(self._x, buf.ctypes.data if buf.size else None, buf.size,
                                                            int(first_block_idx), ts_p, out.ctypes.data, max(1, nb),
                                                            C.byref(got)))
        assert got.value == nb
        return out

    def run(self, data, card=True, first_block_idx=0, timestamp=None, batch_blocks=0, out_fd=None, rxid=None,
            rec_out=None):
        """thr_run_extract_card / thr_run_extract_stream: the whole input `data` (bytes-like: the mapped
        .card file, or a raw stream whose first 2 * block_len bytes are block `first_block_idx`) inside
        the library.  -> the statistics as a dict (`index_error`: the run ended at the reference's
        IndexError block)."""
        eng = self._eng
        o = eng._run_opts(out_fd, rxid, False, 0, batch_blocks, rec_out, timestamp)
        if card:
            return eng._run(data, lambda ptr, n, st: self._lib.thr_run_extract_card(eng._h, ptr, n, C.byref(o),
                                                                                    self._x, st))
        return eng._run(data, lambda ptr, n, st: self._lib.thr_run_extract_stream(
            eng._h, ptr, n, int(first_block_idx), C.byref(o), self._x, st))

    def result(self, template_len):
        """thr_extract_result -> (record, timestamp, template float64[template_len], n_qualifying).
        ValueError (with the library's sentence) if no record has qualified."""
        rec = np.zeros(1, dtype=RECORD_DTYPE)
        ts, n = C.c_double(0), C.c_uint64(0)
        out = np.empty(int(template_len), dtype=np.float64)
        rc = self._lib.thr_extract_result(self._x, rec.ctypes.data, C.byref(ts), out.ctypes.data, out.size, C.byref(n))
        if rc == ERR_STATE:
            raise ValueError(self._lib.thr_last_error().decode())
        _check(self._lib, rc)
        return rec[0], ts.value, out, n.value

    def average(self, classes=()):
        """thr_extract_average: arm averaging before the first feed.  `classes`: a sequence of (lo, hi) ranges of
        carrier_bin + carrier_offset (inclusive, the last match wins), empty: one class of every qualifying
        record; None disarms."""
        if classes is None:
            _check(self._lib, self._lib.thr_extract_average(self._x, None))
            self.n_classes = None
            return
        classes = [(float(lo), float(hi)) for lo, hi in classes]
        if len(classes) > AVERAGE_MAX_CLASSES:
            raise ValueError("an extraction averages at most %d classes, %d given" % (AVERAGE_MAX_CLASSES, len(classes)))
        o = ThrAverageOpts()
        o.n_classes = len(classes)
        for k, (lo, hi) in enumerate(classes):
            o.lo[k], o.hi[k] = lo, hi
        _check(self._lib, self._lib.thr_extract_average(self._x, C.byref(o)))
        self.n_classes = len(classes)

    def average_counts(self):
        """thr_extract_average_counts -> (count uint64[16], n_unclassified)."""
        count = np.zeros(AVERAGE_MAX_CLASSES, dtype=np.uint64)
        n = C.c_uint64(0)
        _check(self._lib, self._lib.thr_extract_average_counts(self._x, count.ctypes.data, C.byref(n)))
        return count, n.value

    def average_result(self, k, template_len):
        """thr_extract_average_result of class `k` -> (template, sem float64[W], acc_e, acc_q uint64[W]).
        ValueError (with the library's sentence) if no record of the class has qualified."""
        w = int(template_len)
        tpl, sem = np.empty(w, dtype=np.float64), np.empty(w, dtype=np.float64)
        acc_e, acc_q = np.zeros(w, dtype=np.uint64), np.zeros(w, dtype=np.uint64)
        rc = self._lib.thr_extract_average_result(self._x, int(k), tpl.ctypes.data, sem.ctypes.data, w,
                                                  acc_e.ctypes.data, acc_q.ctypes.data)
        if rc == ERR_STATE:
            raise ValueError(self._lib.thr_last_error().decode())
        _check(self._lib, rc)
        return tpl, sem, acc_e, acc_q


class Dossiers(object):
    """Detection dossiers riding on an Engine (thr_dossier_*): feed it the blocks of a capture in any batching,
    through any of the engine's input forms; the first `max_keep` blocks that are detected and whose index lies
    in one of `ranges` ((lo, hi) closed, None = open) are kept on the device.  `result()` then returns, per kept
    block, what the reference's analyze_detect derives from it.  Every feed returns the batch's records and
    updates `n_kept`, `n_checked`, `n_skipped`.  The engine must be the default single-template detector."""

    def __init__(self, engine, ranges=((None, None),), max_keep=20):
        self._lib, self._eng = engine._lib, engine
        flat = np.array([[-2**63 if lo is None else int(lo), 2**63 - 1 if hi is None else int(hi)]
                         for lo, hi in ranges], dtype=np.int64).reshape(-1, 2)
        self.max_keep = int(max_keep)
        self.n_kept = self.n_checked = self.n_skipped = 0
        d = C.c_void_p()
        _check(self._lib, self._lib.thr_dossier_create(engine._h, flat.ctypes.data if flat.size else None,
                                                       flat.shape[0], self.max_keep, C.byref(d)))
        self._d = d
        geo = (C.c_int64 * 4)()
        _check(self._lib, self._lib.thr_dossier_geometry(d, geo))
        self.filter_width, self.filtered_len, self.corr_len, self.chunk_blocks = (int(v) for v in geo)

    def close(self):
        if getattr(self, "_d", None):
            if getattr(self._eng, "_h", None):      # (an engine that is gone took the device state with it)
                self._lib.thr_dossier_destroy(self._d)
            self._d = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def full(self):
        return self.n_kept >= self.max_keep

    def reset(self):
        _check(self._lib, self._lib.thr_dossier_reset(self._d))
        self.n_kept = self.n_checked = self.n_skipped = 0

    def _counts(self):
        k, c, s = C.c_size_t(0), C.c_uint64(0), C.c_uint64(0)
        return (k, c, s), (C.byref(k), C.byref(c), C.byref(s))

    def _done(self, rc, counts):
        _check(self._lib, rc)
        self.n_kept, self.n_checked, self.n_skipped = (int(v.value) for v in counts)

    def feed(self, blocks, timestamps=None, block_idx=None):
        """thr_dossier_feed: u8 [B, 2N] or complex64 [B, N] blocks -> the batch's records [B]."""
        eng = self._eng
        a, fmt = eng._as_input(blocks)
        nb = a.shape[0]
        out = np.zeros(nb, dtype=RECORD_DTYPE)
        idx, idx_p = eng._idx_ptr(block_idx, nb)
        ts, ts_p = Extraction._stamps(timestamps, nb)
        counts, refs = self._counts()
        self._done(self._lib.thr_dossier_feed(self._d, a.ctypes.data, fmt, idx_p, ts_p, nb, out.ctypes.data, *refs),
                   counts)
        return out

    def feed_card(self, text, payload_off, timestamps=None, block_idx=None):
        """thr_dossier_feed_card: .card text + payload offsets (see Engine.detect_card) -> records [B]."""
        buf = np.frombuffer(text, dtype=np.uint8)
        off = np.ascontiguousarray(np.asarray(payload_off, dtype=np.int64))
        nb = off.shape[0]
        out = np.zeros(nb, dtype=RECORD_DTYPE)
        idx, idx_p = self._eng._idx_ptr(block_idx, nb)
        ts, ts_p = Extraction._stamps(timestamps, nb)
        counts, refs = self._counts()
        self._done(self._lib.thr_dossier_feed_card(self._d, buf.ctypes.data, buf.size, off.ctypes.data, idx_p, ts_p,
                                                   nb, out.ctypes.data, *refs), counts)
        return out

    def feed_stream(self, stream, first_block_idx=0, timestamps=None):
        """thr_dossier_feed_stream: raw u8 I/Q bytes, overlapping blocks framed on the device -> records."""
        eng = self._eng
        buf = np.frombuffer(stream, dtype=np.uint8)
        stride = 2 * (eng.block_len - eng.history_len)
        nb = 0 if buf.size < 2 * eng.block_len else (buf.size - 2 * eng.block_len) // stride + 1
        out = np.zeros(nb, dtype=RECORD_DTYPE)
        ts, ts_p = Extraction._stamps(timestamps, nb)
        got = C.c_size_t(0)
        counts, refs = self._counts()
        self._done(self._lib.thr_dossier_feed_stream(self._d, buf.ctypes.data if buf.size else None, buf.size,
                                                     int(first_block_idx), ts_p, out.ctypes.data, max(1, nb),
                                                     C.byref(got), *refs), counts)
        assert got.value == nb
        return out

    def result(self, first=0, count=None, arrays=DOSSIER_ARRAYS):
        """thr_dossier_result for the slots [first, first + count) -> dict: records, timestamps, positions,
        autocorr (float64 [17]) and the arrays asked for (hist uint32 [K, 256], fft_mag / synced_fft_mag
        float32 [K, N], filtered float32 [K, N - F/2], synced complex64 [K, N], corr complex64 [K, corr_len],
        scalars DOSSIER_SCALARS_DTYPE [K])."""
        total = C.c_size_t(0)
        _check(self._lib, self._lib.thr_dossier_result(self._d, 0, 0, None, C.byref(total)))
        first = int(first)
        k = max(0, min(total.value - first, total.value if count is None else int(count)))
        n = self._eng.block_len
        shapes = {"hist": ((k, 256), np.uint32), "fft_mag": ((k, n), np.float32),
                  "filtered": ((k, self.filtered_len), np.float32), "synced": ((k, n), np.complex64),
                  "synced_fft_mag": ((k, n), np.float32), "corr": ((k, self.corr_len), np.complex64),
                  "scalars": ((k,), DOSSIER_SCALARS_DTYPE)}
        res = {"records": np.zeros(k, dtype=RECORD_DTYPE), "timestamps": np.zeros(k), "positions": np.zeros(k, np.uint64),
               "autocorr": np.zeros(17)}
        for name in arrays:
            res[name] = np.zeros(*shapes[name])
        if k:
            o = ThrDossierOut()
            for name, a in res.items():
                setattr(o, name, a.ctypes.data)
            _check(self._lib, self._lib.thr_dossier_result(self._d, first, k, C.byref(o), None))
        return res


class Survey(object):
    """A capture survey riding on an Engine (thr_survey_*): feed it the u8 blocks of a capture in any
    batching; every call returns the intervals of `integrate` blocks it completed, as integers
    (spec_sum uint64 [J, N], hist uint64 [J, 256]) with the fed blocks' byte sums (uint64 [B, 2]).  The
    open interval stays on the device.  Any engine will do (Engine.gate builds no template spectra); it
    must stay open while this object is."""

    def __init__(self, engine, integrate=100):
        self._lib, self._eng = engine._lib, engine
        self.integrate = int(integrate)
        s = C.c_void_p()
        _check(self._lib, self._lib.thr_survey_create(engine._h, self.integrate, C.byref(s)))
        self._s = s
        shift = C.c_int(0)
        _check(self._lib, self._lib.thr_survey_shift(self._s, C.byref(shift)))
        self.shift = shift.value

    def close(self):
        if getattr(self, "_s", None):
            if getattr(self._eng, "_h", None):      # (an engine that is gone took the device state with it)
                self._lib.thr_survey_destroy(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def reset(self):
        _check(self._lib, self._lib.thr_survey_reset(self._s))

    def pending(self):
        """-> (blocks fed since the reset, blocks waiting in the open interval)"""
        fed, waiting = C.c_uint64(0), C.c_uint64(0)
        _check(self._lib, self._lib.thr_survey_pending(self._s, C.byref(fed), C.byref(waiting)))
        return fed.value, waiting.value

    def geometry(self):
        """thr_debug_survey_geometry -> (blocks per tile, workgroups, fused kernel?)"""
        tile, wgs, fused = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(self._lib, self._lib.thr_debug_survey_geometry(self._s, C.byref(tile), C.byref(wgs), C.byref(fused)))
        return tile.value, wgs.value, bool(fused.value)

    def _out(self, nb, cap_intervals):
        cap = (self.pending()[1] + nb) // self.integrate if cap_intervals is None else int(cap_intervals)
        n = self._eng.block_len
        return (cap, np.zeros((nb, 2), dtype=np.uint64), np.zeros((max(1, cap), n), dtype=np.uint64),
                np.zeros((max(1, cap), 256), dtype=np.uint64))

    def feed(self, blocks, cap_intervals=None):
        """thr_survey_feed: u8 [B, 2N] packed blocks -> (spec_sum [J, N], hist [J, 256], sums [B, 2]).
        u8 only: anything else is refused like the library refuses a bad argument."""
        a = np.asarray(blocks)
        if a.dtype != np.uint8:
            raise NativeError("Survey.feed: the survey takes raw u8 blocks, not %s (code %d)" % (a.dtype, ERR_ARG), ERR_ARG)
        a = np.ascontiguousarray(a).reshape(-1, 2 * self._eng.block_len)
        nb = a.shape[0]
        cap, sums, spec, hist = self._out(nb, cap_intervals)
        got = C.c_size_t(0)
        _check(self._lib, self._lib.thr_survey_feed(self._s, a.ctypes.data if nb else None, nb, sums.ctypes.data,
                                                    spec.ctypes.data, hist.ctypes.data, cap, C.byref(got)))
        return spec[:got.value], hist[:got.value], sums

    def feed_stream(self, stream, cap_intervals=None):
        """thr_survey_feed_stream: raw u8 I/Q bytes, overlapping blocks framed on the device (see
        Engine.detect_stream) -> (spec_sum, hist, sums [n_whole_blocks, 2])."""
        eng = self._eng
        buf = np.frombuffer(stream, dtype=np.uint8)
        stride = 2 * (eng.block_len - eng.history_len)
        nb = 0 if buf.size < 2 * eng.block_len else (buf.size - 2 * eng.block_len) // stride + 1
        cap, sums, spec, hist = self._out(nb, cap_intervals)
        got, framed = C.c_size_t(0), C.c_size_t(0)
        _check(self._lib, self._lib.thr_survey_feed_stream(self._s, buf.ctypes.data if buf.size else None, buf.size,
                                                           sums.ctypes.data, nb, C.byref(framed), spec.ctypes.data,
                                                           hist.ctypes.data, cap, C.byref(got)))
        assert framed.value == nb
        return spec[:got.value], hist[:got.value], sums


class ChipScan(object):
    """The chip-rate scan riding on an Engine (thr_chipscan): blocks x candidate template lengths.  The
    engine is an ordinary one with block_len 16384; its own template plays no part, its carrier settings
    do.  It must stay open while this object is used; the scan's device buffers are the engine's."""

    def __init__(self, engine):
        self._lib, self._eng = engine._lib, engine

    def close(self):
        self._eng = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def scan(self, blocks, chips, lengths, with_carrier=False):
        """blocks: u8 [B, 2N] or complex64 [B, N]; chips: 0 / 1 per chip; lengths: int32 [K] in any order
        -> CHIP_RECORD_DTYPE records [B, K] in the order of `lengths` (and the blocks' carrier records,
        RECORD_DTYPE [B], if with_carrier)."""
        a, fmt = self._eng._as_input(blocks)
        nb = a.shape[0]
        c = np.ascontiguousarray(np.asarray(chips)).astype(np.uint8).reshape(-1)
        lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int32)).reshape(-1)
        out = np.zeros((nb, lens.size), dtype=CHIP_RECORD_DTYPE)
        car = np.zeros(nb, dtype=RECORD_DTYPE) if with_carrier else None
        _check(self._lib, self._lib.thr_chipscan(self._eng._h, a.ctypes.data if nb else None, fmt, nb,
                                                 c.ctypes.data if c.size else None, c.size,
                                                 lens.ctypes.data if lens.size else None, lens.size,
                                                 out.ctypes.data if out.size else None,
                                                 car.ctypes.data if with_carrier and nb else None))
        return (out, car) if with_carrier else out

    def geometry(self, n_lengths):
        """thr_debug_chipscan_geometry -> (candidates per chunk of the template bank, lengths paired?)"""
        per, paired = C.c_int(0), C.c_int(0)
        _check(self._lib, self._lib.thr_debug_chipscan_geometry(self._eng._h, int(n_lengths), C.byref(per),
                                                                C.byref(paired)))
        return per.value, bool(paired.value)

    def set_bank_budget(self, n_bytes):
        """thr_debug_chipscan_budget: bytes of template bank per chunk (0: the default)"""
        _check(self._lib, self._lib.thr_debug_chipscan_budget(self._eng._h, int(n_bytes)))

    def set_fill(self, workgroups):
        """thr_debug_chipscan_fill: workgroups a scan launch aims at (0: the default, twice the CUs)"""
        _check(self._lib, self._lib.thr_debug_chipscan_fill(self._eng._h, int(workgroups)))

    def groups(self, n_blocks, n_cand):
        """thr_debug_chipscan_groups -> (groups per block, candidates per group) of one launch"""
        groups, per = C.c_int(0), C.c_int(0)
        _check(self._lib, self._lib.thr_debug_chipscan_groups(self._eng._h, int(n_blocks), int(n_cand),
                                                              C.byref(groups), C.byref(per)))
        return groups.value, per.value

    def times(self):
        """thr_debug_chipscan_times -> device ms of the last scan: (carrier stage, bank kernel, scan kernels)"""
        ms = (C.c_double * 3)()
        _check(self._lib, self._lib.thr_debug_chipscan_times(self._eng._h, ms))
        return tuple(ms)


TDOA_TASKS_PER_WORKGROUP = 4    # kWaves of csrc/tdoa.hip: one wavefront per task, four to a workgroup
TDOA_LDS_WINDOW = 256           # kLdsWindow: longer windows are ranked from the columns instead of LDS
TDOA_MODELS = {"poly": 0, "weighted_poly": 1, "nearest": 2, "linear": 3}      # THR_TDOA_*


def tdoa(rx, timestamp, soa, energy, noise, match_ptr, match_idx, match_beacon, dist, window, sample_rate,
         deg=2, device_id=0, model=0):
    """thr_tdoa_model (`model`: a TDOA_MODELS code; None: the older entry point thr_tdoa, the polynomial) on
    detection columns (rx: dense receiver index), the matches as CSR, the beacon index of
    every match (-1: mobile) and dist[receiver][beacon] -> dict of row_rx int32[r, 2] (dense),
    row_det int64[r, 2], tdoa / snr / model_quality float64[r], group_id int64[g], group_ptr int64[g + 1],
    failures int64[f, 2], n_window / n_kept int32[tasks], picks int32[tasks, 2] (positions in the kept list:
    {idx, -1} nearest, {low, high} linear, else -1).  ValueError for what thr_tdoa_model refuses."""
    lib = load_library()
    cols = [np.ascontiguousarray(rx, dtype=np.int32)] + [np.ascontiguousarray(c, dtype=np.float64)
                                                          for c in (timestamp, soa, energy, noise)]
    if len(set(len(c) for c in cols)) != 1:
        raise ValueError("tdoa: the detection columns differ in length")
    ptr = np.ascontiguousarray(match_ptr, dtype=np.int64)
    idx = np.ascontiguousarray(match_idx, dtype=np.int64)
    beacon = np.ascontiguousarray(match_beacon, dtype=np.int32)
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    if ptr.ndim != 1 or len(ptr) != len(beacon) + 1 or dist.ndim != 2 or (len(ptr) and int(ptr[-1]) != len(idx)):
        raise ValueError("tdoa: match_ptr, match_idx, match_beacon or dist have the wrong shape")
    k = np.diff(ptr)
    n_tasks = int((k * (k - 1) // 2)[beacon < 0].sum())
    n_matches = len(beacon)
    row_rx = np.zeros((n_tasks, 2), dtype=np.int32)
    row_det = np.zeros((n_tasks, 2), dtype=np.int64)
    row_val = np.zeros((n_tasks, 3), dtype=np.float64)
    fail = np.zeros((n_tasks, 2), dtype=np.int64)
    group_id = np.zeros(n_matches, dtype=np.int64)
    group_ptr = np.zeros(n_matches + 1, dtype=np.int64)
    n_window = np.zeros(n_tasks, dtype=np.int32)
    n_kept = np.zeros(n_tasks, dtype=np.int32)
    picks = np.full((n_tasks, 2), -1, dtype=np.int32)
    n_rows, n_groups, n_fail = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    args = [int(device_id), len(cols[0])] + [c.ctypes.data for c in cols] + [
        n_matches, ptr.ctypes.data, idx.ctypes.data, beacon.ctypes.data, dist.shape[0], dist.shape[1], dist.ctypes.data,
        float(window), float(sample_rate), int(deg), n_tasks, row_rx.ctypes.data, row_det.ctypes.data,
        row_val.ctypes.data, C.byref(n_rows), group_id.ctypes.data, group_ptr.ctypes.data, C.byref(n_groups),
        fail.ctypes.data, C.byref(n_fail), n_window.ctypes.data, n_kept.ctypes.data]
    rc = lib.thr_tdoa(*args) if model is None else lib.thr_tdoa_model(*(args + [int(model), picks.ctypes.data]))
    if rc == ERR_ARG:
        raise ValueError(lib.thr_last_error().decode())
    _check(lib, rc)
    r, g = n_rows.value, n_groups.value
    return {"row_rx": row_rx[:r], "row_det": row_det[:r], "tdoa": row_val[:r, 0].copy(), "snr": row_val[:r, 1].copy(),
            "model_quality": row_val[:r, 2].copy(), "group_id": group_id[:g], "group_ptr": group_ptr[:g + 1],
            "failures": fail[:n_fail.value], "n_window": n_window, "n_kept": n_kept, "picks": picks}


def tdoa_times():
    """{copies in, kernels, copies out} of this thread's last tdoa(), milliseconds (HIP events)."""
    lib = load_library()
    ms = (C.c_double * 3)()
    _check(lib, lib.thr_debug_tdoa_times(ms))
    return tuple(ms)


POS_GROUPS_PER_WORKGROUP = 32   # kTeams of csrc/pos.hip: one 8-lane team per group
POS_REGISTER_ROWS = 4           # kRegRows: rows per lane held in registers; groups over 32 rows re-read theirs
POS_MAX_RECEIVERS = 64          # kMaxReceivers
POS_OK, POS_UNDERDETERMINED, POS_UNCONVERGED, POS_AT_BOUND, POS_NONFINITE = range(5)      # THR_POS_*


def pos(group_ptr, row_rx0, row_rx1, row_tdoa, row_snr, rx_coords, first_two_rx=(0, 1), x0=(0.1, 0.1), max_iter=100,
        device_id=0):
    """thr_pos on TDOA rows in CSR form (group g: rows group_ptr[g]:group_ptr[g + 1]; row_rx0 / row_rx1:
    dense indices into rx_coords[n_rx, dims]) -> dict of pos float64[g, dims], dop / snr float64[g],
    status / iters int32[g], every group in order.  ValueError for what thr_pos refuses."""
    lib = load_library()
    ptr = np.ascontiguousarray(group_ptr, dtype=np.int64)
    rx0, rx1 = np.ascontiguousarray(row_rx0, dtype=np.int32), np.ascontiguousarray(row_rx1, dtype=np.int32)
    tdoa, snr = np.ascontiguousarray(row_tdoa, dtype=np.float64), np.ascontiguousarray(row_snr, dtype=np.float64)
    xy = np.ascontiguousarray(rx_coords, dtype=np.float64)
    if ptr.ndim != 1 or len(ptr) < 1 or xy.ndim != 2 or not (len(rx0) == len(rx1) == len(tdoa) == len(snr) == int(ptr[-1])):
        raise ValueError("pos: group_ptr, the row columns or rx_coords have the wrong shape")
    first = np.ascontiguousarray(first_two_rx, dtype=np.int32)
    start = np.ascontiguousarray(x0, dtype=np.float64)
    if first.shape != (2,) or start.shape != (2,):
        raise ValueError("pos: first_two_rx and x0 hold two values each")
    n, dims = len(ptr) - 1, xy.shape[1]
    out = {"pos": np.zeros((n, dims), dtype=np.float64), "dop": np.zeros(n, dtype=np.float64),
           "snr": np.zeros(n, dtype=np.float64), "status": np.zeros(n, dtype=np.int32), "iters": np.zeros(n, dtype=np.int32)}
    rc = lib.thr_pos(int(device_id), n, ptr.ctypes.data, rx0.ctypes.data, rx1.ctypes.data, tdoa.ctypes.data,
                     snr.ctypes.data, xy.shape[0], dims, xy.ctypes.data, first.ctypes.data, start.ctypes.data,
                     int(max_iter), *[out[key].ctypes.data for key in ("pos", "dop", "snr", "status", "iters")])
    if rc == ERR_ARG:
        raise ValueError(lib.thr_last_error().decode())
    _check(lib, rc)
    return out


def pos_times():
    """{copies in, kernels, copies out} of this thread's last pos(), milliseconds (HIP events)."""
    lib = load_library()
    ms = (C.c_double * 3)()
    _check(lib, lib.thr_debug_pos_times(ms))
    return tuple(ms)


POST_WORKGROUP = 256            # kBlock of csrc/postdetect.hip: the workgroup size of the chain's own kernels
POST_MAX_RECEIVERS = 64         # kMaxReceivers of csrc/postdetect.hip (pos.hip's limit)
# THR_POST_*: name -> (index, dtype, shape as a function of n, the counts and dims)
POST_OUTPUTS = {
    "txid": (0, np.int32, lambda n, c, d: (n,)),
    "keep": (1, np.uint8, lambda n, c, d: (n,)),
    "kept_order": (2, np.int64, lambda n, c, d: (c["kept"],)),
    "match_ptr": (3, np.int64, lambda n, c, d: (c["matches"] + 1,)),
    "match_idx": (4, np.int64, lambda n, c, d: (c["match_entries"],)),
    "misses": (5, np.int64, lambda n, c, d: (c["misses"],)),
    "collisions": (6, np.int64, lambda n, c, d: (c["collisions"], 2)),
    "row_rx": (7, np.int32, lambda n, c, d: (c["rows"], 2)),
    "row_det": (8, np.int64, lambda n, c, d: (c["rows"], 2)),
    "row_val": (9, np.float64, lambda n, c, d: (c["rows"], 3)),
    "group_id": (10, np.int64, lambda n, c, d: (c["groups"],)),
    "group_ptr": (11, np.int64, lambda n, c, d: (c["groups"] + 1,)),
    "group_timestamp": (12, np.float64, lambda n, c, d: (c["groups"],)),
    "group_tx": (13, np.int32, lambda n, c, d: (c["groups"],)),
    "failures": (14, np.int64, lambda n, c, d: (c["failures"], 2)),
    "n_window": (15, np.int32, lambda n, c, d: (c["tasks"],)),
    "n_kept": (16, np.int32, lambda n, c, d: (c["tasks"],)),
    "pos": (17, np.float64, lambda n, c, d: (c["groups"], d)),
    "dop": (18, np.float64, lambda n, c, d: (c["groups"],)),
    "snr": (19, np.float64, lambda n, c, d: (c["groups"],)),
    "status": (20, np.int32, lambda n, c, d: (c["groups"],)),
    "iters": (21, np.int32, lambda n, c, d: (c["groups"],)),
}


def post_settings(freq_ranges, match_window, min_match, rx_ids, rx_coords, first_two_rx, beacon_ids, dist, tdoa_window,
                  sample_rate, deg=2, x0=(0.1, 0.1), max_iter=100, tdoa_as_text=False, tdoa_model=0):
    """(ThrPostSettings, the arrays it points into -- keep them alive as long as the struct)."""
    fmap = (np.zeros(0, dtype=FREQ_RANGE_DTYPE) if freq_ranges is None
            else np.ascontiguousarray(np.asarray(freq_ranges, dtype=FREQ_RANGE_DTYPE)))
    if freq_ranges is not None and len(fmap) == 0:
        raise ValueError("empty frequency map")
    ids = np.ascontiguousarray(rx_ids, dtype=np.int32)
    xy = np.ascontiguousarray(rx_coords, dtype=np.float64)
    beacons = np.ascontiguousarray(beacon_ids, dtype=np.int32)
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    if ids.ndim != 1 or xy.ndim != 2 or len(xy) != len(ids) or beacons.ndim != 1 or dist.shape != (len(ids), len(beacons)):
        raise ValueError("postdetect: rx_ids, rx_coords, beacon_ids or dist have the wrong shape")
    st = ThrPostSettings()
    st.map, st.n_map = (fmap.ctypes.data if len(fmap) else None), len(fmap)
    st.match_window, st.min_match = float(match_window), int(min_match)
    st.n_rx, st.rx_ids, st.dims, st.rx_coords = len(ids), ids.ctypes.data, xy.shape[1], xy.ctypes.data
    st.first_two_rx[0], st.first_two_rx[1] = int(first_two_rx[0]), int(first_two_rx[1])
    st.n_beacons, st.beacon_ids, st.dist = len(beacons), beacons.ctypes.data, dist.ctypes.data
    st.tdoa_window, st.sample_rate, st.deg, st.max_iter = float(tdoa_window), float(sample_rate), int(deg), int(max_iter)
    st.x0[0], st.x0[1] = float(x0[0]), float(x0[1])
    st.tdoa_as_text = 1 if tdoa_as_text else 0
    st.tdoa_model = int(tdoa_model)
    return st, (fmap, ids, xy, beacons, dist)


def postdetect(rxid, block, timestamp, carrier_bin, carrier_offset, soa, energy, noise, settings, outputs=None,
               device_id=0):
    """thr_postdetect on the raw detection columns of all receivers -> (counts dict, {name: array}) with
    every output of POST_OUTPUTS (or those named in `outputs`) fetched.  `settings`: post_settings()'s
    pair.  ValueError for what thr_postdetect refuses."""
    lib = load_library()
    st, _alive = settings
    cols = [np.ascontiguousarray(col, dtype=kind) for col, kind in (
        (rxid, np.int32), (block, np.int32), (timestamp, np.float64), (carrier_bin, np.int32),
        (carrier_offset, np.float64), (soa, np.float64), (energy, np.float64), (noise, np.float64))]
    n = len(cols[0])
    if any(col.ndim != 1 or len(col) != n for col in cols):
        raise ValueError("postdetect: the detection columns differ in length")
    handle, counts = C.c_void_p(), ThrPostCounts()
    rc = lib.thr_postdetect(int(device_id), n, *[col.ctypes.data for col in cols], C.byref(st), C.byref(handle),
                            C.byref(counts))
    if rc == ERR_ARG:
        raise ValueError(lib.thr_last_error().decode())
    _check(lib, rc)
    try:
        c = {name: int(getattr(counts, name)) for name in POST_COUNTS}
        out = {}
        for name in (POST_OUTPUTS if outputs is None else outputs):
            which, kind, shape = POST_OUTPUTS[name]
            out[name] = np.zeros(shape(n, c, int(st.dims)), dtype=kind)
            _check(lib, lib.thr_post_fetch(handle, which, out[name].ctypes.data, out[name].nbytes))
    finally:
        lib.thr_post_free(handle)
    return c, out


def post_times():
    """{copies in, identify, match, tdoa, pos, copies out} of this thread's last postdetect(), milliseconds."""
    lib = load_library()
    ms = (C.c_double * 6)()
    _check(lib, lib.thr_debug_post_times(ms))
    return tuple(ms)


def live_resources():
    """thr_debug_live_resources -> (device buffers, pinned host buffers, streams, events) the library holds now."""
    lib = load_library()
    out = (C.c_int64 * 4)()
    _check(lib, lib.thr_debug_live_resources(out))
    return tuple(int(v) for v in out)


# the eleven detection columns of thr_toadstats, in its argument order
TSTATS_COLUMNS = (("rxid", np.int32), ("txid", np.int32), ("carrier_bin", np.int32), ("timestamp", np.float64),
                  ("soa", np.float64), ("carrier_offset", np.float64), ("carrier_energy", np.float64),
                  ("carrier_noise", np.float64), ("energy", np.float64), ("noise", np.float64), ("offset", np.float64))
# the nine quantities of a cell, in the order of STATS' second axis
TSTATS_QUANTITIES = ("carrier_energy", "carrier_noise", "carrier_snr_db", "carrier_bin", "carrier_offset", "energy",
                     "noise", "snr_db", "offset")
TSTATS_FLAG_OFFSET_NONFINITE = 1        # THR_TSTATS_FLAG_OFFSET_NONFINITE
# THR_TSTATS_*: name -> (index, dtype, shape as a function of the counts)
TSTATS_OUTPUTS = {
    "cell_rx": (0, np.int32, lambda c: (c["cells"],)),
    "cell_tx": (1, np.int32, lambda c: (c["cells"],)),
    "cell_ptr": (2, np.int64, lambda c: (c["cells"] + 1,)),
    "order": (3, np.int64, lambda c: (c["rows"],)),
    "stats": (4, np.float64, lambda c: (c["cells"], 9, 4)),
    "snr_db": (5, np.float64, lambda c: (c["rows"], 2)),
    "minute_ptr": (6, np.int64, lambda c: (c["cells"] + 1,)),
    "minute_hist": (7, np.int64, lambda c: (c["minute_bins"],)),
    "bin_first": (8, np.int32, lambda c: (c["cells"],)),
    "bin_ptr": (9, np.int64, lambda c: (c["cells"] + 1,)),
    "bin_hist": (10, np.int64, lambda c: (c["carrier_bins"],)),
    "offset_edges": (11, np.float64, lambda c: (c["cells"], 11)),
    "offset_hist": (12, np.int64, lambda c: (c["cells"], 10)),
    "cell_flags": (13, np.int32, lambda c: (c["cells"],)),
    "rx_id": (14, np.int32, lambda c: (c["receivers"],)),
    "rx_count": (15, np.int64, lambda c: (c["receivers"],)),
    "rx_fit": (16, np.float64, lambda c: (c["receivers"], 4)),
    "residual": (17, np.float64, lambda c: (c["rows"],)),
}


def toadstats(columns, sel=None, outputs=None, device_id=0):
    """thr_toadstats on the eleven detection columns (a mapping with the names of TSTATS_COLUMNS) and an
    optional selection of row indices -> (counts dict with time0, {name: array}) with every output of
    TSTATS_OUTPUTS (or those named in `outputs`) fetched.  ValueError for what thr_toadstats refuses."""
    lib = load_library()
    cols = [np.ascontiguousarray(columns[name], dtype=kind) for name, kind in TSTATS_COLUMNS]
    n = len(cols[0])
    if any(col.ndim != 1 or len(col) != n for col in cols):
        raise ValueError("toadstats: the detection columns differ in length")
    if sel is not None:
        sel = np.ascontiguousarray(sel, dtype=np.int64)
        if sel.ndim != 1:
            raise ValueError("toadstats: sel must be one-dimensional")
    keep = np.zeros(1, dtype=np.int64)      # a selection of no rows still needs a pointer that is not NULL
    sel_ptr = None if sel is None else (sel.ctypes.data if len(sel) else keep.ctypes.data)
    handle, counts = C.c_void_p(), ThrTstatsCounts()
    rc = lib.thr_toadstats(int(device_id), n, *[col.ctypes.data if n else None for col in cols], sel_ptr,
                           0 if sel is None else len(sel), C.byref(handle), C.byref(counts))
    if rc == ERR_ARG:
        raise ValueError(lib.thr_last_error().decode())
    _check(lib, rc)
    try:
        c = {name: int(getattr(counts, name)) for name in TSTATS_COUNTS}
        out = {}
        for name in (TSTATS_OUTPUTS if outputs is None else outputs):
            which, kind, shape = TSTATS_OUTPUTS[name]
            out[name] = np.zeros(shape(c), dtype=kind)
            _check(lib, lib.thr_tstats_fetch(handle, which, out[name].ctypes.data, out[name].nbytes))
        c["time0"] = float(counts.time0)
    finally:
        lib.thr_tstats_free(handle)
    return c, out


def toadstats_times():
    """{copies in, sort and cells, reductions and histograms, fit, copies out} of this thread's last toadstats(),
    milliseconds (HIP events)."""
    lib = load_library()
    ms = (C.c_double * 5)()
    _check(lib, lib.thr_debug_toadstats_times(ms))
    return tuple(ms)


def toadstats_geometry():
    """thr_debug_toadstats_geometry -> (tile length T, workgroup size W)."""
    lib = load_library()
    t, w = C.c_int(), C.c_int()
    _check(lib, lib.thr_debug_toadstats_geometry(C.byref(t), C.byref(w)))
    return t.value, w.value


def seg_tile_grid(workgroups):
    """thr_debug_seg_tile_grid: the most workgroups a tile kernel of toadstats, beaconsync, tdoastats, reldist and
    track runs on (0: the default, 2048; 1 .. 65536), for the whole process; resets seg_tile_stats().  For tests: no
    result depends on it.  ValueError for a value outside the range."""
    lib = load_library()
    rc = lib.thr_debug_seg_tile_grid(int(workgroups))
    if rc == ERR_ARG:
        raise ValueError(lib.thr_last_error().decode())
    _check(lib, rc)


def seg_tile_stats():
    """thr_debug_seg_tile_stats -> (tile grids sized since the last seg_tile_grid(), the most trips a workgroup's
    tile loop took among them)."""
    lib = load_library()
    launches, trips = C.c_int(), C.c_int()
    _check(lib, lib.thr_debug_seg_tile_stats(C.byref(launches), C.byref(trips)))
    return launches.value, trips.value


# the detection columns of thr_beaconsync, in its argument order
BSYNC_COLUMNS = (("rxid", np.int32), ("txid", np.int32), ("soa", np.float64), ("energy", np.float64),
                 ("noise", np.float64), ("idx", np.int64))
BSYNC_CUT_FITTED, BSYNC_CUT_DEGENERATE, BSYNC_CELL_NO_FIT = 1, 2, 1       # THR_BSYNC_CUT_*, THR_BSYNC_CELL_NO_FIT
# THR_BSYNC_*: name -> (index, dtype, shape as a function of the counts)
BSYNC_OUTPUTS = {
    "cell_key": (0, np.int32, lambda c: (c["cells"], 3)),
    "cell_ptr": (1, np.int64, lambda c: (c["cells"] + 1,)),
    "row_det": (2, np.int64, lambda c: (c["rows"], 2)),
    "row_match": (3, np.int64, lambda c: (c["rows"],)),
    "sdoa": (4, np.float64, lambda c: (c["rows"],)),
    "disc_ptr": (5, np.int64, lambda c: (c["cells"] + 1,)),
    "disc_idx": (6, np.int64, lambda c: (c["discontinuities"],)),
    "cut_ptr": (7, np.int64, lambda c: (c["cells"] + 1,)),
    "cut_left": (8, np.int64, lambda c: (c["cuts"],)),
    "cut_right": (9, np.int64, lambda c: (c["cuts"],)),
    "cut_flags": (10, np.int32, lambda c: (c["cuts"],)),
    "cut_fit": (11, np.float64, lambda c: (c["cuts"], 7)),
    "cut_snr": (12, np.float64, lambda c: (c["cuts"],)),
    "cut_disc_soa": (13, np.float64, lambda c: (c["cuts"],)),
    "residual": (14, np.float64, lambda c: (c["rows"],)),
    "cell_counts": (15, np.int64, lambda c: (c["cells"], 3)),
    "cell_stats": (16, np.float64, lambda c: (c["cells"], 4)),
    "cell_flags": (17, np.int32, lambda c: (c["cells"],)),
}
# the columns of a .tdoa matrix as thr_tdoastats takes them
TDSTATS_COLUMNS = (("rx0", np.int32), ("rx1", np.int32), ("tx", np.int32), ("timestamp", np.float64),
                   ("det0_idx", np.int64), ("det1_idx", np.int64), ("tdoa", np.float64))
TDSTATS_OUTPUTS = {
    "cell_key": (0, np.int32, lambda c: (c["cells"], 3)),
    "cell_ptr": (1, np.int64, lambda c: (c["cells"] + 1,)),
    "order": (2, np.int64, lambda c: (c["rows"],)),
    "stats": (3, np.float64, lambda c: (c["cells"], 5)),
    "robust_stats": (4, np.float64, lambda c: (c["cells"] * c["robust"], 5)),
    "robust_count": (5, np.int64, lambda c: (c["cells"] * c["robust"],)),
    "mask": (6, np.uint8, lambda c: (c["rows"] * c["robust"],)),
    "median": (7, np.float64, lambda c: (c["cells"] * c["robust"], 2)),
}


def _columns(columns, spec, who):
    cols = [np.ascontiguousarray(columns[name], dtype=kind) for name, kind in spec]
    if any(col.ndim != 1 or len(col) != len(cols[0]) for col in cols):
        raise ValueError("%s: the columns differ in length" % who)
    return cols


def _pair(value, kind, who):
    """A closed range as a two-element array, None for none."""
    if value is None:
        return None
    value = np.ascontiguousarray(value, dtype=kind)
    if value.shape != (2,):
        raise ValueError("%s: a range is two numbers" % who)
    return value


def _fetch_all(lib, stem, handle, counts, table, outputs):
    fetch, free = getattr(lib, "thr_%s_fetch" % stem), getattr(lib, "thr_%s_free" % stem)
    try:
        out = {}
        for name in (table if outputs is None else outputs):
            which, kind, shape = table[name]
            out[name] = np.zeros(shape(counts), dtype=kind)
            _check(lib, fetch(handle, which, out[name].ctypes.data, out[name].nbytes))
    finally:
        free(handle)
    return out


def _ptr(a):
    return None if a is None else a.ctypes.data


def beaconsync(columns, match_ptr, match_idx, deg=2, id_range=None, beacons=None, receivers=None, outputs=None,
               device_id=0):
    """thr_beaconsync on the six detection columns (a mapping with the names of BSYNC_COLUMNS) and the matches
    as CSR -> (counts dict, {name: array}) with every output of BSYNC_OUTPUTS (or those named in `outputs`)
    fetched.  ValueError for what thr_beaconsync refuses."""
    lib = load_library()
    cols = _columns(columns, BSYNC_COLUMNS, "beaconsync")
    n = len(cols[0])
    ptr = np.ascontiguousarray(match_ptr, dtype=np.int64)
    idx = np.ascontiguousarray(match_idx, dtype=np.int64)
    if ptr.ndim != 1 or idx.ndim != 1 or len(ptr) < 1 or (ptr[-1] != len(idx) if len(ptr) else True):
        raise ValueError("beaconsync: match_ptr and match_idx are not a CSR pair")
    rng = _pair(id_range, np.int64, "beaconsync")
    lists = [None if v is None else np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in (beacons, receivers)]
    keep = np.zeros(1, dtype=np.int64)      # an empty array still needs a pointer that is not NULL
    handle, counts = C.c_void_p(), ThrBsyncCounts()
    rc = lib.thr_beaconsync(int(device_id), n, *[col.ctypes.data if n else None for col in cols], len(ptr) - 1,
                            ptr.ctypes.data, idx.ctypes.data if len(idx) else keep.ctypes.data, int(deg), _ptr(rng),
                            None if lists[0] is None else (lists[0].ctypes.data if len(lists[0]) else keep.ctypes.data),
                            0 if lists[0] is None else len(lists[0]),
                            None if lists[1] is None else (lists[1].ctypes.data if len(lists[1]) else keep.ctypes.data),
                            0 if lists[1] is None else len(lists[1]), C.byref(handle), C.byref(counts))
    if rc == ERR_ARG:
        raise ValueError(lib.thr_last_error().decode())
    _check(lib, rc)
    c = {name: int(getattr(counts, name)) for name in BSYNC_COUNTS}
    return c, _fetch_all(lib, "bsync", handle, c, BSYNC_OUTPUTS, outputs)


def tdoastats(columns, timestamp=None, detidx=None, robust=False, outputs=None, device_id=0):
    """thr_tdoastats on the seven columns of a .tdoa matrix (a mapping or a structured array with the names of
    TDSTATS_COLUMNS) -> (counts dict, {name: array}).  ValueError for what thr_tdoastats refuses."""
    lib = load_library()
    cols = _columns(columns, TDSTATS_COLUMNS, "tdoastats")
    n = len(cols[0])
    ts, det = _pair(timestamp, np.float64, "tdoastats"), _pair(detidx, np.int64, "tdoastats")
    handle, counts = C.c_void_p(), ThrTdstatsCounts()
    rc = lib.thr_tdoastats(int(device_id), n, *[col.ctypes.data if n else None for col in cols], _ptr(ts), _ptr(det),
                           int(bool(robust)), C.byref(handle), C.byref(counts))
    if rc == ERR_ARG:
        raise ValueError(lib.thr_last_error().decode())
    _check(lib, rc)
    c = {name: int(getattr(counts, name)) for name in TDSTATS_COUNTS}
    return c, _fetch_all(lib, "tdstats", handle, c, TDSTATS_OUTPUTS, outputs)


def syncstats_times(which):
    """Milliseconds (HIP events) of this thread's last beaconsync() (`which` = "beaconsync": copies in, rows and
    cells, discontinuities and cuts, fits and summary, copies out) or tdoastats() ("tdoastats": copies in,
    selection and cells, statistics, the robust part, copies out)."""
    lib = load_library()
    ms = (C.c_double * 5)()
    _check(lib, getattr(lib, "thr_debug_%s_times" % which)(ms))
    return tuple(ms)


def syncstats_geometry(which):
    """thr_debug_{beaconsync,tdoastats}_geometry -> (tile length T, workgroup size W)."""
    lib = load_library()
    t, w = C.c_int(), C.c_int()
    _check(lib, getattr(lib, "thr_debug_%s_geometry" % which)(C.byref(t), C.byref(w)))
    return t.value, w.value


# the detection columns of thr_reldist, in its argument order
RELDIST_COLUMNS = (("rxid", np.int32), ("txid", np.int32), ("soa", np.float64), ("timestamp", np.float64),
                   ("carrier_bin", np.float64), ("carrier_offset", np.float64), ("idx", np.int64))
RELDIST_METHODS = {"nearest": 0, "linpol": 1}                                 # THR_RELDIST_NEAREST, THR_RELDIST_LINPOL
RELDIST_ROW_HELD, RELDIST_CELL_UNSORTED, RELDIST_CELL_NO_BEACON = 1, 1, 2     # THR_RELDIST_ROW_*, THR_RELDIST_CELL_*
# THR_RELDIST_*: name -> (index, dtype, shape as a function of the counts)
RELDIST_OUTPUTS = {
    "cell_key": (0, np.int32, lambda c: (c["cells"], 4)),
    "cell_ptr": (1, np.int64, lambda c: (c["cells"] + 1,)),
    "row_det": (2, np.int64, lambda c: (c["rows"], 2)),
    "row_match": (3, np.int64, lambda c: (c["rows"],)),
    "nearest_idx": (4, np.int32, lambda c: (c["rows"],)),
    "hi": (5, np.int32, lambda c: (c["rows"],)),
    "row_flags": (6, np.int32, lambda c: (c["rows"],)),
    "raw": (7, np.float64, lambda c: (c["rows"],)),
    "x": (8, np.float64, lambda c: (c["rows"],)),
    "mask1": (9, np.uint8, lambda c: (c["rows"],)),
    "cell_stats": (10, np.float64, lambda c: (c["cells"], 6)),
    "cell_counts": (11, np.int64, lambda c: (c["cells"], 5)),
    "speed_ptr": (12, np.int64, lambda c: (c["cells"] + 1,)),
    "speed_x": (13, np.float64, lambda c: (c["speeds"],)),
    "speed": (14, np.float64, lambda c: (c["speeds"],)),
    "mask2": (15, np.uint8, lambda c: (c["speeds"],)),
    "speed_smooth_ptr": (16, np.int64, lambda c: (c["cells"] + 1,)),
    "speed_smooth_x": (17, np.float64, lambda c: (c["speed_points"],)),
    "speed_smooth": (18, np.float64, lambda c: (c["speed_points"],)),
    "dop": (19, np.float64, lambda c: (c["rows"],)),
    "mask3": (20, np.uint8, lambda c: (c["rows"],)),
    "dop_smooth_ptr": (21, np.int64, lambda c: (c["cells"] + 1,)),
    "dop_smooth_x": (22, np.float64, lambda c: (c["dop_points"],)),
    "dop_smooth": (23, np.float64, lambda c: (c["dop_points"],)),
    "medians": (24, np.float64, lambda c: (c["cells"], 6)),
    "cell_flags": (25, np.int32, lambda c: (c["cells"],)),
}


def reldist(columns, match_ptr, match_idx, beacons, mobiles=None, receivers=None, method="linpol", sample_rate=2.4e6,
            block_len=16384, carrier_hz=433e6, thresh=3.5, smooth_frac=0.025, geometry=None, outputs=None, device_id=0):
    """thr_reldist on the seven detection columns (a mapping with the names of RELDIST_COLUMNS) and the matches as
    CSR -> (counts dict, {name: array}) with every output of RELDIST_OUTPUTS (or those named in `outputs`) fetched.
    `geometry`: rows (beacon, rx0, rx1, d_beacon, dist_rx, dist_beacon), the distances in samples; a cell whose key
    is not listed gets zeros.  ValueError for what thr_reldist refuses."""
    lib = load_library()
    cols = _columns(columns, RELDIST_COLUMNS, "reldist")
    n = len(cols[0])
    ptr = np.ascontiguousarray(match_ptr, dtype=np.int64)
    idx = np.ascontiguousarray(match_idx, dtype=np.int64)
    if ptr.ndim != 1 or idx.ndim != 1 or len(ptr) < 1 or (ptr[-1] != len(idx) if len(ptr) else True):
        raise ValueError("reldist: match_ptr and match_idx are not a CSR pair")
    if method not in RELDIST_METHODS:
        raise ValueError("reldist: method must be 'nearest' or 'linpol', not %r" % (method,))
    if beacons is None:
        raise ValueError("reldist: a list of beacons is needed")
    lists = [None if v is None else np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in (beacons, mobiles, receivers)]
    keep = np.zeros(1, dtype=np.int64)      # an empty array still needs a pointer that is not NULL
    geometry = [] if geometry is None else list(geometry)
    table = (ThrReldistGeom * max(1, len(geometry)))()
    for row, (b, r0, r1, d_beacon, dist_rx, dist_beacon) in zip(table, geometry):
        row.beacon, row.rx0, row.rx1 = int(b), int(r0), int(r1)
        row.d_beacon, row.dist_rx, row.dist_beacon = float(d_beacon), float(dist_rx), float(dist_beacon)
    opts = ThrReldistOpts(RELDIST_METHODS[method], 0, float(sample_rate), float(block_len), float(carrier_hz), float(thresh),
                          float(smooth_frac), table, len(geometry))
    args = []
    for v in lists:
        args += [None if v is None else (v.ctypes.data if len(v) else keep.ctypes.data), 0 if v is None else len(v)]
    handle, counts = C.c_void_p(), ThrReldistCounts()
    rc = lib.thr_reldist(int(device_id), n, *[col.ctypes.data if n else None for col in cols], len(ptr) - 1, ptr.ctypes.data,
                         idx.ctypes.data if len(idx) else keep.ctypes.data, *args, C.byref(opts), C.byref(handle), C.byref(counts))
    if rc == ERR_ARG:
        raise ValueError(lib.thr_last_error().decode())
    _check(lib, rc)
    c = {name: int(getattr(counts, name)) for name in RELDIST_COUNTS}
    return c, _fetch_all(lib, "reldist", handle, c, RELDIST_OUTPUTS, outputs)


def reldist_times():
    """Milliseconds (HIP events) of this thread's last reldist(): copies in, rows and cells, distances masks and
    statistics, the two smoothers, copies out."""
    lib = load_library()
    ms = (C.c_double * 5)()
    _check(lib, lib.thr_debug_reldist_times(ms))
    return tuple(ms)


def reldist_geometry():
    """thr_debug_reldist_geometry -> (tile length T, workgroup size W, lanes that share one smoothed point)."""
    lib = load_library()
    t, w, lanes = C.c_int(), C.c_int(), C.c_int()
    _check(lib, lib.thr_debug_reldist_geometry(C.byref(t), C.byref(w), C.byref(lanes)))
    return t.value, w.value, lanes.value


# the detection columns of thr_tdoamatrix, in its argument order
TDMAT_COLUMNS = (("rxid", np.int32), ("txid", np.int32), ("timestamp", np.float64), ("soa", np.float64),
                 ("energy", np.float64), ("noise", np.float64))
TDMAT_MAX_BEACONS = 64          # THR_TDMAT_MAX_BEACONS
TDMAT_CELL_TOO_FEW = 1          # THR_TDMAT_CELL_TOO_FEW
TDMAT_OK, TDMAT_NO_MODEL, TDMAT_OUT_OF_RANGE, TDMAT_SKIPPED = 0, 1, 2, 3      # THR_TDMAT_* task statuses
# THR_TDMAT_*: name -> (index, dtype, shape as a function of the counts)
TDMAT_OUTPUTS = {
    "cell_key": (0, np.int32, lambda c: (c["cells"], 4)),
    "cell_ptr": (1, np.int64, lambda c: (c["cells"] + 1,)),
    "cell_flags": (2, np.int32, lambda c: (c["cells"],)),
    "cell_counts": (3, np.int64, lambda c: (c["cells"], 5)),
    "cell_stats": (4, np.float64, lambda c: (c["cells"], 5)),
    "medians": (5, np.float64, lambda c: (c["cells"], 2)),
    "task_det": (6, np.int64, lambda c: (c["tasks"], 2)),
    "task_match": (7, np.int64, lambda c: (c["tasks"],)),
    "timestamp": (8, np.float64, lambda c: (c["tasks"],)),
    "tdoa": (9, np.float64, lambda c: (c["tasks"],)),
    "status": (10, np.int32, lambda c: (c["tasks"],)),
    "snr": (11, np.float64, lambda c: (c["tasks"],)),
    "model_quality": (12, np.float64, lambda c: (c["tasks"],)),
    "n_window": (13, np.int32, lambda c: (c["tasks"],)),
    "n_kept": (14, np.int32, lambda c: (c["tasks"],)),
    "outlier": (15, np.uint8, lambda c: (c["tasks"],)),
}


def tdoamatrix(columns, match_ptr, match_idx, beacons, receivers=None, targets=None, dist=None, window=4.0, sample_rate=2.4e6,
               model=0, deg=2, outputs=None, device_id=0):
    """thr_tdoamatrix on the six detection columns (a mapping with the names of TDMAT_COLUMNS) and the matches as CSR
    -> (counts dict, {name: array}) with every output of TDMAT_OUTPUTS (or those named in `outputs`) fetched.
    `dist`: float64[len(receivers)][len(beacons)] in the order of the two lists (None: zeros); `model`: a
    TDOA_MODELS code.  ValueError for what thr_tdoamatrix refuses."""
    lib = load_library()
    cols = _columns(columns, TDMAT_COLUMNS, "tdoamatrix")
    n = len(cols[0])
    ptr = np.ascontiguousarray(match_ptr, dtype=np.int64)
    idx = np.ascontiguousarray(match_idx, dtype=np.int64)
    if ptr.ndim != 1 or idx.ndim != 1 or len(ptr) < 1 or (ptr[-1] != len(idx) if len(ptr) else True):
        raise ValueError("tdoamatrix: match_ptr and match_idx are not a CSR pair")
    if beacons is None:
        raise ValueError("tdoamatrix: a list of beacons is needed")
    lists = [None if v is None else np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in (receivers, beacons, targets)]
    if dist is not None:
        if lists[0] is None:
            raise ValueError("tdoamatrix: dist needs the list of receivers its rows are of")
        dist = np.ascontiguousarray(dist, dtype=np.float64)
        if dist.shape != (len(lists[0]), len(lists[1])):
            raise ValueError("tdoamatrix: dist must be float64[%d receivers][%d beacons]" % (len(lists[0]), len(lists[1])))
    keep = np.zeros(1, dtype=np.int64)      # an empty array still needs a pointer that is not NULL
    args = []
    for v in lists:
        args += [None if v is None else (v.ctypes.data if len(v) else keep.ctypes.data), 0 if v is None else len(v)]
    handle, counts = C.c_void_p(), ThrTdmatCounts()
    rc = lib.thr_tdoamatrix(int(device_id), n, *[col.ctypes.data if n else None for col in cols], len(ptr) - 1, ptr.ctypes.data,
                            idx.ctypes.data if len(idx) else keep.ctypes.data, *args,
                            None if dist is None else (dist.ctypes.data if dist.size else keep.ctypes.data), float(window),
                            float(sample_rate), int(model), int(deg), C.byref(handle), C.byref(counts))
    if rc == ERR_ARG:
        raise ValueError(lib.thr_last_error().decode())
    _check(lib, rc)
    c = {name: int(getattr(counts, name)) for name in TDMAT_COUNTS}
    return c, _fetch_all(lib, "tdmat", handle, c, TDMAT_OUTPUTS, outputs)


def tdoamatrix_times():
    """Milliseconds (HIP events) of this thread's last tdoamatrix(): copies in, rows and tasks, estimate, mask and
    statistics, copies out."""
    lib = load_library()
    ms = (C.c_double * 5)()
    _check(lib, lib.thr_debug_tdoamatrix_times(ms))
    return tuple(ms)


def tdoamatrix_geometry():
    """thr_debug_tdoamatrix_geometry -> (tile length T, workgroup size W, tasks per workgroup of the estimate kernel)."""
    lib = load_library()
    t, w, tasks = C.c_int(), C.c_int(), C.c_int()
    _check(lib, lib.thr_debug_tdoamatrix_geometry(C.byref(t), C.byref(w), C.byref(tasks)))
    return t.value, w.value, tasks.value


POSQ_INCONSISTENT, POSQ_EXCLUDED, POSQ_NO_CANDIDATE = 1, 2, 4      # THR_POSQ_* flags
POSQ_MIN_RX = 5         # the floor of min_rx: one of five receivers left out leaves four, one redundant arrival
# THR_POSQ_*: name -> (index, dtype, shape as a function of the counts)
POSQ_OUTPUTS = {
    "pos": (0, np.float64, lambda c: (c["groups"], 2)),
    "dop": (1, np.float64, lambda c: (c["groups"],)),
    "status": (2, np.int32, lambda c: (c["groups"],)),
    "iters": (3, np.int32, lambda c: (c["groups"],)),
    "q": (4, np.float64, lambda c: (c["groups"], 3)),
    "rms": (5, np.float64, lambda c: (c["groups"], 2)),
    "counts": (6, np.int32, lambda c: (c["groups"], 3)),
    "flags": (7, np.int32, lambda c: (c["groups"],)),
    "full_pos": (8, np.float64, lambda c: (c["groups"], 2)),
    "full_status": (9, np.int32, lambda c: (c["groups"],)),
    "snr": (10, np.float64, lambda c: (c["groups"],)),
    "residual": (11, np.float64, lambda c: (c["rows"],)),
    "used": (12, np.uint8, lambda c: (c["rows"],)),
    "task_ptr": (13, np.int64, lambda c: (c["groups"] + 1,)),
    "task_rx": (14, np.int32, lambda c: (c["tasks"],)),
    "task_pos": (15, np.float64, lambda c: (c["tasks"], 2)),
    "task_rms": (16, np.float64, lambda c: (c["tasks"],)),
    "task_status": (17, np.int32, lambda c: (c["tasks"],)),
    "task_nrx": (18, np.int32, lambda c: (c["tasks"],)),
    "task_iters": (19, np.int32, lambda c: (c["tasks"],)),
}


def posq(group_ptr, row_rx0, row_rx1, row_tdoa, row_snr, rx_coords, row_weight=None, gate_m=0.0, ratio=0.5, min_rx=POSQ_MIN_RX,
         x0=(0.1, 0.1), max_iter=100, outputs=None, device_id=0):
    """thr_posq on TDOA rows in CSR form (thr_pos's columns: dense receiver indices into rx_coords[n_rx, 2]) with an
    optional weight per row -> (counts dict, {name: array}) with every output of POSQ_OUTPUTS (or those named in
    `outputs`) fetched.  gate_m == 0 switches the exclusion off.  ValueError for what thr_posq refuses."""
    lib = load_library()
    ptr = np.ascontiguousarray(group_ptr, dtype=np.int64)
    rx0, rx1 = np.ascontiguousarray(row_rx0, dtype=np.int32), np.ascontiguousarray(row_rx1, dtype=np.int32)
    tdoa, snr = np.ascontiguousarray(row_tdoa, dtype=np.float64), np.ascontiguousarray(row_snr, dtype=np.float64)
    weight = None if row_weight is None else np.ascontiguousarray(row_weight, dtype=np.float64)
    xy = np.ascontiguousarray(rx_coords, dtype=np.float64)
    if ptr.ndim != 1 or len(ptr) < 1 or xy.ndim != 2 or not (len(rx0) == len(rx1) == len(tdoa) == len(snr) == int(ptr[-1])):
        raise ValueError("posq: group_ptr, the row columns or rx_coords have the wrong shape")
    if weight is not None and weight.shape != tdoa.shape:
        raise ValueError("posq: one weight per row")
    start = np.ascontiguousarray(x0, dtype=np.float64)
    if start.shape != (2,):
        raise ValueError("posq: x0 holds two values")
    opts = ThrPosqOpts(int(max_iter), int(min_rx), (C.c_double * 2)(*start.tolist()), float(gate_m), float(ratio))
    keep = np.zeros(1, dtype=np.float64)      # an empty column still needs a pointer that is not NULL
    handle, counts = C.c_void_p(), ThrPosqCounts()
    rc = lib.thr_posq(int(device_id), len(ptr) - 1, ptr.ctypes.data, rx0.ctypes.data, rx1.ctypes.data, tdoa.ctypes.data,
                      snr.ctypes.data, None if weight is None else (weight.ctypes.data if len(weight) else keep.ctypes.data),
                      xy.shape[0], xy.shape[1], xy.ctypes.data, C.byref(opts), C.byref(handle), C.byref(counts))
    if rc == ERR_ARG:
        raise ValueError(lib.thr_last_error().decode())
    _check(lib, rc)
    c = {name: int(getattr(counts, name)) for name in POSQ_COUNTS}
    return c, _fetch_all(lib, "posq", handle, c, POSQ_OUTPUTS, outputs)


def posq_times():
    """Milliseconds (HIP events) of this thread's last posq(): copies in, full solves, flags and expansion, candidates,
    choice and residuals, copies out."""
    lib = load_library()
    ms = (C.c_double * 6)()
    _check(lib, lib.thr_debug_posq_times(ms))
    return tuple(ms)


TRACK_LOST = 1          # THR_TRACK_LOST
TRACK_GATE_999 = 13.815510557964274     # -2 ln 0.001: the 99.9 % point of chi^2 with 2 degrees of freedom
TRACK_STATS = ("rows", "valid", "used", "rejected", "mean_nis", "duration", "path", "mean_speed")
# THR_TRACK_*: name -> (index, dtype, shape as a function of the counts); the per-row arrays are in input row order
TRACK_OUTPUTS = {
    "order": (0, np.int64, lambda c: (c["rows"],)),
    "track_tx": (1, np.int32, lambda c: (c["tracks"],)),
    "track_ptr": (2, np.int64, lambda c: (c["tracks"] + 1,)),
    "used": (3, np.uint8, lambda c: (c["rows"],)),
    "nis": (4, np.float64, lambda c: (c["rows"],)),
    "filt": (5, np.float64, lambda c: (c["rows"], 4)),
    "filt_var": (6, np.float64, lambda c: (c["rows"], 6)),
    "smooth": (7, np.float64, lambda c: (c["rows"], 4)),
    "smooth_var": (8, np.float64, lambda c: (c["rows"], 6)),
    "track_stats": (9, np.float64, lambda c: (c["tracks"], 8)),
    "track_flags": (10, np.int32, lambda c: (c["tracks"],)),
}


def track(tx, timestamp, x, y, rx, ry, valid=None, q=None, v0=10.0, gate=TRACK_GATE_999, max_rounds=4, outputs=None,
          device_id=0):
    """thr_track on one row per position (rx, ry: the measurement variances of the two axes in m^2; q in m^2/s^3)
    -> (counts dict, {name: array}) with every output of TRACK_OUTPUTS (or those named in `outputs`) fetched.
    ValueError for what thr_track refuses."""
    lib = load_library()
    if q is None:
        raise ValueError("track: q has no default, it is the deployment's")
    tx = np.ascontiguousarray(tx, dtype=np.int32)
    cols = [np.ascontiguousarray(v, dtype=np.float64) for v in (timestamp, x, y, rx, ry)]
    mask = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    if tx.ndim != 1 or any(v.shape != tx.shape for v in cols) or (mask is not None and mask.shape != tx.shape):
        raise ValueError("track: the columns are one-dimensional and of one length")
    n = len(tx)
    opts = ThrTrackOpts(float(q), float(v0), float(gate), int(max_rounds), 0)
    handle, counts = C.c_void_p(), ThrTrackCounts()
    rc = lib.thr_track(int(device_id), n, tx.ctypes.data if n else None, *[v.ctypes.data if n else None for v in cols],
                       None if mask is None or not n else mask.ctypes.data, C.byref(opts), C.byref(handle), C.byref(counts))
    if rc == ERR_ARG:
        raise ValueError(lib.thr_last_error().decode())
    _check(lib, rc)
    c = {name: int(getattr(counts, name)) for name in TRACK_COUNTS}
    return c, _fetch_all(lib, "track", handle, c, TRACK_OUTPUTS, outputs)


def track_times():
    """Milliseconds (HIP events) of this thread's last track(): copies in, sort and layout, filter rounds, smoother,
    statistics, copies out."""
    lib = load_library()
    ms = (C.c_double * 6)()
    _check(lib, lib.thr_debug_track_times(ms))
    return tuple(ms)


def track_geometry():
    """thr_debug_track_geometry -> (tile length T, workgroup size W, doubles of one filter element)."""
    lib = load_library()
    t, w, e = C.c_int(), C.c_int(), C.c_int()
    _check(lib, lib.thr_debug_track_geometry(C.byref(t), C.byref(w), C.byref(e)))
    return t.value, w.value, e.value


POSG_MOVED, POSG_AMBIGUOUS, POSG_NO_MINIMUM = 1, 2, 4      # THR_POSG_* flags
POSG_NO_TASK = -1           # THR_POSG_NO_TASK: the status of a task that does not exist
POSG_ROW_CHUNK = 32         # THR_POSG_ROW_CHUNK: rows the surface kernel stages in LDS at a time
POSG_DIST_RECEIVERS = 32    # kDistRx: up to this many receivers the surface kernel takes a cell's distances once per receiver
POSG_GRIDS = (16, 32, 64)
POSG_MAX_STARTS = 8
POSG_MAX_MAP = 256          # groups whose surface one call can return
POSG_MAX_MARGIN = 10e3      # thr_pos's box reaches this far beyond the receivers
# THR_POSG_*: name -> (index, dtype, shape as a function of the counts)
POSG_OUTPUTS = {
    "pos": (0, np.float64, lambda c: (c["groups"], 2)),
    "dop": (1, np.float64, lambda c: (c["groups"],)),
    "status": (2, np.int32, lambda c: (c["groups"],)),
    "task": (3, np.int32, lambda c: (c["groups"],)),
    "rms": (4, np.float64, lambda c: (c["groups"],)),
    "pos2": (5, np.float64, lambda c: (c["groups"], 2)),
    "rms2": (6, np.float64, lambda c: (c["groups"],)),
    "n_minima": (7, np.int32, lambda c: (c["groups"],)),
    "flags": (8, np.int32, lambda c: (c["groups"],)),
    "snr": (9, np.float64, lambda c: (c["groups"],)),
    "n_local": (10, np.int32, lambda c: (c["groups"],)),
    "start_cell": (11, np.int32, lambda c: (c["groups"], c["starts"])),
    "start_f": (12, np.float64, lambda c: (c["groups"], c["starts"])),
    "task_pos": (13, np.float64, lambda c: (c["groups"], c["tasks"], 2)),
    "task_dop": (14, np.float64, lambda c: (c["groups"], c["tasks"])),
    "task_rms": (15, np.float64, lambda c: (c["groups"], c["tasks"])),
    "task_status": (16, np.int32, lambda c: (c["groups"], c["tasks"])),
    "task_iters": (17, np.int32, lambda c: (c["groups"], c["tasks"])),
    "map": (18, np.float64, lambda c: (c["map_groups"], c["grid"], c["grid"])),
    "map_min": (19, np.uint8, lambda c: (c["map_groups"], c["grid"], c["grid"])),
}


def posg(group_ptr, row_rx0, row_rx1, row_tdoa, row_snr, rx_coords, margin_m, grid=32, starts=4, merge_m=1.0, ratio=2.0,
         floor_m=0.0, map_first=0, map_count=0, x0=(0.1, 0.1), max_iter=100, outputs=None, device_id=0):
    """thr_posg on TDOA rows in CSR form (thr_pos's columns: dense receiver indices into rx_coords[n_rx, 2]) ->
    (counts dict, {name: array}) with every output of POSG_OUTPUTS (or those named in `outputs`) fetched.
    ValueError for what thr_posg refuses."""
    lib = load_library()
    ptr = np.ascontiguousarray(group_ptr, dtype=np.int64)
    rx0, rx1 = np.ascontiguousarray(row_rx0, dtype=np.int32), np.ascontiguousarray(row_rx1, dtype=np.int32)
    tdoa, snr = np.ascontiguousarray(row_tdoa, dtype=np.float64), np.ascontiguousarray(row_snr, dtype=np.float64)
    xy = np.ascontiguousarray(rx_coords, dtype=np.float64)
    if ptr.ndim != 1 or len(ptr) < 1 or xy.ndim != 2 or not (len(rx0) == len(rx1) == len(tdoa) == len(snr) == int(ptr[-1])):
        raise ValueError("posg: group_ptr, the row columns or rx_coords have the wrong shape")
    start = np.ascontiguousarray(x0, dtype=np.float64)
    if start.shape != (2,):
        raise ValueError("posg: x0 holds two values")
    opts = ThrPosgOpts(int(max_iter), int(grid), int(starts), (C.c_double * 2)(*start.tolist()), float(margin_m), float(merge_m),
                       float(ratio), float(floor_m), int(map_first), int(map_count))
    handle, counts = C.c_void_p(), ThrPosgCounts()
    rc = lib.thr_posg(int(device_id), len(ptr) - 1, ptr.ctypes.data, rx0.ctypes.data, rx1.ctypes.data, tdoa.ctypes.data,
                      snr.ctypes.data, xy.shape[0], xy.shape[1], xy.ctypes.data, C.byref(opts), C.byref(handle), C.byref(counts))
    if rc == ERR_ARG:
        raise ValueError(lib.thr_last_error().decode())
    _check(lib, rc)
    c = {name: int(getattr(counts, name)) for name in POSG_COUNTS}
    return c, _fetch_all(lib, "posg", handle, c, POSG_OUTPUTS, outputs)


def posg_times():
    """Milliseconds (HIP events) of this thread's last posg(): copies in, task 0 (the fixed start), surface minima and
    starts, refinement (tasks 1 .. K), choice, copies out."""
    lib = load_library()
    ms = (C.c_double * 6)()
    _check(lib, lib.thr_debug_posg_times(ms))
    return tuple(ms)


COVERAGE_UNCOVERED, COVERAGE_DEGENERATE, COVERAGE_LOSSY = 1, 2, 4      # THR_COV_* flags
COVERAGE_MAX_TRIALS = 4096      # THR_COV_MAX_TRIALS
COVERAGE_MAX_KEEP = 64          # THR_COV_MAX_KEEP: cells whose trials one call can return
COVERAGE_MAX_CELLS = 1 << 20
COVERAGE_MAX_TASKS = 1 << 28    # cells x trials
COVERAGE_SLAB_BYTES = 512 << 20  # THR_COV_SLAB_BYTES: the byte budget of one slab
COVERAGE_PRED = ("dop", "pred_sxx", "pred_sxy", "pred_syy", "pred_rms")                      # the columns of "pred"
COVERAGE_CELL_COUNTS = ("n_ok", "n_at_bound", "n_unconverged", "n_nonfinite", "n_good", "n_gross")   # of "counts"
COVERAGE_STATS = ("bias_x", "bias_y", "sxx", "sxy", "syy", "rms", "q50", "q95")              # of "stats"
# THR_COV_*: name -> (index, dtype, shape as a function of the counts)
COVERAGE_OUTPUTS = {
    "cx": (0, np.float64, lambda c: (c["nx"],)),
    "cy": (1, np.float64, lambda c: (c["ny"],)),
    "n_heard": (2, np.int32, lambda c: (c["cells"],)),
    "heard_mask": (3, np.uint64, lambda c: (c["cells"],)),
    "flags": (4, np.int32, lambda c: (c["cells"],)),
    "pred": (5, np.float64, lambda c: (c["cells"], 5)),
    "counts": (6, np.int32, lambda c: (c["cells"], 6)),
    "iters_sum": (7, np.int64, lambda c: (c["cells"],)),
    "stats": (8, np.float64, lambda c: (c["cells"], 8)),
    "keep_ptr": (9, np.int64, lambda c: (c["keep_tasks"] + 1,)),
    "keep_rx0": (10, np.int32, lambda c: (c["keep_rows"],)),
    "keep_rx1": (11, np.int32, lambda c: (c["keep_rows"],)),
    "keep_tdoa": (12, np.float64, lambda c: (c["keep_rows"],)),
    "keep_noise": (13, np.float64, lambda c: (c["keep_tasks"], c["n_rx"])),
    "keep_pos": (14, np.float64, lambda c: (c["keep_tasks"], 2)),
    "keep_status": (15, np.int32, lambda c: (c["keep_tasks"],)),
    "keep_iters": (16, np.int32, lambda c: (c["keep_tasks"],)),
    "keep_err": (17, np.float64, lambda c: (c["keep_tasks"],)),
}


def coverage(rx_coords, sigma_rx, lo, hi, nx, ny, gross_m, trials=256, range_m=0.0, seed=0, x0=(0.1, 0.1), max_iter=100,
             slab_groups=0, keep_first=0, keep_count=0, outputs=None, device_id=0):
    """thr_coverage for receivers rx_coords[n_rx, 2] with arrival noise sigma_rx[n_rx] (metres) on the nx x ny raster
    over lo .. hi -> (counts dict, {name: array}) with every output of COVERAGE_OUTPUTS (or those named in `outputs`)
    fetched.  `seed` is a 64-bit number: its low and high words are the generator's key.  ValueError for what
    thr_coverage refuses."""
    lib = load_library()
    xy = np.ascontiguousarray(rx_coords, dtype=np.float64)
    sigma = np.ascontiguousarray(sigma_rx, dtype=np.float64)
    if xy.ndim != 2 or xy.shape[1] != 2 or sigma.shape != (xy.shape[0],):
        raise ValueError("coverage: rx_coords is [n_rx, 2] and sigma_rx [n_rx]")
    corners = [np.ascontiguousarray(v, dtype=np.float64) for v in (lo, hi, x0)]
    if any(v.shape != (2,) for v in corners):
        raise ValueError("coverage: lo, hi and x0 hold two values each")
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("coverage: seed must lie in 0 .. 2^64 - 1")
    pair = lambda v: (C.c_double * 2)(*v.tolist())     # noqa: E731
    opts = ThrCoverageOpts(pair(corners[0]), pair(corners[1]), int(nx), int(ny), int(trials), int(max_iter), float(range_m),
                           float(gross_m), pair(corners[2]), seed & 0xFFFFFFFF, seed >> 32, int(slab_groups), int(keep_first),
                           int(keep_count))
    handle, counts = C.c_void_p(), ThrCoverageCounts()
    rc = lib.thr_coverage(int(device_id), xy.shape[0], xy.ctypes.data, sigma.ctypes.data, C.byref(opts), C.byref(handle),
                          C.byref(counts))
    if rc == ERR_ARG:
        raise ValueError(lib.thr_last_error().decode())
    _check(lib, rc)
    c = {name: int(getattr(counts, name)) for name in COVERAGE_COUNTS}
    return c, _fetch_all(lib, "coverage", handle, c, COVERAGE_OUTPUTS, outputs)


def coverage_times():
    """Milliseconds (HIP events) of this thread's last coverage(): copies in, cells, synthesis, solve, reduction and sort,
    copies out."""
    lib = load_library()
    ms = (C.c_double * 6)()
    _check(lib, lib.thr_debug_coverage_times(ms))
    return tuple(ms)


POS3_GROUPS_PER_WORKGROUP = 32  # kTeams of csrc/pos3.hip: one 8-lane team per group
POS3_REGISTER_ROWS = 4          # kRegRows: rows per lane held in registers; groups over 32 rows re-read theirs
POS3_KNOWN_HEIGHT, POS3_FREE_Z = 0, 1       # THR_POS3_*
POS3_OUTPUTS = ("pos", "dop", "hdop", "vdop", "rms", "snr", "status", "iters")


def pos3(group_ptr, row_rx0, row_rx1, row_tdoa, row_snr, rx_xyz, mode, group_h=None, x0=(0.1, 0.1, 0.0), z_range=None,
         max_iter=100, device_id=0):
    """thr_pos3 on TDOA rows in CSR form (thr_pos's columns: dense receiver indices into rx_xyz[n_rx, 3]) -> dict of
    pos float64[g, 3], dop / hdop / vdop / rms / snr float64[g], status / iters int32[g], every group in order.
    mode POS3_KNOWN_HEIGHT reads group_h[g]; POS3_FREE_Z reads x0[2] and z_range.  ValueError for what thr_pos3 refuses."""
    lib = load_library()
    ptr = np.ascontiguousarray(group_ptr, dtype=np.int64)
    rx0, rx1 = np.ascontiguousarray(row_rx0, dtype=np.int32), np.ascontiguousarray(row_rx1, dtype=np.int32)
    tdoa, snr = np.ascontiguousarray(row_tdoa, dtype=np.float64), np.ascontiguousarray(row_snr, dtype=np.float64)
    xyz = np.ascontiguousarray(rx_xyz, dtype=np.float64)
    if (ptr.ndim != 1 or len(ptr) < 1 or xyz.ndim != 2 or xyz.shape[1] != 3 or
            not (len(rx0) == len(rx1) == len(tdoa) == len(snr) == int(ptr[-1]))):
        raise ValueError("pos3: group_ptr, the row columns or rx_xyz[n_rx, 3] have the wrong shape")
    n = len(ptr) - 1
    start = np.ascontiguousarray(x0, dtype=np.float64)
    if start.shape != (3,):
        raise ValueError("pos3: x0 holds three values")
    heights = None if group_h is None else np.ascontiguousarray(group_h, dtype=np.float64)
    if heights is not None and heights.shape != (n,):
        raise ValueError("pos3: group_h holds one height per group")
    box = None if z_range is None else np.ascontiguousarray(z_range, dtype=np.float64)
    if box is not None and box.shape != (2,):
        raise ValueError("pos3: z_range holds two values")
    out = {"pos": np.zeros((n, 3), dtype=np.float64)}
    out.update({key: np.zeros(n, dtype=np.float64) for key in ("dop", "hdop", "vdop", "rms", "snr")})
    out.update({key: np.zeros(n, dtype=np.int32) for key in ("status", "iters")})
    rc = lib.thr_pos3(int(device_id), n, ptr.ctypes.data, rx0.ctypes.data, rx1.ctypes.data, tdoa.ctypes.data,
                      snr.ctypes.data, xyz.shape[0], xyz.ctypes.data, int(mode),
                      None if heights is None else heights.ctypes.data, start.ctypes.data,
                      None if box is None else box.ctypes.data, int(max_iter), *[out[key].ctypes.data for key in POS3_OUTPUTS])
    if rc == ERR_ARG:
        raise ValueError(lib.thr_last_error().decode())
    _check(lib, rc)
    return out


def pos3_times():
    """{copies in, the kernel, copies out} of this thread's last pos3(), milliseconds (HIP events)."""
    lib = load_library()
    ms = (C.c_double * 3)()
    _check(lib, lib.thr_debug_pos3_times(ms))
    return tuple(ms)


POSG3_MOVED, POSG3_AMBIGUOUS, POSG3_NO_MINIMUM, POSG3_MIRROR = 1, 2, 4, 8      # THR_POSG3_* flags
POSG3_NO_TASK = -1          # THR_POSG3_NO_TASK: the status of a task that does not exist
POSG3_ROW_CHUNK = 32        # kRowChunk of csrc/posg3.hip: a longer group stages its chunks again for every plane
POSG3_DIST_RECEIVERS = 32   # kDistRx: up to this many receivers the volume kernel takes a cell's distances once per receiver
POSG3_GRIDS = (16, 32)
POSG3_MAX_GRID_Z = 32       # planes with z free: 2 .. 32; one plane with the height known
POSG3_MAX_STARTS = 8
POSG3_MAX_MAP = 256         # groups whose volume one call can return
POSG3_MAX_MARGIN = 10e3     # thr_pos3's box reaches this far beyond the receivers
_volume = lambda c: (c["map_groups"], c["grid_z"], c["grid"], c["grid"])      # noqa: E731
# THR_POSG3_*: name -> (index, dtype, shape as a function of the counts)
POSG3_OUTPUTS = {
    "pos": (0, np.float64, lambda c: (c["groups"], 3)),
    "dop": (1, np.float64, lambda c: (c["groups"],)),
    "status": (2, np.int32, lambda c: (c["groups"],)),
    "task": (3, np.int32, lambda c: (c["groups"],)),
    "rms": (4, np.float64, lambda c: (c["groups"],)),
    "pos2": (5, np.float64, lambda c: (c["groups"], 3)),
    "rms2": (6, np.float64, lambda c: (c["groups"],)),
    "n_minima": (7, np.int32, lambda c: (c["groups"],)),
    "flags": (8, np.int32, lambda c: (c["groups"],)),
    "snr": (9, np.float64, lambda c: (c["groups"],)),
    "n_local": (10, np.int32, lambda c: (c["groups"],)),
    "start_cell": (11, np.int32, lambda c: (c["groups"], c["starts"])),
    "start_f": (12, np.float64, lambda c: (c["groups"], c["starts"])),
    "task_pos": (13, np.float64, lambda c: (c["groups"], c["tasks"], 3)),
    "task_dop": (14, np.float64, lambda c: (c["groups"], c["tasks"])),
    "task_rms": (15, np.float64, lambda c: (c["groups"], c["tasks"])),
    "task_status": (16, np.int32, lambda c: (c["groups"], c["tasks"])),
    "task_iters": (17, np.int32, lambda c: (c["groups"], c["tasks"])),
    "map": (18, np.float64, _volume),
    "map_min": (19, np.uint8, _volume),
    "hdop": (20, np.float64, lambda c: (c["groups"],)),
    "vdop": (21, np.float64, lambda c: (c["groups"],)),
    "task_hdop": (22, np.float64, lambda c: (c["groups"], c["tasks"])),
    "task_vdop": (23, np.float64, lambda c: (c["groups"], c["tasks"])),
}


def posg3(group_ptr, row_rx0, row_rx1, row_tdoa, row_snr, rx_xyz, mode, margin_m, group_h=None, x0=(0.1, 0.1, 0.0), z_range=None,
          z_grid=None, grid=32, grid_z=8, starts=4, merge_m=1.0, ratio=2.0, floor_m=0.0, map_first=0, map_count=0, max_iter=100,
          outputs=None, device_id=0):
    """thr_posg3 on TDOA rows in CSR form (thr_pos3's columns: dense receiver indices into rx_xyz[n_rx, 3]) ->
    (counts dict, {name: array}) with every output of POSG3_OUTPUTS (or those named in `outputs`) fetched.  mode
    POS3_KNOWN_HEIGHT reads group_h[g] (grid_z must be 1); POS3_FREE_Z reads x0[2], z_range and z_grid.  ValueError for
    what thr_posg3 refuses."""
    lib = load_library()
    ptr = np.ascontiguousarray(group_ptr, dtype=np.int64)
    rx0, rx1 = np.ascontiguousarray(row_rx0, dtype=np.int32), np.ascontiguousarray(row_rx1, dtype=np.int32)
    tdoa, snr = np.ascontiguousarray(row_tdoa, dtype=np.float64), np.ascontiguousarray(row_snr, dtype=np.float64)
    xyz = np.ascontiguousarray(rx_xyz, dtype=np.float64)
    if (ptr.ndim != 1 or len(ptr) < 1 or xyz.ndim != 2 or xyz.shape[1] != 3 or
            not (len(rx0) == len(rx1) == len(tdoa) == len(snr) == int(ptr[-1]))):
        raise ValueError("posg3: group_ptr, the row columns or rx_xyz[n_rx, 3] have the wrong shape")
    n = len(ptr) - 1
    start = np.ascontiguousarray(x0, dtype=np.float64)
    if start.shape != (3,):
        raise ValueError("posg3: x0 holds three values")
    heights = None if group_h is None else np.ascontiguousarray(group_h, dtype=np.float64)
    if heights is not None and heights.shape != (n,):
        raise ValueError("posg3: group_h holds one height per group")
    pairs = [None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in (z_range, z_grid)]
    if any(v is not None and v.shape != (2,) for v in pairs):
        raise ValueError("posg3: z_range and z_grid hold two values each")
    opts = ThrPosg3Opts(int(max_iter), int(grid), int(grid_z), int(starts), (C.c_double * 3)(*start.tolist()), float(margin_m),
                        float(merge_m), float(ratio), float(floor_m), int(map_first), int(map_count))
    handle, counts = C.c_void_p(), ThrPosg3Counts()
    rc = lib.thr_posg3(int(device_id), n, ptr.ctypes.data, rx0.ctypes.data, rx1.ctypes.data, tdoa.ctypes.data, snr.ctypes.data,
                       xyz.shape[0], xyz.ctypes.data, int(mode), _ptr(heights), _ptr(pairs[0]), _ptr(pairs[1]), C.byref(opts),
                       C.byref(handle), C.byref(counts))
    if rc == ERR_ARG:
        raise ValueError(lib.thr_last_error().decode())
    _check(lib, rc)
    c = {name: int(getattr(counts, name)) for name in POSG3_COUNTS}
    return c, _fetch_all(lib, "posg3", handle, c, POSG3_OUTPUTS, outputs)


def posg3_times():
    """Milliseconds (HIP events) of this thread's last posg3(): copies in, task 0 (the fixed start), surface, minima and
    starts, refinement (tasks 1 .. K), choice, copies out."""
    lib = load_library()
    ms = (C.c_double * 6)()
    _check(lib, lib.thr_debug_posg3_times(ms))
    return tuple(ms)


POSQ3_INCONSISTENT, POSQ3_EXCLUDED, POSQ3_NO_CANDIDATE = 1, 2, 4      # THR_POSQ3_* flags
# the floors of min_rx (known height, free z): N receivers give N - 1 independent TDOAs, and a candidate (N - 1
# receivers) must keep one redundant arrival: N - 2 > unknowns
POSQ3_MIN_RX = (5, 6)
# THR_POSQ3_*: name -> (index, dtype, shape as a function of the counts); POSQ_OUTPUTS' names, indices and types
POSQ3_OUTPUTS = {
    "pos": (0, np.float64, lambda c: (c["groups"], 3)),
    "dop": (1, np.float64, lambda c: (c["groups"],)),
    "status": (2, np.int32, lambda c: (c["groups"],)),
    "iters": (3, np.int32, lambda c: (c["groups"],)),
    "q": (4, np.float64, lambda c: (c["groups"], 6)),
    "rms": (5, np.float64, lambda c: (c["groups"], 2)),
    "counts": (6, np.int32, lambda c: (c["groups"], 3)),
    "flags": (7, np.int32, lambda c: (c["groups"],)),
    "full_pos": (8, np.float64, lambda c: (c["groups"], 3)),
    "full_status": (9, np.int32, lambda c: (c["groups"],)),
    "snr": (10, np.float64, lambda c: (c["groups"],)),
    "residual": (11, np.float64, lambda c: (c["rows"],)),
    "used": (12, np.uint8, lambda c: (c["rows"],)),
    "task_ptr": (13, np.int64, lambda c: (c["groups"] + 1,)),
    "task_rx": (14, np.int32, lambda c: (c["tasks"],)),
    "task_pos": (15, np.float64, lambda c: (c["tasks"], 3)),
    "task_rms": (16, np.float64, lambda c: (c["tasks"],)),
    "task_status": (17, np.int32, lambda c: (c["tasks"],)),
    "task_nrx": (18, np.int32, lambda c: (c["tasks"],)),
    "task_iters": (19, np.int32, lambda c: (c["tasks"],)),
    "hdop": (20, np.float64, lambda c: (c["groups"],)),
    "vdop": (21, np.float64, lambda c: (c["groups"],)),
}


def posq3(group_ptr, row_rx0, row_rx1, row_tdoa, row_snr, rx_xyz, mode, group_h=None, row_weight=None, gate_m=0.0, ratio=0.5,
          min_rx=None, x0=(0.1, 0.1, 0.0), z_range=None, max_iter=100, outputs=None, device_id=0):
    """thr_posq3 on TDOA rows in CSR form (thr_pos3's columns: dense receiver indices into rx_xyz[n_rx, 3]) with an
    optional weight per row -> (counts dict, {name: array}) with every output of POSQ3_OUTPUTS (or those named in
    `outputs`) fetched.  mode POS3_KNOWN_HEIGHT reads group_h[g]; POS3_FREE_Z reads x0[2] and z_range.  gate_m == 0
    switches the exclusion off; min_rx None is the mode's floor (POSQ3_MIN_RX).  ValueError for what thr_posq3 refuses."""
    lib = load_library()
    ptr = np.ascontiguousarray(group_ptr, dtype=np.int64)
    rx0, rx1 = np.ascontiguousarray(row_rx0, dtype=np.int32), np.ascontiguousarray(row_rx1, dtype=np.int32)
    tdoa, snr = np.ascontiguousarray(row_tdoa, dtype=np.float64), np.ascontiguousarray(row_snr, dtype=np.float64)
    weight = None if row_weight is None else np.ascontiguousarray(row_weight, dtype=np.float64)
    xyz = np.ascontiguousarray(rx_xyz, dtype=np.float64)
    if (ptr.ndim != 1 or len(ptr) < 1 or xyz.ndim != 2 or xyz.shape[1] != 3 or
            not (len(rx0) == len(rx1) == len(tdoa) == len(snr) == int(ptr[-1]))):
        raise ValueError("posq3: group_ptr, the row columns or rx_xyz[n_rx, 3] have the wrong shape")
    if weight is not None and weight.shape != tdoa.shape:
        raise ValueError("posq3: one weight per row")
    n = len(ptr) - 1
    start = np.ascontiguousarray(x0, dtype=np.float64)
    if start.shape != (3,):
        raise ValueError("posq3: x0 holds three values")
    heights = None if group_h is None else np.ascontiguousarray(group_h, dtype=np.float64)
    if heights is not None and heights.shape != (n,):
        raise ValueError("posq3: group_h holds one height per group")
    box = None if z_range is None else np.ascontiguousarray(z_range, dtype=np.float64)
    if box is not None and box.shape != (2,):
        raise ValueError("posq3: z_range holds two values")
    if min_rx is None:
        min_rx = POSQ3_MIN_RX[1 if int(mode) == POS3_FREE_Z else 0]
    opts = ThrPosq3Opts(int(max_iter), int(min_rx), int(box is not None), (C.c_double * 3)(*start.tolist()),
                        (C.c_double * 2)(*(box.tolist() if box is not None else (0.0, 0.0))), float(gate_m), float(ratio))
    keep = np.zeros(1, dtype=np.float64)      # an empty column still needs a pointer that is not NULL
    handle, counts = C.c_void_p(), ThrPosq3Counts()
    rc = lib.thr_posq3(int(device_id), n, ptr.ctypes.data, rx0.ctypes.data, rx1.ctypes.data, tdoa.ctypes.data, snr.ctypes.data,
                       None if weight is None else (weight.ctypes.data if len(weight) else keep.ctypes.data),
                       xyz.shape[0], xyz.ctypes.data, int(mode), _ptr(heights), C.byref(opts), C.byref(handle), C.byref(counts))
    if rc == ERR_ARG:
        raise ValueError(lib.thr_last_error().decode())
    _check(lib, rc)
    c = {name: int(getattr(counts, name)) for name in POSQ_COUNTS}
    return c, _fetch_all(lib, "posq3", handle, c, POSQ3_OUTPUTS, outputs)


def posq3_times():
    """Milliseconds (HIP events) of this thread's last posq3(): copies in, full solves, flags and expansion, candidates,
    choice and residuals, copies out."""
    lib = load_library()
    ms = (C.c_double * 6)()
    _check(lib, lib.thr_debug_posq3_times(ms))
    return tuple(ms)
