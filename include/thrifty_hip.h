/*
 * thrifty_hip.h -- C ABI of the MI355X (gfx950) matched-filter detection engine.
 *
 * This is the drop-in boundary for the `thrifty detect` hot path.  Each entry
 * point names the reference interface it stands in for (paths relative to the
 * swkrueger/Thrifty checkout).  Conventions follow the reference's native twin
 * (fastcard/fastcard.h:46-53, fastdet/corr_detector.h:24-38): an opaque handle
 * created from a caller-owned settings struct, `int` status returns
 * (0 = ok, <0 = error; the message is available from thr_last_error()), the
 * library owns all FFT/work buffers, a handle is single-threaded / not
 * re-entrant, and distinct handles are fully independent (one per device and
 * stream), so a host may drive 8 GPUs from 8 processes or threads.
 *
 * No exceptions cross this boundary and no torch / C++ types appear in it: the
 * entry points are function-try-blocks (csrc/handle.hip: thr::on_exception) -- host
 * memory exhaustion or a thread the OS refuses come back as THR_ERR_DEVICE with a
 * message, a half-built handle or input window is torn down first.
 */
#ifndef THRIFTY_HIP_H
#define THRIFTY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: + thr_create_preshift / thr_create_fastdet, thr_detect_stream[_device], thr_detect_card,
 *    thr_identify (additions only: every version-1 entry point is unchanged) */
/* (3: THR_N_KERNEL_SLOTS 4 -> 5 (the arrays of thr_profile_read grow; slot 4 = the long-block
 *    combination kernel); everything else unchanged) */
/* 4: + thr_frame_card (addition only) */
/* 5: + thr_submit / thr_submit_card / thr_submit_stream / thr_collect / thr_inputs_consumed / thr_poll (asynchronous host
 *    boundary), thr_set_stream_default, thr_format_toad (additions only) */
/* 6: + thr_create_ex (explicit variant and kernel-path selection), thr_plan_sections,
 *    thr_host_register / thr_host_unregister, thr_input_window (additions only).
 *    No environment variable changes what a handle computes or how it schedules any more. */
/* 7: + thr_run_card / thr_run_stream (the whole file -> .toad loop in one call, text on a library
 *    thread), thr_get_settings, thr_input_window_ex (populator threads / segment size) / _release,
 *    thr_detect_offsets, thr_set_wait_mode, THR_PATH_GENERIC_ROWS, THR_ERR_INDEX, THR_FLAG_INT_OFFSET
 *    (additions only) */
/* 8: block_len 16384 with ONE template short enough for four 4096-sample sections (and no stddev
 *    term in the correlation threshold): THR_PATH_AUTO runs the correlate stage sectioned
 *    (csrc/detect16k_sec.hip); thr_plan_sections answers for block_len 16384 too,
 *    THR_PATH_UNSECTIONED applies to it, + THR_PATH_UNSECTIONED_GENERIC_ROWS, thr_debug_sections
 *    (additions; records of such handles change in the last bits of their float fields only) */
/* 9: block_len 16384: SEVERAL short templates run the sectioned correlate stage too (one forward
 *    transform per section, one product + inverse per template); + THR_FLAG_FIT_UNCONVERGED (the
 *    carrier fit's MINPACK exit code), thr_get_path_info (which kernels a handle's launches take, and
 *    why); thr_detect_offsets refuses non-finite offsets (additions; records of several-template
 *    handles change in the last bits of their float fields only) */
/* 10: + the carrier gate -- fastcard's job, raw capture -> carrier verdict -> .card, on the device:
 *    THR_VARIANT_GATE for thr_create_ex, thr_gate / thr_gate_stream / thr_gate_card,
 *    thr_gate_slot_stride, thr_format_card, thr_run_gate_stream / thr_run_gate_card (the whole file ->
 *    .card loop in one call) (additions only; thr_detect*, thr_submit*, thr_run_card / thr_run_stream,
 *    thr_detect_offsets and thr_debug_stage* refuse a gate handle with THR_ERR_STATE; the queries,
 *    thr_input_window*, thr_set_stream*, thr_sync, thr_profile_*, thr_debug_fft -- the carrier stage's
 *    spectrum -- and thr_compact_device are defined for it) */
/* 11: + template extraction -- the reference's `thrifty template_extract` (template_extract.py:36-58) on
 *    the device: thr_extract_create / _destroy / _reset, thr_extract_feed / _feed_card / _feed_stream,
 *    thr_extract_submit_card / _submit_stream, thr_extract_result, thr_run_extract_card /
 *    thr_run_extract_stream (additions only)
 *    within 11, a pure addition (no existing entry point or struct changes, the number stays):
 *    + thr_match / thr_debug_match_times -- the reference's `thrifty match` (matchmaker.py:17-79)
 *    + thr_tdoa / thr_debug_tdoa_times -- the reference's `thrifty tdoa` (tdoa_est.py:43-105, 234-303)
 *    + thr_pos / thr_debug_pos_times -- the reference's `thrifty pos` (pos_est.py:31-156)
 *    + thr_postdetect / thr_post_fetch / thr_post_free / thr_debug_post_times -- identify, match, tdoa and
 *      pos in one call with device-resident intermediates (the reference's kitchen_sink.postdetect)
 *    + thr_debug_live_resources -- what the process holds of the HIP runtime (the handles own it)
 *    + thr_survey_create / _destroy / _reset / _shift / _pending / _feed / _feed_stream,
 *      thr_debug_survey_geometry -- capture survey: mean spectrum, byte histogram, per-block byte sums
 *    + thr_chipscan / thr_debug_chipscan_geometry / _budget / _times -- chip-rate scan: blocks x candidate
 *      template lengths (the reference's scripts/chip_rate_search.py as an exhaustive scan)
 *    + thr_debug_chipscan_fill / _groups -- the scan's cut into groups of consecutive candidates: set the
 *      workgroups a launch aims at, read the cut (records unchanged)
 *    + thr_toadstats / thr_tstats_fetch / thr_tstats_free / thr_debug_toadstats_times / _geometry -- the
 *      numbers of the reference's `thrifty analyze_toads` (toads_analysis.py): per (rxid, txid) statistics,
 *      histograms and the per-receiver timestamp line
 *    + thr_debug_section_counts -- sections the one-template section kernel searched / left out by their
 *      energy bound (records unchanged)
 *    + thr_beaconsync / thr_bsync_fetch / thr_bsync_free and thr_tdoastats / thr_tdstats_fetch /
 *      thr_tdstats_free, with thr_debug_{beaconsync,tdoastats}_{times,geometry} -- the numbers of the
 *      reference's `thrifty analyze_beacon` and `thrifty analyze_tdoa`, for every cell in one call
 *    + thr_dossier_create / _destroy / _reset / _feed / _feed_card / _feed_stream / _result / _geometry -- the
 *      numbers of the reference's `thrifty analyze_detect` (detect_analysis.py): the first detected blocks
 *      inside a list of index ranges, kept on the device, and per kept block what its plots are drawn from
 *    + thr_tdoa_model and THR_TDOA_* -- thr_tdoa with the reference's weighted, nearest and linear models
 *      (tdoa_est.py:108-222); thr_post_settings.reserved (always 0) is now .tdoa_model, 0 = the polynomial
 *    + thr_reldist / thr_reldist_fetch / thr_reldist_free / thr_debug_reldist_times / _geometry -- the numbers
 *      of the reference's scripts/reldist_nearest.py (position along a baseline relative to a beacon, speed,
 *      carrier Doppler, both smoothed) for every (mobile, beacon, rx0 < rx1) cell in one call
 *    + thr_posq / thr_posq_fetch / thr_posq_free / thr_debug_posq_times -- thr_pos's 2-D solve with row weights,
 *      the residuals, the inverse normal matrix, and the exclusion of one receiver whose arrivals contradict
 *      the others (the open items of the reference's pos_est.py)
 *    + thr_track / thr_track_fetch / thr_track_free / thr_debug_track_times / _geometry -- per transmitter a
 *      constant-velocity Kalman filter over the positions in time order, a gate on the innovations and a
 *      fixed-interval smoother (the last open item of the reference's pos_est.py)
 *    + thr_posg / thr_posg_fetch / thr_posg_free / thr_debug_posg_times -- thr_pos's 2-D solve started from the
 *      lowest local minima of the cost surface on a grid over the receivers' surroundings as well: the best
 *      minimum, the runner-up, and whether the fixed start was wrong or two positions fit (the reference's "TODO:
 *      use analytic solution or previous position as initial value")
 *    + thr_debug_seg_tile_grid / thr_debug_seg_tile_stats -- the cap on the workgroups of a tile kernel of thr_toadstats,
 *      thr_beaconsync, thr_tdoastats, thr_reldist and thr_track (tests reach the loop's later trips at small
 *      shapes), and how many trips the launches since took (results unchanged)
 *    + thr_tdoamatrix / thr_tdmat_fetch / thr_tdmat_free / thr_debug_tdoamatrix_times / _geometry -- the numbers of
 *      the reference's scripts/tdoa_matrix.py: the TDOAs of every transmitter estimated again with ONE beacon's
 *      matches as the clock model, for every (rx0 < rx1, beacon, transmitter) cell in one call, with the cell's
 *      outlier mask and statistics (thr_tdoa_model's per-task arithmetic: csrc/tdoa_task.hpp states it once)
 *    + thr_coverage / thr_coverage_fetch / thr_coverage_free / thr_debug_coverage_times -- a coverage map of a
 *      deployment without a recording: per cell of a raster the dop, the predicted covariance of thr_pos's
 *      estimator under per-receiver arrival noise, and the error statistics of T simulated transmissions, each
 *      solved by thr_pos's own iteration (the reference's "TODO: estimate confidence with SNR and DOP")
 *    + thr_pos3 / thr_debug_pos3_times -- thr_pos's solve for receivers with three coordinates (pos-rx.cfg's
 *      `id: x y z`, the z of the reference's POSITION_INFO_DTYPE): (x, y) with the transmitter's height known, or
 *      (x, y, z) with dop split into its horizontal and vertical parts
 *    + thr_posg3 / thr_posg3_fetch / thr_posg3_free / thr_debug_posg3_times -- thr_posg's idea for thr_pos3's two
 *      modes: the cost on a grid x grid x grid_z volume (one plane with the height known), its lowest local minima as
 *      further starts of thr_pos3's own iteration, the best minimum, the runner-up, and a flag where the two differ
 *      in height only (the mirror about nearly coplanar antennas)
 *    + thr_posq3 / thr_posq3_fetch / thr_posq3_free / thr_debug_posq3_times -- thr_posq's weights, residuals,
 *      inverse normal matrix and receiver exclusion for thr_pos3's two modes
 *    + thr_extract_average / thr_extract_average_counts / thr_extract_average_result and thr_average_opts -- an
 *      extraction that also sums the cut of EVERY qualifying detection, per transmitter class: the averaged
 *      template, its standard error per sample and the counts (thr_extract_result's outputs unchanged) */
#define THR_ABI_VERSION 11

/* status codes */
#define THR_OK 0
#define THR_ERR_ARG (-1)      /* bad argument / unsupported configuration      */
#define THR_ERR_DEVICE (-2)   /* HIP runtime error (no GPU, OOM, launch failure) */
#define THR_ERR_STATE (-3)    /* call sequence error                            */
#define THR_ERR_INDEX (-4)    /* thr_run_*: a block on which the reference raises IndexError
                                 (THR_FLAG_INDEX_ERROR) ended the run                */

/* thr_record.flags */
#define THR_FLAG_CARRIER 1u      /* carrier_detect verdict (carrier_detect.py:95)  */
#define THR_FLAG_CORR 2u         /* correlation peak verdict (soa_estimator.py:85) */
#define THR_FLAG_INDEX_ERROR 4u  /* reference raises IndexError here: carrier bin
                                    + 3 >= block_len (carrier_sync.py:187)         */

#define THR_FLAG_FIT_UNCONVERGED 16u /* the Dirichlet carrier fit ended with MINPACK lmdif exit code 5 .. 8
                                    (600 evaluations, or a tolerance below machine precision): SciPy's
                                    curve_fit raises RuntimeError("Optimal parameters not found: ...")
                                    there and the reference does not catch it (carrier_sync.py:189), so
                                    its detect loop dies on that block.  The record is complete -- shift,
                                    FFT#2 and correlation ran with lmdif's last iterate -- and says so;
                                    Detector(strict_fit=True) raises like the reference.  Degenerate
                                    geometries only (templates far shorter than block_len / 24: the seven
                                    fitted points sit on a flat main lobe), and there the exit code hangs
                                    on the last digit of the seven magnitudes: the flagged blocks are the
                                    reference's to within that noise, not block for block. */
#define THR_FLAG_INT_OFFSET 8u   /* PreshiftDetector, cosine interpolator: the reference returned the
                                    Python int 0 (cos(omega) > 1, carrier_interpolators.py:87-88), so
                                    carrier_offset is 0 and prints as "0", not "0.0"                  */

/* input sample formats for thr_detect*() */
#define THR_IN_U8 0   /* interleaved unsigned 8-bit I,Q (RTL-SDR; block_data.py:38-52) */
#define THR_IN_C64 1  /* interleaved float32 re,im (a `Signal` already converted)     */

/*
 * Detector configuration.  Mirrors `DetectorSettings` (thrifty/detect.py:24-31)
 * plus what `Detector.__init__` derives from it (detect.py:40-58); the native
 * twin's equivalent is fargs_t + CorrDetector's ctor (corr_detector.h:26-30).
 */
typedef struct thr_settings {
    int32_t block_len;        /* samples per block, power of two                   */
    int32_t history_len;      /* samples repeated from the previous block          */
    int32_t n_templates;      /* >= 1 (the reference has exactly 1); 0: THR_VARIANT_GATE */
    int32_t template_len;     /* samples per template (all templates equal length) */
    const double* templates;  /* [n_templates][template_len], real, time domain    */
    int32_t carrier_len;      /* Dirichlet-kernel width; 0 = template_len          */
    int32_t carrier_window[2];/* closed bin interval, negative = wrap
                                 (carrier_detect.py:17-58); {0,-1} = all bins       */
    double carrier_thresh[3]; /* (constant, snr, stddev) carrier_detect.py:110-115 */
    double corr_thresh[3];    /* (constant, snr, stddev) soa_estimator.py:127-134  */
    int32_t device_id;        /* HIP device ordinal                                */
    int32_t max_batch;        /* largest number of blocks per thr_detect*() call   */
} thr_settings;

/*
 * One detection record per (block, template): the payload of
 * `DetectionResult` / `CarrierSyncInfo` / `CorrDetectionInfo`
 * (thrifty/toads_data.py:8-45) and of fastdet's CorrDetection
 * (corr_detector.h:14-22).  64 bytes, written densely as out[block][template].
 */
typedef struct thr_record {
    int64_t block_idx;      /* caller's block index (passed through)              */
    uint32_t flags;         /* THR_FLAG_*                                          */
    int32_t template_id;    /* 0 .. n_templates-1                                  */
    int32_t carrier_bin;    /* CarrierSyncInfo.bin                                 */
    int32_t corr_sample;    /* CorrDetectionInfo.sample (-1 if no carrier)         */
    double carrier_offset;  /* CarrierSyncInfo.offset (0 if no carrier)            */
    double corr_offset;     /* CorrDetectionInfo.offset, clipped to +-0.6          */
    float carrier_energy;   /* CarrierSyncInfo.energy (peak magnitude)             */
    float carrier_noise;    /* CarrierSyncInfo.noise  (rms)                        */
    float corr_energy;      /* CorrDetectionInfo.energy (peak magnitude)           */
    float corr_noise;       /* CorrDetectionInfo.noise  (rms)                      */
    uint64_t reserved;      /* 0 (default detector); see thr_create_preshift       */
} thr_record;

typedef struct thr_handle thr_handle;

/* Library / ABI identification. */
int thr_abi_version(void);
const char* thr_last_error(void);

/*
 * Replaces `Detector.__init__` (detect.py:40-58: DefaultSynchronizer +
 * SoaEstimator construction incl. template zero-pad + FFT,
 * soa_estimator.py:63-76) and fastcard_new()/CorrDetector::CorrDetector
 * (fastcard.c:13-117, corr_detector.cpp:31-86).  `settings` and the template
 * array need only live for the duration of the call.
 */
int thr_create(const thr_settings* settings, thr_handle** out);
/*
 * PreshiftDetector variant -- replaces `PreshiftDetector.__init__` + `TemplateShifts`
 * (thrifty/experimental/detect_preshift.py:24-60; defaults num=21, parabolic carrier
 * interpolator experimental/carrier_interpolators.py:40-45, corr_shift off): the
 * carrier offset is a 3-point parabola on |FFT#1|, FFT#1 is rolled by the rounded shift
 * (freq_shift_integer, carrier_sync.py:241-245) and correlated against the nearest of
 * `num_shifts` template spectra pre-shifted by -0.5 .. +0.5 bin.  Every other entry
 * point then behaves as documented with these semantics: carrier_offset is the float32
 * parabola offset; THR_FLAG_INDEX_ERROR marks carrier_bin + 1 >= block_len (where the
 * reference's fft_mag[peak+1] raises); `reserved` = (uint32 rolled shift << 32) | bank
 * index.  One template only; thr_debug_stage dumps (np.roll(FFT#1, shift) and the correlation,
 * what the reference class returns under yield_data) need a THR_PATH_MULTIPASS handle.  block_len 16384
 * runs ONE fused kernel per block (FFT, verdict, gather-multiply, IFFT); other lengths
 * use the multi-pass pipeline.
 */
int thr_create_preshift(const thr_settings* settings, int num_shifts, thr_handle** out);
/*
 * fastdet-compatible variant -- the algorithm of the reference's NATIVE detector
 * (fastcard/cardet.c:7-41 + fastdet/corr_detector.cpp:88-197), which differs from the Python
 * one: float32 power-domain verdicts `max > c + s * noise_power` for carrier and correlation
 * (carrier_thresh / corr_thresh hold c, s in the POWER domain; the third coefficient must be
 * 0), carrier noise (sum - 2 max)/(N - 1), correlation noise clamped at 0 and computed from
 * the integer-truncated peak power, integer roll by -argmax against the unshifted template
 * (no FFT#2), carrier offset = parabola on sqrt(power) and correlation offset = Gaussian on
 * log sqrt(power), both clipped to +-0.5, window [min, max] non-wrapping (a window with
 * min < 0 <= max is refused like cardet_normalize_window, cardet.c:44-48).  Records then hold
 * what fastdet prints (fastdet.cpp:188-206): energies / noises are the square roots of the
 * powers.  Same kernel structure as the preshift variant (one fused kernel at 16384).
 * Parity status: restated from the C/C++ sources; fastdet itself needs FFTW3f, VOLK and
 * librtlsdr and cannot be built in this environment, so this variant is NOT pinned against
 * reference output.
 */
int thr_create_fastdet(const thr_settings* settings, thr_handle** out);
/*
 * The three constructors above in one call, plus an explicit choice of kernel path.  `variant`:
 * THR_VARIANT_DEFAULT (thr_create), THR_VARIANT_PRESHIFT (thr_create_preshift; variant_arg =
 * num_shifts | THR_INTERP_* << 16: the bank size and the carrier interpolator, one of the reference's
 * thrifty/experimental/carrier_interpolators.py -- parabolic (:40-45, what thr_create_preshift uses
 * and the reference's default), none (:17-18), gaussian (:48-54), cosine (:84-92); float32 like the
 * magnitudes they are given) or THR_VARIANT_FASTDET (thr_create_fastdet).  `path`:
 *   THR_PATH_AUTO         what the other constructors use: the fastest kernels for the block
 *                         length (LDS-resident for 1024 ... 65536, multi-pass otherwise);
 *   THR_PATH_MULTIPASS    the generic multi-pass pipeline (Stockham passes through HBM) whatever
 *                         the block length -- an independent implementation of the same arithmetic,
 *                         kept for cross-checking the fused kernels on identical input;
 *   THR_PATH_UNSECTIONED  the correlate stage as ONE block_len-point transform pair instead of
 *                         overlap-save sections: block_len 32768 / 65536 (decimated sub-transforms,
 *                         detect_long.hip, instead of sections of 16384 points, detect_seg.hip --
 *                         AUTO falls back to it by itself for templates longer than 9361 samples at
 *                         65536) and block_len 16384 (k_correlate instead of up to four sections of
 *                         4096 points, detect16k_sec.hip, which AUTO takes for templates -- one or
 *                         several, ABI 9 -- of at most about 1000 samples with no stddev threshold
 *                         term; thr_get_path_info says which a handle got and why).  thr_debug_stage
 *                         dumps always come from the unsectioned kernels.
 *   THR_PATH_GENERIC_ROWS AUTO, except that the correlate kernel of block_len 16384 (and of the
 *                         sections of longer blocks) is the generic one, with the unique-window test
 *                         in all 16 rows of lags, instead of the window-row specialisation the
 *                         geometry selects (csrc/correlate16k_geom.hpp): same arithmetic, so the
 *                         records are equal byte for byte -- which is what the tests use it for.
 *                         (A sectioned block_len 16384 handle: the same, for its sections' rows.)
 *   THR_PATH_UNSECTIONED_GENERIC_ROWS  both of the above (block_len 16384: the generic k_correlate).
 * All paths implement the same reference semantics and agree to rounding (tests/test_gpu_*.py).
 *
 * THR_VARIANT_GATE (ABI 10): the carrier gate, see thr_gate below.  n_templates = 0, templates =
 * NULL, template_len / carrier_len / corr_thresh ignored; carrier_thresh = {constant, snr, 0} in the
 * POWER domain, narrowed to float32 like fastcard's (fargs_type.h); carrier_window = [min, max] checked
 * like cardet_normalize_window (cardet.c:43-70: negative = from the end, min < 0 <= max refused,
 * out of range refused, swapped if reversed).  No template spectra and no correlate buffers are built.
 */
#define THR_VARIANT_DEFAULT 0
#define THR_VARIANT_PRESHIFT 1
#define THR_VARIANT_FASTDET 2
#define THR_VARIANT_GATE 3
#define THR_INTERP_PARABOLIC 0
#define THR_INTERP_NONE 1
#define THR_INTERP_GAUSSIAN 2
#define THR_INTERP_COSINE 3
#define THR_PATH_AUTO 0
#define THR_PATH_MULTIPASS 1
#define THR_PATH_UNSECTIONED 2
#define THR_PATH_GENERIC_ROWS 3
#define THR_PATH_UNSECTIONED_GENERIC_ROWS 4
int thr_create_ex(const thr_settings* settings, int variant, int variant_arg, int path, thr_handle** out);
/*
 * The overlap-save plan THR_PATH_AUTO uses for the correlate stage of a long block (host-only, no
 * device involved; exported so that the plan itself can be checked against the reference's
 * `despread` / `get_peak`, soa_estimator.py:97-102,137-143, on a CPU).  Section g transforms samples
 * [start[g], start[g] + 16384) of the frequency-shifted block against the template zero-padded to
 * 16384; lag j of that circular correlation, 0 <= j <= 16384 - template_len, is lag start[g] + j of
 * the block's.  In block coordinates section g searches the window lags [win_lo[g], win_hi[g]) and
 * sums (stddev threshold term) the lags [sum_lo[g], sum_hi[g]): the window ranges tile the unique
 * window of soa_estimator.calculate_window (soa_estimator.py:20-39) and the sum ranges tile
 * [0, corr_len), each exactly once, ascending in g, and every searched lag has both neighbours
 * inside its section.  Arrays hold THR_MAX_SECTIONS ints.  *n_sections = 0 when the block is not
 * sectioned (block_len < 16384, or more than THR_MAX_SECTIONS would be needed: templates longer
 * than 9361 samples at block_len 65536).
 * block_len 16384 (ABI 8): sections of 4096 samples, [start[g], start[g] + 4096), starts on multiples
 * of 8 samples, at most FOUR (a fifth would cost more than the 16384-point transform pair: *n_sections
 * = 0 then, as for templates longer than 4081 samples); only the unique window is tiled (win_lo /
 * win_hi; sum_lo = sum_hi = start: a stddev threshold term keeps the unsectioned kernel), and a
 * searched lag has both neighbours inside its section unless it is the first or the last kept lag
 * of the block, where the reference takes no neighbours either (soa_estimator.py:163-164).
 * Geometry only: whether an engine handle uses the plan also depends on its block length, template
 * count, thresholds and path (thr_debug_sections).
 */
#define THR_MAX_SECTIONS 8
int thr_plan_sections(int block_len, int history_len, int template_len, int* n_sections, int* start,
                      int* win_lo, int* win_hi, int* sum_lo, int* sum_hi);
/* Replaces fastcard_free() (fastcard.c:119-146). */
void thr_destroy(thr_handle* h);

/*
 * Replaces the body of the hot loop: `Detector.detect` (detect.py:60-78) ==
 * Synchronizer.sync (carrier_sync.py:52-76) + SoaEstimator.soa_estimate
 * (soa_estimator.py:78-92), and fastcard_process() + CorrDetector::detect()
 * (fastcard.c:177-189, corr_detector.cpp:177-197), for `n_blocks` blocks at once.
 *
 * Host-buffer form: `samples` is n_blocks * block_len samples in `format`
 * (u8: 2 bytes/sample; c64: 8 bytes/sample) in host memory; `block_idx` (may be
 * NULL -> 0,1,2,...) is copied into the records; `out` receives
 * n_blocks * n_templates records, ordered [block][template].  Synchronous.
 */
int thr_detect(thr_handle* h, const void* samples, int format, const int64_t* block_idx,
               size_t n_blocks, thr_record* out);

/*
 * thr_detect() with the sub-bin carrier offsets GIVEN -- replaces `Synchronizer.sync` with a replaced
 * `interpolator` (carrier_sync.py:52-76: `offset = self.interpolator(fft_mag, peak_idx)`, then the
 * shift by -(peak_idx + offset)): what the reference's InterpolationDetector
 * (thrifty/experimental/detect_carrier_interpol.py:17-40) does with any function of
 * thrifty/experimental/carrier_interpolators.py:17-81.  The caller has run the carrier stage once
 * (thr_detect + thr_debug_fft give it the peak bin and |FFT#1|), evaluated its interpolator on the
 * host and hands the results back: block i is shifted by -(its carrier bin + carrier_offset[i])
 * instead of by the Dirichlet fit; everything downstream (FFT#2, correlation, SoA) is unchanged and
 * the record carries carrier_offset[i].  Entries of blocks without a carrier are ignored.  The
 * reference's IndexError rule belongs to ITS interpolator (carrier_sync.py:187) and is not applied:
 * THR_FLAG_INDEX_ERROR is never set here.  One batch (n_blocks <= max_batch), host pointers,
 * synchronous, the default detector only.  A slow path by design (two passes over the block and a
 * host round trip per batch) -- for analysis scripts, not for throughput.
 */
int thr_detect_offsets(thr_handle* h, const void* samples, int format, const int64_t* block_idx,
                       size_t n_blocks, const double* carrier_offset, thr_record* out);

/*
 * .card form (ingest on the device).  `text` holds .card records
 * "<timestamp> <block_idx> <base64 of 2*block_len bytes>" (block_data.py:120-131;
 * fastcard_cli.c:187-192); `payload_off[i]` is the byte offset of the i-th block's base64
 * payload inside `text` (the host only splits lines).  The text crosses PCIe once and is
 * decoded on the device (replaces base64.b64decode + np.fromstring, block_data.py:129, and
 * fastcard/lib/base64.c), then processed exactly like thr_detect().  Host pointers,
 * synchronous.  Invalid base64 -> THR_ERR_ARG.
 */
/*
 * Host-side framing for thr_detect_card(): find the records of a .card text.  Skips what the
 * reference's card_reader skips (block_data.py:101-131: '#' comments, blank lines, fastcard's
 * banner lines "Using Volk machine:" / "linux;"); every other line must be
 * "<timestamp> <block_idx> <payload>" with a payload of exactly 4*ceil(2*block_len/3)
 * characters.  Frames at most `max_records` whole lines starting at `text`; a last line without
 * a newline counts only if `at_eof`.  Outputs per record: timestamp (correctly rounded, like
 * Python's float()), block index, payload offset relative to `text`; `*consumed` = bytes
 * framed (the next call starts there).  No device involved.  Malformed line -> THR_ERR_ARG -- from
 * the call that STARTS at it: a call that meets it after whole records returns those first (the
 * reference's per-line loop had processed them before it raised).
 */
int thr_frame_card(const char* text, size_t text_len, int block_len, int at_eof, size_t max_records,
                   double* timestamps, int64_t* block_idx, int64_t* payload_off, size_t* n_records,
                   size_t* consumed);

/*
 * Page-lock caller memory that the host entry points read from -- typically the mmap of the input
 * file (`thrifty detect rx.card` / `--raw`): the chunk copies of thr_detect / thr_detect_card /
 * thr_detect_stream and their thr_submit_* forms then run as DMA straight from the page cache and
 * RETURN AT ONCE, instead of occupying the calling thread for the length of each copy while the
 * HIP runtime stages pageable memory (same PCIe rate either way -- measured 56 GB/s on MI355X --
 * but the host thread frames the next chunk and formats the previous one's output meanwhile).
 * Purely an optimisation: everything works on unregistered memory, and a failed registration
 * (THR_ERR_DEVICE: locked-memory limit, exotic mapping) leaves nothing behind.  The range is
 * widened to whole pages; read-only and private file mappings are fine.  No handle: the lock
 * belongs to the process.  Unregister (same pointer) before unmapping; inputs of open tickets
 * must have been consumed (thr_inputs_consumed / thr_collect).
 */
int thr_host_register(const void* p, size_t bytes);
int thr_host_unregister(const void* p);
/*
 * The streaming form, for inputs of any size: declare [p, p + bytes) -- the mmap of the input file
 * -- as the window this handle's host entry points will read FRONT TO BACK.  A worker thread of
 * the library page-locks it 128 MiB at a time, at most 1 GiB ahead of the chunk copies, and
 * unlocks what they have left behind, so the locking costs neither the caller's time (it runs
 * beside the copies: measured 10-40 ms per GiB, about what the staging of pageable memory costs the
 * calling thread) nor more locked memory than that, however large the file.  Source ranges
 * outside the window, behind its read position or far ahead of it are copied as ordinary pageable
 * memory, as is everything once a lock is refused -- results never depend on the window.
 * (NULL, 0) closes it; thr_destroy does too.  Not while tickets are open (THR_ERR_STATE).  The
 * mapping must stay valid until the window is closed.
 */
int thr_input_window(thr_handle* h, const void* p, size_t bytes);
/*
 * The same with its two resources stated: `populate_threads` (1 .. 16; 0 = the default, 3) threads
 * map the pages of a segment ahead of the locking worker -- on a node whose CPUs are shared by
 * several ranks a caller gives each rank its share (thrifty_amd.parallel.populate_threads: CPUs /
 * world - 3, at least 1); `segment_bytes` (a power of two >= 64 KiB; 0 = the default, 128 MiB) is
 * the locking granularity -- the tests shrink it to put segment boundaries where they want them.
 */
int thr_input_window_ex(thr_handle* h, const void* p, size_t bytes, int populate_threads, size_t segment_bytes);
/*
 * "The input has been read": no further copy will come out of the window.  Returns at once; what is
 * still page-locked (the segments of the last chunks) is unlocked by the window's own thread in the
 * background -- a few milliseconds of hipHostUnregister that a caller writing its last output line
 * need not wait for.  Source ranges inside the window are copied as pageable memory from here on.
 * The mapping must STILL stay valid until thr_input_window(h, NULL, 0), the next
 * thr_input_window[_ex] on this handle or thr_destroy has returned: those wait for the unlocking.
 * Not while tickets are open (THR_ERR_STATE).
 */
int thr_input_window_release(thr_handle* h);

int thr_detect_card(thr_handle* h, const char* text, size_t text_len, const int64_t* payload_off,
                    const int64_t* block_idx, size_t n_blocks, thr_record* out);

/*
 * Raw-stream framing on the device.  Replaces the overlap bookkeeping of
 * `block_reader` (thrifty/block_data.py:70-98: block = previous block's last
 * `history_len` samples + `block_len - history_len` new ones) and of fastcard's
 * raw_reader_next (fastcard/lib/raw_reader.c:15-46): `stream` is the receiver's
 * interleaved u8 I/Q byte stream and block i is the 2*block_len bytes starting
 * 2*(block_len - history_len)*i bytes into it -- the kernels read overlapping
 * windows in place, nothing is copied or re-framed.  Needs an even
 * block_len - history_len (4-byte aligned block starts), else THR_ERR_ARG.
 * The reference's very first block has an all-zero (0.0, not quantiser-zero)
 * history and therefore no u8 form: callers send that one block through
 * thr_detect(..., THR_IN_C64, ...) (thrifty_amd/block_data.py:RawStream does).
 *
 * thr_detect_stream: host pointer, synchronous; processes the
 *   (n_bytes - 2*block_len) / (2*(block_len - history_len)) + 1 whole blocks the
 *   stream holds (0 if shorter than one block), numbers them first_block_idx,
 *   first_block_idx+1, ..., writes [n_blocks][n_templates] records and stores
 *   the block count in *n_blocks_out.  `out_capacity` is in blocks.
 * thr_detect_stream_device: device pointers, asynchronous like
 *   thr_detect_device; n_blocks <= max_batch; d_stream must hold
 *   (n_blocks-1)*2*(block_len-history_len) + 2*block_len bytes.
 */
int thr_detect_stream(thr_handle* h, const uint8_t* stream, size_t n_bytes, int64_t first_block_idx,
                      thr_record* out, size_t out_capacity, size_t* n_blocks_out);
int thr_detect_stream_device(thr_handle* h, const uint8_t* d_stream, const int64_t* d_block_idx,
                             size_t n_blocks, thr_record* d_out);

/*
 * Device-resident form (what bench.py times): `d_samples`, `d_block_idx`
 * (may be NULL) and `d_out` are device pointers on the handle's device.  The
 * work is enqueued on the handle's stream and NOT synchronised; call
 * thr_sync() (or synchronise the stream you passed to thr_set_stream()).
 */
int thr_detect_device(thr_handle* h, const void* d_samples, int format,
                      const int64_t* d_block_idx, size_t n_blocks, thr_record* d_out);
int thr_sync(thr_handle* h);
/* Use an externally owned hipStream_t (e.g. a torch side stream); NULL restores the handle's own
 * (non-blocking) stream -- NOTE that torch's DEFAULT stream has the handle value 0, i.e. NULL:
 * passing it here selects the engine's own stream, which does not synchronise with the legacy
 * default stream; to run ON the default stream call thr_set_stream_default() instead
 * (thrifty_amd._native.Engine.set_stream(0) does). */
int thr_set_stream(thr_handle* h, void* hip_stream);
/* Run on the device's legacy default stream (the one torch's default stream and every other
 * blocking stream are ordered with) -- what a caller holding `torch.cuda.current_stream()` on the
 * default stream wants: fills and copies queued there are then ordered before the engine's
 * kernels without any explicit synchronisation. */
int thr_set_stream_default(thr_handle* h);

/*
 * Asynchronous host boundary (precedent: the producer/consumer split fastdet
 * planned and never built, fastdet/fastdet.cpp:179-180).  thr_submit*() is thr_detect*() for ONE
 * batch (n_blocks <= max_batch) cut in two: it stages the inputs, enqueues the copies and kernels,
 * and returns a ticket while the device works; thr_collect(ticket) waits for that batch and fills
 * the `out` array given at submit time (caller-owned; it must stay valid and untouched until the
 * collect returns -- the records travel through pinned staging owned by the library).  The INPUT
 * arrays (samples / text / stream, offsets, indices) must stay valid until
 * thr_inputs_consumed(ticket) -- which waits for the batch's host-to-device copies only, not for
 * its kernels -- or thr_collect(ticket) has returned.  Up to THR_MAX_IN_FLIGHT tickets may be open per
 * handle (a further submit fails with THR_ERR_STATE); tickets may be collected in any order, each
 * exactly once; batches execute in submission order.  Ticket 0 is what an empty batch gets and
 * needs no collect.  The synchronous host entry points refuse to run while tickets are open.
 * thr_poll: *done = 1 if thr_collect(ticket) would not block.
 * Same single-threaded-per-handle rule as everything else.
 */
#define THR_MAX_IN_FLIGHT 3
int thr_submit(thr_handle* h, const void* samples, int format, const int64_t* block_idx,
               size_t n_blocks, thr_record* out, uint64_t* ticket);
int thr_submit_card(thr_handle* h, const char* text, size_t text_len, const int64_t* payload_off,
                    const int64_t* block_idx, size_t n_blocks, thr_record* out, uint64_t* ticket);
int thr_submit_stream(thr_handle* h, const uint8_t* stream, size_t n_bytes, int64_t first_block_idx,
                      thr_record* out, size_t out_capacity, size_t* n_blocks_out, uint64_t* ticket);
int thr_collect(thr_handle* h, uint64_t ticket);
/*
 * How thr_collect (and the drains of the synchronous host entry points, and thr_run_*) wait for a
 * batch: 0 (default) = hipEventSynchronize -- the HIP runtime polls, the calling thread is busy for
 * the length of the wait: lowest latency, one CPU per handle; 1 = ask (hipEventQuery) and nap 40 us
 * in between -- for hosts whose CPUs are shared by several ranks (eight ranks on a 16-CPU cgroup:
 * eight polling threads would take half of it from the ranks' text and page-locking threads).  With
 * batches in flight ahead of the one waited for, the naps cost no throughput.
 */
int thr_set_wait_mode(thr_handle* h, int sleeping);
int thr_inputs_consumed(thr_handle* h, uint64_t ticket);
int thr_poll(thr_handle* h, uint64_t ticket, int* done);

/*
 * `.toad` text for a batch of DETECTED records -- replaces `DetectionResult.serialize`
 * (thrifty/toads_data.py:47-61) called once per detection by detector_cli (detect.py:217-219).
 * One line per record, each ending in '\n':
 *   [rxid ][txid ]t block soa sample offset energy noise cbin coffset cenergy cnoise
 * t as %.6f, soa = new_len * block_idx + corr_sample + corr_offset as %.8f, the integers as
 * str(int), every other float as Python's repr() of the value widened to a double (what
 * '{}'.format gives for a float and for an np.float32).  with_rxid / with_txid: prepend the
 * ids like serialize() does for values that are not None (txid = the record's template_id:
 * multi-template detection); carrier_offset_f32: 1 = round the carrier offset to float32 first
 * (PreshiftDetector's np.float32 offset), 2 = print it as an integer (its interpolator `none`
 * returns the int 0); a record flagged THR_FLAG_INT_OFFSET prints it as an integer whatever the mode.
 * `out_capacity` must be >= n * THR_TOAD_LINE_MAX.
 * Host only, no device, handle-free.
 */
#define THR_TOAD_LINE_MAX 384
int thr_format_toad(const thr_record* recs, const double* timestamps, size_t n, int64_t new_len,
                    int with_rxid, int64_t rxid, int with_txid, int carrier_offset_f32, char* out,
                    size_t out_capacity, size_t* out_len);

/*
 * The whole `thrifty detect <file> -o <toad>` loop in ONE call -- replaces the reference's per-block
 * loop (detect.py:197-223: card_reader / block_reader -> Detector.detect -> `if detected:
 * print(result.serialize())`; block_data.py:70-131) for an input that lies in memory (the mmap of
 * the file, or a rank's shard of it).  Built on the entry points above and nothing else: the calling
 * thread frames batches (thr_frame_card), keeps up to THR_MAX_IN_FLIGHT of them submitted
 * (thr_submit_card / thr_submit_stream) and collects them in order; a thread of the library keeps the
 * DETECTED records of each collected batch, formats them (thr_format_toad) and write()s the text to
 * `out_fd`, and / or appends the records -- each with its timestamp's bits in `reserved` -- to
 * `rec_out` (what the ranks of a sharded run exchange).  No interpreter in the loop, no hand-over of
 * a lock between the two threads.
 *
 * Semantics are those of the batched Python loop (thrifty_amd/detect.py), i.e. the reference's:
 *  - output order = input order; only blocks whose correlation verdict is positive produce a line;
 *  - a block flagged THR_FLAG_INDEX_ERROR (the reference raises IndexError there,
 *    carrier_sync.py:187) ends the run: the detections before it are written, the call returns
 *    THR_ERR_INDEX and `stats` names the block;
 *  - a malformed .card line (THR_ERR_ARG from thr_frame_card) or an invalid base64 payload ends it
 *    likewise, after everything before the offending batch has been written.
 * thr_run_card: `text` = .card text (whole lines; the last one may lack its newline).
 * thr_run_stream: `stream` = raw interleaved u8 I/Q whose first 2*block_len bytes are block
 *   `first_block_idx` (overlap framing as thr_detect_stream; the caller sends the reference's
 *   zero-history lead-in blocks through thr_detect as before and starts here behind them); every
 *   block of a batch is stamped with the wall clock when the batch is framed (`timestamp` NaN) or
 *   with `timestamp`.
 * If the handle has an input window (thr_input_window) around the input, the copies are DMA from
 * the page cache as usual.  The handle must have no open tickets.
 */
typedef struct thr_run_opts {
    uint32_t struct_bytes;        /* sizeof(thr_run_opts) -- guards the layout                     */
    int32_t batch_blocks;         /* blocks per submitted batch; 0 = the handle's max_batch          */
    int32_t out_fd;               /* >= 0: the .toad text is written here; -1: no text               */
    int32_t with_rxid;            /* the arguments of thr_format_toad ...                            */
    int64_t rxid;
    int32_t with_txid;
    int32_t carrier_offset_mode;  /* ... its carrier_offset_f32                                      */
    double timestamp;             /* thr_run_stream only, see above                                  */
    thr_record* rec_out;          /* NULL, or room for rec_capacity detected records                 */
    size_t rec_capacity;
} thr_run_opts;
typedef struct thr_run_stats {
    uint64_t blocks;              /* blocks whose records were handed to the formatter               */
    uint64_t detections;          /* lines written / records appended                                */
    uint64_t batches;
    uint64_t bytes_in;            /* input bytes framed                                              */
    uint64_t text_bytes;          /* bytes written to out_fd                                         */
    uint64_t index_error_at;      /* position (0-based, in this run) of the block that ended the run
                                     with THR_ERR_INDEX; UINT64_MAX otherwise                        */
    int64_t index_error_block;    /* its block index                                                 */
    int32_t index_error_bin;      /* its carrier bin                                                 */
    int32_t reserved_;
    double total_s;               /* where the calling thread's time went: the whole call,           */
    double frame_s, submit_s, wait_s;     /* framing, thr_submit*, waiting in thr_collect            */
    double format_s, write_s;     /* the library thread: thr_format_toad, write()                    */
} thr_run_stats;
int thr_run_card(thr_handle* h, const char* text, size_t text_len, const thr_run_opts* opts,
                 thr_run_stats* stats);
int thr_run_stream(thr_handle* h, const uint8_t* stream, size_t n_bytes, int64_t first_block_idx,
                   const thr_run_opts* opts, thr_run_stats* stats);
/*
 * The carrier gate -- replaces the reference's `fastcard` for inputs that lie in memory
 * (fastcard/fastcard.c:177-189 + cardet.c:7-41 + fastcard_cli.c:171-194): which blocks of a capture
 * carry a carrier, and those blocks as base64, ready to be written as .card lines.  The handle comes
 * from thr_create_ex(..., THR_VARIANT_GATE, ...).  Per block, in float32 like cardet:
 *   sum = sum |X|^2 over all block_len bins, max = the first maximum of |X|^2 over the window,
 *   noise = (sum - 2 max) / (block_len - 1) (0 when sum == 0), threshold = c + s * noise,
 *   passed = max > threshold.
 * (The carrier stage is the detectors': it takes the first maximum of the float32 MAGNITUDE, so the
 * bin can differ from cardet's only where two window powers round to one magnitude.)
 * out[i], one record per block: flags = THR_FLAG_CARRIER when passed, carrier_bin = the maximum's bin,
 * carrier_energy = sqrt(max) and carrier_noise = sqrt(noise) -- what fastcard's info line prints
 * (fastcard_cli.c:175-180; NaN where noise < 0) -- the float32 bits of `threshold` in the low half of
 * `reserved`, corr_sample = -1, every other field 0.
 * slots: the k-th passed block, in input order, gets the slot slots[k * slot_stride ...]: payload_chars
 * = 4 * ceil(2 * block_len / 3) characters of canonical base64 ('=' padded) of its 2 * block_len raw
 * bytes, then '\n'; the bytes from there to the next slot are not written.  thr_gate_slot_stride
 * tells both numbers (slot_stride = payload_chars + 1 rounded up to 16).  `slots_capacity` (bytes) must
 * hold a slot for EVERY block of the call -- all of them may pass -- else THR_ERR_ARG before any device
 * work; *n_passed slots are written.  Only passed blocks are encoded and only their slots cross PCIe.
 * Host pointers, synchronous, any number of blocks (chunks of at most max_batch).
 *   thr_gate         packed u8 blocks, block_idx as in thr_detect (NULL: 0, 1, 2, ...)
 *   thr_gate_stream  raw stream, framing and first_block_idx as in thr_detect_stream: block i is
 *                    the 2 * block_len bytes 2 * (block_len - history_len) * i bytes into `stream`
 *   thr_gate_card    .card text + payload offsets (thr_frame_card), decoded on the device as in
 *                    thr_detect_card: re-filter an existing .card with another window or threshold
 */
int thr_gate_slot_stride(const thr_handle* h, size_t* slot_stride, size_t* payload_chars);
int thr_gate(thr_handle* h, const uint8_t* samples, const int64_t* block_idx, size_t n_blocks, thr_record* out,
             size_t* n_passed, char* slots, size_t slots_capacity);
int thr_gate_stream(thr_handle* h, const uint8_t* stream, size_t n_bytes, int64_t first_block_idx, thr_record* out,
                    size_t out_capacity, size_t* n_blocks_out, size_t* n_passed, char* slots,
                    size_t slots_capacity);
int thr_gate_card(thr_handle* h, const char* text, size_t text_len, const int64_t* payload_off,
                  const int64_t* block_idx, size_t n_blocks, thr_record* out, size_t* n_passed, char* slots,
                  size_t slots_capacity);
/*
 * .card lines from payload slots -- the inverse of thr_frame_card; replaces fastcard_cli.c:187-192
 * ("%ld.%06ld %PRId64 %s\n").  Line i = timestamps[i] split into seconds and microseconds (rounded to
 * the nearest microsecond, ties to even: a fraction >= .9999995 carries into the seconds, like
 * thrifty_amd.block_data.card_line), block_idx[i], the first `payload_chars` characters of slot i.
 * `out_capacity` must be >= n * (THR_CARD_HEADER_MAX + payload_chars + 1).  Host only, no device,
 * handle-free.
 */
#define THR_CARD_HEADER_MAX 48
int thr_format_card(const double* timestamps, const int64_t* block_idx, const char* slots, size_t slot_stride,
                    size_t payload_chars, size_t n, char* out, size_t out_capacity, size_t* out_len);

/*
 * The whole `fastcard -i <file> [--card] -o <out.card>` loop in ONE call (fastcard_cli.c:143-196) for an
 * input that lies in memory (the mmap of the file), the twin of thr_run_stream / thr_run_card and built
 * the same way, on the entry points above: the calling thread frames a batch and gates it; a thread of
 * the library assembles the .card lines of the passed blocks and writev()s them to `out_fd`, so the text
 * of one batch leaves while the next is on the device (up to three batches between the two threads).
 * Output order = input order.  If the handle has an input window around the input, the chunk copies
 * are DMA from the page cache and the window is released behind them.
 * thr_run_gate_stream: `stream` = the raw u8 I/Q capture from its first byte.  Framing is the
 *   reference's (raw_reader.c:15-46, fastcard_cli.c:151-169): the reader takes block_len - history_len
 *   new samples per block, the first `skip` blocks are dropped, kept block i (index first_block_idx + i;
 *   fastcard: 0) is the window that starts 2 * (block_len - history_len) * (i + skip) - 2 * history_len
 *   bytes into the stream and is read in place; where that is negative the missing history is ZERO
 *   BYTES (the one deviation: the reference leaves it uninitialised, reader.c:49).  Every block of a
 *   batch is stamped with the wall clock when the batch is framed (`timestamp` NaN) or with `timestamp`.
 * thr_run_gate_card: `text` = .card text; timestamps and indices are the input lines', the first `skip`
 *   records are dropped, and the output line of a passed block is its input line, copied.
 * rec_out (optional): the record of EVERY block gated, in input order (rec_capacity too small ->
 * THR_ERR_ARG when it overflows).  A failed write() ends the run with THR_ERR_DEVICE.
 */
typedef struct thr_gate_run_opts {
    uint32_t struct_bytes;        /* sizeof(thr_gate_run_opts) -- guards the layout                  */
    int32_t batch_blocks;         /* blocks per batch; 0 = the handle's max_batch (at most ~64 MiB of input) */
    int32_t out_fd;               /* >= 0: the .card lines are written here; -1: verdicts only       */
    int32_t skip;                 /* leading blocks read and dropped (fastcard -k; its default is 1) */
    double timestamp;             /* thr_run_gate_stream only, see above                             */
    thr_record* rec_out;          /* NULL, or room for rec_capacity records                          */
    size_t rec_capacity;
} thr_gate_run_opts;
typedef struct thr_gate_run_stats {
    uint64_t blocks, passed, batches;
    uint64_t bytes_in;            /* input bytes                                                     */
    uint64_t text_bytes;          /* bytes written to out_fd                                         */
    double total_s;               /* the whole call; the calling thread:                             */
    double frame_s, gate_s, wait_s;   /* framing, inside thr_gate*, waiting for a free batch buffer  */
    double format_s, write_s;     /* the library thread: line headers, writev()                      */
} thr_gate_run_stats;
int thr_run_gate_stream(thr_handle* h, const uint8_t* stream, size_t n_bytes, int64_t first_block_idx,
                        const thr_gate_run_opts* opts, thr_gate_run_stats* stats);
int thr_run_gate_card(thr_handle* h, const char* text, size_t text_len, const thr_gate_run_opts* opts,
                      thr_gate_run_stats* stats);

/*
 * Template extraction -- replaces the reference's `thrifty template_extract` (template_extract.py:36-58:
 * iterate Detector(yield_data=True) over a capture, keep the detection with the largest correlation
 * energy among those with |corr offset| <= max_offset, inverse-transform its shifted spectrum, take
 * abs(signal[sample : sample + template_len]), scale by 2 / (mean + std), subtract the mean).  The
 * carrier shift multiplies every sample by a unit-modulus phasor, so abs(ifft(shifted spectrum)) IS the
 * magnitude of the block's input samples: no spectrum leaves the device.  A thr_extract rides on a
 * default single-template detector handle (preshift, fastdet, gate and several-template handles:
 * THR_ERR_ARG).  Every batch goes through the handle's ordinary detect path; behind its kernels, on the
 * same stream and with no host decision in between, one kernel folds the batch's best qualifying
 * record into a running best in device memory and one copies that block's input samples aside if the
 * batch improved the best.
 *   qualifies: THR_FLAG_CORR set and |corr_offset| <= max_offset;
 *   best: the largest corr_energy, compared as the float32 the record holds; among equal energies the
 *     block fed EARLIEST wins (the reference's test is a strict `>`).  The result does not depend on
 *     how the run is cut into batches.
 * The handle must outlive the extraction object, which is destroyed first; same single-threaded rule
 * as the handle.  While no feed is in progress the handle may be used for anything else.
 *
 * thr_extract_feed / _feed_card / _feed_stream: thr_detect / thr_detect_card / thr_detect_stream for
 *   these blocks, plus the fold.  `timestamps` ([n_blocks], or NULL: 0.0) travel with the blocks so
 *   that the winner's can be reported; `out` (NULL allowed) receives the batch's records as usual.
 *   After an error the running best may include part of the failed call's blocks: reset.
 * thr_extract_submit_card / _submit_stream: the same for ONE batch through thr_submit_card /
 *   thr_submit_stream -- the ticket is the handle's, collected with thr_collect as usual (`timestamps`
 *   need only live for the call; a stream batch carries one `timestamp`); `out` must not be NULL.
 * thr_extract_result: waits, runs the extraction kernel over the kept block and copies out: `best` = the
 *   winning record, `timestamp` its timestamp, template_out[0 .. template_len) the template (float64;
 *   `capacity` in doubles, too small -> THR_ERR_ARG), `n_qualifying` the number of records that
 *   qualified.  Any output may be NULL.  Nothing has qualified -> THR_ERR_STATE with a message that says
 *   so (the reference dies with a TypeError there); *n_qualifying is written in that case too.  The
 *   state is left as it is: more blocks may be fed and the result taken again.
 * thr_extract_reset: forget everything fed so far.
 * Arithmetic of the extraction kernel: u8 samples become float32 as (v - 127.4f) / 128 like everywhere
 * else, magnitudes, sums, mean and population standard deviation are float64, summed in a fixed tree.
 */
typedef struct thr_extract thr_extract;
int thr_extract_create(thr_handle* h, double max_offset, thr_extract** out);
void thr_extract_destroy(thr_extract* x);
int thr_extract_reset(thr_extract* x);
int thr_extract_feed(thr_extract* x, const void* samples, int format, const int64_t* block_idx,
                     const double* timestamps, size_t n_blocks, thr_record* out);
int thr_extract_feed_card(thr_extract* x, const char* text, size_t text_len, const int64_t* payload_off,
                          const int64_t* block_idx, const double* timestamps, size_t n_blocks, thr_record* out);
int thr_extract_feed_stream(thr_extract* x, const uint8_t* stream, size_t n_bytes, int64_t first_block_idx,
                            const double* timestamps, thr_record* out, size_t out_capacity, size_t* n_blocks_out);
int thr_extract_submit_card(thr_extract* x, const char* text, size_t text_len, const int64_t* payload_off,
                            const int64_t* block_idx, const double* timestamps, size_t n_blocks, thr_record* out,
                            uint64_t* ticket);
int thr_extract_submit_stream(thr_extract* x, const uint8_t* stream, size_t n_bytes, int64_t first_block_idx,
                              double timestamp, thr_record* out, size_t out_capacity, size_t* n_blocks_out,
                              uint64_t* ticket);
int thr_extract_result(thr_extract* x, thr_record* best, double* timestamp, double* template_out, size_t capacity,
                       uint64_t* n_qualifying);
/*
 * The whole-capture loop of an extraction in ONE call, the twin of thr_run_card / thr_run_stream and
 * built the same way on the entry points above: the calling thread frames batches, keeps up to
 * THR_MAX_IN_FLIGHT of them submitted with the fold and the keep enqueued behind each, and collects
 * them in order.  `x` must belong to `h`; the extraction continues from whatever `x` has been fed
 * (e.g. a raw capture's zero-history lead-in blocks through thr_extract_feed); take the template with
 * thr_extract_result afterwards.  `opts` / `stats` as for thr_run_card, except that neither an output
 * descriptor nor a record array is required: no text is formatted unless opts->out_fd >= 0 (then the
 * .toad lines of the detections are written there, by the calling thread), rec_out receives the
 * detected records if given.  A THR_FLAG_INDEX_ERROR block ends the run with THR_ERR_INDEX like
 * thr_run_card (the reference's loop dies there); batches behind it were already in flight, so the
 * extraction must be reset before it is used again.  An input window around the input is honoured.
 */
int thr_run_extract_card(thr_handle* h, const char* text, size_t text_len, const thr_run_opts* opts,
                         thr_extract* x, thr_run_stats* stats);
int thr_run_extract_stream(thr_handle* h, const uint8_t* stream, size_t n_bytes, int64_t first_block_idx,
                           const thr_run_opts* opts, thr_extract* x, thr_run_stats* stats);

/*
 * Averaged templates -- the cut of EVERY qualifying detection summed on the device, per transmitter class,
 * where thr_extract_result remembers one block.  The single best block carries all of that block's receiver
 * noise; a capture made for extraction holds hundreds of qualifying detections.  The sums ride behind every
 * batch like the fold and the keep (csrc/template_average.hip), whatever the input form.  W = template_len.
 *
 * Armed: thr_extract_average with `opts` arms averaging on `x`, with NULL disarms it.  Allowed only while
 *   nothing has been fed since thr_extract_create or thr_extract_reset (else THR_ERR_STATE).  THR_ERR_ARG with
 *   a sentence: n_classes outside 0 .. THR_AVERAGE_MAX_CLASSES, a bound that is not finite, lo > hi.  While
 *   armed, a feed of THR_IN_C64 samples is THR_ERR_ARG: the sums are exact integers of the u8 quantiser.
 * Qualifies: the extraction's rule, unchanged: THR_FLAG_CORR set and |corr_offset| <= max_offset.
 * Class of a qualifying record: n_classes == 0: class 0.  Otherwise v = double(carrier_bin) + carrier_offset
 *   and the class is the LAST k with lo[k] <= v <= hi[k] (thr_identify's rule: inclusive, last match wins).
 *   No match: the record is counted in n_unclassified and accumulated nowhere.
 * Per sample n = 0 .. W-1 of the cut, (bI, bQ) the bytes of sample corr_sample + n of that block:
 *   q = (5 bI - 637)^2 + (5 bQ - 637)^2       640^2 times the squared magnitude of (b - 127.4) / 128, exact,
 *                                             q < 2^20
 *   e = floor(sqrt(q * 2^40))                 the INTEGER square root (a float square root corrected by
 *                                             integer comparison): exact in any arithmetic
 *   acc_e[k][n] += e, acc_q[k][n] += q        uint64; count[k] += 1 once per record
 *   Integer sums: the result depends on the SET of qualifying records only -- not on the batching, the input
 *   form, the order of lanes, or the order the atomic additions arrive in.
 * Finish, per class with count >= 1 (float64, conversions round to nearest):
 *   m[n] = double(acc_e[k][n]) / (double(count) * 671088640.0)                 671088640 = 2^20 * 640
 *   template = the extraction kernel's arithmetic on m: mean and population standard deviation by the same
 *     fixed tree, scale = 2 / (mean + std), times scale, minus the recomputed mean (one device function)
 *   var[n] = max(double(acc_q[k][n]) / (double(count) * 409600.0) - m[n] * m[n], 0)       not contracted
 *   sem[n] = sqrt(var[n] / double(count)) * scale
 * The single-best result is untouched: thr_extract_result returns the same bytes armed or not.
 *
 * thr_extract_average_counts: waits like thr_extract_result; count[0 .. 16) (classes beyond n_classes: 0; with
 *   n_classes == 0 everything is in count[0]) and *n_unclassified.  Either may be NULL.  Not armed: THR_ERR_STATE.
 * thr_extract_average_result: waits, finishes class `k` and copies out template_out[W], sem_out[W] (float64),
 *   acc_e_out[W], acc_q_out[W] (the sums; `capacity` in elements holds for all four, too small -> THR_ERR_ARG).
 *   Any output may be NULL.  A class with count == 0: THR_ERR_STATE with a sentence, as thr_extract_result
 *   answers when nothing qualified; the sums (zeros) are written in that case too and the counts stay readable.
 *   Not armed: THR_ERR_STATE; `k` outside the armed classes: THR_ERR_ARG.
 * thr_extract_reset zeroes the sums and keeps the arming.  thr_run_extract_card / thr_run_extract_stream
 * enqueue whatever `x` has armed.  Not offered: complex64 input, weights, sub-sample alignment of the cuts
 * (with |offset| <= 0.2 the jitter costs about 6 % of the amplitude at the Nyquist frequency).
 */
#define THR_AVERAGE_MAX_CLASSES 16
typedef struct thr_average_opts {
    int32_t n_classes;                      /* 0: one class, every qualifying record */
    double lo[THR_AVERAGE_MAX_CLASSES];     /* carrier_bin + carrier_offset, inclusive */
    double hi[THR_AVERAGE_MAX_CLASSES];
} thr_average_opts;
int thr_extract_average(thr_extract* x, const thr_average_opts* opts);
int thr_extract_average_counts(thr_extract* x, uint64_t count[THR_AVERAGE_MAX_CLASSES], uint64_t* n_unclassified);
int thr_extract_average_result(thr_extract* x, int k, double* template_out, double* sem_out, size_t capacity,
                               uint64_t* acc_e_out, uint64_t* acc_q_out);

/*
 * Detection dossiers -- the numbers behind the reference's `thrifty analyze_detect` (detect_analysis.py:
 * ForcibleDetector over the blocks of a capture whose index lies in a list of ranges, keep the first
 * `max` that are detected, and for each of them everything its Plotter derives; the plots stay out).
 * A thr_dossier rides on a default single-template detector handle like template extraction's object (preshift, fastdet,
 * gate and several-template handles: THR_ERR_ARG); forcing a verdict is the handle's business (create it
 * with the threshold (0, 0, 0)).  Behind the kernels of every batch, on the same stream and with no host
 * decision in between, one kernel hands the next free slots to the records that qualify and one copies
 * their input samples into the slots:
 *   qualifies: THR_FLAG_CARRIER and THR_FLAG_CORR both set and block_idx inside one of the `n_ranges`
 *     closed ranges ranges[2 i] .. ranges[2 i + 1] (an open end is INT64_MIN / INT64_MAX; at most 16);
 *   slots are taken in feed order, up to `max_keep`, whatever the batching;
 *   n_checked = in-range records seen, n_skipped = those of them that were not detected; counting ends
 *     with the record that fills the last slot (where the reference's loop breaks).
 * thr_dossier_create: THR_ERR_ARG for n_ranges > 16, max_keep < 1, or max_keep blocks of complex64
 *   samples (8 * block_len bytes each, the larger of the two input formats) above 256 MiB.
 * thr_dossier_feed / _feed_card / _feed_stream: their thr_extract_feed* twins plus the pick; they return
 *   when the batch is done, with the counts after it (any of the three outputs may be NULL).  All feeds of
 *   a dossier carry one sample format.  Feeding on after the slots are full changes nothing.
 * thr_dossier_result: for the slots [first, first + count) (clipped to the kept ones; *n_kept = all kept),
 *   every array of `out` that is not NULL is filled, one row per slot:
 *     records, timestamps, positions (blocks fed before it since the reset);
 *     hist[256]       occurrences of each byte value among the block's 2 N bytes (zeros for complex64 input)
 *     fft_mag[N]      |FFT(x)|, natural order
 *     filtered[N - F/2]  sqrt(sum_j w_j^2 m[i + j]^2), j = -F/2 .. F/2, m = fft_mag (0 below bin 0), w the
 *                     unit-energy Dirichlet weights of F + 1 taps, F = 2 * (N / carrier_len)
 *     synced[N][2]    x[n] * exp(2 pi i s (n / N - 1/2)), s = -(carrier_bin + carrier_offset)
 *     synced_fft_mag[N]  magnitude of the shifted spectrum
 *     corr[corr_len][2]  the correlation, corr_len = N - template_len + 1 (thr_dossier_geometry)
 *     scalars         thr_dossier_scalars below
 *   and autocorr[17] = sum_i t[i + l] t[i], l = 0 .. 16, once.  The spectra and the correlation are the
 *   handle's unsectioned stage dumps (thr_debug_stage) of the kept samples; the work runs in chunks of at
 *   most max_batch blocks.  No kept block: THR_OK with *n_kept = 0.
 * Same single-threaded rule and destroy order as thr_extract: the dossier goes before its handle.
 */
typedef struct thr_dossier_scalars {
    double rms_unsynced, rms_synced;     /* sqrt(mean |x|^2) of the input and of `synced`            */
    double fft_std, corr_std;            /* np.std(fft_mag), np.std(|corr|); 0 without a stddev term */
    double synced_fft_std, filtered_std; /* np.std of synced_fft_mag and of filtered, likewise: the
                                            spectrum views put the carrier threshold formula over them */
    double carrier_threshold;            /* carrier_detect._calculate_threshold                      */
    double corr_threshold;               /* soa_estimator.calculate_threshold                        */
    double fit_amplitude, fit_offset;    /* Dirichlet fit on the 7 magnitudes around carrier_bin;
                                            NaN when fit_valid == 0                                  */
    int32_t fit_valid;                   /* 0: carrier_bin < 6 or > N - 7 (the reference wraps inside
                                            its slice there)                                         */
    int32_t peak_start, peak_len;        /* corr[p - 5 : p + 6] clipped to [0, corr_len)             */
    int32_t reserved;
    double corr_shifted[11];             /* |time_shift(corr[peak window], corr_offset)|, peak_len valid */
} thr_dossier_scalars;
typedef struct thr_dossier_out {
    thr_record* records;
    double* timestamps;
    uint64_t* positions;
    uint32_t* hist;
    float* fft_mag;
    float* filtered;
    float* synced;
    float* synced_fft_mag;
    float* corr;
    thr_dossier_scalars* scalars;
    double* autocorr;
} thr_dossier_out;
typedef struct thr_dossier thr_dossier;
int thr_dossier_create(thr_handle* h, const int64_t* ranges, int n_ranges, int64_t max_keep, thr_dossier** out);
void thr_dossier_destroy(thr_dossier* d);
int thr_dossier_reset(thr_dossier* d);
int thr_dossier_feed(thr_dossier* d, const void* samples, int format, const int64_t* block_idx,
                     const double* timestamps, size_t n_blocks, thr_record* out, size_t* n_kept,
                     uint64_t* n_checked, uint64_t* n_skipped);
int thr_dossier_feed_card(thr_dossier* d, const char* text, size_t text_len, const int64_t* payload_off,
                          const int64_t* block_idx, const double* timestamps, size_t n_blocks, thr_record* out,
                          size_t* n_kept, uint64_t* n_checked, uint64_t* n_skipped);
int thr_dossier_feed_stream(thr_dossier* d, const uint8_t* stream, size_t n_bytes, int64_t first_block_idx,
                            const double* timestamps, thr_record* out, size_t out_capacity, size_t* n_blocks_out,
                            size_t* n_kept, uint64_t* n_checked, uint64_t* n_skipped);
int thr_dossier_result(thr_dossier* d, size_t first, size_t count, const thr_dossier_out* out, size_t* n_kept);
/* thr_dossier_geometry: out[0] = F (filter taps - 1), out[1] = rows of `filtered` (N - F/2), out[2] = corr_len,
 *   out[3] = blocks per result-time chunk. */
int thr_dossier_geometry(thr_dossier* d, int64_t out[4]);

/*
 * Capture survey -- the numbers behind the reference's scripts/fft_analysis.py, hist.py and noise_rms.py
 * (the plots stay out): for a raw u8 capture cut into blocks like everything else, per interval of
 * `integrate` consecutive blocks, the mean magnitude spectrum, the histogram of the byte values and, per
 * block, the byte sums the block's energy follows from.  A trailing partial interval is never reported.
 * Everything that leaves the library is an integer, so the results are bit-identical however a run is
 * cut into calls, chunks, tiles or workgroups:
 *   spec_sum[j][k] = sum over the blocks b of interval j of q_b[k],  q = rint(|FFT(x_b)[k]| * 2^S) as
 *     uint32 (float32 magnitude, square root to 1 ulp, exact scaling, round-half-even), S = 30 - log2
 *     (block_len) -- thr_survey_shift; the mean spectrum is spec_sum / (integrate * 2^S), natural bin order;
 *   hist[j][v] = occurrences of byte value v among the 2 * block_len bytes of each block of interval j
 *     (history bytes of overlapping blocks count in both blocks, as in the scripts);
 *   sums[b] = (sum v, sum v^2) over block b's bytes: with c = (double)127.4f the block's energy
 *     sum |x|^2 = (sum v^2 - 2 c sum v + 2 block_len c^2) / 128^2 exactly, noise_rms.py's norm its root.
 * A thr_survey rides on ANY handle (a gate handle builds no template spectra) and is destroyed before it;
 * same single-threaded rule; refused with THR_ERR_STATE while submitted batches are open.  block_len 16384
 * (not THR_PATH_MULTIPASS) runs one fused kernel; other handles the carrier stage's spectrum dump and two
 * small kernels (thr_debug_survey_geometry: fused, blocks per tile, workgroups).
 *
 * thr_survey_feed: n_blocks packed u8 blocks (host memory, any number; chunks of at most max_batch blocks
 *   and of what 64 MiB of accumulator rows take).  The call completes (open + n_blocks) / integrate
 *   intervals, written to spec_sum[cap_intervals][block_len] and hist[cap_intervals][256] from index 0;
 *   fewer rows than that -> THR_ERR_ARG before any device work.  sums: [n_blocks][2] or NULL.  The open
 *   interval's partial sums stay on the device.  Synchronous; copies go through the handle's input
 *   window when one is set.  After an error the open interval may hold part of the failed call: reset.
 * thr_survey_feed_stream: the same for raw-stream framing (thr_detect_stream: block i starts
 *   2 (block_len - history_len) i bytes in; an odd difference -> THR_ERR_ARG); *n_blocks = blocks framed;
 *   sums_capacity (in blocks) below that -> THR_ERR_ARG.
 * thr_survey_pending: blocks fed since the reset, and how many of them wait in the open interval.
 * thr_survey_reset: forget everything fed so far.
 */
typedef struct thr_survey thr_survey;
int thr_survey_create(thr_handle* h, int integrate, thr_survey** out);
void thr_survey_destroy(thr_survey* s);
int thr_survey_reset(thr_survey* s);
int thr_survey_shift(const thr_survey* s, int* shift);
int thr_survey_pending(const thr_survey* s, uint64_t* blocks_fed, uint64_t* blocks_in_open_interval);
int thr_survey_feed(thr_survey* s, const uint8_t* samples, size_t n_blocks, uint64_t* sums, uint64_t* spec_sum,
                    uint64_t* hist, size_t cap_intervals, size_t* n_intervals);
int thr_survey_feed_stream(thr_survey* s, const uint8_t* stream, size_t n_bytes, uint64_t* sums, size_t sums_capacity,
                           size_t* n_blocks, uint64_t* spec_sum, uint64_t* hist, size_t cap_intervals,
                           size_t* n_intervals);
int thr_debug_survey_geometry(const thr_survey* s, int* tile_blocks, int* workgroups, int* fused);

/*
 * Chip-rate scan -- the objective of the reference's scripts/chip_rate_search.py, evaluated for every
 * block of a batch against a bank of Gold-code templates of DIFFERENT lengths.  The reference's template
 * depends on the chip rate through its length L = int(sps * n_chips) alone (template_generate.py: sample i
 * is chip (i * n_chips) // L), so scanning integer lengths is exhaustive.  Per (block, length) the record
 * is what SoaEstimator(template, thresh_coeffs=(0, 0, 0), block_len, history_len = L - 1) returns on the
 * block's carrier-shifted spectrum: first maximum of |corr| over the lags [0, block_len - L], noise with
 * template_energy = L, Gaussian offset clipped to +-0.6 (0 at the first and the last lag), detected =
 * energy > 0.
 *
 * thr_chipscan rides on an ordinary handle (not a gate, preshift or THR_PATH_MULTIPASS one) with block_len
 * 16384 -- every other block length is refused with THR_ERR_ARG: the scan kernels are the 16384-point ones.
 * The handle's own template plays no part; carrier_len, carrier_thresh and carrier_window are the handle's
 * (the carrier stage, the fit and the shift are the detect path's own kernels, and the shifted spectra
 * never leave the device).  samples: n_blocks packed blocks in host memory, any number >= 1 (chunks of at
 * most max_batch blocks inside).  chips: n_chips values 0 / 1 (1 -> +1, 0 -> -1), 1 <= n_chips <= 2047.
 * lengths: n_lengths >= 1 values 1 <= L <= block_len - 2 in any order, repeats allowed; out is
 * [n_blocks][n_lengths] in the order of the list.  A block without a carrier verdict has sample -1, flags 0
 * and zeros in every record.  carrier_out (or NULL): [n_blocks] records with the carrier fields of
 * thr_detect (block_idx = the block's index in the call, template_id 0, the correlation fields cleared).  Bad arguments -> THR_ERR_ARG before any
 * device work; THR_ERR_STATE on a gate handle and while submitted batches are open.  Synchronous.
 * thr_debug_chipscan_geometry: how a call with n_lengths candidates is cut -- candidates per chunk of the
 * template bank (128 KiB each inside a fixed budget), and whether two lengths share one forward transform
 * (0: they do not).  thr_debug_chipscan_budget: the bank budget in bytes (0: the default, 64 MiB; tests
 * shrink it to meet the chunk seam with few candidates).  thr_debug_chipscan_times: device milliseconds
 * of the last call -- [0] carrier stage, fit and shift, [1] bank kernel, [2] scan and finish kernels.
 * thr_debug_chipscan_fill: the workgroups a scan launch aims at (0: the default, twice the CUs); it moves
 * the cut of a chunk's candidates into groups -- one workgroup walks a group -- and no result (tests make
 * the groups long or short with few candidates).  thr_debug_chipscan_groups: the cut a launch of n_blocks
 * blocks (one block chunk) x n_cand candidates (one bank chunk) would use -- groups per block, and candidates
 * per group (the last group may be shorter).  Read-only; either pointer may be NULL.
 */
typedef struct thr_chip_record {   /* out[block][candidate], 24 bytes */
    int32_t sample;    /* CorrDetectionInfo.sample, -1: block had no carrier */
    uint32_t flags;    /* THR_FLAG_CARRIER | THR_FLAG_CORR */
    float energy, noise;
    double offset;
} thr_chip_record;
int thr_chipscan(thr_handle* h, const void* samples, int format, size_t n_blocks,
                 const uint8_t* chips, int n_chips,          /* 0/1 per chip */
                 const int32_t* lengths, size_t n_lengths,   /* any order, repeats allowed */
                 thr_chip_record* out, thr_record* carrier_out /* [n_blocks] or NULL */);
int thr_debug_chipscan_geometry(thr_handle* h, size_t n_lengths, int* candidates_per_chunk, int* paired);
int thr_debug_chipscan_budget(thr_handle* h, size_t bank_bytes);
int thr_debug_chipscan_times(thr_handle* h, double* ms_out /* [3] */);
int thr_debug_chipscan_fill(thr_handle* h, size_t workgroups);
int thr_debug_chipscan_groups(thr_handle* h, size_t n_blocks, size_t n_cand, int* groups, int* per_group);

/* The settings a handle was created with (`templates` is NULL: the array is not retained). */
int thr_get_settings(const thr_handle* h, thr_settings* out);

/*
 * K7: keep only records whose THR_FLAG_CORR is set, preserving order -- what
 * detector_cli's `if detected: print(result.serialize())` does (detect.py:217-219).
 * Device pointers (`d_in` and `d_out` must not overlap); `*n_kept` is written on the host
 * after an internal sync.
 */
int thr_compact_device(thr_handle* h, const thr_record* d_in, size_t n_records,
                       thr_record* d_out, size_t* n_kept);

/*
 * Per-kernel timing with HIP events on the handle's stream (bench.py's
 * roofline leg).  `on` = n > 0 brackets each kernel of every n-th thr_detect*()
 * batch with events (n = 1: all; sampling keeps the ~35 us/batch cost of the event
 * packets out of most steps); 0 disables.  thr_profile_read() syncs and returns accumulated
 * milliseconds and launch counts per kernel slot and resets the accumulators.
 * Slots: 0 = carrier (FFT#1 + peak), 1 = fit, 2 = correlate (FFT#2..peak; long blocks: the
 * fused kernel -- a block's R0 sub-transforms and their combination in one workgroup, one
 * launch per sub-batch), 3 = finish (SoA), 4 = long blocks only: the two-kernel form
 * (sub-transforms, then combination, per chunk of work-list slots) that takes the sub-batches
 * with fewer carrier-positive blocks than workgroups; both forms are launched every time and
 * the one the batch does not belong to returns at once.
 */
#define THR_N_KERNEL_SLOTS 5
int thr_profile_enable(thr_handle* h, int on);
int thr_profile_read(thr_handle* h, double ms[THR_N_KERNEL_SLOTS],
                     int64_t launches[THR_N_KERNEL_SLOTS]);
const char* thr_kernel_name(int slot);

/*
 * Test hooks (tests/ only).  Host pointers, synchronous.
 * thr_debug_fft: forward FFT of n_blocks blocks -> complex64 spectra in natural
 *   order (parity of K1+K2 against np.fft.fft, signal_utils.py:21-25).
 * thr_debug_stage: per-block intermediates of Detector.detect(yield_data=True)
 *   (detect.py:75-78): the frequency-shifted spectrum and the correlation
 *   (first corr_len lags) for template `template_id`; either output may be NULL.
 */
/* thr_debug_correlate_geom: which window-row specialisation of the correlate kernel this handle's
 *   launches take (csrc/correlate16k_geom.hpp): *rows_lo / *rows_hi = rows of 1024 lags compiled out
 *   below / above the unique window, or -1, -1 for the generic kernel (a window outside the table,
 *   a stddev threshold term, another block length or variant).  Decided by the same function the
 *   launcher calls.  (A block_len 16384 handle whose plain launches run sectioned -- thr_debug_sections
 *   -- reports the entry its stage-dump launches of k_correlate take.) */
int thr_debug_correlate_geom(thr_handle* h, int* rows_lo, int* rows_hi);
/*
 * thr_get_path_info: which kernels this handle's plain launches take, and why (no device work).
 * A settings change that looks harmless can cost a sixth of the throughput -- a stddev term in
 * corr_thresh, a history of 1100 instead of 4096 samples -- so the choice is reportable:
 * `Detector.engine_path` and one logging.info line at construction come from here.
 *   n_sections / section_len   the correlate stage's overlap-save sections (0, 0: unsectioned)
 *   rows_lo / rows_hi          window-row specialisation of k_correlate / k_correlate_seg (-1: generic)
 *   why_unsectioned            THR_WHY_*: 0 when sectioned, otherwise the FIRST reason that applies
 *   carrier_kernel, correlate_kernel   kernel family names (as in profiles/ and bench.py)
 *   text                       the same as one sentence
 */
#define THR_WHY_SECTIONED 0   /* the correlate stage runs in sections                                  */
#define THR_WHY_PATH 1        /* the handle was created with an unsectioned / multi-pass kernel path   */
#define THR_WHY_VARIANT 2     /* preshift / fastdet variant: ONE fused kernel per block                */
#define THR_WHY_STDDEV 3      /* corr_thresh has a stddev term: its sums run over every kept lag       */
#define THR_WHY_GEOMETRY 4    /* template / history: the unique window needs more sections than pay
                                 (block_len 16384: more than four of 4096 samples) or than fit         */
#define THR_WHY_BLOCK_LEN 5   /* this block length has no sectioned form (whole blocks sit in LDS, or
                                 the generic multi-pass pipeline)                                      */
typedef struct thr_path_info {
    int32_t n_sections, section_len;
    int32_t rows_lo, rows_hi;
    int32_t why_unsectioned;
    int32_t n_templates;
    char carrier_kernel[48];
    char correlate_kernel[48];
    char text[256];
} thr_path_info;
int thr_get_path_info(thr_handle* h, thr_path_info* out);

/* thr_debug_sections: the overlap-save sections this handle's plain correlate launches run in:
 *   *n_sections (0: unsectioned) of *section_len samples (16384 for long blocks, 4096 for block_len
 *   16384). */
int thr_debug_sections(thr_handle* h, int* n_sections, int* section_len);
/* thr_debug_section_counts: the (block, section) items the one-template 4096-sample section kernel has
 *   searched (*computed) and has left out because their energy bound ruled the peak out (*skipped) since
 *   the last call; waits for the handle's stream, reads the two counters and zeroes them (32 bits each:
 *   read them before 2^32 items).  Both stay 0 for every other correlate kernel. */
int thr_debug_section_counts(thr_handle* h, long long* computed, long long* skipped);
/* thr_debug_window: the input window's state, in bytes from its (page-aligned) start:
 *   out[0] = everything below this offset has been released by the chunk copies (may be unlocked),
 *   out[1], out[2] = the range that is page-locked now, out[3] = the segment size (0: no window). */
int thr_debug_window(thr_handle* h, size_t out[4]);
/* thr_debug_window_times: seconds the window's threads have spent since it was opened -- out[0]
 *   populating page tables (summed over the populator threads), out[1] in hipHostRegister, out[2] in
 *   hipHostUnregister, out[3] the CALLER waiting in front of a copy for its segments to be locked;
 *   out[4] = number of such waits, out[5] = chunk copies that went out as pageable memory instead. */
int thr_debug_window_times(thr_handle* h, double out[6]);
/* thr_debug_pipe_times: seconds the calling thread has spent inside the chunks of the host entry
 *   points since the last call (reads and resets): out[0] growing staging buffers, out[1] the input's
 *   host-to-device copy calls, out[2] block indices / offsets, out[3] kernel launches, out[4] the
 *   records' device-to-host calls; out[5] = chunks; out[6] event record / wait between the copy and
 *   the main stream, out[7] filling the index array (sample chunks); out[8 + k] = the longest single
 *   occurrence of phase k. */
int thr_debug_pipe_times(thr_handle* h, double out[16]);
/* thr_debug_live_resources: what the library holds of the HIP runtime in this process, now: out[0] device
 *   buffers, out[1] pinned host buffers, out[2] streams, out[3] events -- of every handle, extraction and
 *   post-detect result together.  Everything a handle took is given back by its thr_destroy (thr_extract_destroy,
 *   thr_post_free): the four counts are then what they were before it was created.  Needs no device. */
int thr_debug_live_resources(int64_t out[4]);
int thr_debug_fft(thr_handle* h, const void* samples, int format, size_t n_blocks,
                  float* spectra_out /* [n_blocks][block_len][2] */);
int thr_debug_stage(thr_handle* h, const void* samples, int format, size_t n_blocks,
                    int template_id, float* shifted_fft_out /* [n][block_len][2] */,
                    float* corr_out /* [n][block_len][2] */);
/* thr_debug_stage_offsets: the same dump with the sub-bin carrier offsets GIVEN (NULL: the engine's
 *   own fit), as thr_detect_offsets takes them -- what a replaced `soa_estimate.interpolate`
 *   (reference experimental/detect_xcorr_interpol.py:36-62) looks at when `sync.interpolator` has
 *   been replaced too. */
int thr_debug_stage_offsets(thr_handle* h, const void* samples, int format, size_t n_blocks,
                            int template_id, const double* carrier_offset /* [n] or NULL */,
                            float* shifted_fft_out, float* corr_out);

/*
 * identify: merge-side post-processing of detections (thrifty/identify.py:26-181) --
 * transmitter classification from the carrier bin, the duplicate filter, output order.
 * Columns in, columns out (host pointers, synchronous, handle-free; `device_id` picks
 * the GPU that sorts).  `map` / `n_map`: the frequency map of load_freqmap
 * (identify.py:184-215) flattened in its iteration order -- inclusive ranges on
 * carrier_bin + carrier_offset, the LAST matching entry wins, -1 if none
 * (classify_transmitters, identify.py:109-121); n_map == 0 selects the automatic mode
 * (detect_transmitter_windows + np.digitize, identify.py:26-106).
 * Outputs: txid_out[n]; keep_out[n] = the mask of identify_duplicates (identify.py:140-172,
 * including its quirks: the neighbour test ignores rxid/txid and wraps around the sorted
 * ends); kept_order_out[0 .. *n_kept_out) = indices of the kept detections sorted by
 * timestamp, stable (filter_duplicates, identify.py:175-181).
 */
typedef struct thr_freq_range {
    int32_t rxid;
    int32_t txid;
    double lo;
    double hi;
} thr_freq_range;

int thr_identify(int device_id, size_t n, const int32_t* rxid, const int32_t* block,
                 const double* timestamp, const int32_t* carrier_bin, const double* carrier_offset,
                 const double* energy, const thr_freq_range* map, size_t n_map, int32_t* txid_out,
                 uint8_t* keep_out, int64_t* kept_order_out, size_t* n_kept_out);

/*
 * match: detections of one transmission seen by several receivers (thrifty/matchmaker.py:17-79).
 * Columns in, columns out (host pointers, synchronous, handle-free like thr_identify); the detections
 * are in timestamp order.
 *  1. Groups, per txid: in input order the first detection no group holds yet is a LEADER i; its group
 *     is i and every later detection j of that txid with not (timestamp[j] > timestamp[i] + window)
 *     -- float64, equality stays inside; the next leader is the first detection of the txid behind it.
 *  2. One entry per receiver: inside a group, in input order, a receiver's first detection is its
 *     entry; every further detection j of that receiver records the collision (entry so far, j) and
 *     the entry becomes `entry if energy[entry] > energy[j] else j` (equal energies and a NaN on
 *     either side: the later one).
 *  3. Per leader in ascending input index: the group's entries in the order in which their receivers
 *     first appeared in the group (dict order of Python 3.7+).  At least `min_match` entries: a match,
 *     match_idx_out[match_ptr_out[m] .. match_ptr_out[m + 1]); fewer: the LEADER's index alone goes to
 *     miss_out.  collision_out[c] = {entry so far, j}, ordered by (leader, j).
 * match_ptr_out holds n + 1, match_idx_out and miss_out n, collision_out 2 * n values; the counts say
 * how many were written.  n == 0: THR_OK, three zero counts.  The one deviation from the reference:
 * timestamps that decrease somewhere or hold a NaN (the reference's result then depends on the order)
 * are refused with THR_ERR_ARG and a message naming the first such detection.
 */
int thr_match(int device_id, size_t n, const int32_t* rxid, const int32_t* txid,
              const double* timestamp, const double* energy, double window, int min_match,
              int64_t* match_ptr_out, int64_t* match_idx_out, size_t* n_matches_out,
              int64_t* miss_out, size_t* n_misses_out,
              int64_t* collision_out, size_t* n_collisions_out);
/* Milliseconds of the calling thread's last thr_match: {copies in, kernels, copies out} (HIP events). */
int thr_debug_match_times(double* ms_out /* [3] */);

/*
 * tdoa: time differences of arrival of mobile transmissions, the receivers' clocks synchronised
 * through beacon matches (thrifty/tdoa_est.py:43-105 and 234-303, stat_tools.py:8-41).  Host pointers,
 * synchronous, handle-free like thr_match.
 * In: detection columns (rx = DENSE receiver index 0 .. n_rx - 1, timestamp, soa, corr energy and
 * noise); the matches as CSR (match_ptr[n_matches + 1], match_idx), as thr_match returns them;
 * match_beacon[m] = index 0 .. n_beacons - 1 of the beacon that sent match m, -1 for a mobile match;
 * dist[n_rx][n_beacons] = receiver-to-beacon distances; window (s), sample_rate (Hz), deg 1..3.
 *  1. Every beacon match, in match order, appends each of its itertools.combinations(match, 2)
 *     (det0 = the lower receiver) to the list of its receiver pair.  The lists stay in match order
 *     (the reference's sort with a never-negative cmp is a no-op).
 *  2. Every combination of every mobile match is a TASK, in match then combination order: Python's
 *     bisect_left(list, t0 - window) / bisect_right(list, t0 + window) on the list's det0 timestamps
 *     -- the same loops, so an unsorted list gives what Python gives; with more than one pair in the
 *     window the median / MAD mask of stat_tools.is_outlier on soa0 - soa1 (float64, operation for
 *     operation); fewer than deg + 1 pairs kept: a failure; a least-squares polynomial of soa0 on
 *     soa1 + (dist[rx0][b] - dist[rx1][b]) / 2.997e8 * sample_rate, fitted in a centred and scaled
 *     variable; tdoa = (soa0 - fit(soa1)) / sample_rate of the task's own detections;
 *     |tdoa| >= 30e3 / 2.997e8: a failure.
 *  3. row r: row_rx_out[2r..] = {rx0, rx1} (dense), row_det_out[2r..] = {det0, det1},
 *     row_val_out[3r..] = {tdoa [s], snr, model_quality}, in task order.  Group g (a mobile match with
 *     at least one row, in match order): group_id_out[g] = its index in the matches, rows
 *     group_ptr_out[g] .. group_ptr_out[g + 1].  fail_out[2f..] = {det0, det1} in task order.
 *     n_window_out / n_kept_out (either may be null): per task the pairs in the window and the pairs
 *     the mask kept.
 * Sizes: the caller passes n_tasks = the sum of k (k - 1) / 2 over the mobile matches (k = entries of
 * the match); row_rx_out, row_det_out, fail_out hold 2 * n_tasks, row_val_out 3 * n_tasks, n_window_out
 * and n_kept_out n_tasks, group_id_out n_matches and group_ptr_out n_matches + 1 values; the counts say
 * how many were written (n_tasks == 0: THR_OK with three zero counts once the arguments and device_id
 * have been checked; nothing is launched).  Windows of up to 256 pairs are ranked from LDS; longer
 * ones are recomputed from the columns inside the rank count, whose cost grows with the square of the
 * window, so a window of thousands of pairs is correct but slow.  The beacon of a pair is its match's
 * (match_beacon); the reference reads it off the pair's det0, which is the same for matches of one
 * txid, as thr_match makes them.  Deviations from the reference: a receiver pair without a list is an empty
 * window (reference: KeyError); kept abscissae with fewer than deg + 1 distinct values are a failure
 * (reference: LAPACK's minimum-norm solution); a match with two detections of one receiver, an index
 * out of range or an n_tasks that is not the sum above: THR_ERR_ARG before anything is launched.
 */
int thr_tdoa(int device_id, size_t n_det, const int32_t* rx, const double* timestamp, const double* soa,
             const double* energy, const double* noise, size_t n_matches, const int64_t* match_ptr,
             const int64_t* match_idx, const int32_t* match_beacon, int n_rx, int n_beacons,
             const double* dist, double window, double sample_rate, int deg, size_t n_tasks,
             int32_t* row_rx_out, int64_t* row_det_out, double* row_val_out, size_t* n_rows_out,
             int64_t* group_id_out, int64_t* group_ptr_out, size_t* n_groups_out,
             int64_t* fail_out, size_t* n_fail_out, int32_t* n_window_out, int32_t* n_kept_out);
/*
 * thr_tdoa with the reference's other three models (thrifty/tdoa_est.py:108-222).  Everything up to the
 * KEPT LIST of a task -- the lists, the window, the outlier mask -- and everything after its tdoa -- the
 * |tdoa| >= 30e3 / 2.997e8 failure, snr, model_quality, the output orders -- is thr_tdoa's.  The kept list
 * is the window's pairs the mask left, in list order (the models' own sort, with the same never-negative
 * cmp, leaves it alone); n_kept its length; T, S0, S1 its det0 timestamps and SoAs; b_sdoa[i] =
 * (dist[rx0][b_i] - dist[rx1][b_i]) / 2.997e8 * sample_rate; t0, soa0, soa1 the task's own.  `model`:
 *  THR_TDOA_POLY           thr_tdoa's polynomial; thr_tdoa is this call with null picks.
 *  THR_TDOA_WEIGHTED_POLY  n_kept < deg + 1: a failure.  w = sqrt(1 / |S0 - soa0|); w / max(w); sqrt(w);
 *     (w + 2) / 3 -- float64, each operation correctly rounded, so the weights are numpy's bits; the
 *     polynomial of degree deg minimises sum (w_i (S0_i - p(S1_i + b_sdoa_i)))^2 (np.polyfit's w=), fitted
 *     in the same centred and scaled variable with w_i^2 in the moments; tdoa = (soa0 - p(soa1)) /
 *     sample_rate.  Fewer than deg + 1 distinct kept abscissae: a failure, as for thr_tdoa.
 *  THR_TDOA_NEAREST        n_kept < 1: a failure.  idx = bisect_left(T, t0) -- Python's probes over the kept
 *     list, sorted or not; idx - 1 instead if idx > 0 and (idx == n_kept or |t0 - T[idx - 1]| <
 *     |t0 - T[idx]|) (strict: a tie stays on idx); tdoa = ((soa0 - S0[idx]) - (soa1 - S1[idx]) +
 *     b_sdoa[idx]) / sample_rate, in that order of operations: the reference's bits.
 *  THR_TDOA_LINEAR         n_kept < 2: a failure.  high = bisect_left(T, t0), n_kept - 1 if that is n_kept;
 *     low = high - 1, then down while low >= 0 and the pair's beacon (match_beacon) differs from pair
 *     high's; low < 0: a failure.  weight = (soa0 - S0[low]) / (S0[high] - S0[low]); tau = (S1[low] *
 *     (1 - weight) + S1[high] * weight) - soa1; tdoa = (tau + b_sdoa[high]) / sample_rate -- the
 *     reference's signs and operation order, hence its bits.
 * deg is read by the two polynomials only.  pick_out (may be null) holds 2 * n_tasks values: per task, as
 * positions in the kept list, {idx, -1} (nearest), {low, high} (linear; low == -1 where the walk ran out),
 * {-1, -1} for the polynomials and for a task that failed before it picked.  Deviations from the
 * reference: S0[high] == S0[low] is a failure (linear; reference: ZeroDivisionError); a kept pair with
 * S0_i == soa0 is a failure (weighted; the reference's weights turn inf / NaN and it appends a NaN row).
 * A model outside 0..3: THR_ERR_ARG before anything is launched.
 */
#define THR_TDOA_POLY 0
#define THR_TDOA_WEIGHTED_POLY 1
#define THR_TDOA_NEAREST 2
#define THR_TDOA_LINEAR 3
int thr_tdoa_model(int device_id, size_t n_det, const int32_t* rx, const double* timestamp, const double* soa,
                   const double* energy, const double* noise, size_t n_matches, const int64_t* match_ptr,
                   const int64_t* match_idx, const int32_t* match_beacon, int n_rx, int n_beacons,
                   const double* dist, double window, double sample_rate, int deg, size_t n_tasks,
                   int32_t* row_rx_out, int64_t* row_det_out, double* row_val_out, size_t* n_rows_out,
                   int64_t* group_id_out, int64_t* group_ptr_out, size_t* n_groups_out,
                   int64_t* fail_out, size_t* n_fail_out, int32_t* n_window_out, int32_t* n_kept_out,
                   int model, int32_t* pick_out);
/* Milliseconds of the calling thread's last thr_tdoa / thr_tdoa_model: {copies in, kernels, copies out} (HIP events). */
int thr_debug_tdoa_times(double* ms_out /* [3] */);

/* pos -- the reference's `thrifty pos` (thrifty/pos_est.py) on host columns: synchronous, no handle, no
 * state but the device's.  Group g (one mobile transmission) holds rows group_ptr[g] .. group_ptr[g + 1]
 * (group_ptr[0] == 0, non-decreasing); row i is a TDOA row_tdoa[i] [s] between the receivers row_rx0[i]
 * and row_rx1[i] -- DENSE indices into rx_coords[n_rx][dims] (n_rx <= 64, finite) -- with row_snr[i].
 *  dims == 2: p minimises sum (tdoa_i c - (|rx0_i - p| - |rx1_i - p|))^2, c = 2.997e8, inside the box
 *     min(rx) - 10 km .. max(rx) + 10 km per axis, by a Levenberg-Marquardt iteration from x0[2] of at
 *     most max_iter steps (csrc/pos.hip describes it; the reference uses SciPy's TRF).  A group with
 *     fewer than 3 distinct receivers is THR_POS_UNDERDETERMINED.  max_iter == 0 evaluates snr and dop at
 *     x0 without moving.  first_two_rx is not read.
 *  dims == 1: n_rx == 2 and one row per group; p = (rx[a] + rx[b] -+ tdoa c) / 2 with a, b =
 *     first_two_rx[0], [1], minus where rx[a] > rx[b] -- the reference's three float64 operations.  x0 and
 *     max_iter are not read.
 * Per group, in group order: pos_out[g * dims ..], snr_out[g] = the mean of its rows' snr,
 * dop_out[g] = sqrt(trace(inv(G'G))) at the position, G_i = (rx0_i - p) / |rx0_i - p| - (rx1_i - p) /
 * |rx1_i - p| (-1 where G'G's determinant is 0 or not finite), iters_out[g] = trial points evaluated, and
 * status_out[g]: THR_POS_OK; THR_POS_UNDERDETERMINED; THR_POS_UNCONVERGED (max_iter reached, the last
 * iterate is written); THR_POS_AT_BOUND (converged on the box); THR_POS_NONFINITE (a NaN or Inf tdoa, or
 * a point that coincides with a receiver).  Nothing is compacted: the caller drops what it does not want.
 * An index out of range, a decreasing group_ptr, dims other than 1 or 2, n_rx > 64, a non-finite
 * coordinate or x0, a 1-D group that does not hold one row, a bad device_id: THR_ERR_ARG before anything
 * is launched.  n_groups == 0: THR_OK once the arguments and device_id have been checked.
 */
#define THR_POS_OK 0
#define THR_POS_UNDERDETERMINED 1
#define THR_POS_UNCONVERGED 2
#define THR_POS_AT_BOUND 3
#define THR_POS_NONFINITE 4
int thr_pos(int device_id, size_t n_groups, const int64_t* group_ptr, const int32_t* row_rx0,
            const int32_t* row_rx1, const double* row_tdoa, const double* row_snr, int n_rx, int dims,
            const double* rx_coords, const int32_t* first_two_rx, const double* x0, int max_iter,
            double* pos_out, double* dop_out, double* snr_out, int32_t* status_out, int32_t* iters_out);
/* Milliseconds of the calling thread's last thr_pos: {copies in, kernels, copies out} (HIP events). */
int thr_debug_pos_times(double* ms_out /* [3] */);

/* ---- the post-detect chain: identify -> match -> tdoa -> pos in ONE call (kitchen_sink.postdetect).
 * The raw detection columns of all receivers go in once; the four stages run back to back on the device
 * (the kernels of thr_identify, thr_match, thr_tdoa and thr_pos, in their order) and every intermediate
 * stays there: between two stages only the scalar counts that size the next stage's buffers come back,
 * plus thr_match's verdict on the timestamp order (and, in automatic mode, thr_identify's per-receiver
 * histogram of carrier bins, a few thousand counters).  No column returns until thr_post_fetch.
 *
 * Index spaces: txid and keep are per INPUT detection; kept_order maps the toads order (the kept
 * detections by timestamp) to input indices; everything else -- matches, misses, collisions, row_det,
 * failures -- indexes the toads order, as the staged calls do when they are fed the kept detections.
 * row_rx holds indices into rx_ids.  A stage that produces nothing (nothing kept, no match, no mobile
 * detection pair, no row) leaves the later stages at their n == 0 case: nothing is launched for them.
 *
 * Errors (THR_ERR_ARG): a null pointer, rx_ids / beacon_ids not strictly ascending, n_rx outside 1..64,
 * dims other than 1 or 2 (1-D takes two receivers), deg outside 1..3, tdoa_model outside 0..3, a non-finite coordinate or x0, a
 * negative window, n_beacons, min_match or max_iter -- all before the device is queried; timestamps that
 * decrease or hold a NaN after the identify sort (thr_match's sentence); a detection of a match whose
 * receiver rx_ids lacks ("... detection D is of receiver R ...").  */
typedef struct thr_post_settings {
    const thr_freq_range* map;   /* n_map rows in map order; n_map == 0: automatic windows */
    size_t n_map;
    double match_window;
    int32_t min_match;
    int32_t n_rx;
    const int32_t* rx_ids;       /* [n_rx] strictly ascending */
    int32_t dims;
    int32_t n_beacons;
    const double* rx_coords;     /* [n_rx][dims], rows in rx_ids order */
    int32_t first_two_rx[2];     /* 1-D: indices into rx_ids of the receiver table's first two entries */
    const int32_t* beacon_ids;   /* [n_beacons] strictly ascending */
    const double* dist;          /* [n_rx][n_beacons] receiver-to-beacon distances */
    double tdoa_window;
    double sample_rate;
    int32_t deg;
    int32_t max_iter;
    double x0[2];
    int32_t tdoa_as_text;        /* nonzero: the position stage reads every tdoa as (tdoa * 1e9) / 1e9, the value a
                                  * reader of the .tdoa text (nanoseconds) gets -- what `thrifty pos` works on */
    int32_t tdoa_model;          /* THR_TDOA_*; 0 = the polynomial */
} thr_post_settings;
typedef struct thr_post_counts {
    size_t kept, matches, match_entries, misses, collisions, tasks, rows, groups, failures;
} thr_post_counts;
typedef struct thr_post thr_post;
/* what thr_post_fetch copies: element type and count in terms of n (input detections) and thr_post_counts */
#define THR_POST_TXID 0         /* int32[n] */
#define THR_POST_KEEP 1         /* uint8[n] */
#define THR_POST_KEPT_ORDER 2   /* int64[kept] */
#define THR_POST_MATCH_PTR 3    /* int64[matches + 1] */
#define THR_POST_MATCH_IDX 4    /* int64[match_entries] */
#define THR_POST_MISSES 5       /* int64[misses] */
#define THR_POST_COLLISIONS 6   /* int64[collisions][2] */
#define THR_POST_ROW_RX 7       /* int32[rows][2], indices into rx_ids */
#define THR_POST_ROW_DET 8      /* int64[rows][2] */
#define THR_POST_ROW_VAL 9      /* float64[rows][3]: tdoa, snr, model_quality */
#define THR_POST_GROUP_ID 10    /* int64[groups]: the match a group came from */
#define THR_POST_GROUP_PTR 11   /* int64[groups + 1] */
#define THR_POST_GROUP_TS 12    /* float64[groups]: timestamp of the match's first detection */
#define THR_POST_GROUP_TX 13    /* int32[groups]: its txid */
#define THR_POST_FAILURES 14    /* int64[failures][2] */
#define THR_POST_N_WINDOW 15    /* int32[tasks] */
#define THR_POST_N_KEPT 16      /* int32[tasks] */
#define THR_POST_POS 17         /* float64[groups][dims] */
#define THR_POST_DOP 18         /* float64[groups] */
#define THR_POST_SNR 19         /* float64[groups] */
#define THR_POST_STATUS 20      /* int32[groups], THR_POS_* */
#define THR_POST_ITERS 21       /* int32[groups] */
#define THR_POST_N_OUTPUTS 22
int thr_postdetect(int device_id, size_t n, const int32_t* rxid, const int32_t* block, const double* timestamp,
                   const int32_t* carrier_bin, const double* carrier_offset, const double* soa,
                   const double* energy, const double* noise, const thr_post_settings* settings,
                   thr_post** result_out, thr_post_counts* counts_out);
/* Copies output `which` to dst; dst_bytes must be its exact size (THR_ERR_ARG otherwise). */
int thr_post_fetch(thr_post* result, int which, void* dst, size_t dst_bytes);
void thr_post_free(thr_post* result);
/* Milliseconds of the calling thread's last thr_postdetect: {copies in, identify, match, tdoa, pos, copies
 * out} (HIP events); the last slot adds up the thr_post_fetch calls made since. */
int thr_debug_post_times(double* ms_out /* [6] */);

/* ---- detection statistics (the numbers of the reference's `thrifty analyze_toads`, toads_analysis.py).
 * Input: the eleven columns of n detections and an optional selection `sel` (n_sel strictly ascending row
 * indices; NULL: every row).  Timestamps are taken relative to time0, the selection's smallest one (one
 * float64 subtraction).  A CELL is a distinct (rxid, txid) pair of the selection, cells ordered by rxid, then
 * txid (signed); inside a cell the rows keep their input order.  Per cell, nine quantities in this order:
 * carrier_energy, carrier_noise, 20 log10(carrier_energy / carrier_noise), carrier_bin, carrier_offset,
 * energy, noise, 20 log10(energy / noise), offset -- mean, population std (two passes), min, max with IEEE
 * semantics (a NaN makes all four NaN) -- and three integer histograms: detections per minute
 * (floor(timestamp / 60), length = largest minute + 1), carrier bins (from the cell's smallest bin), and
 * numpy.histogram(offset, 10) with its edges.  Per receiver (all selected rows of one rxid): the line
 * timestamp ~ a * soa + b, fitted in u = (soa - mean) / max|soa - mean| on timestamp - mean, the residual
 * a * soa + b - timestamp of every row, the residuals' population std and largest magnitude; a receiver with
 * fewer than two distinct soa gets NaN.  A cell with a non-finite offset gets NaN edges, a zero histogram
 * and THR_TSTATS_FLAG_OFFSET_NONFINITE.
 *
 * Errors (THR_ERR_ARG): a null pointer; an empty selection; a sel index out of range or not strictly
 * ascending; a non-finite timestamp in the selection; timestamps that span more than 2^26 minutes -- all
 * from a host pass before anything is launched; histograms that would together exceed 2^26 counters (known
 * once the cells' extremes are, after the first reduction pass). */
typedef struct thr_tstats_counts {
    size_t rows, cells, receivers, minute_bins, carrier_bins, offset_bins;
    double time0;
} thr_tstats_counts;
typedef struct thr_tstats thr_tstats;
#define THR_TSTATS_FLAG_OFFSET_NONFINITE 1
/* what thr_tstats_fetch copies, in terms of thr_tstats_counts */
#define THR_TSTATS_CELL_RX 0        /* int32[cells] */
#define THR_TSTATS_CELL_TX 1        /* int32[cells] */
#define THR_TSTATS_CELL_PTR 2       /* int64[cells + 1] */
#define THR_TSTATS_ORDER 3          /* int64[rows]: input indices grouped by cell, input order inside a cell */
#define THR_TSTATS_STATS 4          /* float64[cells][9][4]: mean, std, min, max */
#define THR_TSTATS_SNR_DB 5         /* float64[rows][2]: carrier dB, correlation dB, selection order */
#define THR_TSTATS_MINUTE_PTR 6     /* int64[cells + 1] */
#define THR_TSTATS_MINUTE_HIST 7    /* int64[minute_bins] */
#define THR_TSTATS_BIN_FIRST 8      /* int32[cells]: the cell's smallest carrier bin */
#define THR_TSTATS_BIN_PTR 9        /* int64[cells + 1] */
#define THR_TSTATS_BIN_HIST 10      /* int64[carrier_bins] */
#define THR_TSTATS_OFFSET_EDGES 11  /* float64[cells][11] */
#define THR_TSTATS_OFFSET_HIST 12   /* int64[cells][10] */
#define THR_TSTATS_CELL_FLAGS 13    /* int32[cells], THR_TSTATS_FLAG_* */
#define THR_TSTATS_RX_ID 14         /* int32[receivers] */
#define THR_TSTATS_RX_COUNT 15      /* int64[receivers] */
#define THR_TSTATS_RX_FIT 16        /* float64[receivers][4]: a, b, residual std, max |residual| */
#define THR_TSTATS_RESIDUAL 17      /* float64[rows], selection order */
#define THR_TSTATS_N_OUTPUTS 18
int thr_toadstats(int device_id, size_t n, const int32_t* rxid, const int32_t* txid, const int32_t* carrier_bin,
                  const double* timestamp, const double* soa, const double* carrier_offset,
                  const double* carrier_energy, const double* carrier_noise, const double* energy,
                  const double* noise, const double* offset, const int64_t* sel, size_t n_sel,
                  thr_tstats** result_out, thr_tstats_counts* counts_out);
/* Copies output `which` to dst; dst_bytes must be its exact size (THR_ERR_ARG otherwise). */
int thr_tstats_fetch(thr_tstats* result, int which, void* dst, size_t dst_bytes);
void thr_tstats_free(thr_tstats* result);
/* Milliseconds of the calling thread's last thr_toadstats: {copies in, sort and cells, reductions and
 * histograms, fit, copies out} (HIP events); the last slot adds up the thr_tstats_fetch calls made since. */
int thr_debug_toadstats_times(double* ms_out /* [5] */);
/* The tile length T (positions of the sorted order one workgroup reduces per loop trip) and the workgroup size. */
int thr_debug_toadstats_geometry(int* tile_len, int* workgroup);
/* For tests.  The tile kernels of thr_toadstats, thr_beaconsync, thr_tdoastats, thr_reldist and thr_track run on
 * min(tiles, cap) workgroups, each of which walks the tiles w, w + grid, w + 2 grid, ...  `workgroups` sets the cap
 * for the whole process: 0 restores the default (2048), 1 .. 65536 is taken as it is, anything else is THR_ERR_ARG.
 * The cap decides which workgroup reduces which tile and moves no result: every value gives the bytes of the default.
 * A call also resets what thr_debug_seg_tile_stats counts.  Not meant to be changed while another thread is inside
 * one of those five calls (that call may then use either cap for a launch; its results are the same). */
int thr_debug_seg_tile_grid(int workgroups);
/* Since the last thr_debug_seg_tile_grid (or the library's load): *launches = how many times a tile grid was sized
 * (a grid may serve several launches of one call), *max_trips = the largest ceil(tiles / workgroups) among them,
 * i.e. the most trips any workgroup's tile loop took (0 when nothing was launched). */
int thr_debug_seg_tile_stats(int* launches, int* max_trips);

/* ---- clock-sync quality (the numbers of the reference's `thrifty analyze_beacon`, beacon_analysis.py:62-136)
 * for every cell at once.  Input: the detection columns rxid, txid, soa, energy, noise and the detection id
 * idx; the matches as CSR (what thr_match returns); deg in 1..3; an optional closed detection-id range
 * id_range[2] (a row is kept when both of its detections' ids lie inside); optional lists of beacon txids and
 * of receiver ids (NULL: every one that occurs).  A match belongs to the transmitter of its FIRST detection.
 * A CELL is (beacon, rx0 < rx1); its rows are the matches of the beacon that hold both receivers, in match
 * order, as (detection at rx0, detection at rx1); cells are ordered by (beacon, rx0, rx1), signed.
 * Per cell: sdoa = soa1 - soa0, dsdoa = diff(sdoa), mean = sum(dsdoa) / count (one division); row k is a
 * discontinuity when dsdoa[k] > mean * 10 (strict, sign-sensitive, never for a NaN).  With edges = [0, d1, ...,
 * n], cut i is rows [edges[i] + 1, edges[i + 1]); every cell has discontinuities + 1 cuts; a cut with
 * left + 8 >= right is not fitted.  Per fitted cut: the least-squares polynomial of degree deg of soa1 on
 * soa0 as {x_mean, x_scale, y_mean, c0..c3}: soa1 ~ y_mean + sum c_k u^k with u = (soa0 - x_mean) / x_scale
 * (x_scale = max|soa0 - x_mean|; c_k = 0 above deg); the residual soa1 - fit(soa0) of its rows (NaN for rows
 * of no fitted cut); snr = mean(energy^2 / noise^2) over both detections of its rows; disc_soa = soa0 of row
 * `right` when right != n.  Everything of a cut that is not fitted is NaN.  A cut that is long enough but
 * cannot be fitted (all soa0 equal, a NaN) has THR_BSYNC_CUT_DEGENERATE.  Per cell: the population std of all
 * residuals, the largest magnitude, the mean of the fitted cuts' snr; NaN and THR_BSYNC_CELL_NO_FIT without a
 * fitted cut.  A repeated call returns the same bits.
 *
 * Errors (THR_ERR_ARG), all before anything is launched unless noted: a null pointer; deg outside 1..3; a
 * CSR that is not one; a match with two detections of one receiver; an inverted id range; more than 2^28
 * detections, matches or detection pairs, a list of more than 2^20 ids; no match at all, or (known after the
 * first kernel) no row left by the lists and the range. */
typedef struct thr_bsync_counts {
    size_t rows, cells, discontinuities, cuts;
} thr_bsync_counts;
typedef struct thr_bsync thr_bsync;
#define THR_BSYNC_CUT_FITTED 1
#define THR_BSYNC_CUT_DEGENERATE 2
#define THR_BSYNC_CELL_NO_FIT 1
/* what thr_bsync_fetch copies, in terms of thr_bsync_counts */
#define THR_BSYNC_CELL_KEY 0        /* int32[cells][3]: beacon, rx0, rx1 */
#define THR_BSYNC_CELL_PTR 1        /* int64[cells + 1] into the rows */
#define THR_BSYNC_ROW_DET 2         /* int64[rows][2]: detection at rx0, at rx1 (positions in the columns) */
#define THR_BSYNC_ROW_MATCH 3       /* int64[rows]: the match the row came from */
#define THR_BSYNC_SDOA 4            /* float64[rows] */
#define THR_BSYNC_DISC_PTR 5        /* int64[cells + 1] */
#define THR_BSYNC_DISC_IDX 6        /* int64[discontinuities]: row index inside the cell */
#define THR_BSYNC_CUT_PTR 7         /* int64[cells + 1] */
#define THR_BSYNC_CUT_LEFT 8        /* int64[cuts] */
#define THR_BSYNC_CUT_RIGHT 9       /* int64[cuts] */
#define THR_BSYNC_CUT_FLAGS 10      /* int32[cuts]: 0 too short, THR_BSYNC_CUT_* */
#define THR_BSYNC_CUT_FIT 11        /* float64[cuts][7]: x_mean, x_scale, y_mean, c0, c1, c2, c3 */
#define THR_BSYNC_CUT_SNR 12        /* float64[cuts] */
#define THR_BSYNC_CUT_DISC_SOA 13   /* float64[cuts] */
#define THR_BSYNC_RESIDUAL 14       /* float64[rows] */
#define THR_BSYNC_CELL_COUNTS 15    /* int64[cells][3]: rows, discontinuities, fitted cuts */
#define THR_BSYNC_CELL_STATS 16     /* float64[cells][4]: mean dsdoa, residual std, max |residual|, mean snr */
#define THR_BSYNC_CELL_FLAGS 17     /* int32[cells], THR_BSYNC_CELL_* */
#define THR_BSYNC_N_OUTPUTS 18
int thr_beaconsync(int device_id, size_t n_det, const int32_t* rxid, const int32_t* txid, const double* soa,
                   const double* energy, const double* noise, const int64_t* idx, size_t n_matches,
                   const int64_t* match_ptr, const int64_t* match_idx, int deg, const int64_t* id_range /* [2] or NULL */,
                   const int32_t* beacons, size_t n_beacons, const int32_t* receivers, size_t n_receivers,
                   thr_bsync** result_out, thr_bsync_counts* counts_out);
/* Copies output `which` to dst; dst_bytes must be its exact size (THR_ERR_ARG otherwise). */
int thr_bsync_fetch(thr_bsync* result, int which, void* dst, size_t dst_bytes);
void thr_bsync_free(thr_bsync* result);
/* Milliseconds of the calling thread's last thr_beaconsync: {copies in, rows and cells, discontinuities and
 * cuts, fits and summary, copies out} (HIP events); the last slot adds up the fetches made since. */
int thr_debug_beaconsync_times(double* ms_out /* [5] */);
/* The tile length T (positions one workgroup reduces per loop trip) and the workgroup size. */
int thr_debug_beaconsync_geometry(int* tile_len, int* workgroup);

/* ---- TDOA quality (the reference's `thrifty analyze_tdoa`, tdoa_analysis.py) for every cell at once.
 * Input: the columns of a .tdoa matrix; optional closed ranges ts_range[2] on the timestamp and det_range[2]
 * on the detection ids (both ids must lie inside).  A CELL is (rx0, rx1, tx) as stored, cells ordered by that
 * key (signed), rows in input order inside a cell.  Per cell on x = tdoa * 2.997e8: mean, population std (two
 * passes), RMS = sqrt(mean(x^2)), min, max (a NaN makes them NaN).  With `robust`, the same again over the
 * rows that stat_tools.is_outlier(x) keeps (applied to cells of more than one row): median = mean of the two
 * middle values, dev = sqrt((x - median)^2), MAD = median(dev), mask = 0.6745 * dev / MAD > 3.5 in float64,
 * operation for operation (MAD = 0 gives numpy's inf / NaN pattern: a NaN keeps the row).
 * Errors (THR_ERR_ARG): a null pointer, an inverted range, more than 2^28 rows, an empty selection. */
typedef struct thr_tdstats_counts {
    size_t rows, cells, robust;
} thr_tdstats_counts;
typedef struct thr_tdstats thr_tdstats;
#define THR_TDSTATS_CELL_KEY 0      /* int32[cells][3]: rx0, rx1, tx */
#define THR_TDSTATS_CELL_PTR 1      /* int64[cells + 1] */
#define THR_TDSTATS_ORDER 2         /* int64[rows]: input rows grouped by cell, input order inside a cell */
#define THR_TDSTATS_STATS 3         /* float64[cells][5]: mean, std, rms, min, max (metres) */
#define THR_TDSTATS_ROBUST_STATS 4  /* float64[cells][5], empty without `robust` (and so the next three) */
#define THR_TDSTATS_ROBUST_COUNT 5  /* int64[cells]: rows the mask keeps */
#define THR_TDSTATS_MASK 6          /* uint8[rows] in the order of ORDER: 1 = outlier */
#define THR_TDSTATS_MEDIAN 7        /* float64[cells][2]: median, MAD */
#define THR_TDSTATS_N_OUTPUTS 8
int thr_tdoastats(int device_id, size_t n, const int32_t* rx0, const int32_t* rx1, const int32_t* tx,
                  const double* timestamp, const int64_t* det0_idx, const int64_t* det1_idx, const double* tdoa,
                  const double* ts_range /* [2] or NULL */, const int64_t* det_range /* [2] or NULL */, int robust,
                  thr_tdstats** result_out, thr_tdstats_counts* counts_out);
int thr_tdstats_fetch(thr_tdstats* result, int which, void* dst, size_t dst_bytes);
void thr_tdstats_free(thr_tdstats* result);
/* {copies in, selection and cells, statistics, the robust part, copies out} of the thread's last thr_tdoastats */
int thr_debug_tdoastats_times(double* ms_out /* [5] */);
int thr_debug_tdoastats_geometry(int* tile_len, int* workgroup);

/* ---- Relative distance, speed and Doppler (the reference's scripts/reldist_nearest.py) for every cell at once.
 * A CELL is (mobile, beacon, rx0 < rx1), cells ordered by that key (signed).  Its rows are the matches of the
 * mobile that hold both receivers, in match order, as (detection at rx0, detection at rx1); the beacon's rows
 * are the same for the beacon, built once per (beacon, rx0, rx1).  Everything is float64, operation for
 * operation (t: the mobile's row, b: the beacon's rows, nb of them, 0/1: the receiver):
 *   hi      = the first beacon row with b_soa0 >= t_soa0 (np.searchsorted, side='left');
 *   nearest = hi - 1 if hi > 0 and (hi == nb or |t_soa0 - b_soa0[hi-1]| < |t_soa0 - b_soa0[hi]|), else hi;
 *   raw     NEAREST: (t_soa1 - b_soa1[n]) - (t_soa0 - b_soa0[n]);
 *           LINPOL, 1 <= hi <= nb - 1: w = (t_soa0 - b_soa0[hi-1]) / (b_soa0[hi] - b_soa0[hi-1]),
 *           t_soa1 - (b_soa1[hi-1] * (1 - w) + b_soa1[hi] * w); outside the beacon's span the end row is held,
 *           t_soa1 - b_soa1[0] or t_soa1 - b_soa1[nb-1], and the row has THR_RELDIST_ROW_HELD;
 *   x       = (raw + d_beacon + dist_rx) / 2.0 - dist_beacon, with the geometry of the cell's (beacon, rx0, rx1);
 *   mask 1  stat_tools.is_outlier(x, thresh) per cell (as thr_tdoastats, but for one-row cells too);
 *   stats   over the rows mask 1 keeps, times s2m = 2.997e8 / sample_rate: count, mean, population std (two
 *           passes), min, max, and the number of kept rows inside [mean - std, mean + std];
 *   speed   over the kept rows in order: diff(x) / diff(t_soa1) * s2m * sample_rate (m/s), at the rx1 timestamp
 *           of the later row minus the cell's first rx0 timestamp; mask 2 on the speeds;
 *   doppler ((ft0 - ft1) - (fb0[n] - fb1[n])) / 2.0 * (sample_rate / block_len) * 3e8 / carrier_hz * 3.6 (km/h)
 *           with f = carrier_bin + carrier_offset, at the rx0 timestamp minus the cell's first; mask 3 on it;
 *   smooth  the speeds mask 2 keeps and the dopplers mask 3 keeps, each by a local linear regression (LOWESS
 *           without a robustness iteration): with m points, k = max(2, min(m, int(smooth_frac * m + 1e-10)));
 *           the window of point i starts at the smallest L in [0, m - k] for which NOT (L + k < m and
 *           x[L+k] - x[i] < x[i] - x[L]) -- the k consecutive points nearest in abscissa, the lowest window on
 *           ties; h = the largest |x[j] - x[i]| in it; weights (1 - (|D|/h)^3)^3 (all 1 when h is not
 *           positive); the value is the intercept (Swdd Swy - Swd Swdy) / det of the weighted line in
 *           D = x[j] - x[i], det = Sw Swdd - Swd Swd, and Swy / Sw where det <= 1e-12 * Sw * Swdd (singular);
 *           m < 2 or smooth_frac == 0: the values as they are.  One wave takes a point: lane l sums the terms
 *           l, l + 64, ... in order, the 64 partial sums are combined by a butterfly.
 * `idx` (the detections' ids) is taken with the other columns, as thr_beaconsync takes it, and not read: rows
 * name detections by their position in the columns.
 * A cell whose beacon rows are not non-decreasing in soa at rx0 (or, while smoothing, whose own rows are not in
 * the timestamp at rx0) has THR_RELDIST_CELL_UNSORTED, one without beacon rows THR_RELDIST_CELL_NO_BEACON: raw
 * is NaN there, and what follows from it.
 * Errors (THR_ERR_ARG): a null pointer, a CSR that is not one, a match with two detections of one receiver, more
 * than 2^28 detections, matches or rows (2^20 list or table entries), a method that is none, smooth_frac
 * outside [0, 1], no row left. */
#define THR_RELDIST_NEAREST 0
#define THR_RELDIST_LINPOL 1
typedef struct thr_reldist_geom { /* one (beacon, rx0, rx1): the three distances in samples */
    int32_t beacon, rx0, rx1, reserved;
    double d_beacon, dist_rx, dist_beacon;
} thr_reldist_geom;
typedef struct thr_reldist_opts {
    int32_t method, reserved;
    double sample_rate, block_len, carrier_hz, thresh, smooth_frac;
    const thr_reldist_geom* geometry; /* NULL or n_geometry rows; a key that is not listed gets zeros */
    size_t n_geometry;
} thr_reldist_opts;
typedef struct thr_reldist_counts {
    size_t rows, cells, speeds, speed_points, dop_points;
} thr_reldist_counts;
typedef struct thr_reldist_result thr_reldist_result; /* the handle: thr_reldist is the call */
#define THR_RELDIST_ROW_HELD 1
#define THR_RELDIST_CELL_UNSORTED 1
#define THR_RELDIST_CELL_NO_BEACON 2
/* what thr_reldist_fetch copies, in terms of thr_reldist_counts */
#define THR_RELDIST_CELL_KEY 0         /* int32[cells][4]: mobile, beacon, rx0, rx1 */
#define THR_RELDIST_CELL_PTR 1         /* int64[cells + 1] into the rows */
#define THR_RELDIST_ROW_DET 2          /* int64[rows][2]: detection at rx0, at rx1 (positions in the columns) */
#define THR_RELDIST_ROW_MATCH 3        /* int64[rows]: the match the row came from */
#define THR_RELDIST_NEAREST_IDX 4      /* int32[rows]: the nearest beacon row of the cell (-1 without one) */
#define THR_RELDIST_HI 5               /* int32[rows] */
#define THR_RELDIST_ROW_FLAGS 6        /* int32[rows], THR_RELDIST_ROW_* */
#define THR_RELDIST_RAW 7              /* float64[rows], samples */
#define THR_RELDIST_X 8                /* float64[rows], samples */
#define THR_RELDIST_MASK1 9            /* uint8[rows]: 1 = outlier */
#define THR_RELDIST_CELL_STATS 10      /* float64[cells][6]: count, mean, std, min, max (metres), rows within one std */
#define THR_RELDIST_CELL_COUNTS 11     /* int64[cells][5]: rows, beacon rows, kept rows, kept speeds, kept dopplers */
#define THR_RELDIST_SPEED_PTR 12       /* int64[cells + 1] into the speeds */
#define THR_RELDIST_SPEED_X 13         /* float64[speeds], seconds */
#define THR_RELDIST_SPEED 14           /* float64[speeds], m/s */
#define THR_RELDIST_MASK2 15           /* uint8[speeds] */
#define THR_RELDIST_SPEED_SMOOTH_PTR 16 /* int64[cells + 1] into the speed points (the speeds mask 2 keeps) */
#define THR_RELDIST_SPEED_SMOOTH_X 17  /* float64[speed_points] */
#define THR_RELDIST_SPEED_SMOOTH 18    /* float64[speed_points], m/s */
#define THR_RELDIST_DOP 19             /* float64[rows], km/h */
#define THR_RELDIST_MASK3 20           /* uint8[rows] */
#define THR_RELDIST_DOP_SMOOTH_PTR 21  /* int64[cells + 1] into the doppler points (the rows mask 3 keeps) */
#define THR_RELDIST_DOP_SMOOTH_X 22    /* float64[dop_points], seconds */
#define THR_RELDIST_DOP_SMOOTH 23      /* float64[dop_points], km/h */
#define THR_RELDIST_MEDIANS 24         /* float64[cells][6]: median and MAD of x, of the speeds, of the dopplers */
#define THR_RELDIST_CELL_FLAGS 25      /* int32[cells], THR_RELDIST_CELL_* */
#define THR_RELDIST_N_OUTPUTS 26
int thr_reldist(int device_id, size_t n_det, const int32_t* rxid, const int32_t* txid, const double* soa,
                const double* timestamp, const double* carrier_bin, const double* carrier_offset, const int64_t* idx,
                size_t n_matches, const int64_t* match_ptr, const int64_t* match_idx, const int32_t* beacons,
                size_t n_beacons, const int32_t* mobiles /* NULL: every txid that is no beacon */, size_t n_mobiles,
                const int32_t* receivers /* NULL: all */, size_t n_receivers, const thr_reldist_opts* opts,
                thr_reldist_result** result_out, thr_reldist_counts* counts_out);
/* `which` is a THR_RELDIST_* index; dst_bytes must be the size given there */
int thr_reldist_fetch(thr_reldist_result* result, int which, void* dst, size_t dst_bytes);
void thr_reldist_free(thr_reldist_result* result);
/* Milliseconds of the calling thread's last thr_reldist: {copies in, rows and cells, distances masks and
 * statistics, the two smoothers, copies out (summed over the fetches)} */
int thr_debug_reldist_times(double* ms_out /* [5] */);
/* tile length of the reductions, workgroup size, lanes that share one smoothed point */
int thr_debug_reldist_geometry(int* tile_len, int* workgroup, int* point_lanes);

/* ---- Position quality: thr_pos's 2-D solve with optional row weights, every row's residual, inv(A), and the
 * exclusion of one receiver whose arrivals contradict the rest.  Host columns in, synchronous, the results stay
 * on the device behind a handle until thr_posq_fetch (the pattern of thr_reldist).  The columns are thr_pos's;
 * dims must be 2 (THR_ERR_ARG otherwise).  row_weight: NULL, or one finite weight >= 0 per row.
 *   A TASK is a group solved over a subset of its rows from opts->x0 inside thr_pos's box, by thr_pos's own
 *   iteration (csrc/pos_lm.hpp).  Row i of a task counts w_i * (m_used / sum of the task's w): the sum in team
 *   order, then ONE division, so a column of ones is the unweighted solve to the bit; a zero sum ends as
 *   THR_POS_NONFINITE.  F = sum w r^2, A = sum w g g'; rms = sqrt(F / m_used) with the last accepted F;
 *   q = inv(A) = {a11 / det, -a01 / det, a00 / det}, NaN (and dop = -1) where det is 0 or not finite; dop is
 *   thr_pos's expression on A.
 *   1. every group is solved in full.
 *   2. a group is FLAGGED when gate_m > 0, its full status is neither UNDERDETERMINED nor NONFINITE, it names
 *      at least min_rx distinct receivers and rms_full > gate_m.  gate_m == 0: no exclusion.
 *   3. a flagged group gets one candidate task per receiver it names (ascending dense index): the group
 *      without the rows that name that receiver.
 *   4. a candidate is eligible when its status is THR_POS_OK and it names at least min_rx - 1 receivers; the
 *      best one has the smallest rms (the lowest receiver on ties); its receiver is excluded iff
 *      rms_best <= ratio * rms_full.
 *   5. every row's residual tdoa c - (|rx0 - p| - |rx1 - p|) at the chosen position, and whether the row was used.
 * ratio in (0, 1], min_rx in 5 .. 64, gate_m >= 0 and finite, max_iter >= 0: THR_ERR_ARG otherwise. */
typedef struct thr_posq_opts {
    int32_t max_iter, min_rx;
    double x0[2];
    double gate_m, ratio;
} thr_posq_opts;
typedef struct thr_posq_counts {
    size_t groups, rows, flagged, tasks;
} thr_posq_counts;
typedef struct thr_posq_result thr_posq_result; /* the handle: thr_posq is the call */
#define THR_POSQ_INCONSISTENT 1 /* flagged */
#define THR_POSQ_EXCLUDED 2     /* a receiver was excluded: pos, dop, status, iters, q, rms[1] are the candidate's */
#define THR_POSQ_NO_CANDIDATE 4 /* flagged, but no candidate was eligible or the ratio was not met */
/* what thr_posq_fetch copies, in terms of thr_posq_counts */
#define THR_POSQ_POS 0          /* float64[groups][2]: the chosen position */
#define THR_POSQ_DOP 1          /* float64[groups] */
#define THR_POSQ_STATUS 2       /* int32[groups], THR_POS_* */
#define THR_POSQ_ITERS 3        /* int32[groups] */
#define THR_POSQ_Q 4            /* float64[groups][3]: q00, q01, q11 */
#define THR_POSQ_RMS 5          /* float64[groups][2]: rms_full, rms of the chosen task */
#define THR_POSQ_COUNTS 6       /* int32[groups][3]: receivers and rows of the chosen task, excluded dense index or -1 */
#define THR_POSQ_FLAGS 7        /* int32[groups], THR_POSQ_INCONSISTENT | _EXCLUDED | _NO_CANDIDATE */
#define THR_POSQ_FULL_POS 8     /* float64[groups][2]: the full solve */
#define THR_POSQ_FULL_STATUS 9  /* int32[groups] */
#define THR_POSQ_SNR 10         /* float64[groups]: the mean over all rows, as thr_pos */
#define THR_POSQ_RESIDUAL 11    /* float64[rows], metres, at the chosen position */
#define THR_POSQ_USED 12        /* uint8[rows]: 1 = the row belongs to the chosen task */
#define THR_POSQ_TASK_PTR 13    /* int64[groups + 1] into the candidates */
#define THR_POSQ_TASK_RX 14     /* int32[tasks]: the receiver left out (dense index) */
#define THR_POSQ_TASK_POS 15    /* float64[tasks][2] */
#define THR_POSQ_TASK_RMS 16    /* float64[tasks] */
#define THR_POSQ_TASK_STATUS 17 /* int32[tasks] */
#define THR_POSQ_TASK_NRX 18    /* int32[tasks]: distinct receivers of the candidate's rows */
#define THR_POSQ_TASK_ITERS 19  /* int32[tasks] */
#define THR_POSQ_N_OUTPUTS 20
int thr_posq(int device_id, size_t n_groups, const int64_t* group_ptr, const int32_t* row_rx0, const int32_t* row_rx1,
             const double* row_tdoa, const double* row_snr, const double* row_weight /* NULL: unweighted */, int n_rx,
             int dims, const double* rx_coords, const thr_posq_opts* opts, thr_posq_result** result_out,
             thr_posq_counts* counts_out);
/* `which` is a THR_POSQ_* index; dst_bytes must be the size given there */
int thr_posq_fetch(thr_posq_result* result, int which, void* dst, size_t dst_bytes);
void thr_posq_free(thr_posq_result* result);
/* Milliseconds of the calling thread's last thr_posq: {copies in, full solves, flags and expansion, candidates,
 * choice and residuals, copies out (summed over the fetches)} */
int thr_debug_posq_times(double* ms_out /* [6] */);

/* ---- Tracks: per transmitter a constant-velocity Kalman filter over positions in time order, a gate that leaves
 * out the positions the track contradicts, and a fixed-interval (Rauch-Tung-Striebel) smoother.  Host columns in,
 * synchronous, the results stay on the device behind a handle until thr_track_fetch (the pattern of thr_reldist).
 * 2-D only.  Both recursions run as segmented scans of an associative operator (csrc/track_scan.hpp).
 *   input   one row per position: tx, a finite timestamp (seconds), x, y (metres), the measurement variances rx,
 *           ry of the two axes (m^2; finite and > 0 on valid rows, as x and y are finite there), valid (NULL: all).
 *   order   rows are sorted by (tx, timestamp), rows of equal keys in their input order.  A TRACK is one tx.  It
 *           starts at its first valid row; the rows before it, and every row of a track without a valid row, are
 *           NOT TRACKED: their states and nis are NaN, used is 0.
 *   model   the axes are filtered independently and share one mask.  Per axis s = [p, v]; between consecutive rows
 *           dt = t_k - t_(k-1) >= 0, F = [[1, dt], [0, 1]], Q = q [[dt^3/3, dt^2/2], [dt^2/2, dt]]; a row in the
 *           mask is a measurement z = p + noise of variance r, a row outside it a pure prediction.  The start row
 *           has m = [z, 0], P = diag(r, v0^2).
 *   nis     nu_x^2 / S_x + nu_y^2 / S_y with nu = z - (F m)[0] and S = (F P F' + Q)[0][0] + r from the state of the
 *           row before; 0 at the start row, NaN on rows that are invalid or not tracked.
 *   gate    mask_0 = valid.  Round i filters with mask_(i-1), then mask_i = valid & (start | nis_i <= gate) over
 *           ALL rows, so a rejected row can come back.  The rounds end when the mask no longer changes (converged);
 *           otherwise, after max_rounds rounds, one more filter runs with the last mask.  rounds = the filter runs;
 *           nis and used are the last one's.  gate == 0: no gating, one run.  A converged track no longer changes,
 *           so a track's result does not depend on the other tracks of the call.
 *   smooth  RTS over the last filter run: G_k = P_k F' inv(F P_k F' + Q) with the F, Q of row k + 1.
 *   stats   per track {rows, valid rows, used rows, rejected rows (valid, tracked, not used), mean nis of the used
 *           rows, duration (last row's timestamp - start row's), path length (sum of the distances between
 *           consecutive smoothed positions, in row order), mean of the smoothed speed over the tracked rows}; NaN
 *           for the last four of a track without a valid row.  THR_TRACK_LOST: fewer than half of the valid rows
 *           were used (2 * used < valid).
 * An outlier as a track's start row is the known way to lose a track: everything after it contradicts it.  The
 * remedy is the caller's: mark that row invalid.
 * q (m^2/s^3, the spectral density of the acceleration noise) and the scale of rx, ry are the deployment's and
 * have no defaults.  v0 (10 m/s in the Python interface), max_rounds (4), the gate (the 99.9 % point of chi^2
 * with 2 degrees of freedom, 13.815510557964274) and "half" are conventions of the interface, not measurements.
 * Errors (THR_ERR_ARG): a null pointer, more than 2^28 rows, a timestamp that is not finite, on a valid row x, y,
 * rx or ry not finite or a variance <= 0, q < 0, v0 <= 0, gate < 0 (or one of them not finite), max_rounds
 * outside 1 .. 16. */
typedef struct thr_track_opts {
    double q, v0, gate;
    int32_t max_rounds, reserved;
} thr_track_opts;
typedef struct thr_track_counts {
    size_t rows, tracks, used, rejected, rounds, converged;
} thr_track_counts;
typedef struct thr_track_result thr_track_result; /* the handle: thr_track is the call */
#define THR_TRACK_LOST 1
/* what thr_track_fetch copies, in terms of thr_track_counts; the per-row arrays are in input row order */
#define THR_TRACK_ORDER 0       /* int64[rows]: sorted position -> input row */
#define THR_TRACK_TRACK_TX 1    /* int32[tracks], ascending */
#define THR_TRACK_TRACK_PTR 2   /* int64[tracks + 1] into the sorted positions */
#define THR_TRACK_USED 3        /* uint8[rows] */
#define THR_TRACK_NIS 4         /* float64[rows] */
#define THR_TRACK_FILT 5        /* float64[rows][4]: x, vx, y, vy */
#define THR_TRACK_FILT_VAR 6    /* float64[rows][6]: pp, pv, vv of x, then of y */
#define THR_TRACK_SMOOTH 7      /* float64[rows][4] */
#define THR_TRACK_SMOOTH_VAR 8  /* float64[rows][6] */
#define THR_TRACK_TRACK_STATS 9 /* float64[tracks][8], see above */
#define THR_TRACK_TRACK_FLAGS 10 /* int32[tracks], THR_TRACK_LOST */
#define THR_TRACK_N_OUTPUTS 11
int thr_track(int device_id, size_t n, const int32_t* tx, const double* timestamp, const double* x, const double* y,
              const double* rx, const double* ry, const uint8_t* valid /* NULL: all valid */, const thr_track_opts* opts,
              thr_track_result** result_out, thr_track_counts* counts_out);
/* `which` is a THR_TRACK_* index; dst_bytes must be the size given there */
int thr_track_fetch(thr_track_result* result, int which, void* dst, size_t dst_bytes);
void thr_track_free(thr_track_result* result);
/* Milliseconds of the calling thread's last thr_track: {copies in, sort and layout, filter rounds, smoother,
 * statistics, copies out (summed over the fetches)} */
int thr_debug_track_times(double* ms_out /* [6] */);
/* tile length of the scans, workgroup size, doubles of one filter element */
int thr_debug_track_geometry(int* tile_len, int* workgroup, int* element_doubles);

/* ---- Global position solve: grid starts, the best minimum, the ambiguity flag.  Host columns in, synchronous, the
 * results stay on the device behind a handle until thr_posg_fetch (the pattern of thr_posq).  The columns are
 * thr_pos's (CSR groups, dense receiver indices, rx_coords[n_rx][2]); dims must be 2.  All arithmetic is float64,
 * no product and sum is contracted.  G = opts->grid, K = opts->starts.
 *   area     lo = min over the receivers - margin_m, hi = max + margin_m per axis; 0 < margin_m <= 10 km, so the
 *            area lies inside thr_pos's box.  Cell centres cx[i] = lo0 + (i + 0.5) * ((hi0 - lo0) / G), i = 0 .. G-1,
 *            cy[j] alike from lo1, hi1; cell c = j * G + i.
 *   surface  F[c] = sum over the group's rows, in row order, one accumulator from 0.0, of r * r with
 *            r = tc - (|rx0 - p_c| - |rx1 - p_c|), tc = tdoa * 2.997e8, |v| = sqrt(vx * vx + vy * vy): thr_pos's
 *            residual.  Nothing is divided: a centre on a receiver is finite.
 *   minimum  cell c is a LOCAL MINIMUM when for each of its up to 8 neighbours n: F[c] < F[n], or F[c] == F[n] and
 *            n > c; for a neighbour outside the grid: F[c] < +inf.  A NaN makes every comparison false: a NaN cell
 *            is no minimum and keeps its neighbours from being one.  Edge and corner cells can be minima.
 *   starts   the K local minima with the smallest (F, c), in that order; unused slots hold cell -1 and F = NaN.
 *   tasks    K + 1 per group.  Task 0 starts from opts->x0: thr_pos's own solve.  Task k = 1 .. K starts from the
 *            centre of start cell k - 1.  Every task is thr_pos's iteration (csrc/pos_lm.hpp) over all rows with
 *            opts->max_iter, inside thr_pos's box: it returns the bits thr_pos returns on the group with that x0.
 *            A group whose task 0 ends THR_POS_UNDERDETERMINED or THR_POS_NONFINITE gets no grid and no tasks
 *            1 .. K (n_local 0, start cells -1, its map NaN).  A task that does not exist has status
 *            THR_POSG_NO_TASK, iters 0 and NaN elsewhere.
 *   choice   rms_t = sqrt(F_t / rows) with the task's last accepted F.  A task is ELIGIBLE when its status is
 *            THR_POS_OK.  Task u comes BEFORE task t when u is eligible and (rms_u, u) < (rms_t, t).  The BEST is the
 *            eligible task that none comes before.  An eligible task t is a DUPLICATE when some u before it has
 *            sqrt(dx * dx + dy * dy) <= merge_m between their positions.  n_minima = the eligible tasks that are no
 *            duplicates.  The SECOND is the first of those other than the best; pos2, rms2 are NaN without one.
 *   flags    THR_POSG_MOVED: task 0 is not eligible, or the best position is not within merge_m of task 0's.
 *            THR_POSG_AMBIGUOUS: a second exists and rms_second <= fmax(ratio * rms_best, floor_m).
 *            THR_POSG_NO_MINIMUM: no task is eligible; pos, dop, status, rms are then task 0's (task = 0).
 *   map      for the groups map_first .. map_first + map_count - 1 (at most 256): F itself and the local minima.
 * grid 16, 32 or 64; starts 1 .. 8; merge_m > 0, ratio >= 1, floor_m >= 0, all finite; max_iter >= 0; map_first >= 0
 * and map_first + map_count <= n_groups; groups * (starts + 1) <= 2^28: THR_ERR_ARG otherwise, with thr_pos's
 * argument checks, before anything is launched.  grid = 32, starts = 4, merge_m = 1, ratio = 2 and margin_m = the
 * longer side of the receivers' bounding box are conventions of the Python interface, not measurements; floor_m is
 * the deployment's noise level (0: the ratio alone). */
typedef struct thr_posg_opts {
    int32_t max_iter, grid, starts;
    double x0[2];
    double margin_m, merge_m, ratio, floor_m;
    int64_t map_first;
    int32_t map_count;
} thr_posg_opts;
typedef struct thr_posg_counts {
    size_t groups, rows, tasks /* per group: starts + 1 */, starts, grid, map_groups;
} thr_posg_counts;
typedef struct thr_posg_result thr_posg_result; /* the handle: thr_posg is the call */
#define THR_POSG_MOVED 1
#define THR_POSG_AMBIGUOUS 2
#define THR_POSG_NO_MINIMUM 4
#define THR_POSG_NO_TASK (-1) /* the status of a task that does not exist */
#define THR_POSG_ROW_CHUNK 32  /* rows that the surface kernel stages in LDS at a time */
/* what thr_posg_fetch copies, in terms of thr_posg_counts */
#define THR_POSG_POS 0          /* float64[groups][2]: the chosen task's position */
#define THR_POSG_DOP 1          /* float64[groups] */
#define THR_POSG_STATUS 2       /* int32[groups], THR_POS_* */
#define THR_POSG_TASK 3         /* int32[groups]: the chosen task, 0 .. starts */
#define THR_POSG_RMS 4          /* float64[groups] */
#define THR_POSG_POS2 5         /* float64[groups][2]: the second, or NaN */
#define THR_POSG_RMS2 6         /* float64[groups] */
#define THR_POSG_N_MINIMA 7     /* int32[groups] */
#define THR_POSG_FLAGS 8        /* int32[groups], THR_POSG_MOVED | _AMBIGUOUS | _NO_MINIMUM */
#define THR_POSG_SNR 9          /* float64[groups]: the mean over all rows, as thr_pos */
#define THR_POSG_N_LOCAL 10     /* int32[groups]: local-minimum cells of the surface */
#define THR_POSG_START_CELL 11  /* int32[groups][starts] */
#define THR_POSG_START_F 12     /* float64[groups][starts] */
#define THR_POSG_TASK_POS 13    /* float64[groups][tasks][2] */
#define THR_POSG_TASK_DOP 14    /* float64[groups][tasks] */
#define THR_POSG_TASK_RMS 15    /* float64[groups][tasks] */
#define THR_POSG_TASK_STATUS 16 /* int32[groups][tasks], THR_POS_* or THR_POSG_NO_TASK */
#define THR_POSG_TASK_ITERS 17  /* int32[groups][tasks] */
#define THR_POSG_MAP 18         /* float64[map_groups][grid][grid]: F, row j, column i */
#define THR_POSG_MAP_MIN 19     /* uint8[map_groups][grid][grid]: 1 = local minimum */
#define THR_POSG_N_OUTPUTS 20
int thr_posg(int device_id, size_t n_groups, const int64_t* group_ptr, const int32_t* row_rx0, const int32_t* row_rx1,
             const double* row_tdoa, const double* row_snr, int n_rx, int dims, const double* rx_coords,
             const thr_posg_opts* opts, thr_posg_result** result_out, thr_posg_counts* counts_out);
/* `which` is a THR_POSG_* index; dst_bytes must be the size given there */
int thr_posg_fetch(thr_posg_result* result, int which, void* dst, size_t dst_bytes);
void thr_posg_free(thr_posg_result* result);
/* Milliseconds of the calling thread's last thr_posg: {copies in, task 0 (the fixed start), surface minima and
 * starts (one kernel: the surface never leaves LDS), refinement (tasks 1 .. K), choice, copies out (summed over the
 * fetches)} */
int thr_debug_posg_times(double* ms_out /* [6] */);

/* ---- Per-beacon TDOA matrices (the reference's scripts/tdoa_matrix.py:100-141, 144-191) for every cell at once.
 * Host pointers, synchronous, no engine handle; the results stay on the device behind a handle until
 * thr_tdmat_fetch (the pattern of thr_reldist).  The columns are positions into the detection arrays; the matches
 * are CSR (match m is match_idx[match_ptr[m] .. match_ptr[m + 1])), each of ONE transmitter, read off its first
 * detection.
 *   rows    every match whose txid is a listed beacon or a target gives one ROW per pair of its detections at
 *           listed receivers, det0 at the lower receiver (the script's extract_match_matrix: one detection per
 *           receiver per match).  The rows of (tx, rx0, rx1) in match order are that transmitter's LIST at that pair.
 *   tasks   every row of a target t gives one TASK per listed beacon b != t.  The cell key is (rx0, rx1, b, t); the
 *           cells are in ascending key order, the tasks of a cell in row (match) order.  A cell exists when it has a
 *           task.  targets empty: every txid present in a selected match is a target, the beacons included.
 *   flags   THR_TDMAT_CELL_TOO_FEW: the list (b, rx0, rx1) or the list (t, rx0, rx1) has fewer than 3 rows (the
 *           script's constants, whatever the model).  The cell's tasks are not estimated: status THR_TDMAT_SKIPPED,
 *           n_window = n_kept = 0, tdoa NaN.
 *   task    on the list (b, rx0, rx1) exactly thr_tdoa_model's arithmetic (csrc/tdoa_task.hpp): Python's bisect_left /
 *           bisect_right on the list's det0 timestamps at t0 -/+ window, t0 the task's det0 timestamp; the median /
 *           MAD mask on soa0 - soa1 when the window holds more than one pair; the model (THR_TDOA_*, deg 1..3 for the
 *           two polynomials) with beacon_sdoa = (dist[rx0][b] - dist[rx1][b]) / 2.997e8 * sample_rate (dist NULL:
 *           zeros, the script's geometry); |tdoa| >= 30e3 / 2.997e8 is THR_TDMAT_OUT_OF_RANGE, no model
 *           THR_TDMAT_NO_MODEL; both leave tdoa and model_quality NaN.  snr = the mean of the task's two
 *           (energy / noise)**2, model_quality as thr_tdoa_model.
 *   mask    over the tasks of a cell that gave a TDOA, in task order: stat_tools.is_outlier (threshold 3.5) on the
 *           TDOAs in seconds, numpy's float64 operations; a cell of one TDOA keeps it.  A task without a TDOA has
 *           outlier 0.  median and MAD are those of the cell's TDOAs (NaN without one).
 *   stats   over the TDOAs the mask kept, x = tdoa * 2.997e8: mean, population std, rms, min, max (metres); tiled
 *           segmented reductions, slab partials combined in tile order, no atomics: a repeated call returns the same
 *           bits.  A cell without a kept TDOA holds NaN.
 * dist is float64[n_receivers][n_beacons] in the order of the two lists as given (it needs the receiver list).
 * THR_ERR_ARG, before anything is launched: a null argument; a beacon or a receiver listed twice; more than
 * THR_TDMAT_MAX_BEACONS beacons; a model outside THR_TDOA_POLY .. THR_TDOA_LINEAR or a polynomial's deg outside
 * 1..3; a window that is negative or not finite, a sample_rate that is not positive; a malformed CSR or a match with
 * two detections of one receiver (the host pass of thr_reldist); more than 2^28 tasks.  Nothing selected -- no
 * match, no beacon, no pair at listed receivers -- is THR_OK with zero cells (cell_ptr = {0}). */
#define THR_TDMAT_MAX_BEACONS 64
typedef struct thr_tdmat_counts {
    size_t tasks, cells, rows /* of all lists */, tdoas /* tasks with status THR_TDMAT_OK */;
} thr_tdmat_counts;
typedef struct thr_tdmat thr_tdmat; /* the handle: thr_tdoamatrix is the call */
#define THR_TDMAT_CELL_TOO_FEW 1
#define THR_TDMAT_OK 0
#define THR_TDMAT_NO_MODEL 1
#define THR_TDMAT_OUT_OF_RANGE 2
#define THR_TDMAT_SKIPPED 3
/* what thr_tdmat_fetch copies, in terms of thr_tdmat_counts */
#define THR_TDMAT_CELL_KEY 0       /* int32[cells][4]: rx0, rx1, beacon, tx */
#define THR_TDMAT_CELL_PTR 1       /* int64[cells + 1] into the tasks */
#define THR_TDMAT_CELL_FLAGS 2     /* int32[cells], THR_TDMAT_CELL_* */
#define THR_TDMAT_CELL_COUNTS 3    /* int64[cells][5]: beacon rows, target rows, TDOAs, failures, kept */
#define THR_TDMAT_CELL_STATS 4     /* float64[cells][5]: mean, std, rms, min, max of the kept TDOAs (metres) */
#define THR_TDMAT_MEDIANS 5        /* float64[cells][2]: median and MAD of the cell's TDOAs (seconds) */
#define THR_TDMAT_TASK_DET 6       /* int64[tasks][2]: detection at rx0, at rx1 */
#define THR_TDMAT_TASK_MATCH 7     /* int64[tasks]: the match the task's row came from */
#define THR_TDMAT_TIMESTAMP 8      /* float64[tasks]: the timestamp of det0 */
#define THR_TDMAT_TDOA 9           /* float64[tasks], seconds; NaN for a failure or a skipped task */
#define THR_TDMAT_STATUS 10        /* int32[tasks]: THR_TDMAT_OK / _NO_MODEL / _OUT_OF_RANGE / _SKIPPED */
#define THR_TDMAT_SNR 11           /* float64[tasks] */
#define THR_TDMAT_MODEL_QUALITY 12 /* float64[tasks]; NaN without a TDOA */
#define THR_TDMAT_N_WINDOW 13      /* int32[tasks]: beacon rows in the task's window */
#define THR_TDMAT_N_KEPT 14        /* int32[tasks]: those the window's outlier mask kept */
#define THR_TDMAT_OUTLIER 15       /* uint8[tasks]: 1 = the cell mask drops this TDOA */
#define THR_TDMAT_N_OUTPUTS 16
int thr_tdoamatrix(int device_id, size_t n_det, const int32_t* rxid, const int32_t* txid, const double* timestamp,
                   const double* soa, const double* energy, const double* noise, size_t n_matches,
                   const int64_t* match_ptr, const int64_t* match_idx, const int32_t* receivers /* NULL: all */,
                   size_t n_receivers, const int32_t* beacons, size_t n_beacons,
                   const int32_t* targets /* none: every txid present */, size_t n_targets,
                   const double* dist /* NULL: zeros */, double window, double sample_rate, int model, int deg,
                   thr_tdmat** result_out, thr_tdmat_counts* counts_out);
/* `which` is a THR_TDMAT_* index; dst_bytes must be the size given there */
int thr_tdmat_fetch(thr_tdmat* result, int which, void* dst, size_t dst_bytes);
void thr_tdmat_free(thr_tdmat* result);
/* Milliseconds of the calling thread's last thr_tdoamatrix: {copies in, rows and tasks, estimate, mask and
 * statistics, copies out (summed over the fetches)} */
int thr_debug_tdoamatrix_times(double* ms_out /* [5] */);
/* tile length and workgroup size of the segmented stages, tasks (wavefronts) per workgroup of the estimate kernel */
int thr_debug_tdoamatrix_geometry(int* tile_len, int* workgroup, int* tasks_per_workgroup);

/* ---- Coverage map: where can this deployment position a tag, how well, and where does the fixed start lose it.
 * No recording: receiver coordinates rx_coords[n_rx][2] and a timing noise sigma_rx[n_rx] (metres, >= 0) in, per cell
 * of a raster the analytic prediction and the statistics of T simulated transmissions out.  Host pointers,
 * synchronous, the results stay on the device behind a handle until thr_coverage_fetch (the pattern of thr_posg).
 * 2-D only, n_rx <= 64 (thr_pos's limit).  All arithmetic is float64, no product and sum is contracted.
 *   cells    cx[i] = lo0 + (i + 0.5) * ((hi0 - lo0) / nx), i = 0 .. nx - 1; cy[j] alike from lo1, hi1, ny; cell
 *            c = j * nx + i, p_c = (cx[i], cy[j]).
 *   hearing  receiver r HEARS cell c when range_m <= 0 or sqrt(dx * dx + dy * dy) <= range_m, (dx, dy) = rx_r - p_c.
 *            h = the hearing receivers (n_heard; heard_mask bit r).  h < 3: the cell is THR_COV_UNCOVERED, it gets no
 *            trials, its counts are 0 and every float64 output is NaN.  The ROWS of a cell are all pairs (a, b), a < b,
 *            of its hearing receivers, a-major in ascending receiver index: m = h (h - 1) / 2 rows.
 *   analytic at p_c, with e_r = ((rx_r - p) / |rx_r - p|) taken per component as thr_pos takes it (ax / da):
 *            g_row = e_a - e_b; N = sum over the rows in order of g g' (three accumulators from 0.0); dop = thr_pos's
 *            closed form sqrt((N00 + N11) / det N), -1 where det N = N00 * N11 - N01 * N01 is 0 or not finite (the
 *            cell is then THR_COV_DEGENERATE and its predictions are NaN).  thr_pos's estimator is the UNWEIGHTED
 *            least squares over ALL pairs, and the rows' noises n_a - n_b are correlated through the receivers they
 *            share, so its covariance to first order is not sigma^2 inv(N) but
 *                u_r = sum over the rows naming r, in order, of s g_row (s = +1: r is rx0, -1: r is rx1)
 *                M = sum over the hearing r, ascending, of sigma_r^2 u_r u_r'      Cov = inv(N) M inv(N)
 *            with I = (N11, -N01, N00) / det (three divisions), T = I M, Cov = T I, every 2 x 2 product written
 *            a * b + c * d.  pred = (dop, sxx, sxy, syy, rms = sqrt(sxx + syy)).
 *   noise    of (cell c, trial t, receiver r): Philox4x32-10, key (seed_lo, seed_hi), counter (c, t, r, 0),
 *            multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85; output words w0, w1 give
 *            u1 = (w0 + 1) * 2^-32 in (0, 1], u2 = w1 * 2^-32; z = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2),
 *            n_r = sigma_rx[r] * z.  One normal per counter.  Known answers: counter and key 0 ->
 *            6627e8d5 e169c58d bc57ac4c 9b00dbd8; all ones -> 408f276d 41c83b0e a20bc7c6 6d5451fd.
 *   trial    row (a, b) of trial t carries tdoa = ((|rx_a - p| - |rx_b - p|) + (n_a - n_b)) / 2.997e8 and snr 1.0.
 *            Every trial is one group handed to thr_pos's stage (csrc/pos.hip's core, on device pointers) with
 *            opts->x0, opts->max_iter and thr_pos's box: its (pos, status, iters) are the bits thr_pos returns on
 *            that group.  TASK k = covered_index(c) * T + t: cell-major over the covered cells in ascending c.
 *   slabs    the tasks are materialised and solved slab by slab: consecutive tasks, at most slab_groups of
 *            them, the last slab shorter; a slab boundary may fall inside a cell and moves no result.
 *            opts->slab_groups = 0 takes the default, THR_COV_SLAB_BYTES / (bytes of one task's columns with
 *            n_rx (n_rx - 1) / 2 rows); a positive value is a test knob and is capped by that default.
 *   error    of a trial: status THR_POS_NONFINITE or a position that is not finite gives e = +inf; otherwise
 *            dx = x - cx, dy = y - cy, e = sqrt(dx * dx + dy * dy).  A trial is GOOD when its status is THR_POS_OK and
 *            e <= gross_m.
 *   counts   int32[6] per cell: trials ending THR_POS_OK, _AT_BOUND, _UNCONVERGED, _NONFINITE; n_good; n_gross =
 *            T - n_good.  iters_sum is the int64 sum of the trials' iteration counts.
 *   stats    float64[8] per cell: bias_x, bias_y = the means of dx, dy over the good trials; sxx, sxy, syy = the means
 *            of dx * dx, dx * dy, dy * dy; rms = sqrt(sxx + syy); all NaN when n_good == 0.  ONE order: lane l = 0 ..
 *            63 adds its good trials l, l + 64, ... in ascending order to an accumulator that starts at 0.0; then for
 *            d = 32, 16, 8, 4, 2, 1: lane[l] = lane[l] + lane[l + d] for l < d; the sum is lane[0], the mean is
 *            sum / n_good.  No atomics: the same bytes every time and for every slab size.
 *            q50, q95 over ALL T trials with +inf included: sorted[(T + 1) / 2 - 1] and sorted[(95 T + 99) / 100 - 1]
 *            (integer divisions: the nearest-rank ceil(p T) - 1).  q95 = +inf says more than 5 % of the trials have
 *            no position.  One workgroup per cell, e in LDS padded with +inf to a power of two, a bitonic sort.
 *   flags    THR_COV_UNCOVERED; THR_COV_DEGENERATE; THR_COV_LOSSY: n_gross * 2 > T.
 *   keep     for the covered cells among keep_first .. keep_first + keep_count - 1 (keep_count <= 64), their tasks in
 *            order: the CSR columns exactly as the solver saw them (keep_ptr from 0), keep_noise[task][n_rx] (every
 *            receiver, hearing or not), and the trial's pos, status, iters and e.
 * THR_ERR_ARG, each with a sentence, before anything is launched: a null argument; n_rx outside 1 .. 64; a
 * coordinate or sigma that is not finite, sigma < 0; lo, hi not finite or lo >= hi; nx, ny < 1 or nx * ny > 2^20;
 * trials outside 1 .. THR_COV_MAX_TRIALS; cells * trials > 2^28; gross_m not positive and finite; range_m not finite;
 * max_iter < 0; slab_groups < 0; keep_count outside 0 .. 64 or the keep range past the cells; x0 not finite; the
 * area not inside thr_pos's box (10 km beyond the receivers' bounding box, the rule of thr_posg's margin).
 * sigma = 0 for every receiver is allowed: with T = 1 the map is the convergence map of the fixed start.  256 trials,
 * the 95 % point and "half" for LOSSY are conventions, not measurements. */
#define THR_COV_MAX_TRIALS 4096
#define THR_COV_MAX_KEEP 64
#define THR_COV_SLAB_BYTES (512u << 20) /* the byte budget of one slab's columns, noise and solver outputs */
typedef struct thr_coverage_opts {
    double lo[2], hi[2];
    int32_t nx, ny, trials, max_iter;
    double range_m /* <= 0: every receiver hears every cell */, gross_m;
    double x0[2];
    uint32_t seed_lo, seed_hi;
    int64_t slab_groups; /* 0: the default */
    int32_t keep_first, keep_count;
} thr_coverage_opts;
typedef struct thr_coverage_counts {
    size_t cells, nx, ny, n_rx, trials, covered, tasks, rows /* of all tasks */, slabs, slab_groups /* the cap in use */,
        slab_bytes /* the largest slab */, keep_tasks, keep_rows;
} thr_coverage_counts;
typedef struct thr_coverage_result thr_coverage_result; /* the handle: thr_coverage is the call */
#define THR_COV_UNCOVERED 1
#define THR_COV_DEGENERATE 2
#define THR_COV_LOSSY 4
/* what thr_coverage_fetch copies, in terms of thr_coverage_counts */
#define THR_COV_CX 0           /* float64[nx] */
#define THR_COV_CY 1           /* float64[ny] */
#define THR_COV_N_HEARD 2      /* int32[cells] */
#define THR_COV_HEARD_MASK 3   /* uint64[cells] */
#define THR_COV_FLAGS 4        /* int32[cells], THR_COV_UNCOVERED | _DEGENERATE | _LOSSY */
#define THR_COV_PRED 5         /* float64[cells][5]: dop, pred_sxx, pred_sxy, pred_syy, pred_rms */
#define THR_COV_COUNTS 6       /* int32[cells][6]: n_ok, n_at_bound, n_unconverged, n_nonfinite, n_good, n_gross */
#define THR_COV_ITERS_SUM 7    /* int64[cells] */
#define THR_COV_STATS 8        /* float64[cells][8]: bias_x, bias_y, sxx, sxy, syy, rms, q50, q95 */
#define THR_COV_KEEP_PTR 9     /* int64[keep_tasks + 1] */
#define THR_COV_KEEP_RX0 10    /* int32[keep_rows] */
#define THR_COV_KEEP_RX1 11    /* int32[keep_rows] */
#define THR_COV_KEEP_TDOA 12   /* float64[keep_rows] */
#define THR_COV_KEEP_NOISE 13  /* float64[keep_tasks][n_rx], metres */
#define THR_COV_KEEP_POS 14    /* float64[keep_tasks][2] */
#define THR_COV_KEEP_STATUS 15 /* int32[keep_tasks], THR_POS_* */
#define THR_COV_KEEP_ITERS 16  /* int32[keep_tasks] */
#define THR_COV_KEEP_ERR 17    /* float64[keep_tasks] */
#define THR_COV_N_OUTPUTS 18
int thr_coverage(int device_id, int n_rx, const double* rx_coords, const double* sigma_rx, const thr_coverage_opts* opts,
                 thr_coverage_result** result_out, thr_coverage_counts* counts_out);
/* `which` is a THR_COV_* index; dst_bytes must be the size given there */
int thr_coverage_fetch(thr_coverage_result* result, int which, void* dst, size_t dst_bytes);
void thr_coverage_free(thr_coverage_result* result);
/* Milliseconds of the calling thread's last thr_coverage: {copies in, cells (analytic columns and the scans),
 * synthesis (noise and rows, summed over the slabs), solve (summed over the slabs), reduction (the trials' errors,
 * the sums and the sort), copies out (summed over the fetches)} */
int thr_debug_coverage_times(double* ms_out /* [6] */);

/* ---- Positions from receivers with three coordinates: thr_pos's 2-D solve for antennas at different heights.
 * Synchronous, no handle (the pattern of thr_pos).  The columns are thr_pos's (CSR groups, DENSE receiver indices)
 * and the table is rx_xyz[n_rx][3], finite, n_rx <= 64.  One 8-lane team per group runs thr_pos's own iteration
 * (csrc/pos3_lm.hpp restates csrc/pos_lm.hpp's rules for both modes); a row's residual is
 * tdoa c - (|rx0 - p| - |rx1 - p|), c = 2.997e8, |v| = sqrt((vx * vx + vy * vy) + vz * vz).  All arithmetic is
 * float64, no product and sum is contracted.
 *  mode THR_POS3_KNOWN_HEIGHT: the unknowns are (x, y); group_h[n_groups] (finite) gives each transmission's height,
 *     so vz = rz - group_h[g] is a constant of the solve.  Starts from x0[0], x0[1] (x0[2] and z_range are not
 *     read) inside thr_pos's box on x and y.  Fewer than 3 distinct receivers: THR_POS_UNDERDETERMINED.
 *     dop_out = hdop_out = sqrt(trace(inv(G'G))) of the 2 x 2 (the horizontal dilution GIVEN the height),
 *     vdop_out = 0, pos_out[g] = (x, y, group_h[g]).  Where every receiver's z equals group_h[g] the position, dop,
 *     snr, status and iters are the bits thr_pos returns on the table without its z column.
 *  mode THR_POS3_FREE_Z: the unknowns are (x, y, z), from x0[3] inside the box min(rx) - 10 km .. max(rx) + 10 km
 *     per axis, whose z axis is replaced by z_range[2] = {z_lo, z_hi} (finite, z_lo < z_hi) when that is not NULL;
 *     x0[2] must lie inside it.  group_h is not read.  Fewer than 4 distinct receivers: THR_POS_UNDERDETERMINED.
 *     With inv = inv(G'G) (3 x 3, by cofactors): dop_out = sqrt(trace(inv)) (the reference's dop()), hdop_out =
 *     sqrt(inv00 + inv11), vdop_out = sqrt(inv22); all three -1 where the determinant is 0 or not finite.
 *     The cost is even in z about the receivers' plane when all of them share one height: a start ON that plane
 *     has a z gradient of exactly zero and never leaves it (thrifty_amd/pos_3d.py refuses it).
 * Per group, in group order: pos_out[g * 3 ..], rms_out[g] = sqrt(sum r^2 / rows) in metres at the position (NaN for
 * a group without rows), snr_out, status_out (THR_POS_*) and iters_out as thr_pos writes them.  max_iter == 0
 * evaluates at the start.  Nothing is compacted.  THR_ERR_ARG before anything is launched: an index out of range, a
 * decreasing group_ptr, a group over 2^24 rows, more than 2^28 groups or 2^30 rows, n_rx outside 1 .. 64, a
 * non-finite coordinate, height, x0 or z_range, z_lo >= z_hi, x0[2] outside the z range, an unknown mode, a null
 * argument, max_iter < 0, a bad device_id.  n_groups == 0: THR_OK once the arguments and device_id have been checked. */
#define THR_POS3_KNOWN_HEIGHT 0
#define THR_POS3_FREE_Z 1
int thr_pos3(int device_id, size_t n_groups, const int64_t* group_ptr, const int32_t* row_rx0, const int32_t* row_rx1,
             const double* row_tdoa, const double* row_snr, int n_rx, const double* rx_xyz, int mode,
             const double* group_h /* [n_groups], or NULL with z free */, const double* x0 /* [3] */,
             const double* z_range /* [2], or NULL */, int max_iter, double* pos_out /* [n_groups][3] */,
             double* dop_out, double* hdop_out, double* vdop_out, double* rms_out, double* snr_out, int32_t* status_out,
             int32_t* iters_out);
/* Milliseconds of the calling thread's last thr_pos3: {copies in, the kernel, copies out} (HIP events). */
int thr_debug_pos3_times(double* ms_out /* [3] */);

/* ---- Global solve for receivers with three coordinates: thr_posg's grid starts, best minimum and ambiguity flag
 * for thr_pos3's two modes.  Host columns in, synchronous, the results stay on the device behind a handle until
 * thr_posg3_fetch (the pattern of thr_posg).  The columns are thr_pos3's (CSR groups, dense receiver indices,
 * rx_xyz[n_rx][3], n_rx <= 64, mode, group_h).  All arithmetic is float64, no product and sum is contracted.
 * G = opts->grid (16 or 32), Gz = opts->grid_z (1 with the height known, 2 .. 32 with z free), K = opts->starts (1 .. 8).
 *   area     x and y exactly as thr_posg: lo = min over the receivers - margin_m, hi = max + margin_m per axis,
 *            0 < margin_m <= 10 km.  Free z: z_grid[2] = {zg_lo, zg_hi}, both finite, zg_lo < zg_hi, inside the z box
 *            thr_pos3 would use (z_range if given, else min rz - 10 km .. max rz + 10 km).
 *            Centres cx[i] = lo0 + (i + 0.5) * ((hi0 - lo0) / G), cy[j] alike; free z: cz[k] = zg_lo + (k + 0.5) *
 *            ((zg_hi - zg_lo) / Gz); known height: cz = group_h[g], one plane.  Cell c = (k * G + j) * G + i.
 *   surface  F[c] = sum over the group's rows, in row order, one accumulator from 0.0, of r * r with
 *            r = tc - (|rx0 - p_c| - |rx1 - p_c|), tc = tdoa * 2.997e8, v = rx - p_c,
 *            |v| = sqrt((vx * vx + vy * vy) + vz * vz), the additions in this order (csrc/pos3_lm.hpp's).  With every
 *            antenna at group_h[g], vz is 0 and F has thr_posg's bits.
 *   minimum  thr_posg's rule over the up to 26 neighbours n of cell c (8 when Gz = 1): F[c] < F[n], or F[c] == F[n]
 *            and n > c; for a neighbour outside the volume, the planes -1 and Gz included: F[c] < +inf.  A NaN makes
 *            every comparison false.
 *   starts   the K local minima with the smallest (F, c), in that order; unused slots hold cell -1 and F = NaN.
 *   tasks    K + 1 per group.  Task 0 is thr_pos3's own solve from opts->x0[3].  Task k = 1 .. K starts from the centre
 *            of start cell k - 1 (known height: its (cx, cy)).  Every task is thr::pos3lm::solve_team of
 *            csrc/pos3_lm.hpp with thr_pos3's box and opts->max_iter: it returns the bits thr_pos3 returns for that
 *            group with that start -- pos, dop, hdop, vdop, rms = sqrt(F / rows), status and iters.  A group whose
 *            task 0 ends THR_POS_UNDERDETERMINED or THR_POS_NONFINITE gets no grid and no tasks 1 .. K (n_local 0,
 *            start cells -1, its map NaN).  A task that does not exist has status THR_POSG3_NO_TASK, iters 0 and NaN
 *            elsewhere.
 *   choice   thr_posg's pairwise rule word for word: ELIGIBLE means THR_POS_OK; task u comes BEFORE task t when u is
 *            eligible and (rms_u, u) < (rms_t, t); the BEST is the eligible task that none comes before; an eligible
 *            task is a DUPLICATE when some u before it lies within merge_m of it, the distance being
 *            sqrt((dx * dx + dy * dy) + dz * dz) with z free and sqrt(dx * dx + dy * dy) with the height known;
 *            n_minima = the eligible tasks that are no duplicates; the SECOND is the first of those other than the
 *            best; pos2, rms2 are NaN without one.
 *   flags    THR_POSG3_MOVED, _AMBIGUOUS, _NO_MINIMUM as thr_posg defines them (with the distance above).
 *            THR_POSG3_MIRROR, free z only: AMBIGUOUS, and the second lies within merge_m of the best HORIZONTALLY
 *            (sqrt(dx * dx + dy * dy) <= merge_m): x and y can be trusted, the height cannot.  A solve that ends
 *            THR_POS_AT_BOUND is not eligible: a group without an eligible task is NO_MINIMUM and carries task 0's
 *            outputs, thr_pos3's answer.
 *   map      for the groups map_first .. map_first + map_count - 1 (at most 256): F as [Gz][G][G] and the local minima.
 * THR_ERR_ARG before anything is launched: everything thr_pos3 refuses; grid, grid_z or starts out of range;
 * grid_z != 1 with the height known; a missing, non-finite or out-of-box z_grid with z free; merge_m, ratio, floor_m
 * or margin_m as thr_posg refuses them; the map range; groups * (starts + 1) > 2^28.  grid = 32, grid_z = 8, starts = 4,
 * merge_m = 1, ratio = 2, the margin and the default z_grid are conventions of the Python interface, not measurements. */
typedef struct thr_posg3_opts {
    int32_t max_iter, grid, grid_z, starts;
    double x0[3];
    double margin_m, merge_m, ratio, floor_m;
    int64_t map_first;
    int32_t map_count;
} thr_posg3_opts;
typedef struct thr_posg3_counts {
    size_t groups, rows, tasks /* per group: starts + 1 */, starts, grid, grid_z, map_groups;
} thr_posg3_counts;
typedef struct thr_posg3_result thr_posg3_result; /* the handle: thr_posg3 is the call */
#define THR_POSG3_MOVED 1
#define THR_POSG3_AMBIGUOUS 2
#define THR_POSG3_NO_MINIMUM 4
#define THR_POSG3_MIRROR 8
#define THR_POSG3_NO_TASK (-1) /* the status of a task that does not exist */
/* what thr_posg3_fetch copies, in terms of thr_posg3_counts: THR_POSG_*'s indices with positions [3], then the rest */
#define THR_POSG3_POS 0          /* float64[groups][3]: the chosen task's position */
#define THR_POSG3_DOP 1          /* float64[groups] */
#define THR_POSG3_STATUS 2       /* int32[groups], THR_POS_* */
#define THR_POSG3_TASK 3         /* int32[groups]: the chosen task, 0 .. starts */
#define THR_POSG3_RMS 4          /* float64[groups] */
#define THR_POSG3_POS2 5         /* float64[groups][3]: the second, or NaN */
#define THR_POSG3_RMS2 6         /* float64[groups] */
#define THR_POSG3_N_MINIMA 7     /* int32[groups] */
#define THR_POSG3_FLAGS 8        /* int32[groups], THR_POSG3_MOVED | _AMBIGUOUS | _NO_MINIMUM | _MIRROR */
#define THR_POSG3_SNR 9          /* float64[groups]: the mean over all rows, as thr_pos3 */
#define THR_POSG3_N_LOCAL 10     /* int32[groups]: local-minimum cells of the volume */
#define THR_POSG3_START_CELL 11  /* int32[groups][starts] */
#define THR_POSG3_START_F 12     /* float64[groups][starts] */
#define THR_POSG3_TASK_POS 13    /* float64[groups][tasks][3] */
#define THR_POSG3_TASK_DOP 14    /* float64[groups][tasks] */
#define THR_POSG3_TASK_RMS 15    /* float64[groups][tasks] */
#define THR_POSG3_TASK_STATUS 16 /* int32[groups][tasks], THR_POS_* or THR_POSG3_NO_TASK */
#define THR_POSG3_TASK_ITERS 17  /* int32[groups][tasks] */
#define THR_POSG3_MAP 18         /* float64[map_groups][grid_z][grid][grid]: F, plane k, row j, column i */
#define THR_POSG3_MAP_MIN 19     /* uint8[map_groups][grid_z][grid][grid]: 1 = local minimum */
#define THR_POSG3_HDOP 20        /* float64[groups]: the chosen task's, as thr_pos3 */
#define THR_POSG3_VDOP 21        /* float64[groups] */
#define THR_POSG3_TASK_HDOP 22   /* float64[groups][tasks] */
#define THR_POSG3_TASK_VDOP 23   /* float64[groups][tasks] */
#define THR_POSG3_N_OUTPUTS 24
int thr_posg3(int device_id, size_t n_groups, const int64_t* group_ptr, const int32_t* row_rx0, const int32_t* row_rx1,
              const double* row_tdoa, const double* row_snr, int n_rx, const double* rx_xyz, int mode /* THR_POS3_* */,
              const double* group_h /* [n_groups], or NULL with z free */, const double* z_range /* [2], or NULL */,
              const double* z_grid /* [2] with z free; not read with the height known */, const thr_posg3_opts* opts,
              thr_posg3_result** result_out, thr_posg3_counts* counts_out);
/* `which` is a THR_POSG3_* index; dst_bytes must be the size given there */
int thr_posg3_fetch(thr_posg3_result* result, int which, void* dst, size_t dst_bytes);
void thr_posg3_free(thr_posg3_result* result);
/* Milliseconds of the calling thread's last thr_posg3: {copies in, task 0 (the fixed start), surface, minima and
 * starts (one kernel: three planes of the volume at a time in LDS), refinement (tasks 1 .. K), choice, copies out
 * (summed over the fetches)} */
int thr_debug_posg3_times(double* ms_out /* [6] */);

/* ---- Position quality for receivers with three coordinates: thr_posq's row weights, residuals, inv(A) and the
 * exclusion of one receiver, for thr_pos3's two modes.  Host columns in, synchronous, the results stay on the device
 * behind a handle until thr_posq3_fetch (the pattern of thr_posq).  The columns, rx_xyz[n_rx][3], mode and group_h
 * are thr_pos3's; the box, the start (opts->x0, opts->z_range when opts->has_z_range != 0) and every refusal are
 * thr_pos3's too.  row_weight: NULL, or one finite weight >= 0 per row.
 *   A TASK is a group solved over a subset of its rows by thr_pos3's own iteration (csrc/pos3_lm.hpp).  Row i of a
 *   task counts w_i * (m_used / sum of the task's w): the sum in team order, then ONE division, so a column of ones is
 *   the unweighted solve to the bit; a zero sum ends as THR_POS_NONFINITE.  F = sum w r^2, A = sum w g g';
 *   rms = sqrt(F / m_used) with the last accepted F (thr_pos3's rms_out for an unweighted full solve).
 *   q = inv(A) as {q00, q01, q11, q02, q12, q22}.  Free z: by the cofactors thr_pos3 takes its dops from, all six NaN
 *   (and the dops -1) where the determinant is 0 or not finite.  Known height: the first three are thr_posq's 2 x 2
 *   inverse {a11 / det, -a01 / det, a00 / det} and the last three 0.0.  dop, hdop, vdop are thr_pos3's.
 *   Stages 1 .. 5 are thr_posq's, word for word: the full solve; FLAGGED when gate_m > 0, the full status is neither
 *   UNDERDETERMINED nor NONFINITE, the group names at least min_rx distinct receivers and rms_full > gate_m; one
 *   candidate per named receiver (ascending dense index): the group without the rows that name it, from the start
 *   again; a candidate is eligible when THR_POS_OK and it names at least min_rx - 1 receivers, the smallest rms wins
 *   (the lowest receiver on ties) and is excluded iff rms_best <= ratio * rms_full; every row's residual
 *   tdoa c - (|rx0 - p| - |rx1 - p|), |v| = sqrt((vx * vx + vy * vy) + vz * vz), at the chosen position.
 *   With every antenna at group_h[g], every output thr_posq has carries thr_posq's bits on the flat table.
 * min_rx: N receivers give N - 1 independent TDOAs, and a candidate (N - 1 receivers) must keep one redundant
 * arrival, N - 2 > unknowns: 5 .. 64 with the height known, 6 .. 64 with z free.  ratio in (0, 1], gate_m >= 0 and
 * finite, max_iter >= 0: THR_ERR_ARG otherwise. */
typedef struct thr_posq3_opts {
    int32_t max_iter, min_rx, has_z_range;
    double x0[3];
    double z_range[2]; /* read when has_z_range != 0 and z is free */
    double gate_m, ratio;
} thr_posq3_opts;
typedef struct thr_posq3_counts {
    size_t groups, rows, flagged, tasks;
} thr_posq3_counts;
typedef struct thr_posq3_result thr_posq3_result; /* the handle: thr_posq3 is the call */
#define THR_POSQ3_INCONSISTENT 1 /* flagged */
#define THR_POSQ3_EXCLUDED 2     /* a receiver was excluded: pos, dops, status, iters, q, rms[1] are the candidate's */
#define THR_POSQ3_NO_CANDIDATE 4 /* flagged, but no candidate was eligible or the ratio was not met */
/* what thr_posq3_fetch copies, in terms of thr_posq3_counts: THR_POSQ_*'s indices with positions [3] and q [6], then
 * the rest */
#define THR_POSQ3_POS 0          /* float64[groups][3]: the chosen position (known height: z = group_h[g]) */
#define THR_POSQ3_DOP 1          /* float64[groups] */
#define THR_POSQ3_STATUS 2       /* int32[groups], THR_POS_* */
#define THR_POSQ3_ITERS 3        /* int32[groups] */
#define THR_POSQ3_Q 4            /* float64[groups][6]: q00, q01, q11, q02, q12, q22 */
#define THR_POSQ3_RMS 5          /* float64[groups][2]: rms_full, rms of the chosen task */
#define THR_POSQ3_COUNTS 6       /* int32[groups][3]: receivers and rows of the chosen task, excluded dense index or -1 */
#define THR_POSQ3_FLAGS 7        /* int32[groups], THR_POSQ3_INCONSISTENT | _EXCLUDED | _NO_CANDIDATE */
#define THR_POSQ3_FULL_POS 8     /* float64[groups][3]: the full solve */
#define THR_POSQ3_FULL_STATUS 9  /* int32[groups] */
#define THR_POSQ3_SNR 10         /* float64[groups]: the mean over all rows, as thr_pos3 */
#define THR_POSQ3_RESIDUAL 11    /* float64[rows], metres, at the chosen position */
#define THR_POSQ3_USED 12        /* uint8[rows]: 1 = the row belongs to the chosen task */
#define THR_POSQ3_TASK_PTR 13    /* int64[groups + 1] into the candidates */
#define THR_POSQ3_TASK_RX 14     /* int32[tasks]: the receiver left out (dense index) */
#define THR_POSQ3_TASK_POS 15    /* float64[tasks][3] */
#define THR_POSQ3_TASK_RMS 16    /* float64[tasks] */
#define THR_POSQ3_TASK_STATUS 17 /* int32[tasks] */
#define THR_POSQ3_TASK_NRX 18    /* int32[tasks]: distinct receivers of the candidate's rows */
#define THR_POSQ3_TASK_ITERS 19  /* int32[tasks] */
#define THR_POSQ3_HDOP 20        /* float64[groups]: the chosen task's, as thr_pos3 */
#define THR_POSQ3_VDOP 21        /* float64[groups] */
#define THR_POSQ3_N_OUTPUTS 22
int thr_posq3(int device_id, size_t n_groups, const int64_t* group_ptr, const int32_t* row_rx0, const int32_t* row_rx1,
              const double* row_tdoa, const double* row_snr, const double* row_weight /* NULL: unweighted */, int n_rx,
              const double* rx_xyz, int mode /* THR_POS3_* */, const double* group_h /* [n_groups], or NULL with z free */,
              const thr_posq3_opts* opts, thr_posq3_result** result_out, thr_posq3_counts* counts_out);
/* `which` is a THR_POSQ3_* index; dst_bytes must be the size given there */
int thr_posq3_fetch(thr_posq3_result* result, int which, void* dst, size_t dst_bytes);
void thr_posq3_free(thr_posq3_result* result);
/* Milliseconds of the calling thread's last thr_posq3: {copies in, full solves, flags and expansion, candidates,
 * choice and residuals, copies out (summed over the fetches)} */
int thr_debug_posq3_times(double* ms_out /* [6] */);

#ifdef __cplusplus
}
#endif
#endif /* THRIFTY_HIP_H */
