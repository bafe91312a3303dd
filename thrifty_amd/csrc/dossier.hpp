// Detection dossiers (the numbers of the reference's detect_analysis.py on the device): declarations of
// dossier.hip.  The detect pipeline runs unchanged; two small kernels ride behind every batch:
//   k_pick              records that qualify (carrier and correlation detected, block index in one of the
//                       ranges) take the next free slots, in feed order; counts what the reference's loop
//                       would have printed as checked / skipped
//   k_keep_slots        the input samples of the blocks picked in this batch, copied into their slots
// and at result time, over the kept blocks in chunks of at most max_batch:
//   the handle's unsectioned stage-dump launches (spectrum, shifted spectrum, correlation), device to device
//   k_dossier_series    histogram, |FFT|, the Dirichlet-filtered spectrum, the compensated samples, the
//                       shifted spectrum's magnitude, rms values, standard deviations, the two thresholds
//   k_dossier_peaks     the two-parameter Dirichlet fit around the carrier bin, the sub-sample shifted
//                       correlation peak window
//   k_template_autocorr once per dossier: the template's autocorrelation at lags 0 .. 16
#pragma once
#include "host_internal.hpp"

namespace thr {

constexpr int kDossierMaxRanges = 16;
constexpr int kDossierAutocorrLags = 17;     // lags 0 .. 16
constexpr int kDossierPeakWindow = 11;       // corr[p - 5 : p + 6]
constexpr size_t kDossierMaxKeepBytes = size_t(256) << 20;

struct DossierRanges {
    long long lo[kDossierMaxRanges], hi[kDossierMaxRanges];    // closed; an open end is INT64_MIN / INT64_MAX
    int n;
};

// one kept block: its record, timestamp and position in the run (blocks fed since the reset)
struct DossierSlot {
    thr_record rec;
    double timestamp;
    unsigned long long pos;
};

// the pick state of a dossier, in device memory
struct DossierState {
    unsigned long long n_checked;    // in-range records seen, up to and including the one that filled the last slot
    unsigned long long n_skipped;    // of those, the ones not detected
    unsigned n_kept;                 // slots filled so far
    unsigned batch_first;            // the first slot the LAST pick filled (== n_kept: it filled none)
};

// layout of thr_dossier_scalars (include/thrifty_hip.h), filled by k_dossier_series / k_dossier_peaks
using DossierScalars = thr_dossier_scalars;

hipError_t launch_pick(const thr_record* d_recs, const double* d_ts, double ts_all, int n_blocks,
                       unsigned long long base_pos, const DossierRanges& ranges, unsigned max_keep,
                       DossierState* d_state, DossierSlot* d_slots, hipStream_t stream);
// block i of the batch lies at d_in + i * blk_stride, blk_bytes long (both multiples of 4); slot s of the
// keep buffer at d_keep + s * blk_bytes
hipError_t launch_keep_slots(const DossierState* d_state, const DossierSlot* d_slots, const void* d_in,
                             unsigned long long blk_stride, unsigned blk_bytes, unsigned long long base_pos,
                             int n_blocks, unsigned max_keep, void* d_keep, hipStream_t stream);

struct DossierSeriesArgs {
    const void* keep;               // [nb] kept blocks of the chunk, blk_bytes apart
    int format;                     // THR_IN_*
    int n, corr_len, filter_half;   // block_len, lags kept, F / 2
    const DossierSlot* slots;       // [nb] the chunk's slots
    const float2 *fft, *xhat, *corr;    // [nb][n] stage dumps, natural order
    const double* weights2;         // [F + 1] squared Dirichlet weights
    double car_thresh[3], cor_thresh[3];
    unsigned* hist;                 // [nb][256]
    float* fft_mag;                 // [nb][n]
    float* filtered;                // [nb][n - F / 2]
    float2* synced;                 // [nb][n]
    float* synced_fft_mag;          // [nb][n]
    DossierScalars* scalars;        // [nb]
};
hipError_t launch_dossier_series(const DossierSeriesArgs& a, int nb, hipStream_t stream);
hipError_t launch_dossier_peaks(const DossierSlot* d_slots, const float* d_fft_mag, const float2* d_corr, int n,
                                int corr_len, int carrier_len, DossierScalars* d_scalars, int nb,
                                hipStream_t stream);
hipError_t launch_template_autocorr(const double* d_template, int w, double* d_out, hipStream_t stream);

namespace host {
// pipeline.hip calls this behind the kernels of every chunk, next to extract_after_chunk.  Does nothing
// unless the calling thread is inside a thr_dossier_feed* call on `h`.
int dossier_after_chunk(thr_handle* h, int b, const void* d_in, int format, size_t stride, size_t first,
                        size_t nb);
}  // namespace host
}  // namespace thr

struct thr_dossier {
    thr_handle* h = nullptr;
    thr::DossierRanges ranges{};
    unsigned max_keep = 0;
    int format = -1;                                     // THR_IN_* of the kept samples (-1: nothing fed yet)
    int filter_half = 0;                                 // F / 2
    Dev<thr::DossierState> d_state;
    Dev<thr::DossierSlot> d_slots;                       // [max_keep]
    Dev<unsigned char> d_keep;                           // [max_keep] blocks in `format` (the first feed allocates)
    Dev<double> d_weights2;                              // [F + 1]
    Dev<double> d_template;                              // [template_len]
    Dev<double> d_autocorr;                              // [kDossierAutocorrLags]
    bool autocorr_done = false;
    Pinned<double> h_ts[thr_handle::kPipeDepth];         // [max_batch]: a chunk's timestamps
    Dev<double> d_ts[thr_handle::kPipeDepth];
    // result-time work buffers, one chunk of `chunk` blocks (the first thr_dossier_result allocates)
    int chunk = 0;
    Dev<float2> d_fft, d_xhat, d_corr, d_synced;
    Dev<float> d_fft_mag, d_filtered, d_synced_mag;
    Dev<unsigned> d_hist;
    Dev<thr_dossier_scalars> d_scalars;
    unsigned long long fed = 0;                          // blocks fed since the reset
    // the call in progress (dossier_after_chunk reads them)
    const double* cur_ts = nullptr;
    double cur_ts_all = 0;
};
