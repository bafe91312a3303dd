// The four post-detect stages as cores on device pointers (identify.hip, match.hip, tdoa.hip, pos.hip),
// and what their files shared by copy before: with_temp and the hipError_t -> THR_ERR_DEVICE macro (the
// owning DevBuf and Event are hip_own.hpp's).  A core takes device pointers and a stream, owns its
// temporaries, and leaves its outputs in a struct of device buffers that the caller owns, with the counts
// in plain members.  The extern "C" entry points (thr_identify, thr_match, thr_tdoa, thr_pos) are: argument
// checks, copies in, the core, copies out, the time record; thr_postdetect (postdetect.hip) runs the four
// cores back to back.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/thrifty_hip.h"
#include "hip_own.hpp"

namespace thr {

int fail_msg(int code, const char* fmt, ...);
int on_exception(const char* who) noexcept;  // handle.hip

#define THR_HIP_TRY(expr)                                                                    \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return thr::fail_msg(THR_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// a hipCUB device algorithm: size query, grow the shared temporary, run
template <class Call>
hipError_t with_temp(DevBuf& tmp, size_t& tmp_bytes, Call call) {
    size_t need = 0;
    hipError_t e = call(nullptr, need);
    if (e != hipSuccess) return e;
    if (need > tmp_bytes) {
        if ((e = tmp.alloc(need)) != hipSuccess) return e;
        tmp_bytes = need;
    }
    return call(tmp.p, need);
}

// ---------------------------------------------------------------- identify (identify.hip), n >= 1
struct IdentifyOut {
    DevBuf txid;        // int32[n], input order
    DevBuf keep;        // uint8[n], input order
    DevBuf kept_order;  // int64[n], the first n_kept valid: kept detections by timestamp
    int n_kept = 0;
};
// The six columns on the device.  The automatic mode (n_map == 0) takes its receiver list and bin range
// from the HOST copies of rxid and carrier_bin (h_rxid, h_bin: what the caller copied in) and reads the
// per-receiver histogram back, a few thousand counters, to find the window edges on the host.
int identify_core(int n, const int* d_rx, const int* d_blk, const double* d_ts, const int* d_bin,
                  const double* d_off, const double* d_en, const int32_t* h_rxid, const int32_t* h_bin,
                  const thr_freq_range* map, size_t n_map, hipStream_t s, IdentifyOut& out);

// ---------------------------------------------------------------- match (match.hip), n >= 1
constexpr unsigned kMatchSorted = 0xFFFFFFFFu;
struct MatchOut {
    DevBuf ptr;   // int64[n + 1]: n_matches written (the caller adds the terminator, n_entries)
    DevBuf idx;   // int64[n]: n_entries valid
    DevBuf miss;  // int64[n]
    DevBuf coll;  // int64[n][2]
    unsigned first_bad = kMatchSorted;  // the first detection that is NaN or earlier than the one before it
    size_t n_matches = 0, n_entries = 0, n_misses = 0, n_collisions = 0;
};
// THR_OK with first_bad != kMatchSorted: the timestamps are refused and nothing else was written.
int match_core(int n, const int* d_rx, const int* d_tx, const double* d_ts, const double* d_en, double window,
               int min_match, hipStream_t s, MatchOut& out);

// ---------------------------------------------------------------- tdoa (tdoa.hip), n_matches >= 1
struct TdoaOut {
    DevBuf row_rx;     // int32[n_tasks][2] (dense receiver index): n_rows valid
    DevBuf row_det;    // int64[n_tasks][2]
    DevBuf row_val;    // float64[n_tasks][3]: tdoa, snr, model_quality
    DevBuf fail;       // int64[n_tasks][2]: n_fail valid
    DevBuf group_id;   // int64[n_matches]: n_groups valid
    DevBuf group_ptr;  // int64[n_matches + 1]: n_groups written (the caller adds the terminator, n_rows)
    DevBuf n_window;   // int32[n_tasks]
    DevBuf n_kept;     // int32[n_tasks]
    size_t n_tasks = 0, n_pairs = 0, n_rows = 0, n_groups = 0, n_fail = 0;
};
// n_tasks / n_pairs < 0: not known to the caller; they are read off the scans of k_pair_counts.  With no
// task the core returns after those scans (out.n_tasks == 0, nothing else allocated or launched).
// model: THR_TDOA_* (deg is read by the two polynomials only).  picks (may be null): receives int32[n_tasks][2],
// the nearest / linear model's choice per task as positions in the kept list (thr_tdoa_model's pick_out).
int tdoa_core(int n_det, const int* d_rx, const double* d_ts, const double* d_soa, const double* d_en,
              const double* d_no, int n_matches, const long long* d_ptr, const long long* d_idx,
              const int* d_beacon, int n_rx, int n_beacons, const double* d_dist, double window, double sample_rate,
              int deg, int model, long long n_tasks, long long n_pairs, hipStream_t s, TdoaOut& out,
              DevBuf* picks = nullptr);

// ---------------------------------------------------------------- pos (pos.hip), n_groups >= 1
struct PosPlan {  // what the host derives from the receiver table
    double start[2] = {0, 0}, lo[2] = {0, 0}, hi[2] = {0, 0};
    int first = 0, second = 0;
};
// checks n_rx, dims, the coordinates, first_two_rx (1-D) or x0 (2-D); THR_ERR_ARG with `who` in the sentence
int pos_plan(const char* who, int n_rx, int dims, const double* rx_coords, const int32_t* first_two_rx,
             const double* x0, PosPlan& plan);
struct PosOut {
    DevBuf pos;     // float64[n_groups][dims]
    DevBuf dop;     // float64[n_groups]
    DevBuf snr;     // float64[n_groups]
    DevBuf status;  // int32[n_groups]
    DevBuf iters;   // int32[n_groups]
};
int pos_core(int n_groups, const long long* d_ptr, const int* d_rx0, const int* d_rx1, const double* d_tdoa,
             const double* d_snr, const double* d_xy, int dims, const PosPlan& plan, int max_iter, hipStream_t s,
             PosOut& out);

}  // namespace thr
