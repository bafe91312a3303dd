// tdoa on the device (reference thrifty/tdoa_est.py:43-105, 234-303; thrifty/stat_tools.py:8-41): time
// differences of arrival of mobile transmissions, the receivers' clocks tied together by beacon matches.
//   1. every beacon match expands into its k(k-1)/2 detection pairs (det0 = the lower receiver); the pairs
//      go, in match order, into one list per receiver pair (a stable sort by the pair key: histogram,
//      exclusive scan, scatter -- hipCUB's radix sort over the key's bits);
//   2. every mobile match expands the same way into TASKS; one wavefront runs one task: Python's two
//      bisections on the list's det0 timestamps (sorted or not), the median / MAD outlier mask on
//      soa0 - soa1 in the reference's float64 operations, the MODEL over the kept pairs -- a least-squares
//      polynomial of soa0 on soa1 + beacon_sdoa (plain or weighted), the nearest kept pair, or the line
//      through two kept pairs of one beacon (thrifty/tdoa_est.py:89-222) -- and the row;
//   3. rows, failures and the group table are compacted into the reference's orders by prefix sums.
// The fit is not LAPACK's: it runs in u = (x - mean) / max|x - mean| on y - mean(y) (normal equations of
// size deg + 1, partial pivoting, Horner in u), which keeps the digits the raw Vandermonde of abscissae
// near 1e9..1e11 loses.  Everything that decides WHICH pairs are used is the reference's arithmetic.
// The nearest and the linear model bisect the KEPT list (the window's pairs the mask left, in list order):
// kept rank -> window position goes through per-trip ballots and popcounts (kept_at), whatever the window's
// length; their formulas are the reference's operations in its order, so their results are its bits.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/thrifty_hip.h"
#include "post_stages.hpp"
#include "tdoa_task.hpp"

// the outlier mask must equal numpy's bit for bit: no a * b + c may become an fma in this file (the
// build also passes -ffp-contract=off for it, thrifty_amd/build.py: PER_FILE_FLAGS)
#pragma clang fp contract(off)

namespace {

using thr::DevBuf;
using thr::Event;

constexpr int kBlock = 256;               // workgroup size of every kernel here
constexpr int kWave = 64;                 // one task per wavefront
constexpr int kWaves = kBlock / kWave;    // tasks per workgroup of k_estimate (_native.TDOA_TASKS_PER_WORKGROUP)
constexpr int kLdsWindow = 256;           // windows up to this many pairs are staged in LDS (_native.TDOA_LDS_WINDOW)
constexpr int kMaxReceivers = 1024;       // pair key = rx0 * R + rx1 in 20 bits
constexpr double kSpeedOfLight = 2.997e8;           // the reference's constant (tdoa_est.py:25)
// the task itself is tdoa_task.hpp's, written for these
static_assert(kBlock == thr::tdoa_task::kBlock && kWave == thr::tdoa_task::kWave && kLdsWindow == thr::tdoa_task::kLdsWindow &&
                  kSpeedOfLight == thr::tdoa_task::kSpeedOfLight,
              "tdoa.hip and tdoa_task.hpp disagree");

__global__ void k_iota(unsigned* idx, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) idx[i] = unsigned(i);
}
// (energy / noise)**2 of every detection: snr and model_quality are means of these
__global__ void k_quality(const double* __restrict__ energy, const double* __restrict__ noise, int n,
                          double* __restrict__ q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double r = energy[i] / noise[i];
    q[i] = r * r;
}
// pairs of match m: beacon pairs or tasks; slot n_matches holds 0 so that the exclusive sums end in the totals
__global__ void k_pair_counts(const long long* __restrict__ ptr, const int* __restrict__ beacon, int n_matches,
                              unsigned* __restrict__ n_beacon_pairs, unsigned* __restrict__ n_tasks) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m > n_matches) return;
    unsigned pairs = 0;
    bool is_beacon = false;
    if (m < n_matches) {
        const unsigned k = unsigned(ptr[m + 1] - ptr[m]);
        pairs = k * (k - 1u) / 2u;
        if (k == 0) pairs = 0;
        is_beacon = beacon[m] >= 0;
    }
    n_beacon_pairs[m] = is_beacon ? pairs : 0u;
    n_tasks[m] = is_beacon ? 0u : pairs;
}
// itertools.combinations(match, 2) in its order, det0 = the detection of the lower receiver
__global__ void k_expand(const long long* __restrict__ ptr, const long long* __restrict__ idx,
                         const int* __restrict__ beacon, const int* __restrict__ rx, int n_matches, int n_rx,
                         const unsigned* __restrict__ beacon_base, const unsigned* __restrict__ task_base,
                         unsigned* __restrict__ pair_key, int* __restrict__ pair_det0, int* __restrict__ pair_det1,
                         int* __restrict__ pair_beacon, int* __restrict__ task_det0, int* __restrict__ task_det1) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_matches) return;
    const long long first = ptr[m];
    const int k = int(ptr[m + 1] - first), b = beacon[m];
    size_t slot = b >= 0 ? beacon_base[m] : task_base[m];
    for (int i = 0; i < k; ++i)
        for (int j = i + 1; j < k; ++j, ++slot) {
            int d0 = int(idx[first + i]), d1 = int(idx[first + j]);
            if (rx[d0] > rx[d1]) {
                const int t = d0;
                d0 = d1;
                d1 = t;
            }
            if (b >= 0) {
                pair_key[slot] = unsigned(rx[d0]) * unsigned(n_rx) + unsigned(rx[d1]);
                pair_det0[slot] = d0;
                pair_det1[slot] = d1;
                pair_beacon[slot] = b;
            } else {
                task_det0[slot] = d0;
                task_det1[slot] = d1;
            }
        }
}
// the columns the estimator reads, in bucket order (perm = the stable sort of the pairs by key)
__global__ void k_gather_pairs(const unsigned* __restrict__ perm, const int* __restrict__ pair_det0,
                               const int* __restrict__ pair_det1, const int* __restrict__ pair_beacon,
                               const double* __restrict__ ts, const double* __restrict__ soa,
                               const double* __restrict__ q, int n_pairs, double* __restrict__ b_ts,
                               double* __restrict__ b_soa0, double* __restrict__ b_soa1, double* __restrict__ b_q0,
                               double* __restrict__ b_q1, int* __restrict__ b_beacon) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const unsigned src = perm[p];
    const int d0 = pair_det0[src], d1 = pair_det1[src];
    b_ts[p] = ts[d0];
    b_soa0[p] = soa[d0];
    b_soa1[p] = soa[d1];
    b_q0[p] = q[d0];
    b_q1[p] = q[d1];
    b_beacon[p] = pair_beacon[src];
}
// bucket_ptr[key] = first position of `key` in the sorted keys (n_keys + 1 entries, the last one n_pairs)
__global__ void k_bucket_bounds(const unsigned* __restrict__ key_sorted, int n_pairs, int n_keys,
                                unsigned* __restrict__ bucket_ptr) {
    const int key = blockIdx.x * blockDim.x + threadIdx.x;
    if (key > n_keys) return;
    int lo = 0, hi = n_pairs;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (key_sorted[mid] < unsigned(key))
            lo = mid + 1;
        else
            hi = mid;
    }
    bucket_ptr[key] = unsigned(lo);
}

// ---------------------------------------------------------------- the estimator: one wavefront per task
// (the wave helpers, Window, wave_median and the task itself are tdoa_task.hpp's)
struct PairList {  // tdoa_task.hpp's LIST: the beacon pairs of one receiver pair, in match order
    const double *ts, *soa0, *soa1, *q0, *q1;
    int n;
    const int* beacon_of;
    const double *dist0, *dist1;  // the rows of rx0 and of rx1 in dist[n_rx][n_beacons]
    __device__ __forceinline__ int beacon(int i) const { return beacon_of[i]; }
    __device__ __forceinline__ double beacon_tdoa(int i) const {
        const int b = beacon_of[i];
        return (dist0[b] - dist1[b]) / kSpeedOfLight;
    }
};

template <int DEG, int MODEL>
__global__ __launch_bounds__(kBlock) void k_estimate(
    const int* __restrict__ task_det0, const int* __restrict__ task_det1, const int* __restrict__ rx,
    const double* __restrict__ ts, const double* __restrict__ soa, const double* __restrict__ q,
    const unsigned* __restrict__ bucket_ptr, int n_rx, int n_beacons, const double* __restrict__ b_ts,
    const double* __restrict__ b_soa0, const double* __restrict__ b_soa1, const double* __restrict__ b_q0,
    const double* __restrict__ b_q1, const int* __restrict__ b_beacon, const double* __restrict__ dist,
    double window, double sample_rate, int n_tasks, unsigned* __restrict__ ok, double* __restrict__ out_val,
    int* __restrict__ out_n_window, int* __restrict__ out_n_kept, int* __restrict__ out_pick) {
    __shared__ double s_window[kWaves][kLdsWindow];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int task = blockIdx.x * kWaves + wave;
    if (task >= n_tasks) return;  // the whole wavefront
    const int d0 = task_det0[task], d1 = task_det1[task];
    const int rx0 = rx[d0], rx1 = rx[d1];
    const unsigned key = unsigned(rx0) * unsigned(n_rx) + unsigned(rx1);
    const int bucket = int(bucket_ptr[key]), n_list = int(bucket_ptr[key + 1]) - bucket;
    const PairList L{b_ts + bucket, b_soa0 + bucket, b_soa1 + bucket, b_q0 + bucket, b_q1 + bucket, n_list, b_beacon + bucket,
                     dist + size_t(rx0) * n_beacons, dist + size_t(rx1) * n_beacons};
    const thr::tdoa_task::Estimate e =
        thr::tdoa_task::estimate<DEG, MODEL>(L, ts[d0], soa[d0], soa[d1], window, sample_rate, lane, s_window[wave]);
    const bool good = e.good;
    const double tdoa = e.tdoa, quality = e.quality;
    const int pick0 = e.pick0, pick1 = e.pick1;
    if (lane == 0) {
        if (out_n_window) out_n_window[task] = e.n_window;
        if (out_n_kept) out_n_kept[task] = e.n_kept;
    }
    if (lane == 0) {
        ok[task] = good ? 1u : 0u;
        out_val[3 * size_t(task)] = tdoa;
        out_val[3 * size_t(task) + 1] = (q[d0] + q[d1]) / 2.0;
        out_val[3 * size_t(task) + 2] = quality;
        if (out_pick) {
            out_pick[2 * size_t(task)] = pick0;
            out_pick[2 * size_t(task) + 1] = pick1;
        }
    }
}

// ---------------------------------------------------------------- the output orders
__global__ void k_fail_flags(const unsigned* __restrict__ ok, int n_tasks, unsigned* __restrict__ fail) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t <= n_tasks) fail[t] = t < n_tasks ? 1u - ok[t] : 0u;
}
// rows and failures in task order (= match order, then combination order)
__global__ void k_emit_rows(const unsigned* __restrict__ ok, const unsigned* __restrict__ ok_excl,
                            const unsigned* __restrict__ fail_excl, const int* __restrict__ task_det0,
                            const int* __restrict__ task_det1, const int* __restrict__ rx,
                            const double* __restrict__ val, int n_tasks, int* __restrict__ row_rx,
                            long long* __restrict__ row_det, double* __restrict__ row_val,
                            long long* __restrict__ fail) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tasks) return;
    const int d0 = task_det0[t], d1 = task_det1[t];
    if (ok[t]) {
        const size_t r = ok_excl[t];
        row_rx[2 * r] = rx[d0];
        row_rx[2 * r + 1] = rx[d1];
        row_det[2 * r] = d0;
        row_det[2 * r + 1] = d1;
        for (int k = 0; k < 3; ++k) row_val[3 * r + k] = val[3 * size_t(t) + k];
    } else {
        const size_t f = fail_excl[t];
        fail[2 * f] = d0;
        fail[2 * f + 1] = d1;
    }
}
// a mobile match with at least one row is a group
__global__ void k_group_flags(const int* __restrict__ beacon, const unsigned* __restrict__ task_base,
                              const unsigned* __restrict__ ok_excl, int n_matches, unsigned* __restrict__ flag) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m > n_matches) return;
    flag[m] = (m < n_matches && beacon[m] < 0 && ok_excl[task_base[m + 1]] > ok_excl[task_base[m]]) ? 1u : 0u;
}
__global__ void k_emit_groups(const unsigned* __restrict__ flag, const unsigned* __restrict__ flag_excl,
                              const unsigned* __restrict__ task_base, const unsigned* __restrict__ ok_excl,
                              int n_matches, long long* __restrict__ group_id, long long* __restrict__ group_ptr) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_matches || !flag[m]) return;
    group_id[flag_excl[m]] = m;
    group_ptr[flag_excl[m]] = (long long)ok_excl[task_base[m]];
}

#define T_TRY THR_HIP_TRY

// exclusive sum of n unsigned values (n >= 1), the shared temporary grown on demand
hipError_t exclusive_sum(DevBuf& tmp, size_t& tmp_bytes, const unsigned* in, unsigned* out, int n, hipStream_t s) {
    size_t need = 0;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, need, in, out, n, s);
    if (e != hipSuccess) return e;
    if (need > tmp_bytes) {
        if ((e = tmp.alloc(need)) != hipSuccess) return e;
        tmp_bytes = need;
    }
    return hipcub::DeviceScan::ExclusiveSum(tmp.p, need, in, out, n, s);
}

inline dim3 grid_for(size_t n) { return dim3(unsigned((n + kBlock - 1) / kBlock)); }

thread_local double g_times_ms[3] = {0, 0, 0};  // last thr_tdoa of this thread: copies in, kernels, copies out

}  // namespace

// The stage on device pointers (post_stages.hpp).  thr_tdoa has walked the matches on the host and passes
// the task and pair totals; thr_postdetect passes -1 and the totals are read off the two scans.  Nothing
// here validates the CSR: see the callers for why they may hand it over.
int thr::tdoa_core(int n, const int* d_rx, const double* d_ts, const double* d_soa, const double* d_en,
                   const double* d_no, int nm, const long long* d_ptr, const long long* d_idx, const int* d_beacon,
                   int n_rx, int n_beacons, const double* d_dist, double window, double sample_rate, int deg,
                   int model, long long n_tasks, long long n_pairs, hipStream_t s, TdoaOut& out, DevBuf* picks) {
    const int n_keys = n_rx * n_rx;
    const dim3 blk(kBlock);

    // ---- 1. pairs per match, their slots, the expansion
    DevBuf d_q, d_cnt_b, d_cnt_t, d_base_b, d_base_t, d_tmp;
    DevBuf d_key, d_pd0, d_pd1, d_pb, d_td0, d_td1;
    size_t tmp_bytes = 0;
    T_TRY(d_q.alloc(size_t(n) * 8));
    T_TRY(d_cnt_b.alloc((size_t(nm) + 1) * 4));
    T_TRY(d_cnt_t.alloc((size_t(nm) + 1) * 4));
    T_TRY(d_base_b.alloc((size_t(nm) + 1) * 4));
    T_TRY(d_base_t.alloc((size_t(nm) + 1) * 4));
    hipLaunchKernelGGL(k_quality, grid_for(n), blk, 0, s, d_en, d_no, n, d_q.as<double>());
    hipLaunchKernelGGL(k_pair_counts, grid_for(size_t(nm) + 1), blk, 0, s, d_ptr, d_beacon, nm,
                       d_cnt_b.as<unsigned>(), d_cnt_t.as<unsigned>());
    T_TRY(hipGetLastError());
    T_TRY(exclusive_sum(d_tmp, tmp_bytes, d_cnt_b.as<unsigned>(), d_base_b.as<unsigned>(), nm + 1, s));
    T_TRY(exclusive_sum(d_tmp, tmp_bytes, d_cnt_t.as<unsigned>(), d_base_t.as<unsigned>(), nm + 1, s));
    if (n_tasks < 0 || n_pairs < 0) {  // not claimed by the caller: the scans' totals
        unsigned totals[2] = {0, 0};
        T_TRY(hipMemcpy(&totals[0], d_base_t.as<unsigned>() + nm, 4, hipMemcpyDeviceToHost));
        T_TRY(hipMemcpy(&totals[1], d_base_b.as<unsigned>() + nm, 4, hipMemcpyDeviceToHost));
        n_tasks = totals[0];
        n_pairs = totals[1];
    }
    const int nt = int(n_tasks), np = int(n_pairs);
    out.n_tasks = size_t(nt);
    out.n_pairs = size_t(np);
    if (nt == 0) return THR_OK;  // no mobile detection pair: nothing more to launch
    T_TRY(d_key.alloc(size_t(np) * 4));
    T_TRY(d_pd0.alloc(size_t(np) * 4));
    T_TRY(d_pd1.alloc(size_t(np) * 4));
    T_TRY(d_pb.alloc(size_t(np) * 4));
    T_TRY(d_td0.alloc(size_t(nt) * 4));
    T_TRY(d_td1.alloc(size_t(nt) * 4));
    hipLaunchKernelGGL(k_expand, grid_for(nm), blk, 0, s, d_ptr, d_idx,
                       d_beacon, d_rx, nm, n_rx, d_base_b.as<unsigned>(), d_base_t.as<unsigned>(),
                       d_key.as<unsigned>(), d_pd0.as<int>(), d_pd1.as<int>(), d_pb.as<int>(), d_td0.as<int>(),
                       d_td1.as<int>());
    T_TRY(hipGetLastError());

    // ---- 2. the beacon pairs into their receiver pair's list, match order kept
    DevBuf d_key_s, d_iota, d_perm, d_bucket, d_bts, d_bs0, d_bs1, d_bq0, d_bq1, d_bb;
    T_TRY(d_bucket.alloc((size_t(n_keys) + 2) * 4));
    T_TRY(d_bts.alloc(size_t(np) * 8));
    T_TRY(d_bs0.alloc(size_t(np) * 8));
    T_TRY(d_bs1.alloc(size_t(np) * 8));
    T_TRY(d_bq0.alloc(size_t(np) * 8));
    T_TRY(d_bq1.alloc(size_t(np) * 8));
    T_TRY(d_bb.alloc(size_t(np) * 4));
    if (np > 0) {
        T_TRY(d_key_s.alloc(size_t(np) * 4));
        T_TRY(d_iota.alloc(size_t(np) * 4));
        T_TRY(d_perm.alloc(size_t(np) * 4));
        hipLaunchKernelGGL(k_iota, grid_for(np), blk, 0, s, d_iota.as<unsigned>(), np);
        T_TRY(hipGetLastError());
        int key_bits = 1;
        while ((1 << key_bits) < n_keys) ++key_bits;
        size_t need = 0;
        T_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, need, d_key.as<unsigned>(), d_key_s.as<unsigned>(),
                                                 d_iota.as<unsigned>(), d_perm.as<unsigned>(), np, 0, key_bits, s));
        if (need > tmp_bytes) {
            T_TRY(d_tmp.alloc(need));
            tmp_bytes = need;
        }
        T_TRY(hipcub::DeviceRadixSort::SortPairs(d_tmp.p, need, d_key.as<unsigned>(), d_key_s.as<unsigned>(),
                                                 d_iota.as<unsigned>(), d_perm.as<unsigned>(), np, 0, key_bits, s));
        hipLaunchKernelGGL(k_gather_pairs, grid_for(np), blk, 0, s, d_perm.as<unsigned>(), d_pd0.as<int>(),
                           d_pd1.as<int>(), d_pb.as<int>(), d_ts, d_soa, d_q.as<double>(), np,
                           d_bts.as<double>(), d_bs0.as<double>(), d_bs1.as<double>(), d_bq0.as<double>(),
                           d_bq1.as<double>(), d_bb.as<int>());
        hipLaunchKernelGGL(k_bucket_bounds, grid_for(size_t(n_keys) + 1), blk, 0, s, d_key_s.as<unsigned>(), np, n_keys,
                           d_bucket.as<unsigned>());
        T_TRY(hipGetLastError());
    } else {
        T_TRY(hipMemsetAsync(d_bucket.p, 0, (size_t(n_keys) + 2) * 4, s));  // no beacon match: every list is empty
    }

    // ---- 3. one wavefront per task
    DevBuf d_ok, d_val;
    T_TRY(d_ok.alloc((size_t(nt) + 1) * 4));
    T_TRY(d_val.alloc(size_t(nt) * 24));
    T_TRY(out.n_window.alloc(size_t(nt) * 4));
    T_TRY(out.n_kept.alloc(size_t(nt) * 4));
    T_TRY(hipMemsetAsync(d_ok.p, 0, (size_t(nt) + 1) * 4, s));
    const dim3 est_grid(unsigned((nt + kWaves - 1) / kWaves));
    int* d_pick = nullptr;
    if (picks) {
        T_TRY(picks->alloc(size_t(nt) * 8));
        d_pick = picks->as<int>();
    }
#define LAUNCH_ESTIMATE(DEG, MODEL)                                                                                 \
    hipLaunchKernelGGL((k_estimate<DEG, MODEL>), est_grid, blk, 0, s, d_td0.as<int>(), d_td1.as<int>(), d_rx,       \
                       d_ts, d_soa, d_q.as<double>(), d_bucket.as<unsigned>(), n_rx,        \
                       n_beacons, d_bts.as<double>(), d_bs0.as<double>(), d_bs1.as<double>(), d_bq0.as<double>(),     \
                       d_bq1.as<double>(), d_bb.as<int>(), d_dist, window, sample_rate, nt,              \
                       d_ok.as<unsigned>(), d_val.as<double>(), out.n_window.as<int>(), out.n_kept.as<int>(), d_pick)
    if (model == THR_TDOA_NEAREST)
        LAUNCH_ESTIMATE(1, THR_TDOA_NEAREST);  // (the degree is not read)
    else if (model == THR_TDOA_LINEAR)
        LAUNCH_ESTIMATE(1, THR_TDOA_LINEAR);
    else if (model == THR_TDOA_WEIGHTED_POLY) {
        if (deg == 1)
            LAUNCH_ESTIMATE(1, THR_TDOA_WEIGHTED_POLY);
        else if (deg == 2)
            LAUNCH_ESTIMATE(2, THR_TDOA_WEIGHTED_POLY);
        else
            LAUNCH_ESTIMATE(3, THR_TDOA_WEIGHTED_POLY);
    } else if (deg == 1)
        LAUNCH_ESTIMATE(1, THR_TDOA_POLY);
    else if (deg == 2)
        LAUNCH_ESTIMATE(2, THR_TDOA_POLY);
    else
        LAUNCH_ESTIMATE(3, THR_TDOA_POLY);
#undef LAUNCH_ESTIMATE
    T_TRY(hipGetLastError());

    // ---- 4. rows, failures and groups in the reference's orders
    DevBuf d_ok_ex, d_fail, d_fail_ex, d_gflag, d_gflag_ex;
    T_TRY(d_ok_ex.alloc((size_t(nt) + 1) * 4));
    T_TRY(d_fail.alloc((size_t(nt) + 1) * 4));
    T_TRY(d_fail_ex.alloc((size_t(nt) + 1) * 4));
    T_TRY(d_gflag.alloc((size_t(nm) + 1) * 4));
    T_TRY(d_gflag_ex.alloc((size_t(nm) + 1) * 4));
    T_TRY(out.row_rx.alloc(size_t(nt) * 8));
    T_TRY(out.row_det.alloc(size_t(nt) * 16));
    T_TRY(out.row_val.alloc(size_t(nt) * 24));
    T_TRY(out.fail.alloc(size_t(nt) * 16));
    T_TRY(out.group_id.alloc(size_t(nm) * 8));
    T_TRY(out.group_ptr.alloc((size_t(nm) + 1) * 8));
    hipLaunchKernelGGL(k_fail_flags, grid_for(size_t(nt) + 1), blk, 0, s, d_ok.as<unsigned>(), nt, d_fail.as<unsigned>());
    T_TRY(hipGetLastError());
    T_TRY(exclusive_sum(d_tmp, tmp_bytes, d_ok.as<unsigned>(), d_ok_ex.as<unsigned>(), nt + 1, s));
    T_TRY(exclusive_sum(d_tmp, tmp_bytes, d_fail.as<unsigned>(), d_fail_ex.as<unsigned>(), nt + 1, s));
    hipLaunchKernelGGL(k_emit_rows, grid_for(nt), blk, 0, s, d_ok.as<unsigned>(), d_ok_ex.as<unsigned>(),
                       d_fail_ex.as<unsigned>(), d_td0.as<int>(), d_td1.as<int>(), d_rx, d_val.as<double>(), nt,
                       out.row_rx.as<int>(), out.row_det.as<long long>(), out.row_val.as<double>(),
                       out.fail.as<long long>());
    hipLaunchKernelGGL(k_group_flags, grid_for(size_t(nm) + 1), blk, 0, s, d_beacon, d_base_t.as<unsigned>(),
                       d_ok_ex.as<unsigned>(), nm, d_gflag.as<unsigned>());
    T_TRY(hipGetLastError());
    T_TRY(exclusive_sum(d_tmp, tmp_bytes, d_gflag.as<unsigned>(), d_gflag_ex.as<unsigned>(), nm + 1, s));
    hipLaunchKernelGGL(k_emit_groups, grid_for(nm), blk, 0, s, d_gflag.as<unsigned>(), d_gflag_ex.as<unsigned>(),
                       d_base_t.as<unsigned>(), d_ok_ex.as<unsigned>(), nm, out.group_id.as<long long>(),
                       out.group_ptr.as<long long>());
    T_TRY(hipGetLastError());
    unsigned n_rows = 0, n_fail = 0, n_groups = 0;
    T_TRY(hipMemcpy(&n_rows, d_ok_ex.as<unsigned>() + nt, 4, hipMemcpyDeviceToHost));
    T_TRY(hipMemcpy(&n_fail, d_fail_ex.as<unsigned>() + nt, 4, hipMemcpyDeviceToHost));
    T_TRY(hipMemcpy(&n_groups, d_gflag_ex.as<unsigned>() + nm, 4, hipMemcpyDeviceToHost));
    if (size_t(n_rows) + size_t(n_fail) != size_t(nt) || n_groups > n_rows)
        return thr::fail_msg(THR_ERR_DEVICE, "thr_tdoa: %u rows and %u failures for %d tasks", n_rows, n_fail, nt);
    out.n_rows = n_rows;
    out.n_fail = n_fail;
    out.n_groups = n_groups;
    return THR_OK;
}

extern "C" int thr_tdoa_model(int device_id, size_t n_det, const int32_t* rx, const double* timestamp,
                              const double* soa, const double* energy, const double* noise, size_t n_matches,
                              const int64_t* match_ptr, const int64_t* match_idx, const int32_t* match_beacon, int n_rx,
                              int n_beacons, const double* dist, double window, double sample_rate, int deg,
                              size_t n_tasks, int32_t* row_rx_out, int64_t* row_det_out, double* row_val_out,
                              size_t* n_rows_out, int64_t* group_id_out, int64_t* group_ptr_out, size_t* n_groups_out,
                              int64_t* fail_out, size_t* n_fail_out, int32_t* n_window_out, int32_t* n_kept_out,
                              int model, int32_t* pick_out) try {
    if (n_rows_out) *n_rows_out = 0;
    if (n_groups_out) *n_groups_out = 0;
    if (n_fail_out) *n_fail_out = 0;
    g_times_ms[0] = g_times_ms[1] = g_times_ms[2] = 0;
    if (!n_rows_out || !n_groups_out || !n_fail_out || !group_ptr_out || !match_ptr)
        return thr::fail_msg(THR_ERR_ARG, "thr_tdoa: null argument");
    if (model < THR_TDOA_POLY || model > THR_TDOA_LINEAR)
        return thr::fail_msg(THR_ERR_ARG, "thr_tdoa: model must be THR_TDOA_POLY (0) to THR_TDOA_LINEAR (3), not %d", model);
    const bool fits = model == THR_TDOA_POLY || model == THR_TDOA_WEIGHTED_POLY;
    if (fits && (deg < 1 || deg > 3)) return thr::fail_msg(THR_ERR_ARG, "thr_tdoa: deg must be 1, 2 or 3, not %d", deg);
    if (n_rx < 1 || n_rx > kMaxReceivers)
        return thr::fail_msg(THR_ERR_ARG, "thr_tdoa: 1 to %d receivers, not %d", kMaxReceivers, n_rx);
    if (n_beacons < 0 || (n_beacons > 0 && !dist)) return thr::fail_msg(THR_ERR_ARG, "thr_tdoa: bad beacon table");
    if (n_det > size_t(1) << 28 || n_matches > size_t(1) << 28)
        return thr::fail_msg(THR_ERR_ARG, "thr_tdoa: too many detections or matches");
    if (n_matches && (!rx || !timestamp || !soa || !energy || !noise || !match_idx || !match_beacon))
        return thr::fail_msg(THR_ERR_ARG, "thr_tdoa: null argument");

    // ---- everything a kernel will index with is checked here, before anything is launched
    if (match_ptr[0] != 0) return thr::fail_msg(THR_ERR_ARG, "thr_tdoa: match_ptr[0] must be 0");
    size_t total_tasks = 0, total_pairs = 0;
    std::vector<size_t> seen(size_t(n_rx), 0);  // seen[r] = m + 1: receiver r occurs in match m
    for (size_t m = 0; m < n_matches; ++m) {
        const int64_t a = match_ptr[m], e = match_ptr[m + 1];
        if (e < a) return thr::fail_msg(THR_ERR_ARG, "thr_tdoa: match_ptr decreases at match %zu", m);
        if (match_beacon[m] < -1 || match_beacon[m] >= n_beacons)
            return thr::fail_msg(THR_ERR_ARG, "thr_tdoa: match %zu names beacon %d of %d", m, match_beacon[m], n_beacons);
        for (int64_t i = a; i < e; ++i) {
            const int64_t d = match_idx[i];
            if (d < 0 || size_t(d) >= n_det)
                return thr::fail_msg(THR_ERR_ARG, "thr_tdoa: match %zu holds detection %lld of %zu", m, (long long)d, n_det);
            if (rx[d] < 0 || rx[d] >= n_rx)
                return thr::fail_msg(THR_ERR_ARG, "thr_tdoa: detection %lld has receiver index %d of %d", (long long)d, rx[d], n_rx);
            if (seen[size_t(rx[d])] == m + 1)
                return thr::fail_msg(THR_ERR_ARG, "thr_tdoa: match %zu holds two detections of one receiver (detection %lld)",
                                     m, (long long)d);
            seen[size_t(rx[d])] = m + 1;
        }
        const size_t k = size_t(e - a), pairs = k * (k ? k - 1 : 0) / 2;
        (match_beacon[m] >= 0 ? total_pairs : total_tasks) += pairs;
    }
    if (total_tasks > size_t(1) << 28 || total_pairs > size_t(1) << 28)
        return thr::fail_msg(THR_ERR_ARG, "thr_tdoa: too many detection pairs");
    if (total_tasks != n_tasks)
        return thr::fail_msg(THR_ERR_ARG, "thr_tdoa: the mobile matches hold %zu detection pairs, n_tasks says %zu",
                             total_tasks, n_tasks);
    if (n_tasks && (!row_rx_out || !row_det_out || !row_val_out || !group_id_out || !fail_out))
        return thr::fail_msg(THR_ERR_ARG, "thr_tdoa: null argument");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return thr::fail_msg(THR_ERR_DEVICE, "no HIP device available (this engine has no CPU fallback)");
    if (device_id < 0 || device_id >= ndev) return thr::fail_msg(THR_ERR_ARG, "bad device_id %d", device_id);
    group_ptr_out[0] = 0;
    if (n_tasks == 0) return THR_OK;  // no mobile detection pair: nothing to launch (the times stay zero)
    T_TRY(hipSetDevice(device_id));
    const int n = int(n_det), nm = int(n_matches), nt = int(n_tasks);
    const size_t n_idx = size_t(match_ptr[n_matches]);
    hipStream_t s = nullptr;
    Event ev[4];
    for (Event& e : ev) T_TRY(e.create());

    DevBuf d_rx, d_ts, d_soa, d_en, d_no, d_ptr, d_idx, d_beacon, d_dist;
    T_TRY(d_rx.alloc(size_t(n) * 4));
    T_TRY(d_ts.alloc(size_t(n) * 8));
    T_TRY(d_soa.alloc(size_t(n) * 8));
    T_TRY(d_en.alloc(size_t(n) * 8));
    T_TRY(d_no.alloc(size_t(n) * 8));
    T_TRY(d_ptr.alloc((size_t(nm) + 1) * 8));
    T_TRY(d_idx.alloc(n_idx * 8));
    T_TRY(d_beacon.alloc(size_t(nm) * 4));
    T_TRY(d_dist.alloc(size_t(n_rx) * size_t(n_beacons) * 8));
    T_TRY(hipEventRecord(ev[0].e, s));
    T_TRY(hipMemcpy(d_rx.p, rx, size_t(n) * 4, hipMemcpyHostToDevice));
    T_TRY(hipMemcpy(d_ts.p, timestamp, size_t(n) * 8, hipMemcpyHostToDevice));
    T_TRY(hipMemcpy(d_soa.p, soa, size_t(n) * 8, hipMemcpyHostToDevice));
    T_TRY(hipMemcpy(d_en.p, energy, size_t(n) * 8, hipMemcpyHostToDevice));
    T_TRY(hipMemcpy(d_no.p, noise, size_t(n) * 8, hipMemcpyHostToDevice));
    T_TRY(hipMemcpy(d_ptr.p, match_ptr, (size_t(nm) + 1) * 8, hipMemcpyHostToDevice));
    if (n_idx) T_TRY(hipMemcpy(d_idx.p, match_idx, n_idx * 8, hipMemcpyHostToDevice));
    T_TRY(hipMemcpy(d_beacon.p, match_beacon, size_t(nm) * 4, hipMemcpyHostToDevice));
    if (n_beacons) T_TRY(hipMemcpy(d_dist.p, dist, size_t(n_rx) * size_t(n_beacons) * 8, hipMemcpyHostToDevice));
    T_TRY(hipEventRecord(ev[1].e, s));

    thr::TdoaOut out;
    DevBuf d_pick;
    const int rc = thr::tdoa_core(n, d_rx.as<int>(), d_ts.as<double>(), d_soa.as<double>(), d_en.as<double>(),
                                  d_no.as<double>(), nm, d_ptr.as<long long>(), d_idx.as<long long>(), d_beacon.as<int>(),
                                  n_rx, n_beacons, d_dist.as<double>(), window, sample_rate, deg, model,
                                  (long long)n_tasks, (long long)total_pairs, s, out, pick_out ? &d_pick : nullptr);
    if (rc != THR_OK) return rc;
    const size_t n_rows = out.n_rows, n_fail = out.n_fail, n_groups = out.n_groups;
    T_TRY(hipEventRecord(ev[2].e, s));

    T_TRY(hipMemcpy(row_rx_out, out.row_rx.p, n_rows * 8, hipMemcpyDeviceToHost));
    T_TRY(hipMemcpy(row_det_out, out.row_det.p, n_rows * 16, hipMemcpyDeviceToHost));
    T_TRY(hipMemcpy(row_val_out, out.row_val.p, n_rows * 24, hipMemcpyDeviceToHost));
    T_TRY(hipMemcpy(fail_out, out.fail.p, n_fail * 16, hipMemcpyDeviceToHost));
    T_TRY(hipMemcpy(group_id_out, out.group_id.p, n_groups * 8, hipMemcpyDeviceToHost));
    T_TRY(hipMemcpy(group_ptr_out, out.group_ptr.p, n_groups * 8, hipMemcpyDeviceToHost));
    group_ptr_out[n_groups] = int64_t(n_rows);
    if (n_window_out) T_TRY(hipMemcpy(n_window_out, out.n_window.p, size_t(nt) * 4, hipMemcpyDeviceToHost));
    if (n_kept_out) T_TRY(hipMemcpy(n_kept_out, out.n_kept.p, size_t(nt) * 4, hipMemcpyDeviceToHost));
    if (pick_out) T_TRY(hipMemcpy(pick_out, d_pick.p, size_t(nt) * 8, hipMemcpyDeviceToHost));
    T_TRY(hipEventRecord(ev[3].e, s));
    T_TRY(hipEventSynchronize(ev[3].e));
    for (int k = 0; k < 3; ++k) {
        float ms = 0;
        T_TRY(hipEventElapsedTime(&ms, ev[k].e, ev[k + 1].e));
        g_times_ms[k] = ms;
    }
    *n_rows_out = n_rows;
    *n_groups_out = n_groups;
    *n_fail_out = n_fail;
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_tdoa_model");
}

extern "C" int thr_tdoa(int device_id, size_t n_det, const int32_t* rx, const double* timestamp, const double* soa,
                        const double* energy, const double* noise, size_t n_matches, const int64_t* match_ptr,
                        const int64_t* match_idx, const int32_t* match_beacon, int n_rx, int n_beacons,
                        const double* dist, double window, double sample_rate, int deg, size_t n_tasks,
                        int32_t* row_rx_out, int64_t* row_det_out, double* row_val_out, size_t* n_rows_out,
                        int64_t* group_id_out, int64_t* group_ptr_out, size_t* n_groups_out, int64_t* fail_out,
                        size_t* n_fail_out, int32_t* n_window_out, int32_t* n_kept_out) try {
    return thr_tdoa_model(device_id, n_det, rx, timestamp, soa, energy, noise, n_matches, match_ptr, match_idx,
                          match_beacon, n_rx, n_beacons, dist, window, sample_rate, deg, n_tasks, row_rx_out, row_det_out,
                          row_val_out, n_rows_out, group_id_out, group_ptr_out, n_groups_out, fail_out, n_fail_out,
                          n_window_out, n_kept_out, THR_TDOA_POLY, nullptr);
} catch (...) {
    return thr::on_exception("thr_tdoa");
}

extern "C" int thr_debug_tdoa_times(double* ms_out) try {
    if (!ms_out) return thr::fail_msg(THR_ERR_ARG, "thr_debug_tdoa_times: null argument");
    for (int k = 0; k < 3; ++k) ms_out[k] = g_times_ms[k];
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_tdoa_times");
}
