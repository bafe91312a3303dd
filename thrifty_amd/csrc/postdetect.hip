// The post-detect chain in one call (reference thrifty/kitchen_sink.py: postdetect): identify -> match ->
// tdoa -> pos on device-resident intermediates.  The four stages are the cores of identify.hip, match.hip,
// tdoa.hip and pos.hip (post_stages.hpp): the same kernels in the same order as thr_identify, thr_match,
// thr_tdoa and thr_pos.  What the Python modules rebuild on the host between the staged calls is done
// here by five small memory-bound kernels:
//   k_gather_toads   the six toads columns (rxid, txid, timestamp, soa, energy, noise) through kept_order;
//   k_dense_rx       every detection's index in rx_ids (bisection over the table staged in LDS, -1: not
//                    in it) -- monotone in the id, which k_expand's "det0 = the lower receiver" relies on;
//   k_match_meta     per match the beacon index of its first detection's txid (bisection over beacon_ids,
//                    -1: mobile), and the first member of any match whose receiver is unknown (atomicMin);
//   k_group_meta     per TDOA group the timestamp and txid of its match's first detection;
//   k_rows_for_pos   thr_tdoa's row outputs ([r][2] receivers, [r][3] values) as thr_pos's row columns
//                    (with tdoa_as_text: every tdoa through the .tdoa text's nanoseconds and back).
// n_tasks is not claimed by anybody: it is the total of k_pair_counts' scan inside the tdoa core.
//
// The wrappers' host-side validation passes (thr_tdoa's walk over the matches, thr_pos's index checks) are
// not repeated here.  They protect the kernels from a caller's CSR; here the CSR is the match core's own
// output: a match holds one entry per (group, receiver) run, so never two detections of one receiver; an
// entry is a detection index below the number of kept detections; a match has at least one entry (its
// leader's receiver); match_ptr starts at 0 and does not decrease (a prefix sum).  The one thing the data
// can still get wrong -- a receiver that rx_ids lacks -- is caught by k_match_meta before the tdoa core
// indexes anything with it.  The row receivers are indices k_dense_rx made, so they are below n_rx; a
// 1-D table has two receivers, so a match has at most two entries, one task, and a group one row.
//
// Between two stages only scalars return to the host: the counts that size the next stage's buffers, the
// match core's verdict on the timestamp order and k_match_meta's cell (in automatic mode also the identify
// core's histogram of carrier bins).  Every stage may produce nothing; the stages behind it are then
// skipped altogether -- their n == 0 case -- and nothing is launched on an empty grid.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>

#include "../../include/thrifty_hip.h"
#include "post_stages.hpp"

namespace {

using thr::DevBuf;
using thr::Event;

constexpr int kBlock = 256;        // workgroup size of every kernel here (_native.POST_WORKGROUP)
constexpr int kMaxReceivers = 64;  // pos.hip's limit; the receiver table fits one wavefront's worth of LDS
constexpr unsigned kNone = 0xFFFFFFFFu;

inline dim3 grid_for(size_t n) { return dim3(unsigned((n + kBlock - 1) / kBlock)); }

__global__ __launch_bounds__(kBlock) void k_gather_toads(
    const long long* __restrict__ order, int k, const int* __restrict__ rx, const int* __restrict__ tx,
    const double* __restrict__ ts, const double* __restrict__ soa, const double* __restrict__ en,
    const double* __restrict__ no, int* __restrict__ t_rx, int* __restrict__ t_tx, double* __restrict__ t_ts,
    double* __restrict__ t_soa, double* __restrict__ t_en, double* __restrict__ t_no) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= k) return;
    const long long src = order[i];  // < n: the identify core's compaction of a permutation of 0 .. n - 1
    t_rx[i] = rx[src];
    t_tx[i] = tx[src];
    t_ts[i] = ts[src];
    t_soa[i] = soa[src];
    t_en[i] = en[src];
    t_no[i] = no[src];
}

// the index of `id` in ids[0 .. n) (strictly ascending), -1 if it is not there
__device__ __forceinline__ int find_sorted(const int* ids, int n, int id) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (ids[mid] < id)
            lo = mid + 1;
        else
            hi = mid;
    }
    return (lo < n && ids[lo] == id) ? lo : -1;
}

__global__ __launch_bounds__(kBlock) void k_dense_rx(const int* __restrict__ t_rx, int k,
                                                     const int* __restrict__ rx_ids, int n_rx,
                                                     int* __restrict__ dense) {
    __shared__ int s_ids[kMaxReceivers];
    if (int(threadIdx.x) < n_rx) s_ids[threadIdx.x] = rx_ids[threadIdx.x];  // n_rx <= kMaxReceivers <= kBlock
    __syncthreads();
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < k) dense[i] = find_sorted(s_ids, n_rx, t_rx[i]);
}

__global__ __launch_bounds__(kBlock) void k_match_meta(const long long* __restrict__ ptr,
                                                       const long long* __restrict__ idx, int n_matches,
                                                       const int* __restrict__ t_tx, const int* __restrict__ dense,
                                                       const int* __restrict__ beacon_ids, int n_beacons,
                                                       int* __restrict__ beacon, unsigned* first_unknown) {
    const int m = blockIdx.x * kBlock + threadIdx.x;
    if (m >= n_matches) return;
    const long long a = ptr[m], e = ptr[m + 1];
    beacon[m] = find_sorted(beacon_ids, n_beacons, t_tx[idx[a]]);
    for (long long i = a; i < e; ++i)
        if (dense[idx[i]] < 0) {
            atomicMin(first_unknown, unsigned(i));  // the smallest entry position: the first in match order
            break;
        }
}

__global__ __launch_bounds__(kBlock) void k_group_meta(const long long* __restrict__ group_id, int n_groups,
                                                       const long long* __restrict__ ptr,
                                                       const long long* __restrict__ idx,
                                                       const double* __restrict__ t_ts, const int* __restrict__ t_tx,
                                                       double* __restrict__ g_ts, int* __restrict__ g_tx) {
    const int g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= n_groups) return;
    const long long first = idx[ptr[group_id[g]]];
    g_ts[g] = t_ts[first];
    g_tx[g] = t_tx[first];
}

__global__ __launch_bounds__(kBlock) void k_rows_for_pos(const int* __restrict__ row_rx,
                                                         const double* __restrict__ row_val, int n_rows,
                                                         int as_text, int* __restrict__ rx0, int* __restrict__ rx1,
                                                         double* __restrict__ tdoa, double* __restrict__ snr) {
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_rows) return;
    rx0[r] = row_rx[2 * size_t(r)];
    rx1[r] = row_rx[2 * size_t(r) + 1];
    const double t = row_val[3 * size_t(r)];
    tdoa[r] = as_text ? (t * 1e9) / 1e9 : t;  // the .tdoa text holds nanoseconds, its readers divide again
    snr[r] = row_val[3 * size_t(r) + 1];
}

// last thr_postdetect of this thread: copies in, identify, match, tdoa, pos, copies out (the fetches since)
thread_local double g_times_ms[6] = {0, 0, 0, 0, 0, 0};

}  // namespace

struct thr_post {
    int device = 0;
    thr::IdentifyOut id;
    thr::MatchOut mt;
    thr::TdoaOut td;
    thr::PosOut ps;
    DevBuf g_ts, g_tx;
    struct Slot {
        const void* p = nullptr;  // null with bytes != 0: a CSR pointer array of a stage that did not run, [0]
        size_t bytes = 0;
    } slot[THR_POST_N_OUTPUTS];
    Event ev[2];
};

namespace {

struct PostGuard {  // frees the result unless it is handed to the caller
    thr_post* r;
    ~PostGuard() { delete r; }
};

template <class T>
bool strictly_ascending(const T* v, int n) {
    for (int i = 1; i < n; ++i)
        if (!(v[i - 1] < v[i])) return false;
    return true;
}

int check_settings(const thr_post_settings* st, thr::PosPlan& plan) {
    if (st->n_map > 0 && !st->map) return thr::fail_msg(THR_ERR_ARG, "thr_postdetect: null frequency map");
    if (st->n_rx < 1 || st->n_rx > kMaxReceivers)
        return thr::fail_msg(THR_ERR_ARG, "thr_postdetect: 1 to %d receivers, not %d", kMaxReceivers, st->n_rx);
    if (!st->rx_ids || !st->rx_coords) return thr::fail_msg(THR_ERR_ARG, "thr_postdetect: null receiver table");
    if (!strictly_ascending(st->rx_ids, st->n_rx))
        return thr::fail_msg(THR_ERR_ARG, "thr_postdetect: rx_ids must be ascending and distinct");
    if (st->n_beacons < 0 || (st->n_beacons > 0 && (!st->beacon_ids || !st->dist)))
        return thr::fail_msg(THR_ERR_ARG, "thr_postdetect: bad beacon table");
    if (!strictly_ascending(st->beacon_ids, st->n_beacons))
        return thr::fail_msg(THR_ERR_ARG, "thr_postdetect: beacon_ids must be ascending and distinct");
    if (st->deg < 1 || st->deg > 3)
        return thr::fail_msg(THR_ERR_ARG, "thr_postdetect: deg must be 1, 2 or 3, not %d", st->deg);
    if (st->tdoa_model < THR_TDOA_POLY || st->tdoa_model > THR_TDOA_LINEAR)
        return thr::fail_msg(THR_ERR_ARG, "thr_postdetect: tdoa_model must be THR_TDOA_POLY (0) to THR_TDOA_LINEAR (3), not %d",
                             st->tdoa_model);
    if (st->max_iter < 0) return thr::fail_msg(THR_ERR_ARG, "thr_postdetect: max_iter must not be negative");
    return thr::pos_plan("thr_postdetect", st->n_rx, st->dims, st->rx_coords, st->first_two_rx, st->x0, plan);
}

}  // namespace

extern "C" int thr_postdetect(int device_id, size_t n_in, const int32_t* rxid, const int32_t* block,
                              const double* timestamp, const int32_t* carrier_bin, const double* carrier_offset,
                              const double* soa, const double* energy, const double* noise,
                              const thr_post_settings* st, thr_post** result_out, thr_post_counts* counts_out) try {
    if (result_out) *result_out = nullptr;
    if (counts_out) std::memset(counts_out, 0, sizeof(*counts_out));
    for (double& t : g_times_ms) t = 0;
    if (!st || !result_out || !counts_out) return thr::fail_msg(THR_ERR_ARG, "thr_postdetect: null argument");
    if (n_in && (!rxid || !block || !timestamp || !carrier_bin || !carrier_offset || !soa || !energy || !noise))
        return thr::fail_msg(THR_ERR_ARG, "thr_postdetect: null argument");
    if (n_in > size_t(1) << 28) return thr::fail_msg(THR_ERR_ARG, "thr_postdetect: too many detections");
    thr::PosPlan plan;
    if (const int rc = check_settings(st, plan)) return rc;

    thr_post* R = new thr_post;
    PostGuard guard{R};
    thr_post_counts c;
    std::memset(&c, 0, sizeof(c));
    const int n = int(n_in), n_rx = st->n_rx, n_beacons = st->n_beacons, dims = st->dims;
    auto publish = [&]() {
        R->slot[THR_POST_TXID] = {R->id.txid.p, size_t(n) * 4};
        R->slot[THR_POST_KEEP] = {R->id.keep.p, size_t(n)};
        R->slot[THR_POST_KEPT_ORDER] = {R->id.kept_order.p, c.kept * 8};
        R->slot[THR_POST_MATCH_PTR] = {R->mt.ptr.p, (c.matches + 1) * 8};
        R->slot[THR_POST_MATCH_IDX] = {R->mt.idx.p, c.match_entries * 8};
        R->slot[THR_POST_MISSES] = {R->mt.miss.p, c.misses * 8};
        R->slot[THR_POST_COLLISIONS] = {R->mt.coll.p, c.collisions * 16};
        R->slot[THR_POST_ROW_RX] = {R->td.row_rx.p, c.rows * 8};
        R->slot[THR_POST_ROW_DET] = {R->td.row_det.p, c.rows * 16};
        R->slot[THR_POST_ROW_VAL] = {R->td.row_val.p, c.rows * 24};
        R->slot[THR_POST_GROUP_ID] = {R->td.group_id.p, c.groups * 8};
        R->slot[THR_POST_GROUP_PTR] = {R->td.group_ptr.p, (c.groups + 1) * 8};
        R->slot[THR_POST_GROUP_TS] = {R->g_ts.p, c.groups * 8};
        R->slot[THR_POST_GROUP_TX] = {R->g_tx.p, c.groups * 4};
        R->slot[THR_POST_FAILURES] = {R->td.fail.p, c.failures * 16};
        R->slot[THR_POST_N_WINDOW] = {R->td.n_window.p, c.tasks * 4};
        R->slot[THR_POST_N_KEPT] = {R->td.n_kept.p, c.tasks * 4};
        R->slot[THR_POST_POS] = {R->ps.pos.p, c.groups * size_t(dims) * 8};
        R->slot[THR_POST_DOP] = {R->ps.dop.p, c.groups * 8};
        R->slot[THR_POST_SNR] = {R->ps.snr.p, c.groups * 8};
        R->slot[THR_POST_STATUS] = {R->ps.status.p, c.groups * 4};
        R->slot[THR_POST_ITERS] = {R->ps.iters.p, c.groups * 4};
        *counts_out = c;
        *result_out = R;
        guard.r = nullptr;
        return THR_OK;
    };
    if (n == 0) return publish();  // like thr_identify: nothing to do, no device needed

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return thr::fail_msg(THR_ERR_DEVICE, "no HIP device available (this engine has no CPU fallback)");
    if (device_id < 0 || device_id >= ndev) return thr::fail_msg(THR_ERR_ARG, "bad device_id %d", device_id);
    THR_HIP_TRY(hipSetDevice(device_id));
    R->device = device_id;
    hipStream_t s = nullptr;
    const dim3 blk(kBlock);
    Event ev[6];
    for (Event& e : ev) THR_HIP_TRY(e.create());
    for (Event& e : R->ev) THR_HIP_TRY(e.create());

    // ---- copies in: the eight columns and the four small tables
    DevBuf d_rx, d_blk, d_ts, d_bin, d_off, d_soa, d_en, d_no, d_rxids, d_xy, d_bids, d_dist;
    THR_HIP_TRY(d_rx.alloc(size_t(n) * 4));
    THR_HIP_TRY(d_blk.alloc(size_t(n) * 4));
    THR_HIP_TRY(d_ts.alloc(size_t(n) * 8));
    THR_HIP_TRY(d_bin.alloc(size_t(n) * 4));
    THR_HIP_TRY(d_off.alloc(size_t(n) * 8));
    THR_HIP_TRY(d_soa.alloc(size_t(n) * 8));
    THR_HIP_TRY(d_en.alloc(size_t(n) * 8));
    THR_HIP_TRY(d_no.alloc(size_t(n) * 8));
    THR_HIP_TRY(d_rxids.alloc(size_t(n_rx) * 4));
    THR_HIP_TRY(d_xy.alloc(size_t(n_rx) * size_t(dims) * 8));
    THR_HIP_TRY(d_bids.alloc(size_t(n_beacons) * 4));
    THR_HIP_TRY(d_dist.alloc(size_t(n_rx) * size_t(n_beacons) * 8));
    THR_HIP_TRY(hipEventRecord(ev[0].e, s));
    THR_HIP_TRY(hipMemcpy(d_rx.p, rxid, size_t(n) * 4, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipMemcpy(d_blk.p, block, size_t(n) * 4, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipMemcpy(d_ts.p, timestamp, size_t(n) * 8, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipMemcpy(d_bin.p, carrier_bin, size_t(n) * 4, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipMemcpy(d_off.p, carrier_offset, size_t(n) * 8, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipMemcpy(d_soa.p, soa, size_t(n) * 8, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipMemcpy(d_en.p, energy, size_t(n) * 8, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipMemcpy(d_no.p, noise, size_t(n) * 8, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipMemcpy(d_rxids.p, st->rx_ids, size_t(n_rx) * 4, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipMemcpy(d_xy.p, st->rx_coords, size_t(n_rx) * size_t(dims) * 8, hipMemcpyHostToDevice));
    if (n_beacons) {
        THR_HIP_TRY(hipMemcpy(d_bids.p, st->beacon_ids, size_t(n_beacons) * 4, hipMemcpyHostToDevice));
        THR_HIP_TRY(hipMemcpy(d_dist.p, st->dist, size_t(n_rx) * size_t(n_beacons) * 8, hipMemcpyHostToDevice));
    }
    THR_HIP_TRY(hipEventRecord(ev[1].e, s));

    // ---- identify
    if (const int rc = thr::identify_core(n, d_rx.as<int>(), d_blk.as<int>(), d_ts.as<double>(), d_bin.as<int>(),
                                          d_off.as<double>(), d_en.as<double>(), rxid, carrier_bin, st->map, st->n_map,
                                          s, R->id))
        return rc;
    const int k = R->id.n_kept;
    c.kept = size_t(k);
    THR_HIP_TRY(hipEventRecord(ev[2].e, s));

    // ---- match, on the kept detections in timestamp order (the toads order)
    DevBuf t_rx, t_tx, t_ts, t_soa, t_en, t_no, t_dense;
    if (k > 0) {
        THR_HIP_TRY(t_rx.alloc(size_t(k) * 4));
        THR_HIP_TRY(t_tx.alloc(size_t(k) * 4));
        THR_HIP_TRY(t_ts.alloc(size_t(k) * 8));
        THR_HIP_TRY(t_soa.alloc(size_t(k) * 8));
        THR_HIP_TRY(t_en.alloc(size_t(k) * 8));
        THR_HIP_TRY(t_no.alloc(size_t(k) * 8));
        THR_HIP_TRY(t_dense.alloc(size_t(k) * 4));
        hipLaunchKernelGGL(k_gather_toads, grid_for(k), blk, 0, s, R->id.kept_order.as<long long>(), k, d_rx.as<int>(),
                           R->id.txid.as<int>(), d_ts.as<double>(), d_soa.as<double>(), d_en.as<double>(),
                           d_no.as<double>(), t_rx.as<int>(), t_tx.as<int>(), t_ts.as<double>(), t_soa.as<double>(),
                           t_en.as<double>(), t_no.as<double>());
        hipLaunchKernelGGL(k_dense_rx, grid_for(k), blk, 0, s, t_rx.as<int>(), k, d_rxids.as<int>(), n_rx,
                           t_dense.as<int>());
        THR_HIP_TRY(hipGetLastError());
        if (const int rc = thr::match_core(k, t_rx.as<int>(), t_tx.as<int>(), t_ts.as<double>(), t_en.as<double>(),
                                           st->match_window, st->min_match, s, R->mt))
            return rc;
        if (R->mt.first_bad != thr::kMatchSorted) {
            double t = 0;
            THR_HIP_TRY(hipMemcpy(&t, t_ts.as<double>() + R->mt.first_bad, 8, hipMemcpyDeviceToHost));
            return thr::fail_msg(THR_ERR_ARG,
                                 "thr_match: timestamps must be non-decreasing without NaN: detection %u is %s",
                                 R->mt.first_bad, t != t ? "NaN" : "earlier than the one before it");
        }
        c.matches = R->mt.n_matches;
        c.match_entries = R->mt.n_entries;
        c.misses = R->mt.n_misses;
        c.collisions = R->mt.n_collisions;
        const long long end = (long long)c.match_entries;
        THR_HIP_TRY(hipMemcpy(R->mt.ptr.as<long long>() + c.matches, &end, 8, hipMemcpyHostToDevice));
    }
    THR_HIP_TRY(hipEventRecord(ev[3].e, s));

    // ---- tdoa
    if (c.matches > 0) {
        const int nm = int(c.matches);
        DevBuf d_beacon, d_cell;
        THR_HIP_TRY(d_beacon.alloc(size_t(nm) * 4));
        THR_HIP_TRY(d_cell.alloc(4));
        THR_HIP_TRY(hipMemsetAsync(d_cell.p, 0xFF, 4, s));
        hipLaunchKernelGGL(k_match_meta, grid_for(nm), blk, 0, s, R->mt.ptr.as<long long>(), R->mt.idx.as<long long>(),
                           nm, t_tx.as<int>(), t_dense.as<int>(), d_bids.as<int>(), n_beacons, d_beacon.as<int>(),
                           d_cell.as<unsigned>());
        THR_HIP_TRY(hipGetLastError());
        unsigned unknown = kNone;
        THR_HIP_TRY(hipMemcpy(&unknown, d_cell.p, 4, hipMemcpyDeviceToHost));
        if (unknown != kNone) {
            long long det = 0;
            int rx = 0;
            THR_HIP_TRY(hipMemcpy(&det, R->mt.idx.as<long long>() + unknown, 8, hipMemcpyDeviceToHost));
            THR_HIP_TRY(hipMemcpy(&rx, t_rx.as<int>() + det, 4, hipMemcpyDeviceToHost));
            return thr::fail_msg(THR_ERR_ARG, "thr_postdetect: detection %lld is of receiver %d, which rx_ids lacks", det,
                                 rx);
        }
        if (const int rc = thr::tdoa_core(k, t_dense.as<int>(), t_ts.as<double>(), t_soa.as<double>(), t_en.as<double>(),
                                          t_no.as<double>(), nm, R->mt.ptr.as<long long>(), R->mt.idx.as<long long>(),
                                          d_beacon.as<int>(), n_rx, n_beacons, d_dist.as<double>(), st->tdoa_window,
                                          st->sample_rate, st->deg, st->tdoa_model, -1, -1, s, R->td))
            return rc;
        c.tasks = R->td.n_tasks;
        c.rows = R->td.n_rows;
        c.groups = R->td.n_groups;
        c.failures = R->td.n_fail;
        if (c.tasks > 0) {
            const long long end = (long long)c.rows;
            THR_HIP_TRY(hipMemcpy(R->td.group_ptr.as<long long>() + c.groups, &end, 8, hipMemcpyHostToDevice));
        }
        if (c.groups > 0) {
            const int ng = int(c.groups);
            THR_HIP_TRY(R->g_ts.alloc(size_t(ng) * 8));
            THR_HIP_TRY(R->g_tx.alloc(size_t(ng) * 4));
            hipLaunchKernelGGL(k_group_meta, grid_for(ng), blk, 0, s, R->td.group_id.as<long long>(), ng,
                               R->mt.ptr.as<long long>(), R->mt.idx.as<long long>(), t_ts.as<double>(), t_tx.as<int>(),
                               R->g_ts.as<double>(), R->g_tx.as<int>());
            THR_HIP_TRY(hipGetLastError());
        }
        THR_HIP_TRY(hipStreamSynchronize(s));  // d_beacon and d_cell go out of scope
    }
    THR_HIP_TRY(hipEventRecord(ev[4].e, s));

    // ---- pos
    if (c.groups > 0) {
        const int nr = int(c.rows);
        DevBuf p_rx0, p_rx1, p_tdoa, p_snr;
        THR_HIP_TRY(p_rx0.alloc(size_t(nr) * 4));
        THR_HIP_TRY(p_rx1.alloc(size_t(nr) * 4));
        THR_HIP_TRY(p_tdoa.alloc(size_t(nr) * 8));
        THR_HIP_TRY(p_snr.alloc(size_t(nr) * 8));
        hipLaunchKernelGGL(k_rows_for_pos, grid_for(nr), blk, 0, s, R->td.row_rx.as<int>(), R->td.row_val.as<double>(), nr,
                           st->tdoa_as_text, p_rx0.as<int>(), p_rx1.as<int>(), p_tdoa.as<double>(), p_snr.as<double>());
        THR_HIP_TRY(hipGetLastError());
        if (const int rc = thr::pos_core(int(c.groups), R->td.group_ptr.as<long long>(), p_rx0.as<int>(), p_rx1.as<int>(),
                                         p_tdoa.as<double>(), p_snr.as<double>(), d_xy.as<double>(), dims, plan,
                                         st->max_iter, s, R->ps))
            return rc;
        THR_HIP_TRY(hipStreamSynchronize(s));  // the row columns go out of scope
    }
    THR_HIP_TRY(hipEventRecord(ev[5].e, s));
    THR_HIP_TRY(hipEventSynchronize(ev[5].e));
    for (int i = 0; i < 5; ++i) {
        float ms = 0;
        THR_HIP_TRY(hipEventElapsedTime(&ms, ev[i].e, ev[i + 1].e));
        g_times_ms[i] = ms;
    }
    return publish();
} catch (const std::bad_alloc&) {
    return thr::fail_msg(THR_ERR_DEVICE, "thr_postdetect: out of host memory");
} catch (...) {
    return thr::on_exception("thr_postdetect");
}

extern "C" int thr_post_fetch(thr_post* R, int which, void* dst, size_t dst_bytes) try {
    if (!R || which < 0 || which >= THR_POST_N_OUTPUTS)
        return thr::fail_msg(THR_ERR_ARG, "thr_post_fetch: no such result or output (%d)", which);
    const thr_post::Slot& slot = R->slot[which];
    if (dst_bytes != slot.bytes)
        return thr::fail_msg(THR_ERR_ARG, "thr_post_fetch: output %d holds %zu bytes, not %zu", which, slot.bytes, dst_bytes);
    if (slot.bytes == 0) return THR_OK;
    if (!dst) return thr::fail_msg(THR_ERR_ARG, "thr_post_fetch: null argument");
    if (!slot.p) {  // the CSR pointers of a stage that did not run: [0]
        std::memset(dst, 0, slot.bytes);
        return THR_OK;
    }
    THR_HIP_TRY(hipSetDevice(R->device));
    THR_HIP_TRY(hipEventRecord(R->ev[0].e, nullptr));
    THR_HIP_TRY(hipMemcpy(dst, slot.p, slot.bytes, hipMemcpyDeviceToHost));
    THR_HIP_TRY(hipEventRecord(R->ev[1].e, nullptr));
    THR_HIP_TRY(hipEventSynchronize(R->ev[1].e));
    float ms = 0;
    THR_HIP_TRY(hipEventElapsedTime(&ms, R->ev[0].e, R->ev[1].e));
    g_times_ms[5] += ms;
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_post_fetch");
}

extern "C" void thr_post_free(thr_post* R) {
    if (!R) return;
    if (R->ev[0].e) (void)hipSetDevice(R->device);  // a result that used the device frees its buffers there
    delete R;
}

extern "C" int thr_debug_post_times(double* ms_out) try {
    if (!ms_out) return thr::fail_msg(THR_ERR_ARG, "thr_debug_post_times: null argument");
    for (int i = 0; i < 6; ++i) ms_out[i] = g_times_ms[i];
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_post_times");
}
