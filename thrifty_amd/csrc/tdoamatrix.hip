// Per-beacon TDOA matrices on the device: the numbers of the reference's scripts/tdoa_matrix.py (calculate_tdoas,
// print_tdoa_matrix) for EVERY (rx0 < rx1, beacon, transmitter) cell of a deployment in one call (thr_tdoamatrix;
// the contract is in include/thrifty_hip.h).  The script estimates the TDOAs of a transmitter again with the
// matches of ONE beacon as the clock model, per cell a full run of extract_match_matrix + estimate_tdoas.
//
//   1. rows     seg_cells.hpp's front end (check_matches, pair_rows with this file's selector): the detection
//               pairs of the beacons' and the targets' matches at listed receivers, grouped by (tx, rx0, rx1) in
//               match order.  A GROUP is the row list of one transmitter at one receiver pair: as a beacon's it
//               is the LIST every task of that beacon and pair bisects, as a target's it gives the tasks.
//   2. tasks    the group table is a few dozen entries: the host reads it, pairs every target group with every
//               listed beacon b != t, orders the cells by (rx0, rx1, b, t), looks the two distances up and sends
//               the cell table back.  A cell's tasks are its target group's rows; a cell whose beacon list or
//               target list has fewer than 3 rows is THR_TDMAT_CELL_TOO_FEW and its tasks are not estimated.
//   3. estimate one wavefront per task on the beacon's list: tdoa_task.hpp, the arithmetic of thr_tdoa_model.
//   4. mask     the TDOAs a cell's tasks gave, compacted in task order; stat_tools.is_outlier per cell is
//               seg_cells.hpp's outlier_mask (median and MAD from two sorts by (cell, value)).
//   5. stats    mean, population std, rms, min and max of tdoa * 2.997e8 over the rows the mask kept: tiled
//               segmented reductions (seg_reduce.hpp), slab partials combined in tile order.
//
// No floating-point atomic; every sum has one order.  Lifetimes as in syncstats.hip: the null stream, and a
// temporary leaves scope only after a synchronisation (record_times, a read-back hipMemcpy) or through hipFree.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/thrifty_hip.h"
#include "post_stages.hpp"
#include "seg_reduce.hpp"
#include "seg_cells.hpp"
#include "tdoa_task.hpp"

// numpy's float64 operations one by one: no a * b + c may become an fma in this file (the build also passes
// -ffp-contract=off, thrifty_amd/build.py)
#pragma clang fp contract(off)

namespace {

using thr::DevBuf;
using thr::Event;
using namespace thr::seg;
namespace tt = thr::tdoa_task;

constexpr int kMinRows = 3;  // the script's `num_beacon < 3 or num_tx < 3`
static_assert(tt::kBlock == kBlock, "one workgroup size");
static_assert(THR_TDMAT_N_OUTPUTS <= kMaxOutputs, "the result handle holds every output");

// ------------------------------------------------------------------ 1. rows
struct Dets {
    const int *rx, *tx;
    const double *ts, *soa, *en, *no;
    const long long *mptr, *midx;
    const int *beacons, *targets, *receivers;
    int n_beacons, n_targets, n_receivers;  // -1: no list
};
struct TxPairs {  // k_pairs' selector: matches of the beacons and the targets, pairs of listed receivers
    Dets d;
    __device__ bool wanted(int tx) const {
        return find_sorted(d.beacons, d.n_beacons, tx) >= 0 || find_sorted(d.targets, d.n_targets, tx) >= 0;
    }
    __device__ bool kept(long long da, long long db) const {
        return find_sorted(d.receivers, d.n_receivers, d.rx[da]) >= 0 && find_sorted(d.receivers, d.n_receivers, d.rx[db]) >= 0;
    }
};
struct Src {  // the rows of all groups, in group order
    long long *det, *match;
    double *t0, *s0, *s1, *q0, *q1;  // timestamp at rx0, soa at rx0 / rx1, (energy / noise)**2 at rx0 / rx1
};
__global__ __launch_bounds__(kBlock) void k_src(Dets d, const unsigned* __restrict__ perm, const long long* __restrict__ det,
                                                const long long* __restrict__ match, int n, Src o) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const size_t j = perm[p];
    const long long d0 = det[2 * j], d1 = det[2 * j + 1];
    o.det[2 * size_t(p)] = d0;
    o.det[2 * size_t(p) + 1] = d1;
    o.match[p] = match[j];
    o.t0[p] = d.ts[d0];
    o.s0[p] = d.soa[d0];
    o.s1[p] = d.soa[d1];
    const double r0 = d.en[d0] / d.no[d0], r1 = d.en[d1] / d.no[d1];
    o.q0[p] = r0 * r0;
    o.q1[p] = r1 * r1;
}

// ------------------------------------------------------------------ 2. tasks (the cell table comes from the host)
struct Cell {
    int key[4];                   // rx0, rx1, beacon, tx
    long long start, msrc, bsrc;  // first task; first row of the target's and of the beacon's group
    int n, nb, flags, pad;        // tasks (= target rows), beacon rows
    double dist[2];               // dist(rx0, beacon), dist(rx1, beacon)
};
__global__ __launch_bounds__(kBlock) void k_pos_cell(const Cell* __restrict__ cells, int nc, int m, int* __restrict__ pos_cell) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= m) return;
    int lo = 0, hi = nc;  // the last c with start <= p
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cells[mid].start <= p) lo = mid; else hi = mid;
    }
    pos_cell[p] = lo;
}
__global__ __launch_bounds__(kBlock) void k_cell_out(const Cell* __restrict__ cells, int nc, int m, int* __restrict__ key,
                                                     long long* __restrict__ ptr, int* __restrict__ flags) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= nc) return;
    for (int k = 0; k < 4; ++k) key[4 * size_t(c) + k] = cells[c].key[k];
    ptr[c] = cells[c].start;
    flags[c] = cells[c].flags;
    if (c == nc - 1) ptr[nc] = m;
}

// ------------------------------------------------------------------ 3. the estimate: one wavefront per task
struct BeaconList {  // tdoa_task.hpp's LIST: one beacon's rows at one receiver pair
    const double *ts, *soa0, *soa1, *q0, *q1;
    int n;
    double dist0, dist1;
    __device__ __forceinline__ int beacon(int) const { return 0; }
    __device__ __forceinline__ double beacon_tdoa(int) const { return (dist0 - dist1) / tt::kSpeedOfLight; }
};
struct Tasks {
    long long *det, *match;
    double *ts, *tdoa, *snr, *quality;
    int *status, *n_window, *n_kept;
    unsigned* ok;  // n + 1 entries, the last one 0 (set before the launch)
};
template <int DEG, int MODEL>
__global__ __launch_bounds__(kBlock) void k_estimate(const Cell* __restrict__ cells, const int* __restrict__ pos_cell, Src g,
                                                     double window, double sample_rate, int n_tasks, Tasks o) {
    __shared__ double s_window[tt::kWaves][tt::kLdsWindow];
    const int lane = threadIdx.x % tt::kWave, wave = threadIdx.x / tt::kWave;
    const long long task = (long long)blockIdx.x * tt::kWaves + wave;
    if (task >= n_tasks) return;  // the whole wavefront
    const Cell& c = cells[pos_cell[task]];
    const size_t sr = size_t(c.msrc + (task - c.start));
    int status = THR_TDMAT_SKIPPED, n_window = 0, n_kept = 0;
    double tdoa = NAN, quality = NAN;
    if (c.flags == 0) {
        const BeaconList L{g.t0 + c.bsrc, g.s0 + c.bsrc, g.s1 + c.bsrc, g.q0 + c.bsrc, g.q1 + c.bsrc, c.nb, c.dist[0], c.dist[1]};
        const tt::Estimate e = tt::estimate<DEG, MODEL>(L, g.t0[sr], g.s0[sr], g.s1[sr], window, sample_rate, lane, s_window[wave]);
        status = e.good ? THR_TDMAT_OK : (e.modelled ? THR_TDMAT_OUT_OF_RANGE : THR_TDMAT_NO_MODEL);
        n_window = e.n_window;
        n_kept = e.n_kept;
        if (e.good) {
            tdoa = e.tdoa;
            quality = e.quality;
        }
    }
    if (lane == 0) {
        o.det[2 * size_t(task)] = g.det[2 * sr];
        o.det[2 * size_t(task) + 1] = g.det[2 * sr + 1];
        o.match[task] = g.match[sr];
        o.ts[task] = g.t0[sr];
        o.tdoa[task] = tdoa;
        o.snr[task] = (g.q0[sr] + g.q1[sr]) / 2.0;
        o.quality[task] = quality;
        o.status[task] = status;
        o.n_window[task] = n_window;
        o.n_kept[task] = n_kept;
        o.ok[task] = status == THR_TDMAT_OK ? 1u : 0u;
    }
}

// ------------------------------------------------------------------ 4. + 5. the TDOAs of a cell, mask, statistics
// vptr[c] = the number of TDOAs before the cell's first task; vptr[nc] = all
__global__ __launch_bounds__(kBlock) void k_ptr(const long long* __restrict__ in_ptr, const unsigned* __restrict__ incl, int nc,
                                                int n, long long* __restrict__ out) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c > nc) return;
    const long long a = c == nc ? n : in_ptr[c];
    out[c] = a == 0 ? 0 : (long long)incl[a - 1];
}
// the TDOAs in task order: seconds (the mask's values), metres (the statistics'), their cells and their tasks
__global__ __launch_bounds__(kBlock) void k_values(const unsigned* __restrict__ ok, const unsigned* __restrict__ incl,
                                                   const double* __restrict__ tdoa, const int* __restrict__ pos_cell, int n,
                                                   double* __restrict__ val, double* __restrict__ x, int* __restrict__ vcell,
                                                   unsigned* __restrict__ vtask) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n || !ok[p]) return;
    const unsigned j = incl[p] - 1;
    val[j] = tdoa[p];
    x[j] = tdoa[p] * tt::kSpeedOfLight;
    vcell[j] = pos_cell[p];
    vtask[j] = unsigned(p);
}
struct LoadMax {  // K = 1, no sum, no minimum: a cell's largest value, NaN when it holds one
    const double* v;
    __device__ void operator()(int p, double (&o)[1]) const { o[0] = v[p]; }
};
__global__ __launch_bounds__(kBlock) void k_mask_out(const unsigned char* __restrict__ vmask, const unsigned* __restrict__ vtask,
                                                     int n, unsigned char* __restrict__ mask) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j < n) mask[vtask[j]] = vmask[j];
}
// cv: LoadKept1<true>'s count, sums of x and x^2, min, max over the kept rows; cv2: LoadKept2<true>'s (null: no TDOA
// anywhere).  stats[c] = {mean, std, rms, min, max}, NaN for a cell without a kept row; counts[c] = {beacon rows,
// target rows, TDOAs, failures, kept}
__global__ __launch_bounds__(kBlock) void k_fin(const Cell* __restrict__ cells, const long long* __restrict__ vptr,
                                                const double* __restrict__ cv, const double* __restrict__ cv2, int nc,
                                                double* __restrict__ stats, long long* __restrict__ counts) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= nc) return;
    const double n = cv ? cv[5 * size_t(c)] : 0.0;
    double* s = stats + 5 * size_t(c);
    if (n > 0.0) {
        const double* v = cv + 5 * size_t(c);
        s[0] = v[1] / n;
        s[1] = sqrt(cv2[c] / n);
        s[2] = sqrt(v[2] / n);
        s[3] = v[3];
        s[4] = v[4];
    } else {
        for (int k = 0; k < 5; ++k) s[k] = NAN;
    }
    const long long got = vptr[c + 1] - vptr[c];
    long long* o = counts + 5 * size_t(c);
    o[0] = cells[c].nb;
    o[1] = cells[c].n;
    o[2] = got;
    o[3] = cells[c].flags ? 0 : cells[c].n - got;
    o[4] = (long long)n;
}

thread_local double g_tdmat_ms[5] = {0, 0, 0, 0, 0};

// a sorted copy; false when a value occurs twice
bool sorted_unique(const int32_t* list, size_t n, std::vector<int32_t>& out) {
    out.assign(list, list + n);
    std::sort(out.begin(), out.end());
    return std::adjacent_find(out.begin(), out.end()) == out.end();
}
int index_of(const int32_t* list, size_t n, int32_t v) {
    for (size_t i = 0; i < n; ++i)
        if (list[i] == v) return int(i);
    return -1;
}

}  // namespace

struct thr_tdmat : thr::seg::Result {};

extern "C" int thr_tdoamatrix(int device_id, size_t n_det, const int32_t* rxid, const int32_t* txid, const double* timestamp,
                              const double* soa, const double* energy, const double* noise, size_t n_matches,
                              const int64_t* match_ptr, const int64_t* match_idx, const int32_t* receivers, size_t n_receivers,
                              const int32_t* beacons, size_t n_beacons, const int32_t* targets, size_t n_targets,
                              const double* dist, double window, double sample_rate, int model, int deg, thr_tdmat** result_out,
                              thr_tdmat_counts* counts_out) try {
    if (result_out) *result_out = nullptr;
    if (counts_out) std::memset(counts_out, 0, sizeof(*counts_out));
    for (double& t : g_tdmat_ms) t = 0;
    if (!result_out || !counts_out || !match_ptr) return thr::fail_msg(THR_ERR_ARG, "thr_tdoamatrix: null argument");
    if (n_det && (!rxid || !txid || !timestamp || !soa || !energy || !noise))
        return thr::fail_msg(THR_ERR_ARG, "thr_tdoamatrix: null argument");
    if ((n_matches && match_ptr[n_matches] && !match_idx) || (n_beacons && !beacons) || (n_receivers && !receivers) ||
        (n_targets && !targets))
        return thr::fail_msg(THR_ERR_ARG, "thr_tdoamatrix: null argument");
    if (n_det > (size_t(1) << 28) || n_matches > (size_t(1) << 28) || n_receivers > (size_t(1) << 20) || n_targets > (size_t(1) << 20))
        return thr::fail_msg(THR_ERR_ARG, "thr_tdoamatrix: too many detections, matches or list entries");
    if (n_beacons > THR_TDMAT_MAX_BEACONS)
        return thr::fail_msg(THR_ERR_ARG, "thr_tdoamatrix: at most %d beacons, not %zu", THR_TDMAT_MAX_BEACONS, n_beacons);
    if (model < THR_TDOA_POLY || model > THR_TDOA_LINEAR)
        return thr::fail_msg(THR_ERR_ARG, "thr_tdoamatrix: model must be THR_TDOA_POLY (0) to THR_TDOA_LINEAR (3), not %d", model);
    const bool fits = model == THR_TDOA_POLY || model == THR_TDOA_WEIGHTED_POLY;
    if (fits && (deg < 1 || deg > 3)) return thr::fail_msg(THR_ERR_ARG, "thr_tdoamatrix: deg must be 1, 2 or 3, not %d", deg);
    if (!(window >= 0.0) || !(sample_rate > 0.0) || !std::isfinite(window) || !std::isfinite(sample_rate))
        return thr::fail_msg(THR_ERR_ARG, "thr_tdoamatrix: window must be a number >= 0, sample_rate positive");
    if (dist && !receivers) return thr::fail_msg(THR_ERR_ARG, "thr_tdoamatrix: dist needs the list of receivers its rows are of");
    std::vector<int32_t> bl, rl;
    if (!sorted_unique(beacons, n_beacons, bl)) return thr::fail_msg(THR_ERR_ARG, "thr_tdoamatrix: a beacon is listed twice");
    if (receivers && !sorted_unique(receivers, n_receivers, rl))
        return thr::fail_msg(THR_ERR_ARG, "thr_tdoamatrix: a receiver is listed twice");
    uint64_t n_pairs = 0;
    THR_TRY(check_matches("thr_tdoamatrix", n_det, rxid, n_matches, match_ptr, match_idx, &n_pairs, /*may_be_empty=*/true));
    const size_t n_entries = size_t(match_ptr[n_matches]);

    THR_TRY(pick_device(device_id));
    thr_tdmat* R = new thr_tdmat;
    ResultGuard guard{R};
    R->device = device_id;
    R->n_out = THR_TDMAT_N_OUTPUTS;
    hipStream_t s = nullptr;
    Event ev[5];
    for (Event& e : ev) THR_HIP_TRY(e.create());
    for (Event& e : R->ev) THR_HIP_TRY(e.create());
    DevBuf* O = R->out;
    size_t* B = R->bytes;
    // nothing selected: no cell, no task; cell_ptr is its one entry
    auto empty = [&]() -> int {
        for (int k = 0; k < THR_TDMAT_N_OUTPUTS; ++k) THR_HIP_TRY(O[k].alloc(0));
        THR_HIP_TRY(O[THR_TDMAT_CELL_PTR].alloc(8));
        THR_HIP_TRY(hipMemset(O[THR_TDMAT_CELL_PTR].p, 0, 8));
        B[THR_TDMAT_CELL_PTR] = 8;
        *result_out = R;
        guard.r = nullptr;
        return THR_OK;
    };
    if (n_pairs == 0 || n_beacons == 0) return empty();

    // ---- copies in
    DevBuf d_rx, d_tx, d_f64[4], d_mptr, d_midx, d_bl, d_tl, d_rl;
    const double* h_f64[4] = {timestamp, soa, energy, noise};
    Dets D;
    THR_HIP_TRY(d_rx.alloc(n_det * 4));
    THR_HIP_TRY(d_tx.alloc(n_det * 4));
    for (DevBuf& b : d_f64) THR_HIP_TRY(b.alloc(n_det * 8));
    THR_HIP_TRY(d_mptr.alloc((n_matches + 1) * 8));
    THR_HIP_TRY(d_midx.alloc(n_entries * 8));
    THR_HIP_TRY(hipEventRecord(ev[0].e, s));
    THR_HIP_TRY(hipMemcpy(d_rx.p, rxid, n_det * 4, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipMemcpy(d_tx.p, txid, n_det * 4, hipMemcpyHostToDevice));
    for (int k = 0; k < 4; ++k) THR_HIP_TRY(hipMemcpy(d_f64[k].p, h_f64[k], n_det * 8, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipMemcpy(d_mptr.p, match_ptr, (n_matches + 1) * 8, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipMemcpy(d_midx.p, match_idx, n_entries * 8, hipMemcpyHostToDevice));
    THR_TRY(upload_list(beacons, n_beacons, d_bl, D.n_beacons));
    THR_TRY(upload_list(n_targets ? targets : nullptr, n_targets, d_tl, D.n_targets));
    THR_TRY(upload_list(receivers, n_receivers, d_rl, D.n_receivers));
    THR_HIP_TRY(hipEventRecord(ev[1].e, s));
    D.rx = d_rx.as<int>();
    D.tx = d_tx.as<int>();
    D.ts = d_f64[0].as<double>();
    D.soa = d_f64[1].as<double>();
    D.en = d_f64[2].as<double>();
    D.no = d_f64[3].as<double>();
    D.mptr = d_mptr.as<long long>();
    D.midx = d_midx.as<long long>();
    D.beacons = d_bl.as<int>();
    D.targets = d_tl.as<int>();
    D.receivers = d_rl.as<int>();

    // ---- 1. rows
    Scratch w;
    Work W{w};
    PairRows src;
    DevBuf d_gptr, d_gkey, d_src_i64[2], d_src_f64[5];
    THR_TRY(pair_rows(TxPairs{D}, int(n_matches), w, src, d_gptr, d_gkey, s));
    if (src.m == 0) return empty();
    const int ns = src.m, ng = src.cells.nc;
    THR_HIP_TRY(d_src_i64[0].alloc(size_t(ns) * 16));
    THR_HIP_TRY(d_src_i64[1].alloc(size_t(ns) * 8));
    for (DevBuf& b : d_src_f64) THR_HIP_TRY(b.alloc(size_t(ns) * 8));
    Src G{d_src_i64[0].as<long long>(), d_src_i64[1].as<long long>(), d_src_f64[0].as<double>(), d_src_f64[1].as<double>(),
          d_src_f64[2].as<double>(),    d_src_f64[3].as<double>(),    d_src_f64[4].as<double>()};
    THR_TRY(launch(k_src, ns, s, D, src.cells.perm.as<unsigned>(), src.det.as<long long>(), src.match.as<long long>(), ns, G));
    std::vector<int32_t> h_gkey(size_t(ng) * 3);  // tx, rx0, rx1: ascending
    std::vector<long long> h_gptr(size_t(ng) + 1);
    THR_HIP_TRY(hipMemcpy(h_gkey.data(), d_gkey.p, h_gkey.size() * 4, hipMemcpyDeviceToHost));  // synchronises
    THR_HIP_TRY(hipMemcpy(h_gptr.data(), d_gptr.p, h_gptr.size() * 8, hipMemcpyDeviceToHost));

    // ---- 2. tasks: every target group with every listed beacon but itself
    std::vector<int32_t> tl;
    if (n_targets) tl.assign(targets, targets + n_targets);
    std::sort(tl.begin(), tl.end());
    std::vector<Cell> cells;
    for (int g = 0; g < ng; ++g) {
        const int32_t* key = &h_gkey[size_t(g) * 3];
        if (n_targets && !std::binary_search(tl.begin(), tl.end(), key[0])) continue;
        for (const int32_t b : bl) {
            if (b == key[0]) continue;
            Cell c{};
            c.key[0] = key[1];
            c.key[1] = key[2];
            c.key[2] = b;
            c.key[3] = key[0];
            c.msrc = h_gptr[g];
            c.n = int(h_gptr[g + 1] - h_gptr[g]);
            const int32_t want[3] = {b, key[1], key[2]};
            for (int lo = 0, hi = ng; lo < hi;) {  // the groups are ordered by their key
                const int mid = (lo + hi) >> 1;
                const int32_t* k2 = &h_gkey[size_t(mid) * 3];
                if (std::lexicographical_compare(k2, k2 + 3, want, want + 3)) {
                    lo = mid + 1;
                } else {
                    hi = mid;
                    if (std::equal(k2, k2 + 3, want)) {
                        c.bsrc = h_gptr[mid];
                        c.nb = int(h_gptr[mid + 1] - h_gptr[mid]);
                    }
                }
            }
            if (c.nb < kMinRows || c.n < kMinRows) c.flags = THR_TDMAT_CELL_TOO_FEW;
            if (dist) {  // the table's rows and columns are in the order of the caller's lists
                const int bi = index_of(beacons, n_beacons, b);
                c.dist[0] = dist[size_t(index_of(receivers, n_receivers, key[1])) * n_beacons + bi];
                c.dist[1] = dist[size_t(index_of(receivers, n_receivers, key[2])) * n_beacons + bi];
            }
            cells.push_back(c);
        }
    }
    if (cells.empty()) return empty();
    std::sort(cells.begin(), cells.end(),
              [](const Cell& a, const Cell& b) { return std::lexicographical_compare(a.key, a.key + 4, b.key, b.key + 4); });
    uint64_t total = 0;
    for (Cell& c : cells) {
        c.start = (long long)total;
        total += uint64_t(c.n);
    }
    if (total > (uint64_t(1) << 28)) return thr::fail_msg(THR_ERR_ARG, "thr_tdoamatrix: too many tasks");
    const int m = int(total), nc = int(cells.size());
    DevBuf d_cells, d_pos_cell, d_ok;
    THR_HIP_TRY(d_cells.alloc(cells.size() * sizeof(Cell)));
    THR_HIP_TRY(hipMemcpy(d_cells.p, cells.data(), cells.size() * sizeof(Cell), hipMemcpyHostToDevice));
    THR_HIP_TRY(d_pos_cell.alloc(size_t(m) * 4));
    THR_HIP_TRY(d_ok.alloc((size_t(m) + 1) * 4));
    THR_HIP_TRY(O[THR_TDMAT_CELL_KEY].alloc(size_t(nc) * 16));
    THR_HIP_TRY(O[THR_TDMAT_CELL_PTR].alloc((size_t(nc) + 1) * 8));
    THR_HIP_TRY(O[THR_TDMAT_CELL_FLAGS].alloc(size_t(nc) * 4));
    const Cell* dc = d_cells.as<Cell>();
    const int* pos_cell = d_pos_cell.as<int>();
    const long long* cell_ptr = O[THR_TDMAT_CELL_PTR].as<long long>();
    THR_TRY(launch(k_pos_cell, m, s, dc, nc, m, d_pos_cell.as<int>()));
    THR_TRY(launch(k_cell_out, nc, s, dc, nc, m, O[THR_TDMAT_CELL_KEY].as<int>(), O[THR_TDMAT_CELL_PTR].as<long long>(),
                   O[THR_TDMAT_CELL_FLAGS].as<int>()));
    THR_HIP_TRY(hipEventRecord(ev[2].e, s));

    // ---- 3. one wavefront per task
    for (int k : {THR_TDMAT_TASK_MATCH, THR_TDMAT_TIMESTAMP, THR_TDMAT_TDOA, THR_TDMAT_SNR, THR_TDMAT_MODEL_QUALITY})
        THR_HIP_TRY(O[k].alloc(size_t(m) * 8));
    for (int k : {THR_TDMAT_STATUS, THR_TDMAT_N_WINDOW, THR_TDMAT_N_KEPT}) THR_HIP_TRY(O[k].alloc(size_t(m) * 4));
    THR_HIP_TRY(O[THR_TDMAT_TASK_DET].alloc(size_t(m) * 16));
    THR_HIP_TRY(O[THR_TDMAT_OUTLIER].alloc(size_t(m)));
    THR_HIP_TRY(hipMemsetAsync(O[THR_TDMAT_OUTLIER].p, 0, size_t(m), s));
    THR_HIP_TRY(hipMemsetAsync(d_ok.p, 0, (size_t(m) + 1) * 4, s));
    Tasks T{O[THR_TDMAT_TASK_DET].as<long long>(), O[THR_TDMAT_TASK_MATCH].as<long long>(), O[THR_TDMAT_TIMESTAMP].as<double>(),
            O[THR_TDMAT_TDOA].as<double>(),        O[THR_TDMAT_SNR].as<double>(),           O[THR_TDMAT_MODEL_QUALITY].as<double>(),
            O[THR_TDMAT_STATUS].as<int>(),         O[THR_TDMAT_N_WINDOW].as<int>(),         O[THR_TDMAT_N_KEPT].as<int>(),
            d_ok.as<unsigned>()};
    const dim3 est_grid(unsigned((m + tt::kWaves - 1) / tt::kWaves));
#define LAUNCH_ESTIMATE(DEG, MODEL) THR_TRY(launch_grid(k_estimate<DEG, MODEL>, est_grid, s, dc, pos_cell, G, window, sample_rate, m, T))
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
    THR_HIP_TRY(hipEventRecord(ev[3].e, s));

    // ---- 4. the cell mask over the TDOAs, 5. the statistics over the rows it kept
    DevBuf d_incl, d_vptr, d_val, d_x, d_vcell, d_vtask, d_vmask, d_slab, d_probe, d_cv, d_cv2;
    unsigned n_val = 0;
    THR_HIP_TRY(d_incl.alloc((size_t(m) + 1) * 4));
    THR_HIP_TRY(d_vptr.alloc((size_t(nc) + 1) * 8));
    THR_HIP_TRY(O[THR_TDMAT_MEDIANS].alloc(size_t(nc) * 2 * 8));
    THR_HIP_TRY(O[THR_TDMAT_CELL_STATS].alloc(size_t(nc) * 5 * 8));
    THR_HIP_TRY(O[THR_TDMAT_CELL_COUNTS].alloc(size_t(nc) * 5 * 8));
    THR_TRY(scan(d_ok.as<unsigned>(), d_incl.as<unsigned>(), m, w, s, &n_val));
    THR_TRY(launch(k_ptr, nc + 1, s, cell_ptr, d_incl.as<unsigned>(), nc, m, d_vptr.as<long long>()));
    const int nv = int(n_val);
    Series SV;
    SV.n = nv;
    SV.nc = nc;
    double* med = O[THR_TDMAT_MEDIANS].as<double>();
    if (nv) {
        for (DevBuf* b : {&d_val, &d_x, &W.dev}) THR_HIP_TRY(b->alloc(size_t(nv) * 8));
        for (DevBuf* b : {&d_vcell, &d_vtask, &w.head, &w.incl}) THR_HIP_TRY(b->alloc(size_t(nv) * 4));
        THR_HIP_TRY(d_vmask.alloc(size_t(nv)));
        THR_HIP_TRY(d_slab.alloc(size_t(tiles_of(nv) + nc) * 5 * 8));  // no layout of nv positions has more fragments
        THR_HIP_TRY(d_probe.alloc(size_t(nc) * 8));
        THR_HIP_TRY(d_cv.alloc(size_t(nc) * 5 * 8));
        THR_HIP_TRY(d_cv2.alloc(size_t(nc) * 8));
        THR_TRY(launch(k_values, m, s, d_ok.as<unsigned>(), d_incl.as<unsigned>(), O[THR_TDMAT_TDOA].as<double>(), pos_cell, m,
                       d_val.as<double>(), d_x.as<double>(), d_vcell.as<int>(), d_vtask.as<unsigned>()));
        SV.pos_cell = d_vcell.as<int>();
        SV.ptr = d_vptr.as<long long>();
        THR_TRY(build_layout(SV.pos_cell, nv, nc, w, SV.L, s));
        const double* x = d_x.as<double>();
        const unsigned char* vmask = d_vmask.as<unsigned char>();
        THR_TRY((reduce<1, 0, 0>(LoadMax{d_val.as<double>()}, SV.L, d_slab.as<double>(), d_probe.as<double>(), s)));
        THR_TRY(outlier_mask(d_val.as<double>(), SV, d_probe.as<double>(), 1, 3.5, W, med, 2, d_vmask.as<unsigned char>(), s));
        THR_TRY(launch(k_mask_out, nv, s, vmask, d_vtask.as<unsigned>(), nv, O[THR_TDMAT_OUTLIER].as<unsigned char>()));
        THR_TRY((reduce<5, 3, 1>(LoadKept1<true>{x, vmask}, SV.L, d_slab.as<double>(), d_cv.as<double>(), s)));
        THR_TRY((reduce<1, 1, 0>(LoadKept2<true>{x, d_cv.as<double>(), vmask, SV.pos_cell}, SV.L, d_slab.as<double>(),
                                 d_cv2.as<double>(), s)));
    } else {
        THR_TRY(outlier_mask(nullptr, SV, nullptr, 1, 3.5, W, med, 2, nullptr, s));  // no TDOA at all: NaN medians
    }
    THR_TRY(launch(k_fin, nc, s, dc, d_vptr.as<long long>(), nv ? d_cv.as<double>() : nullptr, nv ? d_cv2.as<double>() : nullptr, nc,
                   O[THR_TDMAT_CELL_STATS].as<double>(), O[THR_TDMAT_CELL_COUNTS].as<long long>()));
    THR_HIP_TRY(hipEventRecord(ev[4].e, s));
    THR_TRY(record_times(ev, g_tdmat_ms));  // synchronises: the temporaries go out of scope

    B[THR_TDMAT_CELL_KEY] = size_t(nc) * 16;
    B[THR_TDMAT_CELL_PTR] = (size_t(nc) + 1) * 8;
    B[THR_TDMAT_CELL_FLAGS] = size_t(nc) * 4;
    B[THR_TDMAT_CELL_COUNTS] = B[THR_TDMAT_CELL_STATS] = size_t(nc) * 5 * 8;
    B[THR_TDMAT_MEDIANS] = size_t(nc) * 2 * 8;
    B[THR_TDMAT_TASK_DET] = size_t(m) * 16;
    B[THR_TDMAT_TASK_MATCH] = B[THR_TDMAT_TIMESTAMP] = B[THR_TDMAT_TDOA] = B[THR_TDMAT_SNR] = B[THR_TDMAT_MODEL_QUALITY] =
        size_t(m) * 8;
    B[THR_TDMAT_STATUS] = B[THR_TDMAT_N_WINDOW] = B[THR_TDMAT_N_KEPT] = size_t(m) * 4;
    B[THR_TDMAT_OUTLIER] = size_t(m);
    counts_out->tasks = size_t(m);
    counts_out->cells = size_t(nc);
    counts_out->rows = size_t(ns);
    counts_out->tdoas = size_t(nv);
    *result_out = R;
    guard.r = nullptr;
    return THR_OK;
} catch (const std::bad_alloc&) {
    return thr::fail_msg(THR_ERR_DEVICE, "thr_tdoamatrix: out of host memory");
} catch (...) {
    return thr::on_exception("thr_tdoamatrix");
}

extern "C" int thr_tdmat_fetch(thr_tdmat* R, int which, void* dst, size_t dst_bytes) try {
    return fetch("thr_tdmat_fetch", R, which, dst, dst_bytes, &g_tdmat_ms[4]);
} catch (...) {
    return thr::on_exception("thr_tdmat_fetch");
}

extern "C" void thr_tdmat_free(thr_tdmat* R) { free_result(R); }

extern "C" int thr_debug_tdoamatrix_times(double* ms_out) try {
    return copy_times("thr_debug_tdoamatrix_times", g_tdmat_ms, ms_out);
} catch (...) {
    return thr::on_exception("thr_debug_tdoamatrix_times");
}

extern "C" int thr_debug_tdoamatrix_geometry(int* tile_len, int* workgroup, int* tasks_per_workgroup) try {
    return geometry("thr_debug_tdoamatrix_geometry", tile_len, workgroup, tasks_per_workgroup, tt::kWaves);
} catch (...) {
    return thr::on_exception("thr_debug_tdoamatrix_geometry");
}
