// Position quality on the device (thr_posq): thr_pos's 2-D solve with optional row weights, every row's
// residual, the inverse normal matrix, and the exclusion of one receiver whose arrivals contradict the rest.
// The open items of the reference's pos_est.py ("use SNR or some confidence value as weight", "also return
// residual or a measure of the quality", "split DOP into multiple values").
//
// A TASK is a group solved over a subset of its rows, by the iteration of csrc/pos_lm.hpp -- the template that
// k_pos2d (pos.hip) instantiates with no weights and every row on.  Five kernels:
//   A  k_full       one 8-lane team per group: the full solve;
//   B  k_flag       one lane per group: is the group flagged (include/thrifty_hip.h states the rule), and how many
//                   candidates does it get -- one per receiver it names.  An exclusive scan (hipCUB) of the counts
//                   is the candidates' CSR pointer; its last entry is read back;
//   C  k_expand     one lane per group: the candidates' (group, receiver), receivers ascending by dense index;
//   D  k_cand       one team per candidate: the group without the rows that name the receiver, from x0 again
//                   (DESIGN.md 3.17 says why not from the full solution);
//   E  k_choose     one lane per group: eligibility, the best candidate, the ratio test, the chosen task's
//                   numbers, and every row's residual at the chosen position.
// Nothing is accumulated across teams, no atomic: a repeated call returns the same bits.  All launches go to the
// null stream; temporaries are freed by hipFree, which waits for it.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>

#include "../../include/thrifty_hip.h"
#include "lmdif8.hpp"
#include "pos_lm.hpp"
#include "post_stages.hpp"
#include "seg_cells.hpp"

// the team's lanes must agree bit for bit, and an all-ones weight column must give the unweighted bits: no
// a * b + c may become an fma in this file (the build also passes -ffp-contract=off for it, thrifty_amd/build.py)
#pragma clang fp contract(off)

namespace {

using thr::DevBuf;
using thr::Event;
using namespace thr::poslm;
using thr::seg::launch;
using thr::seg::launch_grid;

constexpr int kBlock = thr::seg::kBlock;  // workgroup size (launch() assumes it)
constexpr int kTeams = kBlock / kTeam;     // tasks per workgroup
constexpr int kRegRows = 4;                // rows per lane kept in registers, as k_pos2d
constexpr int kMaxReceivers = 64;          // the receivers of a group are a 64-bit mask
static_assert(THR_POSQ_N_OUTPUTS <= thr::seg::kMaxOutputs, "the result handle holds every output");

struct Cols {  // the input columns on the device
    const long long* ptr;
    const int *rx0, *rx1;
    const double *tdoa, *snr, *weight, *xy;
};
struct Solved {  // what a solve leaves per task
    double *pos, *dop, *q, *rms;
    int *status, *iters, *nrx, *mused;
};

__device__ __forceinline__ void store_fit(const Fit& fit, int t, const Solved& o) {
    const Sums& c = fit.cur;
    const double det = c.a00 * c.a11 - c.a01 * c.a01;
    const bool bad = det == 0.0 || !isfinite(det);
    o.pos[2 * size_t(t)] = fit.p0;
    o.pos[2 * size_t(t) + 1] = fit.p1;
    o.dop[t] = dop_of(c);
    o.q[3 * size_t(t)] = bad ? NAN : c.a11 / det;
    o.q[3 * size_t(t) + 1] = bad ? NAN : -c.a01 / det;
    o.q[3 * size_t(t) + 2] = bad ? NAN : c.a00 / det;
    o.rms[t] = sqrt(c.F / double(fit.m_used));
    o.status[t] = fit.status;
    o.iters[t] = fit.iters;
    o.nrx[t] = fit.n_distinct;
    o.mused[t] = fit.m_used;
}

// A: group g = one team, every row on
template <bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void k_full(Cols c, int n_groups, double x0, double y0, Box box, int max_iter, Solved o,
                                                 double* __restrict__ snr_out, unsigned long long* __restrict__ mask_out) {
    const int team = (blockIdx.x * kBlock + threadIdx.x) / kTeam, j = threadIdx.x & (kTeam - 1);
    const bool live = team < n_groups;
    const long long beg = live ? c.ptr[team] : 0;
    const int m = live ? int(c.ptr[team + 1] - beg) : 0;
    const Fit fit = solve_team<WEIGHTED, kRegRows>(live, beg, m, j, c.rx0, c.rx1, c.tdoa, c.snr, c.weight, c.xy, x0, y0, box,
                                                   max_iter, AllRows{});
    if (live && j == 0) {
        store_fit(fit, team, o);
        snr_out[team] = fit.snr_mean;
        mask_out[team] = fit.mask;
    }
}

// B: count[g] = candidates of group g (0 when it is not flagged); count[n_groups] = 0, so that the exclusive scan
// over n_groups + 1 entries is the CSR pointer with its terminator
__global__ __launch_bounds__(kBlock) void k_flag(const int* __restrict__ status, const int* __restrict__ nrx,
                                                 const double* __restrict__ rms, int n_groups, double gate_m, int min_rx,
                                                 long long* __restrict__ count, unsigned* __restrict__ flagged) {
    const int g = blockIdx.x * kBlock + threadIdx.x;
    if (g > n_groups) return;
    if (g == n_groups) {
        count[g] = 0;
        return;
    }
    const bool f = gate_m > 0.0 && status[g] != kUnderdetermined && status[g] != kNonfinite && nrx[g] >= min_rx &&
                   rms[g] > gate_m;  // a NaN rms does not flag
    count[g] = f ? nrx[g] : 0;
    flagged[g] = f ? 1u : 0u;
}

// C: the candidates of group g, one per set bit of its receivers' mask, ascending
__global__ __launch_bounds__(kBlock) void k_expand(const long long* __restrict__ task_ptr,
                                                   const unsigned long long* __restrict__ mask, int n_groups,
                                                   int* __restrict__ task_group, int* __restrict__ task_rx) {
    const int g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= n_groups) return;
    long long t = task_ptr[g];
    const long long end = task_ptr[g + 1];
    unsigned long long left = mask[g];
    for (int r = 0; r < kMaxReceivers && t < end; ++r)
        if ((left >> r) & 1ull) {
            task_group[t] = g;
            task_rx[t] = r;
            ++t;
        }
}

// D: candidate t = one team: its group without the rows that name task_rx[t]
template <bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void k_cand(Cols c, const int* __restrict__ task_group, const int* __restrict__ task_rx,
                                                 int n_tasks, double x0, double y0, Box box, int max_iter, Solved o) {
    const int team = (blockIdx.x * kBlock + threadIdx.x) / kTeam, j = threadIdx.x & (kTeam - 1);
    const bool live = team < n_tasks;
    const int g = live ? task_group[team] : 0, ex = live ? task_rx[team] : -1;
    const long long beg = live ? c.ptr[g] : 0;
    const int m = live ? int(c.ptr[g + 1] - beg) : 0;
    const Fit fit = solve_team<WEIGHTED, kRegRows>(live, beg, m, j, c.rx0, c.rx1, c.tdoa, c.snr, c.weight, c.xy, x0, y0, box,
                                                   max_iter, NotReceiver{c.rx0, c.rx1, ex});
    if (live && j == 0) store_fit(fit, team, o);
}

struct Chosen {  // the per-group outputs
    double *pos, *dop, *q, *rms;
    int *status, *iters, *counts, *flags;
    double* residual;
    unsigned char* used;
};

// E: one lane per group
__global__ __launch_bounds__(kBlock) void k_choose(Cols c, int n_groups, Solved full, const unsigned* __restrict__ flagged,
                                                   const long long* __restrict__ task_ptr, const int* __restrict__ task_rx,
                                                   Solved cand, double ratio, int min_rx, Chosen o) {
    const int g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= n_groups) return;
    const double rms_full = full.rms[g];
    int flags = 0, excluded = -1;
    long long best = -1;
    if (flagged && flagged[g]) {
        flags = THR_POSQ_INCONSISTENT;
        for (long long t = task_ptr[g]; t < task_ptr[g + 1]; ++t)  // ascending receivers: a tie keeps the lower one
            if (cand.status[t] == kOk && cand.nrx[t] >= min_rx - 1 && (best < 0 || cand.rms[t] < cand.rms[best])) best = t;
        if (best >= 0 && cand.rms[best] <= ratio * rms_full) {
            flags |= THR_POSQ_EXCLUDED;
            excluded = task_rx[best];
        } else {
            flags |= THR_POSQ_NO_CANDIDATE;
            best = -1;
        }
    }
    const Solved& from = best >= 0 ? cand : full;
    const size_t t = best >= 0 ? size_t(best) : size_t(g);
    const double p0 = from.pos[2 * t], p1 = from.pos[2 * t + 1];
    o.pos[2 * size_t(g)] = p0;
    o.pos[2 * size_t(g) + 1] = p1;
    o.dop[g] = from.dop[t];
    for (int k = 0; k < 3; ++k) o.q[3 * size_t(g) + k] = from.q[3 * t + k];
    o.rms[2 * size_t(g)] = rms_full;
    o.rms[2 * size_t(g) + 1] = from.rms[t];
    o.status[g] = from.status[t];
    o.iters[g] = from.iters[t];
    o.counts[3 * size_t(g)] = from.nrx[t];
    o.counts[3 * size_t(g) + 1] = from.mused[t];
    o.counts[3 * size_t(g) + 2] = excluded;
    o.flags[g] = flags;
    for (long long i = c.ptr[g]; i < c.ptr[g + 1]; ++i) {
        o.residual[i] = residual(load_row(c.rx0, c.rx1, c.tdoa, c.xy, i), p0, p1);
        o.used[i] = (c.rx0[i] != excluded && c.rx1[i] != excluded) ? 1 : 0;
    }
}

thread_local double g_posq_ms[6] = {0, 0, 0, 0, 0, 0};

}  // namespace

struct thr_posq_result : thr::seg::Result {};

extern "C" int thr_posq(int device_id, size_t n_groups, const int64_t* group_ptr, const int32_t* row_rx0,
                        const int32_t* row_rx1, const double* row_tdoa, const double* row_snr, const double* row_weight,
                        int n_rx, int dims, const double* rx_coords, const thr_posq_opts* opts, thr_posq_result** result_out,
                        thr_posq_counts* counts_out) try {
    if (result_out) *result_out = nullptr;
    if (counts_out) std::memset(counts_out, 0, sizeof(*counts_out));
    for (double& t : g_posq_ms) t = 0;
    if (!result_out || !counts_out || !opts || !group_ptr || !rx_coords) return thr::fail_msg(THR_ERR_ARG, "thr_posq: null argument");
    if (dims != 2) return thr::fail_msg(THR_ERR_ARG, "thr_posq: 2 dimensions, not %d", dims);
    if (n_rx < 1 || n_rx > kMaxReceivers) return thr::fail_msg(THR_ERR_ARG, "thr_posq: 1 to %d receivers, not %d", kMaxReceivers, n_rx);
    if (opts->max_iter < 0) return thr::fail_msg(THR_ERR_ARG, "thr_posq: max_iter must not be negative");
    if (!(opts->gate_m >= 0.0) || !std::isfinite(opts->gate_m))
        return thr::fail_msg(THR_ERR_ARG, "thr_posq: gate_m must be finite and not negative (0: no exclusion)");
    if (!(opts->ratio > 0.0 && opts->ratio <= 1.0)) return thr::fail_msg(THR_ERR_ARG, "thr_posq: ratio must lie in (0, 1]");
    if (opts->min_rx < 5 || opts->min_rx > kMaxReceivers)
        return thr::fail_msg(THR_ERR_ARG, "thr_posq: min_rx must lie in 5 .. %d, not %d", kMaxReceivers, opts->min_rx);
    if (n_groups > size_t(1) << 28) return thr::fail_msg(THR_ERR_ARG, "thr_posq: too many groups");

    // ---- everything a kernel will index with is checked here, before anything is launched
    if (group_ptr[0] != 0) return thr::fail_msg(THR_ERR_ARG, "thr_posq: group_ptr[0] must be 0");
    for (size_t g = 0; g < n_groups; ++g) {
        const int64_t len = group_ptr[g + 1] - group_ptr[g];
        if (len < 0) return thr::fail_msg(THR_ERR_ARG, "thr_posq: group_ptr decreases at group %zu", g);
        if (len > (int64_t(1) << 24)) return thr::fail_msg(THR_ERR_ARG, "thr_posq: group %zu is too long", g);
    }
    const size_t n_rows = size_t(group_ptr[n_groups]);
    if (n_rows > size_t(1) << 30) return thr::fail_msg(THR_ERR_ARG, "thr_posq: too many rows");
    if (n_rows && (!row_rx0 || !row_rx1 || !row_tdoa || !row_snr)) return thr::fail_msg(THR_ERR_ARG, "thr_posq: null argument");
    for (size_t i = 0; i < n_rows; ++i)
        if (row_rx0[i] < 0 || row_rx0[i] >= n_rx || row_rx1[i] < 0 || row_rx1[i] >= n_rx)
            return thr::fail_msg(THR_ERR_ARG, "thr_posq: row %zu names receivers %d and %d of %d", i, row_rx0[i], row_rx1[i], n_rx);
    if (row_weight)
        for (size_t i = 0; i < n_rows; ++i)
            if (!(row_weight[i] >= 0.0) || !std::isfinite(row_weight[i]))
                return thr::fail_msg(THR_ERR_ARG, "thr_posq: row %zu has a weight that is negative or not finite", i);
    thr::PosPlan plan;
    THR_TRY(thr::pos_plan("thr_posq", n_rx, dims, rx_coords, nullptr, opts->x0, plan));
    const Box box{plan.lo[0], plan.lo[1], plan.hi[0], plan.hi[1]};
    const double x0 = plan.start[0], y0 = plan.start[1];

    THR_TRY(thr::seg::pick_device(device_id));
    thr_posq_result* R = new thr_posq_result;
    thr::seg::ResultGuard guard{R};
    R->device = device_id;
    R->n_out = THR_POSQ_N_OUTPUTS;
    hipStream_t s = nullptr;
    Event ev[6];
    for (Event& e : ev) THR_HIP_TRY(e.create());
    for (Event& e : R->ev) THR_HIP_TRY(e.create());
    const int ng = int(n_groups);
    const bool weighted = row_weight != nullptr;

    // ---- copies in
    DevBuf d_ptr, d_rx0, d_rx1, d_tdoa, d_snr, d_w, d_xy;
    THR_HIP_TRY(d_ptr.alloc((n_groups + 1) * 8));
    THR_HIP_TRY(d_rx0.alloc(n_rows * 4));
    THR_HIP_TRY(d_rx1.alloc(n_rows * 4));
    THR_HIP_TRY(d_tdoa.alloc(n_rows * 8));
    THR_HIP_TRY(d_snr.alloc(n_rows * 8));
    if (weighted) THR_HIP_TRY(d_w.alloc(n_rows * 8));
    THR_HIP_TRY(d_xy.alloc(size_t(n_rx) * 16));
    THR_HIP_TRY(hipEventRecord(ev[0].e, s));
    THR_HIP_TRY(hipMemcpy(d_ptr.p, group_ptr, (n_groups + 1) * 8, hipMemcpyHostToDevice));
    if (n_rows) {
        THR_HIP_TRY(hipMemcpy(d_rx0.p, row_rx0, n_rows * 4, hipMemcpyHostToDevice));
        THR_HIP_TRY(hipMemcpy(d_rx1.p, row_rx1, n_rows * 4, hipMemcpyHostToDevice));
        THR_HIP_TRY(hipMemcpy(d_tdoa.p, row_tdoa, n_rows * 8, hipMemcpyHostToDevice));
        THR_HIP_TRY(hipMemcpy(d_snr.p, row_snr, n_rows * 8, hipMemcpyHostToDevice));
        if (weighted) THR_HIP_TRY(hipMemcpy(d_w.p, row_weight, n_rows * 8, hipMemcpyHostToDevice));
    }
    THR_HIP_TRY(hipMemcpy(d_xy.p, rx_coords, size_t(n_rx) * 16, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipEventRecord(ev[1].e, s));
    const Cols C{d_ptr.as<long long>(), d_rx0.as<int>(),  d_rx1.as<int>(), d_tdoa.as<double>(),
                 d_snr.as<double>(),    d_w.as<double>(), d_xy.as<double>()};
    DevBuf* O = R->out;

    // ---- A: the full solves
    DevBuf f_dop, f_q, f_rms, f_iters, f_nrx, f_mused, d_mask;
    THR_HIP_TRY(O[THR_POSQ_FULL_POS].alloc(n_groups * 16));
    THR_HIP_TRY(f_dop.alloc(n_groups * 8));
    THR_HIP_TRY(f_q.alloc(n_groups * 24));
    THR_HIP_TRY(f_rms.alloc(n_groups * 8));
    for (DevBuf* b : {&O[THR_POSQ_FULL_STATUS], &f_iters, &f_nrx, &f_mused}) THR_HIP_TRY(b->alloc(n_groups * 4));
    const Solved full{O[THR_POSQ_FULL_POS].as<double>(), f_dop.as<double>(),               f_q.as<double>(),
                      f_rms.as<double>(),                O[THR_POSQ_FULL_STATUS].as<int>(), f_iters.as<int>(),
                      f_nrx.as<int>(),                   f_mused.as<int>()};
    THR_HIP_TRY(d_mask.alloc(n_groups * 8));
    THR_HIP_TRY(O[THR_POSQ_SNR].alloc(n_groups * 8));
    const dim3 team_grid_full(unsigned((n_groups + kTeams - 1) / kTeams));
    if (ng)
        THR_TRY(weighted ? launch_grid(k_full<true>, team_grid_full, s, C, ng, x0, y0, box, opts->max_iter, full,
                                       O[THR_POSQ_SNR].as<double>(), d_mask.as<unsigned long long>())
                         : launch_grid(k_full<false>, team_grid_full, s, C, ng, x0, y0, box, opts->max_iter, full,
                                       O[THR_POSQ_SNR].as<double>(), d_mask.as<unsigned long long>()));
    THR_HIP_TRY(hipEventRecord(ev[2].e, s));

    // ---- B, C: flags, the candidates' pointer, the candidates
    DevBuf d_count, d_flagged, d_nflag, d_tgroup, d_tmp;
    size_t tmp_bytes = 0;
    long long n_tasks = 0;
    unsigned n_flagged = 0;
    const bool gated = opts->gate_m > 0.0 && ng > 0;
    THR_HIP_TRY(O[THR_POSQ_TASK_PTR].alloc((n_groups + 1) * 8));
    if (gated) {
        THR_HIP_TRY(d_count.alloc((n_groups + 1) * 8));
        THR_HIP_TRY(d_flagged.alloc(n_groups * 4));
        THR_HIP_TRY(d_nflag.alloc(4));
        THR_TRY(launch(k_flag, n_groups + 1, s, full.status, full.nrx, full.rms, ng, opts->gate_m,
                       int(opts->min_rx), d_count.as<long long>(), d_flagged.as<unsigned>()));
        THR_HIP_TRY(thr::with_temp(d_tmp, tmp_bytes, [&](void* t, size_t& b) {
            return hipcub::DeviceScan::ExclusiveSum(t, b, d_count.as<long long>(), O[THR_POSQ_TASK_PTR].as<long long>(), ng + 1, s);
        }));
        THR_HIP_TRY(thr::with_temp(d_tmp, tmp_bytes, [&](void* t, size_t& b) {
            return hipcub::DeviceReduce::Sum(t, b, d_flagged.as<unsigned>(), d_nflag.as<unsigned>(), ng, s);
        }));
        THR_HIP_TRY(hipMemcpy(&n_tasks, O[THR_POSQ_TASK_PTR].as<long long>() + ng, 8, hipMemcpyDeviceToHost));  // synchronises
        THR_HIP_TRY(hipMemcpy(&n_flagged, d_nflag.p, 4, hipMemcpyDeviceToHost));
        if (n_tasks < 0 || n_tasks > (1ll << 28)) return thr::fail_msg(THR_ERR_ARG, "thr_posq: too many candidates");
    } else {
        THR_HIP_TRY(hipMemsetAsync(O[THR_POSQ_TASK_PTR].p, 0, (n_groups + 1) * 8, s));
    }
    const size_t nt = size_t(n_tasks);
    THR_HIP_TRY(d_tgroup.alloc(nt * 4));
    THR_HIP_TRY(O[THR_POSQ_TASK_RX].alloc(nt * 4));
    if (nt)
        THR_TRY(launch(k_expand, n_groups, s, O[THR_POSQ_TASK_PTR].as<long long>(), d_mask.as<unsigned long long>(), ng,
                       d_tgroup.as<int>(), O[THR_POSQ_TASK_RX].as<int>()));
    THR_HIP_TRY(hipEventRecord(ev[3].e, s));

    // ---- D: the candidates
    DevBuf c_dop, c_q, c_mused;
    THR_HIP_TRY(O[THR_POSQ_TASK_POS].alloc(nt * 16));
    THR_HIP_TRY(O[THR_POSQ_TASK_RMS].alloc(nt * 8));
    THR_HIP_TRY(c_dop.alloc(nt * 8));
    THR_HIP_TRY(c_q.alloc(nt * 24));
    for (DevBuf* b : {&O[THR_POSQ_TASK_STATUS], &O[THR_POSQ_TASK_ITERS], &O[THR_POSQ_TASK_NRX], &c_mused}) THR_HIP_TRY(b->alloc(nt * 4));
    const Solved cand{O[THR_POSQ_TASK_POS].as<double>(), c_dop.as<double>(),           c_q.as<double>(),
                      O[THR_POSQ_TASK_RMS].as<double>(), O[THR_POSQ_TASK_STATUS].as<int>(), O[THR_POSQ_TASK_ITERS].as<int>(),
                      O[THR_POSQ_TASK_NRX].as<int>(),    c_mused.as<int>()};
    if (nt) {
        const dim3 grid(unsigned((nt + kTeams - 1) / kTeams));
        THR_TRY(weighted ? launch_grid(k_cand<true>, grid, s, C, d_tgroup.as<int>(), O[THR_POSQ_TASK_RX].as<int>(), int(nt), x0, y0,
                                       box, opts->max_iter, cand)
                         : launch_grid(k_cand<false>, grid, s, C, d_tgroup.as<int>(), O[THR_POSQ_TASK_RX].as<int>(), int(nt), x0, y0,
                                       box, opts->max_iter, cand));
    }
    THR_HIP_TRY(hipEventRecord(ev[4].e, s));

    // ---- E: the choice and the residuals
    THR_HIP_TRY(O[THR_POSQ_POS].alloc(n_groups * 16));
    THR_HIP_TRY(O[THR_POSQ_DOP].alloc(n_groups * 8));
    THR_HIP_TRY(O[THR_POSQ_Q].alloc(n_groups * 24));
    THR_HIP_TRY(O[THR_POSQ_RMS].alloc(n_groups * 16));
    THR_HIP_TRY(O[THR_POSQ_COUNTS].alloc(n_groups * 12));
    for (DevBuf* b : {&O[THR_POSQ_STATUS], &O[THR_POSQ_ITERS], &O[THR_POSQ_FLAGS]}) THR_HIP_TRY(b->alloc(n_groups * 4));
    THR_HIP_TRY(O[THR_POSQ_RESIDUAL].alloc(n_rows * 8));
    THR_HIP_TRY(O[THR_POSQ_USED].alloc(n_rows));
    const Chosen chosen{O[THR_POSQ_POS].as<double>(),    O[THR_POSQ_DOP].as<double>(),          O[THR_POSQ_Q].as<double>(),
                        O[THR_POSQ_RMS].as<double>(),    O[THR_POSQ_STATUS].as<int>(),          O[THR_POSQ_ITERS].as<int>(),
                        O[THR_POSQ_COUNTS].as<int>(),    O[THR_POSQ_FLAGS].as<int>(),           O[THR_POSQ_RESIDUAL].as<double>(),
                        O[THR_POSQ_USED].as<unsigned char>()};
    THR_TRY(launch(k_choose, n_groups, s, C, ng, full, gated ? d_flagged.as<unsigned>() : nullptr,
                   O[THR_POSQ_TASK_PTR].as<long long>(), O[THR_POSQ_TASK_RX].as<int>(), cand, opts->ratio, int(opts->min_rx), chosen));
    THR_HIP_TRY(hipEventRecord(ev[5].e, s));
    THR_HIP_TRY(hipEventSynchronize(ev[5].e));  // the temporaries go out of scope
    for (int k = 0; k < 5; ++k) {
        float ms = 0;
        THR_HIP_TRY(hipEventElapsedTime(&ms, ev[k].e, ev[k + 1].e));
        g_posq_ms[k] = ms;
    }

    size_t* B = R->bytes;
    B[THR_POSQ_POS] = B[THR_POSQ_RMS] = B[THR_POSQ_FULL_POS] = n_groups * 16;
    B[THR_POSQ_DOP] = B[THR_POSQ_SNR] = n_groups * 8;
    B[THR_POSQ_STATUS] = B[THR_POSQ_ITERS] = B[THR_POSQ_FLAGS] = B[THR_POSQ_FULL_STATUS] = n_groups * 4;
    B[THR_POSQ_Q] = n_groups * 24;
    B[THR_POSQ_COUNTS] = n_groups * 12;
    B[THR_POSQ_RESIDUAL] = n_rows * 8;
    B[THR_POSQ_USED] = n_rows;
    B[THR_POSQ_TASK_PTR] = (n_groups + 1) * 8;
    B[THR_POSQ_TASK_RX] = B[THR_POSQ_TASK_STATUS] = B[THR_POSQ_TASK_NRX] = B[THR_POSQ_TASK_ITERS] = nt * 4;
    B[THR_POSQ_TASK_POS] = nt * 16;
    B[THR_POSQ_TASK_RMS] = nt * 8;
    counts_out->groups = n_groups;
    counts_out->rows = n_rows;
    counts_out->flagged = n_flagged;
    counts_out->tasks = nt;
    *result_out = R;
    guard.r = nullptr;
    return THR_OK;
} catch (const std::bad_alloc&) {
    return thr::fail_msg(THR_ERR_DEVICE, "thr_posq: out of host memory");
} catch (...) {
    return thr::on_exception("thr_posq");
}

extern "C" int thr_posq_fetch(thr_posq_result* R, int which, void* dst, size_t dst_bytes) try {
    return thr::seg::fetch("thr_posq_fetch", R, which, dst, dst_bytes, &g_posq_ms[5]);
} catch (...) {
    return thr::on_exception("thr_posq_fetch");
}

extern "C" void thr_posq_free(thr_posq_result* R) { thr::seg::free_result(R); }

extern "C" int thr_debug_posq_times(double* ms_out) try {
    if (!ms_out) return thr::fail_msg(THR_ERR_ARG, "thr_debug_posq_times: null argument");
    for (int k = 0; k < 6; ++k) ms_out[k] = g_posq_ms[k];
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_posq_times");
}
