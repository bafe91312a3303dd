// Position quality for receivers with three coordinates (thr_posq3): thr_pos3's solve in its two modes with
// optional row weights, every row's residual, the inverse normal matrix, and the exclusion of one receiver whose
// arrivals contradict the rest -- thr_posq's stages, word for word, on csrc/pos3_lm.hpp's iteration.
//
// A TASK is a group solved over a subset of its rows.  Five kernels, as posq.hip:
//   A  k_full       one 8-lane team per group: the full solve;
//   B  k_flag       one lane per group: is the group flagged (include/thrifty_hip.h states the rule), and how many
//                   candidates does it get -- one per receiver it names.  An exclusive scan (hipCUB) of the counts
//                   is the candidates' CSR pointer; its last entry is read back;
//   C  k_expand     one lane per group: the candidates' (group, receiver), receivers ascending by dense index;
//   D  k_cand       one team per candidate: the group without the rows that name the receiver, from x0 again;
//   E  k_choose     one lane per group: eligibility, the best candidate, the ratio test, the chosen task's
//                   numbers, and every row's residual (the 3-D norm) at the chosen position.
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
#include "pos3_lm.hpp"
#include "post_stages.hpp"
#include "seg_cells.hpp"

// the team's lanes must agree bit for bit, an all-ones weight column must give the unweighted bits, and the
// known-height mode on a flat table thr_posq's: no a * b + c may become an fma in this file (the build also passes
// -ffp-contract=off for it, thrifty_amd/build.py)
#pragma clang fp contract(off)

namespace {

using thr::DevBuf;
using thr::Event;
using namespace thr::pos3lm;
using thr::poslm::AllRows;
using thr::poslm::NotReceiver;
using thr::seg::launch;
using thr::seg::launch_grid;

constexpr int kBlock = thr::seg::kBlock;  // workgroup size (launch() assumes it)
constexpr int kTeams = kBlock / kTeam;     // tasks per workgroup
constexpr int kRegRows = 4;                // rows per lane kept in registers, as thr_pos3
constexpr int kMaxReceivers = 64;          // the receivers of a group are a 64-bit mask
constexpr double kMaxDist = 10e3;          // the reference's MAX_DIST (pos_est.py:24), as thr_pos3
constexpr int kMinRxKnownHeight = 5;       // one of five receivers left out leaves four: one redundant arrival for (x, y)
constexpr int kMinRxFreeZ = 6;             // one of six left out leaves five: one redundant arrival for (x, y, z)
static_assert(THR_POSQ3_N_OUTPUTS <= thr::seg::kMaxOutputs, "the result handle holds every output");

struct Cols {  // the input columns on the device
    const long long* ptr;
    const int *rx0, *rx1;
    const double *tdoa, *snr, *weight, *xyz, *group_h;
};
struct Solved {  // what a solve leaves per task
    double *pos, *dop, *hdop, *vdop, *q, *rms;
    int *status, *iters, *nrx, *mused;
};

template <bool FREE_Z>
__device__ __forceinline__ void store_fit(const Fit& fit, size_t t, const Solved& o) {
    const Sums& c = fit.cur;
    o.pos[3 * t] = fit.p0;
    o.pos[3 * t + 1] = fit.p1;
    o.pos[3 * t + 2] = fit.p2;
    double* q = o.q + 6 * t;
    if (FREE_Z) {  // inv(A) by the cofactors of dop3_of
        const double c00 = c.a11 * c.a22 - c.a12 * c.a12, c01 = c.a02 * c.a12 - c.a01 * c.a22, c02 = c.a01 * c.a12 - c.a02 * c.a11;
        const double c11 = c.a00 * c.a22 - c.a02 * c.a02, c12 = c.a01 * c.a02 - c.a00 * c.a12, c22 = c.a00 * c.a11 - c.a01 * c.a01;
        const double det = (c.a00 * c00 + c.a01 * c01) + c.a02 * c02;
        const bool bad = det == 0.0 || !isfinite(det);
        q[0] = bad ? NAN : c00 / det;
        q[1] = bad ? NAN : c01 / det;
        q[2] = bad ? NAN : c11 / det;
        q[3] = bad ? NAN : c02 / det;
        q[4] = bad ? NAN : c12 / det;
        q[5] = bad ? NAN : c22 / det;
        double dop, hdop, vdop;
        dop3_of(c, dop, hdop, vdop);
        o.dop[t] = dop;
        o.hdop[t] = hdop;
        o.vdop[t] = vdop;
    } else {  // pos_lm.hpp's 2 x 2 inverse (posq.hip's expressions); the height is given
        const double det = c.a00 * c.a11 - c.a01 * c.a01;
        const bool bad = det == 0.0 || !isfinite(det);
        q[0] = bad ? NAN : c.a11 / det;
        q[1] = bad ? NAN : -c.a01 / det;
        q[2] = bad ? NAN : c.a00 / det;
        q[3] = q[4] = q[5] = 0.0;
        const double dop = dop2_of(c);
        o.dop[t] = dop;
        o.hdop[t] = dop;
        o.vdop[t] = 0.0;
    }
    o.rms[t] = sqrt(c.F / double(fit.m_used));
    o.status[t] = fit.status;
    o.iters[t] = fit.iters;
    o.nrx[t] = fit.n_distinct;
    o.mused[t] = fit.m_used;
}

// A: group g = one team, every row on
template <bool FREE_Z, bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void k_full(Cols c, int n_groups, double x0, double y0, double z0, Box box, int max_iter,
                                                 Solved o, double* __restrict__ snr_out,
                                                 unsigned long long* __restrict__ mask_out) {
    const int team = (blockIdx.x * kBlock + threadIdx.x) / kTeam, j = threadIdx.x & (kTeam - 1);
    const bool live = team < n_groups;
    const long long beg = live ? c.ptr[team] : 0;
    const int m = live ? int(c.ptr[team + 1] - beg) : 0;
    const double h = (!FREE_Z && live) ? c.group_h[team] : 0.0;
    const Fit fit = solve_team<FREE_Z, kRegRows, WEIGHTED, AllRows>(live, beg, m, j, c.rx0, c.rx1, c.tdoa, c.snr, c.xyz, h, x0, y0,
                                                                    z0, box, max_iter, c.weight, AllRows{});
    if (live && j == 0) {
        store_fit<FREE_Z>(fit, size_t(team), o);
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
    const unsigned long long left = mask[g];
    for (int r = 0; r < kMaxReceivers && t < end; ++r)
        if ((left >> r) & 1ull) {
            task_group[t] = g;
            task_rx[t] = r;
            ++t;
        }
}

// D: candidate t = one team: its group without the rows that name task_rx[t]
template <bool FREE_Z, bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void k_cand(Cols c, const int* __restrict__ task_group, const int* __restrict__ task_rx,
                                                 int n_tasks, double x0, double y0, double z0, Box box, int max_iter, Solved o) {
    const int team = (blockIdx.x * kBlock + threadIdx.x) / kTeam, j = threadIdx.x & (kTeam - 1);
    const bool live = team < n_tasks;
    const int g = live ? task_group[team] : 0, ex = live ? task_rx[team] : -1;
    const long long beg = live ? c.ptr[g] : 0;
    const int m = live ? int(c.ptr[g + 1] - beg) : 0;
    const double h = (!FREE_Z && live) ? c.group_h[g] : 0.0;
    const Fit fit = solve_team<FREE_Z, kRegRows, WEIGHTED, NotReceiver>(live, beg, m, j, c.rx0, c.rx1, c.tdoa, c.snr, c.xyz, h, x0,
                                                                        y0, z0, box, max_iter, c.weight,
                                                                        NotReceiver{c.rx0, c.rx1, ex});
    if (live && j == 0) store_fit<FREE_Z>(fit, size_t(team), o);
}

struct Chosen {  // the per-group outputs
    double *pos, *dop, *hdop, *vdop, *q, *rms;
    int *status, *iters, *counts, *flags;
    double* residual;
    unsigned char* used;
};

// E: one lane per group
template <bool FREE_Z>
__global__ __launch_bounds__(kBlock) void k_choose(Cols c, int n_groups, Solved full, const unsigned* __restrict__ flagged,
                                                   const long long* __restrict__ task_ptr, const int* __restrict__ task_rx,
                                                   Solved cand, double ratio, int min_rx, Chosen o) {
    const int g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= n_groups) return;
    const double rms_full = full.rms[g];
    int flags = 0, excluded = -1;
    long long best = -1;
    if (flagged && flagged[g]) {
        flags = THR_POSQ3_INCONSISTENT;
        for (long long t = task_ptr[g]; t < task_ptr[g + 1]; ++t)  // ascending receivers: a tie keeps the lower one
            if (cand.status[t] == kOk && cand.nrx[t] >= min_rx - 1 && (best < 0 || cand.rms[t] < cand.rms[best])) best = t;
        if (best >= 0 && cand.rms[best] <= ratio * rms_full) {
            flags |= THR_POSQ3_EXCLUDED;
            excluded = task_rx[best];
        } else {
            flags |= THR_POSQ3_NO_CANDIDATE;
            best = -1;
        }
    }
    const Solved& from = best >= 0 ? cand : full;
    const size_t t = best >= 0 ? size_t(best) : size_t(g);
    const double p0 = from.pos[3 * t], p1 = from.pos[3 * t + 1], p2 = from.pos[3 * t + 2];
    o.pos[3 * size_t(g)] = p0;
    o.pos[3 * size_t(g) + 1] = p1;
    o.pos[3 * size_t(g) + 2] = p2;
    o.dop[g] = from.dop[t];
    o.hdop[g] = from.hdop[t];
    o.vdop[g] = from.vdop[t];
    for (int k = 0; k < 6; ++k) o.q[6 * size_t(g) + k] = from.q[6 * t + k];
    o.rms[2 * size_t(g)] = rms_full;
    o.rms[2 * size_t(g) + 1] = from.rms[t];
    o.status[g] = from.status[t];
    o.iters[g] = from.iters[t];
    o.counts[3 * size_t(g)] = from.nrx[t];
    o.counts[3 * size_t(g) + 1] = from.mused[t];
    o.counts[3 * size_t(g) + 2] = excluded;
    o.flags[g] = flags;
    const double h = FREE_Z ? 0.0 : c.group_h[g];  // known height: p2 is h, and a row holds rz - h
    for (long long i = c.ptr[g]; i < c.ptr[g + 1]; ++i) {
        o.residual[i] = residual<FREE_Z>(load_row(c.rx0, c.rx1, c.tdoa, c.xyz, h, i), p0, p1, p2);
        o.used[i] = (c.rx0[i] != excluded && c.rx1[i] != excluded) ? 1 : 0;
    }
}

thread_local double g_posq3_ms[6] = {0, 0, 0, 0, 0, 0};

}  // namespace

struct thr_posq3_result : thr::seg::Result {};

extern "C" int thr_posq3(int device_id, size_t n_groups, const int64_t* group_ptr, const int32_t* row_rx0,
                         const int32_t* row_rx1, const double* row_tdoa, const double* row_snr, const double* row_weight,
                         int n_rx, const double* rx_xyz, int mode, const double* group_h, const thr_posq3_opts* opts,
                         thr_posq3_result** result_out, thr_posq3_counts* counts_out) try {
    if (result_out) *result_out = nullptr;
    if (counts_out) std::memset(counts_out, 0, sizeof(*counts_out));
    for (double& t : g_posq3_ms) t = 0;
    if (!result_out || !counts_out || !opts || !group_ptr || !rx_xyz) return thr::fail_msg(THR_ERR_ARG, "thr_posq3: null argument");
    if (mode != THR_POS3_KNOWN_HEIGHT && mode != THR_POS3_FREE_Z)
        return thr::fail_msg(THR_ERR_ARG, "thr_posq3: mode must be THR_POS3_KNOWN_HEIGHT or THR_POS3_FREE_Z, not %d", mode);
    const bool free_z = mode == THR_POS3_FREE_Z;
    if (n_rx < 1 || n_rx > kMaxReceivers) return thr::fail_msg(THR_ERR_ARG, "thr_posq3: 1 to %d receivers, not %d", kMaxReceivers, n_rx);
    if (opts->max_iter < 0) return thr::fail_msg(THR_ERR_ARG, "thr_posq3: max_iter must not be negative");
    if (!(opts->gate_m >= 0.0) || !std::isfinite(opts->gate_m))
        return thr::fail_msg(THR_ERR_ARG, "thr_posq3: gate_m must be finite and not negative (0: no exclusion)");
    if (!(opts->ratio > 0.0 && opts->ratio <= 1.0)) return thr::fail_msg(THR_ERR_ARG, "thr_posq3: ratio must lie in (0, 1]");
    const int floor_rx = free_z ? kMinRxFreeZ : kMinRxKnownHeight;
    if (opts->min_rx < floor_rx || opts->min_rx > kMaxReceivers)
        return thr::fail_msg(THR_ERR_ARG, "thr_posq3: min_rx must lie in %d .. %d %s, not %d", floor_rx, kMaxReceivers,
                             free_z ? "with z free" : "with the height known", opts->min_rx);
    if (n_groups > size_t(1) << 28) return thr::fail_msg(THR_ERR_ARG, "thr_posq3: too many groups");
    if (!free_z && n_groups && !group_h) return thr::fail_msg(THR_ERR_ARG, "thr_posq3: the known-height mode needs group_h");

    // ---- everything a kernel will index with is checked here, before anything is launched
    if (group_ptr[0] != 0) return thr::fail_msg(THR_ERR_ARG, "thr_posq3: group_ptr[0] must be 0");
    for (size_t g = 0; g < n_groups; ++g) {
        const int64_t len = group_ptr[g + 1] - group_ptr[g];
        if (len < 0) return thr::fail_msg(THR_ERR_ARG, "thr_posq3: group_ptr decreases at group %zu", g);
        if (len > (int64_t(1) << 24)) return thr::fail_msg(THR_ERR_ARG, "thr_posq3: group %zu is too long", g);
        if (!free_z && !std::isfinite(group_h[g])) return thr::fail_msg(THR_ERR_ARG, "thr_posq3: the height of group %zu is not finite", g);
    }
    const size_t n_rows = size_t(group_ptr[n_groups]);
    if (n_rows > size_t(1) << 30) return thr::fail_msg(THR_ERR_ARG, "thr_posq3: too many rows");
    if (n_rows && (!row_rx0 || !row_rx1 || !row_tdoa || !row_snr)) return thr::fail_msg(THR_ERR_ARG, "thr_posq3: null argument");
    for (size_t i = 0; i < n_rows; ++i)
        if (row_rx0[i] < 0 || row_rx0[i] >= n_rx || row_rx1[i] < 0 || row_rx1[i] >= n_rx)
            return thr::fail_msg(THR_ERR_ARG, "thr_posq3: row %zu names receivers %d and %d of %d", i, row_rx0[i], row_rx1[i], n_rx);
    if (row_weight)
        for (size_t i = 0; i < n_rows; ++i)
            if (!(row_weight[i] >= 0.0) || !std::isfinite(row_weight[i]))
                return thr::fail_msg(THR_ERR_ARG, "thr_posq3: row %zu has a weight that is negative or not finite", i);
    for (size_t i = 0; i < size_t(n_rx) * 3; ++i)
        if (!std::isfinite(rx_xyz[i])) return thr::fail_msg(THR_ERR_ARG, "thr_posq3: receiver coordinate %zu is not finite", i);
    for (int k = 0; k < (free_z ? 3 : 2); ++k)
        if (!std::isfinite(opts->x0[k])) return thr::fail_msg(THR_ERR_ARG, "thr_posq3: x0 must be finite");
    double lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {  // thr_pos3's box: the reference's rule per axis
        lo[k] = hi[k] = rx_xyz[k];
        for (int r = 1; r < n_rx; ++r) {
            lo[k] = std::fmin(lo[k], rx_xyz[3 * r + k]);
            hi[k] = std::fmax(hi[k], rx_xyz[3 * r + k]);
        }
        lo[k] -= kMaxDist;
        hi[k] += kMaxDist;
    }
    if (free_z && opts->has_z_range) {
        const double* z_range = opts->z_range;
        if (!std::isfinite(z_range[0]) || !std::isfinite(z_range[1]) || !(z_range[0] < z_range[1]))
            return thr::fail_msg(THR_ERR_ARG, "thr_posq3: z_range must be finite with z_lo < z_hi");
        lo[2] = z_range[0], hi[2] = z_range[1];
    }
    if (free_z && !(opts->x0[2] >= lo[2] && opts->x0[2] <= hi[2]))
        return thr::fail_msg(THR_ERR_ARG, "thr_posq3: x0[2] = %g lies outside the z range %g .. %g", opts->x0[2], lo[2], hi[2]);
    const Box box{lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]};
    const double x0 = opts->x0[0], y0 = opts->x0[1], z0 = free_z ? opts->x0[2] : 0.0;

    THR_TRY(thr::seg::pick_device(device_id));
    thr_posq3_result* R = new thr_posq3_result;
    thr::seg::ResultGuard guard{R};
    R->device = device_id;
    R->n_out = THR_POSQ3_N_OUTPUTS;
    hipStream_t s = nullptr;
    Event ev[6];
    for (Event& e : ev) THR_HIP_TRY(e.create());
    for (Event& e : R->ev) THR_HIP_TRY(e.create());
    const int ng = int(n_groups);
    const bool weighted = row_weight != nullptr;

    // ---- copies in
    DevBuf d_ptr, d_rx0, d_rx1, d_tdoa, d_snr, d_w, d_xyz, d_h;
    THR_HIP_TRY(d_ptr.alloc((n_groups + 1) * 8));
    THR_HIP_TRY(d_rx0.alloc(n_rows * 4));
    THR_HIP_TRY(d_rx1.alloc(n_rows * 4));
    THR_HIP_TRY(d_tdoa.alloc(n_rows * 8));
    THR_HIP_TRY(d_snr.alloc(n_rows * 8));
    if (weighted) THR_HIP_TRY(d_w.alloc(n_rows * 8));
    THR_HIP_TRY(d_xyz.alloc(size_t(n_rx) * 24));
    if (!free_z) THR_HIP_TRY(d_h.alloc(n_groups * 8));
    THR_HIP_TRY(hipEventRecord(ev[0].e, s));
    THR_HIP_TRY(hipMemcpy(d_ptr.p, group_ptr, (n_groups + 1) * 8, hipMemcpyHostToDevice));
    if (n_rows) {
        THR_HIP_TRY(hipMemcpy(d_rx0.p, row_rx0, n_rows * 4, hipMemcpyHostToDevice));
        THR_HIP_TRY(hipMemcpy(d_rx1.p, row_rx1, n_rows * 4, hipMemcpyHostToDevice));
        THR_HIP_TRY(hipMemcpy(d_tdoa.p, row_tdoa, n_rows * 8, hipMemcpyHostToDevice));
        THR_HIP_TRY(hipMemcpy(d_snr.p, row_snr, n_rows * 8, hipMemcpyHostToDevice));
        if (weighted) THR_HIP_TRY(hipMemcpy(d_w.p, row_weight, n_rows * 8, hipMemcpyHostToDevice));
    }
    THR_HIP_TRY(hipMemcpy(d_xyz.p, rx_xyz, size_t(n_rx) * 24, hipMemcpyHostToDevice));
    if (!free_z && n_groups) THR_HIP_TRY(hipMemcpy(d_h.p, group_h, n_groups * 8, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipEventRecord(ev[1].e, s));
    const Cols C{d_ptr.as<long long>(), d_rx0.as<int>(),  d_rx1.as<int>(),    d_tdoa.as<double>(),
                 d_snr.as<double>(),    d_w.as<double>(), d_xyz.as<double>(), d_h.as<double>()};
    DevBuf* O = R->out;

    // ---- A: the full solves
    DevBuf f_dop, f_hdop, f_vdop, f_q, f_rms, f_iters, f_nrx, f_mused, d_mask;
    THR_HIP_TRY(O[THR_POSQ3_FULL_POS].alloc(n_groups * 24));
    for (DevBuf* b : {&f_dop, &f_hdop, &f_vdop, &f_rms}) THR_HIP_TRY(b->alloc(n_groups * 8));
    THR_HIP_TRY(f_q.alloc(n_groups * 48));
    for (DevBuf* b : {&O[THR_POSQ3_FULL_STATUS], &f_iters, &f_nrx, &f_mused}) THR_HIP_TRY(b->alloc(n_groups * 4));
    const Solved full{O[THR_POSQ3_FULL_POS].as<double>(), f_dop.as<double>(), f_hdop.as<double>(), f_vdop.as<double>(),
                      f_q.as<double>(), f_rms.as<double>(), O[THR_POSQ3_FULL_STATUS].as<int>(), f_iters.as<int>(),
                      f_nrx.as<int>(), f_mused.as<int>()};
    THR_HIP_TRY(d_mask.alloc(n_groups * 8));
    THR_HIP_TRY(O[THR_POSQ3_SNR].alloc(n_groups * 8));
    if (ng) {
        const dim3 grid(unsigned((n_groups + kTeams - 1) / kTeams));
        auto* k = free_z ? (weighted ? k_full<true, true> : k_full<true, false>) : (weighted ? k_full<false, true> : k_full<false, false>);
        THR_TRY(launch_grid(k, grid, s, C, ng, x0, y0, z0, box, opts->max_iter, full, O[THR_POSQ3_SNR].as<double>(),
                            d_mask.as<unsigned long long>()));
    }
    THR_HIP_TRY(hipEventRecord(ev[2].e, s));

    // ---- B, C: flags, the candidates' pointer, the candidates
    DevBuf d_count, d_flagged, d_nflag, d_tgroup, d_tmp;
    size_t tmp_bytes = 0;
    long long n_tasks = 0;
    unsigned n_flagged = 0;
    const bool gated = opts->gate_m > 0.0 && ng > 0;
    THR_HIP_TRY(O[THR_POSQ3_TASK_PTR].alloc((n_groups + 1) * 8));
    if (gated) {
        THR_HIP_TRY(d_count.alloc((n_groups + 1) * 8));
        THR_HIP_TRY(d_flagged.alloc(n_groups * 4));
        THR_HIP_TRY(d_nflag.alloc(4));
        THR_TRY(launch(k_flag, n_groups + 1, s, full.status, full.nrx, full.rms, ng, opts->gate_m, int(opts->min_rx),
                       d_count.as<long long>(), d_flagged.as<unsigned>()));
        THR_HIP_TRY(thr::with_temp(d_tmp, tmp_bytes, [&](void* t, size_t& b) {
            return hipcub::DeviceScan::ExclusiveSum(t, b, d_count.as<long long>(), O[THR_POSQ3_TASK_PTR].as<long long>(), ng + 1, s);
        }));
        THR_HIP_TRY(thr::with_temp(d_tmp, tmp_bytes, [&](void* t, size_t& b) {
            return hipcub::DeviceReduce::Sum(t, b, d_flagged.as<unsigned>(), d_nflag.as<unsigned>(), ng, s);
        }));
        THR_HIP_TRY(hipMemcpy(&n_tasks, O[THR_POSQ3_TASK_PTR].as<long long>() + ng, 8, hipMemcpyDeviceToHost));  // synchronises
        THR_HIP_TRY(hipMemcpy(&n_flagged, d_nflag.p, 4, hipMemcpyDeviceToHost));
        if (n_tasks < 0 || n_tasks > (1ll << 28)) return thr::fail_msg(THR_ERR_ARG, "thr_posq3: too many candidates");
    } else {
        THR_HIP_TRY(hipMemsetAsync(O[THR_POSQ3_TASK_PTR].p, 0, (n_groups + 1) * 8, s));
    }
    const size_t nt = size_t(n_tasks);
    THR_HIP_TRY(d_tgroup.alloc(nt * 4));
    THR_HIP_TRY(O[THR_POSQ3_TASK_RX].alloc(nt * 4));
    if (nt)
        THR_TRY(launch(k_expand, n_groups, s, O[THR_POSQ3_TASK_PTR].as<long long>(), d_mask.as<unsigned long long>(), ng,
                       d_tgroup.as<int>(), O[THR_POSQ3_TASK_RX].as<int>()));
    THR_HIP_TRY(hipEventRecord(ev[3].e, s));

    // ---- D: the candidates
    DevBuf c_dop, c_hdop, c_vdop, c_q, c_mused;
    THR_HIP_TRY(O[THR_POSQ3_TASK_POS].alloc(nt * 24));
    THR_HIP_TRY(O[THR_POSQ3_TASK_RMS].alloc(nt * 8));
    for (DevBuf* b : {&c_dop, &c_hdop, &c_vdop}) THR_HIP_TRY(b->alloc(nt * 8));
    THR_HIP_TRY(c_q.alloc(nt * 48));
    for (DevBuf* b : {&O[THR_POSQ3_TASK_STATUS], &O[THR_POSQ3_TASK_ITERS], &O[THR_POSQ3_TASK_NRX], &c_mused}) THR_HIP_TRY(b->alloc(nt * 4));
    const Solved cand{O[THR_POSQ3_TASK_POS].as<double>(), c_dop.as<double>(), c_hdop.as<double>(), c_vdop.as<double>(),
                      c_q.as<double>(), O[THR_POSQ3_TASK_RMS].as<double>(), O[THR_POSQ3_TASK_STATUS].as<int>(),
                      O[THR_POSQ3_TASK_ITERS].as<int>(), O[THR_POSQ3_TASK_NRX].as<int>(), c_mused.as<int>()};
    if (nt) {
        const dim3 grid(unsigned((nt + kTeams - 1) / kTeams));
        auto* k = free_z ? (weighted ? k_cand<true, true> : k_cand<true, false>) : (weighted ? k_cand<false, true> : k_cand<false, false>);
        THR_TRY(launch_grid(k, grid, s, C, d_tgroup.as<int>(), O[THR_POSQ3_TASK_RX].as<int>(), int(nt), x0, y0, z0, box,
                            opts->max_iter, cand));
    }
    THR_HIP_TRY(hipEventRecord(ev[4].e, s));

    // ---- E: the choice and the residuals
    THR_HIP_TRY(O[THR_POSQ3_POS].alloc(n_groups * 24));
    for (DevBuf* b : {&O[THR_POSQ3_DOP], &O[THR_POSQ3_HDOP], &O[THR_POSQ3_VDOP]}) THR_HIP_TRY(b->alloc(n_groups * 8));
    THR_HIP_TRY(O[THR_POSQ3_Q].alloc(n_groups * 48));
    THR_HIP_TRY(O[THR_POSQ3_RMS].alloc(n_groups * 16));
    THR_HIP_TRY(O[THR_POSQ3_COUNTS].alloc(n_groups * 12));
    for (DevBuf* b : {&O[THR_POSQ3_STATUS], &O[THR_POSQ3_ITERS], &O[THR_POSQ3_FLAGS]}) THR_HIP_TRY(b->alloc(n_groups * 4));
    THR_HIP_TRY(O[THR_POSQ3_RESIDUAL].alloc(n_rows * 8));
    THR_HIP_TRY(O[THR_POSQ3_USED].alloc(n_rows));
    const Chosen chosen{O[THR_POSQ3_POS].as<double>(),  O[THR_POSQ3_DOP].as<double>(),   O[THR_POSQ3_HDOP].as<double>(),
                        O[THR_POSQ3_VDOP].as<double>(), O[THR_POSQ3_Q].as<double>(),     O[THR_POSQ3_RMS].as<double>(),
                        O[THR_POSQ3_STATUS].as<int>(),  O[THR_POSQ3_ITERS].as<int>(),    O[THR_POSQ3_COUNTS].as<int>(),
                        O[THR_POSQ3_FLAGS].as<int>(),   O[THR_POSQ3_RESIDUAL].as<double>(), O[THR_POSQ3_USED].as<unsigned char>()};
    THR_TRY(launch(free_z ? k_choose<true> : k_choose<false>, n_groups, s, C, ng, full, gated ? d_flagged.as<unsigned>() : nullptr,
                   O[THR_POSQ3_TASK_PTR].as<long long>(), O[THR_POSQ3_TASK_RX].as<int>(), cand, opts->ratio, int(opts->min_rx), chosen));
    THR_HIP_TRY(hipEventRecord(ev[5].e, s));
    THR_HIP_TRY(hipEventSynchronize(ev[5].e));  // the temporaries go out of scope
    for (int k = 0; k < 5; ++k) {
        float ms = 0;
        THR_HIP_TRY(hipEventElapsedTime(&ms, ev[k].e, ev[k + 1].e));
        g_posq3_ms[k] = ms;
    }

    size_t* B = R->bytes;
    B[THR_POSQ3_POS] = B[THR_POSQ3_FULL_POS] = n_groups * 24;
    B[THR_POSQ3_RMS] = n_groups * 16;
    B[THR_POSQ3_DOP] = B[THR_POSQ3_HDOP] = B[THR_POSQ3_VDOP] = B[THR_POSQ3_SNR] = n_groups * 8;
    B[THR_POSQ3_STATUS] = B[THR_POSQ3_ITERS] = B[THR_POSQ3_FLAGS] = B[THR_POSQ3_FULL_STATUS] = n_groups * 4;
    B[THR_POSQ3_Q] = n_groups * 48;
    B[THR_POSQ3_COUNTS] = n_groups * 12;
    B[THR_POSQ3_RESIDUAL] = n_rows * 8;
    B[THR_POSQ3_USED] = n_rows;
    B[THR_POSQ3_TASK_PTR] = (n_groups + 1) * 8;
    B[THR_POSQ3_TASK_RX] = B[THR_POSQ3_TASK_STATUS] = B[THR_POSQ3_TASK_NRX] = B[THR_POSQ3_TASK_ITERS] = nt * 4;
    B[THR_POSQ3_TASK_POS] = nt * 24;
    B[THR_POSQ3_TASK_RMS] = nt * 8;
    counts_out->groups = n_groups;
    counts_out->rows = n_rows;
    counts_out->flagged = n_flagged;
    counts_out->tasks = nt;
    *result_out = R;
    guard.r = nullptr;
    return THR_OK;
} catch (const std::bad_alloc&) {
    return thr::fail_msg(THR_ERR_DEVICE, "thr_posq3: out of host memory");
} catch (...) {
    return thr::on_exception("thr_posq3");
}

extern "C" int thr_posq3_fetch(thr_posq3_result* R, int which, void* dst, size_t dst_bytes) try {
    return thr::seg::fetch("thr_posq3_fetch", R, which, dst, dst_bytes, &g_posq3_ms[5]);
} catch (...) {
    return thr::on_exception("thr_posq3_fetch");
}

extern "C" void thr_posq3_free(thr_posq3_result* R) { thr::seg::free_result(R); }

extern "C" int thr_debug_posq3_times(double* ms_out) try {
    if (!ms_out) return thr::fail_msg(THR_ERR_ARG, "thr_debug_posq3_times: null argument");
    for (int k = 0; k < 6; ++k) ms_out[k] = g_posq3_ms[k];
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_posq3_times");
}
