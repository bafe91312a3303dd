// pos on the device (reference thrifty/pos_est.py): the position of every mobile transmission from its
// TDOA group.  One 8-lane team per group (the layout of k_fit, csrc/lmdif8.hpp): lane j owns rows
// j, j + 8, ... of its group, the first four of them in registers; every sum over rows is a group8_sum,
// bitwise identical in the team's eight lanes, and everything after the sums is computed redundantly by
// all eight from identical inputs, so a team's control flow is uniform.
//
// 2-D: minimise sum (tdoa_i c - (|rx0_i - p| - |rx1_i - p|))^2 from x0 inside the reference's box
// (min(rx) - 10 km .. max(rx) + 10 km).  Not SciPy's TRF: a Levenberg-Marquardt iteration of our own, stated
// once in csrc/pos_lm.hpp (thr_posq's solves are the same template): evaluation, hold / step / gate / damping
// rules, the stopping rule, the statuses and the closed-form dop.  Here it runs with no weights and every row on.
// 1-D (two receivers): the reference's three float64 operations in its order, no iteration.
// dop = sqrt(trace(inv(G'G))) at the estimate, closed form; -1 where the determinant is 0 or not finite.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/thrifty_hip.h"
#include "lmdif8.hpp"
#include "pos_lm.hpp"
#include "post_stages.hpp"

// the team's lanes must agree bit for bit and the 1-D result must equal numpy's: no a * b + c may become
// an fma in this file (the build also passes -ffp-contract=off for it, thrifty_amd/build.py)
#pragma clang fp contract(off)

namespace {

using thr::DevBuf;
using thr::Event;

constexpr int kBlock = 256;                // workgroup size
constexpr int kTeam = 8;                    // lanes per group
constexpr int kTeams = kBlock / kTeam;      // groups per workgroup (_native.POS_GROUPS_PER_WORKGROUP)
constexpr int kRegRows = 4;                 // rows per lane kept in registers: groups up to 32 rows (_native.POS_REGISTER_ROWS)
constexpr int kMaxReceivers = 64;           // the distinct-receiver count is a popcount of a 64-bit mask
constexpr double kMaxDist = 10e3;           // pos_est.py:24
using thr::poslm::kSpeedOfLight;
using thr::poslm::kOk;
using thr::poslm::kNonfinite;
static_assert(kTeam == thr::poslm::kTeam, "the team of pos_lm.hpp");

// group g = one team.  group_ptr, row_rx0 / row_rx1 (< n_rx) and the table were checked on the host.
__global__ __launch_bounds__(kBlock) void k_pos2d(const long long* __restrict__ group_ptr, const int* __restrict__ rx0,
                                                  const int* __restrict__ rx1, const double* __restrict__ tdoa,
                                                  const double* __restrict__ snr, const double* __restrict__ xy,
                                                  int n_groups, double x0, double y0, double lo0, double lo1, double hi0,
                                                  double hi1, int max_iter, double* __restrict__ pos_out,
                                                  double* __restrict__ dop_out, double* __restrict__ snr_out,
                                                  int* __restrict__ status_out, int* __restrict__ iters_out) {
    const int team = (blockIdx.x * kBlock + threadIdx.x) / kTeam, j = threadIdx.x & (kTeam - 1);
    const bool live = team < n_groups;
    const long long beg = live ? group_ptr[team] : 0;
    const int m = live ? int(group_ptr[team + 1] - beg) : 0;
    const thr::poslm::Fit fit = thr::poslm::solve_team<false, kRegRows>(
        live, beg, m, j, rx0, rx1, tdoa, snr, nullptr, xy, x0, y0, thr::poslm::Box{lo0, lo1, hi0, hi1}, max_iter,
        thr::poslm::AllRows{});
    if (live && j == 0) {
        pos_out[2 * team] = fit.p0;
        pos_out[2 * team + 1] = fit.p1;
        dop_out[team] = thr::poslm::dop_of(fit.cur);
        snr_out[team] = fit.snr_mean;
        status_out[team] = fit.status;
        iters_out[team] = fit.iters;
    }
}

// 1-D, two receivers, one row per group (checked on the host): pos_est.py:31-47, one lane per group
__global__ __launch_bounds__(kBlock) void k_pos1d(const long long* __restrict__ group_ptr, const int* __restrict__ rx0,
                                                  const int* __restrict__ rx1, const double* __restrict__ tdoa,
                                                  const double* __restrict__ snr, const double* __restrict__ x,
                                                  int n_groups, int first, int second, double* __restrict__ pos_out,
                                                  double* __restrict__ dop_out, double* __restrict__ snr_out,
                                                  int* __restrict__ status_out, int* __restrict__ iters_out) {
    const int g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= n_groups) return;
    const long long i = group_ptr[g];
    const double tdoa_pos = tdoa[i] * kSpeedOfLight;
    const double rx_dist = x[first] + x[second];
    const double p = x[first] > x[second] ? (rx_dist - tdoa_pos) / 2.0 : (rx_dist + tdoa_pos) / 2.0;
    const double a = x[rx0[i]] - p, b = x[rx1[i]] - p;
    const double gg = a / fabs(a) - b / fabs(b), s = gg * gg;
    pos_out[g] = p;
    dop_out[g] = s == 0.0 ? -1.0 : sqrt(1.0 / s);
    snr_out[g] = snr[i];
    status_out[g] = (isfinite(p) && isfinite(s)) ? kOk : kNonfinite;
    iters_out[g] = 0;
}

#define P_TRY THR_HIP_TRY

thread_local double g_times_ms[3] = {0, 0, 0};  // last thr_pos of this thread: copies in, kernels, copies out

}  // namespace

// What the host derives from the receiver table, with its checks (thr_pos and thr_postdetect share them).
int thr::pos_plan(const char* who, int n_rx, int dims, const double* rx_coords, const int32_t* first_two_rx,
                  const double* x0, PosPlan& plan) {
    if (!rx_coords) return thr::fail_msg(THR_ERR_ARG, "%s: null argument", who);
    if (dims != 1 && dims != 2) return thr::fail_msg(THR_ERR_ARG, "%s: 1 or 2 dimensions, not %d", who, dims);
    if (n_rx < 1 || n_rx > kMaxReceivers)
        return thr::fail_msg(THR_ERR_ARG, "%s: 1 to %d receivers, not %d", who, kMaxReceivers, n_rx);
    for (size_t i = 0; i < size_t(n_rx) * size_t(dims); ++i)
        if (!std::isfinite(rx_coords[i])) return thr::fail_msg(THR_ERR_ARG, "%s: receiver coordinate %zu is not finite", who, i);
    if (dims == 1) {
        if (n_rx != 2) return thr::fail_msg(THR_ERR_ARG, "%s: the 1-D solver takes two receivers, not %d", who, n_rx);
        if (!first_two_rx || first_two_rx[0] < 0 || first_two_rx[0] >= n_rx || first_two_rx[1] < 0 || first_two_rx[1] >= n_rx)
            return thr::fail_msg(THR_ERR_ARG, "%s: first_two_rx must name two of the %d receivers", who, n_rx);
        plan.first = first_two_rx[0], plan.second = first_two_rx[1];
    } else {
        if (!x0 || !std::isfinite(x0[0]) || !std::isfinite(x0[1])) return thr::fail_msg(THR_ERR_ARG, "%s: x0 must be finite", who);
        for (int k = 0; k < 2; ++k) {
            plan.start[k] = x0[k];
            plan.lo[k] = plan.hi[k] = rx_coords[k];
            for (int r = 1; r < n_rx; ++r) {
                plan.lo[k] = std::fmin(plan.lo[k], rx_coords[2 * r + k]);
                plan.hi[k] = std::fmax(plan.hi[k], rx_coords[2 * r + k]);
            }
            plan.lo[k] -= kMaxDist;
            plan.hi[k] += kMaxDist;
        }
    }
    return THR_OK;
}

// The stage on device pointers (post_stages.hpp): one launch.  group_ptr and the row receivers are the
// caller's responsibility (thr_pos checks them on the host, thr_postdetect makes them itself).
int thr::pos_core(int ng, const long long* d_ptr, const int* d_rx0, const int* d_rx1, const double* d_tdoa,
                  const double* d_snr, const double* d_xy, int dims, const PosPlan& plan, int max_iter, hipStream_t s,
                  PosOut& out) {
    const size_t n_groups = size_t(ng);
    P_TRY(out.pos.alloc(n_groups * size_t(dims) * 8));
    P_TRY(out.dop.alloc(n_groups * 8));
    P_TRY(out.snr.alloc(n_groups * 8));
    P_TRY(out.status.alloc(n_groups * 4));
    P_TRY(out.iters.alloc(n_groups * 4));
    if (dims == 1)
        hipLaunchKernelGGL(k_pos1d, dim3(unsigned((n_groups + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                           d_ptr, d_rx0, d_rx1, d_tdoa, d_snr,
                           d_xy, ng, plan.first, plan.second, out.pos.as<double>(), out.dop.as<double>(),
                           out.snr.as<double>(), out.status.as<int>(), out.iters.as<int>());
    else
        hipLaunchKernelGGL(k_pos2d, dim3(unsigned((n_groups + kTeams - 1) / kTeams)), dim3(kBlock), 0, s,
                           d_ptr, d_rx0, d_rx1, d_tdoa, d_snr,
                           d_xy, ng, plan.start[0], plan.start[1], plan.lo[0], plan.lo[1], plan.hi[0], plan.hi[1], max_iter,
                           out.pos.as<double>(), out.dop.as<double>(), out.snr.as<double>(), out.status.as<int>(),
                           out.iters.as<int>());
    P_TRY(hipGetLastError());
    return THR_OK;
}

extern "C" int thr_pos(int device_id, size_t n_groups, const int64_t* group_ptr, const int32_t* row_rx0,
                       const int32_t* row_rx1, const double* row_tdoa, const double* row_snr, int n_rx, int dims,
                       const double* rx_coords, const int32_t* first_two_rx, const double* x0, int max_iter,
                       double* pos_out, double* dop_out, double* snr_out, int32_t* status_out, int32_t* iters_out) try {
    g_times_ms[0] = g_times_ms[1] = g_times_ms[2] = 0;
    if (!group_ptr || !rx_coords) return thr::fail_msg(THR_ERR_ARG, "thr_pos: null argument");
    if (dims != 1 && dims != 2) return thr::fail_msg(THR_ERR_ARG, "thr_pos: 1 or 2 dimensions, not %d", dims);
    if (n_rx < 1 || n_rx > kMaxReceivers)
        return thr::fail_msg(THR_ERR_ARG, "thr_pos: 1 to %d receivers, not %d", kMaxReceivers, n_rx);
    if (max_iter < 0) return thr::fail_msg(THR_ERR_ARG, "thr_pos: max_iter must not be negative");
    if (n_groups > size_t(1) << 28) return thr::fail_msg(THR_ERR_ARG, "thr_pos: too many groups");
    if (n_groups && (!pos_out || !dop_out || !snr_out || !status_out || !iters_out))
        return thr::fail_msg(THR_ERR_ARG, "thr_pos: null argument");

    // ---- everything a kernel will index with is checked here, before anything is launched
    if (group_ptr[0] != 0) return thr::fail_msg(THR_ERR_ARG, "thr_pos: group_ptr[0] must be 0");
    for (size_t g = 0; g < n_groups; ++g) {
        const int64_t len = group_ptr[g + 1] - group_ptr[g];
        if (len < 0) return thr::fail_msg(THR_ERR_ARG, "thr_pos: group_ptr decreases at group %zu", g);
        if (len > (int64_t(1) << 24)) return thr::fail_msg(THR_ERR_ARG, "thr_pos: group %zu is too long", g);
        if (dims == 1 && len != 1)
            return thr::fail_msg(THR_ERR_ARG, "thr_pos: a 1-D group holds one row, group %zu holds %lld", g, (long long)len);
    }
    const size_t n_rows = size_t(group_ptr[n_groups]);
    if (n_rows > size_t(1) << 30) return thr::fail_msg(THR_ERR_ARG, "thr_pos: too many rows");
    if (n_rows && (!row_rx0 || !row_rx1 || !row_tdoa || !row_snr))
        return thr::fail_msg(THR_ERR_ARG, "thr_pos: null argument");
    for (size_t i = 0; i < n_rows; ++i)
        if (row_rx0[i] < 0 || row_rx0[i] >= n_rx || row_rx1[i] < 0 || row_rx1[i] >= n_rx)
            return thr::fail_msg(THR_ERR_ARG, "thr_pos: row %zu names receivers %d and %d of %d", i, row_rx0[i], row_rx1[i], n_rx);
    thr::PosPlan plan;
    if (const int rc = thr::pos_plan("thr_pos", n_rx, dims, rx_coords, first_two_rx, x0, plan)) return rc;

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return thr::fail_msg(THR_ERR_DEVICE, "no HIP device available (this engine has no CPU fallback)");
    if (device_id < 0 || device_id >= ndev) return thr::fail_msg(THR_ERR_ARG, "bad device_id %d", device_id);
    if (n_groups == 0) return THR_OK;  // nothing to launch (the times stay zero)
    P_TRY(hipSetDevice(device_id));
    const int ng = int(n_groups);
    hipStream_t s = nullptr;
    Event ev[4];
    for (Event& e : ev) P_TRY(e.create());

    DevBuf d_ptr, d_rx0, d_rx1, d_tdoa, d_snr, d_xy;
    P_TRY(d_ptr.alloc((n_groups + 1) * 8));
    P_TRY(d_rx0.alloc(n_rows * 4));
    P_TRY(d_rx1.alloc(n_rows * 4));
    P_TRY(d_tdoa.alloc(n_rows * 8));
    P_TRY(d_snr.alloc(n_rows * 8));
    P_TRY(d_xy.alloc(size_t(n_rx) * size_t(dims) * 8));
    P_TRY(hipEventRecord(ev[0].e, s));
    P_TRY(hipMemcpy(d_ptr.p, group_ptr, (n_groups + 1) * 8, hipMemcpyHostToDevice));
    if (n_rows) {
        P_TRY(hipMemcpy(d_rx0.p, row_rx0, n_rows * 4, hipMemcpyHostToDevice));
        P_TRY(hipMemcpy(d_rx1.p, row_rx1, n_rows * 4, hipMemcpyHostToDevice));
        P_TRY(hipMemcpy(d_tdoa.p, row_tdoa, n_rows * 8, hipMemcpyHostToDevice));
        P_TRY(hipMemcpy(d_snr.p, row_snr, n_rows * 8, hipMemcpyHostToDevice));
    }
    P_TRY(hipMemcpy(d_xy.p, rx_coords, size_t(n_rx) * size_t(dims) * 8, hipMemcpyHostToDevice));
    P_TRY(hipEventRecord(ev[1].e, s));

    thr::PosOut out;
    if (const int rc = thr::pos_core(ng, d_ptr.as<long long>(), d_rx0.as<int>(), d_rx1.as<int>(), d_tdoa.as<double>(),
                                     d_snr.as<double>(), d_xy.as<double>(), dims, plan, max_iter, s, out))
        return rc;
    P_TRY(hipEventRecord(ev[2].e, s));

    P_TRY(hipMemcpy(pos_out, out.pos.p, n_groups * size_t(dims) * 8, hipMemcpyDeviceToHost));
    P_TRY(hipMemcpy(dop_out, out.dop.p, n_groups * 8, hipMemcpyDeviceToHost));
    P_TRY(hipMemcpy(snr_out, out.snr.p, n_groups * 8, hipMemcpyDeviceToHost));
    P_TRY(hipMemcpy(status_out, out.status.p, n_groups * 4, hipMemcpyDeviceToHost));
    P_TRY(hipMemcpy(iters_out, out.iters.p, n_groups * 4, hipMemcpyDeviceToHost));
    P_TRY(hipEventRecord(ev[3].e, s));
    P_TRY(hipEventSynchronize(ev[3].e));
    for (int k = 0; k < 3; ++k) {
        float ms = 0;
        P_TRY(hipEventElapsedTime(&ms, ev[k].e, ev[k + 1].e));
        g_times_ms[k] = ms;
    }
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_pos");
}

extern "C" int thr_debug_pos_times(double* ms_out) try {
    if (!ms_out) return thr::fail_msg(THR_ERR_ARG, "thr_debug_pos_times: null argument");
    for (int k = 0; k < 3; ++k) ms_out[k] = g_times_ms[k];
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_pos_times");
}
