// Positions from receivers with three coordinates (thr_pos3): thr_pos's solve for deployments whose antennas sit
// at different heights.  One 8-lane team per TDOA group, the layout and the iteration of csrc/pos3_lm.hpp (which
// are pos_lm.hpp's), in two modes:
//
//   known height (k_pos_h): the unknowns are (x, y); group_h[g] is the transmitter's height, so per row
//     az = rz[rx0] - h and bz = rz[rx1] - h are constants.  Three distinct receivers.  dop is the horizontal
//     dilution given the height, sqrt(trace(inv(A))) of the 2 x 2.  With every receiver at the height h this is
//     k_pos2d (pos.hip) on the flat table to the bit.
//   free z (k_pos_z): the unknowns are (x, y, z) inside the reference's box per axis (the receivers' extent
//     +- 10 km), whose z axis the caller may replace.  Four distinct receivers.  dop is the reference's dop() in
//     three dimensions, hdop = sqrt(inv00 + inv11), vdop = sqrt(inv22).
//
// Both write the r.m.s. residual sqrt(F / m) in metres, the snr mean, status and iters.  No atomics, no scratch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/thrifty_hip.h"
#include "lmdif8.hpp"
#include "pos3_lm.hpp"
#include "post_stages.hpp"

// the team's lanes must agree bit for bit and the known-height mode must return thr_pos's bits on a flat table:
// no a * b + c may become an fma in this file (the build also passes -ffp-contract=off for it, thrifty_amd/build.py)
#pragma clang fp contract(off)

namespace {

using thr::DevBuf;
using thr::Event;

constexpr int kBlock = 256;             // workgroup size
constexpr int kTeam = 8;                // lanes per group
constexpr int kTeams = kBlock / kTeam;  // groups per workgroup (_native.POS3_GROUPS_PER_WORKGROUP)
constexpr int kRegRows = 4;             // rows per lane kept in registers: groups up to 32 rows (_native.POS3_REGISTER_ROWS)
constexpr int kMaxReceivers = 64;       // the distinct-receiver count is a popcount of a 64-bit mask
constexpr double kMaxDist = 10e3;       // the reference's MAX_DIST (pos_est.py:24)
static_assert(kTeam == thr::pos3lm::kTeam, "the team of pos3_lm.hpp");

struct Outputs {
    double *pos, *dop, *hdop, *vdop, *rms, *snr;
    int *status, *iters;
};

// group g = one team.  group_ptr, rx0 / rx1 (< n_rx) and the table were checked on the host.
__global__ __launch_bounds__(kBlock) void k_pos_h(const long long* __restrict__ group_ptr, const int* __restrict__ rx0,
                                                  const int* __restrict__ rx1, const double* __restrict__ tdoa,
                                                  const double* __restrict__ snr, const double* __restrict__ xyz,
                                                  const double* __restrict__ group_h, int n_groups, double x0, double y0,
                                                  thr::pos3lm::Box box, int max_iter, Outputs out) {
    const int team = (blockIdx.x * kBlock + threadIdx.x) / kTeam, j = threadIdx.x & (kTeam - 1);
    const bool live = team < n_groups;
    const long long beg = live ? group_ptr[team] : 0;
    const int m = live ? int(group_ptr[team + 1] - beg) : 0;
    const double h = live ? group_h[team] : 0.0;
    const thr::pos3lm::Fit fit =
        thr::pos3lm::solve_team<false, kRegRows>(live, beg, m, j, rx0, rx1, tdoa, snr, xyz, h, x0, y0, 0.0, box, max_iter);
    if (live && j == 0) {
        const double dop = thr::pos3lm::dop2_of(fit.cur);
        out.pos[3 * size_t(team)] = fit.p0;
        out.pos[3 * size_t(team) + 1] = fit.p1;
        out.pos[3 * size_t(team) + 2] = h;
        out.dop[team] = dop;
        out.hdop[team] = dop;
        out.vdop[team] = 0.0;  // the height is given
        out.rms[team] = sqrt(fit.cur.F / double(m));
        out.snr[team] = fit.snr_mean;
        out.status[team] = fit.status;
        out.iters[team] = fit.iters;
    }
}

__global__ __launch_bounds__(kBlock) void k_pos_z(const long long* __restrict__ group_ptr, const int* __restrict__ rx0,
                                                  const int* __restrict__ rx1, const double* __restrict__ tdoa,
                                                  const double* __restrict__ snr, const double* __restrict__ xyz,
                                                  int n_groups, double x0, double y0, double z0, thr::pos3lm::Box box,
                                                  int max_iter, Outputs out) {
    const int team = (blockIdx.x * kBlock + threadIdx.x) / kTeam, j = threadIdx.x & (kTeam - 1);
    const bool live = team < n_groups;
    const long long beg = live ? group_ptr[team] : 0;
    const int m = live ? int(group_ptr[team + 1] - beg) : 0;
    const thr::pos3lm::Fit fit =
        thr::pos3lm::solve_team<true, kRegRows>(live, beg, m, j, rx0, rx1, tdoa, snr, xyz, 0.0, x0, y0, z0, box, max_iter);
    if (live && j == 0) {
        double dop, hdop, vdop;
        thr::pos3lm::dop3_of(fit.cur, dop, hdop, vdop);
        out.pos[3 * size_t(team)] = fit.p0;
        out.pos[3 * size_t(team) + 1] = fit.p1;
        out.pos[3 * size_t(team) + 2] = fit.p2;
        out.dop[team] = dop;
        out.hdop[team] = hdop;
        out.vdop[team] = vdop;
        out.rms[team] = sqrt(fit.cur.F / double(m));
        out.snr[team] = fit.snr_mean;
        out.status[team] = fit.status;
        out.iters[team] = fit.iters;
    }
}

#define P_TRY THR_HIP_TRY

thread_local double g_times_ms[3] = {0, 0, 0};  // last thr_pos3 of this thread: copies in, the kernel, copies out

}  // namespace

extern "C" int thr_pos3(int device_id, size_t n_groups, const int64_t* group_ptr, const int32_t* row_rx0,
                        const int32_t* row_rx1, const double* row_tdoa, const double* row_snr, int n_rx,
                        const double* rx_xyz, int mode, const double* group_h, const double* x0, const double* z_range,
                        int max_iter, double* pos_out, double* dop_out, double* hdop_out, double* vdop_out,
                        double* rms_out, double* snr_out, int32_t* status_out, int32_t* iters_out) try {
    g_times_ms[0] = g_times_ms[1] = g_times_ms[2] = 0;
    if (!group_ptr || !rx_xyz || !x0) return thr::fail_msg(THR_ERR_ARG, "thr_pos3: null argument");
    if (mode != THR_POS3_KNOWN_HEIGHT && mode != THR_POS3_FREE_Z)
        return thr::fail_msg(THR_ERR_ARG, "thr_pos3: mode must be THR_POS3_KNOWN_HEIGHT or THR_POS3_FREE_Z, not %d", mode);
    const bool free_z = mode == THR_POS3_FREE_Z;
    if (n_rx < 1 || n_rx > kMaxReceivers)
        return thr::fail_msg(THR_ERR_ARG, "thr_pos3: 1 to %d receivers, not %d", kMaxReceivers, n_rx);
    if (max_iter < 0) return thr::fail_msg(THR_ERR_ARG, "thr_pos3: max_iter must not be negative");
    if (n_groups > size_t(1) << 28) return thr::fail_msg(THR_ERR_ARG, "thr_pos3: too many groups");
    if (n_groups && (!pos_out || !dop_out || !hdop_out || !vdop_out || !rms_out || !snr_out || !status_out || !iters_out))
        return thr::fail_msg(THR_ERR_ARG, "thr_pos3: null argument");
    if (!free_z && n_groups && !group_h) return thr::fail_msg(THR_ERR_ARG, "thr_pos3: the known-height mode needs group_h");

    // ---- everything a kernel will index with is checked here, before anything is launched
    if (group_ptr[0] != 0) return thr::fail_msg(THR_ERR_ARG, "thr_pos3: group_ptr[0] must be 0");
    for (size_t g = 0; g < n_groups; ++g) {
        const int64_t len = group_ptr[g + 1] - group_ptr[g];
        if (len < 0) return thr::fail_msg(THR_ERR_ARG, "thr_pos3: group_ptr decreases at group %zu", g);
        if (len > (int64_t(1) << 24)) return thr::fail_msg(THR_ERR_ARG, "thr_pos3: group %zu is too long", g);
        if (!free_z && !std::isfinite(group_h[g])) return thr::fail_msg(THR_ERR_ARG, "thr_pos3: the height of group %zu is not finite", g);
    }
    const size_t n_rows = size_t(group_ptr[n_groups]);
    if (n_rows > size_t(1) << 30) return thr::fail_msg(THR_ERR_ARG, "thr_pos3: too many rows");
    if (n_rows && (!row_rx0 || !row_rx1 || !row_tdoa || !row_snr)) return thr::fail_msg(THR_ERR_ARG, "thr_pos3: null argument");
    for (size_t i = 0; i < n_rows; ++i)
        if (row_rx0[i] < 0 || row_rx0[i] >= n_rx || row_rx1[i] < 0 || row_rx1[i] >= n_rx)
            return thr::fail_msg(THR_ERR_ARG, "thr_pos3: row %zu names receivers %d and %d of %d", i, row_rx0[i], row_rx1[i], n_rx);
    for (size_t i = 0; i < size_t(n_rx) * 3; ++i)
        if (!std::isfinite(rx_xyz[i])) return thr::fail_msg(THR_ERR_ARG, "thr_pos3: receiver coordinate %zu is not finite", i);
    for (int k = 0; k < (free_z ? 3 : 2); ++k)
        if (!std::isfinite(x0[k])) return thr::fail_msg(THR_ERR_ARG, "thr_pos3: x0 must be finite");
    double lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {  // the reference's rule per axis
        lo[k] = hi[k] = rx_xyz[k];
        for (int r = 1; r < n_rx; ++r) {
            lo[k] = std::fmin(lo[k], rx_xyz[3 * r + k]);
            hi[k] = std::fmax(hi[k], rx_xyz[3 * r + k]);
        }
        lo[k] -= kMaxDist;
        hi[k] += kMaxDist;
    }
    if (free_z && z_range) {
        if (!std::isfinite(z_range[0]) || !std::isfinite(z_range[1]) || !(z_range[0] < z_range[1]))
            return thr::fail_msg(THR_ERR_ARG, "thr_pos3: z_range must be finite with z_lo < z_hi");
        lo[2] = z_range[0], hi[2] = z_range[1];
    }
    if (free_z && !(x0[2] >= lo[2] && x0[2] <= hi[2]))
        return thr::fail_msg(THR_ERR_ARG, "thr_pos3: x0[2] = %g lies outside the z range %g .. %g", x0[2], lo[2], hi[2]);

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

    DevBuf d_ptr, d_rx0, d_rx1, d_tdoa, d_snr, d_xyz, d_h;
    P_TRY(d_ptr.alloc((n_groups + 1) * 8));
    P_TRY(d_rx0.alloc(n_rows * 4));
    P_TRY(d_rx1.alloc(n_rows * 4));
    P_TRY(d_tdoa.alloc(n_rows * 8));
    P_TRY(d_snr.alloc(n_rows * 8));
    P_TRY(d_xyz.alloc(size_t(n_rx) * 3 * 8));
    if (!free_z) P_TRY(d_h.alloc(n_groups * 8));
    DevBuf o_pos, o_dop, o_hdop, o_vdop, o_rms, o_snr, o_status, o_iters;
    P_TRY(o_pos.alloc(n_groups * 3 * 8));
    for (DevBuf* b : {&o_dop, &o_hdop, &o_vdop, &o_rms, &o_snr}) P_TRY(b->alloc(n_groups * 8));
    P_TRY(o_status.alloc(n_groups * 4));
    P_TRY(o_iters.alloc(n_groups * 4));
    P_TRY(hipEventRecord(ev[0].e, s));
    P_TRY(hipMemcpy(d_ptr.p, group_ptr, (n_groups + 1) * 8, hipMemcpyHostToDevice));
    if (n_rows) {
        P_TRY(hipMemcpy(d_rx0.p, row_rx0, n_rows * 4, hipMemcpyHostToDevice));
        P_TRY(hipMemcpy(d_rx1.p, row_rx1, n_rows * 4, hipMemcpyHostToDevice));
        P_TRY(hipMemcpy(d_tdoa.p, row_tdoa, n_rows * 8, hipMemcpyHostToDevice));
        P_TRY(hipMemcpy(d_snr.p, row_snr, n_rows * 8, hipMemcpyHostToDevice));
    }
    P_TRY(hipMemcpy(d_xyz.p, rx_xyz, size_t(n_rx) * 3 * 8, hipMemcpyHostToDevice));
    if (!free_z) P_TRY(hipMemcpy(d_h.p, group_h, n_groups * 8, hipMemcpyHostToDevice));
    P_TRY(hipEventRecord(ev[1].e, s));

    const thr::pos3lm::Box box{lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]};
    const Outputs out{o_pos.as<double>(), o_dop.as<double>(), o_hdop.as<double>(), o_vdop.as<double>(),
                      o_rms.as<double>(),  o_snr.as<double>(), o_status.as<int>(), o_iters.as<int>()};
    const dim3 grid(unsigned((n_groups + kTeams - 1) / kTeams));
    if (free_z)
        hipLaunchKernelGGL(k_pos_z, grid, dim3(kBlock), 0, s, d_ptr.as<long long>(), d_rx0.as<int>(), d_rx1.as<int>(),
                           d_tdoa.as<double>(), d_snr.as<double>(), d_xyz.as<double>(), ng, x0[0], x0[1], x0[2], box,
                           max_iter, out);
    else
        hipLaunchKernelGGL(k_pos_h, grid, dim3(kBlock), 0, s, d_ptr.as<long long>(), d_rx0.as<int>(), d_rx1.as<int>(),
                           d_tdoa.as<double>(), d_snr.as<double>(), d_xyz.as<double>(), d_h.as<double>(), ng, x0[0], x0[1],
                           box, max_iter, out);
    P_TRY(hipGetLastError());
    P_TRY(hipEventRecord(ev[2].e, s));

    P_TRY(hipMemcpy(pos_out, o_pos.p, n_groups * 3 * 8, hipMemcpyDeviceToHost));
    P_TRY(hipMemcpy(dop_out, o_dop.p, n_groups * 8, hipMemcpyDeviceToHost));
    P_TRY(hipMemcpy(hdop_out, o_hdop.p, n_groups * 8, hipMemcpyDeviceToHost));
    P_TRY(hipMemcpy(vdop_out, o_vdop.p, n_groups * 8, hipMemcpyDeviceToHost));
    P_TRY(hipMemcpy(rms_out, o_rms.p, n_groups * 8, hipMemcpyDeviceToHost));
    P_TRY(hipMemcpy(snr_out, o_snr.p, n_groups * 8, hipMemcpyDeviceToHost));
    P_TRY(hipMemcpy(status_out, o_status.p, n_groups * 4, hipMemcpyDeviceToHost));
    P_TRY(hipMemcpy(iters_out, o_iters.p, n_groups * 4, hipMemcpyDeviceToHost));
    P_TRY(hipEventRecord(ev[3].e, s));
    P_TRY(hipEventSynchronize(ev[3].e));
    for (int k = 0; k < 3; ++k) {
        float ms = 0;
        P_TRY(hipEventElapsedTime(&ms, ev[k].e, ev[k + 1].e));
        g_times_ms[k] = ms;
    }
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_pos3");
}

extern "C" int thr_debug_pos3_times(double* ms_out) try {
    if (!ms_out) return thr::fail_msg(THR_ERR_ARG, "thr_debug_pos3_times: null argument");
    for (int k = 0; k < 3; ++k) ms_out[k] = g_times_ms[k];
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_pos3_times");
}
