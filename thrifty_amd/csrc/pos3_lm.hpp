// The 8-lane team's Levenberg-Marquardt iteration for receivers with three coordinates, stated once for both
// modes of thr_pos3 (pos3.hip): FREE_Z == false solves (x, y) with the transmitter's height given, FREE_Z == true
// solves (x, y, z).  The team layout and every rule are pos_lm.hpp's:
//
//   * one 8-lane team per TDOA group; lane j owns rows j, j + 8, ..., the first REG_ROWS of them in registers, the
//     rest re-read at every evaluation;
//   * every sum over rows is a group8_sum, bitwise identical in the team's eight lanes, and everything after the
//     sums is computed redundantly by all eight from identical inputs, so a team's control flow is uniform;
//   * all lanes of a wave execute every evaluation (a finished team's state is held by selects), so the DPP sums
//     never read a disabled lane;
//   * an axis on which p sits on the box while the descent direction points out of it is held; the undamped
//     (Gauss-Newton) step is looked at first and taken unjudged where it is shorter than kGaussNewtonGate (|p| + 1);
//     otherwise the damped step (A + mu I) h = -g on the free axes, projected into the box, is accepted when the
//     cost decreases, and mu follows the gain ratio (Nielsen's rule);
//   * the iteration ends on a step below kStepTol (|p| + 1); the statuses are pos_lm.hpp's, and every comparison
//     is written so that a NaN takes the branch that ends or does not accept.
//
// A row's ranges are da = sqrt((ax * ax + ay * ay) + az * az), the additions in exactly this order: with az == 0
// that is pos_lm.hpp's sqrt(ax * ax + ay * ay) to the bit, and with it the known-height mode on receivers that
// all sit at the transmitter's height returns the bits of thr_pos on the flat table (every other expression of
// that mode is pos_lm.hpp's unweighted one, operand for operand).
//
//   known height: az = rz[rx0] - h and bz = rz[rx1] - h are constants of the solve; an evaluation gives the six
//     team sums of pos_lm.hpp (F, the 2 x 2 normal matrix A, the gradient) with the 3-D ranges in the denominators.
//   free z: ten team sums (F, six entries of A, three of g); the step is solved on the free axes only -- 3 x 3 by
//     cofactors, 2 x 2 or 1 x 1 -- from identical values in the eight lanes.
//
// Weights and row subsets (thr_posq3, posq3.hip) are pos_lm.hpp's, behind two trailing template parameters whose
// defaults are the solve above: WEIGHTED == false reads no weight and leaves every expression as it stands;
// WEIGHTED == true counts row i as w_i * (m_used / sum_used w), the sum a group8_sum in team order followed by ONE
// division, so a column of ones gives the factor 1.0 exactly and the unweighted bits, and a zero sum ends kNonfinite.
// A `Used` predicate (poslm::AllRows, poslm::NotReceiver) numbers the used rows in order and gives lane j the numbers
// j, j + 8, ...: what it would hold of the group REBUILT without the other rows.  With the height known the weighted
// expressions are pos_lm.hpp's weighted ones, operand for operand.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "lmdif8.hpp"
#include "pos_lm.hpp"

// the team's lanes must agree bit for bit: no a * b + c may become an fma in what is inlined from here (the
// build also passes -ffp-contract=off to the file that includes this, thrifty_amd/build.py)
#pragma clang fp contract(off)

namespace thr {
namespace pos3lm {

using poslm::clamp;
using poslm::kGaussNewtonGate;
using poslm::kMuMax;
using poslm::kMuStart;
using poslm::kSpeedOfLight;
using poslm::kStepTol;
using poslm::kTeam;
using poslm::kAtBound;
using poslm::kNonfinite;
using poslm::kOk;
using poslm::kUnconverged;
using poslm::kUnderdetermined;

struct Row {
    double ax, ay, az, bx, by, bz, tc;  // rx0, rx1 (z less the known height) and tdoa * c
};
struct Sums {  // the z entries stay 0 with the height known
    double F, a00, a01, a11, g0, g1, a02, a12, a22, g2;
};
struct Box {
    double lo0, lo1, lo2, hi0, hi1, hi2;
};
struct Fit {  // identical in the team's eight lanes
    double p0, p1, p2;
    Sums cur;  // the last accepted evaluation
    int status, iters;
    int n_distinct;  // distinct receivers of the used rows
    double snr_mean; // over ALL rows of the group
    int m_used;      // used rows
    unsigned long long mask;  // receivers of the used rows
};

// the residual of one row at (px, py, pz): the expression every sum and every reported residual goes through (with
// the height known the row holds rz - h and pz is not read)
template <bool FREE_Z>
__device__ __forceinline__ double residual(const Row& r, double px, double py, double pz) {
    const double ax = r.ax - px, ay = r.ay - py, bx = r.bx - px, by = r.by - py;
    const double az = FREE_Z ? r.az - pz : r.az, bz = FREE_Z ? r.bz - pz : r.bz;
    const double da = sqrt((ax * ax + ay * ay) + az * az), db = sqrt((bx * bx + by * by) + bz * bz);
    return r.tc - (da - db);
}

// one row's terms at (px, py, pz), added to the lane's partial sums when `on`; w is read only when WEIGHTED
template <bool FREE_Z, bool WEIGHTED = false>
__device__ __forceinline__ void add_row(const Row& r, bool on, double px, double py, double pz, Sums& s, double w = 1.0) {
    const double ax = r.ax - px, ay = r.ay - py, bx = r.bx - px, by = r.by - py;
    const double az = FREE_Z ? r.az - pz : r.az, bz = FREE_Z ? r.bz - pz : r.bz;
    const double da = sqrt((ax * ax + ay * ay) + az * az), db = sqrt((bx * bx + by * by) + bz * bz);
    const double res = r.tc - (da - db);
    const double gx = ax / da - bx / db, gy = ay / da - by / db;
    if (WEIGHTED) {
        s.F += on ? w * (res * res) : 0.0;
        s.a00 += on ? w * (gx * gx) : 0.0;
        s.a01 += on ? w * (gx * gy) : 0.0;
        s.a11 += on ? w * (gy * gy) : 0.0;
        s.g0 += on ? w * (gx * res) : 0.0;
        s.g1 += on ? w * (gy * res) : 0.0;
    } else {
        s.F += on ? res * res : 0.0;
        s.a00 += on ? gx * gx : 0.0;
        s.a01 += on ? gx * gy : 0.0;
        s.a11 += on ? gy * gy : 0.0;
        s.g0 += on ? gx * res : 0.0;
        s.g1 += on ? gy * res : 0.0;
    }
    if (FREE_Z) {
        const double gz = az / da - bz / db;
        if (WEIGHTED) {
            s.a02 += on ? w * (gx * gz) : 0.0;
            s.a12 += on ? w * (gy * gz) : 0.0;
            s.a22 += on ? w * (gz * gz) : 0.0;
            s.g2 += on ? w * (gz * res) : 0.0;
        } else {
            s.a02 += on ? gx * gz : 0.0;
            s.a12 += on ? gy * gz : 0.0;
            s.a22 += on ? gz * gz : 0.0;
            s.g2 += on ? gz * res : 0.0;
        }
    }
}

// h: the known height (0.0 with z free: rz - 0.0 is rz)
__device__ __forceinline__ Row load_row(const int* __restrict__ rx0, const int* __restrict__ rx1,
                                        const double* __restrict__ tdoa, const double* __restrict__ xyz, double h,
                                        long long i) {
    const int a = rx0[i], b = rx1[i];
    return Row{xyz[3 * a], xyz[3 * a + 1], xyz[3 * a + 2] - h, xyz[3 * b], xyz[3 * b + 1], xyz[3 * b + 2] - h,
               tdoa[i] * kSpeedOfLight};
}

template <bool FREE_Z>
__device__ __forceinline__ bool finite_sums(const Sums& s) {
    const bool flat = isfinite(s.F) && isfinite(s.a00) && isfinite(s.a01) && isfinite(s.a11) && isfinite(s.g0) && isfinite(s.g1);
    return FREE_Z ? flat && isfinite(s.a02) && isfinite(s.a12) && isfinite(s.a22) && isfinite(s.g2) : flat;
}

// known height: dop = sqrt(trace(inv(A))) of the 2 x 2, pos_lm.hpp's closed form; -1 where the determinant is 0 or
// not finite
__device__ __forceinline__ double dop2_of(const Sums& s) {
    const double det = s.a00 * s.a11 - s.a01 * s.a01;
    return (det == 0.0 || !isfinite(det)) ? -1.0 : sqrt((s.a00 + s.a11) / det);
}

// free z: the diagonal of inv(A) by cofactors -> dop = sqrt(trace), hdop = sqrt(inv00 + inv11), vdop = sqrt(inv22);
// all three -1 where the determinant is 0 or not finite
__device__ __forceinline__ void dop3_of(const Sums& s, double& dop, double& hdop, double& vdop) {
    const double c00 = s.a11 * s.a22 - s.a12 * s.a12, c01 = s.a02 * s.a12 - s.a01 * s.a22, c02 = s.a01 * s.a12 - s.a02 * s.a11;
    const double c11 = s.a00 * s.a22 - s.a02 * s.a02, c22 = s.a00 * s.a11 - s.a01 * s.a01;
    const double det = (s.a00 * c00 + s.a01 * c01) + s.a02 * c02;
    const bool bad = det == 0.0 || !isfinite(det);
    const double i00 = c00 / det, i11 = c11 / det, i22 = c22 / det;
    dop = bad ? -1.0 : sqrt((i00 + i11) + i22);
    hdop = bad ? -1.0 : sqrt(i00 + i11);
    vdop = bad ? -1.0 : sqrt(i22);
}

// Rows beg .. beg + m of a group, lane j of the team (j = threadIdx.x & 7); `used(i)` says whether row i (its
// position in the columns) belongs to the task, and Used::kAll that it always does (the rows are then not walked).
// A team that is not `live` (past the last task) runs along with m == 0.  group_ptr, rx0 / rx1 (< 64) and the table
// were checked on the host.  FREE_Z == false: h is the group's height, z0 and the box's z are not read, and Fit::p2
// is h.  `weight` is read only when WEIGHTED.
template <bool FREE_Z, int REG_ROWS, bool WEIGHTED = false, class Used = poslm::AllRows>
__device__ __forceinline__ Fit solve_team(bool live, long long beg, int m, int j, const int* __restrict__ rx0,
                                          const int* __restrict__ rx1, const double* __restrict__ tdoa,
                                          const double* __restrict__ snr, const double* __restrict__ xyz, double h,
                                          double x0, double y0, double z0, const Box& box, int max_iter,
                                          const double* __restrict__ weight = nullptr, Used used = Used{}) {
    const double lo0 = box.lo0, lo1 = box.lo1, lo2 = box.lo2, hi0 = box.hi0, hi1 = box.hi1, hi2 = box.hi2;
    constexpr int kNeeded = FREE_Z ? 4 : 3;  // distinct receivers
    // ---- the lane's rows.  Every row: lane j owns rows j, j + 8, ...  A subset: used row number n of the group
    // (counted over the used rows only) belongs to lane n % 8 as its row n / 8 -- the layout of the group rebuilt
    // without the rows that are off
    Row reg[REG_ROWS];
    bool on[REG_ROWS];
    double wreg[REG_ROWS];
    unsigned long long mask = 0;
    int n_used = m, resume = m;  // resume: the first row that no register holds a used row up to
    if (Used::kAll) {
#pragma unroll
        for (int k = 0; k < REG_ROWS; ++k) {
            const int r = j + kTeam * k;
            on[k] = r < m;
            if (on[k]) mask |= (1ull << rx0[beg + r]) | (1ull << rx1[beg + r]);
            reg[k] = on[k] ? load_row(rx0, rx1, tdoa, xyz, h, beg + r) : Row{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0};
            wreg[k] = (WEIGHTED && on[k]) ? weight[beg + r] : 0.0;
        }
        for (int r = j + kTeam * REG_ROWS; r < m; r += kTeam) mask |= (1ull << rx0[beg + r]) | (1ull << rx1[beg + r]);
    } else {
        int row_of[REG_ROWS];  // relative to beg; -1: none
#pragma unroll
        for (int k = 0; k < REG_ROWS; ++k) row_of[k] = -1;
        n_used = 0;
        for (int r = 0; r < m; ++r) {  // every lane walks the whole group: two ints per row
            if (!used(beg + r)) continue;
            mask |= (1ull << rx0[beg + r]) | (1ull << rx1[beg + r]);
            if ((n_used & (kTeam - 1)) == j) {
#pragma unroll
                for (int k = 0; k < REG_ROWS; ++k)
                    if (k == n_used / kTeam) row_of[k] = r;
            }
            ++n_used;
            if (n_used == kTeam * REG_ROWS) resume = r + 1;
        }
#pragma unroll
        for (int k = 0; k < REG_ROWS; ++k) {
            on[k] = row_of[k] >= 0;
            reg[k] = on[k] ? load_row(rx0, rx1, tdoa, xyz, h, beg + row_of[k]) : Row{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0};
            wreg[k] = (WEIGHTED && on[k]) ? weight[beg + row_of[k]] : 0.0;
        }
    }
    unsigned mlo = unsigned(mask), mhi = unsigned(mask >> 32);
#pragma unroll
    for (int d = 1; d < kTeam; d <<= 1) {
        mlo |= __shfl_xor(mlo, d, 64);
        mhi |= __shfl_xor(mhi, d, 64);
    }
    const int n_distinct = __popc(mlo) + __popc(mhi);
    double snr_sum = 0.0;
    for (int r = j; r < m; r += kTeam) snr_sum += snr[beg + r];  // ALL rows, in the lanes of the whole group
    const double snr_mean = group8_sum(snr_sum) / double(m);

    // the rows past the registers: f(row) for this lane's, in order
    auto reread = [&](auto&& f) {
        if (Used::kAll) {
            for (int r = j + kTeam * REG_ROWS; r < m; r += kTeam) f(beg + r);
        } else {
            int n = kTeam * REG_ROWS;
            for (int r = resume; r < m; ++r) {
                if (!used(beg + r)) continue;
                if ((n & (kTeam - 1)) == j) f(beg + r);
                ++n;
            }
        }
    };

    double w_scale = 1.0;
    if (WEIGHTED) {
        double w_sum = 0.0;
#pragma unroll
        for (int k = 0; k < REG_ROWS; ++k) w_sum += wreg[k];
        reread([&](long long i) { w_sum += weight[i]; });
        w_scale = double(n_used) / group8_sum(w_sum);
#pragma unroll
        for (int k = 0; k < REG_ROWS; ++k) wreg[k] = wreg[k] * w_scale;
    }

    auto evaluate = [&](double px, double py, double pz) {
        Sums s{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < REG_ROWS; ++k) add_row<FREE_Z, WEIGHTED>(reg[k], on[k], px, py, pz, s, wreg[k]);
        if (Used::kAll && !WEIGHTED) {
            for (int r = j + kTeam * REG_ROWS; r < m; r += kTeam)  // long groups re-read their rows
                add_row<FREE_Z>(load_row(rx0, rx1, tdoa, xyz, h, beg + r), true, px, py, pz, s);
        } else {
            reread([&](long long i) {
                add_row<FREE_Z, WEIGHTED>(load_row(rx0, rx1, tdoa, xyz, h, i), true, px, py, pz, s, WEIGHTED ? weight[i] * w_scale : 1.0);
            });
        }
        Sums t{group8_sum(s.F), group8_sum(s.a00), group8_sum(s.a01), group8_sum(s.a11), group8_sum(s.g0),
               group8_sum(s.g1), 0.0, 0.0, 0.0, 0.0};
        if (FREE_Z) {
            t.a02 = group8_sum(s.a02);
            t.a12 = group8_sum(s.a12);
            t.a22 = group8_sum(s.a22);
            t.g2 = group8_sum(s.g2);
        }
        return t;
    };

    double p0 = x0, p1 = y0, p2 = FREE_Z ? z0 : h;
    Sums cur = evaluate(p0, p1, p2);
    int status = kUnconverged, iters = 0;
    bool active = live;
    if (n_distinct < kNeeded) {
        status = kUnderdetermined;
        active = false;
    } else if (!finite_sums<FREE_Z>(cur)) {
        status = kNonfinite;
        active = false;
    }
    double mu = kMuStart * (FREE_Z ? fmax(fmax(cur.a00, cur.a11), cur.a22) : fmax(cur.a00, cur.a11)), nu = 2.0;

    for (int it = 0; it < max_iter; ++it) {
        if (!__any(active)) break;
        // ---- the step, from identical values in the team's eight lanes
        const bool zero_grad = (FREE_Z ? fmax(fmax(fabs(cur.g0), fabs(cur.g1)), fabs(cur.g2)) : fmax(fabs(cur.g0), fabs(cur.g1))) == 0.0;
        const bool hold0 = (p0 <= lo0 && cur.g0 > 0.0) || (p0 >= hi0 && cur.g0 < 0.0);
        const bool hold1 = (p1 <= lo1 && cur.g1 > 0.0) || (p1 >= hi1 && cur.g1 < 0.0);
        const bool hold2 = FREE_Z ? (p2 <= lo2 && cur.g2 > 0.0) || (p2 >= hi2 && cur.g2 < 0.0) : true;
        const double scale = (FREE_Z ? sqrt((p0 * p0 + p1 * p1) + p2 * p2) : sqrt(p0 * p0 + p1 * p1)) + 1.0;
        double h0, h1, h2 = 0.0;
        auto solve = [&](double damp) {
            const double a = cur.a00 + damp, d = cur.a11 + damp;
            if (!FREE_Z) {
                if (hold0 || hold1) {
                    h0 = hold0 ? 0.0 : -cur.g0 / a;
                    h1 = hold1 ? 0.0 : -cur.g1 / d;
                } else {
                    const double det = a * d - cur.a01 * cur.a01;
                    h0 = (cur.a01 * cur.g1 - d * cur.g0) / det;
                    h1 = (cur.a01 * cur.g0 - a * cur.g1) / det;
                }
                h0 = clamp(p0 + h0, lo0, hi0) - p0;
                h1 = clamp(p1 + h1, lo1, hi1) - p1;
                return sqrt(h0 * h0 + h1 * h1);
            }
            const double f = cur.a22 + damp;
            const int held = int(hold0) + int(hold1) + int(hold2);
            if (held == 0) {  // 3 x 3, by cofactors of the symmetric matrix
                const double c00 = d * f - cur.a12 * cur.a12, c01 = cur.a02 * cur.a12 - cur.a01 * f, c02 = cur.a01 * cur.a12 - cur.a02 * d;
                const double c11 = a * f - cur.a02 * cur.a02, c12 = cur.a01 * cur.a02 - a * cur.a12, c22 = a * d - cur.a01 * cur.a01;
                const double det = (a * c00 + cur.a01 * c01) + cur.a02 * c02;
                h0 = -((c00 * cur.g0 + c01 * cur.g1) + c02 * cur.g2) / det;
                h1 = -((c01 * cur.g0 + c11 * cur.g1) + c12 * cur.g2) / det;
                h2 = -((c02 * cur.g0 + c12 * cur.g1) + c22 * cur.g2) / det;
            } else if (held == 1) {  // 2 x 2 on the two free axes u < v
                const double m00 = hold0 ? d : a, m11 = hold2 ? d : f;
                const double m01 = hold0 ? cur.a12 : (hold1 ? cur.a02 : cur.a01);
                const double r0 = hold0 ? cur.g1 : cur.g0, r1 = hold2 ? cur.g1 : cur.g2;
                const double det = m00 * m11 - m01 * m01;
                const double s0 = (m01 * r1 - m11 * r0) / det, s1 = (m01 * r0 - m00 * r1) / det;
                h0 = hold0 ? 0.0 : s0;
                h1 = hold0 ? s0 : (hold1 ? 0.0 : s1);
                h2 = hold2 ? 0.0 : s1;
            } else {  // one free axis, or none
                h0 = hold0 ? 0.0 : -cur.g0 / a;
                h1 = hold1 ? 0.0 : -cur.g1 / d;
                h2 = hold2 ? 0.0 : -cur.g2 / f;
            }
            h0 = clamp(p0 + h0, lo0, hi0) - p0;
            h1 = clamp(p1 + h1, lo1, hi1) - p1;
            h2 = clamp(p2 + h2, lo2, hi2) - p2;
            return sqrt((h0 * h0 + h1 * h1) + h2 * h2);
        };
        double len = solve(0.0);
        const bool gauss_newton = len <= kGaussNewtonGate * scale;  // false for a NaN
        if (!gauss_newton) len = solve(mu);
        const double t0 = p0 + h0, t1 = p1 + h1, t2 = FREE_Z ? p2 + h2 : p2;
        const Sums trial = evaluate(t0, t1, t2);  // every lane of the wave, finished teams too

        if (active) {
            iters = it + 1;
            if (zero_grad || (hold0 && hold1 && hold2)) {
                status = kOk;
                active = false;
            } else if (!finite_sums<FREE_Z>(trial) || !isfinite(len)) {
                status = kNonfinite;
                active = false;
            } else if (gauss_newton) {
                p0 = t0, p1 = t1, p2 = t2, cur = trial;
                if (len <= kStepTol * scale) {
                    status = kOk;
                    active = false;
                }
            } else if (trial.F < cur.F) {
                double pred = -(2.0 * (h0 * cur.g0 + h1 * cur.g1) +
                                (h0 * (cur.a00 * h0 + cur.a01 * h1) + h1 * (cur.a01 * h0 + cur.a11 * h1)));
                if (FREE_Z)
                    pred = -(2.0 * ((h0 * cur.g0 + h1 * cur.g1) + h2 * cur.g2) +
                             ((h0 * ((cur.a00 * h0 + cur.a01 * h1) + cur.a02 * h2) + h1 * ((cur.a01 * h0 + cur.a11 * h1) + cur.a12 * h2)) +
                              h2 * ((cur.a02 * h0 + cur.a12 * h1) + cur.a22 * h2)));
                const double rho = (cur.F - trial.F) / pred, q = 2.0 * rho - 1.0;
                mu *= fmin(fmax(1.0 / 3.0, 1.0 - q * q * q), 2.0);  // a NaN ratio: 1/3 (fmax drops the NaN)
                nu = 2.0;
                p0 = t0, p1 = t1, p2 = t2, cur = trial;
                if (len <= kStepTol * scale) {
                    status = kOk;
                    active = false;
                }
            } else {
                mu = fmin(mu * nu, kMuMax);
                nu = fmin(nu * 2.0, kMuMax);
            }
        }
    }
    if (status == kOk && (p0 <= lo0 || p0 >= hi0 || p1 <= lo1 || p1 >= hi1 || (FREE_Z && (p2 <= lo2 || p2 >= hi2))))
        status = kAtBound;
    return Fit{p0, p1, p2, cur, status, iters, n_distinct, snr_mean, n_used, (unsigned long long)mhi << 32 | mlo};
}

}  // namespace pos3lm
}  // namespace thr
