// The 8-lane team's Levenberg-Marquardt iteration of the 2-D position solver, stated once: k_pos2d (pos.hip)
// and the full and candidate solves of thr_posq (posq.hip) are instantiations of solve_team.
//
// A TASK is a group solved over a subset of its rows, those for which `used(row)` holds.  The used rows are
// numbered in order and lane j owns numbers j, j + 8, ..., the first REG_ROWS of them in registers, the rest
// re-read at every evaluation (the predicate is asked for all of them alike): the lanes hold what they would hold
// of the group REBUILT without the other rows, so a task returns the bits thr_pos returns on that group.  Every
// sum over rows is a group8_sum, bitwise identical in the team's eight lanes, and everything after the sums is
// computed redundantly by all eight from identical inputs, so a team's control flow is uniform.
//
//   * an evaluation at p gives six team sums: the cost F = sum w r^2, the normal matrix A = sum w g g', the
//     gradient sum w g r;
//   * an axis on which p sits on the box while the descent direction points out of it is held;
//   * the undamped (Gauss-Newton) step is looked at first.  Where it is shorter than kGaussNewtonGate (|p| + 1)
//     it is taken without asking the cost, and the iteration ends when such a step is shorter than
//     kStepTol (|p| + 1); the gate is decided afresh in every iteration;
//   * otherwise the damped step (A + mu I) h = -g, projected into the box, is accepted when the cost decreases,
//     and mu follows the gain ratio (Nielsen's rule).
// Every comparison is written so that a NaN takes the branch that ends or does not accept; the loop runs
// max_iter times at most.  All lanes of a wave execute every evaluation (a finished team's state is held by
// selects), so the DPP sums never read a disabled lane.
//
// WEIGHTED == false: no weight enters any expression (the weight pointer is never read), which is k_pos2d to
// the bit.  WEIGHTED == true: row i counts w_i * (m_used / sum_used w), the sum a group8_sum in team order
// followed by ONE division, so a column of ones gives the factor 1.0 exactly and the unweighted bits; a zero
// sum makes the factor infinite, the sums NaN and the task kNonfinite.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "lmdif8.hpp"

// the team's lanes must agree bit for bit: no a * b + c may become an fma in what is inlined from here (the
// build also passes -ffp-contract=off to the files that include this, thrifty_amd/build.py)
#pragma clang fp contract(off)

namespace thr {
namespace poslm {

constexpr int kTeam = 8;                   // lanes per task
constexpr double kSpeedOfLight = 2.997e8;  // the reference's constant (tdoa_est.py:25)
constexpr double kStepTol = 1e-13;         // the iteration ends on a step below kStepTol (|p| + 1)
constexpr double kGaussNewtonGate = 1e-4;  // undamped steps below kGaussNewtonGate (|p| + 1) are taken unjudged
constexpr double kMuStart = 1e-3;          // initial damping, relative to the larger diagonal entry of A
constexpr double kMuMax = 1e100;           // (A + mu I)'s determinant stays finite

enum Status : int { kOk = 0, kUnderdetermined = 1, kUnconverged = 2, kAtBound = 3, kNonfinite = 4 };

struct Row {
    double ax, ay, bx, by, tc;  // rx0, rx1 and tdoa * c
};
struct Sums {
    double F, a00, a01, a11, g0, g1;
};
struct Box {
    double lo0, lo1, hi0, hi1;
};
struct Fit {  // identical in the team's eight lanes
    double p0, p1;
    Sums cur;        // the last accepted evaluation
    int status, iters;
    int n_distinct;  // distinct receivers of the used rows
    int m_used;      // used rows
    double snr_mean; // over ALL rows of the group
    unsigned long long mask;  // receivers of the used rows
};

// the residual of one row at (px, py): the expression every sum and every reported residual goes through
__device__ __forceinline__ double residual(const Row& r, double px, double py) {
    const double ax = r.ax - px, ay = r.ay - py, bx = r.bx - px, by = r.by - py;
    const double da = sqrt(ax * ax + ay * ay), db = sqrt(bx * bx + by * by);
    return r.tc - (da - db);
}

// one row's terms at (px, py), added to the lane's partial sums when `on`
template <bool WEIGHTED>
__device__ __forceinline__ void add_row(const Row& r, bool on, double w, double px, double py, Sums& s) {
    const double ax = r.ax - px, ay = r.ay - py, bx = r.bx - px, by = r.by - py;
    const double da = sqrt(ax * ax + ay * ay), db = sqrt(bx * bx + by * by);
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
}

__device__ __forceinline__ Row load_row(const int* __restrict__ rx0, const int* __restrict__ rx1,
                                        const double* __restrict__ tdoa, const double* __restrict__ xy, long long i) {
    const int a = rx0[i], b = rx1[i];
    return Row{xy[2 * a], xy[2 * a + 1], xy[2 * b], xy[2 * b + 1], tdoa[i] * kSpeedOfLight};
}

__device__ __forceinline__ bool finite6(const Sums& s) {
    return isfinite(s.F) && isfinite(s.a00) && isfinite(s.a01) && isfinite(s.a11) && isfinite(s.g0) && isfinite(s.g1);
}

struct AllRows {  // every row of the group
    static constexpr bool kAll = true;
    __device__ __forceinline__ bool operator()(long long) const { return true; }
};
struct NotReceiver {  // the rows that do not name receiver `ex`
    static constexpr bool kAll = false;
    const int *rx0, *rx1;
    int ex;
    __device__ __forceinline__ bool operator()(long long i) const { return rx0[i] != ex && rx1[i] != ex; }
};

__device__ __forceinline__ double clamp(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

// dop = sqrt(trace(inv(A))), closed form; -1 where the determinant is 0 or not finite
__device__ __forceinline__ double dop_of(const Sums& s) {
    const double det = s.a00 * s.a11 - s.a01 * s.a01;
    return (det == 0.0 || !isfinite(det)) ? -1.0 : sqrt((s.a00 + s.a11) / det);
}

// Rows beg .. beg + m of a group, lane j of the team (j = threadIdx.x & 7); `used(i)` says whether row i (its
// position in the columns) belongs to the task, and Used::kAll that it always does (the rows are then not
// walked).  A team that is not `live` (past the last task) runs along with m == 0.  group_ptr, rx0 / rx1 (< 64) and the table were checked on the host.
template <bool WEIGHTED, int REG_ROWS, class Used>
__device__ __forceinline__ Fit solve_team(bool live, long long beg, int m, int j, const int* __restrict__ rx0,
                                          const int* __restrict__ rx1, const double* __restrict__ tdoa,
                                          const double* __restrict__ snr, const double* __restrict__ weight,
                                          const double* __restrict__ xy, double x0, double y0, const Box& box,
                                          int max_iter, Used used) {
    const double lo0 = box.lo0, lo1 = box.lo1, hi0 = box.hi0, hi1 = box.hi1;
    // ---- the lane's rows: used row number n of the group (counted over the used rows only) belongs to lane
    // n % 8 as its row n / 8 -- the layout of the group rebuilt without the rows that are off
    int row_of[REG_ROWS];  // relative to beg; -1: none
    unsigned long long mask = 0;
    int n_used = 0, resume = m;  // resume: the first row that no register holds a used row up to
#pragma unroll
    for (int k = 0; k < REG_ROWS; ++k) row_of[k] = -1;
    if (Used::kAll) {
#pragma unroll
        for (int k = 0; k < REG_ROWS; ++k) {
            const int r = j + kTeam * k;
            if (r < m) {
                row_of[k] = r;
                mask |= (1ull << rx0[beg + r]) | (1ull << rx1[beg + r]);
            }
        }
        for (int r = j + kTeam * REG_ROWS; r < m; r += kTeam) mask |= (1ull << rx0[beg + r]) | (1ull << rx1[beg + r]);
        n_used = m;
    } else {
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

    Row reg[REG_ROWS];
    bool on[REG_ROWS];
    double wreg[REG_ROWS];
    double w_sum = 0.0, w_scale = 1.0;
#pragma unroll
    for (int k = 0; k < REG_ROWS; ++k) {
        on[k] = row_of[k] >= 0;
        reg[k] = on[k] ? load_row(rx0, rx1, tdoa, xy, beg + row_of[k]) : Row{1.0, 0.0, 0.0, 1.0, 0.0};
        wreg[k] = (WEIGHTED && on[k]) ? weight[beg + row_of[k]] : 0.0;
        w_sum += wreg[k];
    }
    if (WEIGHTED) {
        reread([&](long long i) { w_sum += weight[i]; });
        w_scale = double(n_used) / group8_sum(w_sum);
#pragma unroll
        for (int k = 0; k < REG_ROWS; ++k) wreg[k] = wreg[k] * w_scale;
    }

    auto evaluate = [&](double px, double py) {
        Sums s{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < REG_ROWS; ++k) add_row<WEIGHTED>(reg[k], on[k], wreg[k], px, py, s);
        reread([&](long long i) {  // long tasks re-read their rows
            add_row<WEIGHTED>(load_row(rx0, rx1, tdoa, xy, i), true, WEIGHTED ? weight[i] * w_scale : 1.0, px, py, s);
        });
        return Sums{group8_sum(s.F), group8_sum(s.a00), group8_sum(s.a01), group8_sum(s.a11), group8_sum(s.g0),
                    group8_sum(s.g1)};
    };

    double p0 = x0, p1 = y0;
    Sums cur = evaluate(p0, p1);
    int status = kUnconverged, iters = 0;
    bool active = live;
    if (n_distinct < 3) {
        status = kUnderdetermined;
        active = false;
    } else if (!finite6(cur)) {
        status = kNonfinite;
        active = false;
    }
    double mu = kMuStart * fmax(cur.a00, cur.a11), nu = 2.0;

    for (int it = 0; it < max_iter; ++it) {
        if (!__any(active)) break;
        // ---- the step, from identical values in the team's eight lanes
        const bool zero_grad = fmax(fabs(cur.g0), fabs(cur.g1)) == 0.0;
        const bool hold0 = (p0 <= lo0 && cur.g0 > 0.0) || (p0 >= hi0 && cur.g0 < 0.0);
        const bool hold1 = (p1 <= lo1 && cur.g1 > 0.0) || (p1 >= hi1 && cur.g1 < 0.0);
        const double scale = sqrt(p0 * p0 + p1 * p1) + 1.0;
        double h0, h1;
        auto solve = [&](double damp) {
            const double a = cur.a00 + damp, d = cur.a11 + damp;
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
        };
        double len = solve(0.0);
        const bool gauss_newton = len <= kGaussNewtonGate * scale;  // false for a NaN
        if (!gauss_newton) len = solve(mu);
        const double t0 = p0 + h0, t1 = p1 + h1;
        const Sums trial = evaluate(t0, t1);  // every lane of the wave, finished teams too

        if (active) {
            iters = it + 1;
            if (zero_grad || (hold0 && hold1)) {
                status = kOk;
                active = false;
            } else if (!finite6(trial) || !isfinite(len)) {
                status = kNonfinite;
                active = false;
            } else if (gauss_newton) {
                p0 = t0, p1 = t1, cur = trial;
                if (len <= kStepTol * scale) {
                    status = kOk;
                    active = false;
                }
            } else if (trial.F < cur.F) {
                const double pred = -(2.0 * (h0 * cur.g0 + h1 * cur.g1) +
                                      (h0 * (cur.a00 * h0 + cur.a01 * h1) + h1 * (cur.a01 * h0 + cur.a11 * h1)));
                const double rho = (cur.F - trial.F) / pred, q = 2.0 * rho - 1.0;
                mu *= fmin(fmax(1.0 / 3.0, 1.0 - q * q * q), 2.0);  // a NaN ratio: 1/3 (fmax drops the NaN)
                nu = 2.0;
                p0 = t0, p1 = t1, cur = trial;
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
    if (status == kOk && (p0 <= lo0 || p0 >= hi0 || p1 <= lo1 || p1 >= hi1)) status = kAtBound;
    return Fit{p0, p1, cur, status, iters, n_distinct, n_used, snr_mean, (unsigned long long)mhi << 32 | mlo};
}

}  // namespace poslm
}  // namespace thr
