// Coverage map on the device (thr_coverage): for every cell of a raster over a site the dop, the predicted covariance
// of thr_pos's estimator under per-receiver arrival noise, and the error statistics of T simulated transmissions, each
// solved by thr_pos's own stage (pos_core, post_stages.hpp).  No recording is read.  include/thrifty_hip.h states every
// rule; tests/coverage_ref.py restates them in NumPy.
//
// Kernels:
//   k_cells    one lane per cell: who hears it, the row count, N, dop, M, Cov = inv(N) M inv(N), the two static flags;
//   k_scatter  the covered cells in ascending order (their positions come from a hipCUB scan of the covered flags;
//              a second scan of the row counts gives every task's first row);
//   per slab of consecutive tasks:
//   k_noise    one lane per (task, receiver): Philox4x32-10 -> one normal;
//   k_rows     one lane per (task, pair slot): the row's receivers and tdoa, consecutive lanes write consecutive rows;
//   k_ptr      the slab's group_ptr;   pos_core: thr_pos's kernel on the slab;
//   k_collect  one lane per task: dx, dy, e, status and iters into per-task columns, and the kept tasks' outputs;
//   k_keep_rows  the kept tasks' rows as the solver saw them;
//   k_reduce   one workgroup per cell: wave 0 sums its trials in the order the header states, then all four waves sort
//              e in LDS (bitonic, padded with +inf to a power of two) for the two order statistics.
// Nothing is accumulated across workgroups, no atomic: a repeated call returns the same bits, whatever the slab size.
// All launches go to the null stream; temporaries are freed by hipFree, which waits for it.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>

#include "../../include/thrifty_hip.h"
#include "pos_lm.hpp"
#include "post_stages.hpp"
#include "seg_reduce.hpp"

// a row's distances and a trial's error are thr_pos's and NumPy's expressions: no a * b + c may become an fma in this
// file (the build also passes -ffp-contract=off for it, thrifty_amd/build.py)
#pragma clang fp contract(off)

namespace {

using thr::DevBuf;
using thr::Event;
using thr::poslm::kNonfinite;
using thr::poslm::kOk;
using thr::poslm::kSpeedOfLight;
using thr::seg::launch;

constexpr int kBlock = thr::seg::kBlock;
constexpr int kWave = 64;
constexpr int kMaxReceivers = 64;
constexpr int kMaxTrials = THR_COV_MAX_TRIALS;
constexpr long long kMaxCells = 1ll << 20;
constexpr long long kMaxTasks = 1ll << 28;
static_assert(THR_COV_N_OUTPUTS <= thr::seg::kMaxOutputs, "the result handle holds every output");
static_assert((kMaxTrials & (kMaxTrials - 1)) == 0, "the sort pads to a power of two");

// ---------------------------------------------------------------- Philox4x32-10 and the normal
struct U4 {
    uint32_t x, y, z, w;
};
__host__ __device__ inline U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = uint64_t(0xD2511F53u) * c.x, p1 = uint64_t(0xCD9E8D57u) * c.z;
        c = U4{uint32_t(p1 >> 32) ^ c.y ^ k0, uint32_t(p1), uint32_t(p0 >> 32) ^ c.w ^ k1, uint32_t(p0)};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}
__device__ __forceinline__ double normal_of(uint32_t cell, uint32_t trial, uint32_t rx, uint32_t k0, uint32_t k1) {
    const U4 w = philox4x32_10(U4{cell, trial, rx, 0u}, k0, k1);
    const double u1 = (double(w.x) + 1.0) * 0x1p-32, u2 = double(w.y) * 0x1p-32;
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

struct Raster {
    double lo0, lo1, step0, step1;
    int nx, ny;
};
// the centre of column / row i: lo + (i + 0.5) * step
__device__ __forceinline__ double centre(double lo, double step, int i) { return lo + (double(i) + 0.5) * step; }

// the receiver of the n-th set bit of mask (n < popcount)
__device__ __forceinline__ int nth_bit(unsigned long long mask, int n) {
    for (int k = 0; k < n; ++k) mask &= mask - 1;
    return __ffsll((long long)mask) - 1;
}

// ---------------------------------------------------------------- cells
struct CellOut {
    double *cx, *cy, *pred;
    int *n_heard, *flags, *m_rows, *covered;
    long long* m_rows64;  // the same counts, for the scan
    unsigned long long* mask;
};

__global__ __launch_bounds__(kBlock) void k_cells(Raster R, int n_rx, const double* __restrict__ xy,
                                                  const double* __restrict__ sigma, double range_m, CellOut o) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c < R.nx) o.cx[c] = centre(R.lo0, R.step0, c);
    if (c < R.ny) o.cy[c] = centre(R.lo1, R.step1, c);
    if (c >= R.nx * R.ny) return;
    const double px = centre(R.lo0, R.step0, c % R.nx), py = centre(R.lo1, R.step1, c / R.nx);
    unsigned long long mask = 0;
    for (int r = 0; r < n_rx; ++r) {
        const double dx = xy[2 * r] - px, dy = xy[2 * r + 1] - py;
        if (range_m <= 0.0 || sqrt(dx * dx + dy * dy) <= range_m) mask |= 1ull << r;
    }
    const int h = __popcll(mask);
    const bool covered = h >= 3;
    o.mask[c] = mask;
    o.n_heard[c] = h;
    o.m_rows[c] = covered ? h * (h - 1) / 2 : 0;
    o.m_rows64[c] = covered ? h * (h - 1) / 2 : 0;
    o.covered[c] = covered ? 1 : 0;
    double dop = NAN, sxx = NAN, sxy = NAN, syy = NAN;
    int flags = covered ? 0 : THR_COV_UNCOVERED;
    if (covered) {
        // N over the rows (a < b, a-major)
        double n00 = 0.0, n01 = 0.0, n11 = 0.0;
        for (int a = 0; a < n_rx; ++a) {
            if (!((mask >> a) & 1ull)) continue;
            const double ax = xy[2 * a] - px, ay = xy[2 * a + 1] - py, da = sqrt(ax * ax + ay * ay);
            for (int b = a + 1; b < n_rx; ++b) {
                if (!((mask >> b) & 1ull)) continue;
                const double bx = xy[2 * b] - px, by = xy[2 * b + 1] - py, db = sqrt(bx * bx + by * by);
                const double gx = ax / da - bx / db, gy = ay / da - by / db;
                n00 += gx * gx;
                n01 += gx * gy;
                n11 += gy * gy;
            }
        }
        dop = thr::poslm::dop_of(thr::poslm::Sums{0.0, n00, n01, n11, 0.0, 0.0});
        if (dop == -1.0) {
            flags |= THR_COV_DEGENERATE;
        } else {
            // M = sum_r sigma_r^2 u_r u_r'; a row (a, b) naming r gives s g_row = e_r - e_other either way round
            double m00 = 0.0, m01 = 0.0, m11 = 0.0;
            for (int r = 0; r < n_rx; ++r) {
                if (!((mask >> r) & 1ull)) continue;
                const double rx = xy[2 * r] - px, ry = xy[2 * r + 1] - py, dr = sqrt(rx * rx + ry * ry);
                double ux = 0.0, uy = 0.0;
                for (int b = 0; b < n_rx; ++b) {
                    if (b == r || !((mask >> b) & 1ull)) continue;
                    const double bx = xy[2 * b] - px, by = xy[2 * b + 1] - py, db = sqrt(bx * bx + by * by);
                    ux += rx / dr - bx / db;
                    uy += ry / dr - by / db;
                }
                const double s2 = sigma[r] * sigma[r];
                m00 += s2 * (ux * ux);
                m01 += s2 * (ux * uy);
                m11 += s2 * (uy * uy);
            }
            const double det = n00 * n11 - n01 * n01;
            const double i00 = n11 / det, i01 = -n01 / det, i11 = n00 / det;
            const double t00 = i00 * m00 + i01 * m01, t01 = i00 * m01 + i01 * m11;
            const double t10 = i01 * m00 + i11 * m01, t11 = i01 * m01 + i11 * m11;
            sxx = t00 * i00 + t01 * i01;
            sxy = t00 * i01 + t01 * i11;
            syy = t10 * i01 + t11 * i11;
        }
    }
    o.flags[c] = flags;
    double* p = o.pred + size_t(c) * 5;
    p[0] = dop, p[1] = sxx, p[2] = sxy, p[3] = syy, p[4] = sqrt(sxx + syy);
}

// the covered cells in ascending order; cov_idx is the exclusive scan of the covered flags
__global__ __launch_bounds__(kBlock) void k_scatter(int n_cells, const int* __restrict__ covered,
                                                    const int* __restrict__ cov_idx, int* __restrict__ cov_cell) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c < n_cells && covered[c]) cov_cell[cov_idx[c]] = c;
}

// ---------------------------------------------------------------- the task layout
struct Layout {
    const int* cov_cell;        // [n_cov]
    const int* m_rows;          // [n_cells]
    const long long* row_base;  // [n_cells + 1]: exclusive scan of m_rows
    int n_cov, n_cells, T;
    // the first row of task k among the rows of all tasks; k = n_cov * T gives their number
    __device__ __forceinline__ long long row_of(long long k) const {
        const long long ci = k / T;
        if (ci >= n_cov) return (long long)T * row_base[n_cells];
        const int c = cov_cell[ci];
        return (long long)T * row_base[c] + (k % T) * (long long)m_rows[c];
    }
};

__global__ __launch_bounds__(kBlock) void k_noise(Layout L, long long k0, int n_slab, int n_rx, const double* __restrict__ sigma,
                                                  uint32_t seed_lo, uint32_t seed_hi, double* __restrict__ noise) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (long long)n_slab * n_rx) return;
    const long long k = k0 + i / n_rx;
    const int r = int(i % n_rx);
    const int c = L.cov_cell[k / L.T];
    noise[i] = sigma[r] * normal_of(uint32_t(c), uint32_t(k % L.T), uint32_t(r), seed_lo, seed_hi);
}

// lane = (task, pair slot q < m_max); slot q of a cell with h hearing receivers is pair (i, j), i < j, a-major
__global__ __launch_bounds__(kBlock) void k_rows(Layout L, Raster R, long long k0, int n_slab, int n_rx, int m_max,
                                                 const double* __restrict__ xy, const unsigned long long* __restrict__ heard,
                                                 const double* __restrict__ noise, int* __restrict__ rx0,
                                                 int* __restrict__ rx1, double* __restrict__ tdoa, double* __restrict__ snr) {
    const long long idx = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= (long long)n_slab * m_max) return;
    const long long kl = idx / m_max, k = k0 + kl;
    const int q = int(idx % m_max);
    const int c = L.cov_cell[k / L.T];
    if (q >= L.m_rows[c]) return;
    const unsigned long long mask = heard[c];
    const int h = __popcll(mask);
    int i = 0, rem = q;
    while (rem >= h - 1 - i) {
        rem -= h - 1 - i;
        ++i;
    }
    const int a = nth_bit(mask, i), b = nth_bit(mask, i + 1 + rem);
    const double px = centre(R.lo0, R.step0, c % R.nx), py = centre(R.lo1, R.step1, c / R.nx);
    const double ax = xy[2 * a] - px, ay = xy[2 * a + 1] - py, bx = xy[2 * b] - px, by = xy[2 * b + 1] - py;
    const double da = sqrt(ax * ax + ay * ay), db = sqrt(bx * bx + by * by);
    const double na = noise[kl * n_rx + a], nb = noise[kl * n_rx + b];
    const long long row = L.row_of(k) - L.row_of(k0) + q;
    rx0[row] = a;
    rx1[row] = b;
    tdoa[row] = ((da - db) + (na - nb)) / kSpeedOfLight;
    snr[row] = 1.0;
}

__global__ __launch_bounds__(kBlock) void k_ptr(Layout L, long long k0, int n_slab, long long* __restrict__ ptr) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i <= n_slab) ptr[i] = L.row_of(k0 + i) - L.row_of(k0);
}

struct Trials {  // [tasks]
    double *dx, *dy, *err;
    int *status, *iters;
};
struct Keep {  // the kept tasks are kk0 .. kk1 - 1
    long long kk0, kk1;
    long long* ptr;
    int *rx0, *rx1, *status, *iters;
    double *tdoa, *noise, *pos, *err;
};

__global__ __launch_bounds__(kBlock) void k_collect(Layout L, Raster R, long long k0, int n_slab, int n_rx,
                                                    const double* __restrict__ pos, const int* __restrict__ status,
                                                    const int* __restrict__ iters, const double* __restrict__ noise, Trials t,
                                                    Keep keep) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_slab) return;
    const long long k = k0 + i;
    const int c = L.cov_cell[k / L.T];
    const double x = pos[2 * size_t(i)], y = pos[2 * size_t(i) + 1];
    const int st = status[i];
    const double dx = x - centre(R.lo0, R.step0, c % R.nx), dy = y - centre(R.lo1, R.step1, c / R.nx);
    const double e = (st == kNonfinite || !isfinite(x) || !isfinite(y)) ? INFINITY : sqrt(dx * dx + dy * dy);
    t.dx[k] = dx, t.dy[k] = dy, t.err[k] = e;
    t.status[k] = st, t.iters[k] = iters[i];
    if (k >= keep.kk0 && k < keep.kk1) {
        const long long kk = k - keep.kk0;
        keep.pos[2 * kk] = x, keep.pos[2 * kk + 1] = y;
        keep.status[kk] = st, keep.iters[kk] = iters[i], keep.err[kk] = e;
        for (int r = 0; r < n_rx; ++r) keep.noise[kk * n_rx + r] = noise[size_t(i) * n_rx + r];
        keep.ptr[kk] = L.row_of(k) - L.row_of(keep.kk0);
        if (k + 1 == keep.kk1) keep.ptr[kk + 1] = L.row_of(k + 1) - L.row_of(keep.kk0);
    }
}

// the rows of the slab's kept tasks ka .. kb - 1, copied as the solver saw them
__global__ __launch_bounds__(kBlock) void k_keep_rows(Layout L, long long k0, long long ka, long long kb, int m_max,
                                                      const int* __restrict__ rx0, const int* __restrict__ rx1,
                                                      const double* __restrict__ tdoa, Keep keep) {
    const long long idx = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= (kb - ka) * m_max) return;
    const long long k = ka + idx / m_max;
    const int q = int(idx % m_max);
    if (q >= L.m_rows[L.cov_cell[k / L.T]]) return;
    const long long src = L.row_of(k) - L.row_of(k0) + q, dst = L.row_of(k) - L.row_of(keep.kk0) + q;
    keep.rx0[dst] = rx0[src];
    keep.rx1[dst] = rx1[src];
    keep.tdoa[dst] = tdoa[src];
}

// ---------------------------------------------------------------- per-cell reduction and sort: workgroup = cell
__global__ __launch_bounds__(kBlock) void k_reduce(int T, double gross_m, const int* __restrict__ covered,
                                                   const int* __restrict__ cov_idx, Trials t, int* __restrict__ flags,
                                                   int* __restrict__ counts, long long* __restrict__ iters_sum,
                                                   double* __restrict__ stats) {
    __shared__ double e_lds[kMaxTrials];
    const int c = blockIdx.x, tid = threadIdx.x;
    int* cnt = counts + size_t(c) * 6;
    double* st = stats + size_t(c) * 8;
    if (!covered[c]) {  // the whole workgroup alike
        if (tid < 6) cnt[tid] = 0;
        if (tid < 8) st[tid] = NAN;
        if (tid == 0) iters_sum[c] = 0;
        return;
    }
    const size_t base = size_t(cov_idx[c]) * size_t(T);
    int P = 1;
    while (P < T) P <<= 1;
    for (int i = tid; i < P; i += kBlock) e_lds[i] = i < T ? t.err[base + i] : INFINITY;

    if (tid < kWave) {  // wave 0: the sums, lane l takes trials l, l + 64, ... in order
        double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        int n_ok = 0, n_bound = 0, n_unconv = 0, n_nonf = 0, n_good = 0;
        long long it = 0;
        for (int i = tid; i < T; i += kWave) {
            const int status = t.status[base + i];
            n_ok += status == kOk;
            n_bound += status == thr::poslm::kAtBound;
            n_unconv += status == thr::poslm::kUnconverged;
            n_nonf += status == kNonfinite;
            it += t.iters[base + i];
            if (status == kOk && t.err[base + i] <= gross_m) {
                const double dx = t.dx[base + i], dy = t.dy[base + i];
                ++n_good;
                s[0] += dx, s[1] += dy, s[2] += dx * dx, s[3] += dx * dy, s[4] += dy * dy;
            }
        }
        for (int d = kWave / 2; d >= 1; d >>= 1) {  // lane[l] += lane[l + d], l < d: lane 0 ends with the stated tree
#pragma unroll
            for (int k = 0; k < 5; ++k) s[k] = s[k] + __shfl_down(s[k], d, kWave);
            n_ok += __shfl_down(n_ok, d, kWave);
            n_bound += __shfl_down(n_bound, d, kWave);
            n_unconv += __shfl_down(n_unconv, d, kWave);
            n_nonf += __shfl_down(n_nonf, d, kWave);
            n_good += __shfl_down(n_good, d, kWave);
            it += __shfl_down(it, d, kWave);
        }
        if (tid == 0) {
            const int n_gross = T - n_good;
            cnt[0] = n_ok, cnt[1] = n_bound, cnt[2] = n_unconv, cnt[3] = n_nonf, cnt[4] = n_good, cnt[5] = n_gross;
            iters_sum[c] = it;
            const double n = double(n_good);
            const double sxx = s[2] / n, sxy = s[3] / n, syy = s[4] / n;
            st[0] = n_good ? s[0] / n : NAN;
            st[1] = n_good ? s[1] / n : NAN;
            st[2] = n_good ? sxx : NAN;
            st[3] = n_good ? sxy : NAN;
            st[4] = n_good ? syy : NAN;
            st[5] = n_good ? sqrt(sxx + syy) : NAN;
            if (n_gross * 2 > T) flags[c] |= THR_COV_LOSSY;
        }
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int i = tid; i < P; i += kBlock) {
                const int p = i ^ j;
                if (p > i) {
                    const double a = e_lds[i], b = e_lds[p];
                    if ((a > b) == ((i & k) == 0)) e_lds[i] = b, e_lds[p] = a;
                }
            }
            __syncthreads();
        }
    if (tid == 0) {
        st[6] = e_lds[(T + 1) / 2 - 1];
        st[7] = e_lds[(95 * T + 99) / 100 - 1];
    }
}

thread_local double g_cov_ms[6] = {0, 0, 0, 0, 0, 0};

int fail(const char* what) { return thr::fail_msg(THR_ERR_ARG, "thr_coverage: %s", what); }

}  // namespace

struct thr_coverage_result : thr::seg::Result {};

extern "C" int thr_coverage(int device_id, int n_rx, const double* rx_coords, const double* sigma_rx,
                            const thr_coverage_opts* opts, thr_coverage_result** result_out,
                            thr_coverage_counts* counts_out) try {
    if (result_out) *result_out = nullptr;
    if (counts_out) std::memset(counts_out, 0, sizeof(*counts_out));
    for (double& t : g_cov_ms) t = 0;
    if (!result_out || !counts_out || !opts || !rx_coords || !sigma_rx) return fail("null argument");
    if (n_rx < 1 || n_rx > kMaxReceivers)
        return thr::fail_msg(THR_ERR_ARG, "thr_coverage: 1 to %d receivers, not %d", kMaxReceivers, n_rx);
    for (int r = 0; r < n_rx; ++r)
        if (!std::isfinite(sigma_rx[r]) || sigma_rx[r] < 0.0)
            return thr::fail_msg(THR_ERR_ARG, "thr_coverage: sigma of receiver %d must be finite and not negative", r);
    thr::PosPlan plan;  // checks the coordinates and x0; the solver's box
    THR_TRY(thr::pos_plan("thr_coverage", n_rx, 2, rx_coords, nullptr, opts->x0, plan));
    for (int k = 0; k < 2; ++k) {
        if (!std::isfinite(opts->lo[k]) || !std::isfinite(opts->hi[k])) return fail("the area's corners must be finite");
        if (!(opts->lo[k] < opts->hi[k])) return fail("the area needs lo < hi on both axes");
    }
    if (opts->nx < 1 || opts->ny < 1 || (long long)opts->nx * opts->ny > kMaxCells)
        return thr::fail_msg(THR_ERR_ARG, "thr_coverage: nx and ny must be at least 1 and nx * ny at most %lld, not %d x %d",
                             kMaxCells, opts->nx, opts->ny);
    if (opts->trials < 1 || opts->trials > kMaxTrials)
        return thr::fail_msg(THR_ERR_ARG, "thr_coverage: trials must lie in 1 .. %d, not %d", kMaxTrials, opts->trials);
    if ((long long)opts->nx * opts->ny * opts->trials > kMaxTasks)
        return thr::fail_msg(THR_ERR_ARG, "thr_coverage: cells x trials may not pass %lld", kMaxTasks);
    if (!(opts->gross_m > 0.0) || !std::isfinite(opts->gross_m)) return fail("gross_m must be positive and finite");
    if (!std::isfinite(opts->range_m)) return fail("range_m must be finite (<= 0: every receiver hears every cell)");
    if (opts->max_iter < 0) return fail("max_iter must not be negative");
    if (opts->slab_groups < 0) return fail("slab_groups must not be negative (0: the default)");
    const int n_cells = opts->nx * opts->ny, T = opts->trials;
    if (opts->keep_count < 0 || opts->keep_count > THR_COV_MAX_KEEP)
        return thr::fail_msg(THR_ERR_ARG, "thr_coverage: keep_count must lie in 0 .. %d, not %d", THR_COV_MAX_KEEP, opts->keep_count);
    if (opts->keep_first < 0 || (long long)opts->keep_first + opts->keep_count > n_cells)
        return thr::fail_msg(THR_ERR_ARG, "thr_coverage: the keep range %d + %d passes the %d cells", opts->keep_first,
                             opts->keep_count, n_cells);
    for (int k = 0; k < 2; ++k)
        if (opts->lo[k] < plan.lo[k] || opts->hi[k] > plan.hi[k])
            return fail("the area must lie inside the solver's box, 10 km beyond the receivers' bounding box");
    const Raster raster{opts->lo[0], opts->lo[1], (opts->hi[0] - opts->lo[0]) / double(opts->nx),
                        (opts->hi[1] - opts->lo[1]) / double(opts->ny), opts->nx, opts->ny};
    const int m_max = n_rx * (n_rx - 1) / 2;
    const size_t task_bytes = size_t(m_max) * 24 + size_t(n_rx) * 8 + 8 + 40;
    long long slab_groups = (long long)(size_t(THR_COV_SLAB_BYTES) / task_bytes);
    if (slab_groups < 1) slab_groups = 1;
    if (opts->slab_groups > 0 && opts->slab_groups < slab_groups) slab_groups = opts->slab_groups;

    THR_TRY(thr::seg::pick_device(device_id));
    thr_coverage_result* R = new thr_coverage_result;
    thr::seg::ResultGuard guard{R};
    R->device = device_id;
    R->n_out = THR_COV_N_OUTPUTS;
    hipStream_t s = nullptr;
    Event ev[5], sv[4];
    for (Event& e : ev) THR_HIP_TRY(e.create());
    for (Event& e : sv) THR_HIP_TRY(e.create());
    for (Event& e : R->ev) THR_HIP_TRY(e.create());
    DevBuf* O = R->out;
    size_t* B = R->bytes;
    const size_t nc = size_t(n_cells);

    // ---- copies in
    DevBuf d_xy, d_sigma;
    THR_HIP_TRY(d_xy.alloc(size_t(n_rx) * 16));
    THR_HIP_TRY(d_sigma.alloc(size_t(n_rx) * 8));
    THR_HIP_TRY(hipEventRecord(ev[0].e, s));
    THR_HIP_TRY(hipMemcpy(d_xy.p, rx_coords, size_t(n_rx) * 16, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipMemcpy(d_sigma.p, sigma_rx, size_t(n_rx) * 8, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipEventRecord(ev[1].e, s));

    // ---- cells, the covered list and the row scan
    THR_HIP_TRY(O[THR_COV_CX].alloc(B[THR_COV_CX] = size_t(opts->nx) * 8));
    THR_HIP_TRY(O[THR_COV_CY].alloc(B[THR_COV_CY] = size_t(opts->ny) * 8));
    THR_HIP_TRY(O[THR_COV_N_HEARD].alloc(B[THR_COV_N_HEARD] = nc * 4));
    THR_HIP_TRY(O[THR_COV_HEARD_MASK].alloc(B[THR_COV_HEARD_MASK] = nc * 8));
    THR_HIP_TRY(O[THR_COV_FLAGS].alloc(B[THR_COV_FLAGS] = nc * 4));
    THR_HIP_TRY(O[THR_COV_PRED].alloc(B[THR_COV_PRED] = nc * 40));
    THR_HIP_TRY(O[THR_COV_COUNTS].alloc(B[THR_COV_COUNTS] = nc * 24));
    THR_HIP_TRY(O[THR_COV_ITERS_SUM].alloc(B[THR_COV_ITERS_SUM] = nc * 8));
    THR_HIP_TRY(O[THR_COV_STATS].alloc(B[THR_COV_STATS] = nc * 64));
    DevBuf d_m, d_m64, d_covered, d_cov_idx, d_row_base, d_cov_cell, d_tmp;
    size_t tmp_bytes = 0;
    THR_HIP_TRY(d_m.alloc(nc * 4));
    THR_HIP_TRY(d_m64.alloc((nc + 1) * 8));
    THR_HIP_TRY(hipMemsetAsync(d_m64.p, 0, (nc + 1) * 8, s));
    THR_HIP_TRY(d_covered.alloc((nc + 1) * 4));
    THR_HIP_TRY(d_cov_idx.alloc((nc + 1) * 4));
    THR_HIP_TRY(d_row_base.alloc((nc + 1) * 8));
    THR_HIP_TRY(d_cov_cell.alloc(nc * 4));
    THR_HIP_TRY(hipMemsetAsync(d_covered.p, 0, (nc + 1) * 4, s));
    const CellOut cells{O[THR_COV_CX].as<double>(),   O[THR_COV_CY].as<double>(), O[THR_COV_PRED].as<double>(),
                        O[THR_COV_N_HEARD].as<int>(), O[THR_COV_FLAGS].as<int>(), d_m.as<int>(),
                        d_covered.as<int>(),          d_m64.as<long long>(),
                        O[THR_COV_HEARD_MASK].as<unsigned long long>()};
    THR_TRY(launch(k_cells, nc, s, raster, n_rx, d_xy.as<double>(), d_sigma.as<double>(), opts->range_m, cells));
    THR_HIP_TRY(thr::with_temp(d_tmp, tmp_bytes, [&](void* t, size_t& b) {
        return hipcub::DeviceScan::ExclusiveSum(t, b, d_covered.as<int>(), d_cov_idx.as<int>(), n_cells + 1, s);
    }));
    THR_HIP_TRY(thr::with_temp(d_tmp, tmp_bytes, [&](void* t, size_t& b) {
        return hipcub::DeviceScan::ExclusiveSum(t, b, d_m64.as<long long>(), d_row_base.as<long long>(), n_cells + 1, s);
    }));
    THR_TRY(launch(k_scatter, nc, s, n_cells, d_covered.as<int>(), d_cov_idx.as<int>(), d_cov_cell.as<int>()));
    int n_cov = 0;
    long long rows_per_trial = 0;
    THR_HIP_TRY(hipMemcpy(&n_cov, d_cov_idx.as<int>() + n_cells, 4, hipMemcpyDeviceToHost));  // synchronises
    THR_HIP_TRY(hipMemcpy(&rows_per_trial, d_row_base.as<long long>() + n_cells, 8, hipMemcpyDeviceToHost));
    int keep_cov[2] = {0, 0};
    long long keep_row[2] = {0, 0};
    const int keep_end = opts->keep_first + opts->keep_count;
    THR_HIP_TRY(hipMemcpy(&keep_cov[0], d_cov_idx.as<int>() + opts->keep_first, 4, hipMemcpyDeviceToHost));
    THR_HIP_TRY(hipMemcpy(&keep_cov[1], d_cov_idx.as<int>() + keep_end, 4, hipMemcpyDeviceToHost));
    THR_HIP_TRY(hipMemcpy(&keep_row[0], d_row_base.as<long long>() + opts->keep_first, 8, hipMemcpyDeviceToHost));
    THR_HIP_TRY(hipMemcpy(&keep_row[1], d_row_base.as<long long>() + keep_end, 8, hipMemcpyDeviceToHost));
    THR_HIP_TRY(hipEventRecord(ev[2].e, s));
    const long long n_tasks = (long long)n_cov * T;
    const Layout L{d_cov_cell.as<int>(), d_m.as<int>(), d_row_base.as<long long>(), n_cov, n_cells, T};
    const long long kk0 = (long long)keep_cov[0] * T, kk1 = (long long)keep_cov[1] * T;
    const size_t keep_tasks = size_t(kk1 - kk0), keep_rows = size_t((keep_row[1] - keep_row[0]) * T);

    // ---- the per-task columns and the kept ones
    DevBuf d_dx, d_dy, d_err, d_status, d_iters;
    THR_HIP_TRY(d_dx.alloc(size_t(n_tasks) * 8));
    THR_HIP_TRY(d_dy.alloc(size_t(n_tasks) * 8));
    THR_HIP_TRY(d_err.alloc(size_t(n_tasks) * 8));
    THR_HIP_TRY(d_status.alloc(size_t(n_tasks) * 4));
    THR_HIP_TRY(d_iters.alloc(size_t(n_tasks) * 4));
    const Trials trials{d_dx.as<double>(), d_dy.as<double>(), d_err.as<double>(), d_status.as<int>(), d_iters.as<int>()};
    THR_HIP_TRY(O[THR_COV_KEEP_PTR].alloc(B[THR_COV_KEEP_PTR] = (keep_tasks + 1) * 8));
    THR_HIP_TRY(O[THR_COV_KEEP_RX0].alloc(B[THR_COV_KEEP_RX0] = keep_rows * 4));
    THR_HIP_TRY(O[THR_COV_KEEP_RX1].alloc(B[THR_COV_KEEP_RX1] = keep_rows * 4));
    THR_HIP_TRY(O[THR_COV_KEEP_TDOA].alloc(B[THR_COV_KEEP_TDOA] = keep_rows * 8));
    THR_HIP_TRY(O[THR_COV_KEEP_NOISE].alloc(B[THR_COV_KEEP_NOISE] = keep_tasks * size_t(n_rx) * 8));
    THR_HIP_TRY(O[THR_COV_KEEP_POS].alloc(B[THR_COV_KEEP_POS] = keep_tasks * 16));
    THR_HIP_TRY(O[THR_COV_KEEP_STATUS].alloc(B[THR_COV_KEEP_STATUS] = keep_tasks * 4));
    THR_HIP_TRY(O[THR_COV_KEEP_ITERS].alloc(B[THR_COV_KEEP_ITERS] = keep_tasks * 4));
    THR_HIP_TRY(O[THR_COV_KEEP_ERR].alloc(B[THR_COV_KEEP_ERR] = keep_tasks * 8));
    THR_HIP_TRY(hipMemsetAsync(O[THR_COV_KEEP_PTR].p, 0, 8, s));  // no kept task: keep_ptr = {0}
    const Keep keep{kk0,
                    kk1,
                    O[THR_COV_KEEP_PTR].as<long long>(),
                    O[THR_COV_KEEP_RX0].as<int>(),
                    O[THR_COV_KEEP_RX1].as<int>(),
                    O[THR_COV_KEEP_STATUS].as<int>(),
                    O[THR_COV_KEEP_ITERS].as<int>(),
                    O[THR_COV_KEEP_TDOA].as<double>(),
                    O[THR_COV_KEEP_NOISE].as<double>(),
                    O[THR_COV_KEEP_POS].as<double>(),
                    O[THR_COV_KEEP_ERR].as<double>()};

    // ---- the slabs
    size_t n_slabs = 0, slab_bytes = 0;
    double ms_synth = 0, ms_solve = 0, ms_collect = 0;
    if (n_tasks) {
        const size_t cap = size_t(std::min(slab_groups, n_tasks));
        const size_t cap_rows = cap * size_t(m_max);
        DevBuf d_noise, d_ptr, d_rx0, d_rx1, d_tdoa, d_snr;
        THR_HIP_TRY(d_noise.alloc(cap * size_t(n_rx) * 8));
        THR_HIP_TRY(d_ptr.alloc((cap + 1) * 8));
        THR_HIP_TRY(d_rx0.alloc(cap_rows * 4));
        THR_HIP_TRY(d_rx1.alloc(cap_rows * 4));
        THR_HIP_TRY(d_tdoa.alloc(cap_rows * 8));
        THR_HIP_TRY(d_snr.alloc(cap_rows * 8));
        slab_bytes = cap * task_bytes + 8;
        for (long long k0 = 0; k0 < n_tasks; k0 += slab_groups, ++n_slabs) {
            const int n_slab = int(std::min(slab_groups, n_tasks - k0));
            THR_HIP_TRY(hipEventRecord(sv[0].e, s));
            THR_TRY(launch(k_noise, size_t(n_slab) * size_t(n_rx), s, L, k0, n_slab, n_rx, d_sigma.as<double>(), opts->seed_lo,
                           opts->seed_hi, d_noise.as<double>()));
            THR_TRY(launch(k_rows, size_t(n_slab) * size_t(m_max), s, L, raster, k0, n_slab, n_rx, m_max, d_xy.as<double>(),
                           O[THR_COV_HEARD_MASK].as<unsigned long long>(), d_noise.as<double>(), d_rx0.as<int>(),
                           d_rx1.as<int>(), d_tdoa.as<double>(), d_snr.as<double>()));
            THR_TRY(launch(k_ptr, size_t(n_slab) + 1, s, L, k0, n_slab, d_ptr.as<long long>()));
            THR_HIP_TRY(hipEventRecord(sv[1].e, s));
            thr::PosOut out;
            THR_TRY(thr::pos_core(n_slab, d_ptr.as<long long>(), d_rx0.as<int>(), d_rx1.as<int>(), d_tdoa.as<double>(),
                                  d_snr.as<double>(), d_xy.as<double>(), 2, plan, int(opts->max_iter), s, out));
            THR_HIP_TRY(hipEventRecord(sv[2].e, s));
            THR_TRY(launch(k_collect, size_t(n_slab), s, L, raster, k0, n_slab, n_rx, out.pos.as<double>(), out.status.as<int>(),
                           out.iters.as<int>(), d_noise.as<double>(), trials, keep));
            const long long ka = std::max(k0, kk0), kb = std::min(k0 + n_slab, kk1);
            if (ka < kb)
                THR_TRY(launch(k_keep_rows, size_t(kb - ka) * size_t(m_max), s, L, k0, ka, kb, m_max, d_rx0.as<int>(),
                               d_rx1.as<int>(), d_tdoa.as<double>(), keep));
            THR_HIP_TRY(hipEventRecord(sv[3].e, s));
            THR_HIP_TRY(hipEventSynchronize(sv[3].e));  // the solver's outputs go out of scope
            float ms[3] = {0, 0, 0};
            for (int k = 0; k < 3; ++k) THR_HIP_TRY(hipEventElapsedTime(&ms[k], sv[k].e, sv[k + 1].e));
            ms_synth += ms[0], ms_solve += ms[1], ms_collect += ms[2];
        }
    }

    // ---- the cells' statistics
    THR_HIP_TRY(hipEventRecord(ev[3].e, s));
    hipLaunchKernelGGL(k_reduce, dim3(unsigned(n_cells)), dim3(kBlock), 0, s, T, opts->gross_m, d_covered.as<int>(),
                       d_cov_idx.as<int>(), trials, O[THR_COV_FLAGS].as<int>(), O[THR_COV_COUNTS].as<int>(),
                       O[THR_COV_ITERS_SUM].as<long long>(), O[THR_COV_STATS].as<double>());
    THR_HIP_TRY(hipGetLastError());
    THR_HIP_TRY(hipEventRecord(ev[4].e, s));
    THR_HIP_TRY(hipEventSynchronize(ev[4].e));  // the temporaries go out of scope
    float ms = 0;
    THR_HIP_TRY(hipEventElapsedTime(&ms, ev[0].e, ev[1].e));
    g_cov_ms[0] = ms;
    THR_HIP_TRY(hipEventElapsedTime(&ms, ev[1].e, ev[2].e));
    g_cov_ms[1] = ms;
    THR_HIP_TRY(hipEventElapsedTime(&ms, ev[3].e, ev[4].e));
    g_cov_ms[4] = ms + ms_collect;
    g_cov_ms[2] = ms_synth;
    g_cov_ms[3] = ms_solve;

    counts_out->cells = nc;
    counts_out->nx = size_t(opts->nx);
    counts_out->ny = size_t(opts->ny);
    counts_out->n_rx = size_t(n_rx);
    counts_out->trials = size_t(T);
    counts_out->covered = size_t(n_cov);
    counts_out->tasks = size_t(n_tasks);
    counts_out->rows = size_t(rows_per_trial) * size_t(T);
    counts_out->slabs = n_slabs;
    counts_out->slab_groups = size_t(slab_groups);
    counts_out->slab_bytes = slab_bytes;
    counts_out->keep_tasks = keep_tasks;
    counts_out->keep_rows = keep_rows;
    *result_out = R;
    guard.r = nullptr;
    return THR_OK;
} catch (const std::bad_alloc&) {
    return thr::fail_msg(THR_ERR_DEVICE, "thr_coverage: out of host memory");
} catch (...) {
    return thr::on_exception("thr_coverage");
}

extern "C" int thr_coverage_fetch(thr_coverage_result* R, int which, void* dst, size_t dst_bytes) try {
    return thr::seg::fetch("thr_coverage_fetch", R, which, dst, dst_bytes, &g_cov_ms[5]);
} catch (...) {
    return thr::on_exception("thr_coverage_fetch");
}

extern "C" void thr_coverage_free(thr_coverage_result* R) { thr::seg::free_result(R); }

extern "C" int thr_debug_coverage_times(double* ms_out) try {
    if (!ms_out) return thr::fail_msg(THR_ERR_ARG, "thr_debug_coverage_times: null argument");
    for (int k = 0; k < 6; ++k) ms_out[k] = g_cov_ms[k];
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_coverage_times");
}
