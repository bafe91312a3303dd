// Global position solve on the device (thr_posg): thr_pos's 2-D solve started not only from the fixed x0 but from the
// lowest local minima of the group's cost surface on a G x G grid over the receivers' surroundings as well; the best
// minimum, the runner-up, and two flags -- the fixed start was wrong, or two positions fit.  The reference's "TODO: use
// analytic solution or previous position as initial value" (pos_est.py).  include/thrifty_hip.h states every rule.
//
// Four kernels:
//   A  k_tasks (task 0)   one 8-lane team per group: thr_pos's own solve from x0 (csrc/pos_lm.hpp);
//   B  k_grid<G>          one wave per group, one wave per workgroup: the surface F in LDS (G^2 doubles), the group's
//                         rows staged in LDS kRowChunk at a time and read as broadcasts; lane l owns the cells
//                         l, l + 64, ...; each cell's sum is one accumulator over the rows in order; with up to
//                         kDistRx receivers a cell's distances are taken once per receiver, not twice per row.  Then the
//                         local-minimum test from LDS and K rounds of a wave-wide minimum over the key (F, c);
//   C  k_tasks (1 .. K)   one team per (group, start): the same solve from the start cell's centre;
//   D  k_pick             one lane per group: at most 9 tasks, compared pairwise in registers.
// Nothing is accumulated across lanes or teams, no atomic: a repeated call returns the same bits.  All launches go to
// the null stream; temporaries are freed by hipFree, which waits for it.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>

#include "../../include/thrifty_hip.h"
#include "lmdif8.hpp"
#include "pos_lm.hpp"
#include "post_stages.hpp"
#include "seg_reduce.hpp"

// a task must return thr_pos's bits and a cell's sum NumPy's: no a * b + c may become an fma in this file (the build
// also passes -ffp-contract=off for it, thrifty_amd/build.py)
#pragma clang fp contract(off)

namespace {

using thr::DevBuf;
using thr::Event;
using namespace thr::poslm;
using thr::seg::launch;
using thr::seg::launch_grid;

constexpr int kBlock = thr::seg::kBlock;  // workgroup size of k_tasks and k_pick (launch() assumes it)
constexpr int kTeams = kBlock / kTeam;     // tasks per workgroup of k_tasks
constexpr int kRegRows = 4;                // rows per lane kept in registers, as k_pos2d
constexpr int kMaxReceivers = 64;
constexpr int kWave = 64;                  // k_grid: one wave per group and per workgroup
constexpr int kRowChunk = THR_POSG_ROW_CHUNK;  // rows staged in LDS at a time
constexpr int kMaxStarts = 8;
constexpr int kMaxTasks = kMaxStarts + 1;
constexpr int kMaxMap = 256;
constexpr int kDistRx = 32;                // up to this many receivers, a cell's distances are taken once per receiver
constexpr double kMaxMargin = 10e3;        // thr_pos's box reaches this far beyond the receivers
static_assert(THR_POSG_N_OUTPUTS <= thr::seg::kMaxOutputs, "the result handle holds every output");
static_assert(kRowChunk <= kWave, "one lane stages one row");

struct Cols {  // the input columns on the device
    const long long* ptr;
    const int *rx0, *rx1;
    const double *tdoa, *snr, *xy;
};
struct Area {  // the search area: the first cell's corner and the cells' size
    double lo0, lo1, step0, step1;
};
struct TaskOut {  // [groups][K + 1]
    double *pos, *dop, *rms;
    int *status, *iters;
};

// the centre of column / row i: lo + (i + 0.5) * step, the form include/thrifty_hip.h gives
__device__ __forceinline__ double centre(double lo, double step, int i) { return lo + (double(i) + 0.5) * step; }

// A, C: team = (group, task task_lo + team % task_n).  Task 0 starts from (x0, y0), task k from start cell k - 1;
// a task without a start cell (-1) does not exist: its team runs along with m == 0.
__global__ __launch_bounds__(kBlock) void k_tasks(Cols c, int n_groups, int K, int G, int task_lo, int task_n,
                                                  const int* __restrict__ start_cell, Area area, double x0, double y0, Box box,
                                                  int max_iter, TaskOut o, double* __restrict__ snr_out) {
    const long long team = ((long long)blockIdx.x * kBlock + threadIdx.x) / kTeam;
    const int j = threadIdx.x & (kTeam - 1);
    const long long gl = team / task_n;
    const bool in_range = gl < n_groups;
    const int g = in_range ? int(gl) : 0, k = task_lo + int(team % task_n);
    bool live = in_range;
    double sx = x0, sy = y0;
    if (in_range && k > 0) {
        const int cell = start_cell[size_t(g) * K + (k - 1)];
        live = cell >= 0;
        if (live) {
            sx = centre(area.lo0, area.step0, cell % G);
            sy = centre(area.lo1, area.step1, cell / G);
        }
    }
    const long long beg = live ? c.ptr[g] : 0;
    const int m = live ? int(c.ptr[g + 1] - beg) : 0;
    const Fit fit = solve_team<false, kRegRows>(live, beg, m, j, c.rx0, c.rx1, c.tdoa, c.snr, nullptr, c.xy, sx, sy, box,
                                                max_iter, AllRows{});
    if (in_range && j == 0) {
        const size_t t = size_t(g) * size_t(K + 1) + size_t(k);
        o.pos[2 * t] = live ? fit.p0 : NAN;
        o.pos[2 * t + 1] = live ? fit.p1 : NAN;
        o.dop[t] = live ? dop_of(fit.cur) : NAN;
        o.rms[t] = live ? sqrt(fit.cur.F / double(fit.m_used)) : NAN;
        o.status[t] = live ? fit.status : THR_POSG_NO_TASK;
        o.iters[t] = live ? fit.iters : 0;
        if (k == 0) snr_out[g] = fit.snr_mean;
    }
}

// (fa, ca) < (fb, cb); false when a NaN is compared
__device__ __forceinline__ bool key_less(double fa, int ca, double fb, int cb) { return fa < fb || (fa == fb && ca < cb); }

// B: workgroup = wave = group.  status0: task 0's status of every group.  n_dist receivers (0: none) have their
// distances from a cell taken once, in dynamic LDS [n_dist][64], and the rows read them: |rx - p| is the same
// expression whichever row names rx, so F keeps its bits and a cell costs n_rx square roots, not two per row.
template <int G>
__global__ __launch_bounds__(kWave) void k_grid(Cols c, const int* __restrict__ status0, int task_stride, int n_dist, Area area, int K,
                                                long long map_first, int map_count, int* __restrict__ start_cell,
                                                double* __restrict__ start_f, int* __restrict__ n_local,
                                                double* __restrict__ map, unsigned char* __restrict__ map_min) {
    constexpr int kCells = G * G, kOwn = kCells / kWave;
    static_assert(kOwn >= 1 && kOwn <= 64, "a lane's local minima are a 64-bit mask");
    __shared__ double F[kCells];
    __shared__ double rows[kRowChunk * 5];
    __shared__ int row_rx[kRowChunk * 2];
    __shared__ double rx_xy[kDistRx * 2];
    extern __shared__ double dist[];
    const int g = blockIdx.x, lane = threadIdx.x;
    const bool mapped = g >= map_first && g - map_first < map_count;
    const size_t map_at = mapped ? size_t(g - map_first) * kCells : 0;
    const int st = status0[size_t(g) * task_stride];
    if (st == kUnderdetermined || st == kNonfinite) {  // the whole wave alike: no grid
        if (lane < K) {
            start_cell[size_t(g) * K + lane] = -1;
            start_f[size_t(g) * K + lane] = NAN;
        }
        if (lane == 0) n_local[g] = 0;
        if (mapped)
            for (int k = 0; k < kOwn; ++k) {
                map[map_at + lane + kWave * k] = NAN;
                map_min[map_at + lane + kWave * k] = 0;
            }
        return;
    }
    const long long beg = c.ptr[g];
    const int m = int(c.ptr[g + 1] - beg);
    for (int k = 0; k < kOwn; ++k) F[lane + kWave * k] = 0.0;
    if (lane < 2 * n_dist) rx_xy[lane] = c.xy[lane];

    // ---- the surface: chunk by chunk, every cell walks the chunk's rows in order
    for (int r0 = 0; r0 < m; r0 += kRowChunk) {
        const int n = m - r0 < kRowChunk ? m - r0 : kRowChunk;
        __syncthreads();  // the chunk before has been read
        if (lane < n) {
            const Row r = load_row(c.rx0, c.rx1, c.tdoa, c.xy, beg + r0 + lane);
            rows[5 * lane] = r.ax, rows[5 * lane + 1] = r.ay, rows[5 * lane + 2] = r.bx, rows[5 * lane + 3] = r.by;
            rows[5 * lane + 4] = r.tc;
            row_rx[2 * lane] = c.rx0[beg + r0 + lane], row_rx[2 * lane + 1] = c.rx1[beg + r0 + lane];
        }
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < kOwn; ++k) {
            const int cell = lane + kWave * k;
            const double px = centre(area.lo0, area.step0, cell % G), py = centre(area.lo1, area.step1, cell / G);
            double acc = F[cell];
            if (n_dist) {
                for (int r = 0; r < n_dist; ++r) {  // residual()'s da / db, once per receiver; the lane reads only its own
                    const double ax = rx_xy[2 * r] - px, ay = rx_xy[2 * r + 1] - py;
                    dist[r * kWave + lane] = sqrt(ax * ax + ay * ay);
                }
                for (int r = 0; r < n; ++r) {
                    const double res = rows[5 * r + 4] - (dist[row_rx[2 * r] * kWave + lane] - dist[row_rx[2 * r + 1] * kWave + lane]);
                    acc += res * res;
                }
            } else {
                for (int r = 0; r < n; ++r) {  // every lane reads the same row: LDS broadcasts
                    const double res = residual(Row{rows[5 * r], rows[5 * r + 1], rows[5 * r + 2], rows[5 * r + 3], rows[5 * r + 4]}, px, py);
                    acc += res * res;
                }
            }
            F[cell] = acc;
        }
    }
    __syncthreads();

    // ---- local minima, from LDS
    unsigned long long mine = 0;  // bit k: this lane's cell k is a local minimum
#pragma unroll 1
    for (int k = 0; k < kOwn; ++k) {
        const int cell = lane + kWave * k, i = cell % G, jr = cell / G;
        const double f = F[cell];
        bool ok = true;
        for (int dj = -1; dj <= 1; ++dj)
            for (int di = -1; di <= 1; ++di) {
                if (di == 0 && dj == 0) continue;
                const int ii = i + di, jj = jr + dj;
                if (ii < 0 || ii >= G || jj < 0 || jj >= G) {
                    ok = ok && f < INFINITY;
                } else {
                    const int nb = jj * G + ii;
                    const double fn = F[nb];
                    ok = ok && (f < fn || (f == fn && nb > cell));
                }
            }
        if (ok) mine |= 1ull << k;
        if (mapped) {
            map[map_at + cell] = f;
            map_min[map_at + cell] = ok ? 1 : 0;
        }
    }
    int count = __popcll(mine);
    for (int d = 1; d < kWave; d <<= 1) count += __shfl_xor(count, d, kWave);
    if (lane == 0) n_local[g] = count;

    // ---- the K lowest of them by (F, c): every round a wave-wide minimum over the keys after the last pick
    double last_f = -INFINITY;
    int last_c = -1;
    for (int s = 0; s < K; ++s) {
        double bf = INFINITY;
        int bc = INT_MAX;
#pragma unroll 1
        for (int k = 0; k < kOwn; ++k) {
            if (!((mine >> k) & 1ull)) continue;
            const int cell = lane + kWave * k;
            const double f = F[cell];
            if (key_less(last_f, last_c, f, cell) && key_less(f, cell, bf, bc)) bf = f, bc = cell;
        }
        for (int d = 1; d < kWave; d <<= 1) {  // identical in all lanes afterwards: the keys are distinct
            const double of = __shfl_xor(bf, d, kWave);
            const int oc = __shfl_xor(bc, d, kWave);
            if (key_less(of, oc, bf, bc)) bf = of, bc = oc;
        }
        if (lane == 0) {
            start_cell[size_t(g) * K + s] = bc == INT_MAX ? -1 : bc;
            start_f[size_t(g) * K + s] = bc == INT_MAX ? NAN : bf;
        }
        last_f = bf, last_c = bc;
    }
}

struct Picked {  // the per-group outputs
    double *pos, *dop, *rms, *pos2, *rms2;
    int *status, *task, *n_minima, *flags;
};

// D: one lane per group.  Every loop runs to kMaxTasks with constant indices: the tasks stay in registers.
__global__ __launch_bounds__(kBlock) void k_pick(int n_groups, int K, TaskOut t, double merge_m, double ratio, double floor_m,
                                                 Picked o) {
    const int g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= n_groups) return;
    const size_t base = size_t(g) * size_t(K + 1);
    double x[kMaxTasks], y[kMaxTasks], rms[kMaxTasks];
    bool elig[kMaxTasks], dup[kMaxTasks], first[kMaxTasks];
#pragma unroll
    for (int a = 0; a < kMaxTasks; ++a) {
        const bool there = a <= K;
        x[a] = there ? t.pos[2 * (base + a)] : NAN;
        y[a] = there ? t.pos[2 * (base + a) + 1] : NAN;
        rms[a] = there ? t.rms[base + a] : NAN;
        elig[a] = there && t.status[base + a] == kOk;
    }
    int best = -1, n_minima = 0;
#pragma unroll
    for (int a = 0; a < kMaxTasks; ++a) {
        bool any_before = false, duplicate = false;
#pragma unroll
        for (int b = 0; b < kMaxTasks; ++b) {
            if (b == a) continue;
            const bool before = elig[b] && (rms[b] < rms[a] || (rms[b] == rms[a] && b < a));
            const double dx = x[a] - x[b], dy = y[a] - y[b];
            any_before = any_before || before;
            duplicate = duplicate || (before && sqrt(dx * dx + dy * dy) <= merge_m);
        }
        first[a] = elig[a] && !any_before;
        dup[a] = duplicate;
        if (first[a]) best = a;
        if (elig[a] && !duplicate) ++n_minima;
    }
    int second = -1;
    double second_rms = INFINITY;
#pragma unroll
    for (int a = 0; a < kMaxTasks; ++a)  // ascending a: equal rms keeps the lower task
        if (elig[a] && !dup[a] && !first[a] && (second < 0 || rms[a] < second_rms)) second = a, second_rms = rms[a];
    double bx = x[0], by = y[0], brms = rms[0], sx = NAN, sy = NAN;
#pragma unroll
    for (int a = 0; a < kMaxTasks; ++a) {
        if (a == best) bx = x[a], by = y[a], brms = rms[a];
        if (a == second) sx = x[a], sy = y[a];
    }
    int flags = 0;
    if (best < 0) flags |= THR_POSG_NO_MINIMUM;
    {
        const double dx = bx - x[0], dy = by - y[0];
        if (!elig[0] || !(sqrt(dx * dx + dy * dy) <= merge_m)) flags |= THR_POSG_MOVED;
    }
    if (second >= 0 && second_rms <= fmax(ratio * brms, floor_m)) flags |= THR_POSG_AMBIGUOUS;
    const int chosen = best < 0 ? 0 : best;
    o.pos[2 * size_t(g)] = bx;
    o.pos[2 * size_t(g) + 1] = by;
    o.dop[g] = t.dop[base + chosen];
    o.status[g] = t.status[base + chosen];
    o.rms[g] = brms;
    o.task[g] = chosen;
    o.pos2[2 * size_t(g)] = sx;
    o.pos2[2 * size_t(g) + 1] = sy;
    o.rms2[g] = second >= 0 ? second_rms : NAN;
    o.n_minima[g] = n_minima;
    o.flags[g] = flags;
}

template <int G>
int launch_k_grid(int ng, hipStream_t s, Cols C, const int* status0, int task_stride, int n_dist, Area area, int K, long long map_first,
                  int map_count, int* start_cell, double* start_f, int* n_local, double* map, unsigned char* map_min) {
    hipLaunchKernelGGL(k_grid<G>, dim3(unsigned(ng)), dim3(kWave), size_t(n_dist) * kWave * sizeof(double), s, C, status0, task_stride,
                       n_dist, area, K, map_first, map_count,
                       start_cell, start_f, n_local, map, map_min);
    THR_HIP_TRY(hipGetLastError());
    return THR_OK;
}

thread_local double g_posg_ms[6] = {0, 0, 0, 0, 0, 0};

}  // namespace

struct thr_posg_result : thr::seg::Result {};

extern "C" int thr_posg(int device_id, size_t n_groups, const int64_t* group_ptr, const int32_t* row_rx0,
                        const int32_t* row_rx1, const double* row_tdoa, const double* row_snr, int n_rx, int dims,
                        const double* rx_coords, const thr_posg_opts* opts, thr_posg_result** result_out,
                        thr_posg_counts* counts_out) try {
    if (result_out) *result_out = nullptr;
    if (counts_out) std::memset(counts_out, 0, sizeof(*counts_out));
    for (double& t : g_posg_ms) t = 0;
    if (!result_out || !counts_out || !opts || !group_ptr || !rx_coords) return thr::fail_msg(THR_ERR_ARG, "thr_posg: null argument");
    if (dims != 2) return thr::fail_msg(THR_ERR_ARG, "thr_posg: 2 dimensions, not %d", dims);
    if (n_rx < 1 || n_rx > kMaxReceivers) return thr::fail_msg(THR_ERR_ARG, "thr_posg: 1 to %d receivers, not %d", kMaxReceivers, n_rx);
    if (opts->max_iter < 0) return thr::fail_msg(THR_ERR_ARG, "thr_posg: max_iter must not be negative");
    if (opts->grid != 16 && opts->grid != 32 && opts->grid != 64)
        return thr::fail_msg(THR_ERR_ARG, "thr_posg: grid must be 16, 32 or 64, not %d", opts->grid);
    if (opts->starts < 1 || opts->starts > kMaxStarts)
        return thr::fail_msg(THR_ERR_ARG, "thr_posg: starts must lie in 1 .. %d, not %d", kMaxStarts, opts->starts);
    if (!(opts->margin_m > 0.0 && opts->margin_m <= kMaxMargin))
        return thr::fail_msg(THR_ERR_ARG, "thr_posg: margin_m must lie in (0, %g] metres", kMaxMargin);
    if (!(opts->merge_m > 0.0) || !std::isfinite(opts->merge_m)) return thr::fail_msg(THR_ERR_ARG, "thr_posg: merge_m must be positive and finite");
    if (!(opts->ratio >= 1.0) || !std::isfinite(opts->ratio)) return thr::fail_msg(THR_ERR_ARG, "thr_posg: ratio must be at least 1 and finite");
    if (!(opts->floor_m >= 0.0) || !std::isfinite(opts->floor_m))
        return thr::fail_msg(THR_ERR_ARG, "thr_posg: floor_m must be finite and not negative (0: the ratio alone)");
    if (n_groups > size_t(1) << 28 || n_groups * size_t(opts->starts + 1) > size_t(1) << 28)
        return thr::fail_msg(THR_ERR_ARG, "thr_posg: too many groups or tasks");
    if (opts->map_count < 0 || opts->map_count > kMaxMap)
        return thr::fail_msg(THR_ERR_ARG, "thr_posg: map_count must lie in 0 .. %d, not %d", kMaxMap, opts->map_count);
    if (opts->map_first < 0 || uint64_t(opts->map_first) + uint64_t(opts->map_count) > uint64_t(n_groups))
        return thr::fail_msg(THR_ERR_ARG, "thr_posg: the map range %lld + %d passes the %zu groups", (long long)opts->map_first,
                             opts->map_count, n_groups);

    // ---- everything a kernel will index with is checked here, before anything is launched
    if (group_ptr[0] != 0) return thr::fail_msg(THR_ERR_ARG, "thr_posg: group_ptr[0] must be 0");
    for (size_t g = 0; g < n_groups; ++g) {
        const int64_t len = group_ptr[g + 1] - group_ptr[g];
        if (len < 0) return thr::fail_msg(THR_ERR_ARG, "thr_posg: group_ptr decreases at group %zu", g);
        if (len > (int64_t(1) << 24)) return thr::fail_msg(THR_ERR_ARG, "thr_posg: group %zu is too long", g);
    }
    const size_t n_rows = size_t(group_ptr[n_groups]);
    if (n_rows > size_t(1) << 30) return thr::fail_msg(THR_ERR_ARG, "thr_posg: too many rows");
    if (n_rows && (!row_rx0 || !row_rx1 || !row_tdoa || !row_snr)) return thr::fail_msg(THR_ERR_ARG, "thr_posg: null argument");
    for (size_t i = 0; i < n_rows; ++i)
        if (row_rx0[i] < 0 || row_rx0[i] >= n_rx || row_rx1[i] < 0 || row_rx1[i] >= n_rx)
            return thr::fail_msg(THR_ERR_ARG, "thr_posg: row %zu names receivers %d and %d of %d", i, row_rx0[i], row_rx1[i], n_rx);
    thr::PosPlan plan;
    THR_TRY(thr::pos_plan("thr_posg", n_rx, dims, rx_coords, nullptr, opts->x0, plan));
    const Box box{plan.lo[0], plan.lo[1], plan.hi[0], plan.hi[1]};
    const double x0 = plan.start[0], y0 = plan.start[1];
    const int G = opts->grid, K = opts->starts, T = K + 1;
    double lo[2], hi[2];
    for (int k = 0; k < 2; ++k) {
        lo[k] = hi[k] = rx_coords[k];
        for (int r = 1; r < n_rx; ++r) {
            lo[k] = std::fmin(lo[k], rx_coords[2 * r + k]);
            hi[k] = std::fmax(hi[k], rx_coords[2 * r + k]);
        }
        lo[k] = lo[k] - opts->margin_m;
        hi[k] = hi[k] + opts->margin_m;
    }
    const Area area{lo[0], lo[1], (hi[0] - lo[0]) / double(G), (hi[1] - lo[1]) / double(G)};

    THR_TRY(thr::seg::pick_device(device_id));
    thr_posg_result* R = new thr_posg_result;
    thr::seg::ResultGuard guard{R};
    R->device = device_id;
    R->n_out = THR_POSG_N_OUTPUTS;
    hipStream_t s = nullptr;
    Event ev[6];
    for (Event& e : ev) THR_HIP_TRY(e.create());
    for (Event& e : R->ev) THR_HIP_TRY(e.create());
    const int ng = int(n_groups);
    const size_t nt = n_groups * size_t(T), ns = n_groups * size_t(K), n_map = size_t(opts->map_count) * size_t(G) * size_t(G);

    // ---- copies in
    DevBuf d_ptr, d_rx0, d_rx1, d_tdoa, d_snr, d_xy;
    THR_HIP_TRY(d_ptr.alloc((n_groups + 1) * 8));
    THR_HIP_TRY(d_rx0.alloc(n_rows * 4));
    THR_HIP_TRY(d_rx1.alloc(n_rows * 4));
    THR_HIP_TRY(d_tdoa.alloc(n_rows * 8));
    THR_HIP_TRY(d_snr.alloc(n_rows * 8));
    THR_HIP_TRY(d_xy.alloc(size_t(n_rx) * 16));
    THR_HIP_TRY(hipEventRecord(ev[0].e, s));
    THR_HIP_TRY(hipMemcpy(d_ptr.p, group_ptr, (n_groups + 1) * 8, hipMemcpyHostToDevice));
    if (n_rows) {
        THR_HIP_TRY(hipMemcpy(d_rx0.p, row_rx0, n_rows * 4, hipMemcpyHostToDevice));
        THR_HIP_TRY(hipMemcpy(d_rx1.p, row_rx1, n_rows * 4, hipMemcpyHostToDevice));
        THR_HIP_TRY(hipMemcpy(d_tdoa.p, row_tdoa, n_rows * 8, hipMemcpyHostToDevice));
        THR_HIP_TRY(hipMemcpy(d_snr.p, row_snr, n_rows * 8, hipMemcpyHostToDevice));
    }
    THR_HIP_TRY(hipMemcpy(d_xy.p, rx_coords, size_t(n_rx) * 16, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipEventRecord(ev[1].e, s));
    const Cols C{d_ptr.as<long long>(), d_rx0.as<int>(), d_rx1.as<int>(), d_tdoa.as<double>(), d_snr.as<double>(), d_xy.as<double>()};
    DevBuf* O = R->out;

    // ---- A: task 0, thr_pos's own solve
    THR_HIP_TRY(O[THR_POSG_TASK_POS].alloc(nt * 16));
    for (int w : {THR_POSG_TASK_DOP, THR_POSG_TASK_RMS}) THR_HIP_TRY(O[w].alloc(nt * 8));
    for (int w : {THR_POSG_TASK_STATUS, THR_POSG_TASK_ITERS}) THR_HIP_TRY(O[w].alloc(nt * 4));
    THR_HIP_TRY(O[THR_POSG_SNR].alloc(n_groups * 8));
    THR_HIP_TRY(O[THR_POSG_START_CELL].alloc(ns * 4));
    THR_HIP_TRY(O[THR_POSG_START_F].alloc(ns * 8));
    THR_HIP_TRY(O[THR_POSG_N_LOCAL].alloc(n_groups * 4));
    THR_HIP_TRY(O[THR_POSG_MAP].alloc(n_map * 8));
    THR_HIP_TRY(O[THR_POSG_MAP_MIN].alloc(n_map));
    const TaskOut tasks{O[THR_POSG_TASK_POS].as<double>(), O[THR_POSG_TASK_DOP].as<double>(), O[THR_POSG_TASK_RMS].as<double>(),
                        O[THR_POSG_TASK_STATUS].as<int>(), O[THR_POSG_TASK_ITERS].as<int>()};
    int* start_cell = O[THR_POSG_START_CELL].as<int>();
    if (ng)
        THR_TRY(launch_grid(k_tasks, dim3(unsigned((n_groups + kTeams - 1) / kTeams)), s, C, ng, K, G, 0, 1, start_cell, area, x0, y0,
                            box, int(opts->max_iter), tasks, O[THR_POSG_SNR].as<double>()));
    THR_HIP_TRY(hipEventRecord(ev[2].e, s));

    // ---- B: the surface, its local minima, the starts
    if (ng) {
        auto* grid_fn = G == 16 ? launch_k_grid<16> : (G == 32 ? launch_k_grid<32> : launch_k_grid<64>);
        THR_TRY(grid_fn(ng, s, C, tasks.status, T, n_rx <= kDistRx ? n_rx : 0, area, K, (long long)opts->map_first, int(opts->map_count), start_cell,
                        O[THR_POSG_START_F].as<double>(), O[THR_POSG_N_LOCAL].as<int>(), O[THR_POSG_MAP].as<double>(),
                        O[THR_POSG_MAP_MIN].as<unsigned char>()));
    }
    THR_HIP_TRY(hipEventRecord(ev[3].e, s));

    // ---- C: tasks 1 .. K
    if (ng)
        THR_TRY(launch_grid(k_tasks, dim3(unsigned((ns + kTeams - 1) / kTeams)), s, C, ng, K, G, 1, K, start_cell, area, x0, y0, box,
                            int(opts->max_iter), tasks, O[THR_POSG_SNR].as<double>()));
    THR_HIP_TRY(hipEventRecord(ev[4].e, s));

    // ---- D: the choice
    for (int w : {THR_POSG_POS, THR_POSG_POS2}) THR_HIP_TRY(O[w].alloc(n_groups * 16));
    for (int w : {THR_POSG_DOP, THR_POSG_RMS, THR_POSG_RMS2}) THR_HIP_TRY(O[w].alloc(n_groups * 8));
    for (int w : {THR_POSG_STATUS, THR_POSG_TASK, THR_POSG_N_MINIMA, THR_POSG_FLAGS}) THR_HIP_TRY(O[w].alloc(n_groups * 4));
    const Picked picked{O[THR_POSG_POS].as<double>(),  O[THR_POSG_DOP].as<double>(), O[THR_POSG_RMS].as<double>(),
                        O[THR_POSG_POS2].as<double>(), O[THR_POSG_RMS2].as<double>(), O[THR_POSG_STATUS].as<int>(),
                        O[THR_POSG_TASK].as<int>(),    O[THR_POSG_N_MINIMA].as<int>(), O[THR_POSG_FLAGS].as<int>()};
    THR_TRY(launch(k_pick, n_groups, s, ng, K, tasks, opts->merge_m, opts->ratio, opts->floor_m, picked));
    THR_HIP_TRY(hipEventRecord(ev[5].e, s));
    THR_HIP_TRY(hipEventSynchronize(ev[5].e));  // the temporaries go out of scope
    for (int k = 0; k < 5; ++k) {
        float ms = 0;
        THR_HIP_TRY(hipEventElapsedTime(&ms, ev[k].e, ev[k + 1].e));
        g_posg_ms[k] = ms;
    }

    size_t* B = R->bytes;
    B[THR_POSG_POS] = B[THR_POSG_POS2] = n_groups * 16;
    B[THR_POSG_DOP] = B[THR_POSG_RMS] = B[THR_POSG_RMS2] = B[THR_POSG_SNR] = n_groups * 8;
    B[THR_POSG_STATUS] = B[THR_POSG_TASK] = B[THR_POSG_N_MINIMA] = B[THR_POSG_FLAGS] = B[THR_POSG_N_LOCAL] = n_groups * 4;
    B[THR_POSG_START_CELL] = ns * 4;
    B[THR_POSG_START_F] = ns * 8;
    B[THR_POSG_TASK_POS] = nt * 16;
    B[THR_POSG_TASK_DOP] = B[THR_POSG_TASK_RMS] = nt * 8;
    B[THR_POSG_TASK_STATUS] = B[THR_POSG_TASK_ITERS] = nt * 4;
    B[THR_POSG_MAP] = n_map * 8;
    B[THR_POSG_MAP_MIN] = n_map;
    counts_out->groups = n_groups;
    counts_out->rows = n_rows;
    counts_out->tasks = size_t(T);
    counts_out->starts = size_t(K);
    counts_out->grid = size_t(G);
    counts_out->map_groups = size_t(opts->map_count);
    *result_out = R;
    guard.r = nullptr;
    return THR_OK;
} catch (const std::bad_alloc&) {
    return thr::fail_msg(THR_ERR_DEVICE, "thr_posg: out of host memory");
} catch (...) {
    return thr::on_exception("thr_posg");
}

extern "C" int thr_posg_fetch(thr_posg_result* R, int which, void* dst, size_t dst_bytes) try {
    return thr::seg::fetch("thr_posg_fetch", R, which, dst, dst_bytes, &g_posg_ms[5]);
} catch (...) {
    return thr::on_exception("thr_posg_fetch");
}

extern "C" void thr_posg_free(thr_posg_result* R) { thr::seg::free_result(R); }

extern "C" int thr_debug_posg_times(double* ms_out) try {
    if (!ms_out) return thr::fail_msg(THR_ERR_ARG, "thr_debug_posg_times: null argument");
    for (int k = 0; k < 6; ++k) ms_out[k] = g_posg_ms[k];
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_posg_times");
}
