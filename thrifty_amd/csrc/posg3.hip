// Global solve for receivers with three coordinates (thr_posg3): thr_posg's idea for thr_pos3's two modes.  Every group's
// cost on a G x G x Gz volume over the receivers' surroundings (one plane at the group's height when that is known), the
// lowest local minima of it as further starts of thr_pos3's own iteration beside the fixed x0, the best minimum, the
// runner-up, and the flags -- among them MIRROR: the two differ in height only.  include/thrifty_hip.h states every rule.
//
// Four kernels:
//   A  k_tasks3 (task 0)   one 8-lane team per group: thr_pos3's own solve from x0 (csrc/pos3_lm.hpp, unchanged);
//   B  k_volume<G>         one wave per group, one wave per workgroup.  The volume never exists whole: a rolling window
//                          of three z-planes (3 G^2 doubles) lives in LDS.  Plane k + 1 is computed, then plane k is
//                          tested against the planes k - 1, k and k + 1 (outside planes count as +inf), its map plane is
//                          written, and its local minima are merged into a running list of the K lowest (F, c) that is
//                          identical in all lanes (wave-wide minimum rounds, per plane; a plane whose lowest minimum
//                          does not beat the list's worst costs one round).  The rows are staged in LDS kRowChunk at a
//                          time and read as broadcasts; a group of more rows stages its chunks again for every plane,
//                          a single-chunk group once.  Lane l owns the cells l, l + 64, ... of every plane and walks
//                          them two at a time (two independent chains: one wave per SIMD has nothing else to hide a
//                          square root behind); each cell's sum is one accumulator over the rows in order.  With up to
//                          kDistRx receivers a cell's distances are taken once per receiver, not twice per row.  With the
//                          height known the window is the one plane, and the kernel is posg.hip's k_grid;
//   C  k_tasks3 (1 .. K)   one team per (group, start): the same solve from the start cell's centre;
//   D  k_pick3             one lane per group: at most 9 tasks, compared pairwise in registers.
// Nothing is accumulated across lanes or teams, no read-modify-write on memory: a repeated call returns the same bits.
// All launches go to the null stream; temporaries are freed by hipFree, which waits for it.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>

#include "../../include/thrifty_hip.h"
#include "lmdif8.hpp"
#include "pos3_lm.hpp"
#include "post_stages.hpp"
#include "seg_reduce.hpp"

// a task must return thr_pos3's bits, and a cell's sum the statement's (and thr_posg's on a flat table): no a * b + c
// may become an fma in this file (the build also passes -ffp-contract=off for it, thrifty_amd/build.py)
#pragma clang fp contract(off)

namespace {

using thr::DevBuf;
using thr::Event;
using namespace thr::pos3lm;
using thr::seg::launch;
using thr::seg::launch_grid;

constexpr int kBlock = thr::seg::kBlock;  // workgroup size of k_tasks3 and k_pick3 (launch() assumes it)
constexpr int kTeams = kBlock / kTeam;     // tasks per workgroup of k_tasks3
constexpr int kRegRows = 4;                // rows per lane kept in registers, as pos3.hip
constexpr int kMaxReceivers = 64;
constexpr int kWave = 64;                  // k_volume: one wave per group and per workgroup
constexpr int kRowChunk = 32;              // rows staged in LDS at a time (THR_POSG_ROW_CHUNK's value)
constexpr int kMaxStarts = 8;
constexpr int kMaxTasks = kMaxStarts + 1;
constexpr int kMaxMap = 256;
constexpr int kMaxGridZ = 32;
constexpr int kDistRx = 32;                // up to this many receivers, a cell's distances are taken once per receiver
constexpr double kMaxMargin = 10e3;        // thr_pos3's box reaches this far beyond the receivers
static_assert(THR_POSG3_N_OUTPUTS <= thr::seg::kMaxOutputs, "the result handle holds every output");
static_assert(kRowChunk <= kWave, "one lane stages one row");

struct Cols {  // the input columns on the device
    const long long* ptr;
    const int *rx0, *rx1;
    const double *tdoa, *snr, *xyz, *group_h;  // group_h: null with z free
};
struct Area {  // the search volume: the first cell's corner and the cells' size (z: with z free only)
    double lo0, lo1, lo2, step0, step1, step2;
};
struct TaskOut {  // [groups][K + 1]
    double *pos, *dop, *hdop, *vdop, *rms;
    int *status, *iters;
};

// the centre of column / row / plane i: lo + (i + 0.5) * step, the form include/thrifty_hip.h gives
__device__ __forceinline__ double centre(double lo, double step, int i) { return lo + (double(i) + 0.5) * step; }

// A, C: team = (group, task task_lo + team % task_n).  Task 0 starts from (x0, y0, z0), task k from start cell k - 1;
// a task without a start cell (-1) does not exist: its team runs along with m == 0.
template <bool FREE_Z>
__global__ __launch_bounds__(kBlock) void k_tasks3(Cols c, int n_groups, int K, int G, int task_lo, int task_n,
                                                   const int* __restrict__ start_cell, Area area, double x0, double y0, double z0,
                                                   Box box, int max_iter, TaskOut o, double* __restrict__ snr_out) {
    const long long team = ((long long)blockIdx.x * kBlock + threadIdx.x) / kTeam;
    const int j = threadIdx.x & (kTeam - 1);
    const long long gl = team / task_n;
    const bool in_range = gl < n_groups;
    const int g = in_range ? int(gl) : 0, k = task_lo + int(team % task_n);
    bool live = in_range;
    double sx = x0, sy = y0, sz = z0;
    if (in_range && k > 0) {
        const int cell = start_cell[size_t(g) * K + (k - 1)];
        live = cell >= 0;
        if (live) {
            sx = centre(area.lo0, area.step0, cell % G);
            sy = centre(area.lo1, area.step1, (cell / G) % G);
            if (FREE_Z) sz = centre(area.lo2, area.step2, cell / (G * G));
        }
    }
    const long long beg = live ? c.ptr[g] : 0;
    const int m = live ? int(c.ptr[g + 1] - beg) : 0;
    const double h = (!FREE_Z && live) ? c.group_h[g] : 0.0;
    const Fit fit = solve_team<FREE_Z, kRegRows>(live, beg, m, j, c.rx0, c.rx1, c.tdoa, c.snr, c.xyz, h, sx, sy, sz, box, max_iter);
    if (in_range && j == 0) {
        const size_t t = size_t(g) * size_t(K + 1) + size_t(k);
        double dop, hdop, vdop;  // as k_pos_h / k_pos_z (pos3.hip) write them
        if (FREE_Z) {
            dop3_of(fit.cur, dop, hdop, vdop);
        } else {
            dop = hdop = dop2_of(fit.cur);
            vdop = 0.0;
        }
        o.pos[3 * t] = live ? fit.p0 : NAN;
        o.pos[3 * t + 1] = live ? fit.p1 : NAN;
        o.pos[3 * t + 2] = live ? (FREE_Z ? fit.p2 : h) : NAN;
        o.dop[t] = live ? dop : NAN;
        o.hdop[t] = live ? hdop : NAN;
        o.vdop[t] = live ? vdop : NAN;
        o.rms[t] = live ? sqrt(fit.cur.F / double(m)) : NAN;
        o.status[t] = live ? fit.status : THR_POSG3_NO_TASK;
        o.iters[t] = live ? fit.iters : 0;
        if (k == 0) snr_out[g] = fit.snr_mean;
    }
}

// (fa, ca) < (fb, cb); false when a NaN is compared
__device__ __forceinline__ bool key_less(double fa, int ca, double fb, int cb) { return fa < fb || (fa == fb && ca < cb); }

// B: workgroup = wave = group.  status0: task 0's status of every group.  n_dist receivers (0: none) have their
// distances from a cell taken once, in dynamic LDS [2][n_dist][64] (a lane walks its cells two at a time), and the rows
// read them: |rx - p| is the same expression whichever row names rx, so F keeps its bits and a cell costs n_rx square
// roots, not two per row.  gz planes (1 with the height known: the plane lies at group_h[g], and the window is that
// plane alone).
template <int G>
__global__ __launch_bounds__(kWave) void k_volume(Cols c, const int* __restrict__ status0, int task_stride, int n_dist, Area area, int gz,
                                                  int K, long long map_first, int map_count, int* __restrict__ start_cell,
                                                  double* __restrict__ start_f, int* __restrict__ n_local,
                                                  double* __restrict__ map, unsigned char* __restrict__ map_min) {
    constexpr int kCells = G * G, kOwn = kCells / kWave;
    static_assert(kOwn >= 2 && kOwn <= 32 && kOwn % 2 == 0, "a lane's local minima of a plane are a 32-bit mask; two cells per trip");
    __shared__ double rows[kRowChunk * 7];
    __shared__ double rx_xyz[kDistRx * 3];
    __shared__ int row_rx[kRowChunk * 2];
    extern __shared__ double window[];  // min(gz, 3) planes: plane p lives in slot p % 3; then dist[2][n_dist][64]
    double* const F = window;
    double* const dist = window + (gz < 3 ? gz : 3) * kCells;
    const int g = blockIdx.x, lane = threadIdx.x;
    const bool mapped = g >= map_first && g - map_first < map_count;
    const size_t map_at = mapped ? size_t(g - map_first) * size_t(gz) * kCells : 0;
    const int st = status0[size_t(g) * task_stride];
    if (st == kUnderdetermined || st == kNonfinite) {  // the whole wave alike: no grid
        if (lane < K) {
            start_cell[size_t(g) * K + lane] = -1;
            start_f[size_t(g) * K + lane] = NAN;
        }
        if (lane == 0) n_local[g] = 0;
        if (mapped)
            for (int k = 0; k < kOwn * gz; ++k) {
                map[map_at + lane + kWave * k] = NAN;
                map_min[map_at + lane + kWave * k] = 0;
            }
        return;
    }
    const long long beg = c.ptr[g];
    const int m = int(c.ptr[g + 1] - beg);
    const bool free_z = c.group_h == nullptr;
    const bool one_chunk = m <= kRowChunk;
    if (lane < 3 * n_dist) rx_xyz[lane] = c.xyz[lane];
    if (lane + kWave < 3 * n_dist) rx_xyz[lane + kWave] = c.xyz[lane + kWave];

    // the rows r0 .. r0 + n of the group, one per lane: the receivers' coordinates as they are and tdoa * c
    auto stage = [&](int r0, int n) {
        if (lane < n) {
            const long long i = beg + r0 + lane;
            const int a = c.rx0[i], b = c.rx1[i];
            double* r = rows + 7 * lane;
            r[0] = c.xyz[3 * a], r[1] = c.xyz[3 * a + 1], r[2] = c.xyz[3 * a + 2];
            r[3] = c.xyz[3 * b], r[4] = c.xyz[3 * b + 1], r[5] = c.xyz[3 * b + 2];
            r[6] = c.tdoa[i] * kSpeedOfLight;
            row_rx[2 * lane] = a, row_rx[2 * lane + 1] = b;
        }
    };
    if (one_chunk) stage(0, m);
    __syncthreads();

    double lf[kMaxStarts];  // the K lowest local minima so far by (F, c), identical in all lanes; constant indices only
    int lc[kMaxStarts];
#pragma unroll
    for (int s = 0; s < kMaxStarts; ++s) lf[s] = INFINITY, lc[s] = INT_MAX;
    int count = 0;  // this lane's local minima

#pragma unroll 1
    for (int kp = 0; kp <= gz; ++kp) {
        // ---- plane kp into its slot: chunk by chunk, every cell walks the chunk's rows in order
        if (kp < gz) {
            double* Fp = F + (kp % 3) * kCells;
            const double pz = free_z ? centre(area.lo2, area.step2, kp) : c.group_h[g];
            for (int k = 0; k < kOwn; ++k) Fp[lane + kWave * k] = 0.0;
#pragma unroll 1
            for (int r0 = 0; r0 < m; r0 += kRowChunk) {
                const int n = m - r0 < kRowChunk ? m - r0 : kRowChunk;
                if (!one_chunk) {
                    __syncthreads();  // the chunk before has been read
                    stage(r0, n);
                    __syncthreads();
                }
#pragma unroll 1
                for (int k = 0; k < kOwn; k += 2) {  // two cells per trip: two independent chains of square roots and sums
                    const int c0 = lane + kWave * k, c1 = c0 + kWave;
                    const double px0 = centre(area.lo0, area.step0, c0 % G), py0 = centre(area.lo1, area.step1, c0 / G);
                    const double px1 = centre(area.lo0, area.step0, c1 % G), py1 = centre(area.lo1, area.step1, c1 / G);
                    double acc0 = Fp[c0], acc1 = Fp[c1];
                    if (n_dist) {
                        double* const d0 = dist + lane;  // the lane reads only its own
                        double* const d1 = d0 + n_dist * kWave;
                        for (int r = 0; r < n_dist; ++r) {  // once per receiver
                            const double rx = rx_xyz[3 * r], ry = rx_xyz[3 * r + 1], vz = rx_xyz[3 * r + 2] - pz;
                            const double vx0 = rx - px0, vy0 = ry - py0, vx1 = rx - px1, vy1 = ry - py1;
                            d0[r * kWave] = sqrt((vx0 * vx0 + vy0 * vy0) + vz * vz);
                            d1[r * kWave] = sqrt((vx1 * vx1 + vy1 * vy1) + vz * vz);
                        }
                        for (int r = 0; r < n; ++r) {
                            const int ia = row_rx[2 * r] * kWave, ib = row_rx[2 * r + 1] * kWave;
                            const double tc = rows[7 * r + 6];
                            const double res0 = tc - (d0[ia] - d0[ib]), res1 = tc - (d1[ia] - d1[ib]);
                            acc0 += res0 * res0;
                            acc1 += res1 * res1;
                        }
                    } else {
                        for (int r = 0; r < n; ++r) {  // every lane reads the same row: LDS broadcasts
                            const double* w = rows + 7 * r;
                            const double az = w[2] - pz, bz = w[5] - pz;
                            const double ax0 = w[0] - px0, ay0 = w[1] - py0, bx0 = w[3] - px0, by0 = w[4] - py0;
                            const double ax1 = w[0] - px1, ay1 = w[1] - py1, bx1 = w[3] - px1, by1 = w[4] - py1;
                            const double res0 = w[6] - (sqrt((ax0 * ax0 + ay0 * ay0) + az * az) - sqrt((bx0 * bx0 + by0 * by0) + bz * bz));
                            const double res1 = w[6] - (sqrt((ax1 * ax1 + ay1 * ay1) + az * az) - sqrt((bx1 * bx1 + by1 * by1) + bz * bz));
                            acc0 += res0 * res0;
                            acc1 += res1 * res1;
                        }
                    }
                    Fp[c0] = acc0;
                    Fp[c1] = acc1;
                }
            }
        }
        __syncthreads();  // plane kp is whole
        if (kp == 0) continue;

        // ---- plane t = kp - 1 against the planes t - 1, t, t + 1: local minima, from LDS
        const int t = kp - 1;
        const double* Ft = F + (t % 3) * kCells;
        unsigned mine = 0;  // bit k: this lane's cell k of plane t is a local minimum
#pragma unroll 1
        for (int k = 0; k < kOwn; ++k) {
            const int col = lane + kWave * k, i = col % G, jr = col / G, cell = t * kCells + col;
            const double f = Ft[col];
            // every neighbour is read, whatever the earlier ones said (a neighbour outside the plane reads the cell
            // itself and is not looked at): the up to 26 reads are independent and none waits for a comparison
            const bool finite = f < INFINITY;
            bool ok = true;
#pragma unroll
            for (int dk = -1; dk <= 1; ++dk) {
                const int kk = t + dk;
                if (kk < 0 || kk >= gz) {  // nine neighbours outside; the whole wave alike
                    ok &= finite;
                    continue;
                }
                const double* Fn = F + (kk % 3) * kCells;
#pragma unroll
                for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
                    for (int di = -1; di <= 1; ++di) {
                        if (di == 0 && dj == 0 && dk == 0) continue;
                        const int ii = i + di, jj = jr + dj;
                        const bool inside = ii >= 0 && ii < G && jj >= 0 && jj < G;
                        const int at = inside ? jj * G + ii : col, nb = kk * kCells + at;
                        const double fn = Fn[at];
                        const bool below = (f < fn) | ((f == fn) & (nb > cell));
                        ok &= inside ? below : finite;
                    }
            }
            if (ok) mine |= 1u << k;
            if (mapped) {
                map[map_at + cell] = f;
                map_min[map_at + cell] = ok ? 1 : 0;
            }
        }
        count += __popc(mine);

        // ---- merge them into the list: every round a wave-wide minimum over the plane's keys after the last pick
        if (__any(mine != 0)) {
            double last_f = -INFINITY;
            int last_c = -1;
            for (int s = 0; s < K; ++s) {
                double bf = INFINITY;
                int bc = INT_MAX;
#pragma unroll 1
                for (int k = 0; k < kOwn; ++k) {
                    if (!((mine >> k) & 1u)) continue;
                    const int col = lane + kWave * k, cell = t * kCells + col;
                    const double f = Ft[col];
                    if (key_less(last_f, last_c, f, cell) && key_less(f, cell, bf, bc)) bf = f, bc = cell;
                }
                for (int d = 1; d < kWave; d <<= 1) {  // identical in all lanes afterwards: the keys are distinct
                    const double of = __shfl_xor(bf, d, kWave);
                    const int oc = __shfl_xor(bc, d, kWave);
                    if (key_less(of, oc, bf, bc)) bf = of, bc = oc;
                }
                double wf = lf[0];  // the list's worst: entry K - 1 (the sentinel while the list is short)
                int wc = lc[0];
#pragma unroll
                for (int a = 1; a < kMaxStarts; ++a)
                    if (a == K - 1) wf = lf[a], wc = lc[a];
                if (bc == INT_MAX || !key_less(bf, bc, wf, wc)) break;  // the plane's later minima are higher still
#pragma unroll
                for (int a = kMaxStarts - 1; a >= 1; --a) {  // insertion: the entries above the new key move down
                    const bool above = key_less(bf, bc, lf[a - 1], lc[a - 1]), here = key_less(bf, bc, lf[a], lc[a]);
                    lf[a] = above ? lf[a - 1] : (here ? bf : lf[a]);
                    lc[a] = above ? lc[a - 1] : (here ? bc : lc[a]);
                }
                if (key_less(bf, bc, lf[0], lc[0])) lf[0] = bf, lc[0] = bc;
                last_f = bf, last_c = bc;
            }
        }
        __syncthreads();  // plane t - 1's slot is plane kp + 1's
    }
    for (int d = 1; d < kWave; d <<= 1) count += __shfl_xor(count, d, kWave);
    if (lane == 0) n_local[g] = count;
#pragma unroll
    for (int s = 0; s < kMaxStarts; ++s)
        if (lane == s && s < K) {
            start_cell[size_t(g) * K + s] = lc[s] == INT_MAX ? -1 : lc[s];
            start_f[size_t(g) * K + s] = lc[s] == INT_MAX ? NAN : lf[s];
        }
}

struct Picked {  // the per-group outputs
    double *pos, *dop, *hdop, *vdop, *rms, *pos2, *rms2;
    int *status, *task, *n_minima, *flags;
};

// D: one lane per group.  Every loop runs to kMaxTasks with constant indices: the tasks stay in registers.  The rule is
// posg.hip's k_pick with the distance of the mode and the MIRROR flag.
template <bool FREE_Z>
__global__ __launch_bounds__(kBlock) void k_pick3(int n_groups, int K, TaskOut t, double merge_m, double ratio, double floor_m,
                                                  Picked o) {
    const int g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= n_groups) return;
    const size_t base = size_t(g) * size_t(K + 1);
    double x[kMaxTasks], y[kMaxTasks], z[kMaxTasks], rms[kMaxTasks];
    bool elig[kMaxTasks], dup[kMaxTasks], first[kMaxTasks];
#pragma unroll
    for (int a = 0; a < kMaxTasks; ++a) {
        const bool there = a <= K;
        x[a] = there ? t.pos[3 * (base + a)] : NAN;
        y[a] = there ? t.pos[3 * (base + a) + 1] : NAN;
        z[a] = there ? t.pos[3 * (base + a) + 2] : NAN;
        rms[a] = there ? t.rms[base + a] : NAN;
        elig[a] = there && t.status[base + a] == kOk;
    }
    auto apart = [](double dx, double dy, double dz) { return FREE_Z ? sqrt((dx * dx + dy * dy) + dz * dz) : sqrt(dx * dx + dy * dy); };
    int best = -1, n_minima = 0;
#pragma unroll
    for (int a = 0; a < kMaxTasks; ++a) {
        bool any_before = false, duplicate = false;
#pragma unroll
        for (int b = 0; b < kMaxTasks; ++b) {
            if (b == a) continue;
            const bool before = elig[b] && (rms[b] < rms[a] || (rms[b] == rms[a] && b < a));
            any_before = any_before || before;
            duplicate = duplicate || (before && apart(x[a] - x[b], y[a] - y[b], z[a] - z[b]) <= merge_m);
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
    double bx = x[0], by = y[0], bz = z[0], brms = rms[0], sx = NAN, sy = NAN, sz = NAN;
#pragma unroll
    for (int a = 0; a < kMaxTasks; ++a) {
        if (a == best) bx = x[a], by = y[a], bz = z[a], brms = rms[a];
        if (a == second) sx = x[a], sy = y[a], sz = z[a];
    }
    int flags = 0;
    if (best < 0) flags |= THR_POSG3_NO_MINIMUM;
    if (!elig[0] || !(apart(bx - x[0], by - y[0], bz - z[0]) <= merge_m)) flags |= THR_POSG3_MOVED;
    if (second >= 0 && second_rms <= fmax(ratio * brms, floor_m)) {
        flags |= THR_POSG3_AMBIGUOUS;
        const double dx = sx - bx, dy = sy - by;
        if (FREE_Z && sqrt(dx * dx + dy * dy) <= merge_m) flags |= THR_POSG3_MIRROR;
    }
    const int chosen = best < 0 ? 0 : best;
    o.pos[3 * size_t(g)] = bx;
    o.pos[3 * size_t(g) + 1] = by;
    o.pos[3 * size_t(g) + 2] = bz;
    o.dop[g] = t.dop[base + chosen];
    o.hdop[g] = t.hdop[base + chosen];
    o.vdop[g] = t.vdop[base + chosen];
    o.status[g] = t.status[base + chosen];
    o.rms[g] = brms;
    o.task[g] = chosen;
    o.pos2[3 * size_t(g)] = sx;
    o.pos2[3 * size_t(g) + 1] = sy;
    o.pos2[3 * size_t(g) + 2] = sz;
    o.rms2[g] = second >= 0 ? second_rms : NAN;
    o.n_minima[g] = n_minima;
    o.flags[g] = flags;
}

template <int G>
int launch_k_volume(int ng, hipStream_t s, Cols C, const int* status0, int task_stride, int n_dist, Area area, int gz, int K,
                    long long map_first, int map_count, int* start_cell, double* start_f, int* n_local, double* map,
                    unsigned char* map_min) {
    const size_t lds = (size_t(gz < 3 ? gz : 3) * G * G + size_t(2) * n_dist * kWave) * sizeof(double);  // the window, then dist
    hipLaunchKernelGGL(k_volume<G>, dim3(unsigned(ng)), dim3(kWave), lds, s, C, status0, task_stride,
                       n_dist, area, gz, K, map_first, map_count, start_cell, start_f, n_local, map, map_min);
    THR_HIP_TRY(hipGetLastError());
    return THR_OK;
}

thread_local double g_posg3_ms[6] = {0, 0, 0, 0, 0, 0};

}  // namespace

struct thr_posg3_result : thr::seg::Result {};

extern "C" int thr_posg3(int device_id, size_t n_groups, const int64_t* group_ptr, const int32_t* row_rx0,
                         const int32_t* row_rx1, const double* row_tdoa, const double* row_snr, int n_rx,
                         const double* rx_xyz, int mode, const double* group_h, const double* z_range, const double* z_grid,
                         const thr_posg3_opts* opts, thr_posg3_result** result_out, thr_posg3_counts* counts_out) try {
    if (result_out) *result_out = nullptr;
    if (counts_out) std::memset(counts_out, 0, sizeof(*counts_out));
    for (double& t : g_posg3_ms) t = 0;
    if (!result_out || !counts_out || !opts || !group_ptr || !rx_xyz) return thr::fail_msg(THR_ERR_ARG, "thr_posg3: null argument");
    if (mode != THR_POS3_KNOWN_HEIGHT && mode != THR_POS3_FREE_Z)
        return thr::fail_msg(THR_ERR_ARG, "thr_posg3: mode must be THR_POS3_KNOWN_HEIGHT or THR_POS3_FREE_Z, not %d", mode);
    const bool free_z = mode == THR_POS3_FREE_Z;
    if (n_rx < 1 || n_rx > kMaxReceivers) return thr::fail_msg(THR_ERR_ARG, "thr_posg3: 1 to %d receivers, not %d", kMaxReceivers, n_rx);
    if (opts->max_iter < 0) return thr::fail_msg(THR_ERR_ARG, "thr_posg3: max_iter must not be negative");
    if (opts->grid != 16 && opts->grid != 32) return thr::fail_msg(THR_ERR_ARG, "thr_posg3: grid must be 16 or 32, not %d", opts->grid);
    if (free_z ? (opts->grid_z < 2 || opts->grid_z > kMaxGridZ) : opts->grid_z != 1)
        return thr::fail_msg(THR_ERR_ARG, "thr_posg3: grid_z must be 1 with the height known and lie in 2 .. %d with z free, not %d",
                             kMaxGridZ, opts->grid_z);
    if (opts->starts < 1 || opts->starts > kMaxStarts)
        return thr::fail_msg(THR_ERR_ARG, "thr_posg3: starts must lie in 1 .. %d, not %d", kMaxStarts, opts->starts);
    if (!(opts->margin_m > 0.0 && opts->margin_m <= kMaxMargin))
        return thr::fail_msg(THR_ERR_ARG, "thr_posg3: margin_m must lie in (0, %g] metres", kMaxMargin);
    if (!(opts->merge_m > 0.0) || !std::isfinite(opts->merge_m)) return thr::fail_msg(THR_ERR_ARG, "thr_posg3: merge_m must be positive and finite");
    if (!(opts->ratio >= 1.0) || !std::isfinite(opts->ratio)) return thr::fail_msg(THR_ERR_ARG, "thr_posg3: ratio must be at least 1 and finite");
    if (!(opts->floor_m >= 0.0) || !std::isfinite(opts->floor_m))
        return thr::fail_msg(THR_ERR_ARG, "thr_posg3: floor_m must be finite and not negative (0: the ratio alone)");
    if (n_groups > size_t(1) << 28 || n_groups * size_t(opts->starts + 1) > size_t(1) << 28)
        return thr::fail_msg(THR_ERR_ARG, "thr_posg3: too many groups or tasks");
    if (opts->map_count < 0 || opts->map_count > kMaxMap)
        return thr::fail_msg(THR_ERR_ARG, "thr_posg3: map_count must lie in 0 .. %d, not %d", kMaxMap, opts->map_count);
    if (opts->map_first < 0 || uint64_t(opts->map_first) + uint64_t(opts->map_count) > uint64_t(n_groups))
        return thr::fail_msg(THR_ERR_ARG, "thr_posg3: the map range %lld + %d passes the %zu groups", (long long)opts->map_first,
                             opts->map_count, n_groups);
    if (!free_z && n_groups && !group_h) return thr::fail_msg(THR_ERR_ARG, "thr_posg3: the known-height mode needs group_h");

    // ---- everything a kernel will index with is checked here, before anything is launched (thr_pos3's checks)
    if (group_ptr[0] != 0) return thr::fail_msg(THR_ERR_ARG, "thr_posg3: group_ptr[0] must be 0");
    for (size_t g = 0; g < n_groups; ++g) {
        const int64_t len = group_ptr[g + 1] - group_ptr[g];
        if (len < 0) return thr::fail_msg(THR_ERR_ARG, "thr_posg3: group_ptr decreases at group %zu", g);
        if (len > (int64_t(1) << 24)) return thr::fail_msg(THR_ERR_ARG, "thr_posg3: group %zu is too long", g);
        if (!free_z && !std::isfinite(group_h[g])) return thr::fail_msg(THR_ERR_ARG, "thr_posg3: the height of group %zu is not finite", g);
    }
    const size_t n_rows = size_t(group_ptr[n_groups]);
    if (n_rows > size_t(1) << 30) return thr::fail_msg(THR_ERR_ARG, "thr_posg3: too many rows");
    if (n_rows && (!row_rx0 || !row_rx1 || !row_tdoa || !row_snr)) return thr::fail_msg(THR_ERR_ARG, "thr_posg3: null argument");
    for (size_t i = 0; i < n_rows; ++i)
        if (row_rx0[i] < 0 || row_rx0[i] >= n_rx || row_rx1[i] < 0 || row_rx1[i] >= n_rx)
            return thr::fail_msg(THR_ERR_ARG, "thr_posg3: row %zu names receivers %d and %d of %d", i, row_rx0[i], row_rx1[i], n_rx);
    for (size_t i = 0; i < size_t(n_rx) * 3; ++i)
        if (!std::isfinite(rx_xyz[i])) return thr::fail_msg(THR_ERR_ARG, "thr_posg3: receiver coordinate %zu is not finite", i);
    for (int k = 0; k < (free_z ? 3 : 2); ++k)
        if (!std::isfinite(opts->x0[k])) return thr::fail_msg(THR_ERR_ARG, "thr_posg3: x0 must be finite");
    double rlo[3], rhi[3], lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {  // the receivers' extent, and thr_pos3's box around it
        rlo[k] = rhi[k] = rx_xyz[k];
        for (int r = 1; r < n_rx; ++r) {
            rlo[k] = std::fmin(rlo[k], rx_xyz[3 * r + k]);
            rhi[k] = std::fmax(rhi[k], rx_xyz[3 * r + k]);
        }
        lo[k] = rlo[k], hi[k] = rhi[k];
        lo[k] -= kMaxMargin;
        hi[k] += kMaxMargin;
    }
    if (free_z && z_range) {
        if (!std::isfinite(z_range[0]) || !std::isfinite(z_range[1]) || !(z_range[0] < z_range[1]))
            return thr::fail_msg(THR_ERR_ARG, "thr_posg3: z_range must be finite with z_lo < z_hi");
        lo[2] = z_range[0], hi[2] = z_range[1];
    }
    if (free_z && !(opts->x0[2] >= lo[2] && opts->x0[2] <= hi[2]))
        return thr::fail_msg(THR_ERR_ARG, "thr_posg3: x0[2] = %g lies outside the z range %g .. %g", opts->x0[2], lo[2], hi[2]);
    if (free_z) {
        if (!z_grid) return thr::fail_msg(THR_ERR_ARG, "thr_posg3: the free-z mode needs z_grid");
        if (!std::isfinite(z_grid[0]) || !std::isfinite(z_grid[1]) || !(z_grid[0] < z_grid[1]))
            return thr::fail_msg(THR_ERR_ARG, "thr_posg3: z_grid must be finite with zg_lo < zg_hi");
        if (!(z_grid[0] >= lo[2] && z_grid[1] <= hi[2]))
            return thr::fail_msg(THR_ERR_ARG, "thr_posg3: z_grid %g .. %g leaves the z box %g .. %g", z_grid[0], z_grid[1], lo[2], hi[2]);
    }
    const Box box{lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]};
    const int G = opts->grid, GZ = opts->grid_z, K = opts->starts, T = K + 1;
    double alo[2], ahi[2];
    for (int k = 0; k < 2; ++k) {  // thr_posg's area
        alo[k] = rlo[k] - opts->margin_m;
        ahi[k] = rhi[k] + opts->margin_m;
    }
    const Area area{alo[0], alo[1], free_z ? z_grid[0] : 0.0, (ahi[0] - alo[0]) / double(G), (ahi[1] - alo[1]) / double(G),
                    free_z ? (z_grid[1] - z_grid[0]) / double(GZ) : 0.0};

    THR_TRY(thr::seg::pick_device(device_id));
    thr_posg3_result* R = new thr_posg3_result;
    thr::seg::ResultGuard guard{R};
    R->device = device_id;
    R->n_out = THR_POSG3_N_OUTPUTS;
    hipStream_t s = nullptr;
    Event ev[6];
    for (Event& e : ev) THR_HIP_TRY(e.create());
    for (Event& e : R->ev) THR_HIP_TRY(e.create());
    const int ng = int(n_groups);
    const size_t nt = n_groups * size_t(T), ns = n_groups * size_t(K);
    const size_t n_map = size_t(opts->map_count) * size_t(GZ) * size_t(G) * size_t(G);

    // ---- copies in
    DevBuf d_ptr, d_rx0, d_rx1, d_tdoa, d_snr, d_xyz, d_h;
    THR_HIP_TRY(d_ptr.alloc((n_groups + 1) * 8));
    THR_HIP_TRY(d_rx0.alloc(n_rows * 4));
    THR_HIP_TRY(d_rx1.alloc(n_rows * 4));
    THR_HIP_TRY(d_tdoa.alloc(n_rows * 8));
    THR_HIP_TRY(d_snr.alloc(n_rows * 8));
    THR_HIP_TRY(d_xyz.alloc(size_t(n_rx) * 24));
    if (!free_z) THR_HIP_TRY(d_h.alloc(n_groups * 8));
    THR_HIP_TRY(hipEventRecord(ev[0].e, s));
    THR_HIP_TRY(hipMemcpy(d_ptr.p, group_ptr, (n_groups + 1) * 8, hipMemcpyHostToDevice));
    if (n_rows) {
        THR_HIP_TRY(hipMemcpy(d_rx0.p, row_rx0, n_rows * 4, hipMemcpyHostToDevice));
        THR_HIP_TRY(hipMemcpy(d_rx1.p, row_rx1, n_rows * 4, hipMemcpyHostToDevice));
        THR_HIP_TRY(hipMemcpy(d_tdoa.p, row_tdoa, n_rows * 8, hipMemcpyHostToDevice));
        THR_HIP_TRY(hipMemcpy(d_snr.p, row_snr, n_rows * 8, hipMemcpyHostToDevice));
    }
    THR_HIP_TRY(hipMemcpy(d_xyz.p, rx_xyz, size_t(n_rx) * 24, hipMemcpyHostToDevice));
    if (!free_z && n_groups) THR_HIP_TRY(hipMemcpy(d_h.p, group_h, n_groups * 8, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipEventRecord(ev[1].e, s));
    const Cols C{d_ptr.as<long long>(), d_rx0.as<int>(), d_rx1.as<int>(), d_tdoa.as<double>(), d_snr.as<double>(), d_xyz.as<double>(),
                 free_z || !n_groups ? nullptr : d_h.as<double>()};
    DevBuf* O = R->out;

    // ---- A: task 0, thr_pos3's own solve
    THR_HIP_TRY(O[THR_POSG3_TASK_POS].alloc(nt * 24));
    for (int w : {THR_POSG3_TASK_DOP, THR_POSG3_TASK_HDOP, THR_POSG3_TASK_VDOP, THR_POSG3_TASK_RMS}) THR_HIP_TRY(O[w].alloc(nt * 8));
    for (int w : {THR_POSG3_TASK_STATUS, THR_POSG3_TASK_ITERS}) THR_HIP_TRY(O[w].alloc(nt * 4));
    THR_HIP_TRY(O[THR_POSG3_SNR].alloc(n_groups * 8));
    THR_HIP_TRY(O[THR_POSG3_START_CELL].alloc(ns * 4));
    THR_HIP_TRY(O[THR_POSG3_START_F].alloc(ns * 8));
    THR_HIP_TRY(O[THR_POSG3_N_LOCAL].alloc(n_groups * 4));
    THR_HIP_TRY(O[THR_POSG3_MAP].alloc(n_map * 8));
    THR_HIP_TRY(O[THR_POSG3_MAP_MIN].alloc(n_map));
    const TaskOut tasks{O[THR_POSG3_TASK_POS].as<double>(),  O[THR_POSG3_TASK_DOP].as<double>(), O[THR_POSG3_TASK_HDOP].as<double>(),
                        O[THR_POSG3_TASK_VDOP].as<double>(), O[THR_POSG3_TASK_RMS].as<double>(), O[THR_POSG3_TASK_STATUS].as<int>(),
                        O[THR_POSG3_TASK_ITERS].as<int>()};
    int* start_cell = O[THR_POSG3_START_CELL].as<int>();
    auto* tasks_fn = free_z ? k_tasks3<true> : k_tasks3<false>;
    if (ng)
        THR_TRY(launch_grid(tasks_fn, dim3(unsigned((n_groups + kTeams - 1) / kTeams)), s, C, ng, K, G, 0, 1, start_cell, area,
                            opts->x0[0], opts->x0[1], free_z ? opts->x0[2] : 0.0, box, int(opts->max_iter), tasks,
                            O[THR_POSG3_SNR].as<double>()));
    THR_HIP_TRY(hipEventRecord(ev[2].e, s));

    // ---- B: the volume plane by plane, its local minima, the starts
    if (ng) {
        auto* volume_fn = G == 16 ? launch_k_volume<16> : launch_k_volume<32>;
        THR_TRY(volume_fn(ng, s, C, tasks.status, T, n_rx <= kDistRx ? n_rx : 0, area, GZ, K, (long long)opts->map_first,
                          int(opts->map_count), start_cell, O[THR_POSG3_START_F].as<double>(), O[THR_POSG3_N_LOCAL].as<int>(),
                          O[THR_POSG3_MAP].as<double>(), O[THR_POSG3_MAP_MIN].as<unsigned char>()));
    }
    THR_HIP_TRY(hipEventRecord(ev[3].e, s));

    // ---- C: tasks 1 .. K
    if (ng)
        THR_TRY(launch_grid(tasks_fn, dim3(unsigned((ns + kTeams - 1) / kTeams)), s, C, ng, K, G, 1, K, start_cell, area, opts->x0[0],
                            opts->x0[1], free_z ? opts->x0[2] : 0.0, box, int(opts->max_iter), tasks, O[THR_POSG3_SNR].as<double>()));
    THR_HIP_TRY(hipEventRecord(ev[4].e, s));

    // ---- D: the choice
    for (int w : {THR_POSG3_POS, THR_POSG3_POS2}) THR_HIP_TRY(O[w].alloc(n_groups * 24));
    for (int w : {THR_POSG3_DOP, THR_POSG3_HDOP, THR_POSG3_VDOP, THR_POSG3_RMS, THR_POSG3_RMS2}) THR_HIP_TRY(O[w].alloc(n_groups * 8));
    for (int w : {THR_POSG3_STATUS, THR_POSG3_TASK, THR_POSG3_N_MINIMA, THR_POSG3_FLAGS}) THR_HIP_TRY(O[w].alloc(n_groups * 4));
    const Picked picked{O[THR_POSG3_POS].as<double>(),  O[THR_POSG3_DOP].as<double>(),  O[THR_POSG3_HDOP].as<double>(),
                        O[THR_POSG3_VDOP].as<double>(), O[THR_POSG3_RMS].as<double>(),  O[THR_POSG3_POS2].as<double>(),
                        O[THR_POSG3_RMS2].as<double>(), O[THR_POSG3_STATUS].as<int>(),  O[THR_POSG3_TASK].as<int>(),
                        O[THR_POSG3_N_MINIMA].as<int>(), O[THR_POSG3_FLAGS].as<int>()};
    auto* pick_fn = free_z ? k_pick3<true> : k_pick3<false>;
    THR_TRY(launch(pick_fn, n_groups, s, ng, K, tasks, opts->merge_m, opts->ratio, opts->floor_m, picked));
    THR_HIP_TRY(hipEventRecord(ev[5].e, s));
    THR_HIP_TRY(hipEventSynchronize(ev[5].e));  // the temporaries go out of scope
    for (int k = 0; k < 5; ++k) {
        float ms = 0;
        THR_HIP_TRY(hipEventElapsedTime(&ms, ev[k].e, ev[k + 1].e));
        g_posg3_ms[k] = ms;
    }

    size_t* B = R->bytes;
    B[THR_POSG3_POS] = B[THR_POSG3_POS2] = n_groups * 24;
    B[THR_POSG3_DOP] = B[THR_POSG3_HDOP] = B[THR_POSG3_VDOP] = B[THR_POSG3_RMS] = B[THR_POSG3_RMS2] = B[THR_POSG3_SNR] = n_groups * 8;
    B[THR_POSG3_STATUS] = B[THR_POSG3_TASK] = B[THR_POSG3_N_MINIMA] = B[THR_POSG3_FLAGS] = B[THR_POSG3_N_LOCAL] = n_groups * 4;
    B[THR_POSG3_START_CELL] = ns * 4;
    B[THR_POSG3_START_F] = ns * 8;
    B[THR_POSG3_TASK_POS] = nt * 24;
    B[THR_POSG3_TASK_DOP] = B[THR_POSG3_TASK_HDOP] = B[THR_POSG3_TASK_VDOP] = B[THR_POSG3_TASK_RMS] = nt * 8;
    B[THR_POSG3_TASK_STATUS] = B[THR_POSG3_TASK_ITERS] = nt * 4;
    B[THR_POSG3_MAP] = n_map * 8;
    B[THR_POSG3_MAP_MIN] = n_map;
    counts_out->groups = n_groups;
    counts_out->rows = n_rows;
    counts_out->tasks = size_t(T);
    counts_out->starts = size_t(K);
    counts_out->grid = size_t(G);
    counts_out->grid_z = size_t(GZ);
    counts_out->map_groups = size_t(opts->map_count);
    *result_out = R;
    guard.r = nullptr;
    return THR_OK;
} catch (const std::bad_alloc&) {
    return thr::fail_msg(THR_ERR_DEVICE, "thr_posg3: out of host memory");
} catch (...) {
    return thr::on_exception("thr_posg3");
}

extern "C" int thr_posg3_fetch(thr_posg3_result* R, int which, void* dst, size_t dst_bytes) try {
    return thr::seg::fetch("thr_posg3_fetch", R, which, dst, dst_bytes, &g_posg3_ms[5]);
} catch (...) {
    return thr::on_exception("thr_posg3_fetch");
}

extern "C" void thr_posg3_free(thr_posg3_result* R) { thr::seg::free_result(R); }

extern "C" int thr_debug_posg3_times(double* ms_out) try {
    if (!ms_out) return thr::fail_msg(THR_ERR_ARG, "thr_debug_posg3_times: null argument");
    for (int k = 0; k < 6; ++k) ms_out[k] = g_posg3_ms[k];
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_posg3_times");
}
