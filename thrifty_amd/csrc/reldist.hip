// Relative distance, speed and Doppler on the device: the numbers of the reference's scripts/reldist_nearest.py
// for EVERY (mobile, beacon, rx0 < rx1) cell of a deployment in one call (thr_reldist; the formulas are in
// include/thrifty_hip.h, operation for operation).
//
//   1. groups    seg_cells.hpp's front end (check_matches, pair_rows with this file's selector): one thread per
//                match counts and then emits the detection pairs it holds, two stable radix sorts leave them
//                grouped by (txid, rx0, rx1) in match order.  One reduction per
//                group counts the places where soa (and the timestamp) at rx0 decreases.  A GROUP is the row
//                list of one transmitter at one pair: a beacon's group serves every mobile of that pair.
//   2. cells     the group table is a few dozen entries: the host reads it, pairs every mobile group with every
//                beacon's group of the same receivers, orders the cells by (mobile, beacon, rx0, rx1), looks
//                the geometry up and sends the cell table back.  A cell's rows are its mobile group's.
//   3. rows      one thread per row: bisection in the beacon's soa at rx0 (numpy's order: a NaN is last), the
//                nearest row, raw by either method, x, the doppler.
//   4. masks     stat_tools.is_outlier per cell is seg_cells.hpp's outlier_mask, the one thr_tdoastats calls:
//                median and MAD from two sorts by (cell, value); statistics over the kept rows by tiled
//                segmented reductions (seg_reduce.hpp); the speeds are one scan (which kept row is whose
//                predecessor) and one thread per kept row; masks 2 and 3 the same way on speeds and dopplers.
//   5. smoother  the kept speeds and the kept dopplers as two point lists; k_smooth gives ONE WAVE to a point:
//                the window by bisection on the monotone predicate, h by a lane-strided maximum, then the five
//                sums (w, w D, w y, w D D, w D y) lane-strided over the window's k terms and combined by a
//                xor butterfly.  n x k weighted terms: the only compute-heavy part of the stage.  The abscissae
//                and values of neighbouring points' windows overlap almost entirely and are read through L2.
//                A point's value depends on its cell's points alone: not on the grid, not on the other cells.
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

// numpy's float64 operations one by one: no a * b + c may become an fma in this file (the build also passes
// -ffp-contract=off, thrifty_amd/build.py)
#pragma clang fp contract(off)

namespace {

using thr::DevBuf;
using thr::Event;
using namespace thr::seg;

constexpr double kLight = 2.997e8;
constexpr int kPointLanes = 64;       // one wave per smoothed point
constexpr int kMaxSmoothGrid = 8192;  // workgroups of k_smooth: each wave loops over its points
constexpr double kSingular = 1e-12;   // det <= kSingular * Sw * Swdd: the weighted mean instead of the line
static_assert(kBlock % kPointLanes == 0, "whole waves");

// ------------------------------------------------------------------ 1. groups
struct Dets {
    const int *rx, *tx;
    const double *soa, *ts, *cbin, *coff;
    const long long *mptr, *midx;
    const int *beacons, *mobiles, *receivers;
    int n_beacons, n_mobiles, n_receivers;  // -1: no list
};
struct TxPairs {  // k_pairs' selector: matches of the beacons and the mobiles, pairs of listed receivers
    Dets d;
    // without a list of mobiles every transmitter is a beacon or a mobile
    __device__ bool wanted(int tx) const {
        return d.n_mobiles < 0 || find_sorted(d.beacons, d.n_beacons, tx) >= 0 || find_sorted(d.mobiles, d.n_mobiles, tx) >= 0;
    }
    __device__ bool kept(long long da, long long db) const {
        return find_sorted(d.receivers, d.n_receivers, d.rx[da]) >= 0 && find_sorted(d.receivers, d.n_receivers, d.rx[db]) >= 0;
    }
};

struct Src {  // the rows of all groups, in group order
    long long *det, *match;
    double *s0, *s1, *f, *t0, *t1;  // soa at rx0 / rx1, carrier at rx0 minus at rx1, the two timestamps
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
    o.s0[p] = d.soa[d0];
    o.s1[p] = d.soa[d1];
    o.f[p] = (d.cbin[d0] + d.coff[d0]) - (d.cbin[d1] + d.coff[d1]);
    o.t0[p] = d.ts[d0];
    o.t1[p] = d.ts[d1];
}
struct LoadOrder {  // the places where a group's soa / timestamp at rx0 decreases
    const double *s0, *t0;
    const int* pos_grp;
    int n;
    __device__ void operator()(int p, double (&v)[2]) const {
        if (p + 1 >= n || pos_grp[p + 1] != pos_grp[p]) return;
        v[0] = s0[p + 1] < s0[p] ? 1.0 : 0.0;
        v[1] = t0[p + 1] < t0[p] ? 1.0 : 0.0;
    }
};

// ------------------------------------------------------------------ 2. cells (the table comes from the host)
struct Cell {
    int key[4];                  // mobile, beacon, rx0, rx1
    long long start, msrc, bsrc; // first row; first row of the mobile's and of the beacon's group
    int n, nb, flags, pad;       // rows, beacon rows
    double geo[3];               // d_beacon, dist_rx, dist_beacon
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

// ------------------------------------------------------------------ 3. rows
// numpy's order for searchsorted: a NaN is larger than every number
__device__ __forceinline__ bool np_less(double a, double b) { return a < b || (b != b && a == a); }
struct Consts {
    int method;
    double s2m, rate, hz_per_bin, carrier, thresh, frac;
};
struct Rows {
    long long *det, *match;
    int *nearest, *hi, *flags;
    double *raw, *x, *dop, *s1, *t0rel, *t1rel;
};
__global__ __launch_bounds__(kBlock) void k_rel(const Cell* __restrict__ cells, const int* __restrict__ pos_cell, Src g,
                                                Consts k, int m, Rows o) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= m) return;
    const Cell& c = cells[pos_cell[p]];
    const size_t sr = size_t(c.msrc + (p - c.start));
    o.det[2 * size_t(p)] = g.det[2 * sr];
    o.det[2 * size_t(p) + 1] = g.det[2 * sr + 1];
    o.match[p] = g.match[sr];
    const double t0 = g.s0[sr], t1 = g.s1[sr];
    o.s1[p] = t1;
    o.t0rel[p] = g.t0[sr] - g.t0[c.msrc];
    o.t1rel[p] = g.t1[sr] - g.t0[c.msrc];
    int hi = -1, n = -1, fl = 0;
    double raw = NAN, dop = NAN;
    if (c.flags == 0) {
        const double *b0 = g.s0 + c.bsrc, *b1 = g.s1 + c.bsrc, *bf = g.f + c.bsrc;
        const int nb = c.nb;
        int lo = 0;
        hi = nb;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (np_less(b0[mid], t0)) lo = mid + 1; else hi = mid;
        }
        n = (hi > 0 && (hi == nb || fabs(t0 - b0[hi - 1]) < fabs(t0 - b0[hi]))) ? hi - 1 : hi;
        if (k.method == THR_RELDIST_NEAREST) {
            raw = (t1 - b1[n]) - (t0 - b0[n]);
        } else if (hi == 0 || hi == nb) {
            raw = t1 - b1[hi == 0 ? 0 : nb - 1];
            fl = THR_RELDIST_ROW_HELD;
        } else {
            const double w = (t0 - b0[hi - 1]) / (b0[hi] - b0[hi - 1]);
            raw = t1 - (b1[hi - 1] * (1.0 - w) + b1[hi] * w);
        }
        const double dop_bin = (g.f[sr] - bf[n]) / 2.0;
        dop = dop_bin * k.hz_per_bin * 3e8 / k.carrier * 3.6;
    }
    o.hi[p] = hi;
    o.nearest[p] = n;
    o.flags[p] = fl;
    o.raw[p] = raw;
    o.x[p] = (raw + c.geo[0] + c.geo[1]) / 2.0 - c.geo[2];
    o.dop[p] = dop;
}

// ------------------------------------------------------------------ 4. masks, statistics, speeds
struct LoadMax {  // K = 1, no sum, no minimum: a cell's largest value, NaN when it holds one
    const double* v;
    __device__ void operator()(int p, double (&o)[1]) const { o[0] = v[p]; }
};
// med[c * 6], med[c * 6 + 1] = median, MAD of the cell's values; mask[p] = is_outlier.  The NaN probe is the cell's
// max, reduced here into probe[nc] through the stage's slab.
int masked(const double* vals, const Series& S, double thresh, Work& k, double* slab, double* probe, double* med,
           unsigned char* mask, hipStream_t s) {
    if (S.n) THR_TRY((reduce<1, 0, 0>(LoadMax{vals}, S.L, slab, probe, s)));
    return outlier_mask(vals, S, probe, 1, thresh, k, med, 6, mask, s);
}
// cv: LoadKept1<false>'s count, sum, min, max of the kept rows per cell; cv2: LoadKept2<false>'s
__global__ __launch_bounds__(kBlock) void k_mean_std(const double* __restrict__ cv, const double* __restrict__ cv2, int nc,
                                                     double* __restrict__ ms) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= nc) return;
    ms[2 * size_t(c)] = cv[4 * size_t(c) + 1] / cv[4 * size_t(c)];
    ms[2 * size_t(c) + 1] = sqrt(cv2[c] / cv[4 * size_t(c)]);
}
struct LoadSt3 {  // kept rows inside [mean - std, mean + std]
    const double *x, *ms;
    const unsigned char* mask;
    const int* pos_cell;
    __device__ void operator()(int p, double (&v)[1]) const {
        if (mask[p]) return;
        const double mean = ms[2 * size_t(pos_cell[p])], std = ms[2 * size_t(pos_cell[p]) + 1];
        v[0] = (x[p] >= mean - std && x[p] <= mean + std) ? 1.0 : 0.0;
    }
};
__global__ __launch_bounds__(kBlock) void k_stat_fin(const double* __restrict__ cv, const double* __restrict__ ms,
                                                     const double* __restrict__ within, double s2m, int nc,
                                                     double* __restrict__ stats) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= nc) return;
    double* o = stats + 6 * size_t(c);
    o[0] = cv[4 * size_t(c)];
    o[1] = ms[2 * size_t(c)] * s2m;
    o[2] = ms[2 * size_t(c) + 1] * s2m;
    o[3] = cv[4 * size_t(c) + 2] * s2m;
    o[4] = cv[4 * size_t(c) + 3] * s2m;
    o[5] = within[c];
}

__global__ __launch_bounds__(kBlock) void k_keep(const unsigned char* __restrict__ mask, int n, unsigned* __restrict__ flag) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p < n) flag[p] = mask[p] ? 0u : 1u;
}
// out[c] = the number of flagged positions before the cell's first; out[nc] = all
__global__ __launch_bounds__(kBlock) void k_ptr(const long long* __restrict__ in_ptr, const unsigned* __restrict__ incl, int nc,
                                                int n, long long* __restrict__ out) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c > nc) return;
    const long long a = c == nc ? n : in_ptr[c];
    out[c] = a == 0 ? 0 : (long long)incl[a - 1];
}
// kept[e] = the position of kept row e; second[p] = 1 for a kept row that is not its cell's first kept one
__global__ __launch_bounds__(kBlock) void k_kept(const unsigned* __restrict__ keep, const unsigned* __restrict__ incl,
                                                 const int* __restrict__ pos_cell, const long long* __restrict__ kept_ptr, int m,
                                                 unsigned* __restrict__ kept, unsigned* __restrict__ second) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= m) return;
    unsigned sec = 0;
    if (keep[p]) {
        kept[incl[p] - 1] = unsigned(p);
        sec = (long long)(incl[p] - 1) != kept_ptr[pos_cell[p]] ? 1u : 0u;
    }
    second[p] = sec;
}
// numpy: diff(x) / diff(soa1) * s2m * sample_rate over the kept rows, at the later row's rx1 timestamp
__global__ __launch_bounds__(kBlock) void k_speed(const unsigned* __restrict__ second, const unsigned* __restrict__ incl_keep,
                                                  const unsigned* __restrict__ incl_sec, const unsigned* __restrict__ kept,
                                                  const int* __restrict__ pos_cell, Rows r, Consts k, int m,
                                                  double* __restrict__ sx, double* __restrict__ sv, int* __restrict__ scell) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= m || !second[p]) return;
    const unsigned q = incl_sec[p] - 1, pp = kept[incl_keep[p] - 2];
    sv[q] = (r.x[p] - r.x[pp]) / (r.s1[p] - r.s1[pp]) * k.s2m * k.rate;
    sx[q] = r.t1rel[p];
    scell[q] = pos_cell[p];
}
__global__ __launch_bounds__(kBlock) void k_points(const unsigned* __restrict__ keep, const unsigned* __restrict__ incl,
                                                   const double* __restrict__ xs, const double* __restrict__ ys,
                                                   const int* __restrict__ cell, int n, double* __restrict__ px,
                                                   double* __restrict__ py, int* __restrict__ pcell) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n || !keep[p]) return;
    const unsigned j = incl[p] - 1;
    px[j] = xs[p];
    py[j] = ys[p];
    pcell[j] = cell[p];
}
__global__ __launch_bounds__(kBlock) void k_counts(const Cell* __restrict__ cells, const double* __restrict__ stats,
                                                   const long long* __restrict__ sp_ptr, const long long* __restrict__ dp_ptr,
                                                   int nc, long long* __restrict__ counts) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= nc) return;
    long long* o = counts + 5 * size_t(c);
    o[0] = cells[c].n;
    o[1] = cells[c].nb;
    o[2] = (long long)stats[6 * size_t(c)];
    o[3] = sp_ptr[c + 1] - sp_ptr[c];
    o[4] = dp_ptr[c + 1] - dp_ptr[c];
}

// ------------------------------------------------------------------ 5. the smoother: one wave per point
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = kPointLanes / 2; off > 0; off >>= 1) v = v + __shfl_xor(v, off, kPointLanes);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = kPointLanes / 2; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off, kPointLanes);
        v = o > v ? o : v;
    }
    return v;
}
__global__ __launch_bounds__(kBlock) void k_smooth(const double* __restrict__ px, const double* __restrict__ py,
                                                   const int* __restrict__ pcell, const long long* __restrict__ pptr,
                                                   int n_pts, double frac, double* __restrict__ out) {
    const int lane = threadIdx.x % kPointLanes;
    const long long wave = ((long long)blockIdx.x * kBlock + threadIdx.x) / kPointLanes;
    const long long n_waves = (long long)gridDim.x * (kBlock / kPointLanes);
    for (long long i = wave; i < n_pts; i += n_waves) {
        const int c = pcell[i];
        const long long a = pptr[c];
        const int m = int(pptr[c + 1] - a);
        if (m < 2 || frac == 0.0) {
            if (lane == 0) out[i] = py[i];
            continue;
        }
        int k = int(frac * double(m) + 1e-10);
        k = k < m ? k : m;
        k = k > 2 ? k : 2;
        const double* x = px + a;
        const double* y = py + a;
        const double xi = px[i];
        int lo = 0, hi = m - k;  // the smallest L for which the window would not rather start at L + 1
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;  // mid + k < m
            if (x[mid + k] - xi < xi - x[mid]) lo = mid + 1; else hi = mid;
        }
        x += lo;
        y += lo;
        double h = 0.0;
        for (int j = lane; j < k; j += kPointLanes) {
            const double d = fabs(x[j] - xi);
            h = d > h ? d : h;
        }
        h = wave_max(h);
        double sw = 0.0, swd = 0.0, swy = 0.0, swdd = 0.0, swdy = 0.0;
        for (int j = lane; j < k; j += kPointLanes) {
            const double d = x[j] - xi, yj = y[j];
            double w = 1.0;
            if (h > 0.0) {
                const double u = fabs(d) / h, t = 1.0 - (u * u) * u;
                w = (t * t) * t;
            }
            const double wd = w * d;
            sw = sw + w;
            swd = swd + wd;
            swy = swy + w * yj;
            swdd = swdd + wd * d;
            swdy = swdy + wd * yj;
        }
        sw = wave_sum(sw);
        swd = wave_sum(swd);
        swy = wave_sum(swy);
        swdd = wave_sum(swdd);
        swdy = wave_sum(swdy);
        if (lane == 0) {
            const double det = sw * swdd - swd * swd;
            out[i] = det > kSingular * (sw * swdd) ? (swdd * swy - swd * swdy) / det : swy / sw;
        }
    }
}

// the values a mask keeps as a point list (ptr, x, y into the three outputs), smoothed into `smooth`
int smooth_kept(const unsigned char* mask, const double* xs, const double* ys, const Series& S, double frac, Work& k,
                DevBuf& flag, DevBuf& incl, DevBuf& o_ptr, DevBuf& o_x, DevBuf& o_smooth, size_t* n_out, hipStream_t s) {
    unsigned n_pts = 0;
    THR_TRY(launch(k_keep, S.n, s, mask, S.n, flag.as<unsigned>()));
    THR_TRY(scan(flag.as<unsigned>(), incl.as<unsigned>(), S.n, k.w, s, &n_pts));
    DevBuf pcell, o_y;
    THR_HIP_TRY(pcell.alloc(size_t(n_pts) * 4));
    THR_HIP_TRY(o_ptr.alloc((size_t(S.nc) + 1) * 8));
    THR_HIP_TRY(o_x.alloc(size_t(n_pts) * 8));
    THR_HIP_TRY(o_y.alloc(size_t(n_pts) * 8));
    THR_HIP_TRY(o_smooth.alloc(size_t(n_pts) * 8));
    THR_TRY(launch(k_ptr, S.nc + 1, s, S.ptr, incl.as<unsigned>(), S.nc, S.n, o_ptr.as<long long>()));
    if (n_pts) {
        THR_TRY(launch(k_points, S.n, s, flag.as<unsigned>(), incl.as<unsigned>(), xs, ys, S.pos_cell, S.n, o_x.as<double>(),
                       o_y.as<double>(), pcell.as<int>()));
        const size_t groups = (size_t(n_pts) + kBlock / kPointLanes - 1) / (kBlock / kPointLanes);
        THR_TRY(launch_grid(k_smooth, dim3(unsigned(groups < kMaxSmoothGrid ? groups : kMaxSmoothGrid)), s, o_x.as<double>(),
                            o_y.as<double>(), pcell.as<int>(), o_ptr.as<long long>(), int(n_pts), frac, o_smooth.as<double>()));
    }
    THR_HIP_TRY(hipStreamSynchronize(s));  // pcell and o_y go out of scope here
    *n_out = n_pts;
    return THR_OK;
}

thread_local double g_reldist_ms[5] = {0, 0, 0, 0, 0};

bool positive(double v) { return std::isfinite(v) && v > 0.0; }

}  // namespace

struct thr_reldist_result : thr::seg::Result {};

extern "C" int thr_reldist(int device_id, size_t n_det, const int32_t* rxid, const int32_t* txid, const double* soa,
                           const double* timestamp, const double* carrier_bin, const double* carrier_offset, const int64_t* idx,
                           size_t n_matches, const int64_t* match_ptr, const int64_t* match_idx, const int32_t* beacons,
                           size_t n_beacons, const int32_t* mobiles, size_t n_mobiles, const int32_t* receivers,
                           size_t n_receivers, const thr_reldist_opts* opts, thr_reldist_result** result_out,
                           thr_reldist_counts* counts_out) try {
    if (result_out) *result_out = nullptr;
    if (counts_out) std::memset(counts_out, 0, sizeof(*counts_out));
    for (double& t : g_reldist_ms) t = 0;
    if (!result_out || !counts_out || !opts || !beacons) return thr::fail_msg(THR_ERR_ARG, "thr_reldist: null argument");
    if (n_det && (!rxid || !txid || !soa || !timestamp || !carrier_bin || !carrier_offset || !idx))
        return thr::fail_msg(THR_ERR_ARG, "thr_reldist: null argument");
    if (!match_ptr || (n_matches && match_ptr[n_matches] && !match_idx) || (opts->n_geometry && !opts->geometry))
        return thr::fail_msg(THR_ERR_ARG, "thr_reldist: null argument");
    if (n_det > (size_t(1) << 28) || n_matches > (size_t(1) << 28) || n_beacons > (size_t(1) << 20) ||
        n_mobiles > (size_t(1) << 20) || n_receivers > (size_t(1) << 20) || opts->n_geometry > (size_t(1) << 20))
        return thr::fail_msg(THR_ERR_ARG, "thr_reldist: too many detections, matches or list entries");
    if (opts->method != THR_RELDIST_NEAREST && opts->method != THR_RELDIST_LINPOL)
        return thr::fail_msg(THR_ERR_ARG, "thr_reldist: method must be THR_RELDIST_NEAREST or THR_RELDIST_LINPOL, not %d", opts->method);
    if (!(opts->smooth_frac >= 0.0 && opts->smooth_frac <= 1.0))
        return thr::fail_msg(THR_ERR_ARG, "thr_reldist: smooth_frac must lie in [0, 1], not %g", opts->smooth_frac);
    if (!positive(opts->sample_rate) || !positive(opts->block_len) || !positive(opts->carrier_hz) || opts->thresh != opts->thresh)
        return thr::fail_msg(THR_ERR_ARG, "thr_reldist: sample_rate, block_len and carrier_hz must be positive, thresh a number");
    uint64_t n_pairs = 0;
    THR_TRY(check_matches("thr_reldist", n_det, rxid, n_matches, match_ptr, match_idx, &n_pairs));
    const size_t n_entries = size_t(match_ptr[n_matches]);

    THR_TRY(pick_device(device_id));
    thr_reldist_result* R = new thr_reldist_result;
    ResultGuard guard{R};
    R->device = device_id;
    R->n_out = THR_RELDIST_N_OUTPUTS;
    hipStream_t s = nullptr;
    Event ev[5];
    for (Event& e : ev) THR_HIP_TRY(e.create());
    for (Event& e : R->ev) THR_HIP_TRY(e.create());

    // ---- copies in
    DevBuf d_rx, d_tx, d_f64[4], d_mptr, d_midx, d_bl, d_ml, d_rl;
    const double* h_f64[4] = {soa, timestamp, carrier_bin, carrier_offset};
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
    THR_TRY(upload_list(mobiles, n_mobiles, d_ml, D.n_mobiles));
    THR_TRY(upload_list(receivers, n_receivers, d_rl, D.n_receivers));
    THR_HIP_TRY(hipEventRecord(ev[1].e, s));
    D.rx = d_rx.as<int>();
    D.tx = d_tx.as<int>();
    D.soa = d_f64[0].as<double>();
    D.ts = d_f64[1].as<double>();
    D.cbin = d_f64[2].as<double>();
    D.coff = d_f64[3].as<double>();
    D.mptr = d_mptr.as<long long>();
    D.midx = d_midx.as<long long>();
    D.beacons = d_bl.as<int>();
    D.mobiles = d_ml.as<int>();
    D.receivers = d_rl.as<int>();
    Consts K;
    K.method = opts->method;
    K.s2m = kLight / opts->sample_rate;
    K.rate = opts->sample_rate;
    K.hz_per_bin = opts->sample_rate / opts->block_len;
    K.carrier = opts->carrier_hz;
    K.thresh = opts->thresh;
    K.frac = opts->smooth_frac;

    // ---- 1. groups
    Scratch w;
    Work W{w};
    PairRows src;
    DevBuf d_gptr, d_gkey, d_src_i64[2], d_src_f64[5];
    THR_TRY(pair_rows(TxPairs{D}, int(n_matches), w, src, d_gptr, d_gkey, s));
    if (src.m == 0) return thr::fail_msg(THR_ERR_ARG, "thr_reldist: the selection is empty");
    const int ns = src.m;
    const Cells& groups = src.cells;
    const int ng = groups.nc;
    THR_HIP_TRY(d_src_i64[0].alloc(size_t(ns) * 16));
    THR_HIP_TRY(d_src_i64[1].alloc(size_t(ns) * 8));
    for (DevBuf& b : d_src_f64) THR_HIP_TRY(b.alloc(size_t(ns) * 8));
    Src G{d_src_i64[0].as<long long>(), d_src_i64[1].as<long long>(), d_src_f64[0].as<double>(), d_src_f64[1].as<double>(),
          d_src_f64[2].as<double>(),    d_src_f64[3].as<double>(),    d_src_f64[4].as<double>()};
    THR_TRY(launch(k_src, ns, s, D, groups.perm.as<unsigned>(), src.det.as<long long>(), src.match.as<long long>(), ns, G));
    std::vector<int32_t> h_gkey(size_t(ng) * 3);
    std::vector<long long> h_gptr(size_t(ng) + 1);
    std::vector<double> h_gbad(size_t(ng) * 2);
    {
        Layout LG;
        DevBuf d_gslab, d_gbad;
        THR_TRY(build_layout(groups.pos_cell.as<int>(), ns, ng, w, LG, s));
        THR_HIP_TRY(d_gslab.alloc(size_t(LG.nf) * 2 * 8));
        THR_HIP_TRY(d_gbad.alloc(size_t(ng) * 2 * 8));
        THR_TRY((reduce<2, 2, 0>(LoadOrder{G.s0, G.t0, groups.pos_cell.as<int>(), ns}, LG, d_gslab.as<double>(), d_gbad.as<double>(), s)));
        THR_HIP_TRY(hipMemcpy(h_gbad.data(), d_gbad.p, h_gbad.size() * 8, hipMemcpyDeviceToHost));  // synchronises
        THR_HIP_TRY(hipMemcpy(h_gkey.data(), d_gkey.p, h_gkey.size() * 4, hipMemcpyDeviceToHost));
        THR_HIP_TRY(hipMemcpy(h_gptr.data(), d_gptr.p, h_gptr.size() * 8, hipMemcpyDeviceToHost));
    }

    // ---- 2. cells: every mobile group with every beacon's group of the same receivers
    std::vector<int32_t> bl(beacons, beacons + n_beacons), ml;
    std::sort(bl.begin(), bl.end());
    bl.erase(std::unique(bl.begin(), bl.end()), bl.end());
    if (mobiles) ml.assign(mobiles, mobiles + n_mobiles);
    std::sort(ml.begin(), ml.end());
    std::vector<Cell> cells;
    const bool smoothing = opts->smooth_frac > 0.0;
    for (int g = 0; g < ng; ++g) {
        const int32_t* key = &h_gkey[size_t(g) * 3];
        const bool is_beacon = std::binary_search(bl.begin(), bl.end(), key[0]);
        if (mobiles ? !std::binary_search(ml.begin(), ml.end(), key[0]) : is_beacon) continue;
        for (const int32_t b : bl) {
            if (b == key[0]) continue;
            Cell c{};
            c.key[0] = key[0];
            c.key[1] = b;
            c.key[2] = key[1];
            c.key[3] = key[2];
            c.msrc = h_gptr[g];
            c.n = int(h_gptr[g + 1] - h_gptr[g]);
            int bg = -1;  // the groups are ordered by their key
            for (int lo = 0, hi = ng; lo < hi;) {
                const int mid = (lo + hi) >> 1;
                const int32_t* k2 = &h_gkey[size_t(mid) * 3];
                const int32_t want[3] = {b, key[1], key[2]};
                if (std::lexicographical_compare(k2, k2 + 3, want, want + 3)) {
                    lo = mid + 1;
                } else {
                    hi = mid;
                    if (std::equal(k2, k2 + 3, want)) bg = mid;
                }
            }
            if (bg < 0) {
                c.flags = THR_RELDIST_CELL_NO_BEACON;
            } else {
                c.bsrc = h_gptr[bg];
                c.nb = int(h_gptr[bg + 1] - h_gptr[bg]);
                if (h_gbad[size_t(bg) * 2] > 0.0 || (smoothing && h_gbad[size_t(g) * 2 + 1] > 0.0)) c.flags = THR_RELDIST_CELL_UNSORTED;
            }
            for (size_t i = 0; i < opts->n_geometry; ++i) {
                const thr_reldist_geom& q = opts->geometry[i];
                if (q.beacon == b && q.rx0 == key[1] && q.rx1 == key[2]) {
                    c.geo[0] = q.d_beacon;
                    c.geo[1] = q.dist_rx;
                    c.geo[2] = q.dist_beacon;
                    break;
                }
            }
            cells.push_back(c);
        }
    }
    if (cells.empty()) return thr::fail_msg(THR_ERR_ARG, "thr_reldist: the selection is empty");
    std::sort(cells.begin(), cells.end(),
              [](const Cell& a, const Cell& b) { return std::lexicographical_compare(a.key, a.key + 4, b.key, b.key + 4); });
    uint64_t total = 0;
    for (Cell& c : cells) {
        c.start = (long long)total;
        total += uint64_t(c.n);
    }
    if (total > (uint64_t(1) << 28) || cells.size() > (size_t(1) << 28)) return thr::fail_msg(THR_ERR_ARG, "thr_reldist: too many rows");
    const int m = int(total), nc = int(cells.size());
    DevBuf d_cells, d_pos_cell;
    DevBuf* O = R->out;
    THR_HIP_TRY(d_cells.alloc(cells.size() * sizeof(Cell)));
    THR_HIP_TRY(hipMemcpy(d_cells.p, cells.data(), cells.size() * sizeof(Cell), hipMemcpyHostToDevice));
    THR_HIP_TRY(d_pos_cell.alloc(size_t(m) * 4));
    THR_HIP_TRY(O[THR_RELDIST_CELL_KEY].alloc(size_t(nc) * 16));
    THR_HIP_TRY(O[THR_RELDIST_CELL_PTR].alloc((size_t(nc) + 1) * 8));
    THR_HIP_TRY(O[THR_RELDIST_CELL_FLAGS].alloc(size_t(nc) * 4));
    const Cell* dc = d_cells.as<Cell>();
    const int* pos_cell = d_pos_cell.as<int>();
    const long long* cell_ptr = O[THR_RELDIST_CELL_PTR].as<long long>();
    THR_TRY(launch(k_pos_cell, m, s, dc, nc, m, d_pos_cell.as<int>()));
    THR_TRY(launch(k_cell_out, nc, s, dc, nc, m, O[THR_RELDIST_CELL_KEY].as<int>(), O[THR_RELDIST_CELL_PTR].as<long long>(),
                   O[THR_RELDIST_CELL_FLAGS].as<int>()));
    THR_HIP_TRY(hipEventRecord(ev[2].e, s));

    // ---- 3. rows
    DevBuf d_s1, d_t0rel, d_t1rel;
    for (DevBuf* b : {&d_s1, &d_t0rel, &d_t1rel, &O[THR_RELDIST_RAW], &O[THR_RELDIST_X], &O[THR_RELDIST_DOP], &O[THR_RELDIST_ROW_MATCH]})
        THR_HIP_TRY(b->alloc(size_t(m) * 8));
    for (DevBuf* b : {&O[THR_RELDIST_NEAREST_IDX], &O[THR_RELDIST_HI], &O[THR_RELDIST_ROW_FLAGS]}) THR_HIP_TRY(b->alloc(size_t(m) * 4));
    for (DevBuf* b : {&O[THR_RELDIST_MASK1], &O[THR_RELDIST_MASK3]}) THR_HIP_TRY(b->alloc(size_t(m)));
    THR_HIP_TRY(O[THR_RELDIST_ROW_DET].alloc(size_t(m) * 16));
    Rows Rw{O[THR_RELDIST_ROW_DET].as<long long>(), O[THR_RELDIST_ROW_MATCH].as<long long>(), O[THR_RELDIST_NEAREST_IDX].as<int>(),
            O[THR_RELDIST_HI].as<int>(),            O[THR_RELDIST_ROW_FLAGS].as<int>(),       O[THR_RELDIST_RAW].as<double>(),
            O[THR_RELDIST_X].as<double>(),          O[THR_RELDIST_DOP].as<double>(),          d_s1.as<double>(),
            d_t0rel.as<double>(),                   d_t1rel.as<double>()};
    THR_TRY(launch(k_rel, m, s, dc, pos_cell, G, K, m, Rw));

    // ---- 4. mask 1, the statistics, the speeds, masks 2 and 3
    if (ns < m) {  // every beacon repeats a mobile's rows: head and incl hold the larger count
        THR_HIP_TRY(w.head.alloc(size_t(m) * 4));
        THR_HIP_TRY(w.incl.alloc(size_t(m) * 4));
    }
    Series SR;
    SR.n = m;
    SR.nc = nc;
    SR.pos_cell = pos_cell;
    SR.ptr = cell_ptr;
    THR_TRY(build_layout(pos_cell, m, nc, w, SR.L, s));
    DevBuf d_cv, d_cv2, d_ms, d_within, d_keep, d_kincl, d_sec, d_sincl, d_kept, d_kptr, d_scell, d_flag, d_fincl, d_slab, d_probe;
    THR_HIP_TRY(W.sorted.alloc(size_t(m) * 8));
    THR_HIP_TRY(W.dev.alloc(size_t(m) * 8));
    THR_HIP_TRY(d_slab.alloc(size_t(tiles_of(m) + nc) * 4 * 8));  // no layout of at most m positions has more fragments
    THR_HIP_TRY(d_probe.alloc(size_t(nc) * 8));
    THR_HIP_TRY(d_cv.alloc(size_t(nc) * 4 * 8));
    THR_HIP_TRY(d_cv2.alloc(size_t(nc) * 8));
    THR_HIP_TRY(d_ms.alloc(size_t(nc) * 2 * 8));
    THR_HIP_TRY(d_within.alloc(size_t(nc) * 8));
    THR_HIP_TRY(d_kptr.alloc((size_t(nc) + 1) * 8));
    for (DevBuf* b : {&d_keep, &d_kincl, &d_sec, &d_sincl, &d_kept, &d_flag, &d_fincl}) THR_HIP_TRY(b->alloc(size_t(m) * 4));
    THR_HIP_TRY(O[THR_RELDIST_MEDIANS].alloc(size_t(nc) * 6 * 8));
    THR_HIP_TRY(O[THR_RELDIST_CELL_STATS].alloc(size_t(nc) * 6 * 8));
    THR_HIP_TRY(O[THR_RELDIST_CELL_COUNTS].alloc(size_t(nc) * 5 * 8));
    THR_HIP_TRY(O[THR_RELDIST_SPEED_PTR].alloc((size_t(nc) + 1) * 8));
    double *med = O[THR_RELDIST_MEDIANS].as<double>(), *slab = d_slab.as<double>();
    const double* x = O[THR_RELDIST_X].as<double>();
    const unsigned char* mask1 = O[THR_RELDIST_MASK1].as<unsigned char>();
    THR_TRY(masked(x, SR, K.thresh, W, slab, d_probe.as<double>(), med, O[THR_RELDIST_MASK1].as<unsigned char>(), s));
    const double *cv = d_cv.as<double>(), *ms = d_ms.as<double>();
    THR_TRY((reduce<4, 2, 1>(LoadKept1<false>{x, mask1}, SR.L, slab, d_cv.as<double>(), s)));
    THR_TRY((reduce<1, 1, 0>(LoadKept2<false>{x, cv, mask1, pos_cell}, SR.L, slab, d_cv2.as<double>(), s)));
    THR_TRY(launch(k_mean_std, nc, s, cv, d_cv2.as<double>(), nc, d_ms.as<double>()));
    THR_TRY((reduce<1, 1, 0>(LoadSt3{x, ms, mask1, pos_cell}, SR.L, slab, d_within.as<double>(), s)));
    THR_TRY(launch(k_stat_fin, nc, s, cv, ms, d_within.as<double>(), K.s2m, nc, O[THR_RELDIST_CELL_STATS].as<double>()));
    // the speeds: one per kept row that has a kept row before it in its cell
    unsigned n_kept = 0, n_speed = 0;
    THR_TRY(launch(k_keep, m, s, mask1, m, d_keep.as<unsigned>()));
    THR_TRY(scan(d_keep.as<unsigned>(), d_kincl.as<unsigned>(), m, w, s, &n_kept));
    THR_TRY(launch(k_ptr, nc + 1, s, cell_ptr, d_kincl.as<unsigned>(), nc, m, d_kptr.as<long long>()));
    THR_TRY(launch(k_kept, m, s, d_keep.as<unsigned>(), d_kincl.as<unsigned>(), pos_cell, d_kptr.as<long long>(), m,
                   d_kept.as<unsigned>(), d_sec.as<unsigned>()));
    THR_TRY(scan(d_sec.as<unsigned>(), d_sincl.as<unsigned>(), m, w, s, &n_speed));
    THR_TRY(launch(k_ptr, nc + 1, s, cell_ptr, d_sincl.as<unsigned>(), nc, m, O[THR_RELDIST_SPEED_PTR].as<long long>()));
    THR_HIP_TRY(O[THR_RELDIST_SPEED_X].alloc(size_t(n_speed) * 8));
    THR_HIP_TRY(O[THR_RELDIST_SPEED].alloc(size_t(n_speed) * 8));
    THR_HIP_TRY(O[THR_RELDIST_MASK2].alloc(size_t(n_speed)));
    THR_HIP_TRY(d_scell.alloc(size_t(n_speed) * 4));
    THR_TRY(launch(k_speed, m, s, d_sec.as<unsigned>(), d_kincl.as<unsigned>(), d_sincl.as<unsigned>(), d_kept.as<unsigned>(),
                   pos_cell, Rw, K, m, O[THR_RELDIST_SPEED_X].as<double>(), O[THR_RELDIST_SPEED].as<double>(), d_scell.as<int>()));
    Series SS;
    SS.n = int(n_speed);
    SS.nc = nc;
    SS.pos_cell = d_scell.as<int>();
    SS.ptr = O[THR_RELDIST_SPEED_PTR].as<long long>();
    if (SS.n) THR_TRY(build_layout(SS.pos_cell, SS.n, nc, w, SS.L, s));
    THR_TRY(masked(O[THR_RELDIST_SPEED].as<double>(), SS, K.thresh, W, slab, d_probe.as<double>(), med + 2, O[THR_RELDIST_MASK2].as<unsigned char>(), s));
    THR_TRY(masked(O[THR_RELDIST_DOP].as<double>(), SR, K.thresh, W, slab, d_probe.as<double>(), med + 4, O[THR_RELDIST_MASK3].as<unsigned char>(), s));
    THR_HIP_TRY(hipEventRecord(ev[3].e, s));

    // ---- 5. the smoothers
    size_t n_sp = 0, n_dp = 0;
    THR_TRY(smooth_kept(O[THR_RELDIST_MASK2].as<unsigned char>(), O[THR_RELDIST_SPEED_X].as<double>(), O[THR_RELDIST_SPEED].as<double>(),
                        SS, K.frac, W, d_flag, d_fincl, O[THR_RELDIST_SPEED_SMOOTH_PTR], O[THR_RELDIST_SPEED_SMOOTH_X],
                        O[THR_RELDIST_SPEED_SMOOTH], &n_sp, s));
    THR_TRY(smooth_kept(O[THR_RELDIST_MASK3].as<unsigned char>(), d_t0rel.as<double>(), O[THR_RELDIST_DOP].as<double>(), SR, K.frac, W,
                        d_flag, d_fincl, O[THR_RELDIST_DOP_SMOOTH_PTR], O[THR_RELDIST_DOP_SMOOTH_X], O[THR_RELDIST_DOP_SMOOTH], &n_dp, s));
    THR_TRY(launch(k_counts, nc, s, dc, O[THR_RELDIST_CELL_STATS].as<double>(), O[THR_RELDIST_SPEED_SMOOTH_PTR].as<long long>(),
                   O[THR_RELDIST_DOP_SMOOTH_PTR].as<long long>(), nc, O[THR_RELDIST_CELL_COUNTS].as<long long>()));
    THR_HIP_TRY(hipEventRecord(ev[4].e, s));
    THR_TRY(record_times(ev, g_reldist_ms));  // synchronises: the temporaries go out of scope

    size_t* B = R->bytes;
    B[THR_RELDIST_CELL_KEY] = size_t(nc) * 16;
    B[THR_RELDIST_CELL_PTR] = B[THR_RELDIST_SPEED_PTR] = B[THR_RELDIST_SPEED_SMOOTH_PTR] = B[THR_RELDIST_DOP_SMOOTH_PTR] =
        (size_t(nc) + 1) * 8;
    B[THR_RELDIST_ROW_DET] = size_t(m) * 16;
    B[THR_RELDIST_ROW_MATCH] = B[THR_RELDIST_RAW] = B[THR_RELDIST_X] = B[THR_RELDIST_DOP] = size_t(m) * 8;
    B[THR_RELDIST_NEAREST_IDX] = B[THR_RELDIST_HI] = B[THR_RELDIST_ROW_FLAGS] = size_t(m) * 4;
    B[THR_RELDIST_MASK1] = B[THR_RELDIST_MASK3] = size_t(m);
    B[THR_RELDIST_CELL_STATS] = B[THR_RELDIST_MEDIANS] = size_t(nc) * 6 * 8;
    B[THR_RELDIST_CELL_COUNTS] = size_t(nc) * 5 * 8;
    B[THR_RELDIST_SPEED_X] = B[THR_RELDIST_SPEED] = size_t(n_speed) * 8;
    B[THR_RELDIST_MASK2] = size_t(n_speed);
    B[THR_RELDIST_SPEED_SMOOTH_X] = B[THR_RELDIST_SPEED_SMOOTH] = n_sp * 8;
    B[THR_RELDIST_DOP_SMOOTH_X] = B[THR_RELDIST_DOP_SMOOTH] = n_dp * 8;
    B[THR_RELDIST_CELL_FLAGS] = size_t(nc) * 4;
    counts_out->rows = size_t(m);
    counts_out->cells = size_t(nc);
    counts_out->speeds = size_t(n_speed);
    counts_out->speed_points = n_sp;
    counts_out->dop_points = n_dp;
    *result_out = R;
    guard.r = nullptr;
    return THR_OK;
} catch (const std::bad_alloc&) {
    return thr::fail_msg(THR_ERR_DEVICE, "thr_reldist: out of host memory");
} catch (...) {
    return thr::on_exception("thr_reldist");
}

extern "C" int thr_reldist_fetch(thr_reldist_result* R, int which, void* dst, size_t dst_bytes) try {
    return fetch("thr_reldist_fetch", R, which, dst, dst_bytes, &g_reldist_ms[4]);
} catch (...) {
    return thr::on_exception("thr_reldist_fetch");
}

extern "C" void thr_reldist_free(thr_reldist_result* R) { free_result(R); }

extern "C" int thr_debug_reldist_times(double* ms_out) try {
    return copy_times("thr_debug_reldist_times", g_reldist_ms, ms_out);
} catch (...) {
    return thr::on_exception("thr_debug_reldist_times");
}

extern "C" int thr_debug_reldist_geometry(int* tile_len, int* workgroup, int* point_lanes) try {
    return geometry("thr_debug_reldist_geometry", tile_len, workgroup, point_lanes, kPointLanes);
} catch (...) {
    return thr::on_exception("thr_debug_reldist_geometry");
}
