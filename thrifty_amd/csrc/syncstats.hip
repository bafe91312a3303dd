// Clock-sync quality on the device: the numbers of the reference's `thrifty analyze_beacon`
// (beacon_analysis.py: analyze, fit_poly_model) for EVERY (beacon, rx0 < rx1) cell in one call, and of
// `thrifty analyze_tdoa` (tdoa_analysis.py, with stat_tools.is_outlier as scripts/tdoa_matrix.py applies it)
// for every (rx0, rx1, tx) cell of a .tdoa matrix.
//
// thr_beaconsync
//   1. rows             one thread per match counts and then emits the detection pairs it holds (beacon and
//                       receiver lists are sorted on the host and searched by bisection; the id range is
//                       applied here); two stable hipCUB radix sorts (by rx1, then by (beacon, rx0)) leave the
//                       rows grouped by cell in match order; head flags, one scan, the cell table;
//   2. discontinuities  sdoa and dsdoa are one subtraction each; a cell's sum of dsdoa is a tiled segmented
//                       reduction (below); flags dsdoa > (sum / count) * 10, one scan of them gives the
//                       discontinuity CSR and every row's cut; the cut table is one thread per cut;
//   3. fits             per cut, two reductions (means and extremes; then the moments of
//                       u = (soa0 - mean) / max|soa0 - mean| against w = sdoa - mean), a (deg + 1)-square
//                       solve per cut, the residual of every row; soa1 = soa0 + sdoa, so the polynomial of
//                       soa1 on u is the one of w plus x_scale * u and the means (sdoa is five orders of
//                       magnitude smaller than soa1: the fit loses nothing to the size of the SOAs);
//   4. summary          per cell: std of the residuals (two passes), largest magnitude, mean of the cuts' snr.
// thr_tdoastats
//   filter by scan and scatter; the same two sorts by (rx0, rx1, tx); count, mean, std (two passes), RMS, min,
//   max; with `robust`, values and then deviations sorted by (cell, value) -- a sort by value followed by a
//   stable sort by cell -- give median and MAD, the mask is numpy's three float64 operations, and the same
//   statistics are taken again over the rows the mask keeps.
//
// Every reduction is seg_reduce.hpp's: tiles, fragments, a segmented scan through LDS, a slab, a combining
// launch (the form and why it returns the same bits every time are described there).  What reldist.hip needs
// too is seg_cells.hpp's: the host pass over the matches and the rows of detection pairs (check_matches,
// pair_rows: this file brings the selector), the row sorts, the layouts (build_layout: the fragments of the
// cells, then of the cuts), the outlier mask and the statistics of the rows it keeps.  This file brings one
// load functor per reduction of its own.
//
// Lifetimes: everything runs on the null stream.  A temporary that a queued kernel may still use is released
// in two ways only: after an explicit synchronisation (record_times' hipEventSynchronize at the end of a call,
// the hipStreamSynchronize that ends the robust part, the hipMemcpy that reads a count back), or by hipFree,
// which HIP defines to wait for the device first -- with_temp relies on that when the hipCUB temporary grows,
// and so does an early error return.  The buffers of the repeated sorts live in Scratch, so that the robust
// part does not pay that wait once per sort.
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

// the threshold and the outlier mask repeat numpy's float64 operations one by one: no a * b + c may become
// an fma in this file (the build also passes -ffp-contract=off, thrifty_amd/build.py)
#pragma clang fp contract(off)

namespace {

using thr::DevBuf;
using thr::Event;
using namespace thr::seg;  // kBlock, kTile, the keys, the reduction, Result and its fetch

constexpr int kMinCut = 8;   // a cut with left + kMinCut >= right is not fitted
constexpr double kLight = 2.997e8;

// ------------------------------------------------------------------ beacon sync: rows
struct Dets {
    const int *rx, *tx;
    const double *soa, *en, *no;
    const long long *id, *mptr, *midx;
    const int *beacons, *receivers;
    int n_beacons, n_receivers;  // -1: no list
    int has_range;
    long long lo, hi;
};
struct BeaconPairs {  // k_pairs' selector: matches of the listed beacons, pairs of listed receivers inside the id range
    Dets d;
    __device__ bool wanted(int tx) const { return find_sorted(d.beacons, d.n_beacons, tx) >= 0; }
    __device__ bool kept(long long da, long long db) const {
        if (find_sorted(d.receivers, d.n_receivers, d.rx[da]) < 0 || find_sorted(d.receivers, d.n_receivers, d.rx[db]) < 0)
            return false;
        if (!d.has_range) return true;
        const long long ia = d.id[da], ib = d.id[db];
        return ia >= d.lo && ia <= d.hi && ib >= d.lo && ib <= d.hi;
    }
};
// per position: the row's detections and match, sdoa, soa at rx0, the two detections' energy^2 / noise^2 summed
__global__ __launch_bounds__(kBlock) void k_rows(Dets d, const unsigned* __restrict__ perm, const long long* __restrict__ det,
                                                 const long long* __restrict__ match, int m, long long* __restrict__ row_det,
                                                 long long* __restrict__ row_match, double* __restrict__ sdoa,
                                                 double* __restrict__ soa0, double* __restrict__ snr2) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= m) return;
    const size_t j = perm[p];
    const long long d0 = det[2 * j], d1 = det[2 * j + 1];
    row_det[2 * size_t(p)] = d0;
    row_det[2 * size_t(p) + 1] = d1;
    row_match[p] = match[j];
    const double s0 = d.soa[d0], s1 = d.soa[d1];
    sdoa[p] = s1 - s0;
    soa0[p] = s0;
    const double e0 = d.en[d0], n0 = d.no[d0], e1 = d.en[d1], n1 = d.no[d1];
    snr2[p] = (e0 * e0) / (n0 * n0) + (e1 * e1) / (n1 * n1);
}

// ------------------------------------------------------------------ beacon sync: discontinuities and cuts
struct LoadDsdoa {  // dsdoa[k] lives at row k; a cell's last row has none
    const double* sdoa;
    const int* pos_cell;
    int m;
    __device__ void operator()(int p, double (&v)[1]) const {
        v[0] = (p + 1 < m && pos_cell[p + 1] == pos_cell[p]) ? sdoa[p + 1] - sdoa[p] : 0.0;
    }
};
// flag[p] = dsdoa > mean * 10 (strict; a NaN on either side is no discontinuity); the mean is ONE division
__global__ __launch_bounds__(kBlock) void k_disc_flags(const double* __restrict__ sdoa, const int* __restrict__ pos_cell,
                                                       const long long* __restrict__ cell_ptr, const double* __restrict__ cell_sum,
                                                       int m, unsigned* __restrict__ flag, double* __restrict__ cell_stats) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= m) return;
    const int c = pos_cell[p];
    const long long n = cell_ptr[c + 1] - cell_ptr[c], k = p - cell_ptr[c];
    const double mean = cell_sum[c] / double(n - 1);  // one row: 0 / 0, NaN as numpy's mean of nothing
    if (k == 0) cell_stats[4 * size_t(c)] = mean;
    flag[p] = (k < n - 1 && (sdoa[p + 1] - sdoa[p]) > mean * 10.0) ? 1u : 0u;
}
// cut_seg[p]: the global cut of row p = excl[p] + c (every cell has one cut more than discontinuities), -1
// for a cell's row 0 and for a discontinuity row, which belong to no cut
__global__ __launch_bounds__(kBlock) void k_disc_layout(const unsigned* __restrict__ flag, const unsigned* __restrict__ incl,
                                                        const int* __restrict__ pos_cell, const long long* __restrict__ cell_ptr,
                                                        int m, int nc, long long* __restrict__ disc_ptr,
                                                        long long* __restrict__ disc_idx, long long* __restrict__ cut_ptr,
                                                        int* __restrict__ cut_seg) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= m) return;
    const int c = pos_cell[p];
    const unsigned fl = flag[p], excl = incl[p] - fl;
    const long long k = p - cell_ptr[c];
    if (k == 0) {
        disc_ptr[c] = excl;
        cut_ptr[c] = (long long)excl + c;
    }
    if (p == m - 1) {
        disc_ptr[nc] = incl[p];
        cut_ptr[nc] = (long long)incl[p] + nc;
    }
    if (fl) disc_idx[excl] = k;
    cut_seg[p] = (k == 0 || fl) ? -1 : int(excl) + c;
}
// one thread per cut: its cell (bisection in cut_ptr), left = edges[i] + 1, right = edges[i + 1]
__global__ __launch_bounds__(kBlock) void k_cuts(const long long* __restrict__ cut_ptr, const long long* __restrict__ disc_ptr,
                                                 const long long* __restrict__ disc_idx, const long long* __restrict__ cell_ptr,
                                                 int nc, int n_cuts, int* __restrict__ cut_cell, long long* __restrict__ left,
                                                 long long* __restrict__ right) {
    const int g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= n_cuts) return;
    int lo = 0, hi = nc;  // the last c with cut_ptr[c] <= g
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cut_ptr[mid] <= g) lo = mid; else hi = mid;
    }
    const int c = lo;
    const long long i = g - cut_ptr[c], nd = disc_ptr[c + 1] - disc_ptr[c];
    cut_cell[g] = c;
    left[g] = (i == 0 ? 0 : disc_idx[disc_ptr[c] + i - 1]) + 1;
    right[g] = i == nd ? cell_ptr[c + 1] - cell_ptr[c] : disc_idx[disc_ptr[c] + i];
}

// ------------------------------------------------------------------ beacon sync: fits
struct LoadCut1 {  // sums of soa0, sdoa, snr; min and max of soa0
    const double *soa0, *sdoa, *snr2;
    __device__ void operator()(int p, double (&v)[5]) const {
        const double x = soa0[p];
        v[0] = x;
        v[1] = sdoa[p];
        v[2] = snr2[p];
        v[3] = x;
        v[4] = x;
    }
};
// cut_par[g] = {x_mean, x_scale, mean of sdoa}; snr = sum / (2 * rows).  fl(x - mean) is monotone in x, so
// the largest magnitude is taken at the smallest or the largest soa0.
__global__ __launch_bounds__(kBlock) void k_cut_mid(const double* __restrict__ cv, const long long* __restrict__ left,
                                                    const long long* __restrict__ right, int n_cuts,
                                                    double* __restrict__ cut_par, double* __restrict__ cut_snr,
                                                    int* __restrict__ cut_flags) {
    const int g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= n_cuts) return;
    const double* v = cv + size_t(g) * 5;
    const long long l = left[g], r = right[g];
    int fl = 0;
    double xm = NAN, sc = NAN, sm = NAN, snr = NAN;
    if (l + kMinCut < r) {
        const double n = double(r - l);
        xm = v[0] / n;
        sm = v[1] / n;
        snr = v[2] / (2.0 * n);
        sc = fmax(fabs(v[4] - xm), fabs(v[3] - xm));
        fl = (v[3] < v[4] && isfinite(sc) && isfinite(sm)) ? THR_BSYNC_CUT_FITTED : THR_BSYNC_CUT_DEGENERATE;
    }
    cut_par[3 * size_t(g)] = xm;
    cut_par[3 * size_t(g) + 1] = sc;
    cut_par[3 * size_t(g) + 2] = sm;
    cut_snr[g] = fl == THR_BSYNC_CUT_FITTED ? snr : NAN;
    cut_flags[g] = fl;
}
struct LoadCut2 {  // sums of u^1..u^6 and of w, u w, u^2 w, u^3 w
    const double *soa0, *sdoa, *cut_par;
    const int *cut_seg, *cut_flags;
    __device__ void operator()(int p, double (&v)[10]) const {
        const int g = cut_seg[p];
        if (g < 0 || cut_flags[g] != THR_BSYNC_CUT_FITTED) return;
        const double* par = cut_par + 3 * size_t(g);
        const double u = (soa0[p] - par[0]) / par[1], w = sdoa[p] - par[2];
        double pw = u;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            v[k] = pw;
            pw = pw * u;
        }
        v[6] = w;
        v[7] = u * w;
        v[8] = (u * u) * w;
        v[9] = ((u * u) * u) * w;
    }
};
// Gaussian elimination with partial pivoting, n <= 4; false when a pivot is zero or not finite
__device__ bool solve_small(int n, double (&A)[4][4], double (&b)[4]) {
    for (int col = 0; col < n; ++col) {
        int piv = col;
        for (int r = col + 1; r < n; ++r)
            if (fabs(A[r][col]) > fabs(A[piv][col])) piv = r;
        if (!(fabs(A[piv][col]) > 0.0) || !isfinite(A[piv][col])) return false;
        if (piv != col) {
            for (int k = 0; k < n; ++k) {
                const double t = A[col][k];
                A[col][k] = A[piv][k];
                A[piv][k] = t;
            }
            const double t = b[col];
            b[col] = b[piv];
            b[piv] = t;
        }
        for (int r = col + 1; r < n; ++r) {
            const double f = A[r][col] / A[col][col];
            for (int k = col; k < n; ++k) A[r][k] = A[r][k] - f * A[col][k];
            b[r] = b[r] - f * b[col];
        }
    }
    for (int r = n - 1; r >= 0; --r) {
        double acc = b[r];
        for (int k = r + 1; k < n; ++k) acc = acc - A[r][k] * b[k];
        b[r] = acc / A[r][r];
    }
    return true;
}
// cut_c[g][4]: the polynomial of w on u.  fit[g] = {x_mean, x_scale, y_mean, c0..c3} of soa1 - y_mean on u:
// soa1 = soa0 + sdoa = (x_mean + x_scale u) + (s_mean + w), so y_mean = fl(x_mean + s_mean), the rounding
// error of that sum (exact, two-sum) goes to c0 and x_scale to c1.
__global__ __launch_bounds__(kBlock) void k_cut_fit(const double* __restrict__ mv, const double* __restrict__ cut_par,
                                                    const long long* __restrict__ left, const long long* __restrict__ right,
                                                    const int* __restrict__ cut_cell, const long long* __restrict__ cell_ptr,
                                                    const double* __restrict__ soa0, int deg, int n_cuts,
                                                    int* __restrict__ cut_flags, double* __restrict__ cut_c,
                                                    double* __restrict__ fit, double* __restrict__ cut_snr,
                                                    double* __restrict__ disc_soa) {
    const int g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= n_cuts) return;
    double* f = fit + 7 * size_t(g);
    double* cc = cut_c + 4 * size_t(g);
    for (int k = 0; k < 7; ++k) f[k] = NAN;
    for (int k = 0; k < 4; ++k) cc[k] = NAN;
    disc_soa[g] = NAN;
    if (cut_flags[g] != THR_BSYNC_CUT_FITTED) return;
    const double* v = mv + size_t(g) * 10;
    double S[7], A[4][4], b[4];
    S[0] = double(right[g] - left[g]);
    for (int k = 1; k <= 6; ++k) S[k] = v[k - 1];
    for (int i = 0; i < 4; ++i) {
        b[i] = v[6 + i];
        for (int j = 0; j < 4; ++j) A[i][j] = S[i + j];
    }
    bool ok = solve_small(deg + 1, A, b);
    for (int k = 0; k <= deg; ++k) ok = ok && isfinite(b[k]);
    if (!ok) {
        cut_flags[g] = THR_BSYNC_CUT_DEGENERATE;
        cut_snr[g] = NAN;
        return;
    }
    for (int k = 0; k < 4; ++k) cc[k] = k <= deg ? b[k] : 0.0;
    const double xm = cut_par[3 * size_t(g)], sc = cut_par[3 * size_t(g) + 1], sm = cut_par[3 * size_t(g) + 2];
    const double ym = xm + sm, bb = ym - xm, err = (xm - (ym - bb)) + (sm - bb);
    f[0] = xm;
    f[1] = sc;
    f[2] = ym;
    f[3] = cc[0] + err;
    f[4] = cc[1] + sc;
    f[5] = cc[2];
    f[6] = cc[3];
    const int c = cut_cell[g];
    const long long n = cell_ptr[c + 1] - cell_ptr[c];
    if (right[g] != n) disc_soa[g] = soa0[cell_ptr[c] + right[g]];
}
__global__ __launch_bounds__(kBlock) void k_residual(const double* __restrict__ soa0, const double* __restrict__ sdoa,
                                                     const int* __restrict__ cut_seg, const int* __restrict__ cut_flags,
                                                     const double* __restrict__ cut_par, const double* __restrict__ cut_c,
                                                     int m, double* __restrict__ residual) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= m) return;
    const int g = cut_seg[p];
    double r = NAN;
    if (g >= 0 && cut_flags[g] == THR_BSYNC_CUT_FITTED) {
        const double* par = cut_par + 3 * size_t(g);
        const double* c = cut_c + 4 * size_t(g);
        const double u = (soa0[p] - par[0]) / par[1], w = sdoa[p] - par[2];
        r = w - (((c[3] * u + c[2]) * u + c[1]) * u + c[0]);
    }
    residual[p] = r;
}

// ------------------------------------------------------------------ beacon sync: the cell summary
struct LoadSum1 {  // sums: residual, fitted rows, the cuts' snr (at each fitted cut's first row), fitted cuts; max |r|
    const double *residual, *cut_snr;
    const int *cut_seg, *cut_flags, *pos_cell;
    const long long *left, *cell_ptr;
    __device__ void operator()(int p, double (&v)[5]) const {
        v[4] = -INFINITY;
        const int g = cut_seg[p];
        if (g < 0 || cut_flags[g] != THR_BSYNC_CUT_FITTED) return;
        const double r = residual[p];
        v[0] = r;
        v[1] = 1.0;
        if (p - cell_ptr[pos_cell[p]] == left[g]) {
            v[2] = cut_snr[g];
            v[3] = 1.0;
        }
        v[4] = fabs(r);
    }
};
struct LoadSum2 {  // (r - mean)^2 over the rows of fitted cuts; cs: the five sums of LoadSum1 per cell
    const double *residual, *cs;
    const int *cut_seg, *cut_flags, *pos_cell;
    __device__ void operator()(int p, double (&v)[1]) const {
        const int g = cut_seg[p];
        if (g < 0 || cut_flags[g] != THR_BSYNC_CUT_FITTED) return;
        const double* c = cs + 5 * size_t(pos_cell[p]);
        const double d = residual[p] - c[0] / c[1];
        v[0] = d * d;
    }
};
// cell_stats[c] = {mean dsdoa (written before), std, max |r|, mean snr}; counts = {rows, discontinuities, fitted cuts}
__global__ __launch_bounds__(kBlock) void k_cell_fin(const double* __restrict__ cs, const double* __restrict__ cs2,
                                                     const long long* __restrict__ cell_ptr, const long long* __restrict__ disc_ptr,
                                                     int nc, double* __restrict__ cell_stats, long long* __restrict__ cell_counts,
                                                     int* __restrict__ cell_flags) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= nc) return;
    const double* v = cs + 5 * size_t(c);
    const long long fitted = (long long)v[3];
    cell_counts[3 * size_t(c)] = cell_ptr[c + 1] - cell_ptr[c];
    cell_counts[3 * size_t(c) + 1] = disc_ptr[c + 1] - disc_ptr[c];
    cell_counts[3 * size_t(c) + 2] = fitted;
    cell_flags[c] = fitted ? 0 : THR_BSYNC_CELL_NO_FIT;
    cell_stats[4 * size_t(c) + 1] = fitted ? sqrt(cs2[c] / v[1]) : NAN;
    cell_stats[4 * size_t(c) + 2] = fitted ? v[4] : NAN;
    cell_stats[4 * size_t(c) + 3] = fitted ? v[2] / v[3] : NAN;
}

// ------------------------------------------------------------------ tdoa statistics
struct Tdoa {
    const int *rx0, *rx1, *tx;
    const double *ts, *tdoa;
    const long long *d0, *d1;
    int has_ts, has_det;
    double ts_lo, ts_hi;
    long long det_lo, det_hi;
};
__global__ __launch_bounds__(kBlock) void k_td_keep(Tdoa d, int n, unsigned* __restrict__ keep) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    bool k = true;
    if (d.has_ts) k = d.ts[i] >= d.ts_lo && d.ts[i] <= d.ts_hi;
    if (d.has_det) k = k && d.d0[i] >= d.det_lo && d.d0[i] <= d.det_hi && d.d1[i] >= d.det_lo && d.d1[i] <= d.det_hi;
    keep[i] = k ? 1u : 0u;
}
__global__ __launch_bounds__(kBlock) void k_td_keys(Tdoa d, int n, const unsigned* __restrict__ keep,
                                                    const unsigned* __restrict__ incl, unsigned long long* __restrict__ key_hi,
                                                    unsigned* __restrict__ key_lo, unsigned* __restrict__ sel) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const unsigned j = incl[i] - 1;
    sel[j] = unsigned(i);
    key_hi[j] = ((unsigned long long)key_i32(d.rx0[i]) << 32) | key_i32(d.rx1[i]);
    key_lo[j] = key_i32(d.tx[i]);
}
__global__ __launch_bounds__(kBlock) void k_td_rows(Tdoa d, const unsigned* __restrict__ perm, const unsigned* __restrict__ sel,
                                                    int m, long long* __restrict__ order, double* __restrict__ x) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= m) return;
    const unsigned row = sel[perm[p]];
    order[p] = row;
    x[p] = d.tdoa[row] * kLight;
}
struct LoadTd1 {  // sums of x and x^2, min, max
    const double* x;
    __device__ void operator()(int p, double (&v)[4]) const {
        const double a = x[p];
        v[0] = a;
        v[1] = a * a;
        v[2] = a;
        v[3] = a;
    }
};
struct LoadTd2 {  // (x - mean)^2; cv: LoadTd1's four values per cell, the mean is its sum over the cell's count
    const double *x, *cv;
    const int* pos_cell;
    const long long* cell_ptr;
    __device__ void operator()(int p, double (&v)[1]) const {
        const int c = pos_cell[p];
        const double d = x[p] - cv[4 * size_t(c)] / double(cell_ptr[c + 1] - cell_ptr[c]);
        v[0] = d * d;
    }
};
// stats[c] = {mean, std, rms, min, max}
__global__ __launch_bounds__(kBlock) void k_td_fin(const double* __restrict__ cv, const double* __restrict__ cv2,
                                                   const long long* __restrict__ cell_ptr, int nc, double* __restrict__ stats) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= nc) return;
    const double n = double(cell_ptr[c + 1] - cell_ptr[c]);
    double* s = stats + 5 * size_t(c);
    s[0] = cv[4 * size_t(c)] / n;
    s[1] = sqrt(cv2[c] / n);
    s[2] = sqrt(cv[4 * size_t(c) + 1] / n);
    s[3] = cv[4 * size_t(c) + 2];
    s[4] = cv[4 * size_t(c) + 3];
}
// over the kept rows (LoadKept1<true>: count, sums of x and x^2, min, max): stats[c] as k_td_fin, and the count
__global__ __launch_bounds__(kBlock) void k_rb_fin(const double* __restrict__ cv, const double* __restrict__ cv2, int nc,
                                                   double* __restrict__ stats, long long* __restrict__ count) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= nc) return;
    const double* v = cv + 5 * size_t(c);
    const double n = v[0];
    double* s = stats + 5 * size_t(c);
    count[c] = (long long)n;
    s[0] = v[1] / n;
    s[1] = sqrt(cv2[c] / n);
    s[2] = sqrt(v[2] / n);
    s[3] = v[3];
    s[4] = v[4];
}

// last call of this thread: copies in, rows and cells, reductions, fits (or the robust part), copies out
thread_local double g_bsync_ms[5] = {0, 0, 0, 0, 0};
thread_local double g_tdstats_ms[5] = {0, 0, 0, 0, 0};

}  // namespace

struct thr_bsync : thr::seg::Result {};
struct thr_tdstats : thr::seg::Result {};

extern "C" int thr_beaconsync(int device_id, size_t n_det, const int32_t* rxid, const int32_t* txid, const double* soa,
                              const double* energy, const double* noise, const int64_t* idx, size_t n_matches,
                              const int64_t* match_ptr, const int64_t* match_idx, int deg, const int64_t* id_range,
                              const int32_t* beacons, size_t n_beacons, const int32_t* receivers, size_t n_receivers,
                              thr_bsync** result_out, thr_bsync_counts* counts_out) try {
    if (result_out) *result_out = nullptr;
    if (counts_out) std::memset(counts_out, 0, sizeof(*counts_out));
    for (double& t : g_bsync_ms) t = 0;
    if (!result_out || !counts_out) return thr::fail_msg(THR_ERR_ARG, "thr_beaconsync: null argument");
    if (deg < 1 || deg > 3) return thr::fail_msg(THR_ERR_ARG, "thr_beaconsync: deg must be 1, 2 or 3, not %d", deg);
    if (n_det && (!rxid || !txid || !soa || !energy || !noise || !idx))
        return thr::fail_msg(THR_ERR_ARG, "thr_beaconsync: null argument");
    if (!match_ptr || (n_matches && match_ptr[n_matches] && !match_idx))
        return thr::fail_msg(THR_ERR_ARG, "thr_beaconsync: null argument");
    if (n_det > (size_t(1) << 28) || n_matches > (size_t(1) << 28) || n_beacons > (size_t(1) << 20) ||
        n_receivers > (size_t(1) << 20))
        return thr::fail_msg(THR_ERR_ARG, "thr_beaconsync: too many detections, matches or list entries");
    if (id_range && id_range[0] > id_range[1])
        return thr::fail_msg(THR_ERR_ARG, "thr_beaconsync: the id range %lld-%lld is empty", (long long)id_range[0],
                             (long long)id_range[1]);
    uint64_t n_pairs = 0;
    THR_TRY(check_matches("thr_beaconsync", n_det, rxid, n_matches, match_ptr, match_idx, &n_pairs));
    const size_t n_entries = size_t(match_ptr[n_matches]);

    THR_TRY(pick_device(device_id));
    thr_bsync* R = new thr_bsync;
    ResultGuard guard{R};
    R->device = device_id;
    R->n_out = THR_BSYNC_N_OUTPUTS;
    hipStream_t s = nullptr;
    Event ev[5];
    for (Event& e : ev) THR_HIP_TRY(e.create());
    for (Event& e : R->ev) THR_HIP_TRY(e.create());

    // ---- copies in
    DevBuf d_rx, d_tx, d_soa, d_en, d_no, d_id, d_mptr, d_midx, d_bl, d_rl;
    Dets D;
    THR_HIP_TRY(d_rx.alloc(n_det * 4));
    THR_HIP_TRY(d_tx.alloc(n_det * 4));
    THR_HIP_TRY(d_soa.alloc(n_det * 8));
    THR_HIP_TRY(d_en.alloc(n_det * 8));
    THR_HIP_TRY(d_no.alloc(n_det * 8));
    THR_HIP_TRY(d_id.alloc(n_det * 8));
    THR_HIP_TRY(d_mptr.alloc((n_matches + 1) * 8));
    THR_HIP_TRY(d_midx.alloc(n_entries * 8));
    THR_HIP_TRY(hipEventRecord(ev[0].e, s));
    THR_HIP_TRY(hipMemcpy(d_rx.p, rxid, n_det * 4, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipMemcpy(d_tx.p, txid, n_det * 4, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipMemcpy(d_soa.p, soa, n_det * 8, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipMemcpy(d_en.p, energy, n_det * 8, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipMemcpy(d_no.p, noise, n_det * 8, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipMemcpy(d_id.p, idx, n_det * 8, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipMemcpy(d_mptr.p, match_ptr, (n_matches + 1) * 8, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipMemcpy(d_midx.p, match_idx, n_entries * 8, hipMemcpyHostToDevice));
    THR_TRY(upload_list(beacons, n_beacons, d_bl, D.n_beacons));
    THR_TRY(upload_list(receivers, n_receivers, d_rl, D.n_receivers));
    THR_HIP_TRY(hipEventRecord(ev[1].e, s));
    D.rx = d_rx.as<int>();
    D.tx = d_tx.as<int>();
    D.soa = d_soa.as<double>();
    D.en = d_en.as<double>();
    D.no = d_no.as<double>();
    D.id = d_id.as<long long>();
    D.mptr = d_mptr.as<long long>();
    D.midx = d_midx.as<long long>();
    D.beacons = d_bl.as<int>();
    D.receivers = d_rl.as<int>();
    D.has_range = id_range ? 1 : 0;
    D.lo = id_range ? id_range[0] : 0;
    D.hi = id_range ? id_range[1] : 0;

    // ---- 1. rows and cells
    Scratch w;
    PairRows rows;
    DevBuf* O = R->out;
    THR_TRY(pair_rows(BeaconPairs{D}, int(n_matches), w, rows, O[THR_BSYNC_CELL_PTR], O[THR_BSYNC_CELL_KEY], s));
    if (rows.m == 0) return thr::fail_msg(THR_ERR_ARG, "thr_beaconsync: the selection is empty");
    const int m = rows.m;
    const Cells& cells = rows.cells;
    const int nc = cells.nc;
    const int* pos_cell = cells.pos_cell.as<int>();
    const long long* cell_ptr = O[THR_BSYNC_CELL_PTR].as<long long>();
    DevBuf d_soa0, d_snr2;
    THR_HIP_TRY(O[THR_BSYNC_ROW_DET].alloc(size_t(m) * 16));
    THR_HIP_TRY(O[THR_BSYNC_ROW_MATCH].alloc(size_t(m) * 8));
    THR_HIP_TRY(O[THR_BSYNC_SDOA].alloc(size_t(m) * 8));
    THR_HIP_TRY(d_soa0.alloc(size_t(m) * 8));
    THR_HIP_TRY(d_snr2.alloc(size_t(m) * 8));
    const double *sdoa = O[THR_BSYNC_SDOA].as<double>(), *soa0 = d_soa0.as<double>(), *snr2 = d_snr2.as<double>();
    THR_TRY(launch(k_rows, m, s, D, cells.perm.as<unsigned>(), rows.det.as<long long>(), rows.match.as<long long>(), m,
                   O[THR_BSYNC_ROW_DET].as<long long>(), O[THR_BSYNC_ROW_MATCH].as<long long>(), O[THR_BSYNC_SDOA].as<double>(),
                   d_soa0.as<double>(), d_snr2.as<double>()));
    THR_HIP_TRY(hipEventRecord(ev[2].e, s));

    // ---- 2. discontinuities and cuts
    Layout LC;
    THR_TRY(build_layout(pos_cell, m, nc, w, LC, s));
    DevBuf d_slab, d_cv, d_cv2, d_flag, d_cutseg;
    THR_HIP_TRY(d_slab.alloc(size_t(LC.nf) * 5 * 8));
    THR_HIP_TRY(d_cv.alloc(size_t(nc) * 5 * 8));
    THR_HIP_TRY(d_cv2.alloc(size_t(nc) * 8));
    THR_HIP_TRY(d_flag.alloc(size_t(m) * 4));
    THR_HIP_TRY(d_cutseg.alloc(size_t(m) * 4));
    THR_HIP_TRY(O[THR_BSYNC_CELL_STATS].alloc(size_t(nc) * 4 * 8));
    THR_HIP_TRY(O[THR_BSYNC_DISC_PTR].alloc((size_t(nc) + 1) * 8));
    THR_HIP_TRY(O[THR_BSYNC_CUT_PTR].alloc((size_t(nc) + 1) * 8));
    THR_TRY((reduce<1, 1, 0>(LoadDsdoa{sdoa, pos_cell, m}, LC, d_slab.as<double>(), d_cv.as<double>(), s)));
    THR_TRY(launch(k_disc_flags, m, s, sdoa, pos_cell, cell_ptr, d_cv.as<double>(), m, d_flag.as<unsigned>(),
                   O[THR_BSYNC_CELL_STATS].as<double>()));
    unsigned n_disc = 0;
    THR_TRY(scan(d_flag.as<unsigned>(), w.incl.as<unsigned>(), m, w, s, &n_disc));
    const int n_cuts = int(n_disc) + nc;
    THR_HIP_TRY(O[THR_BSYNC_DISC_IDX].alloc(size_t(n_disc) * 8));
    THR_TRY(launch(k_disc_layout, m, s, d_flag.as<unsigned>(), w.incl.as<unsigned>(), pos_cell, cell_ptr, m, nc,
                   O[THR_BSYNC_DISC_PTR].as<long long>(), O[THR_BSYNC_DISC_IDX].as<long long>(),
                   O[THR_BSYNC_CUT_PTR].as<long long>(), d_cutseg.as<int>()));
    const int* cut_seg = d_cutseg.as<int>();
    DevBuf d_cutcell, d_cutv, d_cutpar, d_cutc;
    THR_HIP_TRY(d_cutcell.alloc(size_t(n_cuts) * 4));
    THR_HIP_TRY(d_cutv.alloc(size_t(n_cuts) * 10 * 8));
    THR_HIP_TRY(d_cutpar.alloc(size_t(n_cuts) * 3 * 8));
    THR_HIP_TRY(d_cutc.alloc(size_t(n_cuts) * 4 * 8));
    THR_HIP_TRY(O[THR_BSYNC_CUT_LEFT].alloc(size_t(n_cuts) * 8));
    THR_HIP_TRY(O[THR_BSYNC_CUT_RIGHT].alloc(size_t(n_cuts) * 8));
    THR_HIP_TRY(O[THR_BSYNC_CUT_FLAGS].alloc(size_t(n_cuts) * 4));
    THR_HIP_TRY(O[THR_BSYNC_CUT_FIT].alloc(size_t(n_cuts) * 7 * 8));
    THR_HIP_TRY(O[THR_BSYNC_CUT_SNR].alloc(size_t(n_cuts) * 8));
    THR_HIP_TRY(O[THR_BSYNC_CUT_DISC_SOA].alloc(size_t(n_cuts) * 8));
    const long long *left = O[THR_BSYNC_CUT_LEFT].as<long long>(), *right = O[THR_BSYNC_CUT_RIGHT].as<long long>();
    const int* cut_flags = O[THR_BSYNC_CUT_FLAGS].as<int>();
    THR_TRY(launch(k_cuts, n_cuts, s, O[THR_BSYNC_CUT_PTR].as<long long>(), O[THR_BSYNC_DISC_PTR].as<long long>(),
                   O[THR_BSYNC_DISC_IDX].as<long long>(), cell_ptr, nc, n_cuts, d_cutcell.as<int>(),
                   O[THR_BSYNC_CUT_LEFT].as<long long>(), O[THR_BSYNC_CUT_RIGHT].as<long long>()));
    THR_HIP_TRY(hipEventRecord(ev[3].e, s));

    // ---- 3. fits and residuals, 4. the summary
    Layout LU;
    THR_TRY(build_layout(cut_seg, m, n_cuts, w, LU, s));
    DevBuf d_slab2;
    THR_HIP_TRY(d_slab2.alloc(size_t(LU.nf) * 10 * 8));
    THR_HIP_TRY(O[THR_BSYNC_RESIDUAL].alloc(size_t(m) * 8));
    THR_HIP_TRY(O[THR_BSYNC_CELL_COUNTS].alloc(size_t(nc) * 3 * 8));
    THR_HIP_TRY(O[THR_BSYNC_CELL_FLAGS].alloc(size_t(nc) * 4));
    THR_TRY((reduce<5, 3, 1>(LoadCut1{soa0, sdoa, snr2}, LU, d_slab2.as<double>(), d_cutv.as<double>(), s)));
    THR_TRY(launch(k_cut_mid, n_cuts, s, d_cutv.as<double>(), left, right, n_cuts, d_cutpar.as<double>(),
                   O[THR_BSYNC_CUT_SNR].as<double>(), O[THR_BSYNC_CUT_FLAGS].as<int>()));
    const double* cut_par = d_cutpar.as<double>();
    THR_TRY((reduce<10, 10, 0>(LoadCut2{soa0, sdoa, cut_par, cut_seg, cut_flags}, LU, d_slab2.as<double>(), d_cutv.as<double>(), s)));
    THR_TRY(launch(k_cut_fit, n_cuts, s, d_cutv.as<double>(), cut_par, left, right, d_cutcell.as<int>(), cell_ptr, soa0, deg, n_cuts,
                   O[THR_BSYNC_CUT_FLAGS].as<int>(), d_cutc.as<double>(), O[THR_BSYNC_CUT_FIT].as<double>(),
                   O[THR_BSYNC_CUT_SNR].as<double>(), O[THR_BSYNC_CUT_DISC_SOA].as<double>()));
    THR_TRY(launch(k_residual, m, s, soa0, sdoa, cut_seg, cut_flags, cut_par, d_cutc.as<double>(), m,
                   O[THR_BSYNC_RESIDUAL].as<double>()));
    const double *residual = O[THR_BSYNC_RESIDUAL].as<double>(), *cv = d_cv.as<double>();
    THR_TRY((reduce<5, 4, 0>(LoadSum1{residual, O[THR_BSYNC_CUT_SNR].as<double>(), cut_seg, cut_flags, pos_cell, left, cell_ptr}, LC,
                             d_slab.as<double>(), d_cv.as<double>(), s)));
    THR_TRY((reduce<1, 1, 0>(LoadSum2{residual, cv, cut_seg, cut_flags, pos_cell}, LC, d_slab.as<double>(), d_cv2.as<double>(), s)));
    THR_TRY(launch(k_cell_fin, nc, s, cv, d_cv2.as<double>(), cell_ptr, O[THR_BSYNC_DISC_PTR].as<long long>(), nc,
                   O[THR_BSYNC_CELL_STATS].as<double>(), O[THR_BSYNC_CELL_COUNTS].as<long long>(),
                   O[THR_BSYNC_CELL_FLAGS].as<int>()));
    THR_HIP_TRY(hipEventRecord(ev[4].e, s));
    THR_TRY(record_times(ev, g_bsync_ms));  // synchronises: the temporaries go out of scope

    size_t* B = R->bytes;
    B[THR_BSYNC_CELL_KEY] = size_t(nc) * 12;
    B[THR_BSYNC_CELL_PTR] = B[THR_BSYNC_DISC_PTR] = B[THR_BSYNC_CUT_PTR] = (size_t(nc) + 1) * 8;
    B[THR_BSYNC_ROW_DET] = size_t(m) * 16;
    B[THR_BSYNC_ROW_MATCH] = B[THR_BSYNC_SDOA] = B[THR_BSYNC_RESIDUAL] = size_t(m) * 8;
    B[THR_BSYNC_DISC_IDX] = size_t(n_disc) * 8;
    B[THR_BSYNC_CUT_LEFT] = B[THR_BSYNC_CUT_RIGHT] = B[THR_BSYNC_CUT_SNR] = B[THR_BSYNC_CUT_DISC_SOA] = size_t(n_cuts) * 8;
    B[THR_BSYNC_CUT_FLAGS] = size_t(n_cuts) * 4;
    B[THR_BSYNC_CUT_FIT] = size_t(n_cuts) * 7 * 8;
    B[THR_BSYNC_CELL_COUNTS] = size_t(nc) * 3 * 8;
    B[THR_BSYNC_CELL_STATS] = size_t(nc) * 4 * 8;
    B[THR_BSYNC_CELL_FLAGS] = size_t(nc) * 4;
    counts_out->rows = size_t(m);
    counts_out->cells = size_t(nc);
    counts_out->discontinuities = size_t(n_disc);
    counts_out->cuts = size_t(n_cuts);
    *result_out = R;
    guard.r = nullptr;
    return THR_OK;
} catch (const std::bad_alloc&) {
    return thr::fail_msg(THR_ERR_DEVICE, "thr_beaconsync: out of host memory");
} catch (...) {
    return thr::on_exception("thr_beaconsync");
}

extern "C" int thr_bsync_fetch(thr_bsync* R, int which, void* dst, size_t dst_bytes) try {
    return fetch("thr_bsync_fetch", R, which, dst, dst_bytes, &g_bsync_ms[4]);
} catch (...) {
    return thr::on_exception("thr_bsync_fetch");
}

extern "C" void thr_bsync_free(thr_bsync* R) { free_result(R); }

extern "C" int thr_tdoastats(int device_id, size_t n, const int32_t* rx0, const int32_t* rx1, const int32_t* tx,
                             const double* timestamp, const int64_t* det0_idx, const int64_t* det1_idx, const double* tdoa,
                             const double* ts_range, const int64_t* det_range, int robust, thr_tdstats** result_out,
                             thr_tdstats_counts* counts_out) try {
    if (result_out) *result_out = nullptr;
    if (counts_out) std::memset(counts_out, 0, sizeof(*counts_out));
    for (double& t : g_tdstats_ms) t = 0;
    if (!result_out || !counts_out) return thr::fail_msg(THR_ERR_ARG, "thr_tdoastats: null argument");
    if (n && (!rx0 || !rx1 || !tx || !timestamp || !det0_idx || !det1_idx || !tdoa))
        return thr::fail_msg(THR_ERR_ARG, "thr_tdoastats: null argument");
    if (n == 0) return thr::fail_msg(THR_ERR_ARG, "thr_tdoastats: the selection is empty");
    if (n > size_t(1) << 28) return thr::fail_msg(THR_ERR_ARG, "thr_tdoastats: too many rows");
    if (ts_range && !(ts_range[0] <= ts_range[1])) return thr::fail_msg(THR_ERR_ARG, "thr_tdoastats: the timestamp range is empty");
    if (det_range && det_range[0] > det_range[1]) return thr::fail_msg(THR_ERR_ARG, "thr_tdoastats: the detection id range is empty");

    THR_TRY(pick_device(device_id));
    thr_tdstats* R = new thr_tdstats;
    ResultGuard guard{R};
    R->device = device_id;
    R->n_out = THR_TDSTATS_N_OUTPUTS;
    hipStream_t s = nullptr;
    Event ev[5];
    for (Event& e : ev) THR_HIP_TRY(e.create());
    for (Event& e : R->ev) THR_HIP_TRY(e.create());

    // ---- copies in
    DevBuf d_i32[3], d_f64[2], d_i64[2];
    const int32_t* h_i32[3] = {rx0, rx1, tx};
    const double* h_f64[2] = {timestamp, tdoa};
    const int64_t* h_i64[2] = {det0_idx, det1_idx};
    for (DevBuf& b : d_i32) THR_HIP_TRY(b.alloc(n * 4));
    for (DevBuf& b : d_f64) THR_HIP_TRY(b.alloc(n * 8));
    for (DevBuf& b : d_i64) THR_HIP_TRY(b.alloc(n * 8));
    THR_HIP_TRY(hipEventRecord(ev[0].e, s));
    for (int k = 0; k < 3; ++k) THR_HIP_TRY(hipMemcpy(d_i32[k].p, h_i32[k], n * 4, hipMemcpyHostToDevice));
    for (int k = 0; k < 2; ++k) THR_HIP_TRY(hipMemcpy(d_f64[k].p, h_f64[k], n * 8, hipMemcpyHostToDevice));
    for (int k = 0; k < 2; ++k) THR_HIP_TRY(hipMemcpy(d_i64[k].p, h_i64[k], n * 8, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipEventRecord(ev[1].e, s));
    Tdoa D;
    D.rx0 = d_i32[0].as<int>();
    D.rx1 = d_i32[1].as<int>();
    D.tx = d_i32[2].as<int>();
    D.ts = d_f64[0].as<double>();
    D.tdoa = d_f64[1].as<double>();
    D.d0 = d_i64[0].as<long long>();
    D.d1 = d_i64[1].as<long long>();
    D.has_ts = ts_range ? 1 : 0;
    D.has_det = det_range ? 1 : 0;
    D.ts_lo = ts_range ? ts_range[0] : 0.0;
    D.ts_hi = ts_range ? ts_range[1] : 0.0;
    D.det_lo = det_range ? det_range[0] : 0;
    D.det_hi = det_range ? det_range[1] : 0;

    // ---- 1. the selection, rows and cells
    const int nn = int(n);
    Scratch w;
    DevBuf d_keep;
    THR_HIP_TRY(d_keep.alloc(n * 4));
    THR_HIP_TRY(w.head.alloc(n * 4));
    THR_HIP_TRY(w.incl.alloc(n * 4));
    THR_TRY(launch(k_td_keep, n, s, D, nn, d_keep.as<unsigned>()));
    unsigned n_sel = 0;
    THR_TRY(scan(d_keep.as<unsigned>(), w.incl.as<unsigned>(), nn, w, s, &n_sel));
    if (n_sel == 0) return thr::fail_msg(THR_ERR_ARG, "thr_tdoastats: the selection is empty");
    const int m = int(n_sel);
    DevBuf d_khi, d_klo, d_sel, d_x;
    THR_HIP_TRY(d_khi.alloc(size_t(m) * 8));
    THR_HIP_TRY(d_klo.alloc(size_t(m) * 4));
    THR_HIP_TRY(d_sel.alloc(size_t(m) * 4));
    THR_HIP_TRY(d_x.alloc(size_t(m) * 8));
    THR_TRY(launch(k_td_keys, n, s, D, nn, d_keep.as<unsigned>(), w.incl.as<unsigned>(), d_khi.as<unsigned long long>(),
                   d_klo.as<unsigned>(), d_sel.as<unsigned>()));
    DevBuf* O = R->out;
    Cells cells;
    THR_TRY(sort_cells(d_khi, d_klo, m, w, cells, O[THR_TDSTATS_CELL_PTR], O[THR_TDSTATS_CELL_KEY], s));
    const int nc = cells.nc;
    const int* pos_cell = cells.pos_cell.as<int>();
    const long long* cell_ptr = O[THR_TDSTATS_CELL_PTR].as<long long>();
    const double* x = d_x.as<double>();
    THR_HIP_TRY(O[THR_TDSTATS_ORDER].alloc(size_t(m) * 8));
    THR_HIP_TRY(O[THR_TDSTATS_STATS].alloc(size_t(nc) * 5 * 8));
    THR_TRY(launch(k_td_rows, m, s, D, cells.perm.as<unsigned>(), d_sel.as<unsigned>(), m, O[THR_TDSTATS_ORDER].as<long long>(),
                   d_x.as<double>()));
    THR_HIP_TRY(hipEventRecord(ev[2].e, s));

    // ---- 2. the statistics of every row
    Layout LC;
    THR_TRY(build_layout(pos_cell, m, nc, w, LC, s));
    DevBuf d_slab, d_cv, d_cv2;
    THR_HIP_TRY(d_slab.alloc(size_t(LC.nf) * 5 * 8));
    THR_HIP_TRY(d_cv.alloc(size_t(nc) * 5 * 8));
    THR_HIP_TRY(d_cv2.alloc(size_t(nc) * 8));
    const double* cv = d_cv.as<double>();
    THR_TRY((reduce<4, 2, 1>(LoadTd1{x}, LC, d_slab.as<double>(), d_cv.as<double>(), s)));
    THR_TRY((reduce<1, 1, 0>(LoadTd2{x, cv, pos_cell, cell_ptr}, LC, d_slab.as<double>(), d_cv2.as<double>(), s)));
    THR_TRY(launch(k_td_fin, nc, s, cv, d_cv2.as<double>(), cell_ptr, nc, O[THR_TDSTATS_STATS].as<double>()));
    THR_HIP_TRY(hipEventRecord(ev[3].e, s));

    // ---- 3. the robust part
    if (robust) {
        Work W{w};
        THR_HIP_TRY(W.dev.alloc(size_t(m) * 8));
        THR_HIP_TRY(O[THR_TDSTATS_MEDIAN].alloc(size_t(nc) * 2 * 8));
        THR_HIP_TRY(O[THR_TDSTATS_MASK].alloc(size_t(m)));
        THR_HIP_TRY(O[THR_TDSTATS_ROBUST_STATS].alloc(size_t(nc) * 5 * 8));
        THR_HIP_TRY(O[THR_TDSTATS_ROBUST_COUNT].alloc(size_t(nc) * 8));
        Series SR;
        SR.n = m;
        SR.nc = nc;
        SR.pos_cell = pos_cell;
        SR.ptr = cell_ptr;
        const double* probe = O[THR_TDSTATS_STATS].as<double>() + 4;  // the cell's max: NaN when it holds one
        const unsigned char* mask = O[THR_TDSTATS_MASK].as<unsigned char>();
        THR_TRY(outlier_mask(x, SR, probe, 5, 3.5, W, O[THR_TDSTATS_MEDIAN].as<double>(), 2, O[THR_TDSTATS_MASK].as<unsigned char>(), s));
        THR_TRY((reduce<5, 3, 1>(LoadKept1<true>{x, mask}, LC, d_slab.as<double>(), d_cv.as<double>(), s)));
        THR_TRY((reduce<1, 1, 0>(LoadKept2<true>{x, cv, mask, pos_cell}, LC, d_slab.as<double>(), d_cv2.as<double>(), s)));
        THR_TRY(launch(k_rb_fin, nc, s, cv, d_cv2.as<double>(), nc, O[THR_TDSTATS_ROBUST_STATS].as<double>(),
                       O[THR_TDSTATS_ROBUST_COUNT].as<long long>()));
        THR_HIP_TRY(hipStreamSynchronize(s));  // W's buffers go out of scope here
    }
    THR_HIP_TRY(hipEventRecord(ev[4].e, s));
    THR_TRY(record_times(ev, g_tdstats_ms));

    size_t* B = R->bytes;
    B[THR_TDSTATS_CELL_KEY] = size_t(nc) * 12;
    B[THR_TDSTATS_CELL_PTR] = (size_t(nc) + 1) * 8;
    B[THR_TDSTATS_ORDER] = size_t(m) * 8;
    B[THR_TDSTATS_STATS] = size_t(nc) * 5 * 8;
    if (robust) {
        B[THR_TDSTATS_ROBUST_STATS] = size_t(nc) * 5 * 8;
        B[THR_TDSTATS_ROBUST_COUNT] = size_t(nc) * 8;
        B[THR_TDSTATS_MASK] = size_t(m);
        B[THR_TDSTATS_MEDIAN] = size_t(nc) * 2 * 8;
    }
    counts_out->rows = size_t(m);
    counts_out->cells = size_t(nc);
    counts_out->robust = robust ? 1 : 0;
    *result_out = R;
    guard.r = nullptr;
    return THR_OK;
} catch (const std::bad_alloc&) {
    return thr::fail_msg(THR_ERR_DEVICE, "thr_tdoastats: out of host memory");
} catch (...) {
    return thr::on_exception("thr_tdoastats");
}

extern "C" int thr_tdstats_fetch(thr_tdstats* R, int which, void* dst, size_t dst_bytes) try {
    return fetch("thr_tdstats_fetch", R, which, dst, dst_bytes, &g_tdstats_ms[4]);
} catch (...) {
    return thr::on_exception("thr_tdstats_fetch");
}

extern "C" void thr_tdstats_free(thr_tdstats* R) { free_result(R); }

extern "C" int thr_debug_beaconsync_times(double* ms_out) try {
    return copy_times("thr_debug_beaconsync_times", g_bsync_ms, ms_out);
} catch (...) {
    return thr::on_exception("thr_debug_beaconsync_times");
}

extern "C" int thr_debug_tdoastats_times(double* ms_out) try {
    return copy_times("thr_debug_tdoastats_times", g_tdstats_ms, ms_out);
} catch (...) {
    return thr::on_exception("thr_debug_tdoastats_times");
}

extern "C" int thr_debug_beaconsync_geometry(int* tile_len, int* workgroup) try {
    return geometry("thr_debug_beaconsync_geometry", tile_len, workgroup);
} catch (...) {
    return thr::on_exception("thr_debug_beaconsync_geometry");
}

extern "C" int thr_debug_tdoastats_geometry(int* tile_len, int* workgroup) try {
    return geometry("thr_debug_tdoastats_geometry", tile_len, workgroup);
} catch (...) {
    return thr::on_exception("thr_debug_tdoastats_geometry");
}
