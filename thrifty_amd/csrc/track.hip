// Tracks on the device (thr_track): per transmitter a constant-velocity Kalman filter over the positions in time
// order, a gate on the innovations, and a Rauch-Tung-Striebel smoother -- the last open item of the reference's
// pos_est.py ("apply Kalman filter or something to average out the position estimates").  include/thrifty_hip.h
// states the definition; DESIGN.md 3.18 says why the recursions run as scans.
//
// Rows are sorted by (tx, timestamp) with seg_cells.hpp's sort_cells; a track is a segment, cut into fragments by
// build_layout.  Per axis a row is an element of an associative operator (track_scan.hpp), and a recursion is:
//   1  k_filter<false> / k_smooth<false>   every tile scans its elements; a fragment's last (first) position stores
//                                          the fragment's combination to a slab;
//   2  k_filter_carry / k_smooth_carry     one thread per (track, axis) walks the track's fragments in tile order
//                                          and leaves each fragment the state that enters it.  Every prefix from a
//                                          track's start has A = eta = J = 0 (every suffix to its end E = 0), so
//                                          that state is five doubles: the mean and the covariance;
//   3  k_filter<true> / k_smooth<true>     the tiles scan again, the carry combined into the fragment's first
//                                          (last) element; every position's result is its state.
// The elements are rebuilt from the columns in pass 3, not stored in pass 1: 28 doubles per row would be written and
// read back to save some hundred flops.  k_gate computes nis and the next mask from the state of the row before and
// counts the changed rows in an integer, which the host reads once per round.
// No floating-point atomic; the tree a row is combined in depends on its position in its tile and on nothing else.
// All launches go to the null stream; temporaries are freed by hipFree, which waits for it.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/thrifty_hip.h"
#include "post_stages.hpp"
#include "seg_cells.hpp"
#include "track_scan.hpp"

// a shuffled input must give the same bytes per row: no a * b + c may become an fma in this file (the build also
// passes -ffp-contract=off for it, thrifty_amd/build.py)
#pragma clang fp contract(off)

namespace {

using thr::DevBuf;
using thr::Event;
using thr::seg::kBlock;
using thr::seg::kTile;
using thr::seg::launch;
using thr::seg::launch_grid;
using thr::seg::TilePos;
using thr::seg::tile_pos;
using thr::trk::FilterOp;
using thr::trk::nc_scan;
using thr::trk::SmoothOp;

constexpr int kState = 5;  // m0 m1 P00 P01 P11 of one axis
constexpr int kStats = 9;  // slots of the statistics reduction: 7 sums, 1 minimum, 1 maximum
static_assert(THR_TRACK_N_OUTPUTS <= thr::seg::kMaxOutputs, "the result handle holds every output");
static_assert(thr::trk::scan_lds<FilterOp>() * sizeof(double) <= 64 * 1024, "the two scan buffers fit the static LDS");

struct Rows {  // the m rows in (tx, timestamp) order
    const double *t, *z[2], *r[2];
    const unsigned char* valid;
    const int* track;      // per position
    const long long* ptr;  // per track, n_tracks + 1
    const int* start;      // per track: its first valid position, INT_MAX without one
    int m;
    __device__ bool tracked(int p) const { return p >= start[track[p]]; }
};
struct Frags {  // build_layout's
    const int *pos_frag, *frag_start, *seg_frag;
    int n_tiles;
};

// ---------------------------------------------------------------- sort keys and the rows in order
__device__ __forceinline__ unsigned long long key_f64(double v) {  // order-preserving; -0.0 and 0.0 are one key
    const unsigned long long b = (unsigned long long)__double_as_longlong(v + 0.0);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__global__ __launch_bounds__(kBlock) void k_keys(const int* __restrict__ tx, const double* __restrict__ ts, int m,
                                                 unsigned long long* __restrict__ hi, unsigned* __restrict__ lo) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    const unsigned long long k = key_f64(ts[j]);
    hi[j] = ((unsigned long long)thr::seg::key_i32(tx[j]) << 32) | (k >> 32);
    lo[j] = unsigned(k);
}
struct Cols {
    const int* tx;
    const double *t, *x, *y, *rx, *ry;
    const unsigned char* valid;  // null: all valid
};
struct Sorted {
    int* tx;
    double *t, *x, *y, *rx, *ry;
    unsigned char* valid;
};
__global__ __launch_bounds__(kBlock) void k_gather_rows(Cols in, const unsigned* __restrict__ perm, int m, Sorted out,
                                                        unsigned* __restrict__ head) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= m) return;
    const unsigned j = perm[p];
    out.tx[p] = in.tx[j];
    out.t[p] = in.t[j];
    out.x[p] = in.x[j];
    out.y[p] = in.y[j];
    out.rx[p] = in.rx[j];
    out.ry[p] = in.ry[j];
    out.valid[p] = in.valid ? (in.valid[j] ? 1 : 0) : 1;
    head[p] = (p == 0 || in.tx[perm[p - 1]] != in.tx[j]) ? 1u : 0u;
}
__global__ __launch_bounds__(kBlock) void k_track_layout(const int* __restrict__ tx, const unsigned* __restrict__ head,
                                                         const unsigned* __restrict__ incl, int m, int nt,
                                                         int* __restrict__ track, long long* __restrict__ ptr,
                                                         int* __restrict__ track_tx) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= m) return;
    const int c = int(incl[p]) - 1;
    track[p] = c;
    if (head[p]) {
        ptr[c] = p;
        track_tx[c] = tx[p];
    }
    if (p == m - 1) ptr[nt] = m;
}
struct LoadValid {  // the track's valid rows and the first of them
    const unsigned char* valid;
    __device__ void operator()(int p, double (&v)[2]) const {
        v[0] = valid[p] ? 1.0 : 0.0;
        v[1] = valid[p] ? double(p) : INFINITY;
    }
};
__global__ __launch_bounds__(kBlock) void k_starts(const double* __restrict__ red, int nt, int* __restrict__ start) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c < nt) start[c] = red[2 * size_t(c)] > 0.0 ? int(red[2 * size_t(c) + 1]) : INT_MAX;
}

// ---------------------------------------------------------------- the filter
// the element of position p on one axis (thrifty_hip.h and track_scan.hpp name the slots)
__device__ __forceinline__ void filter_element(const Rows& R, const unsigned char* mask, int axis, double q, double v0sq, int p,
                                               double (&e)[FilterOp::N]) {
#pragma unroll
    for (int k = 0; k < FilterOp::N; ++k) e[k] = 0.0;
    const int st = R.start[R.track[p]];
    if (p < st) {  // not tracked: the identity
        e[0] = e[3] = 1.0;
        return;
    }
    const double z = R.z[axis][p], r = R.r[axis][p];
    if (p == st) {
        e[4] = z;
        e[6] = r;
        e[8] = v0sq;
        return;
    }
    const double dt = R.t[p] - R.t[p - 1];
    const double q00 = q * (dt * dt * dt / 3.0), q01 = q * (dt * dt / 2.0), q11 = q * dt;
    if (!mask[p]) {  // a pure prediction
        e[0] = e[3] = 1.0;
        e[1] = dt;
        e[6] = q00;
        e[7] = q01;
        e[8] = q11;
        return;
    }
    const double s = q00 + r, k0 = q00 / s, k1 = q01 / s;
    e[0] = 1.0 - k0;
    e[1] = (1.0 - k0) * dt;
    e[2] = -k1;
    e[3] = 1.0 - k1 * dt;
    e[4] = k0 * z;
    e[5] = k1 * z;
    e[6] = (1.0 - k0) * q00;
    e[7] = (1.0 - k0) * q01;
    e[8] = q11 - k1 * q01;
    e[9] = z / s;
    e[10] = dt * z / s;
    e[11] = 1.0 / s;
    e[12] = dt / s;
    e[13] = dt * dt / s;
}

// FINAL = false: ftot[f][axis][14] = the combination of fragment f.  FINAL = true: fs[p][axis][5] = the state at p,
// carry[f][axis][5] being the state that enters fragment f (not read for a track's first fragment).
template <bool FINAL>
__global__ __launch_bounds__(kBlock) void k_filter(Rows R, const unsigned char* __restrict__ mask, double q, double v0sq, Frags L,
                                                   double* __restrict__ ftot, const double* __restrict__ carry,
                                                   double* __restrict__ fs) {
    constexpr int N = FilterOp::N;
    __shared__ double lds[thr::trk::scan_lds<FilterOp>()];
    const int t = threadIdx.x, axis = blockIdx.y;
    for (int tile = blockIdx.x; tile < L.n_tiles; tile += gridDim.x) {
        const TilePos x = tile_pos(tile, t, R.m, L.pos_frag, L.frag_start);
        double e[N];
#pragma unroll
        for (int k = 0; k < N; ++k) e[k] = 0.0;
        if (x.live) {
            filter_element(R, mask, axis, q, v0sq, x.p, e);
            if (FINAL && t == x.seg && L.seg_frag[2 * size_t(R.track[x.p])] != x.f) {
                const double* c = carry + (size_t(x.f) * 2 + axis) * kState;
                double in[N], o[N];
#pragma unroll
                for (int k = 0; k < N; ++k) in[k] = 0.0;
                in[4] = c[0], in[5] = c[1], in[6] = c[2], in[7] = c[3], in[8] = c[4];
                FilterOp::combine(in, e, o);
#pragma unroll
                for (int k = 0; k < N; ++k) e[k] = o[k];
            }
        }
        nc_scan<FilterOp, false>(e, t, x.seg, lds);
        if (!x.live) continue;
        if (FINAL) {
            double* o = fs + (size_t(x.p) * 2 + axis) * kState;
            o[0] = e[4], o[1] = e[5], o[2] = e[6], o[3] = e[7], o[4] = e[8];
        } else if (x.p + 1 == x.fend) {
            double* o = ftot + (size_t(x.f) * 2 + axis) * N;
#pragma unroll
            for (int k = 0; k < N; ++k) o[k] = e[k];
        }
    }
}
// one thread per (track, axis): the state that enters each of the track's fragments, in tile order
__global__ __launch_bounds__(kBlock) void k_filter_carry(const int* __restrict__ seg_frag, int nt, const double* __restrict__ ftot,
                                                         double* __restrict__ carry) {
    constexpr int N = FilterOp::N;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= 2 * nt) return;
    const int c = i >> 1, axis = i & 1;
    double in[N];
#pragma unroll
    for (int k = 0; k < N; ++k) in[k] = 0.0;
    for (int f = seg_frag[2 * size_t(c)], fe = seg_frag[2 * size_t(c) + 1]; f < fe; ++f) {
        double* cr = carry + (size_t(f) * 2 + axis) * kState;
        cr[0] = in[4], cr[1] = in[5], cr[2] = in[6], cr[3] = in[7], cr[4] = in[8];
        const double* src = ftot + (size_t(f) * 2 + axis) * N;
        double e[N], o[N];
#pragma unroll
        for (int k = 0; k < N; ++k) e[k] = src[k];
        FilterOp::combine(in, e, o);
        in[4] = o[4], in[5] = o[5], in[6] = o[6], in[7] = o[7], in[8] = o[8];
    }
}

// nis and the next mask of every row from the state of the row before; *changed counts the rows whose mask differs
__global__ __launch_bounds__(kBlock) void k_gate(Rows R, const unsigned char* __restrict__ mask, const double* __restrict__ fs,
                                                 double q, double gate, double* __restrict__ nis,
                                                 unsigned char* __restrict__ mask_out, int* __restrict__ changed) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= R.m) return;
    const int st = R.start[R.track[p]];
    double v = NAN;
    unsigned char keep = 0;
    if (p >= st && R.valid[p]) {
        v = 0.0;
        keep = 1;
        if (p > st) {
            const double dt = R.t[p] - R.t[p - 1];
            const double q00 = q * (dt * dt * dt / 3.0);
#pragma unroll
            for (int axis = 0; axis < 2; ++axis) {
                const double* s = fs + (size_t(p - 1) * 2 + axis) * kState;
                const double mp = s[0] + dt * s[1];
                const double pp = ((s[2] + dt * s[3]) + dt * (s[3] + dt * s[4])) + q00;
                const double nu = R.z[axis][p] - mp, S = pp + R.r[axis][p];
                v += nu * nu / S;
            }
            keep = (gate > 0.0 && !(v <= gate)) ? 0 : 1;
        }
    }
    nis[p] = v;
    mask_out[p] = keep;
    if (keep != mask[p]) atomicAdd(changed, 1);
}

// ---------------------------------------------------------------- the smoother
__device__ __forceinline__ void smooth_element(const Rows& R, const double* fs, int axis, double q, int p, double (&e)[SmoothOp::N]) {
#pragma unroll
    for (int k = 0; k < SmoothOp::N; ++k) e[k] = 0.0;
    const int c = R.track[p];
    if (p < R.start[c]) return;  // not tracked: nothing reads what these rows combine to
    const double* s = fs + (size_t(p) * 2 + axis) * kState;
    const double m0 = s[0], m1 = s[1], p00 = s[2], p01 = s[3], p11 = s[4];
    if (p + 1 == R.ptr[c + 1]) {  // the track's last row
        e[4] = m0, e[5] = m1, e[6] = p00, e[7] = p01, e[8] = p11;
        return;
    }
    const double dt = R.t[p + 1] - R.t[p];
    const double q00 = q * (dt * dt * dt / 3.0), q01 = q * (dt * dt / 2.0), q11 = q * dt;
    // F P = [f00 f01; p01 p11], the prediction's covariance PP = F P F' + Q, G = (F P)' inv(PP)
    const double f00 = p00 + dt * p01, f01 = p01 + dt * p11;
    const double a00 = (f00 + dt * f01) + q00, a01 = f01 + q01, a11 = p11 + q11;
    const double det = a00 * a11 - a01 * a01;
    const double i00 = a11 / det, i01 = -a01 / det, i11 = a00 / det;
    const double g00 = f00 * i00 + p01 * i01, g01 = f00 * i01 + p01 * i11;
    const double g10 = f01 * i00 + p11 * i01, g11 = f01 * i01 + p11 * i11;
    const double fm0 = m0 + dt * m1;
    e[0] = g00, e[1] = g01, e[2] = g10, e[3] = g11;
    e[4] = m0 - (g00 * fm0 + g01 * m1);
    e[5] = m1 - (g10 * fm0 + g11 * m1);
    e[6] = p00 - (g00 * f00 + g01 * p01);
    e[7] = p01 - (g00 * f01 + g01 * p11);
    e[8] = p11 - (g10 * f01 + g11 * p11);
}
// as k_filter, backwards: stot[f][axis][9] from a fragment's first position; scarry[f][axis][5] = the smoothed state
// of the row after fragment f (not read for a track's last fragment); ss[p][axis][5] = the smoothed state at p
template <bool FINAL>
__global__ __launch_bounds__(kBlock) void k_smooth(Rows R, const double* __restrict__ fs, double q, Frags L,
                                                   double* __restrict__ stot, const double* __restrict__ scarry,
                                                   double* __restrict__ ss) {
    constexpr int N = SmoothOp::N;
    __shared__ double lds[thr::trk::scan_lds<SmoothOp>()];
    const int t = threadIdx.x, axis = blockIdx.y;
    for (int tile = blockIdx.x; tile < L.n_tiles; tile += gridDim.x) {
        const TilePos x = tile_pos(tile, t, R.m, L.pos_frag, L.frag_start);
        double e[N];
#pragma unroll
        for (int k = 0; k < N; ++k) e[k] = 0.0;
        if (x.live) {
            smooth_element(R, fs, axis, q, x.p, e);
            if (FINAL && x.p + 1 == x.fend && L.seg_frag[2 * size_t(R.track[x.p]) + 1] != x.f + 1) {
                const double* c = scarry + (size_t(x.f) * 2 + axis) * kState;
                double in[N], o[N];
#pragma unroll
                for (int k = 0; k < N; ++k) in[k] = 0.0;
                in[4] = c[0], in[5] = c[1], in[6] = c[2], in[7] = c[3], in[8] = c[4];
                SmoothOp::combine(e, in, o);
#pragma unroll
                for (int k = 0; k < N; ++k) e[k] = o[k];
            }
        }
        nc_scan<SmoothOp, true>(e, t, x.live ? x.fend - tile * kTile : t + 1, lds);
        if (!x.live) continue;
        if (FINAL) {
            double* o = ss + (size_t(x.p) * 2 + axis) * kState;
            o[0] = e[4], o[1] = e[5], o[2] = e[6], o[3] = e[7], o[4] = e[8];
        } else if (t == x.seg) {
            double* o = stot + (size_t(x.f) * 2 + axis) * N;
#pragma unroll
            for (int k = 0; k < N; ++k) o[k] = e[k];
        }
    }
}
__global__ __launch_bounds__(kBlock) void k_smooth_carry(const int* __restrict__ seg_frag, int nt, const double* __restrict__ stot,
                                                         double* __restrict__ scarry) {
    constexpr int N = SmoothOp::N;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= 2 * nt) return;
    const int c = i >> 1, axis = i & 1;
    double in[N];
#pragma unroll
    for (int k = 0; k < N; ++k) in[k] = 0.0;
    for (int f = seg_frag[2 * size_t(c) + 1] - 1, fa = seg_frag[2 * size_t(c)]; f >= fa; --f) {
        double* cr = scarry + (size_t(f) * 2 + axis) * kState;
        cr[0] = in[4], cr[1] = in[5], cr[2] = in[6], cr[3] = in[7], cr[4] = in[8];
        const double* src = stot + (size_t(f) * 2 + axis) * N;
        double e[N], o[N];
#pragma unroll
        for (int k = 0; k < N; ++k) e[k] = src[k];
        SmoothOp::combine(e, in, o);
        in[4] = o[4], in[5] = o[5], in[6] = o[6], in[7] = o[7], in[8] = o[8];
    }
}

// ---------------------------------------------------------------- statistics and outputs
struct LoadStats {  // rows, valid, used, nis of the used, path, speed, tracked | first timestamp | last timestamp
    Rows R;
    const unsigned char* mask;
    const double *nis, *ss;
    __device__ void operator()(int p, double (&v)[kStats]) const {
        v[0] = 1.0;
        v[1] = R.valid[p] ? 1.0 : 0.0;
        v[7] = INFINITY;
        v[8] = -INFINITY;
        const int st = R.start[R.track[p]];
        if (p < st) return;
        if (mask[p]) {
            v[2] = 1.0;
            v[3] = nis[p];
        }
        const double* s = ss + size_t(p) * 2 * kState;
        if (p > st) {
            const double dx = s[0] - s[0 - 2 * kState], dy = s[kState] - s[kState - 2 * kState];
            v[4] = sqrt(dx * dx + dy * dy);
        }
        v[5] = sqrt(s[1] * s[1] + s[kState + 1] * s[kState + 1]);
        v[6] = 1.0;
        v[7] = v[8] = R.t[p];
    }
};
__global__ __launch_bounds__(kBlock) void k_track_stats(const double* __restrict__ red, int nt, double* __restrict__ stats,
                                                        int* __restrict__ flags) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= nt) return;
    const double* v = red + size_t(c) * kStats;
    double* o = stats + size_t(c) * 8;
    const bool any = v[6] > 0.0;
    o[0] = v[0];
    o[1] = v[1];
    o[2] = v[2];
    o[3] = v[1] - v[2];
    o[4] = v[2] > 0.0 ? v[3] / v[2] : NAN;
    o[5] = any ? v[8] - v[7] : NAN;
    o[6] = any ? v[4] : NAN;
    o[7] = any ? v[5] / v[6] : NAN;
    flags[c] = 2.0 * v[2] < v[1] ? THR_TRACK_LOST : 0;
}
struct RowOut {
    long long* order;
    unsigned char* used;
    double *nis, *filt, *filt_var, *smooth, *smooth_var;
};
__global__ __launch_bounds__(kBlock) void k_outputs(Rows R, const unsigned* __restrict__ perm, const unsigned char* __restrict__ mask,
                                                    const double* __restrict__ nis, const double* __restrict__ fs,
                                                    const double* __restrict__ ss, RowOut out) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= R.m) return;
    const size_t j = perm[p];
    const bool on = R.tracked(p);
    out.order[p] = (long long)j;
    out.used[j] = on ? mask[p] : 0;
    out.nis[j] = on ? nis[p] : NAN;
#pragma unroll
    for (int axis = 0; axis < 2; ++axis) {
        const double* f = fs + (size_t(p) * 2 + axis) * kState;
        const double* s = ss + (size_t(p) * 2 + axis) * kState;
        out.filt[4 * j + 2 * axis] = on ? f[0] : NAN;
        out.filt[4 * j + 2 * axis + 1] = on ? f[1] : NAN;
        out.smooth[4 * j + 2 * axis] = on ? s[0] : NAN;
        out.smooth[4 * j + 2 * axis + 1] = on ? s[1] : NAN;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            out.filt_var[6 * j + 3 * axis + k] = on ? f[2 + k] : NAN;
            out.smooth_var[6 * j + 3 * axis + k] = on ? s[2 + k] : NAN;
        }
    }
}

thread_local double g_track_ms[6] = {0, 0, 0, 0, 0, 0};

}  // namespace

struct thr_track_result : thr::seg::Result {};

extern "C" int thr_track(int device_id, size_t n, const int32_t* tx, const double* timestamp, const double* x, const double* y,
                         const double* rx, const double* ry, const uint8_t* valid, const thr_track_opts* opts,
                         thr_track_result** result_out, thr_track_counts* counts_out) try {
    if (result_out) *result_out = nullptr;
    if (counts_out) std::memset(counts_out, 0, sizeof(*counts_out));
    for (double& t : g_track_ms) t = 0;
    if (!result_out || !counts_out || !opts) return thr::fail_msg(THR_ERR_ARG, "thr_track: null argument");
    if (n && (!tx || !timestamp || !x || !y || !rx || !ry)) return thr::fail_msg(THR_ERR_ARG, "thr_track: null argument");
    if (n > size_t(1) << 28) return thr::fail_msg(THR_ERR_ARG, "thr_track: too many rows");
    if (!(opts->q >= 0.0) || !std::isfinite(opts->q)) return thr::fail_msg(THR_ERR_ARG, "thr_track: q must be finite and not negative");
    if (!(opts->v0 > 0.0) || !std::isfinite(opts->v0)) return thr::fail_msg(THR_ERR_ARG, "thr_track: v0 must be finite and positive");
    if (!(opts->gate >= 0.0) || !std::isfinite(opts->gate))
        return thr::fail_msg(THR_ERR_ARG, "thr_track: gate must be finite and not negative (0: no gating)");
    if (opts->max_rounds < 1 || opts->max_rounds > 16)
        return thr::fail_msg(THR_ERR_ARG, "thr_track: max_rounds must lie in 1 .. 16, not %d", opts->max_rounds);
    for (size_t i = 0; i < n; ++i) {
        if (!std::isfinite(timestamp[i])) return thr::fail_msg(THR_ERR_ARG, "thr_track: row %zu has a timestamp that is not finite", i);
        if (valid && !valid[i]) continue;
        if (!std::isfinite(x[i]) || !std::isfinite(y[i]))
            return thr::fail_msg(THR_ERR_ARG, "thr_track: valid row %zu has a position that is not finite", i);
        if (!(rx[i] > 0.0) || !(ry[i] > 0.0) || !std::isfinite(rx[i]) || !std::isfinite(ry[i]))
            return thr::fail_msg(THR_ERR_ARG, "thr_track: valid row %zu has a variance that is not finite or not positive", i);
    }

    THR_TRY(thr::seg::pick_device(device_id));
    thr_track_result* R = new thr_track_result;
    thr::seg::ResultGuard guard{R};
    R->device = device_id;
    R->n_out = THR_TRACK_N_OUTPUTS;
    hipStream_t s = nullptr;
    Event ev[6];
    for (Event& e : ev) THR_HIP_TRY(e.create());
    for (Event& e : R->ev) THR_HIP_TRY(e.create());
    const int m = int(n);
    const double q = opts->q, v0sq = opts->v0 * opts->v0, gate = opts->gate;
    DevBuf* O = R->out;
    size_t* B = R->bytes;

    // ---- copies in
    DevBuf d_tx, d_t, d_x, d_y, d_rx, d_ry, d_valid;
    THR_HIP_TRY(d_tx.alloc(n * 4));
    for (DevBuf* b : {&d_t, &d_x, &d_y, &d_rx, &d_ry}) THR_HIP_TRY(b->alloc(n * 8));
    if (valid) THR_HIP_TRY(d_valid.alloc(n));
    THR_HIP_TRY(hipEventRecord(ev[0].e, s));
    if (n) {
        THR_HIP_TRY(hipMemcpy(d_tx.p, tx, n * 4, hipMemcpyHostToDevice));
        THR_HIP_TRY(hipMemcpy(d_t.p, timestamp, n * 8, hipMemcpyHostToDevice));
        THR_HIP_TRY(hipMemcpy(d_x.p, x, n * 8, hipMemcpyHostToDevice));
        THR_HIP_TRY(hipMemcpy(d_y.p, y, n * 8, hipMemcpyHostToDevice));
        THR_HIP_TRY(hipMemcpy(d_rx.p, rx, n * 8, hipMemcpyHostToDevice));
        THR_HIP_TRY(hipMemcpy(d_ry.p, ry, n * 8, hipMemcpyHostToDevice));
        if (valid) THR_HIP_TRY(hipMemcpy(d_valid.p, valid, n, hipMemcpyHostToDevice));
    }
    THR_HIP_TRY(hipEventRecord(ev[1].e, s));

    // ---- sort and layout: rows by (tx, timestamp), tracks, their fragments, their start rows
    thr::seg::Scratch w;
    thr::seg::Cells cells;
    thr::seg::Layout L;
    DevBuf key_hi, key_lo, ts_ptr, ts_key, s_tx, s_t, s_x, s_y, s_rx, s_ry, s_valid, d_track, d_start, d_slab, d_red;
    unsigned n_tracks = 0;
    THR_HIP_TRY(w.head.alloc(n * 4));
    THR_HIP_TRY(w.incl.alloc(n * 4));
    THR_HIP_TRY(s_tx.alloc(n * 4));
    for (DevBuf* b : {&s_t, &s_x, &s_y, &s_rx, &s_ry}) THR_HIP_TRY(b->alloc(n * 8));
    THR_HIP_TRY(s_valid.alloc(n));
    THR_HIP_TRY(d_track.alloc(n * 4));
    if (m) {
        THR_HIP_TRY(key_hi.alloc(n * 8));
        THR_HIP_TRY(key_lo.alloc(n * 4));
        THR_TRY(launch(k_keys, n, s, d_tx.as<int>(), d_t.as<double>(), m, key_hi.as<unsigned long long>(), key_lo.as<unsigned>()));
        THR_TRY(thr::seg::sort_cells(key_hi, key_lo, m, w, cells, ts_ptr, ts_key, s));  // its cells are the (tx, timestamp) ties
        const Cols in{d_tx.as<int>(), d_t.as<double>(),  d_x.as<double>(), d_y.as<double>(),
                      d_rx.as<double>(), d_ry.as<double>(), valid ? d_valid.as<unsigned char>() : nullptr};
        const Sorted out{s_tx.as<int>(), s_t.as<double>(), s_x.as<double>(), s_y.as<double>(),
                         s_rx.as<double>(), s_ry.as<double>(), s_valid.as<unsigned char>()};
        THR_TRY(launch(k_gather_rows, n, s, in, cells.perm.as<unsigned>(), m, out, w.head.as<unsigned>()));
        THR_TRY(thr::seg::scan(w.head.as<unsigned>(), w.incl.as<unsigned>(), m, w, s, &n_tracks));
    }
    const int nt = int(n_tracks);
    THR_HIP_TRY(O[THR_TRACK_TRACK_TX].alloc(size_t(nt) * 4));
    THR_HIP_TRY(O[THR_TRACK_TRACK_PTR].alloc((size_t(nt) + 1) * 8));
    THR_HIP_TRY(d_start.alloc(size_t(nt) * 4));
    if (m) {
        THR_TRY(launch(k_track_layout, n, s, s_tx.as<int>(), w.head.as<unsigned>(), w.incl.as<unsigned>(), m, nt, d_track.as<int>(),
                       O[THR_TRACK_TRACK_PTR].as<long long>(), O[THR_TRACK_TRACK_TX].as<int>()));
        THR_TRY(thr::seg::build_layout(d_track.as<int>(), m, nt, w, L, s));
    } else {
        THR_HIP_TRY(hipMemsetAsync(O[THR_TRACK_TRACK_PTR].p, 0, 8, s));
    }
    const size_t nf = size_t(L.nf);
    THR_HIP_TRY(d_slab.alloc(nf * kStats * 8));
    THR_HIP_TRY(d_red.alloc(size_t(nt) * kStats * 8));
    if (m) {
        THR_TRY((thr::seg::reduce<2, 1, 1>(LoadValid{s_valid.as<unsigned char>()}, L, d_slab.as<double>(), d_red.as<double>(), s)));
        THR_TRY(launch(k_starts, size_t(nt), s, d_red.as<double>(), nt, d_start.as<int>()));
    }
    const Rows rows{s_t.as<double>(), {s_x.as<double>(), s_y.as<double>()}, {s_rx.as<double>(), s_ry.as<double>()},
                    s_valid.as<unsigned char>(), d_track.as<int>(), O[THR_TRACK_TRACK_PTR].as<long long>(), d_start.as<int>(), m};
    const Frags frags{L.pos_frag.as<int>(), L.frag_start.as<int>(), L.seg_frag.as<int>(), thr::seg::tiles_of(m)};
    const dim3 tiles2(thr::seg::tile_grid(frags.n_tiles).x, 2);
    THR_HIP_TRY(hipEventRecord(ev[2].e, s));

    // ---- the filter rounds
    DevBuf d_mask[2], d_nis, d_fs, d_ftot, d_carry, d_changed;
    for (DevBuf& b : d_mask) THR_HIP_TRY(b.alloc(n));
    THR_HIP_TRY(d_nis.alloc(n * 8));
    THR_HIP_TRY(d_fs.alloc(n * 2 * kState * 8));
    THR_HIP_TRY(d_ftot.alloc(nf * 2 * FilterOp::N * 8));
    THR_HIP_TRY(d_carry.alloc(nf * 2 * kState * 8));
    THR_HIP_TRY(d_changed.alloc(4));
    int cur = 0, rounds = 0, converged = 0;
    if (m) THR_HIP_TRY(hipMemcpyAsync(d_mask[0].p, s_valid.p, n, hipMemcpyDeviceToDevice, s));
    const auto filter_run = [&](int* changed) -> int {
        const unsigned char* mask = d_mask[cur].as<unsigned char>();
        *changed = 0;
        ++rounds;
        if (!m) return THR_OK;
        THR_TRY(launch_grid(k_filter<false>, tiles2, s, rows, mask, q, v0sq, frags, d_ftot.as<double>(), nullptr, nullptr));
        THR_TRY(launch(k_filter_carry, size_t(nt) * 2, s, frags.seg_frag, nt, d_ftot.as<double>(), d_carry.as<double>()));
        THR_TRY(launch_grid(k_filter<true>, tiles2, s, rows, mask, q, v0sq, frags, nullptr, d_carry.as<double>(), d_fs.as<double>()));
        THR_HIP_TRY(hipMemsetAsync(d_changed.p, 0, 4, s));
        THR_TRY(launch(k_gate, n, s, rows, mask, d_fs.as<double>(), q, gate, d_nis.as<double>(), d_mask[cur ^ 1].as<unsigned char>(),
                       d_changed.as<int>()));
        THR_HIP_TRY(hipMemcpy(changed, d_changed.p, 4, hipMemcpyDeviceToHost));  // synchronises
        return THR_OK;
    };
    for (int round = 0; round < opts->max_rounds && !converged; ++round) {
        int changed = 0;
        THR_TRY(filter_run(&changed));
        if (changed == 0) converged = 1; else cur ^= 1;
    }
    if (!converged) {  // one more run with the last mask: the states, nis and used are this run's
        int changed = 0;
        THR_TRY(filter_run(&changed));
    }
    const unsigned char* mask = d_mask[cur].as<unsigned char>();
    THR_HIP_TRY(hipEventRecord(ev[3].e, s));

    // ---- the smoother
    DevBuf d_ss, d_stot;
    THR_HIP_TRY(d_ss.alloc(n * 2 * kState * 8));
    THR_HIP_TRY(d_stot.alloc(nf * 2 * SmoothOp::N * 8));
    if (m) {
        THR_TRY(launch_grid(k_smooth<false>, tiles2, s, rows, d_fs.as<double>(), q, frags, d_stot.as<double>(), nullptr, nullptr));
        THR_TRY(launch(k_smooth_carry, size_t(nt) * 2, s, frags.seg_frag, nt, d_stot.as<double>(), d_carry.as<double>()));
        THR_TRY(launch_grid(k_smooth<true>, tiles2, s, rows, d_fs.as<double>(), q, frags, nullptr, d_carry.as<double>(), d_ss.as<double>()));
    }
    THR_HIP_TRY(hipEventRecord(ev[4].e, s));

    // ---- statistics and the outputs in input row order
    THR_HIP_TRY(O[THR_TRACK_ORDER].alloc(n * 8));
    THR_HIP_TRY(O[THR_TRACK_USED].alloc(n));
    THR_HIP_TRY(O[THR_TRACK_NIS].alloc(n * 8));
    for (int k : {THR_TRACK_FILT, THR_TRACK_SMOOTH}) THR_HIP_TRY(O[k].alloc(n * 32));
    for (int k : {THR_TRACK_FILT_VAR, THR_TRACK_SMOOTH_VAR}) THR_HIP_TRY(O[k].alloc(n * 48));
    THR_HIP_TRY(O[THR_TRACK_TRACK_STATS].alloc(size_t(nt) * 64));
    THR_HIP_TRY(O[THR_TRACK_TRACK_FLAGS].alloc(size_t(nt) * 4));
    std::vector<double> h_stats(size_t(nt) * 8);
    if (m) {
        THR_TRY((thr::seg::reduce<kStats, 7, 1>(LoadStats{rows, mask, d_nis.as<double>(), d_ss.as<double>()}, L, d_slab.as<double>(),
                                                 d_red.as<double>(), s)));
        THR_TRY(launch(k_track_stats, size_t(nt), s, d_red.as<double>(), nt, O[THR_TRACK_TRACK_STATS].as<double>(),
                       O[THR_TRACK_TRACK_FLAGS].as<int>()));
        const RowOut out{O[THR_TRACK_ORDER].as<long long>(), O[THR_TRACK_USED].as<unsigned char>(), O[THR_TRACK_NIS].as<double>(),
                         O[THR_TRACK_FILT].as<double>(),     O[THR_TRACK_FILT_VAR].as<double>(),     O[THR_TRACK_SMOOTH].as<double>(),
                         O[THR_TRACK_SMOOTH_VAR].as<double>()};
        THR_TRY(launch(k_outputs, n, s, rows, cells.perm.as<unsigned>(), mask, d_nis.as<double>(), d_fs.as<double>(),
                       d_ss.as<double>(), out));
        THR_HIP_TRY(hipMemcpy(h_stats.data(), O[THR_TRACK_TRACK_STATS].p, h_stats.size() * 8, hipMemcpyDeviceToHost));
    }
    THR_HIP_TRY(hipEventRecord(ev[5].e, s));
    THR_HIP_TRY(hipEventSynchronize(ev[5].e));  // the temporaries go out of scope
    for (int k = 0; k < 5; ++k) {
        float ms = 0;
        THR_HIP_TRY(hipEventElapsedTime(&ms, ev[k].e, ev[k + 1].e));
        g_track_ms[k] = ms;
    }

    B[THR_TRACK_ORDER] = B[THR_TRACK_NIS] = n * 8;
    B[THR_TRACK_USED] = n;
    B[THR_TRACK_FILT] = B[THR_TRACK_SMOOTH] = n * 32;
    B[THR_TRACK_FILT_VAR] = B[THR_TRACK_SMOOTH_VAR] = n * 48;
    B[THR_TRACK_TRACK_TX] = B[THR_TRACK_TRACK_FLAGS] = size_t(nt) * 4;
    B[THR_TRACK_TRACK_PTR] = (size_t(nt) + 1) * 8;
    B[THR_TRACK_TRACK_STATS] = size_t(nt) * 64;
    counts_out->rows = n;
    counts_out->tracks = size_t(nt);
    for (int c = 0; c < nt; ++c) {
        counts_out->used += size_t(h_stats[size_t(c) * 8 + 2]);
        counts_out->rejected += size_t(h_stats[size_t(c) * 8 + 3]);
    }
    counts_out->rounds = size_t(rounds);
    counts_out->converged = size_t(converged);
    *result_out = R;
    guard.r = nullptr;
    return THR_OK;
} catch (const std::bad_alloc&) {
    return thr::fail_msg(THR_ERR_DEVICE, "thr_track: out of host memory");
} catch (...) {
    return thr::on_exception("thr_track");
}

extern "C" int thr_track_fetch(thr_track_result* R, int which, void* dst, size_t dst_bytes) try {
    return thr::seg::fetch("thr_track_fetch", R, which, dst, dst_bytes, &g_track_ms[5]);
} catch (...) {
    return thr::on_exception("thr_track_fetch");
}

extern "C" void thr_track_free(thr_track_result* R) { thr::seg::free_result(R); }

extern "C" int thr_debug_track_times(double* ms_out) try {
    if (!ms_out) return thr::fail_msg(THR_ERR_ARG, "thr_debug_track_times: null argument");
    for (int k = 0; k < 6; ++k) ms_out[k] = g_track_ms[k];
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_track_times");
}

extern "C" int thr_debug_track_geometry(int* tile_len, int* workgroup, int* element_doubles) try {
    return thr::seg::geometry("thr_debug_track_geometry", tile_len, workgroup, element_doubles, FilterOp::N);
} catch (...) {
    return thr::on_exception("thr_debug_track_geometry");
}
