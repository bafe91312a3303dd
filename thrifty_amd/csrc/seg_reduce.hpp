// The segmented reduction of the statistics stages (toadstats.hip, syncstats.hip, reldist.hip), and the host side
// those stages share: the result handle with its fetch, the device pick, the time record.
//
// Every reduction has one form: positions are cut into tiles of kTile; a FRAGMENT is a maximal run of one
// segment (a cell, a cut, a receiver's cells) inside one tile; a workgroup reduces a tile with a segmented
// Hillis-Steele scan through LDS and the fragment's last position stores its partials to a slab; a second
// launch combines each segment's fragments in tile order.  No floating-point atomic, nothing depends on the
// grid: a repeated call returns the same bits.
//
// A stage brings the layout -- per position its fragment (pos_frag), per fragment its first position
// (frag_start: nf + 1 entries, the last one m), per segment the range of its fragments -- and a load functor
// that fills the K slots of a position: the first NSUM are summed, the next NMIN take the minimum, the rest
// the maximum.  A kernel that needs more around the load than a functor can hold (toadstats' pass 2) is built
// from tile_pos and seg_scan directly.
//
// Every launch of these stages goes through launch() / launch_grid(), which take the parameter types from the
// kernel; the tail every stage ends in (free, the five times, the geometry) stands once beside fetch().
//
// Everything here is a template, inline, or static: every translation unit of a stage includes it.  The one
// exception is tile_grid(), which is declared here and defined once, in toadstats.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/thrifty_hip.h"
#include "post_stages.hpp"

// both stages repeat numpy's float64 operations one by one: no a * b + c may become an fma in a load functor
// that is inlined here (the build also passes -ffp-contract=off to both files, thrifty_amd/build.py)
#pragma clang fp contract(off)

namespace thr {
namespace seg {

constexpr int kBlock = 256;  // workgroup size of every kernel of these stages
constexpr int kTile = 256;   // positions per tile: one per thread
constexpr int kChunk = 8;    // slots that go through LDS together
constexpr int kScanLds = 2 * kChunk * kTile;  // doubles of LDS that seg_scan alternates between
constexpr int kMaxTileGrid = 2048;            // workgroups of a tile kernel: each loops over its tiles
static_assert(kTile == kBlock, "one position per thread");

inline dim3 grid_for(size_t n) { return dim3(unsigned((n + kBlock - 1) / kBlock)); }
inline int tiles_of(int m) { return (m + kTile - 1) / kTile; }
constexpr int kTileGridLimit = 65536;         // the largest cap thr_debug_seg_tile_grid takes

// The grid of a tile kernel over n_tiles tiles: min(n_tiles, cap) workgroups, the cap being kMaxTileGrid unless
// thr_debug_seg_tile_grid has set another.  That setter is for tests: the cap decides which workgroup walks which
// tile and how many trips its loop takes, and moves no result.  Every tile launch of every stage asks here and is
// counted here (thr_debug_seg_tile_stats).  One definition for the library, beside the two entry points in
// toadstats.hip, where the cap and the counts live.
dim3 tile_grid(int n_tiles);

// a step that returns THR_OK or an error which is already worded
#define THR_TRY(expr)                           \
    do {                                        \
        if (const int rc_ = (expr)) return rc_; \
    } while (0)

// k on `grid` workgroups of kBlock.  The parameter types are the kernel's own, so the arguments convert as in
// a plain call: buf.as<unsigned>() to const unsigned*, nullptr to any pointer.
template <class... P, class... A>
int launch_grid(void (*k)(P...), dim3 grid, hipStream_t s, A&&... a) {
    static_assert(sizeof...(P) == sizeof...(A), "one argument per parameter of the kernel");
    hipLaunchKernelGGL(k, grid, dim3(kBlock), 0, s, static_cast<P>(a)...);
    THR_HIP_TRY(hipGetLastError());
    return THR_OK;
}
// one thread for each of n items; nothing is launched for none
template <class... P, class... A>
int launch(void (*k)(P...), size_t n, hipStream_t s, A&&... a) {
    if (n == 0) return THR_OK;
    return launch_grid(k, grid_for(n), s, static_cast<A&&>(a)...);
}

// order-preserving map of int32 onto unsigned, for the radix sorts' keys
__device__ __forceinline__ unsigned key_i32(int v) { return unsigned(v) ^ 0x80000000u; }
__device__ __forceinline__ int unkey_i32(unsigned k) { return int(k ^ 0x80000000u); }
// numpy's min / max: a NaN wins
__device__ __forceinline__ double pmin(double a, double b) { return a != a ? a : (b != b ? b : (b < a ? b : a)); }
__device__ __forceinline__ double pmax(double a, double b) { return a != a ? a : (b != b ? b : (b > a ? b : a)); }
__device__ __forceinline__ double comb(int slot, int n_sum, int n_min, double a, double b) {
    return slot < n_sum ? a + b : (slot < n_sum + n_min ? pmin(a, b) : pmax(a, b));
}

// Segmented inclusive scan over the workgroup's kTile positions: after it, v of a position holds the
// combination of its fragment's positions up to itself.  The tree a fragment is combined in depends on where
// it lies in its tile and on nothing else.  Two LDS buffers alternate, so one barrier per step is enough:
// the buffer written in step i + 2 was last read in step i, before the barrier of step i + 1.
template <int K, int NSUM, int NMIN>
__device__ __forceinline__ void seg_scan(double (&v)[K], int t, int seg_start, double* lds) {
    int buf = 0;
#pragma unroll
    for (int base = 0; base < K; base += kChunk) {
        for (int d = 1; d < kTile; d <<= 1) {
            double* b = lds + buf * (kChunk * kTile);
#pragma unroll
            for (int k = 0; k < kChunk; ++k)
                if (base + k < K) b[k * kTile + t] = v[base + k];
            __syncthreads();
            if (t - d >= seg_start) {
#pragma unroll
                for (int k = 0; k < kChunk; ++k)
                    if (base + k < K) v[base + k] = comb(base + k, NSUM, NMIN, b[k * kTile + t - d], v[base + k]);
            }
            buf ^= 1;
        }
    }
    __syncthreads();  // the next trip starts writing buffer 0 again
}

// thread t's position in a tile: p, its fragment f, the fragment's start relative to the tile (the scan's
// segment start) and one past its last position
struct TilePos {
    int p, f, seg, fend;
    bool live;
};
__device__ __forceinline__ TilePos tile_pos(int tile, int t, int m, const int* pos_frag, const int* frag_start) {
    TilePos x;
    x.p = tile * kTile + t;
    x.live = x.p < m;
    x.f = 0;
    x.seg = t;  // a position past the end is a segment of its own, which nobody reads
    x.fend = -1;
    if (x.live) {
        x.f = pos_frag[x.p];
        x.seg = frag_start[x.f] - tile * kTile;  // >= 0: every tile starts a fragment
        x.fend = frag_start[x.f + 1];
    }
    return x;
}

// load(p, v) fills the K slots of position p (p < m; they are zero before); the slab gets one row of K per fragment
template <int K, int NSUM, int NMIN, class Load>
__global__ __launch_bounds__(kBlock) void k_reduce(Load load, int m, int n_tiles, const int* __restrict__ pos_frag,
                                                   const int* __restrict__ frag_start, double* __restrict__ slab) {
    __shared__ double lds[kScanLds];
    const int t = threadIdx.x;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const TilePos x = tile_pos(tile, t, m, pos_frag, frag_start);
        double v[K];
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = 0.0;
        if (x.live) load(x.p, v);
        seg_scan<K, NSUM, NMIN>(v, t, x.seg, lds);
        if (x.live && x.p + 1 == x.fend) {
#pragma unroll
            for (int k = 0; k < K; ++k) slab[size_t(x.f) * K + k] = v[k];
        }
    }
}
// out[o][k] = in[a][k] (+) in[a + 1][k] (+) ... in[e - 1][k] in that order, a = begin[o * stride] and
// e = end[o * stride]; slot k's operation as in comb(); zeros for an empty range.  A CSR table `first` is
// (first, first + 1, 1), a table of {begin, end} pairs is (pairs, pairs + 1, 2).
static __global__ __launch_bounds__(kBlock) void k_combine(const double* __restrict__ in, const int* begin, const int* end,
                                                           int stride, int n_out, int K, int n_sum, int n_min,
                                                           double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (long long)n_out * K) return;
    const int o = int(i / K), k = int(i % K);
    const int a = begin[size_t(o) * stride], e = end[size_t(o) * stride];
    double acc = 0.0;
    if (a < e) {
        acc = in[size_t(a) * K + k];
        for (int s = a + 1; s < e; ++s) acc = comb(k, n_sum, n_min, acc, in[size_t(s) * K + k]);
    }
    out[i] = acc;
}
static __global__ __launch_bounds__(kBlock) void k_iota(unsigned* __restrict__ a, int m) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j < m) a[j] = unsigned(j);
}

// slab[nf][K] (device) = the partials of load() over every fragment of the m positions
template <int K, int NSUM, int NMIN, class Load>
int launch_reduce(const Load& load, int m, const int* pos_frag, const int* frag_start, double* slab, hipStream_t s) {
    const int n_tiles = tiles_of(m);
    return launch_grid(k_reduce<K, NSUM, NMIN, Load>, tile_grid(n_tiles), s, load, m, n_tiles, pos_frag, frag_start, slab);
}
inline int launch_combine(const double* in, const int* begin, const int* end, int stride, int n_out, int K, int n_sum,
                          int n_min, double* out, hipStream_t s) {
    return launch(k_combine, size_t(n_out) * K, s, in, begin, end, stride, n_out, K, n_sum, n_min, out);
}

// ------------------------------------------------------------------ the host side of a stage
constexpr int max_of(int a, int b) { return a > b ? a : b; }
constexpr int kMaxOutputs =
    max_of(max_of(THR_TSTATS_N_OUTPUTS, THR_BSYNC_N_OUTPUTS), max_of(THR_TDSTATS_N_OUTPUTS, THR_RELDIST_N_OUTPUTS));
struct Result {  // what a call leaves on the device; thr_tstats, thr_bsync, thr_tdstats and thr_reldist are this
    int device = 0, n_out = 0;
    DevBuf out[kMaxOutputs];
    size_t bytes[kMaxOutputs] = {};
    Event ev[2];
    virtual ~Result() = default;
};
struct ResultGuard {  // frees the result unless it is handed to the caller
    Result* r;
    ~ResultGuard() { delete r; }
};

// one output to the host; the copy's time is added to *ms_out
inline int fetch(const char* who, Result* R, int which, void* dst, size_t dst_bytes, double* ms_out) {
    if (!R || which < 0 || which >= R->n_out) return thr::fail_msg(THR_ERR_ARG, "%s: no such result or output (%d)", who, which);
    const size_t bytes = R->bytes[which];
    if (dst_bytes != bytes)
        return thr::fail_msg(THR_ERR_ARG, "%s: output %d holds %zu bytes, not %zu", who, which, bytes, dst_bytes);
    if (bytes == 0) return THR_OK;
    if (!dst) return thr::fail_msg(THR_ERR_ARG, "%s: null argument", who);
    THR_HIP_TRY(hipSetDevice(R->device));
    THR_HIP_TRY(hipEventRecord(R->ev[0].e, nullptr));
    THR_HIP_TRY(hipMemcpy(dst, R->out[which].p, bytes, hipMemcpyDeviceToHost));
    THR_HIP_TRY(hipEventRecord(R->ev[1].e, nullptr));
    THR_HIP_TRY(hipEventSynchronize(R->ev[1].e));
    float ms = 0;
    THR_HIP_TRY(hipEventElapsedTime(&ms, R->ev[0].e, R->ev[1].e));
    *ms_out += ms;
    return THR_OK;
}

// the tail of a stage: thr_*_free, thr_debug_*_times and thr_debug_*_geometry are one call of these each
inline void free_result(Result* R) {
    if (!R) return;
    (void)hipSetDevice(R->device);  // the buffers are freed on the device they were taken from
    delete R;
}
inline int copy_times(const char* who, const double (&ms)[5], double* ms_out) {
    if (!ms_out) return thr::fail_msg(THR_ERR_ARG, "%s: null argument", who);
    for (int i = 0; i < 5; ++i) ms_out[i] = ms[i];
    return THR_OK;
}
inline int geometry(const char* who, int* tile_len, int* workgroup, int* third, int third_value) {
    if (!tile_len || !workgroup || !third) return thr::fail_msg(THR_ERR_ARG, "%s: null argument", who);
    *tile_len = kTile;
    *workgroup = kBlock;
    *third = third_value;
    return THR_OK;
}
inline int geometry(const char* who, int* tile_len, int* workgroup) {
    int none;
    return geometry(who, tile_len, workgroup, &none, 0);
}

inline int pick_device(int device_id) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return thr::fail_msg(THR_ERR_DEVICE, "no HIP device available (this engine has no CPU fallback)");
    if (device_id < 0 || device_id >= ndev) return thr::fail_msg(THR_ERR_ARG, "bad device_id %d", device_id);
    THR_HIP_TRY(hipSetDevice(device_id));
    return THR_OK;
}

// waits for the last of a call's five events; ms_out[0..3] = the four intervals between them
inline int record_times(Event (&ev)[5], double* ms_out) {
    THR_HIP_TRY(hipEventSynchronize(ev[4].e));
    for (int i = 0; i < 4; ++i) {
        float ms = 0;
        THR_HIP_TRY(hipEventElapsedTime(&ms, ev[i].e, ev[i + 1].e));
        ms_out[i] = ms;
    }
    return THR_OK;
}

}  // namespace seg
}  // namespace thr
