// Detection statistics on the device (reference thrifty/toads_analysis.py: split_rxtx, print_stats, the
// numbers behind its minute / carrier-bin / offset histograms and plot_timestamp_residuals): per
// (rxid, txid) cell the count, mean, population std, min and max of nine quantities and three integer
// histograms; per receiver the straight line timestamp ~ a * soa + b with its residuals.
//
//   1. sort and cells   key = order-preserving pack of (rxid, txid); hipCUB's stable radix sort of (key,
//                       selection index); head flags of cells, receivers and FRAGMENTS, one inclusive scan of
//                       the three; the eleven columns are gathered into sorted order once (k_gather, which
//                       also makes the two dB columns: log10 appears there and nowhere else);
//   2. tiles            every reduction is seg_reduce.hpp's: tiles of kTile positions, fragments, a segmented scan
//                       through LDS, a slab, a combining launch (the form and why it returns the same bits every
//                       time are described there).  A tile holds one fragment of a big cell or many whole small
//                       cells; one combining launch sums each cell's fragments in tile order, another each
//                       receiver's cells in cell order;
//   3. pass 1           sum, min, max of the nine quantities, of timestamp and soa;
//   4. pass 2           sum (x - mean)^2, the fit's centred moments in u = (soa - mean) / max|soa - mean|, the
//                       three histograms: a tile that is one fragment of a cell counts in LDS when the cell's
//                       carrier bins, the ten offset bins and the TILE's own window of minutes fit kHist counters,
//                       and flushes one integer atomic per non-zero counter; every other tile (several fragments,
//                       or a range too wide) uses global integer atomics directly;
//   5. pass 3           residuals scattered to selection order, their sum of squares and largest magnitude
//                       through the same slab form;
//   6. finish           small kernels: the float64 divisions and sqrt, the linspace edges, the line.
// No floating-point atomic anywhere, no flag or ticket between workgroups: separate launches.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>

#include "../../include/thrifty_hip.h"
#include "post_stages.hpp"
#include "seg_reduce.hpp"

// the histogram edges and bin indices repeat numpy's float64 operations one by one: no a * b + c may
// become an fma in this file (the build also passes -ffp-contract=off, thrifty_amd/build.py)
#pragma clang fp contract(off)

namespace {

using thr::DevBuf;
using thr::Event;
using thr::with_temp;
using namespace thr::seg;  // kBlock, kTile (_native.TOADSTATS_WORKGROUP, _TILE), the keys, the reduction, Result

constexpr int kHist = 4096;   // LDS histogram counters of pass 2
constexpr int kQ = 9;         // quantities per cell
constexpr long long kMaxBins = 1ll << 26;

// pass 1 slots: sums (9 quantities, timestamp, soa), mins (9 quantities, soa), maxs (9 quantities, timestamp, soa)
constexpr int kK1 = 32, kS1 = 11, kM1 = 10;
constexpr int kSumTs = 9, kSumSoa = 10, kMinQ = 11, kMinSoa = 20, kMaxQ = 21, kMaxTs = 30, kMaxSoa = 31;
// pass 2 slots, all sums: 9 squared deviations, u, u^2, v, u * v
constexpr int kK2 = 13;
// pass 3 slots: sum of r^2, max |r|
constexpr int kK3 = 2;
// sorted columns: the nine quantities, then timestamp - time0, then soa
constexpr int kCols = 11, kColTs = 9, kColSoa = 10;

struct Cols {
    const int *rx, *tx, *bin;
    const double *ts, *soa, *coff, *ce, *cn, *en, *no, *off;
    const long long* sel;
};
struct Trip {  // head flags of cell, fragment, receiver -- and their inclusive sums
    unsigned c, f, r;
};
struct TripSum {
    __host__ __device__ Trip operator()(const Trip& a, const Trip& b) const {
        return Trip{a.c + b.c, a.f + b.f, a.r + b.r};
    }
};

__global__ __launch_bounds__(kBlock) void k_keys(Cols c, int m, unsigned long long* __restrict__ keys,
                                                 unsigned* __restrict__ idx) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    const long long row = c.sel ? c.sel[j] : (long long)j;  // checked on the host: 0 <= row < n
    keys[j] = ((unsigned long long)key_i32(c.rx[row]) << 32) | key_i32(c.tx[row]);
    idx[j] = unsigned(j);
}

__device__ __forceinline__ Trip flags_at(const unsigned long long* keys, int p) {
    const unsigned long long k = keys[p];
    const bool head = p == 0 || keys[p - 1] != k;
    const bool rxh = p == 0 || (keys[p - 1] >> 32) != (k >> 32);
    return Trip{head ? 1u : 0u, (head || p % kTile == 0) ? 1u : 0u, rxh ? 1u : 0u};
}
__global__ __launch_bounds__(kBlock) void k_heads(const unsigned long long* __restrict__ keys, int m,
                                                  Trip* __restrict__ out) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p < m) out[p] = flags_at(keys, p);
}
// tables of the cells (nc + 1 entries), receivers (nr + 1) and fragments (nf + 1); per position its
// fragment and its cell
__global__ __launch_bounds__(kBlock) void k_layout(
    const unsigned long long* __restrict__ keys, const Trip* __restrict__ incl, int m, int nc, int nf, int nr,
    long long* __restrict__ cell_ptr, int* __restrict__ cell_rx, int* __restrict__ cell_tx,
    int* __restrict__ cell_frag, int* __restrict__ cell_rxi, int* __restrict__ rx_cell, int* __restrict__ rx_id,
    int* __restrict__ rx_ptr, int* __restrict__ frag_start, int* __restrict__ pos_frag, int* __restrict__ pos_cell) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= m) return;
    const Trip fl = flags_at(keys, p), t = incl[p];
    const int c = int(t.c) - 1, f = int(t.f) - 1, r = int(t.r) - 1;
    pos_frag[p] = f;
    pos_cell[p] = c;
    if (fl.f) frag_start[f] = p;
    if (fl.c) {
        const unsigned long long k = keys[p];
        cell_ptr[c] = p;
        cell_rx[c] = unkey_i32(unsigned(k >> 32));
        cell_tx[c] = unkey_i32(unsigned(k));
        cell_frag[c] = f;
        cell_rxi[c] = r;
    }
    if (fl.r) {
        rx_cell[r] = c;
        rx_id[r] = unkey_i32(unsigned(keys[p] >> 32));
        rx_ptr[r] = p;
    }
    if (p == m - 1) {
        cell_ptr[nc] = m;
        cell_frag[nc] = nf;
        rx_cell[nr] = nc;
        rx_ptr[nr] = m;
        frag_start[nf] = m;
    }
}

// The eleven columns in sorted order (S[col * m + p]), ORDER, and the two dB columns in selection order.
// The dB value of a / b: a division, the logarithm, a multiplication by 20, as numpy -- the only two log10
// calls of this file.
__global__ __launch_bounds__(kBlock) void k_gather(Cols c, const unsigned* __restrict__ perm, int m, double time0,
                                                   double* __restrict__ S, long long* __restrict__ order,
                                                   double* __restrict__ snr_db) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= m) return;
    const unsigned j = perm[p];
    const long long row = c.sel ? c.sel[j] : (long long)j;
    order[p] = row;
    const double ce = c.ce[row], cn = c.cn[row], en = c.en[row], no = c.no[row];
    const double cdb = 20.0 * log10(ce / cn), db = 20.0 * log10(en / no);
    const size_t M = size_t(m);
    S[0 * M + p] = ce;
    S[1 * M + p] = cn;
    S[2 * M + p] = cdb;
    S[3 * M + p] = double(c.bin[row]);
    S[4 * M + p] = c.coff[row];
    S[5 * M + p] = en;
    S[6 * M + p] = no;
    S[7 * M + p] = db;
    S[8 * M + p] = c.off[row];
    S[kColTs * M + p] = c.ts[row] - time0;
    S[kColSoa * M + p] = c.soa[row];
    snr_db[2 * size_t(j)] = cdb;
    snr_db[2 * size_t(j) + 1] = db;
}

// pass 1: sums, minima and maxima of the sorted columns (the slots of kK1)
struct LoadPass1 {
    const double* S;
    size_t M;
    __device__ void operator()(int p, double (&v)[kK1]) const {
#pragma unroll
        for (int q = 0; q < kQ; ++q) {
            const double a = S[q * M + p];
            v[q] = a;
            v[kMinQ + q] = a;
            v[kMaxQ + q] = a;
        }
        const double ts = S[kColTs * M + p], soa = S[kColSoa * M + p];
        v[kSumTs] = ts;
        v[kMaxTs] = ts;
        v[kSumSoa] = soa;
        v[kMinSoa] = soa;
        v[kMaxSoa] = soa;
    }
};

// after pass 1, per cell: mean, min, max; the histogram lengths; the offset histogram's edges (numpy's
// linspace(first, last, 11): i * step + first, the last edge set to `last`)
__global__ __launch_bounds__(kBlock) void k_mid_cells(const double* __restrict__ cv, const long long* __restrict__ cell_ptr,
                                                      int nc, double* __restrict__ stats, long long* __restrict__ mlen,
                                                      long long* __restrict__ blen, int* __restrict__ bin_first,
                                                      double* __restrict__ edges, int* __restrict__ flags) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= nc) return;
    const double* v = cv + size_t(c) * kK1;
    const double count = double(cell_ptr[c + 1] - cell_ptr[c]);
    for (int q = 0; q < kQ; ++q) {
        double* s = stats + (size_t(c) * kQ + q) * 4;
        s[0] = v[q] / count;
        s[2] = v[kMinQ + q];
        s[3] = v[kMaxQ + q];
    }
    mlen[c] = (long long)floor(v[kMaxTs] / 60.0) + 1;  // host-checked: below 2^26
    bin_first[c] = int(v[kMinQ + 3]);
    blen[c] = (long long)v[kMaxQ + 3] - (long long)v[kMinQ + 3] + 1;
    double lo = v[kMinQ + 8], hi = v[kMaxQ + 8];
    const bool bad = !(isfinite(lo) && isfinite(hi));
    flags[c] = bad ? THR_TSTATS_FLAG_OFFSET_NONFINITE : 0;
    double* e = edges + size_t(c) * 11;
    if (bad) {
        for (int i = 0; i <= 10; ++i) e[i] = NAN;
        return;
    }
    if (lo == hi) {
        lo = lo - 0.5;
        hi = hi + 0.5;
    }
    const double delta = hi - lo, step = delta / 10.0;
    for (int i = 0; i < 10; ++i) {
        const double y = step == 0.0 ? (double(i) / 10.0) * delta : double(i) * step;
        e[i] = y + lo;
    }
    e[10] = hi;
}
// per receiver: the means of soa and timestamp and the scale max|soa - mean|.  fl(x - mean) is monotone in
// x, so the largest magnitude is taken at the smallest or the largest soa.
__global__ __launch_bounds__(kBlock) void k_mid_rx(const double* __restrict__ rv, const int* __restrict__ rx_ptr, int nr,
                                                   double* __restrict__ rxp, long long* __restrict__ rx_count) {
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= nr) return;
    const double* v = rv + size_t(r) * kK1;
    const long long n = rx_ptr[r + 1] - rx_ptr[r];
    rx_count[r] = n;
    const double mean_soa = v[kSumSoa] / double(n), mean_ts = v[kSumTs] / double(n);
    double scale = fmax(fabs(v[kMaxSoa] - mean_soa), fabs(v[kMinSoa] - mean_soa));
    if (!(v[kMinSoa] < v[kMaxSoa])) scale = NAN;  // fewer than two distinct soa (or a NaN): no line
    rxp[size_t(r) * 3] = mean_soa;
    rxp[size_t(r) * 3 + 1] = mean_ts;
    rxp[size_t(r) * 3 + 2] = scale;
}

// numpy.histogram's bin of x (uniform bins): index, then the two corrections against the edges
__device__ __forceinline__ int offset_bin(double x, const double* e) {
    const double first = e[0], denom = e[10] - e[0];
    const double f = ((x - first) / denom) * 10.0;
    long long i = (long long)f;
    if (i < 0) i = 0;  // cannot happen for first <= x <= last; the index stays inside the ten counters
    if (i >= 10) i = 9;
    if (x < e[i] && i > 0) i -= 1;
    if (i != 9 && x >= e[i + 1]) i += 1;
    return int(i);
}

__global__ __launch_bounds__(kBlock) void k_pass2(
    const double* __restrict__ S, int m, int n_tiles, const int* __restrict__ pos_frag,
    const int* __restrict__ frag_start, const int* __restrict__ pos_cell, const double* __restrict__ stats,
    const int* __restrict__ cell_rxi, const double* __restrict__ rxp, const long long* __restrict__ blen, const int* __restrict__ bin_first, const double* __restrict__ edges,
    const int* __restrict__ flags, const long long* __restrict__ minute_ptr, const long long* __restrict__ bin_ptr,
    unsigned long long* minute_hist, unsigned long long* bin_hist, unsigned long long* offset_hist,
    double* __restrict__ slab) {
    __shared__ double lds[kScanLds];
    __shared__ unsigned hist[kHist];
    __shared__ int s_minute[2];  // the tile's smallest and largest minute
    const int t = threadIdx.x;
    const size_t M = size_t(m);
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const TilePos x = tile_pos(tile, t, m, pos_frag, frag_start);
        // A tile that is one fragment of a cell (workgroup-uniform) counts in LDS when its ranges fit the
        // counters: the cell's carrier bins, the ten offset bins, and the minutes from the TILE's smallest
        // to its largest (rows of a cell are in input order, as a rule by time, so a tile's window is
        // narrow however long the cell's history is).
        const int p0 = tile * kTile, p1 = min(p0 + kTile, m) - 1;
        const int c0 = pos_cell[p0];
        const long long bl0 = blen[c0];
        const bool one = pos_frag[p0] == pos_frag[p1];
        const double ts = x.live ? S[kColTs * M + x.p] : 0.0;
        const long long minute = (long long)floor(ts / 60.0);  // host-checked: below 2^26
        long long m_lo = 0, ml0 = 0;
        bool in_lds = false;
        if (one) {
            if (t == 0) {
                s_minute[0] = 0x7FFFFFFF;
                s_minute[1] = 0;
            }
            for (int i = t; i < kHist; i += kBlock) hist[i] = 0u;
            __syncthreads();
            if (x.live) {
                atomicMin(&s_minute[0], int(minute));
                atomicMax(&s_minute[1], int(minute));
            }
            __syncthreads();
            m_lo = s_minute[0];
            ml0 = s_minute[1] - m_lo + 1;
            in_lds = ml0 + bl0 + 10 <= kHist;
        }
        double v[kK2];
#pragma unroll
        for (int k = 0; k < kK2; ++k) v[k] = 0.0;
        if (x.live) {
            const int c = pos_cell[x.p];
#pragma unroll
            for (int q = 0; q < kQ; ++q) {
                const double d = S[q * M + x.p] - stats[(size_t(c) * kQ + q) * 4];
                v[q] = d * d;
            }
            const double soa = S[kColSoa * M + x.p];
            const double* rp = rxp + size_t(cell_rxi[c]) * 3;
            const double u = (soa - rp[0]) / rp[2], w = ts - rp[1];
            v[9] = u;
            v[10] = u * u;
            v[11] = w;
            v[12] = u * w;
            // histograms: 0 <= minute < the cell's minute count and 0 <= bin - first < blen[c] (its own extremes)
            const long long bin = (long long)S[3 * M + x.p] - bin_first[c];
            const int ob = flags[c] ? -1 : offset_bin(S[8 * M + x.p], edges + size_t(c) * 11);
            if (in_lds) {
                atomicAdd(&hist[minute - m_lo], 1u);
                atomicAdd(&hist[ml0 + bin], 1u);
                if (ob >= 0) atomicAdd(&hist[ml0 + bl0 + ob], 1u);
            } else {
                atomicAdd(&minute_hist[minute_ptr[c] + minute], 1ull);
                atomicAdd(&bin_hist[bin_ptr[c] + bin], 1ull);
                if (ob >= 0) atomicAdd(&offset_hist[size_t(c) * 10 + ob], 1ull);
            }
        }
        if (in_lds) {
            __syncthreads();
            const int total = int(ml0 + bl0) + 10;
            for (int i = t; i < total; i += kBlock) {
                const unsigned cnt = hist[i];
                if (cnt == 0u) continue;
                if (i < ml0)
                    atomicAdd(&minute_hist[minute_ptr[c0] + m_lo + i], (unsigned long long)cnt);
                else if (i < ml0 + bl0)
                    atomicAdd(&bin_hist[bin_ptr[c0] + (i - ml0)], (unsigned long long)cnt);
                else
                    atomicAdd(&offset_hist[size_t(c0) * 10 + (i - ml0 - bl0)], (unsigned long long)cnt);
            }
        }
        seg_scan<kK2, kK2, 0>(v, t, x.seg, lds);  // ends in a barrier: the counters are free again
        if (x.live && x.p + 1 == x.fend) {
#pragma unroll
            for (int k = 0; k < kK2; ++k) slab[size_t(x.f) * kK2 + k] = v[k];
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_fin_cells(const double* __restrict__ cv2, const long long* __restrict__ cell_ptr,
                                                      int nc, double* __restrict__ stats) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nc * kQ) return;
    const int c = i / kQ, q = i % kQ;
    const double count = double(cell_ptr[c + 1] - cell_ptr[c]);
    stats[(size_t(c) * kQ + q) * 4 + 1] = sqrt(cv2[size_t(c) * kK2 + q] / count);
}
// the line in u against v = timestamp - mean: normal equations of size two; line[r] = {c0, c1}
__global__ __launch_bounds__(kBlock) void k_fit_rx(const double* __restrict__ rv2, const long long* __restrict__ rx_count,
                                                   const double* __restrict__ rxp, int nr, double* __restrict__ line,
                                                   double* __restrict__ rx_fit) {
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= nr) return;
    const double* v = rv2 + size_t(r) * kK2;
    const double n = double(rx_count[r]), s1 = v[9], s2 = v[10], t0 = v[11], t1 = v[12];
    const double mean_soa = rxp[size_t(r) * 3], mean_ts = rxp[size_t(r) * 3 + 1], scale = rxp[size_t(r) * 3 + 2];
    const double det = n * s2 - s1 * s1;
    double c1 = (n * t1 - s1 * t0) / det;
    double c0 = (t0 - c1 * s1) / n;
    if (scale != scale) c0 = c1 = NAN;
    line[size_t(r) * 2] = c0;
    line[size_t(r) * 2 + 1] = c1;
    const double a = c1 / scale;
    rx_fit[size_t(r) * 4] = a;
    rx_fit[size_t(r) * 4 + 1] = (mean_ts + c0) - a * mean_soa;
}

// pass 3: the residual of a position, scattered to selection order; its square and its magnitude (the slots of kK3)
struct LoadPass3 {
    const double* S;
    size_t M;
    const int *pos_cell, *cell_rxi;
    const double *rxp, *line;
    const unsigned* perm;
    double* residual;
    __device__ void operator()(int p, double (&v)[kK3]) const {
        const int r = cell_rxi[pos_cell[p]];
        const double* rp = rxp + size_t(r) * 3;
        const double u = (S[kColSoa * M + p] - rp[0]) / rp[2], w = S[kColTs * M + p] - rp[1];
        const double res = (line[size_t(r) * 2] + line[size_t(r) * 2 + 1] * u) - w;  // a * soa + b - timestamp
        residual[perm[p]] = res;
        v[0] = res * res;
        v[1] = fabs(res);
    }
};
__global__ __launch_bounds__(kBlock) void k_fin_rx(const double* __restrict__ rv3, const long long* __restrict__ rx_count,
                                                   int nr, double* __restrict__ rx_fit) {
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= nr) return;
    rx_fit[size_t(r) * 4 + 2] = sqrt(rv3[size_t(r) * kK3] / double(rx_count[r]));
    rx_fit[size_t(r) * 4 + 3] = rv3[size_t(r) * kK3 + 1];
}

// last thr_toadstats of this thread: copies in, sort and cells, reductions and histograms, fit, copies out
thread_local double g_times_ms[5] = {0, 0, 0, 0, 0};

}  // namespace

struct thr_tstats : thr::seg::Result {};

namespace {

// sums cells' fragments, then receivers' cells
int combine2(const double* slab, const int* cell_frag, int nc, const int* rx_cell, int nr, int K, int n_sum, int n_min,
             double* cv, double* rv, hipStream_t s) {
    THR_TRY(launch_combine(slab, cell_frag, cell_frag + 1, 1, nc, K, n_sum, n_min, cv, s));
    return launch_combine(cv, rx_cell, rx_cell + 1, 1, nr, K, n_sum, n_min, rv, s);
}

}  // namespace

extern "C" int thr_toadstats(int device_id, size_t n, const int32_t* rxid, const int32_t* txid,
                             const int32_t* carrier_bin, const double* timestamp, const double* soa,
                             const double* carrier_offset, const double* carrier_energy, const double* carrier_noise,
                             const double* energy, const double* noise, const double* offset, const int64_t* sel,
                             size_t n_sel, thr_tstats** result_out, thr_tstats_counts* counts_out) try {
    if (result_out) *result_out = nullptr;
    if (counts_out) std::memset(counts_out, 0, sizeof(*counts_out));
    for (double& t : g_times_ms) t = 0;
    if (!result_out || !counts_out) return thr::fail_msg(THR_ERR_ARG, "thr_toadstats: null argument");
    if (n && (!rxid || !txid || !carrier_bin || !timestamp || !soa || !carrier_offset || !carrier_energy ||
              !carrier_noise || !energy || !noise || !offset))
        return thr::fail_msg(THR_ERR_ARG, "thr_toadstats: null argument");
    // ---- the host pass: the selection, the timestamps, time0
    const size_t rows = sel ? n_sel : n;
    if (rows == 0) return thr::fail_msg(THR_ERR_ARG, "thr_toadstats: the selection is empty");
    if (rows > size_t(1) << 28) return thr::fail_msg(THR_ERR_ARG, "thr_toadstats: too many detections");
    if (sel)
        for (size_t j = 0; j < rows; ++j) {
            if (sel[j] < 0 || uint64_t(sel[j]) >= n)
                return thr::fail_msg(THR_ERR_ARG, "thr_toadstats: sel[%zu] = %lld is out of range (%zu detections)", j,
                                     (long long)sel[j], n);
            if (j > 0 && sel[j] <= sel[j - 1])
                return thr::fail_msg(THR_ERR_ARG, "thr_toadstats: sel must be strictly ascending (sel[%zu])", j);
        }
    double time0 = INFINITY, t_max = -INFINITY;
    for (size_t j = 0; j < rows; ++j) {
        const size_t row = sel ? size_t(sel[j]) : j;
        const double t = timestamp[row];
        if (!std::isfinite(t))
            return thr::fail_msg(THR_ERR_ARG, "thr_toadstats: the timestamp of detection %zu is not finite", row);
        time0 = t < time0 ? t : time0;
        t_max = t > t_max ? t : t_max;
    }
    if (!(std::floor((t_max - time0) / 60.0) + 1.0 <= double(kMaxBins)))
        return thr::fail_msg(THR_ERR_ARG, "thr_toadstats: the histograms would exceed 2^26 bins (timestamps span %g s)",
                             t_max - time0);

    THR_TRY(pick_device(device_id));
    thr_tstats* R = new thr_tstats;
    ResultGuard guard{R};
    R->device = device_id;
    R->n_out = THR_TSTATS_N_OUTPUTS;
    hipStream_t s = nullptr;
    Event ev[5];
    for (Event& e : ev) THR_HIP_TRY(e.create());
    for (Event& e : R->ev) THR_HIP_TRY(e.create());
    const int m = int(rows);

    // ---- copies in
    DevBuf d_i32[3], d_f64[8], d_sel;
    const int32_t* h_i32[3] = {rxid, txid, carrier_bin};
    const double* h_f64[8] = {timestamp, soa, carrier_offset, carrier_energy, carrier_noise, energy, noise, offset};
    for (DevBuf& b : d_i32) THR_HIP_TRY(b.alloc(n * 4));
    for (DevBuf& b : d_f64) THR_HIP_TRY(b.alloc(n * 8));
    if (sel) THR_HIP_TRY(d_sel.alloc(rows * 8));
    THR_HIP_TRY(hipEventRecord(ev[0].e, s));
    for (int k = 0; k < 3; ++k) THR_HIP_TRY(hipMemcpy(d_i32[k].p, h_i32[k], n * 4, hipMemcpyHostToDevice));
    for (int k = 0; k < 8; ++k) THR_HIP_TRY(hipMemcpy(d_f64[k].p, h_f64[k], n * 8, hipMemcpyHostToDevice));
    if (sel) THR_HIP_TRY(hipMemcpy(d_sel.p, sel, rows * 8, hipMemcpyHostToDevice));
    THR_HIP_TRY(hipEventRecord(ev[1].e, s));
    Cols cols;
    cols.rx = d_i32[0].as<int>();
    cols.tx = d_i32[1].as<int>();
    cols.bin = d_i32[2].as<int>();
    cols.ts = d_f64[0].as<double>();
    cols.soa = d_f64[1].as<double>();
    cols.coff = d_f64[2].as<double>();
    cols.ce = d_f64[3].as<double>();
    cols.cn = d_f64[4].as<double>();
    cols.en = d_f64[5].as<double>();
    cols.no = d_f64[6].as<double>();
    cols.off = d_f64[7].as<double>();
    cols.sel = sel ? d_sel.as<long long>() : nullptr;

    // ---- 1. sort and cells
    DevBuf d_ka, d_kb, d_ia, d_perm, d_trip, d_tincl, d_tmp;
    size_t tmp_bytes = 0;
    THR_HIP_TRY(d_ka.alloc(size_t(m) * 8));
    THR_HIP_TRY(d_kb.alloc(size_t(m) * 8));
    THR_HIP_TRY(d_ia.alloc(size_t(m) * 4));
    THR_HIP_TRY(d_perm.alloc(size_t(m) * 4));
    THR_HIP_TRY(d_trip.alloc(size_t(m) * sizeof(Trip)));
    THR_HIP_TRY(d_tincl.alloc(size_t(m) * sizeof(Trip)));
    unsigned long long* keys = d_kb.as<unsigned long long>();
    unsigned* perm = d_perm.as<unsigned>();
    THR_TRY(launch(k_keys, m, s, cols, m, d_ka.as<unsigned long long>(), d_ia.as<unsigned>()));
    THR_HIP_TRY(with_temp(d_tmp, tmp_bytes, [&](void* t, size_t& b) {
        return hipcub::DeviceRadixSort::SortPairs(t, b, d_ka.as<unsigned long long>(), keys, d_ia.as<unsigned>(), perm, m,
                                                  0, 64, s);
    }));
    THR_TRY(launch(k_heads, m, s, keys, m, d_trip.as<Trip>()));
    THR_HIP_TRY(with_temp(d_tmp, tmp_bytes, [&](void* t, size_t& b) {
        return hipcub::DeviceScan::InclusiveScan(t, b, d_trip.as<Trip>(), d_tincl.as<Trip>(), TripSum(), m, s);
    }));
    Trip total;
    THR_HIP_TRY(hipMemcpy(&total, d_tincl.as<Trip>() + (m - 1), sizeof(Trip), hipMemcpyDeviceToHost));
    const int nc = int(total.c), nf = int(total.f), nr = int(total.r);
    const int n_tiles = tiles_of(m);

    DevBuf* O = R->out;
    DevBuf d_cell_frag, d_cell_rxi, d_rx_cell, d_rx_ptr, d_frag_start, d_pos_frag, d_pos_cell, d_S;
    THR_HIP_TRY(O[THR_TSTATS_CELL_RX].alloc(size_t(nc) * 4));
    THR_HIP_TRY(O[THR_TSTATS_CELL_TX].alloc(size_t(nc) * 4));
    THR_HIP_TRY(O[THR_TSTATS_CELL_PTR].alloc((size_t(nc) + 1) * 8));
    THR_HIP_TRY(O[THR_TSTATS_ORDER].alloc(size_t(m) * 8));
    THR_HIP_TRY(O[THR_TSTATS_SNR_DB].alloc(size_t(m) * 16));
    THR_HIP_TRY(O[THR_TSTATS_RX_ID].alloc(size_t(nr) * 4));
    THR_HIP_TRY(d_cell_frag.alloc((size_t(nc) + 1) * 4));
    THR_HIP_TRY(d_cell_rxi.alloc(size_t(nc) * 4));
    THR_HIP_TRY(d_rx_cell.alloc((size_t(nr) + 1) * 4));
    THR_HIP_TRY(d_rx_ptr.alloc((size_t(nr) + 1) * 4));
    THR_HIP_TRY(d_frag_start.alloc((size_t(nf) + 1) * 4));
    THR_HIP_TRY(d_pos_frag.alloc(size_t(m) * 4));
    THR_HIP_TRY(d_pos_cell.alloc(size_t(m) * 4));
    THR_HIP_TRY(d_S.alloc(size_t(m) * kCols * 8));
    const long long* cell_ptr = O[THR_TSTATS_CELL_PTR].as<long long>();
    const int *cell_frag = d_cell_frag.as<int>(), *cell_rxi = d_cell_rxi.as<int>(), *rx_cell = d_rx_cell.as<int>();
    const int *rx_ptr = d_rx_ptr.as<int>(), *frag_start = d_frag_start.as<int>();
    const int *pos_frag = d_pos_frag.as<int>(), *pos_cell = d_pos_cell.as<int>();
    const double* S = d_S.as<double>();
    THR_TRY(launch(k_layout, m, s, keys, d_tincl.as<Trip>(), m, nc, nf, nr, O[THR_TSTATS_CELL_PTR].as<long long>(),
                   O[THR_TSTATS_CELL_RX].as<int>(), O[THR_TSTATS_CELL_TX].as<int>(), d_cell_frag.as<int>(), d_cell_rxi.as<int>(),
                   d_rx_cell.as<int>(), O[THR_TSTATS_RX_ID].as<int>(), d_rx_ptr.as<int>(), d_frag_start.as<int>(),
                   d_pos_frag.as<int>(), d_pos_cell.as<int>()));
    THR_TRY(launch(k_gather, m, s, cols, perm, m, time0, d_S.as<double>(), O[THR_TSTATS_ORDER].as<long long>(),
                   O[THR_TSTATS_SNR_DB].as<double>()));
    THR_HIP_TRY(hipEventRecord(ev[2].e, s));

    // ---- 2. pass 1 and what follows from it
    DevBuf d_slab, d_cv, d_rv, d_rxp, d_mlen, d_blen;
    THR_HIP_TRY(d_slab.alloc(size_t(nf) * kK1 * 8));
    THR_HIP_TRY(d_cv.alloc(size_t(nc) * kK1 * 8));
    THR_HIP_TRY(d_rv.alloc(size_t(nr) * kK1 * 8));
    THR_HIP_TRY(d_rxp.alloc(size_t(nr) * 3 * 8));
    THR_HIP_TRY(d_mlen.alloc(size_t(nc) * 8));
    THR_HIP_TRY(d_blen.alloc(size_t(nc) * 8));
    THR_HIP_TRY(O[THR_TSTATS_STATS].alloc(size_t(nc) * kQ * 4 * 8));
    THR_HIP_TRY(O[THR_TSTATS_MINUTE_PTR].alloc((size_t(nc) + 1) * 8));
    THR_HIP_TRY(O[THR_TSTATS_BIN_PTR].alloc((size_t(nc) + 1) * 8));
    THR_HIP_TRY(O[THR_TSTATS_BIN_FIRST].alloc(size_t(nc) * 4));
    THR_HIP_TRY(O[THR_TSTATS_OFFSET_EDGES].alloc(size_t(nc) * 11 * 8));
    THR_HIP_TRY(O[THR_TSTATS_OFFSET_HIST].alloc(size_t(nc) * 10 * 8));
    THR_HIP_TRY(O[THR_TSTATS_CELL_FLAGS].alloc(size_t(nc) * 4));
    THR_HIP_TRY(O[THR_TSTATS_RX_COUNT].alloc(size_t(nr) * 8));
    THR_HIP_TRY(O[THR_TSTATS_RX_FIT].alloc(size_t(nr) * 4 * 8));
    THR_HIP_TRY(O[THR_TSTATS_RESIDUAL].alloc(size_t(m) * 8));
    double* stats = O[THR_TSTATS_STATS].as<double>();
    long long *minute_ptr = O[THR_TSTATS_MINUTE_PTR].as<long long>(), *bin_ptr = O[THR_TSTATS_BIN_PTR].as<long long>();
    THR_TRY((launch_reduce<kK1, kS1, kM1>(LoadPass1{S, size_t(m)}, m, pos_frag, frag_start, d_slab.as<double>(), s)));
    THR_TRY(combine2(d_slab.as<double>(), cell_frag, nc, rx_cell, nr, kK1, kS1, kM1, d_cv.as<double>(), d_rv.as<double>(), s));
    THR_TRY(launch(k_mid_cells, nc, s, d_cv.as<double>(), cell_ptr, nc, stats, d_mlen.as<long long>(), d_blen.as<long long>(),
                   O[THR_TSTATS_BIN_FIRST].as<int>(), O[THR_TSTATS_OFFSET_EDGES].as<double>(), O[THR_TSTATS_CELL_FLAGS].as<int>()));
    THR_TRY(launch(k_mid_rx, nr, s, d_rv.as<double>(), rx_ptr, nr, d_rxp.as<double>(), O[THR_TSTATS_RX_COUNT].as<long long>()));
    THR_HIP_TRY(hipMemsetAsync(minute_ptr, 0, 8, s));
    THR_HIP_TRY(hipMemsetAsync(bin_ptr, 0, 8, s));
    THR_HIP_TRY(with_temp(d_tmp, tmp_bytes, [&](void* t, size_t& b) {
        return hipcub::DeviceScan::InclusiveSum(t, b, d_mlen.as<long long>(), minute_ptr + 1, nc, s);
    }));
    THR_HIP_TRY(with_temp(d_tmp, tmp_bytes, [&](void* t, size_t& b) {
        return hipcub::DeviceScan::InclusiveSum(t, b, d_blen.as<long long>(), bin_ptr + 1, nc, s);
    }));
    long long n_minute = 0, n_bin = 0;
    THR_HIP_TRY(hipMemcpy(&n_minute, minute_ptr + nc, 8, hipMemcpyDeviceToHost));
    THR_HIP_TRY(hipMemcpy(&n_bin, bin_ptr + nc, 8, hipMemcpyDeviceToHost));
    if (n_minute + n_bin + 10ll * nc > kMaxBins)
        return thr::fail_msg(THR_ERR_ARG,
                             "thr_toadstats: the histograms would exceed 2^26 bins (%lld minutes, %lld carrier bins, "
                             "%d cells)", n_minute, n_bin, nc);

    // ---- pass 2: deviations, moments, histograms
    THR_HIP_TRY(O[THR_TSTATS_MINUTE_HIST].alloc(size_t(n_minute) * 8));
    THR_HIP_TRY(O[THR_TSTATS_BIN_HIST].alloc(size_t(n_bin) * 8));
    THR_HIP_TRY(hipMemsetAsync(O[THR_TSTATS_MINUTE_HIST].p, 0, size_t(n_minute) * 8, s));
    THR_HIP_TRY(hipMemsetAsync(O[THR_TSTATS_BIN_HIST].p, 0, size_t(n_bin) * 8, s));
    THR_HIP_TRY(hipMemsetAsync(O[THR_TSTATS_OFFSET_HIST].p, 0, size_t(nc) * 10 * 8, s));
    THR_TRY(launch_grid(k_pass2, tile_grid(n_tiles), s, S, m, n_tiles, pos_frag, frag_start, pos_cell, stats, cell_rxi,
                        d_rxp.as<double>(), d_blen.as<long long>(), O[THR_TSTATS_BIN_FIRST].as<int>(),
                        O[THR_TSTATS_OFFSET_EDGES].as<double>(), O[THR_TSTATS_CELL_FLAGS].as<int>(), minute_ptr, bin_ptr,
                        O[THR_TSTATS_MINUTE_HIST].as<unsigned long long>(), O[THR_TSTATS_BIN_HIST].as<unsigned long long>(),
                        O[THR_TSTATS_OFFSET_HIST].as<unsigned long long>(), d_slab.as<double>()));
    THR_TRY(combine2(d_slab.as<double>(), cell_frag, nc, rx_cell, nr, kK2, kK2, 0, d_cv.as<double>(), d_rv.as<double>(), s));
    THR_TRY(launch(k_fin_cells, size_t(nc) * kQ, s, d_cv.as<double>(), cell_ptr, nc, stats));
    THR_HIP_TRY(hipEventRecord(ev[3].e, s));

    // ---- 3. the line, the residuals
    DevBuf d_line;
    THR_HIP_TRY(d_line.alloc(size_t(nr) * 2 * 8));
    THR_TRY(launch(k_fit_rx, nr, s, d_rv.as<double>(), O[THR_TSTATS_RX_COUNT].as<long long>(), d_rxp.as<double>(), nr,
                   d_line.as<double>(), O[THR_TSTATS_RX_FIT].as<double>()));
    THR_TRY((launch_reduce<kK3, 1, 0>(LoadPass3{S, size_t(m), pos_cell, cell_rxi, d_rxp.as<double>(), d_line.as<double>(), perm,
                                                O[THR_TSTATS_RESIDUAL].as<double>()},
                                      m, pos_frag, frag_start, d_slab.as<double>(), s)));
    THR_TRY(combine2(d_slab.as<double>(), cell_frag, nc, rx_cell, nr, kK3, 1, 0, d_cv.as<double>(), d_rv.as<double>(), s));
    THR_TRY(launch(k_fin_rx, nr, s, d_rv.as<double>(), O[THR_TSTATS_RX_COUNT].as<long long>(), nr, O[THR_TSTATS_RX_FIT].as<double>()));
    THR_HIP_TRY(hipEventRecord(ev[4].e, s));
    THR_TRY(record_times(ev, g_times_ms));  // synchronises: the temporaries go out of scope

    size_t* B = R->bytes;
    B[THR_TSTATS_CELL_RX] = B[THR_TSTATS_CELL_TX] = B[THR_TSTATS_BIN_FIRST] = B[THR_TSTATS_CELL_FLAGS] = size_t(nc) * 4;
    B[THR_TSTATS_CELL_PTR] = B[THR_TSTATS_MINUTE_PTR] = B[THR_TSTATS_BIN_PTR] = (size_t(nc) + 1) * 8;
    B[THR_TSTATS_ORDER] = B[THR_TSTATS_RESIDUAL] = size_t(m) * 8;
    B[THR_TSTATS_STATS] = size_t(nc) * kQ * 4 * 8;
    B[THR_TSTATS_SNR_DB] = size_t(m) * 16;
    B[THR_TSTATS_MINUTE_HIST] = size_t(n_minute) * 8;
    B[THR_TSTATS_BIN_HIST] = size_t(n_bin) * 8;
    B[THR_TSTATS_OFFSET_EDGES] = size_t(nc) * 11 * 8;
    B[THR_TSTATS_OFFSET_HIST] = size_t(nc) * 10 * 8;
    B[THR_TSTATS_RX_ID] = size_t(nr) * 4;
    B[THR_TSTATS_RX_COUNT] = size_t(nr) * 8;
    B[THR_TSTATS_RX_FIT] = size_t(nr) * 4 * 8;
    counts_out->rows = rows;
    counts_out->cells = size_t(nc);
    counts_out->receivers = size_t(nr);
    counts_out->minute_bins = size_t(n_minute);
    counts_out->carrier_bins = size_t(n_bin);
    counts_out->offset_bins = size_t(nc) * 10;
    counts_out->time0 = time0;
    *result_out = R;
    guard.r = nullptr;
    return THR_OK;
} catch (const std::bad_alloc&) {
    return thr::fail_msg(THR_ERR_DEVICE, "thr_toadstats: out of host memory");
} catch (...) {
    return thr::on_exception("thr_toadstats");
}

extern "C" int thr_tstats_fetch(thr_tstats* R, int which, void* dst, size_t dst_bytes) try {
    return fetch("thr_tstats_fetch", R, which, dst, dst_bytes, &g_times_ms[4]);
} catch (...) {
    return thr::on_exception("thr_tstats_fetch");
}

extern "C" void thr_tstats_free(thr_tstats* R) { free_result(R); }

extern "C" int thr_debug_toadstats_times(double* ms_out) try {
    return copy_times("thr_debug_toadstats_times", g_times_ms, ms_out);
} catch (...) {
    return thr::on_exception("thr_debug_toadstats_times");
}

extern "C" int thr_debug_toadstats_geometry(int* tile_len, int* workgroup) try {
    return geometry("thr_debug_toadstats_geometry", tile_len, workgroup);
} catch (...) {
    return thr::on_exception("thr_debug_toadstats_geometry");
}

// ---- the tile grid of every stage built on seg_reduce.hpp: the cap on a tile kernel's workgroups, set by tests through
// thr_debug_seg_tile_grid, and what the grids sized since then looked like.  Process-wide; no result depends on it.
namespace {
std::atomic<int> g_tile_grid_cap{kMaxTileGrid};
std::atomic<int> g_tile_launches{0}, g_tile_max_trips{0};
}  // namespace

dim3 thr::seg::tile_grid(int n_tiles) {
    const int cap = g_tile_grid_cap.load(std::memory_order_relaxed);
    const int grid = n_tiles < cap ? n_tiles : cap;
    if (grid > 0) {
        const int trips = (n_tiles + grid - 1) / grid;
        g_tile_launches.fetch_add(1, std::memory_order_relaxed);
        int seen = g_tile_max_trips.load(std::memory_order_relaxed);
        while (trips > seen && !g_tile_max_trips.compare_exchange_weak(seen, trips, std::memory_order_relaxed)) {
        }
    }
    return dim3(unsigned(grid));
}

extern "C" int thr_debug_seg_tile_grid(int workgroups) try {
    if (workgroups < 0 || workgroups > kTileGridLimit)
        return thr::fail_msg(THR_ERR_ARG, "thr_debug_seg_tile_grid: %d workgroups (0: the default, or 1 .. %d)", workgroups,
                             kTileGridLimit);
    g_tile_grid_cap.store(workgroups ? workgroups : kMaxTileGrid);
    g_tile_launches.store(0);
    g_tile_max_trips.store(0);
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_seg_tile_grid");
}

extern "C" int thr_debug_seg_tile_stats(int* launches, int* max_trips) try {
    if (!launches || !max_trips) return thr::fail_msg(THR_ERR_ARG, "thr_debug_seg_tile_stats: null argument");
    *launches = g_tile_launches.load();
    *max_trips = g_tile_max_trips.load();
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_seg_tile_stats");
}
