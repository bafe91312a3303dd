// Rows into cells, cells into fragments, and what a stage does with a cell's values: everything that the
// statistics stages on seg_reduce.hpp share beyond the reduction itself (syncstats.hip, reldist.hip, tdoamatrix.hip).
//   find_sorted / upload_list   an ascending id list on the device, searched by bisection;
//   scan                        an inclusive sum of flags and its total, read back;
//   build_layout / reduce       the fragments of contiguous segments (a Layout), and one reduction over them;
//   sort_cells                  two stable hipCUB radix sorts leave rows grouped by a three-part key in their
//                               first order; head flags, one scan, the cell table;
//   check_matches / pair_rows   the front end of a stage that reads matches: the host pass over them, then one
//                               row per detection pair that the stage's selector keeps, sorted into cells;
//   sort_by_cell_value          values ordered by (cell, value), for medians;
//   outlier_mask                stat_tools.is_outlier per cell: median, MAD and the mask;
//   LoadKept1 / LoadKept2       count, sum, extremes and squared deviations over the rows a mask keeps.
// Lifetimes are the including file's business (syncstats.hip describes the rule: the null stream, hipFree waits).
//
// Everything here is a template, inline, or static: both files include it.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/thrifty_hip.h"
#include "post_stages.hpp"
#include "seg_reduce.hpp"

namespace thr {
namespace seg {

using thr::with_temp;

// position of v in the ascending list, -1 when absent; n < 0: no list, every value passes (position 0)
__device__ __forceinline__ int find_sorted(const int* list, int n, int v) {
    if (n < 0) return 0;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] < v) lo = mid + 1; else hi = mid;
    }
    return (lo < n && list[lo] == v) ? lo : -1;
}

// ------------------------------------------------------------------ segments and their fragments
// seg[p]: the segment of position p, -1 for a position of none.  A segment's positions are contiguous.
static __global__ __launch_bounds__(kBlock) void k_frag_heads(const int* __restrict__ seg, int m, unsigned* __restrict__ head) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p < m) head[p] = (p % kTile == 0 || seg[p] != seg[p - 1]) ? 1u : 0u;
}
// seg_frag[s] = {first fragment, one past the last}; zeroed before: a segment without positions keeps {0, 0}
static __global__ __launch_bounds__(kBlock) void k_frag_layout(const int* __restrict__ seg, const unsigned* __restrict__ head,
                                                               const unsigned* __restrict__ incl, int m, int nf,
                                                               int* __restrict__ pos_frag, int* __restrict__ frag_start,
                                                               int* __restrict__ seg_frag) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= m) return;
    const int f = int(incl[p]) - 1, sg = seg[p];
    pos_frag[p] = f;
    if (head[p]) frag_start[f] = p;
    if (p == m - 1) frag_start[nf] = m;
    if (sg >= 0) {
        if (p == 0 || seg[p - 1] != sg) seg_frag[2 * size_t(sg)] = f;
        if (p == m - 1 || seg[p + 1] != sg) seg_frag[2 * size_t(sg) + 1] = f + 1;
    }
}

struct Layout {
    DevBuf pos_frag, frag_start, seg_frag;
    int m = 0, n_seg = 0, nf = 0;
};
struct Scratch {  // what the hipCUB calls, the layouts and sort_by_cell_value share
    DevBuf tmp, head, incl;
    size_t tmp_bytes = 0;
    DevBuf sort_ia, sort_ib, sort_va, sort_ka, sort_kb;  // sort_by_cell_value's, for sort_m positions
    int sort_m = 0;
};

// incl = the inclusive sums of the n flags, *total = the last of them (0 for none); the read-back synchronises
inline int scan(const unsigned* flag, unsigned* incl, int n, Scratch& w, hipStream_t s, unsigned* total) {
    *total = 0;
    if (n == 0) return THR_OK;
    THR_HIP_TRY(with_temp(w.tmp, w.tmp_bytes,
                          [&](void* t, size_t& b) { return hipcub::DeviceScan::InclusiveSum(t, b, flag, incl, n, s); }));
    THR_HIP_TRY(hipMemcpy(total, incl + (n - 1), 4, hipMemcpyDeviceToHost));
    return THR_OK;
}

inline int build_layout(const int* seg, int m, int n_seg, Scratch& w, Layout& L, hipStream_t s) {
    L.m = m;
    L.n_seg = n_seg;
    THR_HIP_TRY(L.pos_frag.alloc(size_t(m) * 4));
    THR_HIP_TRY(L.seg_frag.alloc(size_t(n_seg) * 8));
    THR_HIP_TRY(hipMemsetAsync(L.seg_frag.p, 0, size_t(n_seg) * 8, s));
    THR_TRY(launch(k_frag_heads, m, s, seg, m, w.head.as<unsigned>()));
    unsigned nf = 0;
    THR_TRY(scan(w.head.as<unsigned>(), w.incl.as<unsigned>(), m, w, s, &nf));
    L.nf = int(nf);
    THR_HIP_TRY(L.frag_start.alloc((size_t(nf) + 1) * 4));
    return launch(k_frag_layout, m, s, seg, w.head.as<unsigned>(), w.incl.as<unsigned>(), m, L.nf, L.pos_frag.as<int>(),
                  L.frag_start.as<int>(), L.seg_frag.as<int>());
}

// out[n_seg][K] (device) = the reduction of load() over every segment of L; slab holds nf * K doubles
template <int K, int NSUM, int NMIN, class Load>
int reduce(const Load& load, const Layout& L, double* slab, double* out, hipStream_t s) {
    THR_TRY((launch_reduce<K, NSUM, NMIN>(load, L.m, L.pos_frag.as<int>(), L.frag_start.as<int>(), slab, s)));
    const int* seg_frag = L.seg_frag.as<int>();
    return launch_combine(slab, seg_frag, seg_frag + 1, 2, L.n_seg, K, NSUM, NMIN, out, s);
}

// ------------------------------------------------------------------ sorting rows into cells
// key_hi / key_lo of row j; the rows end up ordered by (hi, lo), rows of equal keys in their first order
static __global__ __launch_bounds__(kBlock) void k_gather_u64(const unsigned long long* __restrict__ src,
                                                              const unsigned* __restrict__ perm, int m,
                                                              unsigned long long* __restrict__ dst) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p < m) dst[p] = src[perm[p]];
}
static __global__ __launch_bounds__(kBlock) void k_gather_u32(const unsigned* __restrict__ src, const unsigned* __restrict__ perm,
                                                              int m, unsigned* __restrict__ dst) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p < m) dst[p] = src[perm[p]];
}
static __global__ __launch_bounds__(kBlock) void k_cell_heads(const unsigned long long* __restrict__ hi,
                                                              const unsigned* __restrict__ lo, int m, unsigned* __restrict__ head) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p < m) head[p] = (p == 0 || hi[p] != hi[p - 1] || lo[p] != lo[p - 1]) ? 1u : 0u;
}
// per position its cell; per cell its first position and its key (hi's two halves, then lo)
static __global__ __launch_bounds__(kBlock) void k_cell_layout(const unsigned long long* __restrict__ hi,
                                                               const unsigned* __restrict__ lo, const unsigned* __restrict__ head,
                                                               const unsigned* __restrict__ incl, int m, int nc,
                                                               int* __restrict__ pos_cell, long long* __restrict__ cell_ptr,
                                                               int* __restrict__ cell_key) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= m) return;
    const int c = int(incl[p]) - 1;
    pos_cell[p] = c;
    if (head[p]) {
        cell_ptr[c] = p;
        cell_key[3 * size_t(c)] = unkey_i32(unsigned(hi[p] >> 32));
        cell_key[3 * size_t(c) + 1] = unkey_i32(unsigned(hi[p]));
        cell_key[3 * size_t(c) + 2] = unkey_i32(lo[p]);
    }
    if (p == m - 1) cell_ptr[nc] = m;
}

struct Cells {
    DevBuf perm, pos_cell;  // unsigned[m]: the row at position p; int[m]
    int nc = 0;
};
// key_hi, key_lo: unsorted keys of the m rows (read only; key_lo is read again after the second sort).  cell_ptr
// int64[nc + 1] and cell_key int32[nc][3] are allocated here, once the number of cells is known.
inline int sort_cells(DevBuf& key_hi, DevBuf& key_lo, int m, Scratch& w, Cells& out, DevBuf& cell_ptr, DevBuf& cell_key,
                      hipStream_t s) {
    DevBuf ia, ib, lo2, hi2, hi3;
    THR_HIP_TRY(ia.alloc(size_t(m) * 4));
    THR_HIP_TRY(ib.alloc(size_t(m) * 4));
    THR_HIP_TRY(lo2.alloc(size_t(m) * 4));
    THR_HIP_TRY(hi2.alloc(size_t(m) * 8));
    THR_HIP_TRY(hi3.alloc(size_t(m) * 8));
    THR_HIP_TRY(out.perm.alloc(size_t(m) * 4));
    THR_HIP_TRY(out.pos_cell.alloc(size_t(m) * 4));
    THR_TRY(launch(k_iota, m, s, ia.as<unsigned>(), m));
    THR_HIP_TRY(with_temp(w.tmp, w.tmp_bytes, [&](void* t, size_t& b) {
        return hipcub::DeviceRadixSort::SortPairs(t, b, key_lo.as<unsigned>(), lo2.as<unsigned>(), ia.as<unsigned>(),
                                                  ib.as<unsigned>(), m, 0, 32, s);
    }));
    THR_TRY(launch(k_gather_u64, m, s, key_hi.as<unsigned long long>(), ib.as<unsigned>(), m, hi2.as<unsigned long long>()));
    THR_HIP_TRY(with_temp(w.tmp, w.tmp_bytes, [&](void* t, size_t& b) {
        return hipcub::DeviceRadixSort::SortPairs(t, b, hi2.as<unsigned long long>(), hi3.as<unsigned long long>(),
                                                  ib.as<unsigned>(), out.perm.as<unsigned>(), m, 0, 64, s);
    }));
    // lo in the final order: lo2 is in the order of ib, which the second sort permuted again
    THR_TRY(launch(k_gather_u32, m, s, key_lo.as<unsigned>(), out.perm.as<unsigned>(), m, lo2.as<unsigned>()));
    THR_TRY(launch(k_cell_heads, m, s, hi3.as<unsigned long long>(), lo2.as<unsigned>(), m, w.head.as<unsigned>()));
    unsigned nc = 0;
    THR_TRY(scan(w.head.as<unsigned>(), w.incl.as<unsigned>(), m, w, s, &nc));
    out.nc = int(nc);
    THR_HIP_TRY(cell_ptr.alloc((size_t(nc) + 1) * 8));
    THR_HIP_TRY(cell_key.alloc(size_t(nc) * 12));
    return launch(k_cell_layout, m, s, hi3.as<unsigned long long>(), lo2.as<unsigned>(), w.head.as<unsigned>(),
                  w.incl.as<unsigned>(), m, out.nc, out.pos_cell.as<int>(), cell_ptr.as<long long>(), cell_key.as<int>());
}

// ------------------------------------------------------------------ matches into rows of detection pairs
// The host pass over the matches: match_ptr starts at 0 and does not decrease, every match_idx is a detection,
// no receiver appears twice in a match; *n_pairs = the pairs of detections that share a match.  No pair at all is
// an error unless the stage says that it may be (may_be_empty: it answers with an empty result).
inline int check_matches(const char* who, size_t n_det, const int32_t* rxid, size_t n_matches, const int64_t* match_ptr,
                         const int64_t* match_idx, uint64_t* n_pairs, bool may_be_empty = false) {
    if (match_ptr[0] != 0) return thr::fail_msg(THR_ERR_ARG, "%s: match_ptr[0] must be 0", who);
    uint64_t pairs = 0;
    for (size_t m = 0; m < n_matches; ++m) {
        const int64_t a = match_ptr[m], e = match_ptr[m + 1];
        if (e < a) return thr::fail_msg(THR_ERR_ARG, "%s: match_ptr decreases at match %zu", who, m);
        for (int64_t i = a; i < e; ++i) {
            const int64_t d = match_idx[i];
            if (d < 0 || uint64_t(d) >= n_det)
                return thr::fail_msg(THR_ERR_ARG, "%s: match %zu holds detection %lld of %zu", who, m, (long long)d, n_det);
            for (int64_t k = a; k < i; ++k)
                if (rxid[match_idx[k]] == rxid[d])
                    return thr::fail_msg(THR_ERR_ARG, "%s: match %zu holds two detections of one receiver (detection %lld)", who,
                                         m, (long long)d);
        }
        pairs += uint64_t(e - a) * uint64_t(e - a > 0 ? e - a - 1 : 0) / 2;
    }
    if (pairs > (uint64_t(1) << 28)) return thr::fail_msg(THR_ERR_ARG, "%s: too many detection pairs", who);
    if ((n_matches == 0 || pairs == 0) && !may_be_empty) return thr::fail_msg(THR_ERR_ARG, "%s: the selection is empty", who);
    *n_pairs = pairs;
    return THR_OK;
}

// One thread per match.  A stage's Select holds its detections (sel.d: rx, tx, mptr, midx) and decides with
// wanted(tx) which transmitters' matches give rows and with kept(da, db) which pairs of them.  check_matches has
// passed.  EMIT = false counts the match's rows, EMIT = true writes them from offset incl[i] - count[i]: the
// key is (tx, the smaller receiver | the larger one), det the two detections in that order.
template <bool EMIT, class Select>
__global__ __launch_bounds__(kBlock) void k_pairs(Select sel, int n_matches, unsigned* __restrict__ count,
                                                  const unsigned* __restrict__ incl, unsigned long long* __restrict__ key_hi,
                                                  unsigned* __restrict__ key_lo, long long* __restrict__ det,
                                                  long long* __restrict__ match) {
    const auto& d = sel.d;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_matches) return;
    const long long a0 = d.mptr[i], a1 = d.mptr[i + 1];
    unsigned n = 0, at = 0;
    if (EMIT) at = incl[i] - count[i];
    const int tx = a1 > a0 ? d.tx[d.midx[a0]] : 0;
    if (a1 > a0 && sel.wanted(tx)) {
        for (long long a = a0; a < a1; ++a)
            for (long long b = a + 1; b < a1; ++b) {
                long long da = d.midx[a], db = d.midx[b];
                if (!sel.kept(da, db)) continue;
                if (EMIT) {
                    if (d.rx[db] < d.rx[da]) {
                        const long long t = da;
                        da = db;
                        db = t;
                    }
                    const size_t j = size_t(at) + n;
                    key_hi[j] = ((unsigned long long)key_i32(tx) << 32) | key_i32(d.rx[da]);
                    key_lo[j] = key_i32(d.rx[db]);
                    det[2 * j] = da;
                    det[2 * j + 1] = db;
                    match[j] = i;
                }
                ++n;
            }
    }
    if (!EMIT) count[i] = n;
}

struct PairRows {
    int m = 0;          // rows; nothing else is filled when there are none (the caller words that error)
    DevBuf det, match;  // long long[m][2], long long[m], in the order the rows were emitted
    Cells cells;        // cells.perm[p]: the emitted row at position p
    DevBuf cnt, cincl, key_hi, key_lo;  // the front end's own; they live as long as the rows, so that no hipFree
                                        // waits for the device in the middle of the stage
};
// count, scan, emit, sort: the rows of every match that sel keeps, grouped into cells.  w.head and w.incl are
// allocated for the rows.
template <class Select>
int pair_rows(const Select& sel, int n_matches, Scratch& w, PairRows& out, DevBuf& cell_ptr, DevBuf& cell_key, hipStream_t s) {
    DevBuf &cnt = out.cnt, &cincl = out.cincl, &khi = out.key_hi, &klo = out.key_lo;
    THR_HIP_TRY(cnt.alloc(size_t(n_matches) * 4));
    THR_HIP_TRY(cincl.alloc(size_t(n_matches) * 4));
    THR_TRY(launch(k_pairs<false, Select>, n_matches, s, sel, n_matches, cnt.as<unsigned>(), nullptr, nullptr, nullptr, nullptr,
                   nullptr));
    unsigned n_rows = 0;
    THR_TRY(scan(cnt.as<unsigned>(), cincl.as<unsigned>(), n_matches, w, s, &n_rows));
    out.m = int(n_rows);
    if (n_rows == 0) return THR_OK;
    const size_t m = n_rows;
    THR_HIP_TRY(khi.alloc(m * 8));
    THR_HIP_TRY(klo.alloc(m * 4));
    THR_HIP_TRY(out.det.alloc(m * 16));
    THR_HIP_TRY(out.match.alloc(m * 8));
    THR_HIP_TRY(w.head.alloc(m * 4));
    THR_HIP_TRY(w.incl.alloc(m * 4));
    THR_TRY(launch(k_pairs<true, Select>, n_matches, s, sel, n_matches, cnt.as<unsigned>(), cincl.as<unsigned>(),
                   khi.as<unsigned long long>(), klo.as<unsigned>(), out.det.as<long long>(), out.match.as<long long>()));
    return sort_cells(khi, klo, out.m, w, out.cells, cell_ptr, cell_key, s);
}

// ------------------------------------------------------------------ values by (cell, value)
static __global__ __launch_bounds__(kBlock) void k_gather_cell(const int* __restrict__ pos_cell, const unsigned* __restrict__ pos,
                                                               int m, unsigned* __restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < m) out[i] = unsigned(pos_cell[pos[i]]);
}

// values (position order) -> the same values ordered by (cell, value): a sort by value, then a stable sort
// by the cell of the position each value came from.  `out` is allocated on first use and reused after
// (the stream orders a later sort behind the kernels that read the earlier result).
inline int sort_by_cell_value(const double* vals, const int* pos_cell, int m, int nc, Scratch& w, DevBuf& out, hipStream_t s) {
    if (w.sort_m < m) {
        THR_HIP_TRY(w.sort_ia.alloc(size_t(m) * 4));
        THR_HIP_TRY(w.sort_ib.alloc(size_t(m) * 4));
        THR_HIP_TRY(w.sort_va.alloc(size_t(m) * 8));
        THR_HIP_TRY(w.sort_ka.alloc(size_t(m) * 4));
        THR_HIP_TRY(w.sort_kb.alloc(size_t(m) * 4));
        w.sort_m = m;
    }
    if (!out.p) THR_HIP_TRY(out.alloc(size_t(m) * 8));
    unsigned *ia = w.sort_ia.as<unsigned>(), *ib = w.sort_ib.as<unsigned>();
    unsigned *ka = w.sort_ka.as<unsigned>(), *kb = w.sort_kb.as<unsigned>();
    double* va = w.sort_va.as<double>();
    THR_TRY(launch(k_iota, m, s, ia, m));
    THR_HIP_TRY(with_temp(w.tmp, w.tmp_bytes, [&](void* t, size_t& b) {
        return hipcub::DeviceRadixSort::SortPairs(t, b, vals, va, ia, ib, m, 0, 64, s);
    }));
    THR_TRY(launch(k_gather_cell, m, s, pos_cell, ib, m, ka));
    int bits = 1;
    while (bits < 32 && (1ll << bits) < nc) ++bits;
    THR_HIP_TRY(with_temp(w.tmp, w.tmp_bytes, [&](void* t, size_t& b) {
        return hipcub::DeviceRadixSort::SortPairs(t, b, ka, kb, va, out.as<double>(), m, 0, bits, s);
    }));
    return THR_OK;
}

// ------------------------------------------------------------------ stat_tools.is_outlier per cell
// the median of each cell from its values in ascending order: the mean of the two middle ones (the same one
// twice for an odd count); NaN when the cell holds a NaN (probe: its max, which a NaN wins) or nothing
static __global__ __launch_bounds__(kBlock) void k_median(const double* __restrict__ sorted, const long long* __restrict__ ptr,
                                                          const double* __restrict__ probe, int probe_stride, int nc,
                                                          double* __restrict__ out, int out_stride) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= nc) return;
    const long long a = ptr[c], n = ptr[c + 1] - a;
    const double pr = probe[size_t(c) * probe_stride];
    double med = NAN;
    if (n > 0 && pr == pr) med = (sorted[a + (n - 1) / 2] + sorted[a + n / 2]) / 2.0;
    out[size_t(c) * out_stride] = med;
}
// numpy: diff = sqrt(sum((points - median)**2, axis=-1)), one column
static __global__ __launch_bounds__(kBlock) void k_dev(const double* __restrict__ v, const int* __restrict__ pos_cell,
                                                       const double* __restrict__ med, int stride, int n, double* __restrict__ dev) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const double d = v[p] - med[size_t(pos_cell[p]) * stride];
    dev[p] = sqrt(d * d);
}
// numpy: 0.6745 * diff / med_abs_deviation > thresh.  A cell of one row needs no case of its own: its deviation
// is 0 (NaN for a value that is not finite) and its MAD is that same number, so z is 0 / 0 or NaN and no
// threshold is exceeded -- which is what the reference's branch for len(points) <= 1 returns as well.
static __global__ __launch_bounds__(kBlock) void k_mask(const double* __restrict__ dev, const int* __restrict__ pos_cell,
                                                        const double* __restrict__ mad, int stride, double thresh, int n,
                                                        unsigned char* __restrict__ mask) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const double z = (0.6745 * dev[p]) / mad[size_t(pos_cell[p]) * stride];
    mask[p] = z > thresh ? 1 : 0;
}
static __global__ __launch_bounds__(kBlock) void k_fill_nan(double* __restrict__ out, int stride, int n) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c < n) out[size_t(c) * stride] = out[size_t(c) * stride + 1] = NAN;
}

struct Series {  // n positions in nc cells: per position its cell, the cells' CSR, the fragments
    int n = 0, nc = 0;
    const int* pos_cell = nullptr;
    const long long* ptr = nullptr;
    Layout L;
};
struct Work {
    Scratch& w;          // the stage's
    DevBuf sorted, dev;  // dev: allocated by the stage for its largest series; sorted: on first use
};
// med[c * stride], med[c * stride + 1] = median, MAD of the cell's values; mask[p] = is_outlier.  probe[c *
// probe_stride] is a NaN when cell c holds one -- the cell's maximum, which the stage has at hand or reduces
// for this (it is not read for an empty series).
inline int outlier_mask(const double* vals, const Series& S, const double* probe, int probe_stride, double thresh, Work& k,
                        double* med, int stride, unsigned char* mask, hipStream_t s) {
    if (S.n == 0) return launch(k_fill_nan, S.nc, s, med, stride, S.nc);
    for (int pass = 0; pass < 2; ++pass) {
        const double* v = pass ? k.dev.as<double>() : vals;
        THR_TRY(sort_by_cell_value(v, S.pos_cell, S.n, S.nc, k.w, k.sorted, s));
        THR_TRY(launch(k_median, S.nc, s, k.sorted.as<double>(), S.ptr, probe, probe_stride, S.nc, med + pass, stride));
        if (pass == 0) THR_TRY(launch(k_dev, S.n, s, vals, S.pos_cell, med, stride, S.n, k.dev.as<double>()));
    }
    return launch(k_mask, S.n, s, k.dev.as<double>(), S.pos_cell, med + 1, stride, thresh, S.n, mask);
}

// Two passes over the rows a mask keeps.  SQ: whether the sum of squares is carried (K = 5 then, else 4).
template <bool SQ>
struct LoadKept1 {  // count, sum of x, [sum of x^2,] min, max
    static constexpr int K = SQ ? 5 : 4;
    const double* x;
    const unsigned char* mask;
    __device__ void operator()(int p, double (&v)[K]) const {
        v[K - 2] = INFINITY;
        v[K - 1] = -INFINITY;
        if (mask[p]) return;
        const double a = x[p];
        v[0] = 1.0;
        v[1] = a;
        if (SQ) v[2] = a * a;
        v[K - 2] = a;
        v[K - 1] = a;
    }
};
template <bool SQ>
struct LoadKept2 {  // (x - mean)^2; cv: LoadKept1<SQ>'s values per cell
    const double *x, *cv;
    const unsigned char* mask;
    const int* pos_cell;
    __device__ void operator()(int p, double (&v)[1]) const {
        if (mask[p]) return;
        const double* c = cv + LoadKept1<SQ>::K * size_t(pos_cell[p]);
        const double d = x[p] - c[1] / c[0];
        v[0] = d * d;
    }
};

// an ascending copy of a list without repeats, on the device; n_out = -1 when there is no list
inline int upload_list(const int32_t* list, size_t n, DevBuf& d, int& n_out) {
    n_out = -1;
    if (!list) return THR_OK;
    std::vector<int32_t> v(list, list + n);
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    n_out = int(v.size());
    THR_HIP_TRY(d.alloc(v.size() * 4));
    if (!v.empty()) THR_HIP_TRY(hipMemcpy(d.p, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    return THR_OK;
}

}  // namespace seg
}  // namespace thr
