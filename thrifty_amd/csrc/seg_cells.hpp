// Rows into cells, cells into fragments: the builders that the statistics stages on seg_reduce.hpp share
// (syncstats.hip, reldist.hip).  Moved here from syncstats.hip as they stood when a second file needed them:
//   find_sorted / upload_list   an ascending id list on the device, searched by bisection;
//   build_layout / reduce       the fragments of contiguous segments (a Layout), and one reduction over them;
//   sort_cells                  two stable hipCUB radix sorts leave rows grouped by a three-part key in their
//                               first order; head flags, one scan, the cell table;
//   sort_by_cell_value          values ordered by (cell, value), for medians.
// Lifetimes are the including file's business (syncstats.hip describes the rule: the null stream, hipFree waits).
//
// Everything here is a template, inline, or static: both files include it.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
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

inline int build_layout(const int* seg, int m, int n_seg, Scratch& w, Layout& L, hipStream_t s) {
    L.m = m;
    L.n_seg = n_seg;
    THR_HIP_TRY(L.pos_frag.alloc(size_t(m) * 4));
    THR_HIP_TRY(L.seg_frag.alloc(size_t(n_seg) * 8));
    THR_HIP_TRY(hipMemsetAsync(L.seg_frag.p, 0, size_t(n_seg) * 8, s));
    hipLaunchKernelGGL(k_frag_heads, grid_for(m), dim3(kBlock), 0, s, seg, m, w.head.as<unsigned>());
    THR_HIP_TRY(hipGetLastError());
    THR_HIP_TRY(with_temp(w.tmp, w.tmp_bytes, [&](void* t, size_t& b) {
        return hipcub::DeviceScan::InclusiveSum(t, b, w.head.as<unsigned>(), w.incl.as<unsigned>(), m, s);
    }));
    unsigned nf = 0;
    THR_HIP_TRY(hipMemcpy(&nf, w.incl.as<unsigned>() + (m - 1), 4, hipMemcpyDeviceToHost));
    L.nf = int(nf);
    THR_HIP_TRY(L.frag_start.alloc((size_t(nf) + 1) * 4));
    hipLaunchKernelGGL(k_frag_layout, grid_for(m), dim3(kBlock), 0, s, seg, (const unsigned*)w.head.as<unsigned>(),
                       (const unsigned*)w.incl.as<unsigned>(), m, L.nf, L.pos_frag.as<int>(), L.frag_start.as<int>(),
                       L.seg_frag.as<int>());
    THR_HIP_TRY(hipGetLastError());
    return THR_OK;
}

// out[n_seg][K] (device) = the reduction of load() over every segment of L; slab holds nf * K doubles
template <int K, int NSUM, int NMIN, class Load>
int reduce(const Load& load, const Layout& L, double* slab, double* out, hipStream_t s) {
    if (const int rc = launch_reduce<K, NSUM, NMIN>(load, L.m, L.pos_frag.as<int>(), L.frag_start.as<int>(), slab, s)) return rc;
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
    hipLaunchKernelGGL(k_iota, grid_for(m), dim3(kBlock), 0, s, ia.as<unsigned>(), m);
    THR_HIP_TRY(hipGetLastError());
    THR_HIP_TRY(with_temp(w.tmp, w.tmp_bytes, [&](void* t, size_t& b) {
        return hipcub::DeviceRadixSort::SortPairs(t, b, key_lo.as<unsigned>(), lo2.as<unsigned>(), ia.as<unsigned>(),
                                                  ib.as<unsigned>(), m, 0, 32, s);
    }));
    hipLaunchKernelGGL(k_gather_u64, grid_for(m), dim3(kBlock), 0, s, (const unsigned long long*)key_hi.as<unsigned long long>(),
                       (const unsigned*)ib.as<unsigned>(), m, hi2.as<unsigned long long>());
    THR_HIP_TRY(hipGetLastError());
    THR_HIP_TRY(with_temp(w.tmp, w.tmp_bytes, [&](void* t, size_t& b) {
        return hipcub::DeviceRadixSort::SortPairs(t, b, hi2.as<unsigned long long>(), hi3.as<unsigned long long>(),
                                                  ib.as<unsigned>(), out.perm.as<unsigned>(), m, 0, 64, s);
    }));
    // lo in the final order: lo2 is in the order of ib, which the second sort permuted again
    hipLaunchKernelGGL(k_gather_u32, grid_for(m), dim3(kBlock), 0, s, (const unsigned*)key_lo.as<unsigned>(),
                       (const unsigned*)out.perm.as<unsigned>(), m, lo2.as<unsigned>());
    THR_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_cell_heads, grid_for(m), dim3(kBlock), 0, s, (const unsigned long long*)hi3.as<unsigned long long>(),
                       (const unsigned*)lo2.as<unsigned>(), m, w.head.as<unsigned>());
    THR_HIP_TRY(hipGetLastError());
    THR_HIP_TRY(with_temp(w.tmp, w.tmp_bytes, [&](void* t, size_t& b) {
        return hipcub::DeviceScan::InclusiveSum(t, b, w.head.as<unsigned>(), w.incl.as<unsigned>(), m, s);
    }));
    unsigned nc = 0;
    THR_HIP_TRY(hipMemcpy(&nc, w.incl.as<unsigned>() + (m - 1), 4, hipMemcpyDeviceToHost));
    out.nc = int(nc);
    THR_HIP_TRY(cell_ptr.alloc((size_t(nc) + 1) * 8));
    THR_HIP_TRY(cell_key.alloc(size_t(nc) * 12));
    hipLaunchKernelGGL(k_cell_layout, grid_for(m), dim3(kBlock), 0, s, (const unsigned long long*)hi3.as<unsigned long long>(),
                       (const unsigned*)lo2.as<unsigned>(), (const unsigned*)w.head.as<unsigned>(),
                       (const unsigned*)w.incl.as<unsigned>(), m, out.nc, out.pos_cell.as<int>(), cell_ptr.as<long long>(),
                       cell_key.as<int>());
    THR_HIP_TRY(hipGetLastError());
    return THR_OK;
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
    hipLaunchKernelGGL(k_iota, grid_for(m), dim3(kBlock), 0, s, ia, m);
    THR_HIP_TRY(hipGetLastError());
    THR_HIP_TRY(with_temp(w.tmp, w.tmp_bytes, [&](void* t, size_t& b) {
        return hipcub::DeviceRadixSort::SortPairs(t, b, vals, va, ia, ib, m, 0, 64, s);
    }));
    hipLaunchKernelGGL(k_gather_cell, grid_for(m), dim3(kBlock), 0, s, pos_cell, (const unsigned*)ib, m, ka);
    THR_HIP_TRY(hipGetLastError());
    int bits = 1;
    while (bits < 32 && (1ll << bits) < nc) ++bits;
    THR_HIP_TRY(with_temp(w.tmp, w.tmp_bytes, [&](void* t, size_t& b) {
        return hipcub::DeviceRadixSort::SortPairs(t, b, ka, kb, va, out.as<double>(), m, 0, bits, s);
    }));
    return THR_OK;
}

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
