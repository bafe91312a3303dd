// match on the device (reference thrifty/matchmaker.py:17-79): detections of the same transmission
// seen by several receivers.  Input is columns of detections sorted by timestamp.
//   1. groups: per txid, in timestamp order, the first unclaimed detection is a LEADER i and claims
//      every later detection j of its txid with not (ts[j] > ts[i] + window); the next leader is the
//      first detection of that txid past the window -- a greedy chain from the txid's first detection;
//   2. inside a group one entry per receiver: the first detection of a receiver, then for every
//      further one j a collision (entry so far, j) and entry = entry if energy[entry] > energy[j] else j;
//   3. per leader in input order: the entries in the order their receivers first appeared; fewer than
//      min_match entries -> the leader alone is a miss.
// Everything that scales with the number of detections runs here: a stable sort by txid puts every
// txid's detections side by side; the next-leader pointer of every detection is a search on the sorted
// timestamps; the leaders are the nodes reachable from the segment heads, marked by pointer doubling
// (no thread walks a chain); the entries are a segmented scan over the (group, rxid) runs of a second
// stable sort; the output orders are prefix sums over the leaders in input order.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstdint>
#include <utility>

#include "../../include/thrifty_hip.h"
#include "post_stages.hpp"

namespace {

using thr::DevBuf;
using thr::Event;
using thr::with_temp;

constexpr int kBlock = 256;  // workgroup size of every kernel here (tests/test_gpu_match_seams.py: W)
constexpr unsigned kNone = 0xFFFFFFFFu;

__device__ __forceinline__ unsigned key_i32(int v) { return unsigned(v) ^ 0x80000000u; }

__global__ void k_iota(unsigned* idx, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) idx[i] = unsigned(i);
}
// the one deviation from the reference: unsorted or NaN timestamps are refused (the smallest offender)
__global__ void k_check_sorted(const double* __restrict__ ts, int n, unsigned* first_bad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double t = ts[i];
    if (t != t || (i > 0 && !(t >= ts[i - 1]))) atomicMin(first_bad, unsigned(i));
}
__global__ void k_keys_tx(const int* __restrict__ txid, int n, unsigned* __restrict__ keys) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = key_i32(txid[i]);
}
__global__ void k_gather_ts(const double* __restrict__ ts, const unsigned* __restrict__ perm, int n,
                            double* __restrict__ ts_s) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) ts_s[p] = ts[perm[p]];
}

// In txid-sorted order (`key` ascending, timestamps ascending inside one key): jump[p] = the first
// position behind p that p's group cannot hold -- another txid, or ts > ts[p] + window (one float64
// add, one compare; equality stays inside) -- n if there is none.  Either way it is a leader if p is
// one.  Galloping then bisection: the predicate is monotone behind p.  mark[p] = p starts a txid.
__global__ void k_next_leader(const unsigned* __restrict__ key, const double* __restrict__ ts_s, int n,
                              double window, unsigned* __restrict__ jump, unsigned* __restrict__ mark) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const unsigned k = key[p];
    const double limit = __dadd_rn(ts_s[p], window);
    int lo = p, hi = n;  // `lo` belongs to p's group (or is p), `hi` does not (or is n)
    for (int step = 1; lo + step < n; step <<= 1) {
        const int probe = lo + step;
        if (key[probe] != k || ts_s[probe] > limit) {
            hi = probe;
            break;
        }
        lo = probe;
    }
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (key[mid] != k || ts_s[mid] > limit)
            hi = mid;
        else
            lo = mid;
    }
    jump[p] = unsigned(hi);
    mark[p] = (p == 0 || key[p - 1] != k) ? 1u : 0u;
}
// One round of pointer doubling: before round r, jump_in = next^(2^r) and every leader fewer than 2^r
// steps behind a segment head is marked; the round marks those fewer than 2^(r+1) steps behind.  The
// marks are idempotent stores of 1 on nodes that are leaders anyway, so a mark seen early is harmless;
// jump is double-buffered, so every thread squares the same function.
__global__ void k_double(const unsigned* __restrict__ jump_in, unsigned* __restrict__ jump_out,
                         unsigned* mark, int n) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n) return;
    const unsigned j = jump_in[m];
    if (j < unsigned(n)) {
        if (mark[m]) mark[j] = 1u;
        jump_out[m] = jump_in[j];
    } else {
        jump_out[m] = unsigned(n);
    }
}
// group numbers are the inclusive sum of the leader marks, minus one; lead_pos[g] = where group g
// starts in sorted order, lead_pos[number of groups] = n
__global__ void k_group_starts(const unsigned* __restrict__ mark, const unsigned* __restrict__ gincl,
                               int n, unsigned* __restrict__ lead_pos) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (mark[p]) lead_pos[gincl[p] - 1] = unsigned(p);
    if (p == n - 1) lead_pos[gincl[p]] = unsigned(n);
}
__global__ void k_keys_group_rx(const unsigned* __restrict__ gincl, const unsigned* __restrict__ perm,
                                const int* __restrict__ rxid, int n, unsigned long long* __restrict__ keys) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) keys[p] = ((unsigned long long)(gincl[p] - 1) << 32) | key_i32(rxid[perm[p]]);
}

// The running entry of a (group, receiver) run: w = w if energy[w] > energy[j] else j.  A NaN energy
// always takes over and then always loses (both compares are false), which is not associative as it
// stands: 5, NaN, 3 folds to 3, but 5 against (NaN, 3) -> 5.  So a NaN element RESTARTS the fold and
// carries -inf (which loses every `>` exactly as the NaN would); what is left is the maximum with ties
// to the later element, restarted at flags -- associative.
struct Winner {
    double v;
    unsigned idx;    // input index of the detection
    unsigned reset;  // run head, or NaN energy
};
struct WinnerOp {
    __host__ __device__ Winner operator()(const Winner& a, const Winner& b) const {
        if (b.reset) return b;
        Winner r = (a.v > b.v) ? a : b;
        r.reset = a.reset;
        return r;
    }
};
// q runs over the order sorted by (group, rxid), stable: sp[q] = position in txid order
__global__ void k_winner_in(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ sp,
                            const unsigned* __restrict__ perm, const double* __restrict__ energy, int n,
                            Winner* __restrict__ w, unsigned* __restrict__ is_first) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const bool head = q == 0 || keys[q - 1] != keys[q];
    const unsigned p = sp[q], orig = perm[p];
    const double e = energy[orig];
    const bool nan = e != e;
    Winner x;
    x.v = nan ? -INFINITY : e;
    x.idx = orig;
    x.reset = (head || nan) ? 1u : 0u;
    w[q] = x;
    is_first[p] = head ? 1u : 0u;  // the receiver's first detection in its group
}

// per leader, at its INPUT index: entries if the group is a match, match flag, miss flag, collisions
struct Quad {
    unsigned entries, match, miss, coll;
};
struct QuadSum {
    __host__ __device__ Quad operator()(const Quad& a, const Quad& b) const {
        return Quad{a.entries + b.entries, a.match + b.match, a.miss + b.miss, a.coll + b.coll};
    }
};
// first_incl = inclusive sum of is_first in txid order: receivers of a group = firsts in its range
__global__ void k_leader_counts(const unsigned* __restrict__ mark, const unsigned* __restrict__ gincl,
                                const unsigned* __restrict__ lead_pos, const unsigned* __restrict__ first_incl,
                                const unsigned* __restrict__ perm, int n, int min_match,
                                Quad* __restrict__ quad) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || !mark[p]) return;
    const unsigned end = lead_pos[gincl[p]];
    const unsigned n_rx = first_incl[end - 1] - first_incl[p] + 1u, size = end - unsigned(p);
    const bool is_match = (long long)n_rx >= (long long)min_match;
    quad[perm[p]] = Quad{is_match ? n_rx : 0u, is_match ? 1u : 0u, is_match ? 0u : 1u, size - n_rx};
}
__global__ void k_emit_leaders(const unsigned* __restrict__ mark, const unsigned* __restrict__ gincl,
                               const unsigned* __restrict__ perm, const Quad* __restrict__ quad,
                               const Quad* __restrict__ quad_incl, int n, unsigned* __restrict__ entry_base,
                               unsigned* __restrict__ coll_base, long long* __restrict__ match_ptr,
                               long long* __restrict__ miss) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || !mark[p]) return;
    const unsigned g = gincl[p] - 1, i = perm[p];
    const Quad own = quad[i], incl = quad_incl[i];
    coll_base[g] = incl.coll - own.coll;
    if (own.match) {
        entry_base[g] = incl.entries - own.entries;
        match_ptr[incl.match - 1] = (long long)(incl.entries - own.entries);
    } else {
        entry_base[g] = kNone;
        miss[incl.miss - 1] = (long long)i;
    }
}
// every detection that is not its receiver's first in the group is a collision with the entry before
// it; every run's last element holds the run's entry, which goes to the slot of the run's first
// appearance (found by bisection on the sorted keys: no walk along the run)
__global__ void k_emit_members(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ sp,
                               const unsigned* __restrict__ perm, const unsigned* __restrict__ first_incl,
                               const unsigned* __restrict__ lead_pos, const unsigned* __restrict__ entry_base,
                               const unsigned* __restrict__ coll_base, const Winner* __restrict__ w_incl,
                               int n, long long* __restrict__ match_idx, long long* __restrict__ coll) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const unsigned long long k = keys[q];
    const unsigned g = unsigned(k >> 32), lead = lead_pos[g], p = sp[q];
    if (q > 0 && keys[q - 1] == k) {
        const size_t slot = size_t(coll_base[g]) + (p - lead) - (first_incl[p] - first_incl[lead]) - 1u;
        coll[2 * slot] = (long long)w_incl[q - 1].idx;
        coll[2 * slot + 1] = (long long)perm[p];
    }
    const unsigned base = entry_base[g];
    if (base != kNone && (q == n - 1 || keys[q + 1] != k)) {
        unsigned lo = lead, hi = unsigned(q);  // the group occupies the same range in both orders
        while (lo < hi) {
            const unsigned mid = lo + (hi - lo) / 2;
            if (keys[mid] < k)
                lo = mid + 1;
            else
                hi = mid;
        }
        const unsigned p_first = sp[lo];
        match_idx[size_t(base) + (first_incl[p_first] - first_incl[lead])] = (long long)w_incl[q].idx;
    }
}

#define M_TRY THR_HIP_TRY

thread_local double g_times_ms[3] = {0, 0, 0};  // last thr_match of this thread: copies in, kernels, copies out

}  // namespace

// The stage on device pointers (post_stages.hpp): every kernel of the match step and the totals.  Unsorted
// or NaN timestamps come back as out.first_bad; the caller, who knows where the column lives, words them.
int thr::match_core(int n, const int* d_rx, const int* d_tx, const double* d_ts, const double* d_en, double window,
                    int min_match, hipStream_t s, MatchOut& out) {
    const dim3 blk(kBlock), grid((n + kBlock - 1) / kBlock);
    DevBuf d_bad;
    M_TRY(d_bad.alloc(4));

    // ---- 0. the input order
    M_TRY(hipMemset(d_bad.p, 0xFF, 4));
    hipLaunchKernelGGL(k_check_sorted, grid, blk, 0, s, d_ts, n, d_bad.as<unsigned>());
    M_TRY(hipGetLastError());
    unsigned bad = kNone;
    M_TRY(hipMemcpy(&bad, d_bad.p, 4, hipMemcpyDeviceToHost));
    out.first_bad = bad;
    if (bad != kNone) return THR_OK;  // the caller words the refusal

    // ---- 1. stable sort by txid: perm[p] = input index, increasing inside one txid
    DevBuf d_k32a, d_k32b, d_iota, d_perm, d_tss, d_tmp;
    size_t tmp_bytes = 0;
    M_TRY(d_k32a.alloc(size_t(n) * 4));
    M_TRY(d_k32b.alloc(size_t(n) * 4));
    M_TRY(d_iota.alloc(size_t(n) * 4));
    M_TRY(d_perm.alloc(size_t(n) * 4));
    M_TRY(d_tss.alloc(size_t(n) * 8));
    unsigned *key_s = d_k32b.as<unsigned>(), *iota = d_iota.as<unsigned>(), *perm = d_perm.as<unsigned>();
    hipLaunchKernelGGL(k_iota, grid, blk, 0, s, iota, n);
    hipLaunchKernelGGL(k_keys_tx, grid, blk, 0, s, d_tx, n, d_k32a.as<unsigned>());
    M_TRY(hipGetLastError());
    M_TRY(with_temp(d_tmp, tmp_bytes, [&](void* t, size_t& b) {
        return hipcub::DeviceRadixSort::SortPairs(t, b, d_k32a.as<unsigned>(), key_s, iota, perm, n, 0, 32, s);
    }));
    hipLaunchKernelGGL(k_gather_ts, grid, blk, 0, s, d_ts, perm, n, d_tss.as<double>());

    // ---- 2. next-leader pointers, leaders by pointer doubling, group numbers
    DevBuf d_ja, d_jb, d_mark, d_gincl, d_lead;
    M_TRY(d_ja.alloc(size_t(n) * 4));
    M_TRY(d_jb.alloc(size_t(n) * 4));
    M_TRY(d_mark.alloc(size_t(n) * 4));
    M_TRY(d_gincl.alloc(size_t(n) * 4));
    M_TRY(d_lead.alloc((size_t(n) + 1) * 4));
    unsigned *ja = d_ja.as<unsigned>(), *jb = d_jb.as<unsigned>(), *mark = d_mark.as<unsigned>();
    unsigned *gincl = d_gincl.as<unsigned>(), *lead_pos = d_lead.as<unsigned>();
    hipLaunchKernelGGL(k_next_leader, grid, blk, 0, s, key_s, d_tss.as<double>(), n, window, ja, mark);
    int log2n = 0;
    while ((size_t(1) << log2n) < size_t(n)) ++log2n;
    for (int round = 0; round < log2n + 1; ++round) {
        hipLaunchKernelGGL(k_double, grid, blk, 0, s, ja, jb, mark, n);
        std::swap(ja, jb);
    }
    M_TRY(hipGetLastError());
    M_TRY(with_temp(d_tmp, tmp_bytes, [&](void* t, size_t& b) {
        return hipcub::DeviceScan::InclusiveSum(t, b, mark, gincl, n, s);
    }));
    hipLaunchKernelGGL(k_group_starts, grid, blk, 0, s, mark, gincl, n, lead_pos);

    // ---- 3. stable sort by (group, rxid); the running entry of every (group, rxid) run
    DevBuf d_k64a, d_k64b, d_sp, d_win, d_wincl, d_first, d_fincl;
    M_TRY(d_k64a.alloc(size_t(n) * 8));
    M_TRY(d_k64b.alloc(size_t(n) * 8));
    M_TRY(d_sp.alloc(size_t(n) * 4));
    M_TRY(d_win.alloc(size_t(n) * sizeof(Winner)));
    M_TRY(d_wincl.alloc(size_t(n) * sizeof(Winner)));
    unsigned long long* keys = d_k64b.as<unsigned long long>();
    unsigned* sp = d_sp.as<unsigned>();
    unsigned *is_first = ja, *first_incl = jb;  // the jump tables are done with
    hipLaunchKernelGGL(k_keys_group_rx, grid, blk, 0, s, gincl, perm, d_rx, n,
                       d_k64a.as<unsigned long long>());
    M_TRY(hipGetLastError());
    M_TRY(with_temp(d_tmp, tmp_bytes, [&](void* t, size_t& b) {
        return hipcub::DeviceRadixSort::SortPairs(t, b, d_k64a.as<unsigned long long>(), keys, iota, sp, n, 0,
                                                  32 + log2n + 1, s);
    }));
    hipLaunchKernelGGL(k_winner_in, grid, blk, 0, s, keys, sp, perm, d_en, n, d_win.as<Winner>(),
                       is_first);
    M_TRY(hipGetLastError());
    M_TRY(with_temp(d_tmp, tmp_bytes, [&](void* t, size_t& b) {
        return hipcub::DeviceScan::InclusiveScan(t, b, d_win.as<Winner>(), d_wincl.as<Winner>(), WinnerOp(), n, s);
    }));
    M_TRY(with_temp(d_tmp, tmp_bytes, [&](void* t, size_t& b) {
        return hipcub::DeviceScan::InclusiveSum(t, b, is_first, first_incl, n, s);
    }));

    // ---- 4. receivers per group against min_match; output slots in the order of the leaders' input index
    DevBuf d_quad, d_qincl, d_ebase, d_cbase;
    M_TRY(d_quad.alloc(size_t(n) * sizeof(Quad)));
    M_TRY(d_qincl.alloc(size_t(n) * sizeof(Quad)));
    M_TRY(d_ebase.alloc(size_t(n) * 4));
    M_TRY(d_cbase.alloc(size_t(n) * 4));
    M_TRY(out.ptr.alloc((size_t(n) + 1) * 8));
    M_TRY(out.idx.alloc(size_t(n) * 8));
    M_TRY(out.miss.alloc(size_t(n) * 8));
    M_TRY(out.coll.alloc(size_t(n) * 16));
    M_TRY(hipMemsetAsync(d_quad.p, 0, size_t(n) * sizeof(Quad), s));
    hipLaunchKernelGGL(k_leader_counts, grid, blk, 0, s, mark, gincl, lead_pos, first_incl, perm, n, min_match,
                       d_quad.as<Quad>());
    M_TRY(hipGetLastError());
    M_TRY(with_temp(d_tmp, tmp_bytes, [&](void* t, size_t& b) {
        return hipcub::DeviceScan::InclusiveScan(t, b, d_quad.as<Quad>(), d_qincl.as<Quad>(), QuadSum(), n, s);
    }));
    hipLaunchKernelGGL(k_emit_leaders, grid, blk, 0, s, mark, gincl, perm, d_quad.as<Quad>(), d_qincl.as<Quad>(), n,
                       d_ebase.as<unsigned>(), d_cbase.as<unsigned>(), out.ptr.as<long long>(),
                       out.miss.as<long long>());
    hipLaunchKernelGGL(k_emit_members, grid, blk, 0, s, keys, sp, perm, first_incl, lead_pos,
                       d_ebase.as<unsigned>(), d_cbase.as<unsigned>(), d_wincl.as<Winner>(), n,
                       out.idx.as<long long>(), out.coll.as<long long>());
    M_TRY(hipGetLastError());
    Quad total;
    M_TRY(hipMemcpy(&total, d_qincl.as<Quad>() + (n - 1), sizeof(Quad), hipMemcpyDeviceToHost));
    out.n_matches = total.match;
    out.n_entries = total.entries;
    out.n_misses = total.miss;
    out.n_collisions = total.coll;
    return THR_OK;
}

extern "C" int thr_match(int device_id, size_t n_in, const int32_t* rxid, const int32_t* txid,
                         const double* timestamp, const double* energy, double window, int min_match,
                         int64_t* match_ptr_out, int64_t* match_idx_out, size_t* n_matches_out,
                         int64_t* miss_out, size_t* n_misses_out, int64_t* collision_out,
                         size_t* n_collisions_out) try {
    if (n_matches_out) *n_matches_out = 0;
    if (n_misses_out) *n_misses_out = 0;
    if (n_collisions_out) *n_collisions_out = 0;
    g_times_ms[0] = g_times_ms[1] = g_times_ms[2] = 0;
    if (n_in == 0) {
        if (match_ptr_out) match_ptr_out[0] = 0;
        return THR_OK;
    }
    if (!rxid || !txid || !timestamp || !energy || !match_ptr_out || !match_idx_out || !n_matches_out ||
        !miss_out || !n_misses_out || !collision_out || !n_collisions_out)
        return thr::fail_msg(THR_ERR_ARG, "thr_match: null argument");
    if (n_in > size_t(1) << 28) return thr::fail_msg(THR_ERR_ARG, "thr_match: too many detections");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return thr::fail_msg(THR_ERR_DEVICE, "no HIP device available (this engine has no CPU fallback)");
    if (device_id < 0 || device_id >= ndev) return thr::fail_msg(THR_ERR_ARG, "bad device_id %d", device_id);
    M_TRY(hipSetDevice(device_id));
    const int n = int(n_in);
    hipStream_t s = nullptr;
    Event ev[4];
    for (Event& e : ev) M_TRY(e.create());

    DevBuf d_rx, d_tx, d_ts, d_en;
    M_TRY(d_rx.alloc(size_t(n) * 4));
    M_TRY(d_tx.alloc(size_t(n) * 4));
    M_TRY(d_ts.alloc(size_t(n) * 8));
    M_TRY(d_en.alloc(size_t(n) * 8));
    M_TRY(hipEventRecord(ev[0].e, s));
    M_TRY(hipMemcpy(d_rx.p, rxid, size_t(n) * 4, hipMemcpyHostToDevice));
    M_TRY(hipMemcpy(d_tx.p, txid, size_t(n) * 4, hipMemcpyHostToDevice));
    M_TRY(hipMemcpy(d_ts.p, timestamp, size_t(n) * 8, hipMemcpyHostToDevice));
    M_TRY(hipMemcpy(d_en.p, energy, size_t(n) * 8, hipMemcpyHostToDevice));
    M_TRY(hipEventRecord(ev[1].e, s));

    thr::MatchOut out;
    const int rc = thr::match_core(n, d_rx.as<int>(), d_tx.as<int>(), d_ts.as<double>(), d_en.as<double>(), window,
                                   min_match, s, out);
    if (rc != THR_OK) return rc;
    if (out.first_bad != thr::kMatchSorted) {
        const unsigned bad = out.first_bad;
        return thr::fail_msg(THR_ERR_ARG,
                             "thr_match: timestamps must be non-decreasing without NaN: detection %u is %s",
                             bad, timestamp[bad] != timestamp[bad] ? "NaN" : "earlier than the one before it");
    }
    M_TRY(hipEventRecord(ev[2].e, s));

    M_TRY(hipMemcpy(match_ptr_out, out.ptr.p, out.n_matches * 8, hipMemcpyDeviceToHost));
    match_ptr_out[out.n_matches] = int64_t(out.n_entries);
    M_TRY(hipMemcpy(match_idx_out, out.idx.p, out.n_entries * 8, hipMemcpyDeviceToHost));
    M_TRY(hipMemcpy(miss_out, out.miss.p, out.n_misses * 8, hipMemcpyDeviceToHost));
    M_TRY(hipMemcpy(collision_out, out.coll.p, out.n_collisions * 16, hipMemcpyDeviceToHost));
    M_TRY(hipEventRecord(ev[3].e, s));
    M_TRY(hipEventSynchronize(ev[3].e));
    for (int k = 0; k < 3; ++k) {
        float ms = 0;
        M_TRY(hipEventElapsedTime(&ms, ev[k].e, ev[k + 1].e));
        g_times_ms[k] = ms;
    }
    *n_matches_out = out.n_matches;
    *n_misses_out = out.n_misses;
    *n_collisions_out = out.n_collisions;
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_match");
}

extern "C" int thr_debug_match_times(double* ms_out) try {
    if (!ms_out) return thr::fail_msg(THR_ERR_ARG, "thr_debug_match_times: null argument");
    for (int k = 0; k < 3; ++k) ms_out[k] = g_times_ms[k];
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_match_times");
}
