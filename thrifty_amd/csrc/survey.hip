// Capture survey on the device: mean spectrum, byte histogram and per-block byte sums of a raw u8 capture
// per interval of `integrate` blocks (definitions: survey.hpp), and the thr_survey_*
// entry points around the kernels.  A thr_survey rides on a handle as a thr_extract does; its partial
// interval stays on the device between calls.
#include "survey.hpp"

#include "fft_regs.hpp"
#include "passes_w8.hpp"

namespace thr {

using namespace k16;

namespace {

typedef unsigned long long u64;

constexpr size_t kSurveyLds = size_t(OFF_S) * sizeof(cpx) + kSurveyHistBytes;     // 163,840 B: the CU's LDS
static_assert(kSurveyLds <= 163840, "data + tables + histogram copies fit one CU");
static_assert(size_t(N + N / 16) * sizeof(u64) <= size_t(DATA) * sizeof(cpx), "the flush's staging fits the data area");

// the four bytes of a word into the LDS histogram ([value][copy], this lane's copy)
__device__ __forceinline__ void hist_word(unsigned* lhist, unsigned w, unsigned copy) {
    atomicAdd(lhist + ((w & 0xffu) * kSurveyCopies + copy), 1u);
    atomicAdd(lhist + (((w >> 8) & 0xffu) * kSurveyCopies + copy), 1u);
    atomicAdd(lhist + (((w >> 16) & 0xffu) * kSurveyCopies + copy), 1u);
    atomicAdd(lhist + ((w >> 24) * kSurveyCopies + copy), 1u);
}

// counter `v` summed over its copies and cleared, added to the interval's row if it counted anything
__device__ __forceinline__ void hist_flush(unsigned* lhist, unsigned v, u64* hrow) {
    static_assert(kSurveyCopies == 8, "two 16-byte reads per counter");
    uint4* c = reinterpret_cast<uint4*>(lhist + v * kSurveyCopies);
    const uint4 a = c[0], b = c[1];
    c[0] = c[1] = uint4{0u, 0u, 0u, 0u};
    const unsigned n = a.x + a.y + a.z + a.w + b.x + b.y + b.z + b.w;   // (a tile's bytes: < 2^32)
    if (n) atomicAdd(hrow + v, u64(n));
}

// k_carrier's structure on passes_w8.hpp.  Workgroup g takes the tiles g, g + gridDim.x, ... of kSurveyTile
// consecutive blocks; a thread's 32 bins (kbase + 512 k3) are summed as q in 64-bit registers over the
// blocks of a tile and flushed with 64-bit atomic adds at the tile's end, and before that wherever an
// interval ends inside the tile.  Integer adds: the tile length, the grid and the order of the flushes
// cannot change a bit of the result.
__global__ __launch_bounds__(NT) void k_survey16k(const unsigned char* __restrict__ samples, int n_blocks,
                                                  u64 blk_stride, unsigned open, unsigned integrate,
                                                  const cpx* __restrict__ tables, u64* __restrict__ spec,
                                                  u64* __restrict__ hist, u64* __restrict__ sums) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cpx* lds = reinterpret_cast<cpx*>(smem_raw);
    unsigned* lhist = reinterpret_cast<unsigned*>(lds + OFF_S);     // [256][kSurveyCopies]
    u64* stage = reinterpret_cast<u64*>(smem_raw);                  // the flush's transpose, over the data area

    load_tables(lds, tables);
    for (int i = threadIdx.x; i < 256 * kSurveyCopies; i += NT) lhist[i] = 0u;
    __syncthreads();
    cpx tw0[R1], tw1[R1];
    pass1_twiddles(lds, tw0, tw1, pass1_scale<RawSamples<THR_IN_U8>>());
    constexpr float scale = float(1u << (30 - 14));                 // 2^S, S = 30 - log2(16384)

    u64 acc[R3];
#pragma unroll
    for (int k3 = 0; k3 < R3; ++k3) acc[k3] = 0;

    const int n_tiles = (n_blocks + kSurveyTile - 1) / kSurveyTile;
    RawSamples<THR_IN_U8> cur;
    if (int(blockIdx.x) < n_tiles)
        cur.load(samples + size_t(blockIdx.x) * kSurveyTile * blk_stride, opaque_tid());
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int b0 = tile * kSurveyTile;
        const int b1 = b0 + kSurveyTile < n_blocks ? b0 + kSurveyTile : n_blocks;
        for (int b = b0; b < b1; ++b) {
            // (the previous block's pass-3 reads and a flush's reads all precede a barrier)
            fwd_pass1_pre(lds, cur, tw0, tw1);
            // byte statistics from the registers pass 1 has just consumed, before the prefetch refills them
            const int t = opaque_tid();
            unsigned s1 = 0, s2 = 0;
#pragma unroll
            for (int n1 = 0; n1 < R1; ++n1) {
                const unsigned w = cur.word(n1);
                s1 = __builtin_amdgcn_udot4(w, 0x01010101u, s1, false);
                s2 = __builtin_amdgcn_udot4(w, w, s2, false);
                hist_word(lhist, w, unsigned(t) & (kSurveyCopies - 1));
            }
            const int next = b + 1 < b1 ? b + 1 : (tile + int(gridDim.x)) * kSurveyTile;
            if (next < n_blocks) cur.load(samples + size_t(next) * blk_stride, opaque_tid());
            __syncthreads();
            fwd_pass2(lds);
            __builtin_amdgcn_sched_barrier(0);
            cpx v[R3];
            fwd_pass3(lds, v);
            __syncthreads();    // the data area is free: the next pass 1 or the flush may write it
            static_for<R3>([&](auto K) {
                constexpr int k3 = decltype(K)::value;
                const cpx x = v[brev(k3, R3)];
                acc[k3] += survey_q(x.x, x.y, scale);
            });
            // a wave's 4096 bytes: sum v^2 <= 266,342,400
            s1 = wave_sum_u32(s1);
            s2 = wave_sum_u32(s2);
            if ((t & 63) == 0) {
                atomicAdd(sums + 2 * size_t(b), u64(s1));
                atomicAdd(sums + 2 * size_t(b) + 1, u64(s2));
            }
            const unsigned pos = open + unsigned(b);
            if (b + 1 == b1 || (pos + 1u) % integrate == 0u) {
                // flush: through LDS, so that a wave's atomics fall on 512 consecutive bytes (in the thread's
                // own bin map neighbouring lanes are 128 B apart); one pad per 16 entries keeps the
                // transposing writes off each other's banks
                const unsigned row = pos / integrate;
                const int kbase = (t >> 5) + 16 * (t & 31);
                static_for<R3>([&](auto K) {
                    constexpr int k3 = decltype(K)::value;
                    const int bin = kbase + 512 * k3;
                    stage[bin + (bin >> 4)] = acc[k3];
                    acc[k3] = 0;
                });
                __syncthreads();
                u64* srow = spec + size_t(row) * N;
#pragma unroll 4
                for (int j = 0; j < N / NT; ++j) {
                    const int bin = j * NT + t;
                    atomicAdd(srow + bin, stage[bin + (bin >> 4)]);
                }
                if (t < 256) hist_flush(lhist, unsigned(t), hist + size_t(row) * 256);
                __syncthreads();
            }
        }
    }
}

// Natural-order spectra [n_blocks][n] -> accumulator rows: thread (bin k, row r) sums q over the blocks of the
// chunk that belong to row r and adds the sum to spec[r][k], which no other thread touches.
__global__ __launch_bounds__(256) void k_survey_fold(const float2* __restrict__ spectra, int n_blocks, int n,
                                                     float scale, unsigned open, unsigned integrate,
                                                     u64* __restrict__ spec) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const long long first = (long long)blockIdx.y * integrate - open;       // the row's first block, chunk-relative
    const int lo = first > 0 ? int(first) : 0;
    const int hi = first + integrate < n_blocks ? int(first + integrate) : n_blocks;
    u64 acc = 0;
    for (int b = lo; b < hi; ++b) {
        const float2 x = spectra[size_t(b) * n + k];
        acc += survey_q(x.x, x.y, scale);
    }
    spec[size_t(blockIdx.y) * n + k] += acc;
}

constexpr int kBytesThreads = 256;

// One workgroup per block: (sum v, sum v^2) in 64 bits and the block's histogram, added to its interval's row.
__global__ __launch_bounds__(kBytesThreads) void k_survey_bytes(const unsigned char* __restrict__ samples,
                                                                u64 blk_stride, unsigned blk_bytes, unsigned open,
                                                                unsigned integrate, u64* __restrict__ hist,
                                                                u64* __restrict__ sums) {
    __shared__ __attribute__((aligned(16))) unsigned lhist[256 * kSurveyCopies];
    __shared__ u64 red[2];
    const int t = threadIdx.x;
    for (int i = t; i < 256 * kSurveyCopies; i += kBytesThreads) lhist[i] = 0u;
    if (t < 2) red[t] = 0;
    __syncthreads();
    const unsigned char* blk = samples + size_t(blockIdx.x) * blk_stride;
    const unsigned copy = unsigned(t) & (kSurveyCopies - 1);
    u64 s1 = 0, s2 = 0;
    // (blocks of a stream start on 4-byte boundaries: stream_stride; an odd block_len leaves packed blocks
    // on 2-byte ones, and those are read byte by byte)
    const unsigned words = ((blk_stride | blk_bytes) & 3u) == 0u ? blk_bytes / 4u : 0u;
    for (unsigned i = t; i < words; i += kBytesThreads) {
        const unsigned w = reinterpret_cast<const unsigned*>(blk)[i];
        s1 += __builtin_amdgcn_udot4(w, 0x01010101u, 0u, false);
        s2 += __builtin_amdgcn_udot4(w, w, 0u, false);
        hist_word(lhist, w, copy);
    }
    for (unsigned i = words * 4u + t; i < blk_bytes; i += kBytesThreads) {
        const unsigned v = blk[i];
        s1 += v;
        s2 += v * v;
        atomicAdd(lhist + (v * kSurveyCopies + copy), 1u);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        s1 += __shfl_xor(s1, d, 64);
        s2 += __shfl_xor(s2, d, 64);
    }
    if ((t & 63) == 0) {
        atomicAdd(&red[0], s1);
        atomicAdd(&red[1], s2);
    }
    __syncthreads();
    if (t < 2) sums[2 * size_t(blockIdx.x) + t] = red[t];
    const unsigned row = (open + blockIdx.x) / integrate;
    hist_flush(lhist, unsigned(t), hist + size_t(row) * 256);
    static_assert(kBytesThreads == 256, "one thread per counter");
}

}  // namespace

hipError_t prepare_survey_16k() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_survey16k), hipFuncAttributeMaxDynamicSharedMemorySize,
                               int(kSurveyLds));
}

hipError_t launch_survey_16k(const unsigned char* d_samples, int n_blocks, unsigned long long blk_stride,
                             unsigned open, unsigned integrate, const float2* tables, unsigned long long* d_spec,
                             unsigned long long* d_hist, unsigned long long* d_sums, int grid, hipStream_t stream) {
    hipLaunchKernelGGL(k_survey16k, dim3(grid), dim3(NT), kSurveyLds, stream, d_samples, n_blocks, blk_stride, open,
                       integrate, reinterpret_cast<const cpx*>(tables), d_spec, d_hist, d_sums);
    return hipGetLastError();
}

hipError_t launch_survey_fold(const float2* d_spectra, int n_blocks, int block_len, int shift, unsigned open,
                              unsigned integrate, unsigned long long* d_spec, hipStream_t stream) {
    const unsigned rows = unsigned((u64(open) + u64(n_blocks) + integrate - 1) / integrate);
    hipLaunchKernelGGL(k_survey_fold, dim3((block_len + 255) / 256, rows), dim3(256), 0, stream, d_spectra, n_blocks,
                       block_len, std::ldexp(1.0f, shift), open, integrate, d_spec);
    return hipGetLastError();
}

hipError_t launch_survey_bytes(const unsigned char* d_samples, int n_blocks, unsigned long long blk_stride,
                               int block_len, unsigned open, unsigned integrate, unsigned long long* d_hist,
                               unsigned long long* d_sums, hipStream_t stream) {
    hipLaunchKernelGGL(k_survey_bytes, dim3(n_blocks), dim3(kBytesThreads), 0, stream, d_samples, blk_stride,
                       unsigned(block_len) * 2u, open, integrate, d_hist, d_sums);
    return hipGetLastError();
}

}  // namespace thr

namespace {

typedef unsigned long long u64;

struct SurveyDeleter {
    void operator()(thr_survey* s) const { thr_survey_destroy(s); }
};

int survey_zero(thr_survey* s) {
    const size_t n = size_t(s->h->cfg.block_len);
    HIP_TRY(hipMemsetAsync(s->d_spec, 0, s->rows * n * sizeof(u64), s->h->stream));
    HIP_TRY(hipMemsetAsync(s->d_hist, 0, s->rows * 256 * sizeof(u64), s->h->stream));
    HIP_TRY(hipStreamSynchronize(s->h->stream));
    s->fed = s->open = 0;
    return THR_OK;
}

int survey_create_body(thr_survey* s) {
    thr_handle* h = s->h;
    const size_t n = size_t(h->cfg.block_len), k = size_t(s->integrate);
    HIP_TRY(hipSetDevice(h->device));
    s->fused = h->fast;
    int log2n = 0;
    while ((size_t(1) << log2n) < n) ++log2n;
    s->shift = 30 - log2n;
    // blocks per chunk: the handle's max_batch, the input staging and (fold path) the dumped spectra; then
    // the accumulator rows a chunk can touch -- the open interval's and one per `integrate` blocks -- inside
    // kSurveyAccBudget, and the chunk cut down to what those rows take when `integrate` is small
    size_t chunk = std::min(size_t(h->cfg.max_batch), std::max<size_t>(1, thr::kSurveyStageBudget / (2 * n)));
    if (!s->fused) chunk = std::min(chunk, std::max<size_t>(1, thr::kSurveyDumpBudget / (n * sizeof(float2))));
    const size_t budget_rows = std::min(thr::kSurveyMaxRows, thr::kSurveyAccBudget / (n * sizeof(u64)));
    if (budget_rows < 2)
        return fail(THR_ERR_ARG, "thr_survey_create: block_len %zu leaves no two accumulator rows in %zu MiB", n,
                    thr::kSurveyAccBudget >> 20);
    s->rows = std::min(budget_rows, (k - 1 + chunk + k - 1) / k);
    if (s->rows < 2) s->rows = 2;
    s->chunk_max = std::min(chunk, (s->rows - 1) * k);      // (open < k: open + chunk <= rows * k)
    HIP_TRY(s->d_spec.alloc(s->rows * n * sizeof(u64)));
    HIP_TRY(s->d_hist.alloc(s->rows * 256 * sizeof(u64)));
    HIP_TRY(s->d_sums.alloc(s->chunk_max * 2 * sizeof(u64)));
    if (s->fused) {
        HIP_TRY(thr::prepare_survey_16k());
    } else {
        HIP_TRY(s->d_dump.alloc(s->chunk_max * n * sizeof(float2)));
    }
    return survey_zero(s);
}

// A chunk's input: caller memory -> device on the handle's stream, through the handle's input window when
// the range lies inside one (one copy per page-locked segment), as the gate's chunk loop does.
int survey_h2d(thr_handle* h, void* d_dst, const void* src, size_t bytes, const void* next) {
    if (h->win.acquire(src, bytes)) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(src);
        for (size_t done = 0; done < bytes;) {
            const uintptr_t at = a + done;
            const uintptr_t seg_end = h->win.base + (size_t((at - h->win.base) / h->win.kSeg) + 1) * h->win.kSeg;
            const size_t n = std::min<size_t>(bytes - done, size_t(seg_end - at));
            HIP_TRY(hipMemcpyAsync(static_cast<char*>(d_dst) + done, reinterpret_cast<const void*>(at), n,
                                   hipMemcpyHostToDevice, h->stream));
            done += n;
        }
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->win.release_below(reinterpret_cast<uintptr_t>(next));
        return THR_OK;
    }
    HIP_TRY(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, h->stream));
    return THR_OK;
}

// One chunk: copy, kernels, the sums and the completed rows back, the open interval's row to the front.
int survey_chunk(thr_survey* s, const uint8_t* src, size_t nb, size_t step, const void* next, u64* sums,
                 u64* spec_out, u64* hist_out, size_t* completed) {
    thr_handle* h = s->h;
    const size_t n = size_t(h->cfg.block_len), blk = 2 * n, k = size_t(s->integrate);
    const size_t bytes = (nb - 1) * step + blk;
    HIP_TRY(h->d_in.grow(bytes, bytes >> 3));
    THR_TRY(survey_h2d(h, h->d_in, src, bytes, next));
    const unsigned open = unsigned(s->open), integrate = unsigned(s->integrate);
    if (s->fused) {
        HIP_TRY(hipMemsetAsync(s->d_sums, 0, nb * 2 * sizeof(u64), h->stream));
        const int tiles = int((nb + thr::kSurveyTile - 1) / thr::kSurveyTile);
        HIP_TRY(thr::launch_survey_16k(h->d_in, int(nb), step, open, integrate, h->d_tables, s->d_spec, s->d_hist,
                                       s->d_sums, std::min(tiles, h->n_cu), h->stream));
    } else {
        THR_TRY(run_batch(h, h->d_in, THR_IN_U8, nullptr, int(nb), nullptr, s->d_dump, nullptr, nullptr, 0, true,
                          step == blk ? 0 : step));
        HIP_TRY(thr::launch_survey_fold(s->d_dump, int(nb), int(n), s->shift, open, integrate, s->d_spec, h->stream));
        HIP_TRY(thr::launch_survey_bytes(h->d_in, int(nb), step, int(n), open, integrate, s->d_hist, s->d_sums,
                                         h->stream));
    }
    if (sums) HIP_TRY(hipMemcpyAsync(sums, s->d_sums, nb * 2 * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    const size_t done = (s->open + nb) / k, touched = (s->open + nb + k - 1) / k;
    if (done) {
        HIP_TRY(hipMemcpyAsync(spec_out, s->d_spec, done * n * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(hist_out, s->d_hist, done * 256 * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
        size_t clear_from = 0;
        if (touched > done) {       // (rows `done` and 0 are different rows: no overlap)
            HIP_TRY(hipMemcpyAsync(s->d_spec, s->d_spec + done * n, n * sizeof(u64), hipMemcpyDeviceToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(s->d_hist, s->d_hist + done * 256, 256 * sizeof(u64), hipMemcpyDeviceToDevice,
                                   h->stream));
            clear_from = 1;
        }
        HIP_TRY(hipMemsetAsync(s->d_spec + clear_from * n, 0, (touched - clear_from) * n * sizeof(u64), h->stream));
        HIP_TRY(hipMemsetAsync(s->d_hist + clear_from * 256, 0, (touched - clear_from) * 256 * sizeof(u64), h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    s->open = (s->open + nb) % k;
    s->fed += nb;
    *completed = done;
    return THR_OK;
}

// `step`: bytes from a block's first sample to the next one's (2 block_len: packed)
int survey_run(thr_survey* s, const char* who, const uint8_t* src, size_t n_blocks, size_t step, u64* sums,
               u64* spec_sum, u64* hist, size_t cap_intervals, size_t* n_intervals) {
    thr_handle* h = s->h;
    const size_t n = size_t(h->cfg.block_len), k = size_t(s->integrate);
    const size_t total = size_t((s->open + n_blocks) / k);
    if (total > cap_intervals)
        return fail(THR_ERR_ARG, "%s: %zu blocks behind %llu open ones complete %zu intervals of %zu, room for %zu", who,
                    n_blocks, s->open, total, k, cap_intervals);
    if (total && (!spec_sum || !hist)) return fail(THR_ERR_ARG, "%s: null output", who);
    if (h->hp.async_open != 0)
        return fail(THR_ERR_STATE, "%s: %d submitted batch(es) not collected yet", who, h->hp.async_open);
    HIP_TRY(hipSetDevice(h->device));
    size_t out = 0;
    int rc = THR_OK;
    for (size_t done = 0; done < n_blocks && rc == THR_OK;) {
        // (open + nb <= rows * integrate: the chunk's blocks stay inside the allocated rows)
        const size_t nb = std::min({n_blocks - done, s->chunk_max, s->rows * k - size_t(s->open)});
        size_t got = 0;
        rc = survey_chunk(s, src + done * step, nb, step, src + (done + nb) * step, sums ? sums + 2 * done : nullptr,
                          spec_sum ? spec_sum + out * n : nullptr, hist ? hist + out * 256 : nullptr, &got);
        out += got;
        done += nb;
    }
    if (rc != THR_OK) {     // nothing of a failed chunk stays enqueued behind the caller's arrays
        (void)hipStreamSynchronize(h->stream);
        return rc;
    }
    *n_intervals = out;
    return THR_OK;
}

}  // namespace

extern "C" {

int thr_survey_create(thr_handle* h, int integrate, thr_survey** out) try {
    if (!h || !out) return fail(THR_ERR_ARG, "thr_survey_create: null argument");
    *out = nullptr;
    if (integrate < 1) return fail(THR_ERR_ARG, "thr_survey_create: integrate must be >= 1 (got %d)", integrate);
    std::unique_ptr<thr_survey, SurveyDeleter> s(new thr_survey);
    s->h = h;
    s->integrate = integrate;
    THR_TRY(survey_create_body(s.get()));
    *out = s.release();
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_survey_create");
}

// the device the buffers live on, then the survey's members give back what they own
void thr_survey_destroy(thr_survey* s) {
    if (!s) return;
    if (s->h) (void)hipSetDevice(s->h->device);
    delete s;
}

int thr_survey_reset(thr_survey* s) try {
    if (!s) return fail(THR_ERR_ARG, "thr_survey_reset: null survey");
    HIP_TRY(hipSetDevice(s->h->device));
    return survey_zero(s);
} catch (...) {
    return thr::on_exception("thr_survey_reset");
}

int thr_survey_shift(const thr_survey* s, int* shift) try {
    if (!s || !shift) return fail(THR_ERR_ARG, "thr_survey_shift: null argument");
    *shift = s->shift;
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_survey_shift");
}

int thr_survey_pending(const thr_survey* s, uint64_t* blocks_fed, uint64_t* blocks_in_open_interval) try {
    if (!s) return fail(THR_ERR_ARG, "thr_survey_pending: null survey");
    if (blocks_fed) *blocks_fed = s->fed;
    if (blocks_in_open_interval) *blocks_in_open_interval = s->open;
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_survey_pending");
}

int thr_survey_feed(thr_survey* s, const uint8_t* samples, size_t n_blocks, uint64_t* sums, uint64_t* spec_sum,
                    uint64_t* hist, size_t cap_intervals, size_t* n_intervals) try {
    if (!s || !n_intervals || (!samples && n_blocks)) return fail(THR_ERR_ARG, "thr_survey_feed: null argument");
    *n_intervals = 0;
    return survey_run(s, "thr_survey_feed", samples, n_blocks, size_t(s->h->cfg.block_len) * 2,
                      reinterpret_cast<u64*>(sums), reinterpret_cast<u64*>(spec_sum), reinterpret_cast<u64*>(hist),
                      cap_intervals, n_intervals);
} catch (...) {
    return thr::on_exception("thr_survey_feed");
}

int thr_survey_feed_stream(thr_survey* s, const uint8_t* stream, size_t n_bytes, uint64_t* sums, size_t sums_capacity,
                           size_t* n_blocks, uint64_t* spec_sum, uint64_t* hist, size_t cap_intervals,
                           size_t* n_intervals) try {
    if (!s || !n_blocks || !n_intervals || (!stream && n_bytes))
        return fail(THR_ERR_ARG, "thr_survey_feed_stream: null argument");
    *n_blocks = *n_intervals = 0;
    size_t stride = 0;
    THR_TRY(stream_stride(s->h, &stride));
    const size_t blk = size_t(s->h->cfg.block_len) * 2;
    if (n_bytes < blk) return THR_OK;
    const size_t nb = (n_bytes - blk) / stride + 1;
    if (sums && nb > sums_capacity)
        return fail(THR_ERR_ARG, "stream holds %zu blocks, sums array only %zu", nb, sums_capacity);
    THR_TRY(survey_run(s, "thr_survey_feed_stream", stream, nb, stride, reinterpret_cast<u64*>(sums),
                       reinterpret_cast<u64*>(spec_sum), reinterpret_cast<u64*>(hist), cap_intervals, n_intervals));
    *n_blocks = nb;
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_survey_feed_stream");
}

int thr_debug_survey_geometry(const thr_survey* s, int* tile_blocks, int* workgroups, int* fused) try {
    if (!s) return fail(THR_ERR_ARG, "thr_debug_survey_geometry: null survey");
    if (tile_blocks) *tile_blocks = s->fused ? thr::kSurveyTile : 1;
    if (workgroups) *workgroups = s->fused ? s->h->n_cu : (s->h->cfg.block_len + 255) / 256;
    if (fused) *fused = s->fused ? 1 : 0;
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_survey_geometry");
}

}  // extern "C"
