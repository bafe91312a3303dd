// Template extraction on the device -- the reference's template_extract.py:36-58 (best_detection +
// extract_template) without its yield_data round trip.
//
// best_detection keeps, over a whole capture, the detection with the largest correlation energy among
// those with |corr offset| <= max_offset, and inverse-transforms that block's SHIFTED spectrum;
// extract_template takes abs() of W samples of it.  The shift multiplies sample n by
// exp(2 pi i s (n / N - 1/2)), a phasor of modulus one, so that magnitude is the magnitude of the
// block's input samples and nothing but the ordinary records is needed to choose the block.  Per
// batch, behind the detect kernels on the same stream:
//   k_best_fold   one workgroup: every lane packs its qualifying records into orderable keys, wave
//                 and workgroup maximum, lane 0 folds the batch's winner into the running best
//   k_keep_block  reads the "improved" flag from device memory and copies the winner's input samples
//                 aside (or returns): the host never decides, the pipeline never waits
// and once at the end
//   k_extract_template  |x| in float64, mean / population std by a fixed tree, scale, centre.
#include "template_extract.hpp"

#include "card_gate.hpp"
#include "kernel_util.hpp"

namespace thr {
namespace {

constexpr int kFoldThreads = 1024;
constexpr int kKeepThreads = 256;

// float32 bits -> unsigned that orders like the float (negative values below positive ones)
__device__ __forceinline__ unsigned orderable(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#define THR_STEP(CTRL, MASK) v += dpp_u32<CTRL, MASK>(0u, v)
    THR_STEP(DPP_ROW_SHR1, 0xf);
    THR_STEP(DPP_ROW_SHR2, 0xf);
    THR_STEP(DPP_ROW_SHR4, 0xf);
    THR_STEP(DPP_ROW_SHR8, 0xf);
    THR_STEP(DPP_ROW_BCAST15, 0xa);
    THR_STEP(DPP_ROW_BCAST31, 0xc);
#undef THR_STEP
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

__global__ __launch_bounds__(kFoldThreads) void k_best_fold(const thr_record* __restrict__ recs,
                                                            const double* __restrict__ ts, double ts_all,
                                                            int n, unsigned long long base_pos, double max_offset,
                                                            ExtractState* __restrict__ state) {
    __shared__ unsigned long long s_key[kFoldThreads / 64];
    __shared__ unsigned s_cnt[kFoldThreads / 64];
    unsigned long long best = 0;
    unsigned count = 0;
    for (int i = threadIdx.x; i < n; i += kFoldThreads) {
        const thr_record& r = recs[i];
        if ((r.flags & THR_FLAG_CORR) && fabs(r.corr_offset) <= max_offset) {
            // (the earlier block has the larger low word; base_pos + i < 2^32, checked by the host)
            const unsigned long long key =
                ((unsigned long long)orderable(r.corr_energy) << 32) | (unsigned)~(unsigned)(base_pos + (unsigned)i);
            best = key > best ? key : best;
            count += 1;
        }
    }
    best = wave_max(best);
    count = wave_sum_u32(count);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        s_key[wave] = best;
        s_cnt[wave] = count;
    }
    __syncthreads();
    if (wave != 0) return;
    best = wave_max(lane < kFoldThreads / 64 ? s_key[lane] : 0ull);
    count = wave_sum_u32(lane < kFoldThreads / 64 ? s_cnt[lane] : 0u);
    if (lane != 0) return;
    state->n_qualifying += count;
    int improved = 0;
    if (best > state->key) {      // strict: an equal energy later in the run has the smaller key anyway
        const unsigned long long pos = (unsigned)~(unsigned)best;
        const int i = int(pos - base_pos);
        state->key = best;
        state->pos = pos;
        state->timestamp = ts ? ts[i] : ts_all;
        state->rec = recs[i];
        improved = 1;
    }
    state->improved = improved;
}

__global__ __launch_bounds__(kKeepThreads) void k_keep_block(ExtractState* __restrict__ state,
                                                             const unsigned char* __restrict__ in,
                                                             unsigned long long blk_stride, unsigned blk_words,
                                                             int format, unsigned long long base_pos, int n,
                                                             unsigned* __restrict__ keep) {
    if (!state->improved) return;
    const unsigned long long i = state->pos - base_pos;
    if (i >= (unsigned long long)n) return;
    const unsigned* src = reinterpret_cast<const unsigned*>(in + i * blk_stride);
    for (unsigned w = blockIdx.x * kKeepThreads + threadIdx.x; w < blk_words; w += gridDim.x * kKeepThreads)
        keep[w] = src[w];
    if (blockIdx.x == 0 && threadIdx.x == 0) state->keep_format = format;
}

__global__ __launch_bounds__(kCutThreads) void k_extract_template(const ExtractState* __restrict__ state,
                                                                  const void* __restrict__ keep, int block_len,
                                                                  int w, double* __restrict__ out) {
    __shared__ double scratch[kCutThreads];
    const int start = state->rec.corr_sample;
    if (state->key == 0 || start < 0 || start + w > block_len) return;   // (the host has checked)
    const bool u8 = state->keep_format == THR_IN_U8;
    const uchar2* kb = static_cast<const uchar2*>(keep) + start;
    const float2* kc = static_cast<const float2*>(keep) + start;
    double acc = 0;
    for (int i = threadIdx.x; i < w; i += kCutThreads) {
        float re, im;
        if (u8) {
            const uchar2 v = kb[i];
            re = (float(v.x) - 127.4f) / 128.0f;      // raw_to_complex (block_data.py:38-52)
            im = (float(v.y) - 127.4f) / 128.0f;
        } else {
            const float2 v = kc[i];
            re = v.x;
            im = v.y;
        }
        const double m = hypot(double(re), double(im));
        out[i] = m;
        acc += m;
    }
    scale_and_centre(out, w, acc, scratch);
}

}  // namespace

hipError_t launch_best_fold(const thr_record* d_recs, const double* d_ts, double ts_all, int n_blocks,
                            unsigned long long base_pos, double max_offset, ExtractState* d_state,
                            hipStream_t stream) {
    hipLaunchKernelGGL(k_best_fold, dim3(1), dim3(kFoldThreads), 0, stream, d_recs, d_ts, ts_all, n_blocks,
                       base_pos, max_offset, d_state);
    return hipGetLastError();
}

hipError_t launch_keep_block(ExtractState* d_state, const void* d_in, unsigned long long blk_stride,
                             unsigned blk_bytes, int format, unsigned long long base_pos, int n_blocks,
                             void* d_keep, hipStream_t stream) {
    const unsigned words = blk_bytes / 4;
    const unsigned grid = std::max(1u, std::min(64u, (words + kKeepThreads - 1) / kKeepThreads));
    hipLaunchKernelGGL(k_keep_block, dim3(grid), dim3(kKeepThreads), 0, stream, d_state,
                       static_cast<const unsigned char*>(d_in), blk_stride, words, format, base_pos, n_blocks,
                       static_cast<unsigned*>(d_keep));
    return hipGetLastError();
}

hipError_t launch_extract_template(const ExtractState* d_state, const void* d_keep, int block_len,
                                   int template_len, double* d_out, hipStream_t stream) {
    hipLaunchKernelGGL(k_extract_template, dim3(1), dim3(kCutThreads), 0, stream, d_state, d_keep, block_len,
                       template_len, d_out);
    return hipGetLastError();
}

namespace host {
namespace {

thread_local thr_extract* t_armed = nullptr;     // the extraction whose feed this thread is inside

struct Armed {
    Armed(thr_extract* x, const double* ts, double ts_all) {
        x->cur_ts = ts;
        x->cur_ts_all = ts_all;
        t_armed = x;
    }
    ~Armed() { t_armed = nullptr; }
};

struct ExtractDeleter {
    void operator()(thr_extract* x) const { thr_extract_destroy(x); }
};

constexpr unsigned long long kMaxFed = 0xFFFFFFFFull;    // positions are 32 bits of the fold's key

int feed_enter(thr_extract* x, const char* who, size_t n_blocks) {
    if (!x || !x->h) return fail(THR_ERR_ARG, "%s: null extraction", who);
    if (x->fed + n_blocks > kMaxFed)
        return fail(THR_ERR_ARG, "%s: an extraction takes at most %llu blocks between resets", who, kMaxFed);
    return THR_OK;
}

int create_body(thr_extract* x) {
    thr_handle* h = x->h;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(x->d_state.alloc(sizeof(thr::ExtractState)));
    HIP_TRY(x->d_keep.alloc(size_t(h->cfg.block_len) * 8));
    HIP_TRY(x->d_out.alloc(size_t(h->cfg.template_len) * sizeof(double)));
    for (int b = 0; b < thr_handle::kPipeDepth; ++b) {
        HIP_TRY(x->h_ts[b].alloc(size_t(h->cfg.max_batch) * sizeof(double)));
        HIP_TRY(x->d_ts[b].alloc(size_t(h->cfg.max_batch) * sizeof(double)));
    }
    HIP_TRY(hipMemsetAsync(x->d_state, 0, sizeof(thr::ExtractState), h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return THR_OK;
}

}  // namespace

int extract_after_chunk(thr_handle* h, int b, const void* d_in, int format, size_t stride, size_t first,
                        size_t nb) {
    thr_extract* x = t_armed;
    if (!x || x->h != h || nb == 0) return THR_OK;
    const double* d_ts = nullptr;
    if (x->cur_ts) {
        // (pinned staging of buffer b: its previous chunk has been drained, so its copy has left)
        std::memcpy(x->h_ts[b], x->cur_ts + first, nb * sizeof(double));
        HIP_TRY(hipMemcpyAsync(x->d_ts[b], x->h_ts[b], nb * sizeof(double), hipMemcpyHostToDevice, h->stream));
        d_ts = x->d_ts[b];
    }
    const unsigned blk_bytes = unsigned(h->cfg.block_len) * (format == THR_IN_U8 ? 2u : 8u);
    HIP_TRY(thr::launch_best_fold(h->hp.slot[b].d_rec, d_ts, x->cur_ts_all, int(nb), x->fed, x->max_offset, x->d_state,
                                  h->stream));
    HIP_TRY(thr::launch_keep_block(x->d_state, d_in, stride ? stride : blk_bytes, blk_bytes, format, x->fed,
                                   int(nb), x->d_keep, h->stream));
    x->fed += nb;       // (the fold is enqueued: the blocks count, whatever the averaging hook answers)
    if (x->avg_armed) THR_TRY(average_after_chunk(x, b, d_in, format, stride ? stride : blk_bytes, nb));
    return THR_OK;
}

}  // namespace host
}  // namespace thr

extern "C" {

int thr_extract_create(thr_handle* h, double max_offset, thr_extract** out) try {
    if (!h || !out) return fail(THR_ERR_ARG, "thr_extract_create: null argument");
    *out = nullptr;
    if (thr_is_gate(h))
        return fail(THR_ERR_ARG, "thr_extract_create: a carrier-gate handle has no correlation stage to pick a "
                                 "detection with; template extraction needs the default detector");
    if (h->dev.variant != THR_VARIANT_DEFAULT)
        return fail(THR_ERR_ARG, "thr_extract_create: template extraction follows the default detector's records "
                                 "(the reference's template_extract runs Detector); a %s handle is not offered",
                    h->dev.variant == THR_VARIANT_PRESHIFT ? "preshift" : "fastdet");
    if (h->cfg.n_templates != 1)
        return fail(THR_ERR_ARG, "thr_extract_create: template extraction takes ONE base template, this handle "
                                 "has %d", h->cfg.n_templates);
    if (!(max_offset >= 0)) return fail(THR_ERR_ARG, "thr_extract_create: max_offset must be >= 0");
    std::unique_ptr<thr_extract, thr::host::ExtractDeleter> x(new thr_extract);
    x->h = h;
    x->max_offset = max_offset;
    THR_TRY(thr::host::create_body(x.get()));
    *out = x.release();
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_extract_create");
}

// the device the buffers live on, then the extraction's members give back what they own
void thr_extract_destroy(thr_extract* x) {
    if (!x) return;
    if (x->h) (void)hipSetDevice(x->h->device);
    delete x;
}

int thr_extract_reset(thr_extract* x) try {
    if (!x) return fail(THR_ERR_ARG, "thr_extract_reset: null extraction");
    if (x->h->hp.async_open != 0)
        return fail(THR_ERR_STATE, "thr_extract_reset: %d submitted batch(es) not collected yet", x->h->hp.async_open);
    HIP_TRY(hipSetDevice(x->h->device));
    HIP_TRY(hipMemsetAsync(x->d_state, 0, sizeof(thr::ExtractState), x->h->stream));
    THR_TRY(thr::host::average_reset(x));
    x->fed = 0;
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_extract_reset");
}

int thr_extract_feed(thr_extract* x, const void* samples, int format, const int64_t* block_idx,
                     const double* timestamps, size_t n_blocks, thr_record* out) try {
    int rc = thr::host::feed_enter(x, "thr_extract_feed", n_blocks);
    if (rc != THR_OK || n_blocks == 0) return rc;
    if (x->avg_armed && format != THR_IN_U8)
        return fail(THR_ERR_ARG, "thr_extract_feed: averaging is armed and its sums are exact integers of the u8 "
                                 "quantiser: complex64 samples cannot be averaged (feed u8, or disarm)");
    std::vector<thr_record> scratch;
    if (!out) {
        scratch.resize(n_blocks);
        out = scratch.data();
    }
    thr::host::Armed armed(x, timestamps, 0.0);
    return thr_detect(x->h, samples, format, block_idx, n_blocks, out);
} catch (...) {
    return thr::on_exception("thr_extract_feed");
}

int thr_extract_feed_card(thr_extract* x, const char* text, size_t text_len, const int64_t* payload_off,
                          const int64_t* block_idx, const double* timestamps, size_t n_blocks,
                          thr_record* out) try {
    int rc = thr::host::feed_enter(x, "thr_extract_feed_card", n_blocks);
    if (rc != THR_OK || n_blocks == 0) return rc;
    std::vector<thr_record> scratch;
    if (!out) {
        scratch.resize(n_blocks);
        out = scratch.data();
    }
    thr::host::Armed armed(x, timestamps, 0.0);
    return thr_detect_card(x->h, text, text_len, payload_off, block_idx, n_blocks, out);
} catch (...) {
    return thr::on_exception("thr_extract_feed_card");
}

int thr_extract_feed_stream(thr_extract* x, const uint8_t* stream, size_t n_bytes, int64_t first_block_idx,
                            const double* timestamps, thr_record* out, size_t out_capacity,
                            size_t* n_blocks_out) try {
    if (!x || !x->h || !n_blocks_out) return fail(THR_ERR_ARG, "thr_extract_feed_stream: null argument");
    *n_blocks_out = 0;
    size_t stride = 0;
    int rc = stream_stride(x->h, &stride);
    if (rc != THR_OK) return rc;
    const size_t blk = size_t(x->h->cfg.block_len) * 2;
    const size_t n_blocks = n_bytes < blk ? 0 : (n_bytes - blk) / stride + 1;
    if ((rc = thr::host::feed_enter(x, "thr_extract_feed_stream", n_blocks)) != THR_OK) return rc;
    std::vector<thr_record> scratch;
    if (!out) {
        scratch.resize(std::max<size_t>(1, n_blocks));
        out = scratch.data();
        out_capacity = scratch.size();
    }
    thr::host::Armed armed(x, timestamps, 0.0);
    return thr_detect_stream(x->h, stream, n_bytes, first_block_idx, out, out_capacity, n_blocks_out);
} catch (...) {
    return thr::on_exception("thr_extract_feed_stream");
}

int thr_extract_submit_card(thr_extract* x, const char* text, size_t text_len, const int64_t* payload_off,
                            const int64_t* block_idx, const double* timestamps, size_t n_blocks, thr_record* out,
                            uint64_t* ticket) try {
    int rc = thr::host::feed_enter(x, "thr_extract_submit_card", n_blocks);
    if (rc != THR_OK) return rc;
    thr::host::Armed armed(x, timestamps, 0.0);
    return thr_submit_card(x->h, text, text_len, payload_off, block_idx, n_blocks, out, ticket);
} catch (...) {
    return thr::on_exception("thr_extract_submit_card");
}

int thr_extract_submit_stream(thr_extract* x, const uint8_t* stream, size_t n_bytes, int64_t first_block_idx,
                              double timestamp, thr_record* out, size_t out_capacity, size_t* n_blocks_out,
                              uint64_t* ticket) try {
    if (!x || !x->h) return fail(THR_ERR_ARG, "thr_extract_submit_stream: null extraction");
    size_t stride = 0;
    int rc = stream_stride(x->h, &stride);
    if (rc != THR_OK) return rc;
    const size_t blk = size_t(x->h->cfg.block_len) * 2;
    if ((rc = thr::host::feed_enter(x, "thr_extract_submit_stream", n_bytes < blk ? 0 : (n_bytes - blk) / stride + 1)) !=
        THR_OK)
        return rc;
    thr::host::Armed armed(x, nullptr, timestamp);
    return thr_submit_stream(x->h, stream, n_bytes, first_block_idx, out, out_capacity, n_blocks_out, ticket);
} catch (...) {
    return thr::on_exception("thr_extract_submit_stream");
}

int thr_extract_result(thr_extract* x, thr_record* best, double* timestamp, double* template_out, size_t capacity,
                       uint64_t* n_qualifying) try {
    if (!x || !x->h) return fail(THR_ERR_ARG, "thr_extract_result: null extraction");
    thr_handle* h = x->h;
    if (h->hp.async_open != 0)
        return fail(THR_ERR_STATE, "thr_extract_result: %d submitted batch(es) not collected yet (thr_collect first)",
                    h->hp.async_open);
    HIP_TRY(hipSetDevice(h->device));
    thr::ExtractState st;
    HIP_TRY(hipMemcpyAsync(&st, x->d_state, sizeof st, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (n_qualifying) *n_qualifying = st.n_qualifying;
    if (st.key == 0)
        return fail(THR_ERR_STATE, "no detection qualified: none of the %llu blocks fed has a correlation peak "
                                   "with |offset| <= %g, so there is no block to take a template from",
                    x->fed, x->max_offset);
    const int w = h->cfg.template_len, n = h->cfg.block_len;
    if (st.rec.corr_sample < 0 || st.rec.corr_sample + w > n)
        return fail(THR_ERR_STATE, "thr_extract_result: the winner's corr_sample %d leaves no %d samples in a block "
                                   "of %d", st.rec.corr_sample, w, n);
    if (best) *best = st.rec;
    if (timestamp) *timestamp = st.timestamp;
    if (template_out) {
        if (capacity < size_t(w))
            return fail(THR_ERR_ARG, "thr_extract_result: the template has %d samples, room for %zu", w, capacity);
        HIP_TRY(thr::launch_extract_template(x->d_state, x->d_keep, n, w, x->d_out, h->stream));
        HIP_TRY(hipMemcpyAsync(template_out, x->d_out, size_t(w) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_extract_result");
}

}  // extern "C"
