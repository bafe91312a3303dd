// The carrier gate on the device (fastcard's job: raw capture -> carrier verdict -> .card).
//
// The reference's fastcard transforms every block, asks cardet (fastcard/cardet.c:7-41) whether its
// spectrum holds a carrier and prints the blocks that do as .card lines "<timestamp> <block_idx>
// <base64(2N bytes)>" (fastcard_cli.c:183-193, codec fastcard/lib/base64.c).  Here the transform and
// the peak search are the detectors' carrier stage (launch_carrier_* fill CarStats); this file adds
//   k_gate_verdict  cardet's float32 power-domain verdict per block, a record per block, and the
//                   order-preserving list of the blocks that passed (ballot counts + one scan);
//   k_b64_encode    base64 of the listed blocks' raw bytes, read in place -- the mirror image of
//                   k_b64_decode (card_ingest.hip): 12 bytes in, 16 characters out per thread;
// and the host entry points thr_gate / thr_gate_stream / thr_gate_card around them.  Nothing of a
// block that did not pass is read by the encoder or crosses PCIe on the way back.
#include "card_gate.hpp"

namespace thr {

namespace {

// cardet_detect, cardet.c:7-41, on the carrier stage's statistics: sum = sum |X|^2 over all N bins,
// max = the window's largest power (peak_mag is its correctly rounded root).  Every operation is a
// separate float32 rounding as in the C source (no contraction into fused multiply-adds).
__global__ __launch_bounds__(1024) void k_gate_verdict(const CarStats* __restrict__ stats, int n_blocks,
                                                        int fft_len, float thr_const, float thr_snr,
                                                        const long long* __restrict__ block_idx,
                                                        long long first_idx, thr_record* __restrict__ rec,
                                                        int* __restrict__ pos, int* __restrict__ count) {
#pragma clang fp contract(off)
    __shared__ int wave_pass[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;                      // passed blocks in the tiles before this one
    for (int t0 = 0; t0 < n_blocks; t0 += 1024) {
        const int i = t0 + int(threadIdx.x);
        bool pass = false;
        if (i < n_blocks) {
            const CarStats st = stats[i];
            const float sum = st.sum_mag2;
            const float mx = st.peak_mag * st.peak_mag;
            float noise = 0.0f;
            if (sum != 0.0f) noise = (sum - 2.0f * mx) / float(fft_len - 1);
            const float threshold = thr_const + thr_snr * noise;
            pass = mx > threshold;
            thr_record r;
            r.block_idx = block_idx ? block_idx[i] : first_idx + i;
            r.flags = pass ? THR_FLAG_CARRIER : 0u;
            r.template_id = 0;
            r.carrier_bin = st.peak_idx;
            r.corr_sample = -1;
            r.carrier_offset = 0.0;
            r.corr_offset = 0.0;
            r.carrier_energy = sqrtf(mx);        // what fastcard's info line prints (fastcard_cli.c:175-180)
            r.carrier_noise = sqrtf(noise);
            r.corr_energy = 0.0f;
            r.corr_noise = 0.0f;
            r.reserved = (unsigned long long)__float_as_uint(threshold);
            rec[i] = r;
        }
        const unsigned long long m = __ballot(pass);
        if (lane == 0) wave_pass[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const int c = wave_pass[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (pass) pos[base + before + __popcll(m & ((1ull << lane) - 1ull))] = i;
        base += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = base;
}

// 6-bit value -> base64 character by compare / select arithmetic: 'A'..'Z', 'a'..'z', '0'..'9', '+', '/'
__device__ __forceinline__ unsigned b64_char(unsigned v) {
    return v + 'A' + (v >= 26u ? 6u : 0u) - (v >= 52u ? 75u : 0u) - (v >= 62u ? 15u : 0u) + (v >= 63u ? 3u : 0u);
}

// four characters (one little-endian dword) of three bytes
__device__ __forceinline__ unsigned b64_quantum(unsigned b0, unsigned b1, unsigned b2) {
    const unsigned v = (b0 << 16) | (b1 << 8) | b2;
    return b64_char(v >> 18) | (b64_char((v >> 12) & 63u) << 8) | (b64_char((v >> 6) & 63u) << 16) |
           (b64_char(v & 63u) << 24);
}

// one thread = four base64 quanta of one passed block: 12 bytes in (three dword loads: a block's
// window starts on a 4-byte boundary, not more), 16 characters out (one 16-byte store: slots start on
// 16-byte boundaries).  The thread behind a block's last whole group takes what is left byte by byte,
// writes the '=' padding and the newline.  The grid is flat -- (slot, part of the block) is unfolded
// from blockIdx.x -- and sized for every block of the batch passing: slots from *count on return.
__global__ __launch_bounds__(256) void k_b64_encode(const unsigned char* __restrict__ samples,
                                                    unsigned long long blk_stride, int in_bytes,
                                                    const int* __restrict__ pos, const int* __restrict__ count,
                                                    int wg_per_slot, unsigned long long slot_stride,
                                                    unsigned char* __restrict__ out) {
    const int slot = blockIdx.x / wg_per_slot;
    if (slot >= *count) return;
    const int n_whole = in_bytes / 12;          // groups of 12 bytes -> 16 characters
    const int g = (blockIdx.x - slot * wg_per_slot) * blockDim.x + threadIdx.x;
    if (g > n_whole) return;
    const unsigned char* src = samples + size_t(pos[slot]) * blk_stride + size_t(g) * 12;
    unsigned char* dst = out + size_t(slot) * slot_stride + size_t(g) * 16;
    if (g < n_whole) {
        const unsigned* s32 = reinterpret_cast<const unsigned*>(src);
        const unsigned w0 = s32[0], w1 = s32[1], w2 = s32[2];
        uint4 o;
        o.x = b64_quantum(w0 & 0xffu, (w0 >> 8) & 0xffu, (w0 >> 16) & 0xffu);
        o.y = b64_quantum(w0 >> 24, w1 & 0xffu, (w1 >> 8) & 0xffu);
        o.z = b64_quantum((w1 >> 16) & 0xffu, w1 >> 24, w2 & 0xffu);
        o.w = b64_quantum((w2 >> 8) & 0xffu, (w2 >> 16) & 0xffu, w2 >> 24);
        *reinterpret_cast<uint4*>(dst) = o;
        return;
    }
    // the tail: in_bytes - 12 n_whole bytes (0 .. 11), whole quanta first, then the padded one
    int left = in_bytes - 12 * n_whole;
    while (left > 0) {
        const unsigned b0 = src[0], b1 = left > 1 ? src[1] : 0u, b2 = left > 2 ? src[2] : 0u;
        const unsigned q = b64_quantum(b0, b1, b2);
        dst[0] = (unsigned char)(q & 0xffu);
        dst[1] = (unsigned char)((q >> 8) & 0xffu);
        dst[2] = left > 1 ? (unsigned char)((q >> 16) & 0xffu) : (unsigned char)'=';
        dst[3] = left > 2 ? (unsigned char)(q >> 24) : (unsigned char)'=';
        src += 3;
        dst += 4;
        left -= 3;
    }
    dst[0] = (unsigned char)'\n';
}

}  // namespace

hipError_t launch_gate_verdict(const CarStats* d_stats, int n_blocks, int fft_len, float thr_const,
                               float thr_snr, const long long* d_block_idx, long long first_idx,
                               thr_record* d_rec, int* d_pos, int* d_count, hipStream_t stream) {
    hipLaunchKernelGGL(k_gate_verdict, dim3(1), dim3(1024), 0, stream, d_stats, n_blocks, fft_len, thr_const,
                       thr_snr, d_block_idx, first_idx, d_rec, d_pos, d_count);
    return hipGetLastError();
}

hipError_t launch_b64_encode(const unsigned char* d_samples, unsigned long long blk_stride, int block_len,
                             const int* d_pos, const int* d_count, int max_slots, unsigned char* d_out,
                             hipStream_t stream) {
    if (max_slots <= 0) return hipSuccess;
    const int in_bytes = 2 * block_len;
    const int threads = in_bytes / 12 + 1;
    const int wg_per_slot = (threads + 255) / 256;
    if ((long long)wg_per_slot * max_slots > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_b64_encode, dim3(unsigned(wg_per_slot) * unsigned(max_slots)), dim3(256), 0, stream,
                       d_samples, blk_stride, in_bytes, d_pos, d_count, wg_per_slot,
                       (unsigned long long)gate_slot_stride(block_len), d_out);
    return hipGetLastError();
}

}  // namespace thr

namespace {

// What the three entry points share.  `out` receives the records, `slots` the passed blocks' payloads.
struct GateRun {
    thr_gate_handle* h;
    thr_record* out;
    char* slots;
    size_t passed = 0;
    size_t slot_stride, payload_chars;
};

int gate_enter(thr_handle* h, const char* who, size_t n_blocks, size_t slots_capacity) {
    if (!thr_is_gate(h)) return fail(THR_ERR_STATE, "%s: the handle is not a carrier gate (THR_VARIANT_GATE)", who);
    const size_t stride = thr::gate_slot_stride(h->cfg.block_len);
    if (slots_capacity / stride < n_blocks)       // (every block may pass)
        return fail(THR_ERR_ARG, "%s: %zu bytes of payload slots for %zu blocks, need %zu", who, slots_capacity,
                    n_blocks, n_blocks * stride);
    HIP_TRY(hipSetDevice(h->device));
    return THR_OK;
}

// One chunk whose u8 samples are on the device already (d_in; blocks `stride` bytes apart, 0 = packed):
// carrier stage, verdict, encode, and the way back -- records, the count, then count * slot_stride bytes.
int gate_chunk(GateRun& g, const void* d_in, size_t stride, const int64_t* block_idx, int64_t first_idx,
               size_t nb, size_t done, bool card) {
    thr_gate_handle* h = g.h;
    const int n = h->cfg.block_len;
    const size_t slots_bytes = nb * g.slot_stride;
    HIP_TRY(h->d_gate_slots.grow(slots_bytes, slots_bytes >> 3));
    HIP_TRY(h->h_gate_slots.grow(slots_bytes));
    const long long* d_idx = nullptr;
    if (block_idx) {
        HIP_TRY(hipMemcpyAsync(h->d_gate_off, block_idx, nb * sizeof(long long), hipMemcpyHostToDevice, h->stream));
        d_idx = h->d_gate_off;
    }
    THR_TRY(run_batch(h, d_in, THR_IN_U8, nullptr, int(nb), nullptr, nullptr, nullptr, nullptr, 0, true, stride));
    HIP_TRY(thr::launch_gate_verdict(h->d_stats, int(nb), n, h->gate_c, h->gate_s, d_idx, first_idx, h->d_gate_rec,
                                     h->d_gate_pos, h->d_gate_count, h->stream));
    HIP_TRY(thr::launch_b64_encode(static_cast<const unsigned char*>(d_in), h->dev.blk_stride, n, h->d_gate_pos,
                                   h->d_gate_count, int(nb), h->d_gate_slots, h->stream));
    HIP_TRY(hipMemcpyAsync(h->h_gate_count, h->d_gate_count, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(g.out + done, h->d_gate_rec, nb * sizeof(thr_record), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (card && h->h_gate_count[1] != 0)
        return fail(THR_ERR_ARG, "%d .card payload(s) in blocks [%zu, %zu) are not valid base64", h->h_gate_count[1],
                    done, done + nb);
    const size_t count = size_t(h->h_gate_count[0]);
    if (count > nb) return fail(THR_ERR_DEVICE, "gate: %zu of %zu blocks passed", count, nb);
    if (count) {
        HIP_TRY(hipMemcpyAsync(h->h_gate_slots, h->d_gate_slots, count * g.slot_stride, hipMemcpyDeviceToHost,
                               h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        // (only what the encoder wrote: the bytes behind a slot's newline are the caller's)
        for (size_t s = 0; s < count; ++s)
            std::memcpy(g.slots + (g.passed + s) * g.slot_stride,
                        h->h_gate_slots + s * g.slot_stride, g.payload_chars + 1);
    }
    g.passed += count;
    return THR_OK;
}

// A chunk's input: caller memory -> device on the handle's stream.  Inside the handle's input window
// (thr_input_window) the range is page-locked by now: one asynchronous copy per locked segment, as the
// detect entry points do (pipeline.hip: pipe_h2d); `next` = where the following chunk will start reading,
// everything below it may be unlocked once this chunk has been waited for (gate_chunk synchronises).
int gate_h2d(thr_handle* h, void* d_dst, const void* src, size_t bytes, const void* next) {
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

// Blocks per chunk: the staging stays near 64 MiB, and a chunk is ONE internal sub-batch of the carrier
// stage (long blocks and the multi-pass pipeline reuse d_stats from sub-batch to sub-batch).
size_t gate_chunk_blocks(const thr_handle* h, size_t bytes_per_block) {
    size_t nb = pipe_chunk_blocks(h, bytes_per_block);
    if (h->lng) nb = std::min(nb, size_t(h->long_batch));
    if (!h->lng && !h->fast && !h->small) nb = std::min(nb, size_t(h->gen_batch));
    return std::max<size_t>(1, nb);
}

// .card input: the chunk's payload offsets to the device, then k_b64_decode into the sample buffer
int gate_decode(thr_gate_handle* h, const long long* rel, size_t nb, size_t blk) {
    long long* d_rel = h->d_gate_off + h->cfg.max_batch;
    HIP_TRY(hipMemcpyAsync(d_rel, rel, nb * sizeof(long long), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(h->d_gate_count, 0, 2 * sizeof(int), h->stream));
    HIP_TRY(thr::launch_b64_decode(h->d_gate_text, d_rel, int(nb), int(blk), h->d_in, h->d_gate_count + 1,
                                   h->stream));
    return THR_OK;
}

int gate_grow(thr::Dev<unsigned char>& buf, size_t need) {      // (an eighth of slack, as the detect pipeline's staging)
    HIP_TRY(buf.grow(need, need >> 3));
    return THR_OK;
}

int gate_leave(thr_handle* h, int rc) {     // nothing of a failed chunk stays enqueued behind the caller's arrays
    if (rc != THR_OK) (void)hipStreamSynchronize(h->stream);
    return rc;
}

}  // namespace

extern "C" {

int thr_gate_slot_stride(const thr_handle* h, size_t* slot_stride, size_t* payload_chars) try {
    if (!h || !slot_stride) return fail(THR_ERR_ARG, "thr_gate_slot_stride: null argument");
    *slot_stride = thr::gate_slot_stride(h->cfg.block_len);
    if (payload_chars) *payload_chars = thr::gate_payload_chars(h->cfg.block_len);
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_gate_slot_stride");
}

int thr_gate(thr_handle* h, const uint8_t* samples, const int64_t* block_idx, size_t n_blocks, thr_record* out,
             size_t* n_passed, char* slots, size_t slots_capacity) try {
    if (!h || !n_passed || ((!samples || !out || !slots) && n_blocks))
        return fail(THR_ERR_ARG, "thr_gate: null argument");
    *n_passed = 0;
    int rc = gate_enter(h, "thr_gate", n_blocks, slots_capacity);
    if (rc != THR_OK) return rc;
    const size_t blk = size_t(h->cfg.block_len) * 2;
    GateRun g{thr_gate_of(h), out, slots, 0, thr::gate_slot_stride(h->cfg.block_len), thr::gate_payload_chars(h->cfg.block_len)};
    for (size_t done = 0; done < n_blocks && rc == THR_OK;) {
        const size_t nb = std::min(n_blocks - done, gate_chunk_blocks(h, blk));
        if ((rc = gate_grow(h->d_in, nb * blk)) != THR_OK) break;
        if ((rc = gate_h2d(h, h->d_in, samples + done * blk, nb * blk, samples + (done + nb) * blk)) != THR_OK) break;
        rc = gate_chunk(g, h->d_in, 0, block_idx ? block_idx + done : nullptr, int64_t(done), nb, done, false);
        done += nb;
    }
    if (rc == THR_OK) *n_passed = g.passed;
    return gate_leave(h, rc);
} catch (...) {
    return thr::on_exception("thr_gate");
}

int thr_gate_stream(thr_handle* h, const uint8_t* stream, size_t n_bytes, int64_t first_block_idx, thr_record* out,
                    size_t out_capacity, size_t* n_blocks_out, size_t* n_passed, char* slots,
                    size_t slots_capacity) try {
    if (!h || !stream || !n_blocks_out || !n_passed) return fail(THR_ERR_ARG, "thr_gate_stream: null argument");
    *n_blocks_out = *n_passed = 0;
    if (!thr_is_gate(h)) return fail(THR_ERR_STATE, "thr_gate_stream: the handle is not a carrier gate (THR_VARIANT_GATE)");
    size_t stride = 0;
    int rc = stream_stride(h, &stride);
    if (rc != THR_OK) return rc;
    const size_t blk = size_t(h->cfg.block_len) * 2;
    if (n_bytes < blk) return THR_OK;
    const size_t n_blocks = (n_bytes - blk) / stride + 1;
    if (n_blocks > out_capacity)
        return fail(THR_ERR_ARG, "stream holds %zu blocks, records array only %zu", n_blocks, out_capacity);
    if (!out || !slots) return fail(THR_ERR_ARG, "thr_gate_stream: null output");
    if ((rc = gate_enter(h, "thr_gate_stream", n_blocks, slots_capacity)) != THR_OK) return rc;
    GateRun g{thr_gate_of(h), out, slots, 0, thr::gate_slot_stride(h->cfg.block_len), thr::gate_payload_chars(h->cfg.block_len)};
    for (size_t done = 0; done < n_blocks && rc == THR_OK;) {
        const size_t nb = std::min(n_blocks - done, gate_chunk_blocks(h, stride));
        const size_t bytes = (nb - 1) * stride + blk;
        if ((rc = gate_grow(h->d_in, bytes)) != THR_OK) break;
        if ((rc = gate_h2d(h, h->d_in, stream + done * stride, bytes, stream + (done + nb) * stride)) != THR_OK) break;
        rc = gate_chunk(g, h->d_in, stride, nullptr, first_block_idx + int64_t(done), nb, done, false);
        done += nb;
    }
    if (rc == THR_OK) {
        *n_blocks_out = n_blocks;
        *n_passed = g.passed;
    }
    return gate_leave(h, rc);
} catch (...) {
    return thr::on_exception("thr_gate_stream");
}

int thr_gate_card(thr_handle* h, const char* text, size_t text_len, const int64_t* payload_off,
                  const int64_t* block_idx, size_t n_blocks, thr_record* out, size_t* n_passed, char* slots,
                  size_t slots_capacity) try {
    if (!h || !n_passed || ((!text || !payload_off || !out || !slots) && n_blocks))
        return fail(THR_ERR_ARG, "thr_gate_card: null argument");
    *n_passed = 0;
    int rc = gate_enter(h, "thr_gate_card", n_blocks, slots_capacity);
    if (rc != THR_OK) return rc;
    const size_t blk = size_t(h->cfg.block_len) * 2;
    const size_t chars = thr::gate_payload_chars(h->cfg.block_len);
    thr_gate_handle* gh = thr_gate_of(h);
    GateRun g{gh, out, slots, 0, thr::gate_slot_stride(h->cfg.block_len), chars};
    std::vector<long long> rel;
    for (size_t done = 0; done < n_blocks && rc == THR_OK;) {
        const size_t nb = std::min(n_blocks - done, gate_chunk_blocks(h, chars + 32));
        // contiguous span of text covering the chunk's payloads: [lo, hi + chars)
        long long lo = payload_off[done], hi = payload_off[done];
        for (size_t i = 0; i < nb; ++i) {
            const long long o = payload_off[done + i];
            if (o < 0 || size_t(o) + chars > text_len)
                return gate_leave(h, fail(THR_ERR_ARG, "payload %zu (offset %lld, %zu chars) lies outside the text",
                                          done + i, o, chars));
            lo = std::min(lo, o);
            hi = std::max(hi, o);
        }
        const size_t span = size_t(hi - lo) + chars;
        rel.resize(nb);
        for (size_t i = 0; i < nb; ++i) rel[i] = payload_off[done + i] - lo;
        if ((rc = gate_grow(gh->d_gate_text, span)) != THR_OK) break;
        if ((rc = gate_grow(h->d_in, nb * blk)) != THR_OK) break;
        if ((rc = gate_h2d(h, gh->d_gate_text, text + lo, span, text + hi + chars)) != THR_OK) break;
        if ((rc = gate_decode(gh, rel.data(), nb, blk)) != THR_OK) break;
        rc = gate_chunk(g, h->d_in, 0, block_idx ? block_idx + done : nullptr, int64_t(done), nb, done, true);
        done += nb;
    }
    if (rc == THR_OK) *n_passed = g.passed;
    return gate_leave(h, rc);
} catch (...) {
    return thr::on_exception("thr_gate_card");
}

}  // extern "C"
