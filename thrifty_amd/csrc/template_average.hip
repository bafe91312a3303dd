// Averaged templates on the device (include/thrifty_hip.h, "Averaged templates", states the arithmetic).
//
// thr_extract_result remembers ONE block; an extraction with averaging armed also sums the cut of every
// qualifying record, per transmitter class, as exact integers of the u8 quantiser.  Per batch, behind the
// detect kernels, the fold and the keep, on the same stream and in front of the batch's done event:
//   k_avg_classify    one lane per record: qualifies? which class?  -> a byte column (class or -1), the counts
//   k_avg_accumulate  a workgroup owns 256 consecutive samples n of the cut and kAvgChunk consecutive records;
//                     per class present in the chunk it sums e and q in registers over the chunk's records of
//                     that class and adds both to the global uint64 sums ONCE: at most
//                     tiles x chunks x classes present x 256 x 2 integer atomics per batch, never records x W
// and once per result
//   k_avg_finish      m = acc_e / (count * 2^20 * 640), template_extract.hpp's scale_and_centre, var, sem.
// Integer sums commute: batching, input form, lane order and the arrival order of the atomics cannot show.
#include "template_extract.hpp"

namespace thr {

constexpr int kAvgThreads = 256;      // k_avg_classify's and k_avg_accumulate's workgroup; the samples of a tile
constexpr int kAvgChunk = 32;         // records per workgroup of k_avg_accumulate
constexpr int kAvgCounters = THR_AVERAGE_MAX_CLASSES + 2;      // count[16], n_unclassified, cut out of range

namespace {

struct AvgClasses {
    int n;
    double lo[THR_AVERAGE_MAX_CLASSES], hi[THR_AVERAGE_MAX_CLASSES];
};

__global__ __launch_bounds__(kAvgThreads) void k_avg_classify(const thr_record* __restrict__ recs, int n,
                                                              double max_offset, AvgClasses classes, int block_len,
                                                              int w, signed char* __restrict__ cls,
                                                              unsigned long long* __restrict__ counters) {
    __shared__ unsigned s_cnt[kAvgCounters];
    if (threadIdx.x < kAvgCounters) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * kAvgThreads + threadIdx.x;
    if (i < n) {
        const thr_record& r = recs[i];
        int k = -1;
        if ((r.flags & THR_FLAG_CORR) && fabs(r.corr_offset) <= max_offset) {
            int slot;
            if (r.corr_sample < 0 || r.corr_sample + w > block_len) {
                slot = THR_AVERAGE_MAX_CLASSES + 1;      // (never for a THR_FLAG_CORR record: no address is formed)
            } else {
                if (classes.n == 0) {
                    k = 0;
                } else {
                    const double v = double(r.carrier_bin) + r.carrier_offset;
                    for (int c = 0; c < classes.n; ++c)
                        if (classes.lo[c] <= v && v <= classes.hi[c]) k = c;      // the last match wins
                }
                slot = k >= 0 ? k : THR_AVERAGE_MAX_CLASSES;
            }
            atomicAdd(&s_cnt[slot], 1u);
        }
        cls[i] = (signed char)k;
    }
    __syncthreads();
    if (threadIdx.x < kAvgCounters && s_cnt[threadIdx.x] != 0)
        atomicAdd(&counters[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// e = floor(sqrt(q * 2^40)), q < 2^20: sqrt(q) * 2^20 in float64 is within 2^-23 of the root, so the truncation
// is off by at most one either way; the comparisons make it the integer square root whatever the float gave.
__device__ __forceinline__ unsigned long long envelope_fixed(unsigned q) {
    const unsigned long long big = (unsigned long long)q << 40;
    unsigned long long e = (unsigned long long)(sqrt(double(q)) * 1048576.0);
    while (e * e > big) --e;
    while ((e + 1) * (e + 1) <= big) ++e;
    return e;
}

// grid (tiles of 256 samples, chunks of kAvgChunk records).  The class column and corr_sample are read at
// workgroup-uniform addresses; a wave reads in + b * blk_stride + 2 * (corr_sample + n) as 64 consecutive byte
// pairs, aligned to 2 and no more (corr_sample may be odd, a stream's stride is any even number).
__global__ __launch_bounds__(kAvgThreads) void k_avg_accumulate(const thr_record* __restrict__ recs,
                                                                const signed char* __restrict__ cls, int n_recs,
                                                                const unsigned char* __restrict__ in,
                                                                unsigned long long blk_stride, int w,
                                                                unsigned long long* __restrict__ acc) {
    const int first = blockIdx.y * kAvgChunk;
    const int last = min(first + kAvgChunk, n_recs);
    const int n = blockIdx.x * kAvgThreads + threadIdx.x;
    unsigned present = 0;
    for (int r = first; r < last; ++r) {
        const int k = cls[r];
        if (k >= 0) present |= 1u << k;
    }
    while (present) {
        const int k = __builtin_ctz(present);
        present &= present - 1;
        unsigned long long sum_e = 0;
        unsigned sum_q = 0;      // kAvgChunk * 2^20 < 2^32
        for (int r = first; r < last; ++r) {
            if (cls[r] != k) continue;
            if (n < w) {
                const unsigned char* p = in + (unsigned long long)r * blk_stride + 2ull * unsigned(recs[r].corr_sample + n);
                const unsigned short pair = *reinterpret_cast<const unsigned short*>(p);
                const int di = 5 * int(pair & 0xff) - 637, dq = 5 * int(pair >> 8) - 637;
                const unsigned q = unsigned(di * di + dq * dq);
                sum_e += envelope_fixed(q);
                sum_q += q;
            }
        }
        if (n < w) {
            unsigned long long* dst = acc + (size_t)k * 2 * w;
            atomicAdd(dst + n, sum_e);
            atomicAdd(dst + w + n, (unsigned long long)sum_q);
        }
    }
}

__global__ __launch_bounds__(kCutThreads) void k_avg_finish(const unsigned long long* __restrict__ acc,
                                                            const unsigned long long* __restrict__ counters, int k,
                                                            int w, double* __restrict__ out) {
    __shared__ double scratch[kCutThreads];
    const unsigned long long count = counters[k];
    if (count == 0) return;      // (the host has checked)
    const unsigned long long* acc_e = acc + (size_t)k * 2 * w;
    const unsigned long long* acc_q = acc_e + w;
    const double cnt = double(count);
    double* sem = out + w;
    double sum = 0;
    for (int i = threadIdx.x; i < w; i += kCutThreads) {
        const double m = double(acc_e[i]) / (cnt * 671088640.0);
        double var;
        {
#pragma clang fp contract(off)
            const double mm = m * m;
            var = double(acc_q[i]) / (cnt * 409600.0) - mm;
        }
        sem[i] = sqrt(fmax(var, 0.0) / cnt);
        out[i] = m;
        sum += m;
    }
    const double scale = scale_and_centre(out, w, sum, scratch);
    for (int i = threadIdx.x; i < w; i += kCutThreads) sem[i] *= scale;
}

}  // namespace

namespace host {
namespace {

int n_acc_classes(const thr_average_opts& o) { return o.n_classes > 0 ? o.n_classes : 1; }

int average_enter(thr_extract* x, const char* who) {
    if (!x || !x->h) return fail(THR_ERR_ARG, "%s: null extraction", who);
    if (!x->avg_armed)
        return fail(THR_ERR_STATE, "%s: averaging is not armed on this extraction (thr_extract_average first)", who);
    if (x->h->hp.async_open != 0)
        return fail(THR_ERR_STATE, "%s: %d submitted batch(es) not collected yet (thr_collect first)", who,
                    x->h->hp.async_open);
    return THR_OK;
}

int read_counters(thr_extract* x, unsigned long long (&cnt)[kAvgCounters]) {
    HIP_TRY(hipSetDevice(x->h->device));
    HIP_TRY(hipMemcpyAsync(cnt, x->d_avg_cnt, sizeof cnt, hipMemcpyDeviceToHost, x->h->stream));
    HIP_TRY(hipStreamSynchronize(x->h->stream));
    return THR_OK;
}

}  // namespace

int average_reset(thr_extract* x) {
    if (!x->avg_armed) return THR_OK;
    const size_t w = size_t(x->h->cfg.template_len);
    HIP_TRY(hipMemsetAsync(x->d_avg_acc, 0, size_t(n_acc_classes(x->avg_opts)) * 2 * w * sizeof(unsigned long long),
                           x->h->stream));
    HIP_TRY(hipMemsetAsync(x->d_avg_cnt, 0, kAvgCounters * sizeof(unsigned long long), x->h->stream));
    return THR_OK;
}

int average_after_chunk(thr_extract* x, int b, const void* d_in, int format, size_t blk_stride, size_t nb) {
    thr_handle* h = x->h;
    // what the host can check of the addresses k_avg_accumulate forms: the batch is u8 in the slot's own staging
    // buffer (thr_extract_feed has refused complex64; every chunk function passes slot.d_in), its blocks lie inside
    // that buffer, and the class column has a byte per record (corr_sample is checked on the device)
    const size_t blk_bytes = size_t(h->cfg.block_len) * 2;
    const auto& slot = h->hp.slot[b];
    if (format != THR_IN_U8 || d_in != slot.d_in.p || nb > size_t(h->cfg.max_batch) || blk_stride % 2 != 0 ||
        (nb - 1) * blk_stride + blk_bytes > slot.d_in.bytes)
        return fail(THR_ERR_STATE, "averaging: a batch of %zu blocks (format %d) at stride %zu is not u8 inside its "
                                   "staging buffer", nb, format, blk_stride);
    AvgClasses classes;
    classes.n = x->avg_opts.n_classes;
    std::memcpy(classes.lo, x->avg_opts.lo, sizeof classes.lo);
    std::memcpy(classes.hi, x->avg_opts.hi, sizeof classes.hi);
    const int n = int(nb), w = h->cfg.template_len;
    hipLaunchKernelGGL(k_avg_classify, dim3((n + kAvgThreads - 1) / kAvgThreads), dim3(kAvgThreads), 0, h->stream,
                       slot.d_rec, n, x->max_offset, classes, h->cfg.block_len, w, x->d_avg_cls, x->d_avg_cnt);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_avg_accumulate, dim3((w + kAvgThreads - 1) / kAvgThreads, (n + kAvgChunk - 1) / kAvgChunk),
                       dim3(kAvgThreads), 0, h->stream, slot.d_rec, x->d_avg_cls, n,
                       static_cast<const unsigned char*>(d_in), (unsigned long long)blk_stride, w, x->d_avg_acc);
    HIP_TRY(hipGetLastError());
    return THR_OK;
}

}  // namespace host
}  // namespace thr

extern "C" {

int thr_extract_average(thr_extract* x, const thr_average_opts* opts) try {
    if (!x || !x->h) return fail(THR_ERR_ARG, "thr_extract_average: null extraction");
    if (x->fed != 0)
        return fail(THR_ERR_STATE, "thr_extract_average: %llu blocks have been fed since the last reset; averaging is "
                                   "armed or disarmed before the first feed (thr_extract_reset first)", x->fed);
    if (!opts) {
        x->avg_armed = false;
        return THR_OK;
    }
    if (opts->n_classes < 0 || opts->n_classes > THR_AVERAGE_MAX_CLASSES)
        return fail(THR_ERR_ARG, "thr_extract_average: n_classes is %d, an extraction averages 0 .. %d classes",
                    opts->n_classes, THR_AVERAGE_MAX_CLASSES);
    for (int k = 0; k < opts->n_classes; ++k) {
        if (!std::isfinite(opts->lo[k]) || !std::isfinite(opts->hi[k]))
            return fail(THR_ERR_ARG, "thr_extract_average: class %d has a bound that is not finite (%g .. %g)", k,
                        opts->lo[k], opts->hi[k]);
        if (opts->lo[k] > opts->hi[k])
            return fail(THR_ERR_ARG, "thr_extract_average: class %d has lo %g > hi %g", k, opts->lo[k], opts->hi[k]);
    }
    thr_handle* h = x->h;
    const size_t w = size_t(h->cfg.template_len);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(x->d_avg_acc.grow(size_t(thr::host::n_acc_classes(*opts)) * 2 * w * sizeof(unsigned long long)));
    HIP_TRY(x->d_avg_cnt.grow(thr::kAvgCounters * sizeof(unsigned long long)));
    HIP_TRY(x->d_avg_cls.grow(size_t(h->cfg.max_batch)));
    HIP_TRY(x->d_avg_out.grow(2 * w * sizeof(double)));
    x->avg_opts = *opts;
    x->avg_armed = true;
    return thr::host::average_reset(x);
} catch (...) {
    return thr::on_exception("thr_extract_average");
}

int thr_extract_average_counts(thr_extract* x, uint64_t count[THR_AVERAGE_MAX_CLASSES], uint64_t* n_unclassified) try {
    THR_TRY(thr::host::average_enter(x, "thr_extract_average_counts"));
    unsigned long long cnt[thr::kAvgCounters];
    THR_TRY(thr::host::read_counters(x, cnt));
    if (count)
        for (int k = 0; k < THR_AVERAGE_MAX_CLASSES; ++k) count[k] = cnt[k];
    if (n_unclassified) *n_unclassified = cnt[THR_AVERAGE_MAX_CLASSES];
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_extract_average_counts");
}

int thr_extract_average_result(thr_extract* x, int k, double* template_out, double* sem_out, size_t capacity,
                               uint64_t* acc_e_out, uint64_t* acc_q_out) try {
    THR_TRY(thr::host::average_enter(x, "thr_extract_average_result"));
    thr_handle* h = x->h;
    const int n_classes = thr::host::n_acc_classes(x->avg_opts);
    if (k < 0 || k >= n_classes)
        return fail(THR_ERR_ARG, "thr_extract_average_result: class %d, this extraction averages classes 0 .. %d", k,
                    n_classes - 1);
    const size_t w = size_t(h->cfg.template_len);
    if ((template_out || sem_out || acc_e_out || acc_q_out) && capacity < w)
        return fail(THR_ERR_ARG, "thr_extract_average_result: the template has %zu samples, room for %zu", w, capacity);
    unsigned long long cnt[thr::kAvgCounters];
    THR_TRY(thr::host::read_counters(x, cnt));
    if (cnt[THR_AVERAGE_MAX_CLASSES + 1] != 0)
        return fail(THR_ERR_STATE, "thr_extract_average_result: %llu qualifying record(s) had a corr_sample that "
                                   "leaves no %zu samples in a block of %d; they were not accumulated",
                    cnt[THR_AVERAGE_MAX_CLASSES + 1], w, h->cfg.block_len);
    const unsigned long long* acc = x->d_avg_acc.p + size_t(k) * 2 * w;
    if (acc_e_out)
        HIP_TRY(hipMemcpyAsync(acc_e_out, acc, w * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    if (acc_q_out)
        HIP_TRY(hipMemcpyAsync(acc_q_out, acc + w, w * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    if (cnt[k] == 0) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        return fail(THR_ERR_STATE, "no detection qualified for class %d: none of the %llu blocks fed has a correlation "
                                   "peak with |offset| <= %g inside its range, so there is nothing to average "
                                   "(%llu qualifying record(s) matched no class)",
                    k, x->fed, x->max_offset, cnt[THR_AVERAGE_MAX_CLASSES]);
    }
    if (template_out || sem_out) {
        hipLaunchKernelGGL(thr::k_avg_finish, dim3(1), dim3(thr::kCutThreads), 0, h->stream, x->d_avg_acc, x->d_avg_cnt,
                           k, int(w), x->d_avg_out);
        HIP_TRY(hipGetLastError());
        if (template_out)
            HIP_TRY(hipMemcpyAsync(template_out, x->d_avg_out, w * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (sem_out)
            HIP_TRY(hipMemcpyAsync(sem_out, x->d_avg_out.p + w, w * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_extract_average_result");
}

}  // extern "C"
