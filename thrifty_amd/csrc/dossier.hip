// Detection dossiers on the device -- the numbers of the reference's detect_analysis.py (ForcibleDetector
// over the blocks in a list of ranges, the first `max` detected ones kept, and what its Plotter derives
// from each) without its per-block yield_data round trip.  Per batch, behind the detect kernels on the
// same stream (the k_best_fold / k_keep_block model of template_extract.hip):
//   k_pick        one workgroup walks the batch's records in trips of 1024: a ballot per wave and the
//                 waves' counts give every qualifying record its rank in feed order, hence its slot; the
//                 checked / skipped counts stop at the record that fills the last slot
//   k_keep_slots  reads from device memory which slots the pick just filled and copies those blocks'
//                 input samples into them (or returns): the host never decides
// and at result time, per chunk of kept blocks, behind the handle's unsectioned stage-dump launches:
//   k_dossier_series, k_dossier_peaks; once per dossier k_template_autocorr.
// Sums are float64 over a fixed tree; the only atomics are the LDS histogram's integer ones.
#include "dossier.hpp"

#include "card_gate.hpp"
#include "kernel_util.hpp"
#include "lmdif8.hpp"

namespace thr {
namespace {

constexpr int kPickThreads = 1024;
constexpr int kPickWaves = kPickThreads / 64;
constexpr int kKeepThreads = 256;
constexpr int kSeriesThreads = 256;
constexpr int kPeakThreads = 64;
constexpr int kKeepGridY = 64;

__device__ __forceinline__ bool in_ranges(long long v, const DossierRanges& r) {
    bool in = false;
#pragma unroll      // (constant indices: the ranges stay kernel arguments, read by scalar loads)
    for (int k = 0; k < kDossierMaxRanges; ++k) in = in || (k < r.n && v >= r.lo[k] && v <= r.hi[k]);
    return in;
}

__global__ __launch_bounds__(kPickThreads) void k_pick(const thr_record* __restrict__ recs,
                                                       const double* __restrict__ ts, double ts_all, int n,
                                                       unsigned long long base_pos, DossierRanges ranges,
                                                       unsigned max_keep, DossierState* __restrict__ state,
                                                       DossierSlot* __restrict__ slots) {
    __shared__ unsigned s_q[kPickWaves], s_c[kPickWaves], s_s[kPickWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned kept = state->n_kept;
    const unsigned first = kept;
    unsigned long long checked = state->n_checked, skipped = state->n_skipped;
    for (int base = 0; base < n && kept < max_keep; base += kPickThreads) {      // (`kept` is uniform)
        const int i = base + int(threadIdx.x);
        bool in = false, q = false;
        if (i < n) {
            in = in_ranges(recs[i].block_idx, ranges);
            const unsigned both = THR_FLAG_CARRIER | THR_FLAG_CORR;
            q = in && (recs[i].flags & both) == both;
        }
        // rank of this record among the trip's qualifying ones, in feed order
        const unsigned long long bq = __ballot(q);
        if (lane == 0) s_q[wave] = unsigned(__popcll(bq));
        __syncthreads();
        unsigned rank = unsigned(__popcll(bq & ((1ull << lane) - 1ull))), total = 0;
        for (int w = 0; w < kPickWaves; ++w) {
            rank += w < wave ? s_q[w] : 0u;
            total += s_q[w];
        }
        // the reference's loop is still running at this record: fewer than max_keep kept in front of it
        const bool live = kept + rank < max_keep;
        const unsigned long long bc = __ballot(in && live), bs = __ballot(in && !q && live);
        if (lane == 0) {
            s_c[wave] = unsigned(__popcll(bc));
            s_s[wave] = unsigned(__popcll(bs));
        }
        __syncthreads();
        for (int w = 0; w < kPickWaves; ++w) {
            checked += s_c[w];
            skipped += s_s[w];
        }
        if (q && live) {
            DossierSlot& s = slots[kept + rank];
            s.rec = recs[i];
            s.timestamp = ts ? ts[i] : ts_all;
            s.pos = base_pos + (unsigned long long)i;
        }
        kept += total < max_keep - kept ? total : max_keep - kept;
        __syncthreads();        // (the next trip rewrites the counts)
    }
    if (threadIdx.x == 0) {
        state->n_kept = kept;
        state->batch_first = first;
        state->n_checked = checked;
        state->n_skipped = skipped;
    }
}

__global__ __launch_bounds__(kKeepThreads) void k_keep_slots(const DossierState* __restrict__ state,
                                                             const DossierSlot* __restrict__ slots,
                                                             const unsigned char* __restrict__ in,
                                                             unsigned long long blk_stride, unsigned blk_words,
                                                             unsigned long long base_pos, int n, unsigned max_keep,
                                                             unsigned* __restrict__ keep) {
    const unsigned lo = state->batch_first;
    const unsigned hi = state->n_kept < max_keep ? state->n_kept : max_keep;
    if (lo >= hi) return;
    // 16-byte copies where the batch's framing allows them (a raw stream's stride is a multiple of 4 only)
    const bool wide = ((blk_stride | reinterpret_cast<unsigned long long>(in)) & 15ull) == 0 && (blk_words & 3u) == 0;
    for (unsigned s = lo + blockIdx.y; s < hi; s += gridDim.y) {
        const unsigned long long i = slots[s].pos - base_pos;
        if (i >= (unsigned long long)n) continue;
        const unsigned char* src = in + i * blk_stride;
        unsigned* dst = keep + size_t(s) * blk_words;
        if (wide) {
            const uint4* s4 = reinterpret_cast<const uint4*>(src);
            uint4* d4 = reinterpret_cast<uint4*>(dst);
            for (unsigned w = blockIdx.x * kKeepThreads + threadIdx.x; w < blk_words / 4; w += gridDim.x * kKeepThreads)
                d4[w] = s4[w];
        } else {
            const unsigned* s1 = reinterpret_cast<const unsigned*>(src);
            for (unsigned w = blockIdx.x * kKeepThreads + threadIdx.x; w < blk_words; w += gridDim.x * kKeepThreads)
                dst[w] = s1[w];
        }
    }
}

// sum over the workgroup in a fixed tree (every thread gets it)
__device__ __forceinline__ double tree_sum(double v, double* scratch) {
    __syncthreads();
    scratch[threadIdx.x] = v;
    __syncthreads();
    for (int half = kSeriesThreads / 2; half > 0; half >>= 1) {
        if (int(threadIdx.x) < half) scratch[threadIdx.x] += scratch[threadIdx.x + half];
        __syncthreads();
    }
    return scratch[0];
}

// magnitudes of four consecutive complex values: two 16-byte loads
__device__ __forceinline__ float4 mag4(const float2* __restrict__ src, int i4) {
    const float4 a = reinterpret_cast<const float4*>(src)[2 * i4], b = reinterpret_cast<const float4*>(src)[2 * i4 + 1];
    return make_float4(sqrtf(a.x * a.x + a.y * a.y), sqrtf(a.z * a.z + a.w * a.w), sqrtf(b.x * b.x + b.y * b.y),
                       sqrtf(b.z * b.z + b.w * b.w));
}

// mean((m - mean(m))^2) of the float32 magnitudes this workgroup has just written (each thread rereads its own)
__device__ __forceinline__ double variance_of(const float* __restrict__ mags, int n, double sum, double* scratch) {
    const double mean = sum / double(n);
    double acc = 0;
    for (int i4 = threadIdx.x; i4 < n / 4; i4 += kSeriesThreads) {
        const float4 m = reinterpret_cast<const float4*>(mags)[i4];
        const double d0 = double(m.x) - mean, d1 = double(m.y) - mean, d2 = double(m.z) - mean, d3 = double(m.w) - mean;
        acc += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
    return tree_sum(acc, scratch) / double(n);
}

__global__ __launch_bounds__(kSeriesThreads) void k_dossier_series(DossierSeriesArgs a) {
    __shared__ double scratch[kSeriesThreads];
    __shared__ unsigned s_hist[256];
    const int b = blockIdx.x, n = a.n, tid = threadIdx.x;
    const thr_record rec = a.slots[b].rec;
    const bool u8 = a.format == THR_IN_U8;
    s_hist[tid] = 0;
    __syncthreads();

    // ---- the input: histogram, rms, compensated samples (two samples per thread and trip)
    const double shift = -(double(rec.carrier_bin) + rec.carrier_offset);
    const unsigned char* blk = static_cast<const unsigned char*>(a.keep) + size_t(b) * size_t(n) * (u8 ? 2 : 8);
    float4* synced = reinterpret_cast<float4*>(a.synced + size_t(b) * n);
    double e_in = 0, e_out = 0;
    for (int i2 = tid; i2 < n / 2; i2 += kSeriesThreads) {
        float4 x;
        if (u8) {
            const uchar4 v = reinterpret_cast<const uchar4*>(blk)[i2];
            atomicAdd(&s_hist[v.x], 1u);
            atomicAdd(&s_hist[v.y], 1u);
            atomicAdd(&s_hist[v.z], 1u);
            atomicAdd(&s_hist[v.w], 1u);
            x = make_float4((float(v.x) - 127.4f) / 128.0f, (float(v.y) - 127.4f) / 128.0f,       // raw_to_complex
                            (float(v.z) - 127.4f) / 128.0f, (float(v.w) - 127.4f) / 128.0f);
        } else {
            x = reinterpret_cast<const float4*>(blk)[i2];
        }
        e_in += (double(x.x) * x.x + double(x.y) * x.y) + (double(x.z) * x.z + double(x.w) * x.w);
        // phase in turns, reduced in float64: shift * (i / n - 1/2)
        double t0 = shift * (double(2 * i2) / double(n) - 0.5), t1 = shift * (double(2 * i2 + 1) / double(n) - 0.5);
        t0 -= rint(t0);
        t1 -= rint(t1);
        double s0, c0, s1, c1;
        sincospi(2.0 * t0, &s0, &c0);
        sincospi(2.0 * t1, &s1, &c1);
        const float fc0 = float(c0), fs0 = float(s0), fc1 = float(c1), fs1 = float(s1);
        const float4 y = make_float4(x.x * fc0 - x.y * fs0, x.x * fs0 + x.y * fc0, x.z * fc1 - x.w * fs1,
                                     x.z * fs1 + x.w * fc1);
        synced[i2] = y;
        e_out += (double(y.x) * y.x + double(y.y) * y.y) + (double(y.z) * y.z + double(y.w) * y.w);
    }
    const double rms_in = sqrt(tree_sum(e_in, scratch) / double(n));
    const double rms_out = sqrt(tree_sum(e_out, scratch) / double(n));
    a.hist[size_t(b) * 256 + tid] = s_hist[tid];         // (tree_sum's barriers are behind the atomics)

    // ---- |FFT|, its standard deviation where the threshold asks for one
    float* fft_mag = a.fft_mag + size_t(b) * n;
    double sum = 0;
    for (int i4 = tid; i4 < n / 4; i4 += kSeriesThreads) {
        const float4 m = mag4(a.fft + size_t(b) * n, i4);
        reinterpret_cast<float4*>(fft_mag)[i4] = m;
        sum += (double(m.x) + double(m.y)) + (double(m.z) + double(m.w));
    }
    double fft_var = 0;
    if (a.car_thresh[2] != 0.0) fft_var = variance_of(fft_mag, n, tree_sum(sum, scratch), scratch);
    __syncthreads();            // fft_mag is complete: the filter reads its neighbours' bins

    // ---- the Dirichlet-matched spectrum: lfilter(w^2 reversed, 1, m^2) behind its delay, square root
    const int half = a.filter_half, rows = n - half;
    float* filtered = a.filtered + size_t(b) * rows;
    double fsum = 0;
    for (int i = tid; i < rows; i += kSeriesThreads) {
        double acc = 0;
        for (int j = (i < half ? -i : -half); j <= half; ++j) {
            const double m = double(fft_mag[i + j]);
            acc += a.weights2[j + half] * (m * m);
        }
        const float f = float(sqrt(acc));
        filtered[i] = f;
        fsum += double(f);
    }
    double filtered_var = 0;
    if (a.car_thresh[2] != 0.0 && rows > 0) {      // (the spectrum views put the same threshold formula over it)
        const double mean = tree_sum(fsum, scratch) / double(rows);
        double acc = 0;
        for (int i = tid; i < rows; i += kSeriesThreads) {
            const double dv = double(filtered[i]) - mean;
            acc += dv * dv;
        }
        filtered_var = tree_sum(acc, scratch) / double(rows);
    }

    // ---- the shifted spectrum's magnitude; std of |corr| where the threshold asks for one
    float* smag = a.synced_fft_mag + size_t(b) * n;
    double ssum = 0;
    for (int i4 = tid; i4 < n / 4; i4 += kSeriesThreads) {
        const float4 m = mag4(a.xhat + size_t(b) * n, i4);
        reinterpret_cast<float4*>(smag)[i4] = m;
        ssum += (double(m.x) + double(m.y)) + (double(m.z) + double(m.w));
    }
    double synced_var = 0;
    if (a.car_thresh[2] != 0.0) synced_var = variance_of(smag, n, tree_sum(ssum, scratch), scratch);
    double corr_var = 0;
    if (a.cor_thresh[2] != 0.0) {
        const float2* corr = a.corr + size_t(b) * n;
        double csum = 0;
        for (int i = tid; i < a.corr_len; i += kSeriesThreads) csum += double(sqrtf(corr[i].x * corr[i].x + corr[i].y * corr[i].y));
        const double mean = tree_sum(csum, scratch) / double(a.corr_len);
        double acc = 0;
        for (int i = tid; i < a.corr_len; i += kSeriesThreads) {
            const double d = double(sqrtf(corr[i].x * corr[i].x + corr[i].y * corr[i].y)) - mean;
            acc += d * d;
        }
        corr_var = tree_sum(acc, scratch) / double(a.corr_len);
    }
    if (tid == 0) {
        DossierScalars& s = a.scalars[b];
        s.rms_unsynced = rms_in;
        s.rms_synced = rms_out;
        s.fft_std = sqrt(fft_var);
        s.corr_std = sqrt(corr_var);
        s.synced_fft_std = sqrt(synced_var);
        s.filtered_std = sqrt(filtered_var);
        const double cn = double(rec.carrier_noise), xn = double(rec.corr_noise);
        s.carrier_threshold = sqrt(a.car_thresh[0] + a.car_thresh[1] * (cn * cn) + a.car_thresh[2] * fft_var);
        s.corr_threshold = sqrt(a.cor_thresh[0] + a.cor_thresh[1] * (xn * xn) + a.cor_thresh[2] * corr_var);
    }
}

// One wave per kept block.  The fit is lmdif8.hpp's (eight lanes per problem; the wave's eight groups run the
// same problem); its amplitude is the linear least-squares amplitude at the fitted offset, which is where a
// converged two-parameter fit puts it.
__global__ __launch_bounds__(kPeakThreads) void k_dossier_peaks(const DossierSlot* __restrict__ slots,
                                                                const float* __restrict__ fft_mag_all,
                                                                const float2* __restrict__ corr_all, int n,
                                                                int corr_len, int carrier_len,
                                                                DossierScalars* __restrict__ scalars) {
#pragma clang fp contract(off)
    __shared__ double s_re[kDossierPeakWindow], s_im[kDossierPeakWindow];
    const int b = blockIdx.x, lane = threadIdx.x;
    const thr_record rec = slots[b].rec;
    DossierScalars& out = scalars[b];
    const int bin = rec.carrier_bin;
    const bool valid = bin >= 6 && bin <= n - 7;         // (uniform)
    double amp = __longlong_as_double(0x7ff8000000000000ll), off = amp;
    if (valid) {
        const float* m = fft_mag_all + size_t(b) * n + bin;
        const int j = lane & 7;
        const float yj = j < 7 ? m[j - 3] : 0.0f;
        off = lmdif_dirichlet8(yj, m[0], j, double(n), double(carrier_len));
        const lm::Point pt{double(j - 3), 0.0, j < 7, double(n), double(carrier_len)};
        const double dj = lm::residual(pt, 1.0, off);      // |D(x_j - off)|
        amp = group8_sum(dj * double(yj)) / group8_sum(dj * dj);
    }
    // ---- |time_shift(corr[p - 5 : p + 6], corr_offset)| as a direct transform pair
    const int p = rec.corr_sample;
    int start = p - kDossierPeakWindow / 2, stop = p + kDossierPeakWindow / 2 + 1;
    start = start < 0 ? 0 : start;
    stop = stop > corr_len ? corr_len : stop;
    const int len = stop > start ? stop - start : 0;
    if (lane < len) {
        const float2 c = corr_all[size_t(b) * n + start + lane];
        s_re[lane] = double(c.x);
        s_im[lane] = double(c.y);
    }
    __syncthreads();
    double mag = 0;
    if (lane < len) {
        double yr = 0, yi = 0;
        for (int k = 0; k < len; ++k) {
            double xr = 0, xi = 0;      // X[k] = sum_q c[q] exp(-2 pi i k q / len)
            for (int q = 0; q < len; ++q) {
                double s, c;
                sincospi(-2.0 * double((k * q) % len) / double(len), &s, &c);
                xr += s_re[q] * c - s_im[q] * s;
                xi += s_re[q] * s + s_im[q] * c;
            }
            // np.fft.fftfreq: the upper half of the bins are negative frequencies
            const double f = double(k < (len + 1) / 2 ? k : k - len) / double(len);
            double s, c;
            sincos(2.0 * 3.141592653589793 * (rec.corr_offset * f + double((k * lane) % len) / double(len)), &s, &c);
            yr += xr * c - xi * s;
            yi += xr * s + xi * c;
        }
        mag = sqrt(yr * yr + yi * yi) / double(len);
    }
    if (lane < kDossierPeakWindow) out.corr_shifted[lane] = lane < len ? mag : 0.0;
    if (lane == 0) {
        out.fit_valid = valid ? 1 : 0;
        out.fit_amplitude = amp;
        out.fit_offset = off;
        out.peak_start = start;
        out.peak_len = len;
        out.reserved = 0;
    }
}

__global__ __launch_bounds__(kSeriesThreads) void k_template_autocorr(const double* __restrict__ t, int w,
                                                                      double* __restrict__ out) {
    __shared__ double scratch[kSeriesThreads];
    const int lag = blockIdx.x;
    double acc = 0;
    for (int i = threadIdx.x; i + lag < w; i += kSeriesThreads) acc += t[i + lag] * t[i];
    const double total = tree_sum(acc, scratch);
    if (threadIdx.x == 0) out[lag] = total;
}

}  // namespace

hipError_t launch_pick(const thr_record* d_recs, const double* d_ts, double ts_all, int n_blocks,
                       unsigned long long base_pos, const DossierRanges& ranges, unsigned max_keep,
                       DossierState* d_state, DossierSlot* d_slots, hipStream_t stream) {
    hipLaunchKernelGGL(k_pick, dim3(1), dim3(kPickThreads), 0, stream, d_recs, d_ts, ts_all, n_blocks, base_pos,
                       ranges, max_keep, d_state, d_slots);
    return hipGetLastError();
}

hipError_t launch_keep_slots(const DossierState* d_state, const DossierSlot* d_slots, const void* d_in,
                             unsigned long long blk_stride, unsigned blk_bytes, unsigned long long base_pos,
                             int n_blocks, unsigned max_keep, void* d_keep, hipStream_t stream) {
    const unsigned words = blk_bytes / 4;
    const unsigned gx = std::max(1u, std::min(16u, (words / 4 + kKeepThreads - 1) / kKeepThreads));
    const unsigned gy = std::max(1u, std::min(unsigned(kKeepGridY), std::min(unsigned(n_blocks), max_keep)));
    hipLaunchKernelGGL(k_keep_slots, dim3(gx, gy), dim3(kKeepThreads), 0, stream, d_state, d_slots,
                       static_cast<const unsigned char*>(d_in), blk_stride, words, base_pos, n_blocks, max_keep,
                       static_cast<unsigned*>(d_keep));
    return hipGetLastError();
}

hipError_t launch_dossier_series(const DossierSeriesArgs& a, int nb, hipStream_t stream) {
    hipLaunchKernelGGL(k_dossier_series, dim3(nb), dim3(kSeriesThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_dossier_peaks(const DossierSlot* d_slots, const float* d_fft_mag, const float2* d_corr, int n,
                                int corr_len, int carrier_len, DossierScalars* d_scalars, int nb,
                                hipStream_t stream) {
    hipLaunchKernelGGL(k_dossier_peaks, dim3(nb), dim3(kPeakThreads), 0, stream, d_slots, d_fft_mag, d_corr, n,
                       corr_len, carrier_len, d_scalars);
    return hipGetLastError();
}

hipError_t launch_template_autocorr(const double* d_template, int w, double* d_out, hipStream_t stream) {
    hipLaunchKernelGGL(k_template_autocorr, dim3(kDossierAutocorrLags), dim3(kSeriesThreads), 0, stream, d_template,
                       w, d_out);
    return hipGetLastError();
}

namespace host {
namespace {

thread_local thr_dossier* t_armed = nullptr;     // the dossier whose feed this thread is inside

struct Armed {
    Armed(thr_dossier* d, const double* ts, double ts_all) {
        d->cur_ts = ts;
        d->cur_ts_all = ts_all;
        t_armed = d;
    }
    ~Armed() { t_armed = nullptr; }
};

struct DossierDeleter {
    void operator()(thr_dossier* d) const { thr_dossier_destroy(d); }
};

int carrier_len_of(const thr_handle* h) { return h->cfg.carrier_len > 0 ? h->cfg.carrier_len : h->cfg.template_len; }

// carrier_sync.dirichlet_weights(F, N, W), squared: what carrier_detect._filter convolves |X|^2 with
std::vector<double> dirichlet_weights2(int f, int n, int w) {
    const double pi = 3.141592653589793;
    std::vector<double> c(size_t(f) + 1);
    double energy = 0;
    for (int k = 0; k <= f; ++k) {
        const double x = double(k - f / 2);
        double v = std::sin(pi * w * x / n) / std::sin(pi * x / n) / w;
        if (v != v) v = 1.0;
        c[size_t(k)] = v;
        energy += v * v;
    }
    for (double& v : c) v = (v / std::sqrt(energy)) * (v / std::sqrt(energy));
    return c;
}

int create_body(thr_dossier* d) {
    thr_handle* h = d->h;
    HIP_TRY(hipSetDevice(h->device));
    const int n = h->cfg.block_len, w = h->cfg.template_len;
    const int f = 2 * (n / carrier_len_of(h));
    d->filter_half = f / 2;
    HIP_TRY(d->d_state.alloc(sizeof(thr::DossierState)));
    HIP_TRY(d->d_slots.alloc(size_t(d->max_keep) * sizeof(thr::DossierSlot)));
    const std::vector<double> w2 = dirichlet_weights2(f, n, carrier_len_of(h));
    HIP_TRY(d->d_weights2.alloc(w2.size() * sizeof(double)));
    HIP_TRY(d->d_template.alloc(size_t(w) * sizeof(double)));
    HIP_TRY(d->d_autocorr.alloc(thr::kDossierAutocorrLags * sizeof(double)));
    for (int b = 0; b < thr_handle::kPipeDepth; ++b) {
        HIP_TRY(d->h_ts[b].alloc(size_t(h->cfg.max_batch) * sizeof(double)));
        HIP_TRY(d->d_ts[b].alloc(size_t(h->cfg.max_batch) * sizeof(double)));
    }
    HIP_TRY(hipMemcpyAsync(d->d_weights2, w2.data(), w2.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d->d_template, h->tpl_time.data(), size_t(w) * sizeof(double), hipMemcpyHostToDevice,
                           h->stream));
    HIP_TRY(hipMemsetAsync(d->d_state, 0, sizeof(thr::DossierState), h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));      // (`w2` leaves scope)
    return THR_OK;
}

int feed_enter(thr_dossier* d, const char* who, int format) {
    if (!d || !d->h) return fail(THR_ERR_ARG, "%s: null dossier", who);
    if (format != THR_IN_U8 && format != THR_IN_C64) return fail(THR_ERR_ARG, "%s: bad format %d", who, format);
    if (d->format >= 0 && d->format != format)
        return fail(THR_ERR_ARG, "%s: the dossier keeps %s samples, this batch brings the other format; reset first",
                    who, d->format == THR_IN_U8 ? "u8" : "complex64");
    HIP_TRY(hipSetDevice(d->h->device));
    if (!d->d_keep) {
        const size_t blk = size_t(d->h->cfg.block_len) * (format == THR_IN_U8 ? 2 : 8);
        HIP_TRY(d->d_keep.alloc(size_t(d->max_keep) * blk));
    }
    d->format = format;
    return THR_OK;
}

// the counts after the batch (the feed's detect call has drained the pipeline: the pick is done)
int feed_leave(thr_dossier* d, int rc, size_t* n_kept, uint64_t* n_checked, uint64_t* n_skipped) {
    if (rc != THR_OK) return rc;
    thr::DossierState st;
    HIP_TRY(hipMemcpyAsync(&st, d->d_state, sizeof st, hipMemcpyDeviceToHost, d->h->stream));
    HIP_TRY(hipStreamSynchronize(d->h->stream));
    if (n_kept) *n_kept = st.n_kept;
    if (n_checked) *n_checked = st.n_checked;
    if (n_skipped) *n_skipped = st.n_skipped;
    return THR_OK;
}

int ensure_result_buffers(thr_dossier* d) {
    if (d->chunk) return THR_OK;
    thr_handle* h = d->h;
    const size_t n = size_t(h->cfg.block_len);
    // a chunk's three dumps and five outputs stay near 200 MiB whatever the block length
    const int chunk = int(std::max<size_t>(1, std::min<size_t>(size_t(h->cfg.max_batch), (size_t(32) << 20) / (n * 8))));
    const size_t c = size_t(chunk);
    HIP_TRY(d->d_fft.alloc(c * n * sizeof(float2)));
    HIP_TRY(d->d_xhat.alloc(c * n * sizeof(float2)));
    HIP_TRY(d->d_corr.alloc(c * n * sizeof(float2)));
    HIP_TRY(d->d_synced.alloc(c * n * sizeof(float2)));
    HIP_TRY(d->d_fft_mag.alloc(c * n * sizeof(float)));
    HIP_TRY(d->d_filtered.alloc(c * n * sizeof(float)));
    HIP_TRY(d->d_synced_mag.alloc(c * n * sizeof(float)));
    HIP_TRY(d->d_hist.alloc(c * 256 * sizeof(unsigned)));
    HIP_TRY(d->d_scalars.alloc(c * sizeof(thr_dossier_scalars)));
    d->chunk = chunk;
    return THR_OK;
}

// a stage-dump launch writes h->d_rec-sized records somewhere: the chunk's own scratch, not the caller's
int result_chunk(thr_dossier* d, size_t first, size_t nb, size_t row, const thr_dossier_out* out,
                 Dev<thr_record>& d_rec) {
    thr_handle* h = d->h;
    const size_t n = size_t(h->cfg.block_len), blk = n * (d->format == THR_IN_U8 ? 2 : 8);
    const int corr_len = h->cfg.block_len - h->cfg.template_len + 1;
    const size_t dump = nb * n * sizeof(float2);
    HIP_TRY(hipMemsetAsync(d->d_fft, 0, dump, h->stream));
    HIP_TRY(hipMemsetAsync(d->d_xhat, 0, dump, h->stream));
    HIP_TRY(hipMemsetAsync(d->d_corr, 0, dump, h->stream));
    const unsigned char* keep = d->d_keep + first * blk;
    THR_TRY(run_batch(h, keep, d->format, nullptr, int(nb), d_rec, d->d_fft, d->d_xhat, d->d_corr, 0, false));
    thr::DossierSeriesArgs a{};
    a.keep = keep;
    a.format = d->format;
    a.n = int(n);
    a.corr_len = corr_len;
    a.filter_half = d->filter_half;
    a.slots = d->d_slots + first;
    a.fft = d->d_fft;
    a.xhat = d->d_xhat;
    a.corr = d->d_corr;
    a.weights2 = d->d_weights2;
    for (int k = 0; k < 3; ++k) {
        a.car_thresh[k] = h->cfg.carrier_thresh[k];
        a.cor_thresh[k] = h->cfg.corr_thresh[k];
    }
    a.hist = d->d_hist;
    a.fft_mag = d->d_fft_mag;
    a.filtered = d->d_filtered;
    a.synced = d->d_synced;
    a.synced_fft_mag = d->d_synced_mag;
    a.scalars = d->d_scalars;
    HIP_TRY(thr::launch_dossier_series(a, int(nb), h->stream));
    HIP_TRY(thr::launch_dossier_peaks(d->d_slots + first, d->d_fft_mag, d->d_corr, int(n), corr_len, carrier_len_of(h),
                                      d->d_scalars, int(nb), h->stream));
    const size_t rows_f = n - size_t(d->filter_half);
    auto back = [&](void* dst, const void* src, size_t bytes) {
        return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream) : hipSuccess;
    };
    HIP_TRY(back(out->hist ? out->hist + row * 256 : nullptr, d->d_hist, nb * 256 * sizeof(unsigned)));
    HIP_TRY(back(out->fft_mag ? out->fft_mag + row * n : nullptr, d->d_fft_mag, nb * n * sizeof(float)));
    HIP_TRY(back(out->filtered ? out->filtered + row * rows_f : nullptr, d->d_filtered, nb * rows_f * sizeof(float)));
    HIP_TRY(back(out->synced ? out->synced + row * n * 2 : nullptr, d->d_synced, nb * n * sizeof(float2)));
    HIP_TRY(back(out->synced_fft_mag ? out->synced_fft_mag + row * n : nullptr, d->d_synced_mag,
                 nb * n * sizeof(float)));
    HIP_TRY(back(out->scalars ? out->scalars + row : nullptr, d->d_scalars, nb * sizeof(thr_dossier_scalars)));
    if (out->corr)
        HIP_TRY(hipMemcpy2DAsync(out->corr + row * size_t(corr_len) * 2, size_t(corr_len) * sizeof(float2), d->d_corr,
                                 n * sizeof(float2), size_t(corr_len) * sizeof(float2), nb, hipMemcpyDeviceToHost,
                                 h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));      // (the next chunk reuses the buffers)
    return THR_OK;
}

}  // namespace

int dossier_after_chunk(thr_handle* h, int b, const void* d_in, int format, size_t stride, size_t first,
                        size_t nb) {
    thr_dossier* d = t_armed;
    if (!d || d->h != h || nb == 0) return THR_OK;
    const double* d_ts = nullptr;
    if (d->cur_ts) {
        // (pinned staging of buffer b: its previous chunk has been drained, so its copy has left)
        std::memcpy(d->h_ts[b], d->cur_ts + first, nb * sizeof(double));
        HIP_TRY(hipMemcpyAsync(d->d_ts[b], d->h_ts[b], nb * sizeof(double), hipMemcpyHostToDevice, h->stream));
        d_ts = d->d_ts[b];
    }
    const unsigned blk_bytes = unsigned(h->cfg.block_len) * (format == THR_IN_U8 ? 2u : 8u);
    HIP_TRY(thr::launch_pick(h->hp.slot[b].d_rec, d_ts, d->cur_ts_all, int(nb), d->fed, d->ranges, d->max_keep,
                             d->d_state, d->d_slots, h->stream));
    HIP_TRY(thr::launch_keep_slots(d->d_state, d->d_slots, d_in, stride ? stride : blk_bytes, blk_bytes, d->fed,
                                   int(nb), d->max_keep, d->d_keep, h->stream));
    d->fed += nb;
    return THR_OK;
}

}  // namespace host
}  // namespace thr

extern "C" {

int thr_dossier_create(thr_handle* h, const int64_t* ranges, int n_ranges, int64_t max_keep, thr_dossier** out) try {
    if (!h || !out || (n_ranges > 0 && !ranges)) return fail(THR_ERR_ARG, "thr_dossier_create: null argument");
    *out = nullptr;
    if (thr_is_gate(h))
        return fail(THR_ERR_ARG, "thr_dossier_create: a carrier-gate handle has no correlation stage; dossiers need "
                                 "the default detector");
    if (h->dev.variant != THR_VARIANT_DEFAULT)
        return fail(THR_ERR_ARG, "thr_dossier_create: dossiers follow the default detector's records (the reference's "
                                 "analyze_detect runs Detector); a %s handle is not offered",
                    h->dev.variant == THR_VARIANT_PRESHIFT ? "preshift" : "fastdet");
    if (h->cfg.n_templates != 1)
        return fail(THR_ERR_ARG, "thr_dossier_create: a dossier takes ONE template, this handle has %d",
                    h->cfg.n_templates);
    if (n_ranges < 0 || n_ranges > thr::kDossierMaxRanges)
        return fail(THR_ERR_ARG, "thr_dossier_create: %d ranges, at most %d", n_ranges, thr::kDossierMaxRanges);
    if (max_keep < 1) return fail(THR_ERR_ARG, "thr_dossier_create: max_keep must be >= 1");
    if (h->cfg.block_len % 4 != 0) return fail(THR_ERR_ARG, "thr_dossier_create: block_len must be a multiple of 4");
    const size_t blk = size_t(h->cfg.block_len) * 8;
    if (size_t(max_keep) > thr::kDossierMaxKeepBytes / blk)
        return fail(THR_ERR_ARG, "thr_dossier_create: %lld kept blocks of %zu bytes exceed %zu MiB", (long long)max_keep,
                    blk, thr::kDossierMaxKeepBytes >> 20);
    std::unique_ptr<thr_dossier, thr::host::DossierDeleter> d(new thr_dossier);
    d->h = h;
    d->max_keep = unsigned(max_keep);
    d->ranges.n = n_ranges;
    for (int k = 0; k < n_ranges; ++k) {
        d->ranges.lo[k] = ranges[2 * k];
        d->ranges.hi[k] = ranges[2 * k + 1];
    }
    THR_TRY(thr::host::create_body(d.get()));
    *out = d.release();
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_dossier_create");
}

// the device the buffers live on, then the dossier's members give back what they own
void thr_dossier_destroy(thr_dossier* d) {
    if (!d) return;
    if (d->h) (void)hipSetDevice(d->h->device);
    delete d;
}

int thr_dossier_reset(thr_dossier* d) try {
    if (!d || !d->h) return fail(THR_ERR_ARG, "thr_dossier_reset: null dossier");
    if (d->h->hp.async_open != 0)
        return fail(THR_ERR_STATE, "thr_dossier_reset: %d submitted batch(es) not collected yet", d->h->hp.async_open);
    HIP_TRY(hipSetDevice(d->h->device));
    HIP_TRY(hipMemsetAsync(d->d_state, 0, sizeof(thr::DossierState), d->h->stream));
    HIP_TRY(hipStreamSynchronize(d->h->stream));
    d->d_keep.release();
    d->format = -1;
    d->fed = 0;
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_dossier_reset");
}

int thr_dossier_feed(thr_dossier* d, const void* samples, int format, const int64_t* block_idx,
                     const double* timestamps, size_t n_blocks, thr_record* out, size_t* n_kept,
                     uint64_t* n_checked, uint64_t* n_skipped) try {
    THR_TRY(thr::host::feed_enter(d, "thr_dossier_feed", format));
    int rc = THR_OK;
    if (n_blocks != 0) {
        std::vector<thr_record> scratch;
        if (!out) {
            scratch.resize(n_blocks);
            out = scratch.data();
        }
        thr::host::Armed armed(d, timestamps, 0.0);
        rc = thr_detect(d->h, samples, format, block_idx, n_blocks, out);
    }
    return thr::host::feed_leave(d, rc, n_kept, n_checked, n_skipped);
} catch (...) {
    return thr::on_exception("thr_dossier_feed");
}

int thr_dossier_feed_card(thr_dossier* d, const char* text, size_t text_len, const int64_t* payload_off,
                          const int64_t* block_idx, const double* timestamps, size_t n_blocks, thr_record* out,
                          size_t* n_kept, uint64_t* n_checked, uint64_t* n_skipped) try {
    THR_TRY(thr::host::feed_enter(d, "thr_dossier_feed_card", THR_IN_U8));
    int rc = THR_OK;
    if (n_blocks != 0) {
        std::vector<thr_record> scratch;
        if (!out) {
            scratch.resize(n_blocks);
            out = scratch.data();
        }
        thr::host::Armed armed(d, timestamps, 0.0);
        rc = thr_detect_card(d->h, text, text_len, payload_off, block_idx, n_blocks, out);
    }
    return thr::host::feed_leave(d, rc, n_kept, n_checked, n_skipped);
} catch (...) {
    return thr::on_exception("thr_dossier_feed_card");
}

int thr_dossier_feed_stream(thr_dossier* d, const uint8_t* stream, size_t n_bytes, int64_t first_block_idx,
                            const double* timestamps, thr_record* out, size_t out_capacity, size_t* n_blocks_out,
                            size_t* n_kept, uint64_t* n_checked, uint64_t* n_skipped) try {
    if (!n_blocks_out) return fail(THR_ERR_ARG, "thr_dossier_feed_stream: null argument");
    *n_blocks_out = 0;
    THR_TRY(thr::host::feed_enter(d, "thr_dossier_feed_stream", THR_IN_U8));
    size_t stride = 0;
    THR_TRY(stream_stride(d->h, &stride));
    const size_t blk = size_t(d->h->cfg.block_len) * 2;
    const size_t n_blocks = n_bytes < blk ? 0 : (n_bytes - blk) / stride + 1;
    std::vector<thr_record> scratch;
    if (!out) {
        scratch.resize(std::max<size_t>(1, n_blocks));
        out = scratch.data();
        out_capacity = scratch.size();
    }
    int rc;
    {
        thr::host::Armed armed(d, timestamps, 0.0);
        rc = thr_detect_stream(d->h, stream, n_bytes, first_block_idx, out, out_capacity, n_blocks_out);
    }
    return thr::host::feed_leave(d, rc, n_kept, n_checked, n_skipped);
} catch (...) {
    return thr::on_exception("thr_dossier_feed_stream");
}

int thr_dossier_geometry(thr_dossier* d, int64_t out[4]) try {
    if (!d || !d->h || !out) return fail(THR_ERR_ARG, "thr_dossier_geometry: null argument");
    const thr_handle* h = d->h;
    out[0] = 2 * d->filter_half;
    out[1] = h->cfg.block_len - d->filter_half;
    out[2] = h->cfg.block_len - h->cfg.template_len + 1;
    out[3] = int64_t(std::max<size_t>(1, std::min<size_t>(size_t(h->cfg.max_batch),
                                                          (size_t(32) << 20) / (size_t(h->cfg.block_len) * 8))));
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_dossier_geometry");
}

int thr_dossier_result(thr_dossier* d, size_t first, size_t count, const thr_dossier_out* out, size_t* n_kept) try {
    if (!d || !d->h) return fail(THR_ERR_ARG, "thr_dossier_result: null dossier");
    thr_handle* h = d->h;
    if (h->hp.async_open != 0)
        return fail(THR_ERR_STATE, "thr_dossier_result: %d submitted batch(es) not collected yet (thr_collect first)",
                    h->hp.async_open);
    HIP_TRY(hipSetDevice(h->device));
    thr::DossierState st;
    HIP_TRY(hipMemcpyAsync(&st, d->d_state, sizeof st, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (n_kept) *n_kept = st.n_kept;
    if (!out || first >= st.n_kept || count == 0) return THR_OK;
    count = std::min<size_t>(count, st.n_kept - first);
    if (out->records || out->timestamps || out->positions) {
        std::vector<thr::DossierSlot> slots(count);
        HIP_TRY(hipMemcpy(slots.data(), d->d_slots + first, count * sizeof(thr::DossierSlot), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < count; ++i) {
            if (out->records) out->records[i] = slots[i].rec;
            if (out->timestamps) out->timestamps[i] = slots[i].timestamp;
            if (out->positions) out->positions[i] = slots[i].pos;
        }
    }
    if (out->autocorr) {
        if (!d->autocorr_done) {
            HIP_TRY(thr::launch_template_autocorr(d->d_template, h->cfg.template_len, d->d_autocorr, h->stream));
            d->autocorr_done = true;
        }
        HIP_TRY(hipMemcpyAsync(out->autocorr, d->d_autocorr, thr::kDossierAutocorrLags * sizeof(double),
                               hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    if (!(out->hist || out->fft_mag || out->filtered || out->synced || out->synced_fft_mag || out->corr || out->scalars))
        return THR_OK;
    THR_TRY(thr::host::ensure_result_buffers(d));
    Dev<thr_record> d_rec;
    HIP_TRY(d_rec.alloc(size_t(d->chunk) * sizeof(thr_record)));
    for (size_t off = 0; off < count; off += size_t(d->chunk))
        THR_TRY(thr::host::result_chunk(d, first + off, std::min(size_t(d->chunk), count - off), off, out, d_rec));
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_dossier_result");
}

}  // extern "C"
