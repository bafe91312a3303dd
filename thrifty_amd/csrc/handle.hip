// The engine handle: error state, per-handle constants, creation / destruction, queries.
#include "host_internal.hpp"

#include "card_gate.hpp"

namespace thr {
namespace host {

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

}  // namespace host
}  // namespace thr

namespace thr {
// error reporting for the other translation units of the library (identify.hip)
int fail_msg(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    host::g_last_error = buf;
    return code;
}
// No exception leaves the C ABI (include/thrifty_hip.h): every entry point that allocates or starts
// a thread is a function-try-block ending here.  Host memory exhaustion and a refused thread
// (std::system_error: a pids / thread limit, eight ranks on one host) become THR_ERR_DEVICE.
int on_exception(const char* who) noexcept {
    try {
        try {
            throw;
        } catch (const std::bad_alloc&) {
            return fail_msg(THR_ERR_DEVICE, "%s: out of host memory", who);
        } catch (const std::exception& e) {
            return fail_msg(THR_ERR_DEVICE, "%s: %s", who, e.what());
        } catch (...) {
            return fail_msg(THR_ERR_DEVICE, "%s: unknown C++ exception", who);
        }
    } catch (...) {         // (the message itself could not be stored)
        return THR_ERR_DEVICE;
    }
}
}  // namespace thr

namespace thr {
namespace host {

// Plain iterative radix-2 FFT in double, host side, setup only (template
// spectrum; the reference does this once in float64 too, soa_estimator.py:68-72).
void host_fft(std::vector<std::complex<double>>& a) {
    const size_t n = a.size();
    for (size_t i = 1, j = 0; i < n; ++i) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(a[i], a[j]);
    }
    const double pi = 3.14159265358979323846;
    for (size_t len = 2; len <= n; len <<= 1) {
        // exact-ish twiddles: evaluate each directly (no recurrence drift)
        std::vector<std::complex<double>> w(len / 2);
        for (size_t k = 0; k < len / 2; ++k)
            w[k] = std::complex<double>(std::cos(2 * pi * double(k) / double(len)),
                                        -std::sin(2 * pi * double(k) / double(len)));
        for (size_t i = 0; i < n; i += len)
            for (size_t k = 0; k < len / 2; ++k) {
                const std::complex<double> u = a[i + k], v = a[i + k + len / 2] * w[k];
                a[i + k] = u + v;
                a[i + k + len / 2] = u - v;
            }
    }
}

float2 unit_root(long long num, long long den) {  // exp(-2 pi i num/den), exact reduction
    const double pi = 3.14159265358979323846;
    num %= den;
    if (num < 0) num += den;
    const double a = 2 * pi * double(num) / double(den);
    return float2{float(std::cos(a)), float(-std::sin(a))};
}


int window_indices(int start, int stop, int n, int* lo, int* count) {
    // carrier_detect.py:17-58
    if (std::abs(start) >= n || std::abs(stop) >= n)
        return fail(THR_ERR_ARG, "Frequency window out of range: %d - %d", start, stop);
    if (start < 0 && stop >= 0) {
        start += n;
        stop += n;
    }
    if (start < 0) start += n;
    if (stop < 0) stop += n;
    if (stop < start) std::swap(start, stop);
    *lo = start;
    *count = std::min(stop - start + 1, n);
    return THR_OK;
}

// Overlap-save sections of a long block's correlate stage (detect_seg.hip).  A section is 16384
// samples; against a W-sample template its lags 0 .. V - 1, V = 16384 - W + 1, are exact lags of
// the block (soa_estimator.py:97-102 keeps only lags that do not wrap).  Sections start every D
// samples, D = the largest even number <= V - 2 (even: u8 samples are fetched as 4-byte pairs; - 2:
// a section must also hold the lag below and the lag above every lag it owns, for the peak's
// neighbours, soa_estimator.py:159-170), the last one at block_len - 16384.  Section g > 0 owns the
// block's lags from its start + 1 up to the next section's start; section 0 owns lag 0 too, the
// last one everything up to corr_len.  Returns false (d.n_seg = 0) when the block needs more than
// kMaxSections -- templates longer than about half a section: the decimated kernels keep those.
bool plan_sections(thr::DevCfg& d, int template_len) {
    const int m = 16384, n = d.block_len;
    d.n_seg = 0;
    const int v = m - template_len + 1;
    if (n <= m || v < 4) return false;
    const int stride = (v - 2) & ~1;
    const int n_seg = (n - m + stride - 1) / stride + 1;
    if (n_seg > thr::kMaxSections) return false;
    int own_lo = 0;   // first lag of the block section g owns
    for (int g = 0; g < n_seg; ++g) {
        const int start = std::min(g * stride, n - m);
        const int own_hi = g + 1 < n_seg ? std::min((g + 1) * stride, n - m) + 1 : d.corr_len;
        d.seg_start[g] = start;
        d.seg_sum_lo[g] = own_lo - start;
        d.seg_sum_hi[g] = own_hi - start;
        d.seg_lo[g] = std::max(own_lo, d.corr_lo) - start;
        d.seg_hi[g] = std::max(std::min(own_hi, d.corr_hi), std::max(own_lo, d.corr_lo)) - start;
        own_lo = own_hi;
    }
    d.n_seg = n_seg;
    return true;
}

// The same idea one size down (detect16k_sec.hip): a 16384-sample block whose template is short
// enough that FOUR 4096-sample sections or fewer cover its unique window [corr_lo, corr_hi) -- then
// the sections' transforms cost less than the block's (4 x 4096 x 12 < 16384 x 14 butterfly
// stages).  Only the window is covered (no stddev term on this path: its sums run over every kept
// lag).  A section holds V = 4096 - W + 1 exact lags; it owns at most V - 2 of them (the lag below
// and the lag above every owned lag must be in it too, for the peak's neighbours,
// soa_estimator.py:159-170 -- except at the two ends of the kept lags, where the reference takes no
// neighbours either).  Sections start on multiples of 8 samples (u8 samples are fetched 16 bytes
// per thread), every D = (V - 2) & ~7 samples from the last multiple of 8 at or below corr_lo - 1,
// the last one no later than block_len - 4096.  BASELINE (history 4096, 1023 samples): starts
// 1536 + 3072 g, every section owns its lags [1, 3073).
bool plan_sections_4k(thr::DevCfg& d, int template_len) {
    const int m = 4096, n = d.block_len;
    d.n_seg = 0;
    const int v = m - template_len + 1;
    if (n != 16384 || v < 16) return false;
    const int stride = (v - 2) & ~7;
    const int s0 = std::max(d.corr_lo - 1, 0) & ~7;
    int own_lo = d.corr_lo, g = 0;
    while (own_lo < d.corr_hi) {
        if (g == 4) return false;      // a fifth section: the 16384-point kernel is cheaper
        const int start = std::min(s0 + g * stride, n - m);
        // lags [start, start + v) are in the section; it owns from the previous section's end up to its
        // last lag but one -- or up to its last lag, where that is the last kept lag of the block
        const int cap = start + v == d.corr_len ? d.corr_len : start + v - 1;
        const int own_hi = std::min(cap, d.corr_hi);
        if (own_hi <= own_lo || (own_lo > 0 && own_lo - 1 < start)) return false;
        d.seg_start[g] = start;
        d.seg_lo[g] = own_lo - start;
        d.seg_hi[g] = own_hi - start;
        d.seg_sum_lo[g] = d.seg_sum_hi[g] = 0;
        own_lo = own_hi;
        ++g;
    }
    d.n_seg = g;
    return g > 0;
}

namespace {

// a host array into a device array of its own
template <class T, class U>
int upload(Dev<T>& owner, const std::vector<U>& v) {
    HIP_TRY(owner.alloc(v.size() * sizeof(U)));
    HIP_TRY(hipMemcpy(owner, v.data(), v.size() * sizeof(U), hipMemcpyHostToDevice));
    return THR_OK;
}

using Spectrum = std::vector<std::complex<double>>;

Spectrum template_fft(const thr_handle* h, int t, int len) {     // FFT(template t zero-padded to len)
    const int w = h->cfg.template_len;
    Spectrum buf(len, 0.0);
    for (int i = 0; i < w; ++i) buf[i] = h->cfg.templates[size_t(t) * w + i];
    host_fft(buf);
    return buf;
}

float2 conj_over(const std::complex<double>& v, int n) {
    const std::complex<double> c = std::conj(v) / double(n);
    return float2{float(c.real()), float(c.imag())};
}

// conj(spec[first + step * k]) / n for the 16384 bins k, in the digit-reversed, lane-coalesced order
// k_correlate consumes: thread tid holds k = (tid >> 5) + 16 (tid & 31) + 512 k3
void permute_16k(float2* out, const Spectrum& spec, int first, int step, int n) {
    for (int tid = 0; tid < 512; ++tid)
        for (int k3 = 0; k3 < 32; ++k3) {
            const int k = (tid >> 5) + 16 * (tid & 31) + 512 * k3;
            out[((k3 >> 1) * 512 + tid) * 2 + (k3 & 1)] = conj_over(spec[first + step * k], n);
        }
}

// the short-block layout: thread column c = k1 * 32 + k2 (k1 < r1) holds bins k1 + r1 k2 + tb k3, tb = 32 r1;
// float4 j of the column = k3 in {2j, 2j + 1}, stored [j][c] for coalescing
void permute_short(float2* out, const Spectrum& spec, int r1, int tb, int n) {
    for (int c = 0; c < tb; ++c)
        for (int k3 = 0; k3 < 32; ++k3) {
            const int k = (c >> 5) + r1 * (c & 31) + tb * k3;
            out[((k3 >> 1) * tb + c) * 2 + (k3 & 1)] = conj_over(spec[k], n);
        }
}

}  // namespace

int build_constants(thr_handle* h) {
    const int n = h->cfg.block_len;
    // --- LDS twiddle tables (forward sign): C[32][32], A[16][32], Bt[16][32]  (fast path)
    std::vector<float2> tab(2048);
    for (int a = 0; a < 32; ++a)
        for (int b = 0; b < 32; ++b) tab[a * 32 + b] = unit_root((long long)a * b, 1024);
    for (int k1 = 0; k1 < 16; ++k1)
        for (int n2 = 0; n2 < 32; ++n2) tab[1024 + k1 * 32 + n2] = unit_root((long long)k1 * n2, 512);
    for (int k1 = 0; k1 < 16; ++k1)
        for (int mp = 0; mp < 32; ++mp)
            tab[1536 + k1 * 32 + mp] = unit_root((long long)k1 * mp, h->lng ? 16384 : n);
    THR_TRY(upload(h->d_tables, tab));
    // --- pass-1 / pass-B twiddles W_16384^(k1 q) of k_correlate and of the
    //     short-block kernels as one L2-resident table in global memory
    h->dev.gtw = nullptr;
    if (h->small || h->fast || h->seg || h->sec4k) {
        std::vector<float2> g(2 * 16 * 1024);
        for (int k1 = 0; k1 < 16; ++k1)
            for (int q = 0; q < 1024; ++q) g[k1 * 1024 + q] = unit_root((long long)k1 * q, 16384);
        // the same table again in the PAIRS a thread of pass B reads (thread n3 of row k1 needs
        // W^(k1 (32 n2 + n3)) for n2 = 0 .. 31): [(k1 * 16 + j) * 32 + n3] = (n2 = 2 j, n2 = 2 j + 1) --
        // sixteen 16-byte loads instead of thirty-two 8-byte ones (passes_w8.hpp: inv_passB)
        for (int k1 = 0; k1 < 16; ++k1)
            for (int j = 0; j < 16; ++j)
                for (int n3 = 0; n3 < 32; ++n3)
                    for (int e = 0; e < 2; ++e)
                        g[16 * 1024 + ((k1 * 16 + j) * 32 + n3) * 2 + e] =
                            unit_root((long long)k1 * (32 * (2 * j + e) + n3), 16384);
        THR_TRY(upload(h->d_gtw, g));
        h->dev.gtw = h->d_gtw;
    }
    // --- full-length root table for the shift phasor
    std::vector<float2> tw(n);
    for (int j = 0; j < n; ++j) tw[j] = unit_root(j, n);
    THR_TRY(upload(h->d_twn, tw));
    // --- template spectra: conj(FFT(zero-padded template)) / N, in the order the path's correlate
    //     kernel consumes
    const int w = h->cfg.template_len, nt = h->cfg.n_templates;
    std::vector<float2> spec(size_t(nt) * n);
    for (int t = 0; t < nt; ++t) {
        double energy = 0;
        for (int i = 0; i < w; ++i) {
            const double v = h->cfg.templates[size_t(t) * w + i];
            energy += v * v;
        }
        h->dev.tmpl_energy[t] = float(energy);
        const Spectrum buf = template_fft(h, t, n);
        float2* out = spec.data() + size_t(t) * n;
        if (h->lng) {
            // sub-transform k0 holds bins k0 + R0*q; within it the 16384 kernels' permutation
            const int r0 = n / 16384;
            for (int k0 = 0; k0 < r0; ++k0) permute_16k(out + size_t(k0) * 16384, buf, k0, r0, n);
        } else if (h->small) {
            permute_short(out, buf, n / 1024, 32 * (n / 1024), n);
        } else if (h->fast) {
            permute_16k(out, buf, 0, 1, n);
        } else {
            for (int k = 0; k < n; ++k) out[k] = conj_over(buf[k], n);
        }
    }
    if (h->seg) {
        // sectioned correlate stage: the template zero-padded to 16384, as for block_len 16384
        const int m = 16384;
        std::vector<float2> s16(size_t(nt) * m);
        for (int t = 0; t < nt; ++t) permute_16k(s16.data() + size_t(t) * m, template_fft(h, t, m), 0, 1, m);
        THR_TRY(upload(h->d_tspec16k, s16));
    }
    if (h->sec4k) {
        // 4096-sample sections of a 16384-sample block: the template zero-padded to 4096, thread column
        // c = row * 32 + k2 holds bins row + 4 k2 + 128 k3 (the short-block layout, R1 = 4)
        const int m = 4096;
        std::vector<float2> s4(size_t(nt) * m);
        for (int t = 0; t < nt; ++t) permute_short(s4.data() + size_t(t) * m, template_fft(h, t, m), 4, 128, m);
        THR_TRY(upload(h->d_tspec4k, s4));
        if (nt > 1) {
            // the C table in pairs, for the kernel form that re-reads its twiddle column every pass
            std::vector<float2> cp(1024);
            for (int j = 0; j < 16; ++j)
                for (int c = 0; c < 32; ++c) {
                    cp[(j * 32 + c) * 2] = tab[(2 * j) * 32 + c];
                    cp[(j * 32 + c) * 2 + 1] = tab[(2 * j + 1) * 32 + c];
                }
            THR_TRY(upload(h->d_ctab_pair, cp));
            const size_t pb = thr::park_bytes_4k(4 * h->n_cu);
            if (pb) HIP_TRY(h->d_park.alloc(pb));
        }
    }
    if (nt == 0) return THR_OK;     // carrier gate: no template spectra
    return (h->fast || h->lng || h->small) ? upload(h->d_tspec, spec) : upload(h->d_tspec_nat, spec);
}

// Pre-shifted template spectra of the PreshiftDetector variant (detect_preshift.py:24-40):
// conj(FFT(template_padded * exp(-2 pi i shift_j (n/N - 1/2)))) / N, shift_j = linspace(-.5, .5, num).
int build_preshift_bank(thr_handle* h) {
    const int n = h->cfg.block_len, w = h->cfg.template_len, num = h->preshift_num;
    std::vector<float2> bank(size_t(num) * n);
    const double pi = 3.14159265358979323846;
    for (int j = 0; j < num; ++j) {
        // (fastdet-compatible variant: ONE unshifted template spectrum)
        const double shift = h->dev.variant == 2 ? 0.0 : num > 1 ? -0.5 + double(j) / double(num - 1) : -0.5;
        std::vector<std::complex<double>> buf(n, 0.0);
        for (int i = 0; i < w; ++i) {
            const double ph = -2.0 * pi * shift * (double(i) / double(n) - 0.5);
            buf[i] = h->cfg.templates[i] * std::complex<double>(std::cos(ph), std::sin(ph));
        }
        host_fft(buf);
        float2* out = bank.data() + size_t(j) * n;
        for (int k = 0; k < n; ++k) {
            // 16384 kernel: bin k = k1 + 16 k2 + 512 k3 lives at (k3 * 16 + k1) * 32 + k2
            const int pos = h->fast ? (((k >> 9) * 16 + (k & 15)) * 32 + ((k >> 4) & 31)) : k;
            out[pos] = conj_over(buf[k], n);
        }
    }
    return upload(h->d_bank, bank);
}


}  // namespace host
}  // namespace thr

extern "C" {

int thr_abi_version(void) { return THR_ABI_VERSION; }

const char* thr_last_error(void) { return g_last_error.c_str(); }

const char* thr_kernel_name(int slot) {
    static const char* names[THR_N_KERNEL_SLOTS] = {"k_carrier", "k_fit",    "k_correlate",
                                                    "k_finish",  "k_correlate_sub+k_combine (small batches)"};
    return (slot >= 0 && slot < THR_N_KERNEL_SLOTS) ? names[slot] : "";
}

static int create_impl(const thr_settings* s, int preshift_num, thr_handle** out, int variant = -1,
                       int path = THR_PATH_AUTO, int interp = 0);

int thr_create(const thr_settings* s, thr_handle** out) { return create_impl(s, 0, out); }

static int create_fastdet(const thr_settings* s, thr_handle** out, int path) {
    if (!s || !out) return fail(THR_ERR_ARG, "thr_create_fastdet: null argument");
    if (s->n_templates != 1) return fail(THR_ERR_ARG, "the fastdet variant takes exactly one template");
    if (s->carrier_thresh[2] != 0.0 || s->corr_thresh[2] != 0.0)
        return fail(THR_ERR_ARG, "fastdet thresholds are constant + snr * noise_power (no stddev term)");
    if (s->carrier_window[0] < 0 && s->carrier_window[1] >= 0)   // cardet.c:44-48
        return fail(THR_ERR_ARG, "Carrier frequency window range not supported.");
    return create_impl(s, 1, out, 2, path);
}

// Carrier gate (fastcard's verdict, cardet.c:7-70): the carrier stage and nothing behind it.  The
// window is cardet_normalize_window's -- inclusive, never wrapping -- and goes to the carrier kernels as
// (first bin, count); thresholds are float32 like fargs_t's.
static int create_gate(const thr_settings* s, thr_handle** out, int path) {
    if (!s || !out) return fail(THR_ERR_ARG, "thr_create_ex: null argument");
    if (s->n_templates != 0 || s->templates)
        return fail(THR_ERR_ARG, "the gate variant takes no templates (n_templates = 0, templates = NULL)");
    if (s->carrier_thresh[2] != 0.0)
        return fail(THR_ERR_ARG, "the gate threshold is constant + snr * noise_power (no stddev term)");
    const int n = s->block_len;
    int lo = s->carrier_window[0], hi = s->carrier_window[1];
    if (lo < 0 && hi >= 0)                                        // cardet.c:44-48
        return fail(THR_ERR_ARG, "Carrier frequency window range not supported.");
    if (lo < 0) lo += n;
    if (hi < 0) hi += n;
    if (n > 0 && (lo < 0 || hi < 0 || lo >= n || hi >= n))        // cardet.c:57-62
        return fail(THR_ERR_ARG, "Carrier frequency window out of range.");
    return create_impl(s, 0, out, THR_VARIANT_GATE, path);
}

int thr_create_fastdet(const thr_settings* s, thr_handle** out) try {
    return create_fastdet(s, out, THR_PATH_AUTO);
} catch (...) {
    return thr::on_exception("thr_create_fastdet");
}

static int create_preshift(const thr_settings* s, int num_arg, thr_handle** out, int path) {
    const int num_shifts = num_arg & 0xFFFF, interp = (num_arg >> 16) & 0xFFFF;
    if (num_arg < 0 || interp > THR_INTERP_COSINE)
        return fail(THR_ERR_ARG, "unknown carrier interpolator %d", interp);
    if (num_shifts < 1 || num_shifts > 4096)
        return fail(THR_ERR_ARG, "num_shifts %d out of range [1, 4096]", num_shifts);
    if (s && s->n_templates != 1)
        return fail(THR_ERR_ARG, "the preshift variant takes exactly one template");
    return create_impl(s, num_shifts, out, -1, path, interp);
}

int thr_create_preshift(const thr_settings* s, int num_shifts, thr_handle** out) try {
    return create_preshift(s, num_shifts, out, THR_PATH_AUTO);
} catch (...) {
    return thr::on_exception("thr_create_preshift");
}


int thr_debug_correlate_geom(thr_handle* h, int* rows_lo, int* rows_hi) try {
    if (!h || !rows_lo || !rows_hi) return fail(THR_ERR_ARG, "thr_debug_correlate_geom: null argument");
    *rows_lo = *rows_hi = -1;
    int lo = -1, hi = -1;
    bool got = false;
    if (h->fast && !h->preshift_num)
        got = thr::correlate_geom_16k(h->dev, &lo, &hi);
    else if (h->seg)
        got = thr::correlate_geom_seg(h->dev, &lo, &hi);
    if (got) {
        *rows_lo = lo;
        *rows_hi = hi;
    }
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_correlate_geom");
}

int thr_debug_sections(thr_handle* h, int* n_sections, int* section_len) try {
    if (!h || !n_sections || !section_len) return fail(THR_ERR_ARG, "thr_debug_sections: null argument");
    *n_sections = (h->seg || h->sec4k) ? h->dev.n_seg : 0;
    *section_len = h->sec4k ? 4096 : h->seg ? 16384 : 0;
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_sections");
}

int thr_debug_section_counts(thr_handle* h, long long* computed, long long* skipped) try {
    if (!h || !computed || !skipped) return fail(THR_ERR_ARG, "thr_debug_section_counts: null argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    unsigned n[2] = {0u, 0u};   // d_work_count[2], [3]: k_correlate_4k adds to them, nothing else re-arms them
    HIP_TRY(hipMemcpyAsync(n, h->d_work_count.p + 2, sizeof n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemsetAsync(h->d_work_count.p + 2, 0, sizeof n, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *computed = (long long)n[0];
    *skipped = (long long)n[1];
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_section_counts");
}

int thr_get_path_info(thr_handle* h, thr_path_info* out) try {
    if (!h || !out) return fail(THR_ERR_ARG, "thr_get_path_info: null argument");
    std::memset(out, 0, sizeof(*out));
    out->n_templates = h->cfg.n_templates;
    out->n_sections = (h->seg || h->sec4k) ? h->dev.n_seg : 0;
    out->section_len = h->sec4k ? 4096 : h->seg ? 16384 : 0;
    out->why_unsectioned = h->why_unsectioned;
    out->rows_lo = out->rows_hi = -1;
    const int n = h->cfg.block_len;
    const char* car;
    const char* cor;
    if (h->preshift_num && h->fast) {
        car = cor = "k_preshift";
    } else if (h->fast) {
        car = h->dev.car_prune == 1 ? "k_carrier_pruned" : h->dev.car_prune == 2 ? "k_carrier_pruned (pre-shifted window)"
                                                                                  : "k_carrier";
        cor = h->sec4k ? "k_correlate_4k" : "k_correlate";
        if (!h->sec4k) thr::correlate_geom_16k(h->dev, &out->rows_lo, &out->rows_hi);
    } else if (h->lng && !h->preshift_num) {
        const thr::LongCarrierForm form = thr::long_carrier_form(h->dev, false);
        car = form == thr::kLongCarDit          ? "k_carrier_dit+k_select_dit"
              : form == thr::kLongCarSubPruned ? "k_carrier_sub_pruned+k_select"
                                                : "k_carrier_sub+k_select";
        cor = h->seg ? "k_correlate_seg" : "k_correlate_sub";
        if (h->seg) thr::correlate_geom_seg(h->dev, &out->rows_lo, &out->rows_hi);
    } else if (h->small) {
        car = "k_carrier_small";
        cor = "k_correlate_small";
    } else {
        car = "g_* (multi-pass)";
        cor = "g_* (multi-pass)";
    }
    if (thr_is_gate(h)) {      // carrier gate: the carrier stage, then k_gate_verdict + k_b64_encode (card_gate.hip)
        cor = "none";
        out->rows_lo = out->rows_hi = -1;
    }
    std::snprintf(out->carrier_kernel, sizeof(out->carrier_kernel), "%s", car);
    std::snprintf(out->correlate_kernel, sizeof(out->correlate_kernel), "%s", cor);
    static const char* const why[] = {
        "",
        "the handle was created with an unsectioned / multi-pass kernel path",
        "preshift / fastdet variant: one fused kernel per block",
        "corr_thresh has a stddev term, whose sums run over every kept lag",
        "the unique window of this history / template length needs more sections than pay",
        "this block length has no sectioned form"};
    if (thr_is_gate(h))
        std::snprintf(out->text, sizeof(out->text),
                      "block_len %d, carrier gate: carrier stage %s, then k_gate_verdict + k_b64_encode; no correlate stage",
                      n, car);
    else if (out->n_sections)
        std::snprintf(out->text, sizeof(out->text),
                      "block_len %d, %d template(s): carrier stage %s, correlate stage %s in %d sections of %d samples",
                      n, h->cfg.n_templates, car, cor, out->n_sections, out->section_len);
    else if (out->rows_lo >= 0)
        std::snprintf(out->text, sizeof(out->text),
                      "block_len %d, %d template(s): carrier stage %s, correlate stage %s (window rows %d, %d), "
                      "unsectioned: %s",
                      n, h->cfg.n_templates, car, cor, out->rows_lo, out->rows_hi, why[h->why_unsectioned]);
    else
        std::snprintf(out->text, sizeof(out->text),
                      "block_len %d, %d template(s): carrier stage %s, correlate stage %s, unsectioned: %s", n,
                      h->cfg.n_templates, car, cor, why[h->why_unsectioned]);
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_get_path_info");
}


int thr_plan_sections(int block_len, int history_len, int template_len, int* n_sections, int* start,
                      int* win_lo, int* win_hi, int* sum_lo, int* sum_hi) try {
    if (!n_sections || !start || !win_lo || !win_hi || !sum_lo || !sum_hi)
        return fail(THR_ERR_ARG, "thr_plan_sections: null argument");
    if (block_len <= 0 || (block_len & (block_len - 1)) || template_len < 1 || template_len > block_len ||
        history_len < template_len - 1 || history_len >= block_len)
        return fail(THR_ERR_ARG, "thr_plan_sections: bad geometry (%d, %d, %d)", block_len, history_len,
                    template_len);
    thr::DevCfg d{};
    d.block_len = block_len;
    d.corr_len = block_len - template_len + 1;
    const int pad = history_len - template_len + 1;   // soa_estimator.py:20-39
    d.corr_lo = pad / 2;
    d.corr_hi = d.corr_len - (pad - pad / 2);
    if (block_len == 16384)
        plan_sections_4k(d, template_len);   // (4096-sample sections; the sums are not sectioned: 0, 0)
    else
        plan_sections(d, template_len);
    *n_sections = d.n_seg;
    for (int g = 0; g < d.n_seg; ++g) {
        start[g] = d.seg_start[g];
        win_lo[g] = d.seg_lo[g] + d.seg_start[g];
        win_hi[g] = d.seg_hi[g] + d.seg_start[g];
        sum_lo[g] = d.seg_sum_lo[g] + d.seg_start[g];
        sum_hi[g] = d.seg_sum_hi[g] + d.seg_start[g];
    }
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_plan_sections");
}

int thr_create_ex(const thr_settings* s, int variant, int variant_arg, int path, thr_handle** out) try {
    if (path != THR_PATH_AUTO && path != THR_PATH_MULTIPASS && path != THR_PATH_UNSECTIONED &&
        path != THR_PATH_GENERIC_ROWS && path != THR_PATH_UNSECTIONED_GENERIC_ROWS)
        return fail(THR_ERR_ARG, "thr_create_ex: unknown path %d", path);
    switch (variant) {
        case THR_VARIANT_DEFAULT: return create_impl(s, 0, out, -1, path);
        case THR_VARIANT_PRESHIFT: return create_preshift(s, variant_arg, out, path);
        case THR_VARIANT_FASTDET: return create_fastdet(s, out, path);
        case THR_VARIANT_GATE: return create_gate(s, out, path);
    }
    return fail(THR_ERR_ARG, "thr_create_ex: unknown variant %d", variant);
} catch (...) {
    return thr::on_exception("thr_create_ex");
}


static int create_body(const thr_settings* s, int preshift_num, thr_handle** out, int variant, int path, int interp);

static int create_impl(const thr_settings* s, int preshift_num, thr_handle** out, int variant, int path,
                       int interp) try {
    if (!s || !out) return fail(THR_ERR_ARG, "thr_create: null argument");
    *out = nullptr;
    return create_body(s, preshift_num, out, variant, path, interp);
} catch (...) {
    return thr::on_exception("thr_create");
}

// Every return before the last one, and an exception (host memory), gives back what the handle had taken:
// `h` owns it until it is released into *out.
static int create_body(const thr_settings* s, int preshift_num, thr_handle** out, int variant, int path,
                       int interp) {
    const int n = s->block_len;
    if (n <= 0 || (n & (n - 1))) return fail(THR_ERR_ARG, "block_len %d is not a power of two", n);
    if (n < 64 || n > (1 << 20))
        return fail(THR_ERR_ARG, "block_len %d out of range [64, 1048576]", n);
    const bool gate = variant == THR_VARIANT_GATE;
    if (gate) {
        if (s->history_len < 0 || s->history_len >= n)
            return fail(THR_ERR_ARG, "history_len %d must satisfy 0 <= history_len < block_len", s->history_len);
    } else if (s->n_templates < 1 || s->n_templates > thr::kMaxTemplates)
        return fail(THR_ERR_ARG, "n_templates %d out of range [1, %d]", s->n_templates,
                    thr::kMaxTemplates);
    else if (!s->templates || s->template_len < 1 || s->template_len > n)
        return fail(THR_ERR_ARG, "bad template (len %d)", s->template_len);
    else if (s->history_len < s->template_len - 1 || s->history_len >= n)
        return fail(THR_ERR_ARG, "history_len %d must satisfy template_len-1 <= history_len < block_len",
                    s->history_len);  // soa_estimator.py:32 asserts the lower bound
    if (s->max_batch < 1) return fail(THR_ERR_ARG, "max_batch must be >= 1");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(THR_ERR_DEVICE, "no HIP device available (this engine has no CPU fallback)");
    if (s->device_id < 0 || s->device_id >= ndev)
        return fail(THR_ERR_ARG, "device_id %d out of range (%d devices)", s->device_id, ndev);

    thr_gate_handle* gh = gate ? new thr_gate_handle() : nullptr;
    std::unique_ptr<thr_handle, HandleDeleter> h(gate ? gh : new thr_handle());
    h->cfg = *s;
    h->cfg.templates = nullptr;  // not retained beyond this call (re-pointed below)
    if (gate) {
        h->cfg.n_templates = h->cfg.template_len = 0;
        gh->gate_c = float(s->carrier_thresh[0]);
        gh->gate_s = float(s->carrier_thresh[1]);
    }
    h->device = s->device_id;
    h->preshift_num = preshift_num;
    h->path = path;
    const bool multipass = path == THR_PATH_MULTIPASS;
    h->fast = (n == 16384) && !multipass;
    // the preshift variant has a fused kernel for 16384 only; other lengths use the multi-pass pipeline
    h->lng = thr::long_supported(n) && !multipass && !preshift_num;
    if (hipSetDevice(h->device) != hipSuccess)
        return fail(THR_ERR_DEVICE, "hipSetDevice(%d) failed", h->device);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) != hipSuccess)
        return fail(THR_ERR_DEVICE, "hipGetDeviceProperties failed");
    h->n_cu = prop.multiProcessorCount;
    if ((h->fast || h->lng || thr::small_supported(n)) &&
        size_t(prop.maxSharedMemoryPerMultiProcessor) < thr::lds_bytes_16k())
        return fail(THR_ERR_DEVICE, "device has %zu B LDS per CU, need %zu",
                    size_t(prop.maxSharedMemoryPerMultiProcessor), thr::lds_bytes_16k());
    thr::DevCfg& d = h->dev;
    d.block_len = n;
    d.history_len = s->history_len;
    d.n_templates = s->n_templates;
    d.carrier_len = s->carrier_len > 0 ? s->carrier_len : s->template_len;
    if (gate) {       // cardet_normalize_window (checked by create_gate): [min, max], swapped if reversed
        int lo = s->carrier_window[0], hi = s->carrier_window[1];
        if (lo < 0) lo += n;
        if (hi < 0) hi += n;
        d.n_templates = 0;
        d.carrier_len = 1;
        d.win_lo = std::min(lo, hi);
        d.win_count = std::abs(hi - lo) + 1;
    } else
        THR_TRY(window_indices(s->carrier_window[0], s->carrier_window[1], n, &d.win_lo, &d.win_count));
    // soa_estimator.py:20-39
    const int corr_len = n - s->template_len + 1;
    const int pad = s->history_len - s->template_len + 1;
    d.corr_lo = pad / 2;
    d.corr_hi = corr_len - (pad - pad / 2);
    d.corr_len = corr_len;
    if (!gate && d.corr_hi <= d.corr_lo)
        return fail(THR_ERR_ARG, "empty correlation window [%d, %d)", d.corr_lo, d.corr_hi);
    for (int i = 0; i < 3; ++i) {
        d.car_thr[i] = s->carrier_thresh[i];
        d.cor_thr[i] = s->corr_thresh[i];
    }
#ifdef THR_DEV
    if (h->d_timeline.alloc(128 * sizeof(unsigned long long)) == hipSuccess)
        hipMemset(h->d_timeline, 0, 128 * sizeof(unsigned long long));
    d.timeline = h->d_timeline;
#endif
    d.variant = variant >= 0 ? variant : (preshift_num ? 1 : 0);     // (THR_VARIANT_GATE: the tag of a thr_gate_handle)
    d.interp = d.variant == 1 ? interp : 0;
    d.car_want_std = !gate && s->carrier_thresh[2] != 0.0;     // (the gate has no stddev term)
    d.car_prune = 0;
    bool prune_ok = !d.car_want_std;
#ifdef THR_DEV
    if (getenv("THR_NO_PRUNE")) prune_ok = false;   // dev A/B: the full-spectrum carrier kernel
#endif
    if (prune_ok) {
        // long blocks: R0 sub-transforms, each pruned to its 128 lowest bins (mode 1 only)
        const int span = 128 * (h->lng ? n / 16384 : 1);
        if (d.win_lo >= 3 && d.win_lo + d.win_count + 3 <= span)
            d.car_prune = 1;  // window and fit margin already inside bins [0, span)
        else if (d.win_count + 6 <= 128 && !h->lng)
            d.car_prune = 2;  // any narrow window: pre-shift by win_lo - 3
    }
    d.cor_want_std = s->corr_thresh[2] != 0.0;
    d.no_row_geom = path == THR_PATH_GENERIC_ROWS || path == THR_PATH_UNSECTIONED_GENERIC_ROWS;
    h->small = thr::small_supported(n) && !multipass && !preshift_num;
    // long blocks: the correlate stage in overlap-save sections wherever the template allows
    const bool unsectioned = path == THR_PATH_UNSECTIONED || path == THR_PATH_UNSECTIONED_GENERIC_ROWS;
    h->seg = h->lng && !gate && !unsectioned && plan_sections(d, s->template_len);
    if (!h->seg) d.n_seg = 0;
    // block_len 16384, short template(s), no stddev term: the correlate stage as 4096-sample
    // sections (detect16k_sec.hip); stage dumps and every other launch keep k_correlate
    h->sec4k = h->fast && !gate && !preshift_num && d.variant == 0 && !d.cor_want_std &&
               !unsectioned && plan_sections_4k(d, s->template_len);
    if (!h->seg && !h->sec4k) d.n_seg = 0;
    // why not sectioned: the first reason that applies (thr_get_path_info)
    h->why_unsectioned = (h->seg || h->sec4k)                       ? THR_WHY_SECTIONED
                         : (multipass || unsectioned)               ? THR_WHY_PATH
                         : (preshift_num || d.variant != 0 || gate) ? THR_WHY_VARIANT
                         : !(h->fast || h->lng)                     ? THR_WHY_BLOCK_LEN
                         : (h->fast && d.cor_want_std)              ? THR_WHY_STDDEV
                                                                    : THR_WHY_GEOMETRY;

    h->cfg.templates = s->templates;
    int rc = build_constants(h.get());
    if (rc == THR_OK && preshift_num) rc = build_preshift_bank(h.get());
    h->cfg.templates = nullptr;
    if (rc != THR_OK) return rc;
    // (time domain, for thr_dossier_create's autocorrelation: the caller's array is gone after this call)
    if (s->templates && s->n_templates >= 1)
        h->tpl_time.assign(s->templates, s->templates + size_t(s->n_templates) * size_t(s->template_len));

    // (the > 64 KiB dynamic-LDS opt-in is per device and kernel, not per handle: each family of
    // kernels is prepared once per device and process -- dozens of hipFuncSetAttribute calls
    // that a second handle on the same device need not repeat)
    static std::mutex prep_mu;
    static std::vector<unsigned> prepared;      // per device: bit per kernel family / block length
    auto once = [&](unsigned bit, auto&& fn) -> hipError_t {
        std::lock_guard<std::mutex> lk(prep_mu);
        if (prepared.size() <= size_t(h->device)) prepared.resize(size_t(h->device) + 1, 0u);
        if (prepared[h->device] & bit) return hipSuccess;
        const hipError_t e = fn();
        if (e == hipSuccess) prepared[h->device] |= bit;
        return e;
    };
    const unsigned len_bit = 1u << (8 + (31 - __builtin_clz(unsigned(n))) % 20);   // (per block length)
    if (h->fast) HIP_TRY(once(1u, [] { return thr::prepare_16k(); }));
    if (h->fast && preshift_num) HIP_TRY(once(2u, [] { return thr::prepare_preshift_16k(); }));
    if (h->small) HIP_TRY(once(len_bit, [&] { return thr::prepare_small(n); }));
    if (h->seg) HIP_TRY(once(4u, [] { return thr::prepare_seg(); }));
    if (h->lng) {
        HIP_TRY(once(len_bit, [&] { return thr::prepare_long(n); }));
        const int r0 = n / 16384;
        // sub-batch: large enough to amortise the kernels' launch latency, ramps and tails
        // (the exchange rows no longer grow with it -- one row set per workgroup -- so the
        // sub-batch is as large as the small per-block buffers allow: fewer kernel ramps and
        // tails, +3.7 % from 4096 to 16384 blocks)
        h->long_batch = std::min(s->max_batch, std::max(64, 16384 / std::max(1, s->n_templates)));
        const size_t lb = size_t(h->long_batch);
        const size_t win_w = size_t(std::min(h->dev.win_count + 6, n));
        // (the decimation-in-time carrier stage parks R0 complex values per window bin here)
        HIP_TRY(h->d_win_pow.alloc(lb * win_w * sizeof(float) * 2 * r0));
        HIP_TRY(h->d_partial.alloc(lb * r0 * 2 * sizeof(float)));
        if (gate) {      // (no correlate stage: none of its exchange buffers)
            h->long_chunk = 0;
        } else {
            h->long_chunk = std::min(h->long_batch, thr::long_chunk_blocks(n, s->n_templates));
            const size_t lc = size_t(h->long_chunk);
            // (one chunk of the two-kernel form, or one row per workgroup of the fused form)
            const size_t rows = std::max(lc, size_t(std::min(h->long_batch, h->n_cu)));
            HIP_TRY(h->d_dsub.alloc(rows * s->n_templates * size_t(n) * sizeof(float2)));
            HIP_TRY(h->d_xhat_scratch.alloc(size_t(h->n_cu) * 16384 * sizeof(float2)));
        }
        if (h->seg)
            HIP_TRY(h->d_seg_stats.alloc(lb * s->n_templates * size_t(d.n_seg) * sizeof(thr::CorrStats)));
    }
    if (!h->fast && !h->lng) {
        // sub-batch so that the 3 ping-pong buffers stay near 256 MiB (Infinity-Cache sized)
        const size_t per_block = size_t(3) * n * sizeof(float2);
        h->gen_batch = int(std::max<size_t>(1, std::min<size_t>(size_t(s->max_batch),
                                                                (size_t(256) << 20) / per_block)));
        if (!h->small)   // (short blocks run LDS-resident)
            HIP_TRY(h->d_gen_scratch.alloc(thr::generic_scratch_bytes(n, h->gen_batch)));
    }
    HIP_TRY(h->own_stream.create(hipStreamNonBlocking));
    h->stream = h->own_stream;
    const size_t mb = size_t(s->max_batch);
    HIP_TRY(h->d_stats.alloc(mb * sizeof(thr::CarStats)));
    if (gate) {
        HIP_TRY(gh->d_gate_pos.alloc(mb * sizeof(int)));
        HIP_TRY(gh->d_gate_count.alloc(2 * sizeof(int)));
        HIP_TRY(gh->h_gate_count.alloc(2 * sizeof(int)));
        HIP_TRY(gh->d_gate_rec.alloc(mb * sizeof(thr_record)));
        HIP_TRY(gh->d_gate_off.alloc(2 * mb * sizeof(long long)));
    } else {
        HIP_TRY(h->d_shifts.alloc(mb * sizeof(thr::ShiftParams)));
        HIP_TRY(h->d_corr_stats.alloc(mb * s->n_templates * sizeof(thr::CorrStats)));
    }
    if (h->sec4k)
        HIP_TRY(h->d_seg_stats.alloc(mb * s->n_templates * size_t(d.n_seg) * sizeof(thr::CorrStats)));
    HIP_TRY(h->d_work_list.alloc(mb * sizeof(int)));
    HIP_TRY(h->d_work_count.alloc(4 * sizeof(int)));  // [0] work count, [1] dynamic cursor, [2] / [3] sections searched / skipped
    HIP_TRY(hipMemset(h->d_work_count, 0, 4 * sizeof(int)));  // re-armed by k_finish
    HIP_TRY(h->d_ncompact.alloc(sizeof(int)));
    *out = h.release();
    return THR_OK;
}

// The order: the device the handle lives on; nothing of the handle's may still run on its two streams; the
// window's threads stop (they call hipHostUnregister: they go while the runtime still knows the handle's
// device and before anything is freed under them); then the handle's members give back what they own --
// a gate handle's own members first (~thr_handle is virtual), then events and buffers, the streams last
// (host_internal.hpp declares them first).  A stream set with thr_set_stream is the caller's.
void thr_destroy(thr_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->own_stream) (void)hipStreamSynchronize(h->own_stream);
    if (h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);
    h->win.close();
    delete h;
}

int thr_set_wait_mode(thr_handle* h, int sleeping) try {
    if (!h) return fail(THR_ERR_ARG, "thr_set_wait_mode: null handle");
    h->sleepy_waits = sleeping != 0;
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_set_wait_mode");
}

int thr_get_settings(const thr_handle* h, thr_settings* out) try {
    if (!h || !out) return fail(THR_ERR_ARG, "thr_get_settings: null argument");
    *out = h->cfg;
    out->templates = nullptr;
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_get_settings");
}

int thr_set_stream(thr_handle* h, void* hip_stream) try {
    if (!h) return fail(THR_ERR_ARG, "null handle");
    h->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : h->own_stream;
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_set_stream");
}

int thr_set_stream_default(thr_handle* h) try {
    if (!h) return fail(THR_ERR_ARG, "null handle");
    h->stream = nullptr;   // the legacy default stream (handle value 0): ordered with every blocking stream
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_set_stream_default");
}

int thr_sync(thr_handle* h) try {
    if (!h) return fail(THR_ERR_ARG, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_sync");
}


int thr_profile_enable(thr_handle* h, int on) try {
    if (!h) return fail(THR_ERR_ARG, "null handle");
    h->prof_every = on < 0 ? 0 : on;
    h->batch_no = 0;
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_profile_enable");
}

int thr_profile_read(thr_handle* h, double ms[THR_N_KERNEL_SLOTS],
                     int64_t launches[THR_N_KERNEL_SLOTS]) try {
    if (!h || !ms || !launches) return fail(THR_ERR_ARG, "thr_profile_read: null argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int s = 0; s < THR_N_KERNEL_SLOTS; ++s) {
        for (auto& e : h->pending[s]) {
            float t = 0;
            if (hipEventElapsedTime(&t, e.a, e.b) == hipSuccess) {
                h->ms[s] += t;
                h->launches[s] += 1;
            }
            h->free_events.push_back(std::move(e));
        }
        h->pending[s].clear();
        ms[s] = h->ms[s];
        launches[s] = h->launches[s];
        h->ms[s] = 0;
        h->launches[s] = 0;
    }
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_profile_read");
}

int thr_debug_live_resources(int64_t out[4]) try {
    if (!out) return fail(THR_ERR_ARG, "thr_debug_live_resources: null argument");
    for (int k = 0; k < 4; ++k) out[k] = thr::g_live[k].load();
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_live_resources");
}

#ifdef THR_DEV
int thr_debug_timeline(thr_handle* h, unsigned long long* out128) try {
    hipSetDevice(h->device);
    hipStreamSynchronize(h->stream);
    return hipMemcpy(out128, h->dev.timeline, 128 * sizeof(unsigned long long), hipMemcpyDeviceToHost) ==
                   hipSuccess ? 0 : -2;
} catch (...) {
    return thr::on_exception("thr_debug_timeline");
}
#endif


}  // extern "C"
