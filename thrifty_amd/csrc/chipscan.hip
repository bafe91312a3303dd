// Chip-rate scan on the device: a batch of blocks against a bank of Gold-code templates of different
// lengths (definitions: chipscan.hpp), and the thr_chipscan entry points around the
// kernels.  The carrier stage, the fit and the frequency shift are the handle's own (run_batch with the
// shifted-spectrum dump into a device buffer); what is new is the template bank and the scan.
#include "chipscan.hpp"

#include "card_gate.hpp"
#include "fft_regs.hpp"
#include "passes_w8.hpp"

namespace thr {

using namespace k16;

namespace {

// Pass 1's input for k_chip_bank: the thread's samples n = n1 * 1024 + 2t, 2t + 1 of the zero-padded
// template, formed where they are consumed.  n < len keeps the chip index below n_chips.
struct ChipSamples {
    const unsigned char* chips;
    unsigned n_chips, len;
    unsigned t;
    __device__ __forceinline__ float at(unsigned n) const {
        if (n >= len) return 0.f;
        return chips[(n * n_chips) / len] ? 1.f : -1.f;
    }
    __device__ __forceinline__ void get(int n1, cpx& a, cpx& b) const {
        const unsigned n = unsigned(n1) * S1 + 2u * t;
        a = cpx{at(n), 0.f};
        b = cpx{at(n + 1u), 0.f};
    }
};

// One workgroup per candidate length: template -> forward transform -> conj(.) / N in the lane-coalesced,
// digit-reversed order k_chip_scan multiplies with (thread t, float4 j: bins kbase + 512 (2j), + 512 (2j + 1),
// kbase = (t >> 5) + 16 (t & 31); float4 index j * 512 + t -- handle.hip's permute_16k).
__global__ __launch_bounds__(NT) void k_chip_bank(const unsigned char* __restrict__ chips, int n_chips,
                                                  const int* __restrict__ lens, const cpx* __restrict__ tables,
                                                  f4* __restrict__ bank) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cpx* lds = reinterpret_cast<cpx*>(smem_raw);
    load_tables(lds, tables);
    __syncthreads();
    const int t = opaque_tid();
    const ChipSamples raw{chips, unsigned(n_chips), unsigned(lens[blockIdx.x]), unsigned(t)};
    fwd_pass1<false, false>(lds, raw, nullptr, cpx{1.f, 0.f}, cpx{1.f, 0.f});
    __syncthreads();
    fwd_pass2(lds);
    __builtin_amdgcn_sched_barrier(0);
    cpx v[R3];
    fwd_pass3(lds, v);
    constexpr float s = 1.0f / float(N);      // (a power of two: exact)
    f4* out = bank + size_t(blockIdx.x) * (N / 2) + t;
    static_for<R3 / 2>([&](auto J) {
        constexpr int j = decltype(J)::value;
        const cpx a = v[brev(2 * j, R3)], b = v[brev(2 * j + 1, R3)];
        out[j * NT] = f4{a.x * s, -a.y * s, b.x * s, -b.y * s};
    });
}

// Workgroup (b, g): block b's shifted spectrum against the candidates [g * per_group, (g + 1) * per_group)
// of the chunk.  k_correlate's template loop (correlate16k.hpp, MULTI) without its forward half: the
// spectrum is read once and stays in 64 VGPRs, every candidate costs one product, the inverse transform,
// the peak search over ITS lags [0, 16384 - L] and one reduction barrier; the next candidate's spectrum
// slice is requested before pass C of the current one.
__global__ __launch_bounds__(NT) void k_chip_scan(const cpx* __restrict__ xhat, const f4* __restrict__ bank,
                                                  const int* __restrict__ lens, int n_cand, int groups,
                                                  int per_group, const thr_record* __restrict__ records,
                                                  int rec_stride, const cpx* __restrict__ tables,
                                                  const cpx* __restrict__ gtw, ChipStats* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cpx* lds = reinterpret_cast<cpx*>(smem_raw);
    unsigned char* sc_red = reinterpret_cast<unsigned char*>(lds + OFF_S);

    const int b = int(blockIdx.x) / groups;
    const int g = int(blockIdx.x) - b * groups;
    // (uniform: the whole workgroup leaves before its first barrier; the spectrum of a block without a
    // carrier was never written)
    if (!(records[size_t(b) * rec_stride].flags & THR_FLAG_CARRIER)) return;
    const int k_lo = g * per_group;
    const int k_hi = k_lo + per_group < n_cand ? k_lo + per_group : n_cand;
    if (k_lo >= k_hi) return;

    load_tables(lds, tables);
    __syncthreads();
    int parity = 0;

    cpx xh[R3];
    {
        const int t = opaque_tid();
        const cpx* in = xhat + size_t(b) * N + ((t >> 5) + 16 * (t & 31));
        static_for<R3>([&](auto K) {
            constexpr int k3 = decltype(K)::value;
            xh[brev(k3, R3)] = in[512 * k3];
        });
    }
    f4 tq[R3 / 2];
    {
        const f4* ts = bank + size_t(k_lo) * (N / 2) + opaque_tid();
        static_for<R3 / 2>([&](auto J) { tq[decltype(J)::value] = ts[decltype(J)::value * NT]; });
    }
    for (int k = k_lo; k < k_hi; ++k) {
        const int t = opaque_tid();  // re-derive per candidate: keeps LICM off the loop body
        const unsigned win_w = unsigned(N - lens[k] + 1);   // corr_len: the lags [0, corr_len) are searched
        cpx z[R3];
        static_for<R3 / 2>([&](auto J) {
            constexpr int j = decltype(J)::value;
            const f4 q = tq[j];
            cmul2(xh[brev(2 * j, R3)], cpx{q.x, q.y}, xh[brev(2 * j + 1, R3)], cpx{q.z, q.w},
                  z[brev(2 * j, R3)], z[brev(2 * j + 1, R3)]);
        });
        // (rows whose pass-C readers are behind the previous candidate's reduction barrier)
        inv_passA(lds, z);
        __builtin_amdgcn_sched_barrier(0);
        inv_passB<true, true>(lds, gtw);
        __syncthreads();
        if (k + 1 < k_hi) {
            const f4* ts = bank + size_t(k + 1) * (N / 2) + opaque_tid();
            static_for<R3 / 2>([&](auto J) { tq[decltype(J)::value] = ts[decltype(J)::value * NT]; });
        }
        cpx c0[R1], c1[R1];
        inv_passC(lds, c0, c1);

        // |corr|^2 and the first maximum, as in k_correlate: the wave's maximum first, then the first
        // lag that holds it, one (power, ~lag) key per wave through LDS
        float pw0[R1], pw1[R1], ew0[R1], ew1[R1];
        float tmax = -1.0f;
        static_for<R1>([&](auto K) {
            constexpr int n1 = decltype(K)::value;
            pw0[n1] = cnorm(c0[brev(n1, R1)]);
            pw1[n1] = cnorm(c1[brev(n1, R1)]);
            const int n = n1 * S1 + 2 * t;
            ew0[n1] = unsigned(n) < win_w ? pw0[n1] : -1.f;
            ew1[n1] = unsigned(n + 1) < win_w ? pw1[n1] : -1.f;
            tmax = __builtin_fmaxf(tmax, __builtin_fmaxf(ew0[n1], ew1[n1]));
        });
        const float wmax = wave_max_f32(tmax);
        int first = 63;    // 2 n1 + e of the thread's first lag with the wave's maximum
        static_for<R1>([&](auto K) {
            constexpr int n1 = R1 - 1 - decltype(K)::value;
            first = ew1[n1] == wmax ? 2 * n1 + 1 : first;
            first = ew0[n1] == wmax ? 2 * n1 : first;
        });
        const unsigned lag = first == 63 ? 0xFFFFFFFFu : unsigned((first >> 1) * S1 + 2 * t + (first & 1));
        const unsigned wlag = wave_min_u32(lag);
        unsigned long long best =
            wmax < 0.f ? 0ull : ((unsigned long long)__float_as_uint(wmax) << 32) | (0xFFFFFFFFu - wlag);
        block_reduce_wave_keys<NT / 64>(best, sc_red, parity);
        parity ^= 1;
        // (best == 0: no finite power among the lags -- a spectrum of NaNs; lag 0 then)
        const int pk = best == 0ull ? 0 : int(0xFFFFFFFFu - unsigned(best & 0xFFFFFFFFu));
        // the peak's neighbours: lag n = n1 * 1024 + 2t + e, so this thread holds pk - 1 + d iff
        // (2t + e - pk + 1 - d) mod 1024 == 0 and the row exists; lag -1 and lag 16384 have no owner
        ChipStats* cs = stats + size_t(b) * n_cand + k;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int delta = pk - 1 - (2 * t + e);
            const unsigned d = unsigned(-delta) & 1023u;
            const int n1s = (delta + int(d)) >> 10;
            const bool owner = d < 3u && n1s >= 0 && n1s < R1;
            float val = 0.f;
            static_for<R1>([&](auto K) {
                constexpr int n1 = decltype(K)::value;
                val = (n1s == n1) ? (e ? pw1[n1] : pw0[n1]) : val;
            });
            if (owner) cs->m2[d] = val;
        }
        if (t == 0) {
            cs->pm2 = __uint_as_float(unsigned(best >> 32));
            cs->pk = pk;
        }
    }
}

// soa_estimator.py:78-170 with thresh_coeffs (0, 0, 0) and template_energy = L, float64 like the reference
__global__ __launch_bounds__(256) void k_chip_finish(int n_blocks, int n_cand, int n_lengths, int k0,
                                                     const int* __restrict__ lens,
                                                     const ChipStats* __restrict__ stats,
                                                     const thr_record* __restrict__ records, int rec_stride,
                                                     const CorrStats* __restrict__ corr_stats,
                                                     thr_chip_record* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_blocks * n_cand) return;
    const int b = i / n_cand, k = i - b * n_cand;
    thr_chip_record r;
    r.sample = -1;
    r.flags = 0u;
    r.energy = r.noise = 0.f;
    r.offset = 0.0;
    if (records[size_t(b) * rec_stride].flags & THR_FLAG_CARRIER) {
        const ChipStats cs = stats[i];
        const double n = double(N);
        const int corr_len = N - lens[k] + 1;
        const double xenergy = double(corr_stats[size_t(b) * rec_stride].sum_x2) / n;  // mean |X^|^2
        const double pm2 = double(cs.pm2);
        const double peak_mag = sqrt(pm2);
        const double noise_rms = sqrt((xenergy * double(lens[k]) - pm2) / n);
        const bool det = peak_mag > 0.0;
        double off = 0.0;
        if (det && cs.pk != 0 && cs.pk != corr_len - 1) {
            // log-parabola on magnitudes == the same formula on log |.|^2
            const double la = log(double(cs.m2[0])), lb = log(double(cs.m2[1])), lc = log(double(cs.m2[2]));
            off = 0.5 * (lc - la) / (2 * lb - la - lc);
            off = off < -0.6 ? -0.6 : off > 0.6 ? 0.6 : off;
        }
        r.sample = cs.pk;
        r.flags = THR_FLAG_CARRIER | (det ? THR_FLAG_CORR : 0u);
        r.energy = float(peak_mag);
        r.noise = float(noise_rms);
        r.offset = off;
    }
    out[size_t(b) * n_lengths + k0 + k] = r;
}

__global__ __launch_bounds__(256) void k_chip_carrier(int n_blocks, long long first,
                                                      const thr_record* __restrict__ records, int rec_stride,
                                                      thr_record* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_blocks) return;
    thr_record r = records[size_t(b) * rec_stride];
    r.block_idx = first + b;        // (the call's block index, not the chunk's)
    r.flags &= ~THR_FLAG_CORR;
    r.template_id = 0;
    r.corr_sample = -1;
    r.corr_offset = 0.0;
    r.corr_energy = r.corr_noise = 0.f;
    out[b] = r;
}

}  // namespace

hipError_t prepare_chipscan() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_chip_bank),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, int(LDS_BYTES));
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_chip_scan),
                               hipFuncAttributeMaxDynamicSharedMemorySize, int(LDS_BYTES));
}

hipError_t launch_chip_bank(const unsigned char* d_chips, int n_chips, const int* d_lens, int n_cand,
                            const float2* tables, float4* bank, hipStream_t stream) {
    hipLaunchKernelGGL(k_chip_bank, dim3(n_cand), dim3(NT), LDS_BYTES, stream, d_chips, n_chips, d_lens,
                       reinterpret_cast<const cpx*>(tables), reinterpret_cast<f4*>(bank));
    return hipGetLastError();
}

hipError_t launch_chip_scan(const float2* d_xhat, const float4* bank, const int* d_lens, int n_cand, int n_blocks,
                            int groups, int per_group, const thr_record* records, int rec_stride,
                            const float2* tables, const float2* gtw, ChipStats* stats, hipStream_t stream) {
    hipLaunchKernelGGL(k_chip_scan, dim3(n_blocks * groups), dim3(NT), LDS_BYTES, stream,
                       reinterpret_cast<const cpx*>(d_xhat), reinterpret_cast<const f4*>(bank), d_lens, n_cand,
                       groups, per_group, records, rec_stride, reinterpret_cast<const cpx*>(tables),
                       reinterpret_cast<const cpx*>(gtw), stats);
    return hipGetLastError();
}

hipError_t launch_chip_finish(int n_blocks, int n_cand, int n_lengths, int k0, const int* d_lens,
                              const ChipStats* stats, const thr_record* records, int rec_stride,
                              const CorrStats* corr_stats, thr_chip_record* out, hipStream_t stream) {
    hipLaunchKernelGGL(k_chip_finish, dim3((n_blocks * n_cand + 255) / 256), dim3(256), 0, stream, n_blocks, n_cand,
                       n_lengths, k0, d_lens, stats, records, rec_stride, corr_stats, out);
    return hipGetLastError();
}

hipError_t launch_chip_carrier(int n_blocks, long long first, const thr_record* records, int rec_stride,
                               thr_record* out, hipStream_t stream) {
    hipLaunchKernelGGL(k_chip_carrier, dim3((n_blocks + 255) / 256), dim3(256), 0, stream, n_blocks, first, records,
                       rec_stride, out);
    return hipGetLastError();
}

}  // namespace thr

namespace {

constexpr size_t kN = 16384;

size_t chip_candidates_per_chunk(const thr_handle* h, size_t n_lengths) {
    const size_t budget = h->chip.bank_budget ? h->chip.bank_budget : thr::kChipBankBudget;
    return std::min(n_lengths, std::max<size_t>(1, budget / thr::kChipSpectrumBytes));
}

// How a launch of nb blocks x nk candidates of one chunk is cut: enough workgroups for every CU twice over
// (or thr_debug_chipscan_fill's target), where the candidates allow; every group but the last walks per_group
// candidates.  The cut moves no arithmetic: a pair's result does not depend on its place in a group.
struct ChipGroups {
    size_t groups, per_group;
};
ChipGroups chip_scan_groups(const thr_handle* h, size_t nb, size_t nk) {
    const size_t fill = h->chip.fill ? h->chip.fill : 2 * size_t(h->n_cu);
    size_t groups = std::min(nk, std::max<size_t>(1, (fill + nb - 1) / nb));
    const size_t per_group = (nk + groups - 1) / groups;
    groups = (nk + per_group - 1) / per_group;
    return ChipGroups{groups, per_group};
}

// what a handle must be for the scan; `who` names the entry point in the message
int chip_handle_ok(const thr_handle* h, const char* who) {
    if (thr_is_gate(h))
        return fail(THR_ERR_STATE, "%s: a carrier-gate handle (THR_VARIANT_GATE) has no shift stage", who);
    if (h->cfg.block_len != int(kN))
        return fail(THR_ERR_ARG, "%s: block_len %d -- the chip-rate scan runs the 16384-point kernels only, other "
                                 "block lengths are not supported", who, h->cfg.block_len);
    if (!h->fast || h->preshift_num)
        return fail(THR_ERR_ARG, "%s: needs an ordinary handle (not THR_PATH_MULTIPASS, not a preshift one)", who);
    return THR_OK;
}

struct ChipTimer {      // device time of the call's three stages, summed over the chunks
    thr_handle* h;
    bool open[3] = {false, false, false};
    int begin(int stage) {
        HIP_TRY(hipEventRecord(h->chip.ev[2 * stage], h->stream));
        return THR_OK;
    }
    int end(int stage) {
        HIP_TRY(hipEventRecord(h->chip.ev[2 * stage + 1], h->stream));
        open[stage] = true;
        return THR_OK;
    }
    int collect() {     // after a stream synchronisation
        for (int s = 0; s < 3; ++s) {
            if (!open[s]) continue;
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, h->chip.ev[2 * s], h->chip.ev[2 * s + 1]));
            h->chip.ms[s] += double(ms);
            open[s] = false;
        }
        return THR_OK;
    }
};

int chipscan_body(thr_handle* h, const void* samples, int format, size_t n_blocks, const uint8_t* chips,
                  int n_chips, const int32_t* lengths, size_t n_lengths, thr_chip_record* out,
                  thr_record* carrier_out) {
    auto& c = h->chip;
    const size_t blk = kN * (format == THR_IN_U8 ? 2 : 8);
    const size_t T = size_t(h->cfg.n_templates);
    const size_t cb = std::min(size_t(h->cfg.max_batch), thr::kChipDumpBudget / thr::kChipSpectrumBytes);
    const size_t ck = chip_candidates_per_chunk(h, n_lengths);
    THR_TRY(ensure_staging(h, format));
    HIP_TRY(thr::prepare_chipscan());
    for (auto& e : c.ev)
        if (!e) HIP_TRY(e.create());
    HIP_TRY(c.d_xhat.grow(cb * thr::kChipSpectrumBytes));
    HIP_TRY(c.d_bank.grow(ck * thr::kChipSpectrumBytes));
    HIP_TRY(c.d_stats.grow(cb * ck * sizeof(thr::ChipStats)));
    HIP_TRY(c.d_out.grow(cb * n_lengths * sizeof(thr_chip_record)));
    HIP_TRY(c.d_car.grow(cb * sizeof(thr_record)));
    HIP_TRY(c.d_len.grow(n_lengths * sizeof(int)));
    HIP_TRY(c.d_chips.grow(size_t(thr::kChipMaxChips)));
    HIP_TRY(hipMemcpyAsync(c.d_len, lengths, n_lengths * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(c.d_chips, chips, size_t(n_chips), hipMemcpyHostToDevice, h->stream));
    c.ms[0] = c.ms[1] = c.ms[2] = 0.0;
    ChipTimer timer{h};
    bool bank_built = false;        // one candidate chunk: its bank serves every block chunk
    for (size_t b0 = 0; b0 < n_blocks; b0 += cb) {
        const size_t nb = std::min(cb, n_blocks - b0);
        HIP_TRY(hipMemcpyAsync(h->d_in, static_cast<const unsigned char*>(samples) + b0 * blk, nb * blk,
                               hipMemcpyHostToDevice, h->stream));
        THR_TRY(timer.begin(0));
        THR_TRY(run_batch(h, h->d_in, format, nullptr, int(nb), h->d_rec, nullptr, c.d_xhat, nullptr, 0, false));
        THR_TRY(timer.end(0));
        for (size_t k0 = 0; k0 < n_lengths; k0 += ck) {
            const size_t nk = std::min(ck, n_lengths - k0);
            if (!bank_built) {
                THR_TRY(timer.begin(1));
                HIP_TRY(thr::launch_chip_bank(c.d_chips, n_chips, c.d_len + k0, int(nk), h->d_tables, c.d_bank,
                                              h->stream));
                THR_TRY(timer.end(1));
                bank_built = ck >= n_lengths;
            }
            const ChipGroups cut = chip_scan_groups(h, nb, nk);
            THR_TRY(timer.begin(2));
            HIP_TRY(thr::launch_chip_scan(c.d_xhat, c.d_bank, c.d_len + k0, int(nk), int(nb), int(cut.groups),
                                          int(cut.per_group), h->d_rec, int(T), h->d_tables,
                                          static_cast<const float2*>(h->dev.gtw), c.d_stats, h->stream));
            HIP_TRY(thr::launch_chip_finish(int(nb), int(nk), int(n_lengths), int(k0), c.d_len + k0, c.d_stats,
                                            h->d_rec, int(T), h->d_corr_stats, c.d_out, h->stream));
            THR_TRY(timer.end(2));
            // (the next candidate chunk rewrites the bank and the statistics)
            HIP_TRY(hipStreamSynchronize(h->stream));
            THR_TRY(timer.collect());
        }
        if (carrier_out) {
            HIP_TRY(thr::launch_chip_carrier(int(nb), (long long)b0, h->d_rec, int(T), c.d_car, h->stream));
            HIP_TRY(hipMemcpyAsync(carrier_out + b0, c.d_car, nb * sizeof(thr_record), hipMemcpyDeviceToHost,
                                   h->stream));
        }
        HIP_TRY(hipMemcpyAsync(out + b0 * n_lengths, c.d_out, nb * n_lengths * sizeof(thr_chip_record),
                               hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return THR_OK;
}

}  // namespace

extern "C" {

int thr_chipscan(thr_handle* h, const void* samples, int format, size_t n_blocks, const uint8_t* chips, int n_chips,
                 const int32_t* lengths, size_t n_lengths, thr_chip_record* out, thr_record* carrier_out) try {
    if (!h || !samples || !chips || !lengths || !out) return fail(THR_ERR_ARG, "thr_chipscan: null argument");
    THR_TRY(chip_handle_ok(h, "thr_chipscan"));
    if (format != THR_IN_U8 && format != THR_IN_C64) return fail(THR_ERR_ARG, "thr_chipscan: bad format %d", format);
    if (n_blocks < 1 || n_lengths < 1)
        return fail(THR_ERR_ARG, "thr_chipscan: needs at least one block and one length (got %zu, %zu)", n_blocks,
                    n_lengths);
    if (n_lengths > (size_t(1) << 20))
        return fail(THR_ERR_ARG, "thr_chipscan: %zu lengths (at most 1048576 per call)", n_lengths);
    if (n_chips < 1 || n_chips > thr::kChipMaxChips)
        return fail(THR_ERR_ARG, "thr_chipscan: n_chips %d out of range [1, %d]", n_chips, thr::kChipMaxChips);
    for (int i = 0; i < n_chips; ++i)
        if (chips[i] > 1) return fail(THR_ERR_ARG, "thr_chipscan: chip %d is %d, not 0 or 1", i, int(chips[i]));
    for (size_t k = 0; k < n_lengths; ++k)
        if (lengths[k] < 1 || lengths[k] > int(kN) - 2)
            return fail(THR_ERR_ARG, "thr_chipscan: length %d (entry %zu) out of range [1, %d]", lengths[k], k,
                        int(kN) - 2);
    if (h->hp.async_open != 0)
        return fail(THR_ERR_STATE, "thr_chipscan: %d submitted batch(es) not collected yet", h->hp.async_open);
    HIP_TRY(hipSetDevice(h->device));
    const int rc = chipscan_body(h, samples, format, n_blocks, chips, n_chips, lengths, n_lengths, out, carrier_out);
    if (rc != THR_OK) (void)hipStreamSynchronize(h->stream);   // nothing stays enqueued behind the caller's arrays
    return rc;
} catch (...) {
    return thr::on_exception("thr_chipscan");
}

int thr_debug_chipscan_geometry(thr_handle* h, size_t n_lengths, int* candidates_per_chunk, int* paired) try {
    if (!h) return fail(THR_ERR_ARG, "thr_debug_chipscan_geometry: null handle");
    THR_TRY(chip_handle_ok(h, "thr_debug_chipscan_geometry"));
    if (candidates_per_chunk) *candidates_per_chunk = int(chip_candidates_per_chunk(h, std::max<size_t>(1, n_lengths)));
    if (paired) *paired = 0;
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_chipscan_geometry");
}

int thr_debug_chipscan_budget(thr_handle* h, size_t bank_bytes) try {
    if (!h) return fail(THR_ERR_ARG, "thr_debug_chipscan_budget: null handle");
    h->chip.bank_budget = bank_bytes;
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_chipscan_budget");
}

int thr_debug_chipscan_fill(thr_handle* h, size_t workgroups) try {
    if (!h) return fail(THR_ERR_ARG, "thr_debug_chipscan_fill: null handle");
    h->chip.fill = workgroups;
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_chipscan_fill");
}

int thr_debug_chipscan_groups(thr_handle* h, size_t n_blocks, size_t n_cand, int* groups, int* per_group) try {
    if (!h) return fail(THR_ERR_ARG, "thr_debug_chipscan_groups: null handle");
    THR_TRY(chip_handle_ok(h, "thr_debug_chipscan_groups"));
    if (n_blocks < 1 || n_cand < 1)
        return fail(THR_ERR_ARG, "thr_debug_chipscan_groups: needs at least one block and one candidate (got %zu, %zu)",
                    n_blocks, n_cand);
    const ChipGroups cut = chip_scan_groups(h, n_blocks, n_cand);
    if (groups) *groups = int(cut.groups);
    if (per_group) *per_group = int(cut.per_group);
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_chipscan_groups");
}

int thr_debug_chipscan_times(thr_handle* h, double* ms_out) try {
    if (!h || !ms_out) return fail(THR_ERR_ARG, "thr_debug_chipscan_times: null argument");
    for (int k = 0; k < 3; ++k) ms_out[k] = h->chip.ms[k];
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_chipscan_times");
}

}  // extern "C"
