// Capture survey (what an operator reads off a raw capture before detecting anything: mean |FFT|, byte
// histogram, per-block byte sums): declarations of survey.hip.  Everything that leaves the library is an
// integer, so a run gives the same bits however it is cut into calls, chunks, tiles or workgroups:
//   spec_sum[j][k] = sum over the blocks of interval j of q_b[k],  q = rint(|X_b[k]| * 2^S),  S = 30 - log2 N
//   hist[j][v]     = how often byte value v occurs in the 2N bytes of the interval's blocks
//   sums[b]        = (sum v, sum v^2) over block b's 2N bytes
// Kernels:
//   k_survey16k     block_len 16384: the carrier stage's LDS transform, folded on the chip (tiles of blocks,
//                   64-bit register accumulators, one flush per tile and interval) with the byte statistics
//                   taken from the registers the transform's input already sits in
//   k_survey_fold   every other length (and THR_PATH_MULTIPASS at 16384): the natural-order spectra the
//                   carrier stage dumps, one thread per (interval, bin), plain adds
//   k_survey_bytes  the byte statistics of that path: one workgroup per block
#pragma once
#include "host_internal.hpp"
#include "kernel_util.hpp"

namespace thr {

constexpr int kSurveyTile = 8;          // blocks per tile of k_survey16k (the flush's amortisation)
// LDS histogram: kSurveyCopies copies of the 256 counters, copy = lane & 7, laid out [value][copy] -- the
// copies of ONE value sit in 8 neighbouring banks, so a quiet capture (every lane the same value) meets 8
// addresses in 8 banks with 8 lanes each instead of one address with 64
constexpr int kSurveyCopies = 8;
constexpr size_t kSurveyHistBytes = 256 * kSurveyCopies * sizeof(unsigned);
// accumulator rows on the device (uint64[block_len] each): at most this many bytes, whatever `integrate` is
constexpr size_t kSurveyAccBudget = size_t(64) << 20;
constexpr size_t kSurveyDumpBudget = size_t(128) << 20;     // fold path: a chunk's dumped spectra
constexpr size_t kSurveyStageBudget = size_t(256) << 20;    // a chunk's input bytes
constexpr size_t kSurveyMaxRows = 32768;                    // (k_survey_fold's grid.y)

// q = rint(|x| * 2^S): v_sqrt_f32 (1 ulp), an exact power-of-two scaling, round-half-even.  |X| <= 1.41 N,
// so q < 1.52e9 fits 32 bits.
__device__ __forceinline__ unsigned survey_q(float re, float im, float scale) {
    const float m = __builtin_amdgcn_sqrtf(fmaf(re, re, im * im));
    return unsigned(__builtin_rintf(m * scale));
}

// integer wave sum on the DPP path (kernel_util.hpp's wave_sum, for unsigned)
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
    v += dpp_u32<DPP_ROW_SHR1, 0xf>(0u, v);
    v += dpp_u32<DPP_ROW_SHR2, 0xf>(0u, v);
    v += dpp_u32<DPP_ROW_SHR4, 0xf>(0u, v);
    v += dpp_u32<DPP_ROW_SHR8, 0xf>(0u, v);
    v += dpp_u32<DPP_ROW_BCAST15, 0xa>(0u, v);
    v += dpp_u32<DPP_ROW_BCAST31, 0xc>(0u, v);
    return unsigned(__builtin_amdgcn_readlane(int(v), 63));
}

// `open` blocks of the first interval were fed by earlier chunks: block b of the chunk belongs to accumulator
// row (open + b) / integrate.  d_sums: [n_blocks][2], zeroed by the caller (the waves add into it).
hipError_t prepare_survey_16k();
hipError_t launch_survey_16k(const unsigned char* d_samples, int n_blocks, unsigned long long blk_stride,
                             unsigned open, unsigned integrate, const float2* tables, unsigned long long* d_spec,
                             unsigned long long* d_hist, unsigned long long* d_sums, int grid, hipStream_t stream);
hipError_t launch_survey_fold(const float2* d_spectra, int n_blocks, int block_len, int shift, unsigned open,
                              unsigned integrate, unsigned long long* d_spec, hipStream_t stream);
hipError_t launch_survey_bytes(const unsigned char* d_samples, int n_blocks, unsigned long long blk_stride,
                               int block_len, unsigned open, unsigned integrate, unsigned long long* d_hist,
                               unsigned long long* d_sums, hipStream_t stream);

}  // namespace thr

struct thr_survey {
    thr_handle* h = nullptr;
    int integrate = 0;
    int shift = 0;                          // S
    bool fused = false;                     // k_survey16k; else the carrier stage's dump + fold + bytes
    size_t chunk_max = 0;                   // blocks per chunk at most
    size_t rows = 0;                        // accumulator rows allocated
    Dev<unsigned long long> d_spec;         // [rows][block_len]; row 0 = the open interval
    Dev<unsigned long long> d_hist;         // [rows][256]
    Dev<unsigned long long> d_sums;         // [chunk_max][2]
    Dev<float2> d_dump;                     // fold path: [chunk_max][block_len]
    unsigned long long fed = 0;             // blocks since the reset
    unsigned long long open = 0;            // of them, in the interval that is not complete yet
};
