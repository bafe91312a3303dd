// Chip-rate scan (thr_chipscan: blocks x candidate template lengths): declarations
// of chipscan.hip.  A Gold-code template of the reference depends on the chip rate through its length L
// alone, so the candidates are integer lengths; each has its own zero padding, corr_len = 16384 - L + 1,
// window [0, corr_len) and noise term (template energy L).  Kernels:
//   k_chip_bank    one workgroup per candidate: the +-1 template from the chip array (sample i = chip
//                  (i n_chips) / L, integer), zero-padded, the forward LDS transform, conj(.) / N stored in
//                  the order k_chip_scan's threads consume it (k_correlate's template layout)
//   k_chip_scan    one workgroup per (block, group of candidates): the block's carrier-shifted spectrum in
//                  registers once, then per candidate product, inverse LDS transform, |.|^2, first maximum
//                  over the candidate's lags and the peak's two neighbours
//   k_chip_finish  one lane per (block, candidate): energy, noise, Gaussian offset, flags (log and sqrt
//                  stay out of the transform kernels)
//   k_chip_carrier one lane per block: the carrier fields of the block's record (carrier_out)
#pragma once
#include "host_internal.hpp"

namespace thr {

constexpr size_t kChipBankBudget = size_t(64) << 20;     // template bank: 128 KiB per candidate of a chunk
constexpr size_t kChipDumpBudget = size_t(256) << 20;    // a block chunk's shifted spectra, 128 KiB per block
constexpr int kChipMaxChips = 2047;                      // (i n_chips < 2^25 for every sample i < 16384)
constexpr size_t kChipSpectrumBytes = size_t(16384) * sizeof(float2);

// k_chip_scan -> k_chip_finish, one per (block, candidate) of a chunk
struct ChipStats {
    float pm2;       // |corr[pk]|^2
    float m2[3];     // |corr[pk-1 .. pk+1]|^2 (a neighbour outside [0, 16384) is not written)
    int pk;          // first maximum over the lags [0, corr_len)
    int pad[3];
};

hipError_t prepare_chipscan();
// lens: [n_cand] device array of this chunk's lengths; bank: [n_cand][8192] float4
hipError_t launch_chip_bank(const unsigned char* d_chips, int n_chips, const int* d_lens, int n_cand,
                            const float2* tables, float4* bank, hipStream_t stream);
// records: the chunk's thr_record [n_blocks][rec_stride] (flags of template 0 decide); stats:
// [n_blocks][n_cand].  groups * per_group >= n_cand: workgroup (b, g) takes candidates [g, g + 1) * per_group.
hipError_t launch_chip_scan(const float2* d_xhat, const float4* bank, const int* d_lens, int n_cand, int n_blocks,
                            int groups, int per_group, const thr_record* records, int rec_stride,
                            const float2* tables, const float2* gtw, ChipStats* stats, hipStream_t stream);
// out: [n_blocks][n_lengths], this chunk's candidates at columns [k0, k0 + n_cand); sum_x2 = sum |X^|^2 of
// block b at corr_stats[b * rec_stride].sum_x2
hipError_t launch_chip_finish(int n_blocks, int n_cand, int n_lengths, int k0, const int* d_lens,
                              const ChipStats* stats, const thr_record* records, int rec_stride,
                              const CorrStats* corr_stats, thr_chip_record* out, hipStream_t stream);
// out[b]: block b's carrier fields, block_idx = first + b
hipError_t launch_chip_carrier(int n_blocks, long long first, const thr_record* records, int rec_stride,
                               thr_record* out, hipStream_t stream);

}  // namespace thr
