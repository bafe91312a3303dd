// Template extraction (the reference's template_extract.py:36-58 on the device): declarations of
// template_extract.hip.  The detect pipeline runs unchanged; three small kernels ride behind it:
//   k_best_fold        the batch's strongest qualifying record, folded into a running best
//   k_keep_block       that block's input samples, saved before the batch's buffer is recycled
//   k_extract_template |x| over [corr_sample, corr_sample + W) of the kept block, scaled and centred
#pragma once
#include "host_internal.hpp"

namespace thr {

// The running best of an extraction, in device memory.  key = (orderable bits of the float32
// corr_energy) << 32 | ~(position in the run): the maximum of the keys is the largest energy and,
// among equal energies, the earliest block -- whatever the batching and whatever order lanes, waves
// or batches are looked at in.  key == 0: nothing has qualified (a qualifying energy's key has bit 63
// set or a non-zero high word).
struct ExtractState {
    unsigned long long key;
    unsigned long long pos;           // position of the winner in the run (blocks fed since the reset)
    unsigned long long n_qualifying;  // records that qualified so far
    double timestamp;                 // the winner's
    thr_record rec;                   // the winner's
    int improved;                     // the LAST fold replaced the winner: k_keep_block copies
    int keep_format;                  // THR_IN_* of the kept samples
};

// d_ts == nullptr: every block of the batch carries ts_all
hipError_t launch_best_fold(const thr_record* d_recs, const double* d_ts, double ts_all, int n_blocks,
                            unsigned long long base_pos, double max_offset, ExtractState* d_state,
                            hipStream_t stream);
// block i of the batch lies at d_in + i * blk_stride, blk_bytes long (both multiples of 4)
hipError_t launch_keep_block(ExtractState* d_state, const void* d_in, unsigned long long blk_stride,
                             unsigned blk_bytes, int format, unsigned long long base_pos, int n_blocks,
                             void* d_keep, hipStream_t stream);
hipError_t launch_extract_template(const ExtractState* d_state, const void* d_keep, int block_len,
                                   int template_len, double* d_out, hipStream_t stream);

#ifdef __HIPCC__
constexpr int kCutThreads = 256;      // workgroup of k_extract_template and of template_average.hip's k_avg_finish

// sum over the workgroup in a fixed tree (every thread gets it)
__device__ __forceinline__ double tree_sum(double v, double* scratch) {
    __syncthreads();
    scratch[threadIdx.x] = v;
    __syncthreads();
    for (int half = kCutThreads / 2; half > 0; half >>= 1) {
        if (int(threadIdx.x) < half) scratch[threadIdx.x] += scratch[threadIdx.x + half];
        __syncthreads();
    }
    return scratch[0];
}

// The extraction's arithmetic on magnitudes: out[0 .. w) holds them, `acc` is this thread's sum of the ones it
// wrote (i = threadIdx.x, + kCutThreads, ...).  Mean and population standard deviation by the fixed tree, times
// scale = 2 / (mean + std), minus the recomputed mean.  Returns the scale.  Stated ONCE: k_extract_template and
// k_avg_finish both call it.
__device__ __forceinline__ double scale_and_centre(double* __restrict__ out, int w, double acc, double* scratch) {
    const double mean = tree_sum(acc, scratch) / double(w);
    acc = 0;
    for (int i = threadIdx.x; i < w; i += kCutThreads) {
        const double d = out[i] - mean;
        acc += d * d;
    }
    const double sd = sqrt(tree_sum(acc, scratch) / double(w));      // ddof = 0
    const double scale = 2.0 / (mean + sd);
    acc = 0;
    for (int i = threadIdx.x; i < w; i += kCutThreads) {
        const double v = out[i] * scale;
        out[i] = v;
        acc += v;
    }
    const double mean2 = tree_sum(acc, scratch) / double(w);         // (the reference recomputes it)
    for (int i = threadIdx.x; i < w; i += kCutThreads) out[i] -= mean2;
    return scale;
}
#endif

namespace host {
// pipeline.hip calls this behind the kernels of every chunk, in front of the records' way back (the
// chunk's done event then covers it: buffer b is not refilled under k_keep_block).  Does nothing
// unless the calling thread is inside a thr_extract_feed* / thr_extract_submit* call on `h`.
int extract_after_chunk(thr_handle* h, int b, const void* d_in, int format, size_t stride, size_t first,
                        size_t nb);
// template_average.hip: extract_after_chunk calls it behind the fold and the keep when `x` has averaging armed
// (block i of the batch at d_in + i * blk_stride, u8); thr_extract_reset calls average_reset
int average_after_chunk(thr_extract* x, int b, const void* d_in, int format, size_t blk_stride, size_t nb);
int average_reset(thr_extract* x);
}  // namespace host
}  // namespace thr

struct thr_extract {
    thr_handle* h = nullptr;
    double max_offset = 0;
    Dev<thr::ExtractState> d_state;
    Dev<void> d_keep;                                    // 8 * block_len bytes
    Dev<double> d_out;                                   // [template_len]
    Pinned<double> h_ts[thr_handle::kPipeDepth];         // [max_batch]: a chunk's timestamps
    Dev<double> d_ts[thr_handle::kPipeDepth];
    unsigned long long fed = 0;                          // blocks fed since the reset
    // the call in progress (extract_after_chunk reads them)
    const double* cur_ts = nullptr;                      // [n_blocks] of the call, or nullptr: cur_ts_all
    double cur_ts_all = 0;
    // averaging (thr_extract_average, template_average.hip): nothing is allocated until it is armed
    bool avg_armed = false;
    thr_average_opts avg_opts{};
    Dev<unsigned long long> d_avg_acc;                   // [max(1, n_classes)][2][template_len]: acc_e, acc_q
    Dev<unsigned long long> d_avg_cnt;                   // thr::kAvgCounters: count[16], n_unclassified, out of range
    Dev<signed char> d_avg_cls;                          // [max_batch]: the class of a record of the batch, or -1
    Dev<double> d_avg_out;                               // [2][template_len]: template, sem
};
