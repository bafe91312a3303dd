// Internal header of the host side of libthriftyhip.so (include/thrifty_hip.h is the public one):
// the engine handle and its pipeline slots, ProfScope, error reporting, and the functions the host
// translation units share.  The handle OWNS what it holds: every buffer, stream and event is one of
// hip_own.hpp's types and goes back to the runtime when the handle is deleted (thr_destroy).
//   hip_own.hpp       Dev<T>, Pinned<T>, Stream, Event, DevBuf: allocation, release and the live counts
//   input_window.hpp  InputWindow, the page-locked stretch of the input file (bodies in window.hip)
//   handle.hip    error state, constants (twiddles, template spectra, section plans), thr_create* /
//                 thr_destroy, settings / path / profile queries
//   window.hip    thr_input_window* (the page-locked input file), thr_host_register
//   pipeline.hip  the double-buffered chunk pipeline (H2D staging, run_batch*, record copies)
//   entry.hip     thr_detect* / thr_submit* / thr_collect and the debug entry points
//   text.hip      host-only text routines: thr_frame_card, thr_format_toad
// (run_file.hip, identify.hip and card_ingest.hip never look inside a handle.)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <complex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <charconv>
#include <exception>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "detect_common.hpp"
#include "hip_own.hpp"
#include "input_window.hpp"

namespace thr {
struct ChipStats;     // chipscan.hpp
int fail_msg(int code, const char* fmt, ...);     // error text for thr_last_error(); returns `code`
int on_exception(const char* who) noexcept;      // the catch (...) of every entry point
namespace host {
int fail(int code, const char* fmt, ...);         // the same, for the host translation units

#define HIP_TRY(expr)                                                                  \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess)                                                          \
            return fail(THR_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr,                \
                        hipGetErrorString(_e), __FILE__, __LINE__);                    \
    } while (0)

// a status that is not THR_OK leaves the calling function
#define THR_TRY(expr)                       \
    do {                                    \
        const int rc_ = (expr);             \
        if (rc_ != THR_OK) return rc_;      \
    } while (0)

using thr::Dev;       // (the handle structs are declared at global scope)
using thr::Event;
using thr::Pinned;
using thr::Stream;

struct EventPair {
    Event a, b;
};

}  // namespace host
}  // namespace thr
using namespace thr::host;

// Members are destroyed in reverse order of declaration: BOTH streams are declared first, so every buffer
// and event has gone back before either stream does (thr_destroy, handle.hip, has the whole order).
struct thr_handle {
    Stream own_stream;
    Stream copy_stream;             // the pipeline's H2D copies (created with the pipeline, ensure_pipe)
    hipStream_t stream = nullptr;   // own_stream, or the caller's (thr_set_stream: not owned)
    thr_settings cfg{};
    thr::DevCfg dev{};
    int device = 0;
    int n_cu = 0;
    bool fast = false;       // LDS-resident 16384 kernels; else the generic multi-pass path
    bool lng = false;        // block_len = 2 or 4 x 16384: R0 LDS sub-transforms per block
    bool small = false;      // block_len = 1024 ... 8192: 16 / R1 blocks per workgroup in LDS
    int long_batch = 0;      // long path: blocks per internal sub-batch
    int long_chunk = 0;      // long path: work-list slots per correlate-stage chunk (sizes d_dsub)
    Dev<float> d_win_pow;    // long: [long_batch][win_w] |X|^2 of the window bins (+-3)
    Dev<float> d_partial;    // long: [long_batch][R0][2] partial sums of FFT#1
    Dev<float2> d_dsub;      // long: [long_chunk][T][R0][16384] sub-transform outputs
    bool seg = false;               // long: correlate stage as overlap-save sections (detect_seg.hip)
    Dev<float4> d_tspec16k;         // sectioned: templates zero-padded to 16384, k_correlate's layout
    Dev<thr::CorrStats> d_seg_stats;   // sectioned: [long_batch][T][n_seg]
    bool sec4k = false;             // block_len 16384, short template: correlate stage as 4096-sample sections (detect16k_sec.hip)
    Dev<float4> d_tspec4k;          // sec4k: the templates zero-padded to 4096, the short-block kernels' layout
    Dev<float4> d_ctab_pair;        // sec4k, several templates: C[32][32] as [j][c] = (C[2j][c], C[2j+1][c])
    Dev<float4> d_park;             // sec4k, several templates: spectrum scratch (thr::park_bytes_4k; may stay null)
    int path = 0;                   // THR_PATH_* the handle was created with
    int why_unsectioned = 0;        // THR_WHY_* (thr_get_path_info)
    int gen_batch = 0;       // generic path: blocks per internal sub-batch
    Dev<float2> d_gen_scratch;      // generic path: 3 * gen_batch * N complex
    Dev<float2> d_tspec_nat;        // generic path: conj(FFT(template))/N, natural order
    // constants
    Dev<float2> d_tables;
    Dev<float2> d_twn;
    Dev<float4> d_tspec;
    std::vector<double> tpl_time;   // the templates as given, [n_templates][template_len] (dossier.hip)
    // per-batch work buffers
    Dev<thr::CarStats> d_stats;
    Dev<thr::ShiftParams> d_shifts;
    Dev<thr::CorrStats> d_corr_stats;
    Dev<int> d_work_list;
    Dev<int> d_work_count;
    Dev<float4> d_xhat_scratch;     // long (unsectioned), several templates: one spectrum per workgroup
    Dev<int> d_ncompact;
    Dev<int> d_compact_tiles;       // per-tile counts / offsets of thr_compact_device (lazy)
#ifdef THR_DEV
    Dev<unsigned long long> d_timeline;   // behind dev.timeline
#endif
    // PreshiftDetector variant (thr_create_preshift): bank of pre-shifted template spectra
    int preshift_num = 0;       // 0 = default detector
    Dev<float2> d_gtw;          // combined twiddle table W_16384^(k1 q), L2-resident (dev.gtw is a raw alias)
    Dev<float2> d_bank;         // [num][N]; 16384: [k3][k1][k2] gather layout, else natural order
    // host-buffer entry points (thr_detect / _stream / _card): kPipeDepth sets of staging buffers so
    // that the H2D copy of chunk i + 1 (copy stream) runs under the kernels of chunk i (lazy)
    static constexpr int kPipeDepth = THR_MAX_IN_FLIGHT;
    struct Slot {
        Event ev_h2d;                 // chunk's inputs have landed (copy stream)
        Event ev_done;                // chunk's records are in h_rec (main stream)
        Dev<unsigned char> d_in;
        Dev<thr_record> d_rec;
        Pinned<thr_record> h_rec;     // pinned: D2H never blocks the host
        Dev<unsigned char> d_text;
        Dev<int> d_bad;
        // a chunk's block indices and (.card) payload offsets, packed [idx[nb] | off[nb]]: pinned on the
        // host, ONE asynchronous copy into d_idx (2 * max_batch entries; the offsets follow the indices)
        Dev<long long> d_idx;
        Pinned<long long> h_meta;
        // records of the slot's chunk still to be handed to the caller
        thr_record* pend_dst = nullptr;
        size_t pend_n = 0;
        size_t pend_first = 0;        // (first block of the chunk: error messages)
        bool pend_card = false;
        // thr_submit*() / thr_collect(): the ticket the pending chunk belongs to (0: none / a chunk of
        // the synchronous entry points)
        uint64_t ticket = 0;
        // input window: the chunk's source range [win_lo, win_end) (win_end 0: not windowed).  Chunks of a
        // raw stream OVERLAP by the history: what may be unlocked behind a finished chunk ends where the
        // earliest chunk still open begins, not where the finished one ended.
        uintptr_t win_lo = 0, win_end = 0;
    };
    struct HostPipe {
        bool ready = false;
        Pinned<int> h_bad;            // int[kPipeDepth]
        Slot slot[kPipeDepth];
        uint64_t next_ticket = 1;     // tickets handed out so far
        int async_open = 0;           // tickets not yet collected
    } hp;
    InputWindow win;
    // thr_detect_offsets: the caller's sub-bin carrier offsets for the batch in flight (device
    // array; nullptr = the Dirichlet fit), and the staging behind it
    const double* forced = nullptr;
    Dev<double> d_forced;
    bool sleepy_waits = false;   // thr_set_wait_mode: wait for a batch by query + short sleeps, not by polling
    // seconds the calling thread spent per phase of the host entry points' chunks
    // (thr_debug_pipe_times): grow staging, H2D calls, metadata, launches, D2H calls, chunks
    double t_pipe[8] = {};
    double t_pipe_max[8] = {};   // the longest single occurrence of each phase

    // thr_chipscan (chipscan.hip): allocated by the first call, grown by a larger one
    struct ChipScan {
        Dev<float2> d_xhat;             // [blocks per chunk][16384] carrier-shifted spectra, natural order
        Dev<float4> d_bank;             // [candidates per chunk][8192] conj(FFT(template)) / N, k_chip_scan's order
        Dev<thr::ChipStats> d_stats;    // [blocks per chunk][candidates per chunk]
        Dev<thr_chip_record> d_out;     // [blocks per chunk][n_lengths]
        Dev<thr_record> d_car;          // [blocks per chunk] carrier records (carrier_out)
        Dev<int> d_len;                 // [n_lengths]
        Dev<unsigned char> d_chips;     // [n_chips]
        Event ev[6];                    // carrier stage, bank kernel, scan + finish: begin and end
        size_t bank_budget = 0;         // thr_debug_chipscan_budget (0: thr::kChipBankBudget)
        size_t fill = 0;                // thr_debug_chipscan_fill: workgroups per launch aimed at (0: 2 x CUs)
        double ms[3] = {};              // the last call's device time per stage (thr_debug_chipscan_times)
    } chip;
    // single-chunk staging of the test hooks (lazy)
    Dev<unsigned char> d_in;
    Dev<long long> d_idx;
    Dev<thr_record> d_rec;
    // profiling
    int prof_every = 0;      // 0 = off, n = bracket the kernels of every n-th batch
    long long batch_no = 0;
    bool prof = false;       // this batch is being timed
    std::vector<EventPair> free_events;
    std::vector<EventPair> pending[THR_N_KERNEL_SLOTS];
    double ms[THR_N_KERNEL_SLOTS] = {};
    int64_t launches[THR_N_KERNEL_SLOTS] = {};

    thr_handle() = default;
    thr_handle(const thr_handle&) = delete;
    virtual ~thr_handle() = default;     // (a gate handle is deleted through this)
};
struct HandleDeleter {
    void operator()(thr_handle* h) const { thr_destroy(h); }
};


namespace thr {
namespace host {

struct ProfScope {
    thr_handle* h;
    int slot;
    EventPair ev{};
    bool on;
    hipStream_t stream;
    ProfScope(thr_handle* h_, int slot_, hipStream_t stream_ = nullptr)
        : h(h_), slot(slot_), on(h_->prof), stream(stream_ ? stream_ : h_->stream) {
        if (on) {
            if (!h->free_events.empty()) {
                ev = std::move(h->free_events.back());
                h->free_events.pop_back();
            } else {
                (void)ev.a.create();
                (void)ev.b.create();
            }
            (void)hipEventRecord(ev.a, stream);
        }
    }
    ~ProfScope() {
        if (on) {
            (void)hipEventRecord(ev.b, stream);
            h->pending[slot].push_back(std::move(ev));
        }
    }
};


// ---- handle.hip
void host_fft(std::vector<std::complex<double>>& a);
float2 unit_root(long long num, long long den);
int window_indices(int start, int stop, int n, int* lo, int* count);
bool plan_sections(thr::DevCfg& d, int template_len);
bool plan_sections_4k(thr::DevCfg& d, int template_len);
int build_constants(thr_handle* h);
int build_preshift_bank(thr_handle* h);
// ---- pipeline.hip
int ensure_pipe(thr_handle* h);
int pipe_h2d(thr_handle* h, int b, void* d_dst, const void* src, size_t bytes);
void pipe_inputs_done(thr_handle* h, int b);
size_t pipe_chunk_blocks(const thr_handle* h, size_t bytes_per_block);
int wait_event(thr_handle* h, hipEvent_t ev);
int pipe_drain(thr_handle* h, int b);
int pipe_inputs_enqueued(thr_handle* h, int b);
int pipe_records_enqueued(thr_handle* h, int b, thr_record* dst, size_t n_rec, size_t first, bool card);
int pipe_finish(thr_handle* h, int rc);
int ensure_staging(thr_handle* h, int format);
int run_batch(thr_handle* h, const void* d_samples, int format, const long long* d_block_idx,
              int n_blocks, thr_record* d_out, float2* dump_fft, float2* dump_xhat,
              float2* dump_corr, int dump_template, bool carrier_only, size_t stride = 0);
int stream_stride(thr_handle* h, size_t* stride);
int chunk_samples(thr_handle* h, int b, const void* src, int format, size_t blk_bytes, size_t stride,
                  const int64_t* block_idx, int64_t first_idx, size_t nb, thr_record* dst, size_t first);
int chunk_card(thr_handle* h, int b, const char* text, size_t text_len, const int64_t* payload_off,
               const int64_t* block_idx, size_t first, size_t nb, thr_record* dst);
int pipe_enter_sync(thr_handle* h, const char* who);

}  // namespace host
}  // namespace thr
