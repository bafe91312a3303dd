// The input window of a handle (thr_input_window*): declarations; the member bodies are in window.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <thread>
#include <vector>

// thr_input_window(): a caller mapping (the input file) that the host entry points read
// sequentially.  Library threads keep a bounded stretch of it page-locked around the read position,
// one segment (128 MiB) at a time: populators map the pages of the segments ahead, a locking worker
// hipHostRegister()s them up to kAhead segments in front of the chunk copies, an unlocking worker
// hipHostUnregister()s what the copies have left behind.  The copies are then asynchronous DMA out
// of the page cache (they return at once instead of occupying the calling thread while the runtime
// stages pageable memory), the locking -- 5 ms per GiB on mapped pages, 17 ms per GiB to unlock --
// runs beside the caller instead of in front of it, and never more than 2 x kAhead segments are
// locked whatever the size of the file.  (Round 5: locking and unlocking on ONE thread filled a
// whole run -- the caller waited for locks queued behind unlocks; see profiles/README.md.)
struct InputWindow {
    static constexpr size_t kSegDefault = size_t(128) << 20;
    static constexpr size_t kAheadBytes = size_t(1) << 30;   // the worker runs at most this far ahead of `consumed`
    size_t kSeg = kSegDefault;                // bytes per segment (thr_input_window_ex: tests shrink it)
    size_t kAhead = 8;                        // segments the worker may run ahead of `consumed` (1 GiB)
    uintptr_t base = 0, end = 0;              // page-aligned span; base == 0: no window
    size_t n_seg = 0;
    size_t reg_lo = 0, reg_hi = 0;            // segments [reg_lo, reg_hi) are locked now
    size_t consumed = 0;                      // segments below this one are not needed any more
    bool stop = false, failed = false;
    bool draining = false;                    // release_all(): nothing more is locked, everything locked is let go
    int device = 0;
    std::thread worker, unlocker;
    std::mutex mu;
    std::condition_variable cv;
    // page-table population runs in front of the locking, on threads of its own: locking pages
    // that are already mapped goes at ~100 GB/s, faulting them in one by one inside
    // hipHostRegister at ~30 (measured), and the fabric copies run at 56
    static constexpr int kPopulators = 3;      // default; thr_input_window_ex sizes it (ranks share the host's CPUs)
    std::vector<std::thread> populators;
    std::vector<unsigned char> populated;      // per segment: its pages are mapped
    size_t pop_next = 0;                       // next segment a populator takes
    // where the window's threads spend their time (thr_debug_window_times; seconds, under `mu`)
    double t_populate = 0, t_register = 0, t_unregister = 0, t_acquire = 0;
    size_t n_acquire_waits = 0, n_pageable = 0;
    static double now_s() {
        return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    }
    uintptr_t seg_lo(size_t s) const { return base + s * kSeg; }
    size_t seg_len(size_t s) const { return size_t(std::min<uintptr_t>(end, seg_lo(s) + kSeg) - seg_lo(s)); }

    void populate_run();
    // the locking worker: page-locks segment reg_hi while it lies less than kAhead segments ahead of
    // `consumed` and its pages are mapped
    void run();
    // the unlocking worker, a thread of its own: hipHostUnregister costs three times what
    // hipHostRegister costs on mapped pages (measured: 47 against 15 ms per 2.9 GB), and on ONE
    // thread the two together filled the whole run -- the caller waited for locks that were queued
    // behind unlocks of segments nobody needed any more
    void unlock_run();
    void open(const void* p, size_t bytes, int dev, int n_populators = kPopulators, size_t seg_bytes = 0);
    void close();
    // The reader is done with the window: nothing more is locked, and the unlocking worker lets go of
    // everything that still is -- in the background; close() (or the next open()) waits for it.
    void release_all();
    // [src, src + bytes) is about to be copied: wait until its segments are locked.  False: copy
    // it as pageable memory (outside the window, behind it, too far ahead, or locking failed).
    bool acquire(const void* src, size_t bytes);
    // every copy that ends at or before `upto` has completed
    void release_below(uintptr_t upto);
};
