// thr_input_window*: the page-locked input file (InputWindow, input_window.hpp), thr_host_register.
#include "host_internal.hpp"

#include <sys/mman.h>

void InputWindow::populate_run() {
    std::unique_lock<std::mutex> lk(mu);
    while (!stop) {
        if (pop_next < consumed) pop_next = consumed;
        if (!draining && pop_next < n_seg && pop_next < consumed + kAhead) {
            const size_t sgm = pop_next++;
            lk.unlock();
            void* at = reinterpret_cast<void*>(seg_lo(sgm));
            const double t0 = now_s();
#ifdef MADV_POPULATE_READ
            int rc = madvise(at, seg_len(sgm), MADV_POPULATE_READ);
#else
            int rc = -1;
#endif
            if (rc != 0) {     // older kernels: touch a byte of every page
                volatile const unsigned char* q = static_cast<const unsigned char*>(at);
                unsigned acc = 0;
                for (size_t i = 0; i < seg_len(sgm); i += 4096) acc += q[i];
                (void)acc;
            }
            lk.lock();
            t_populate += now_s() - t0;
            populated[sgm] = 1;
            cv.notify_all();
            continue;
        }
        cv.wait(lk);
    }
}

void InputWindow::run() {
    (void)hipSetDevice(device);
    std::unique_lock<std::mutex> lk(mu);
    while (!stop) {
        // (never more than 2 x kAhead segments locked, however far the unlocker lags behind)
        if (!failed && !draining && reg_hi < n_seg && reg_hi < consumed + kAhead && reg_hi < reg_lo + 2 * kAhead) {
            if (reg_hi < consumed) {      // the reader skipped ahead: nothing in between is wanted
                if (reg_lo == reg_hi)     // (once the unlocker has let go of what was locked below)
                    reg_lo = reg_hi = consumed;
                else
                    cv.wait(lk);
                continue;
            }
            const size_t sgm = reg_hi;
            if (!populated[sgm]) {        // (a populator has it, or will take it next)
                cv.wait(lk);
                continue;
            }
            lk.unlock();
            const double t0 = now_s();
            const hipError_t rc = hipHostRegister(reinterpret_cast<void*>(seg_lo(sgm)), seg_len(sgm),
                                                  hipHostRegisterDefault);
            if (rc != hipSuccess) (void)hipGetLastError();
            lk.lock();
            t_register += now_s() - t0;
            if (rc == hipSuccess)
                ++reg_hi;
            else
                failed = true;            // (locked-memory limit, exotic mapping): pageable copies from here on
            cv.notify_all();
            continue;
        }
        cv.wait(lk);
    }
}

void InputWindow::unlock_run() {
    (void)hipSetDevice(device);
    std::unique_lock<std::mutex> lk(mu);
    while (!stop) {
        if (reg_lo < std::min(consumed, reg_hi)) {
            const size_t sgm = reg_lo;
            lk.unlock();
            const double t0 = now_s();
            (void)hipHostUnregister(reinterpret_cast<void*>(seg_lo(sgm)));
            lk.lock();
            t_unregister += now_s() - t0;
            ++reg_lo;
            cv.notify_all();
            continue;
        }
        cv.wait(lk);
    }
}

void InputWindow::open(const void* p, size_t bytes, int dev, int n_populators, size_t seg_bytes) {
    close();
    const uintptr_t page = 4096;
    kSeg = seg_bytes ? seg_bytes : kSegDefault;
    kAhead = std::max<size_t>(2, kAheadBytes / kSeg);
    base = reinterpret_cast<uintptr_t>(p) & ~(page - 1);
    end = (reinterpret_cast<uintptr_t>(p) + bytes + page - 1) & ~(page - 1);
    n_seg = size_t((end - base + kSeg - 1) / kSeg);
    reg_lo = reg_hi = consumed = pop_next = 0;
    t_populate = t_register = t_unregister = t_acquire = 0;
    n_acquire_waits = n_pageable = 0;
    populated.assign(n_seg, 0);
    stop = failed = draining = false;
    device = dev;
    populators.clear();
    try {
        worker = std::thread([this] { run(); });
        unlocker = std::thread([this] { unlock_run(); });
        for (int i = 0; i < std::max(1, n_populators); ++i) populators.emplace_back([this] { populate_run(); });
    } catch (...) {        // a thread could not be started: stop the ones that were, no window
        close();
        throw;
    }
}

void InputWindow::close() {
    if (!worker.joinable() && !unlocker.joinable() && populators.empty()) return;
    {
        std::lock_guard<std::mutex> lk(mu);
        stop = true;
    }
    cv.notify_all();
    if (worker.joinable()) worker.join();
    if (unlocker.joinable()) unlocker.join();
    for (auto& t : populators) t.join();
    populators.clear();
    for (size_t sgm = reg_lo; sgm < reg_hi; ++sgm)      // what is still locked
        (void)hipHostUnregister(reinterpret_cast<void*>(seg_lo(sgm)));
    reg_lo = reg_hi = 0;
    base = end = 0;
    n_seg = 0;
}

void InputWindow::release_all() {
    if (!worker.joinable()) return;
    {
        std::lock_guard<std::mutex> lk(mu);
        draining = true;
        consumed = n_seg;
    }
    cv.notify_all();
}

bool InputWindow::acquire(const void* src, size_t bytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(src);
    if (base == 0 || bytes == 0 || a < base || a + bytes > end) return false;
    const size_t s0 = size_t((a - base) / kSeg), s1 = size_t((a + bytes - 1 - base) / kSeg);
    std::unique_lock<std::mutex> lk(mu);
    if (failed || draining || s0 < reg_lo || s1 >= consumed + kAhead) {
        ++n_pageable;
        return false;
    }
    if (!(failed || reg_hi > s1)) {
        const double t0 = now_s();
        cv.wait(lk, [&] { return failed || reg_hi > s1; });
        t_acquire += now_s() - t0;
        ++n_acquire_waits;
    }
    return !failed && s0 >= reg_lo;
}

void InputWindow::release_below(uintptr_t upto) {
    if (base == 0 || upto <= base) return;
    const size_t sgm = size_t((std::min(upto, end) - base) / kSeg);
    {
        std::lock_guard<std::mutex> lk(mu);
        if (sgm <= consumed) return;
        consumed = sgm;
    }
    cv.notify_all();
}

extern "C" {

namespace {
constexpr uintptr_t kPage = 4096;
}
int thr_host_register(const void* p, size_t bytes) try {
    if (!p || bytes == 0) return fail(THR_ERR_ARG, "thr_host_register: empty range");
    const uintptr_t a = reinterpret_cast<uintptr_t>(p) & ~(kPage - 1);
    const uintptr_t e = (reinterpret_cast<uintptr_t>(p) + bytes + kPage - 1) & ~(kPage - 1);
    const hipError_t rc = hipHostRegister(reinterpret_cast<void*>(a), size_t(e - a), hipHostRegisterDefault);
    if (rc != hipSuccess) {
        (void)hipGetLastError();
        return fail(THR_ERR_DEVICE, "hipHostRegister(%zu bytes) failed: %s", size_t(e - a), hipGetErrorString(rc));
    }
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_host_register");
}

int thr_host_unregister(const void* p) try {
    if (!p) return fail(THR_ERR_ARG, "thr_host_unregister: null");
    const uintptr_t a = reinterpret_cast<uintptr_t>(p) & ~(kPage - 1);
    const hipError_t rc = hipHostUnregister(reinterpret_cast<void*>(a));
    if (rc != hipSuccess) {
        (void)hipGetLastError();
        return fail(THR_ERR_DEVICE, "hipHostUnregister failed: %s", hipGetErrorString(rc));
    }
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_host_unregister");
}

int thr_input_window(thr_handle* h, const void* p, size_t bytes) try {
    return thr_input_window_ex(h, p, bytes, 0, 0);
} catch (...) {
    return thr::on_exception("thr_input_window");
}

int thr_input_window_ex(thr_handle* h, const void* p, size_t bytes, int populate_threads, size_t segment_bytes) try {
    if (!h) return fail(THR_ERR_ARG, "thr_input_window: null handle");
    if (populate_threads < 0 || populate_threads > 16)
        return fail(THR_ERR_ARG, "thr_input_window_ex: populate_threads %d out of range [0, 16]", populate_threads);
    if (segment_bytes && (segment_bytes < (size_t(1) << 16) || (segment_bytes & (segment_bytes - 1))))
        return fail(THR_ERR_ARG, "thr_input_window_ex: segment_bytes %zu is not a power of two >= 64 KiB", segment_bytes);
    if (hipSetDevice(h->device) != hipSuccess) return fail(THR_ERR_DEVICE, "hipSetDevice(%d) failed", h->device);
    if (h->hp.async_open != 0)
        return fail(THR_ERR_STATE, "thr_input_window: %d submitted batch(es) not collected yet", h->hp.async_open);
    if (h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);     // no copy may still read the old window
    h->win.close();
    for (auto& s : h->hp.slot) s.win_lo = s.win_end = 0;
    if (p && bytes)
        h->win.open(p, bytes, h->device, populate_threads ? populate_threads : InputWindow::kPopulators, segment_bytes);
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_input_window_ex");
}

int thr_debug_window(thr_handle* h, size_t out[4]) try {
    if (!h || !out) return fail(THR_ERR_ARG, "thr_debug_window: null argument");
    std::lock_guard<std::mutex> lk(h->win.mu);
    out[0] = h->win.base ? h->win.consumed * h->win.kSeg : 0;
    out[1] = h->win.reg_lo * h->win.kSeg;
    out[2] = h->win.reg_hi * h->win.kSeg;
    out[3] = h->win.base ? h->win.kSeg : 0;
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_window");
}


int thr_debug_window_times(thr_handle* h, double out[6]) try {
    if (!h || !out) return fail(THR_ERR_ARG, "thr_debug_window_times: null argument");
    std::lock_guard<std::mutex> lk(h->win.mu);
    out[0] = h->win.t_populate;
    out[1] = h->win.t_register;
    out[2] = h->win.t_unregister;
    out[3] = h->win.t_acquire;
    out[4] = double(h->win.n_acquire_waits);
    out[5] = double(h->win.n_pageable);
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_debug_window_times");
}

int thr_input_window_release(thr_handle* h) try {
    if (!h) return fail(THR_ERR_ARG, "thr_input_window_release: null handle");
    if (hipSetDevice(h->device) != hipSuccess) return fail(THR_ERR_DEVICE, "hipSetDevice(%d) failed", h->device);
    if (h->hp.async_open != 0)
        return fail(THR_ERR_STATE, "thr_input_window_release: %d submitted batch(es) not collected yet",
                    h->hp.async_open);
    if (h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);     // no copy reads the window any more
    for (auto& s : h->hp.slot) s.win_lo = s.win_end = 0;
    h->win.release_all();
    return THR_OK;
} catch (...) {
    return thr::on_exception("thr_input_window_release");
}


}  // extern "C"
