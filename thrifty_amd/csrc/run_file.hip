// thr_run_card / thr_run_stream: the whole `thrifty detect rx.card -o rx.toad` loop in one call.
//
// The reference runs, per block, card_reader / block_reader -> Detector.detect -> `if detected:
// print(result.serialize())` (detect.py:197-223, block_data.py:70-131).  thrifty_amd.detect drove the
// batched form of that loop from Python through five ctypes calls per batch (thr_frame_card,
// thr_submit_card two ahead, thr_collect, thr_format_toad, file.write); at a million blocks a second
// that interpreter thread was the bound.  Here the same loop is C++ on top of the SAME public entry
// points -- nothing in this file reaches into a handle -- with the text on a thread of its own:
//
//   caller's thread : frame a batch (thr_frame_card) -> thr_submit_card / thr_submit_stream, up to
//                     THR_MAX_IN_FLIGHT open -> thr_collect the oldest -> queue its records
//   formatter thread: keep the detected records (THR_FLAG_CORR; a THR_FLAG_INDEX_ERROR record ends
//                     the run where the reference's loop raised) -> thr_format_toad -> write(fd)
//                     and / or append them to the caller's record array
//
// A handle stays single-threaded (only the caller's thread touches it); the formatter uses the
// handle-free thr_format_toad.  The caller's loop, the framers and what the formatter does with a batch
// (Sink) are run_loop.hpp's, shared with run_extract.hip; the text thread and its queue are this file's.
#include <atomic>
#include <condition_variable>
#include <exception>
#include <mutex>
#include <thread>

#include "run_loop.hpp"

namespace {

using namespace thr::run;

// The text thread and the batches it shares with the caller's thread (drive()'s `D`, run_loop.hpp):
// free -> in flight (caller's thread) -> queued (formatter) -> free
struct Formatter {
    Run& R;
    Sink sink;
    std::vector<Batch> ring;
    std::deque<int> free_slots, queued;
    std::mutex mu;
    std::condition_variable cv;
    bool producer_done = false;
    std::atomic<bool> stop{false};    // the formatter hit the end of the run (index error / write error)
    std::thread thread;

    explicit Formatter(Run& r) : R(r), sink(r), ring(size_t(THR_MAX_IN_FLIGHT + 3)) {
        for (int i = 0; i < int(ring.size()); ++i) free_slots.push_back(i);
        thread = std::thread([this] { loop(); });
    }
    ~Formatter() { finish(); }

    bool ended() const { return stop.load(); }

    // the end of the input for the formatter: it drains its queue and returns
    void finish() {
        if (!thread.joinable()) return;
        {
            std::lock_guard<std::mutex> lk(mu);
            producer_done = true;
        }
        cv.notify_all();
        thread.join();
    }

    int acquire() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !free_slots.empty(); });
        const int s = free_slots.front();
        free_slots.pop_front();
        return s;
    }
    void release(int s) {
        {
            std::lock_guard<std::mutex> lk(mu);
            free_slots.push_back(s);
        }
        cv.notify_all();
    }
    void deliver(int s) {
        R.st.blocks += ring[size_t(s)].nb;
        {
            std::lock_guard<std::mutex> lk(mu);
            queued.push_back(s);
        }
        cv.notify_all();
    }

    void loop() {
        for (;;) {
            int s;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !queued.empty() || producer_done; });
                if (queued.empty()) return;
                s = queued.front();
                queued.pop_front();
            }
            // (this is a std::thread: an exception that left it -- std::bad_alloc from the sink's three
            // vectors -- would end the whole process in std::terminate.  It ends the RUN instead; the slot
            // goes back either way, so the caller's thread never blocks in acquire())
            if (!stop.load()) try {
                sink.take(ring[size_t(s)]);
            } catch (const std::exception& e) {
                sink.rc = THR_ERR_STATE;
                sink.err = std::string("thr_run: the text thread failed: ") + e.what();
            } catch (...) {
                sink.rc = THR_ERR_STATE;
                sink.err = "thr_run: the text thread failed (unknown exception)";
            }
            if (sink.ended()) stop.store(true);
            release(s);
        }
    }
};

const char* const INDEX_TAIL = "detections before it were written";

}  // namespace

extern "C" {

int thr_run_card(thr_handle* h, const char* text, size_t text_len, const thr_run_opts* opts,
                 thr_run_stats* stats) try {
    Run R{"thr_run", INDEX_TAIL};
    int rc = check("thr_run_card", h, opts, stats, true, h, R);
    if (rc != THR_OK) return rc;
    if (!text && text_len) return thr::fail_msg(THR_ERR_ARG, "thr_run_card: null text");
    CardFramer next{R, text, text_len};
    rc = drive<Formatter>(R, next, [&](Batch& b) -> int {
        return thr_submit_card(h, text, text_len, b.off.data(), b.idx.data(), b.nb, b.recs.data(), &b.ticket);
    });
    R.st.bytes_in = next.pos;
    *stats = R.st;
    return rc;
} catch (...) {
    return thr::on_exception("thr_run_card");
}

int thr_run_stream(thr_handle* h, const uint8_t* stream, size_t n_bytes, int64_t first_block_idx,
                   const thr_run_opts* opts, thr_run_stats* stats) try {
    Run R{"thr_run", INDEX_TAIL};
    int rc = check("thr_run_stream", h, opts, stats, true, h, R);
    if (rc != THR_OK) return rc;
    if (!stream && n_bytes) return thr::fail_msg(THR_ERR_ARG, "thr_run_stream: null stream");
    StreamFramer next(R, n_bytes);
    rc = drive<Formatter>(R, next, [&](Batch& b) -> int {
        size_t got = 0;
        const int src = thr_submit_stream(h, stream + next.offset(b), next.bytes(b), first_block_idx + b.idx[0],
                                          b.recs.data(), b.nb, &got, &b.ticket);
        if (src == THR_OK && got != b.nb)
            return thr::fail_msg(THR_ERR_STATE, "thr_run_stream: framed %zu blocks, engine took %zu", b.nb, got);
        return src;
    });
    R.st.bytes_in = next.bytes_in();
    *stats = R.st;
    return rc;
} catch (...) {
    return thr::on_exception("thr_run_stream");
}

}  // extern "C"
