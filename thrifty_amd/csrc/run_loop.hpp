// The whole-file loop that thr_run_card / thr_run_stream (run_file.hip) and thr_run_extract_card /
// thr_run_extract_stream (run_extract.hip) share: the options check, the two framers, the calling thread's
// frame -> submit -> collect loop and the sink a collected batch goes through.  Host only, and on top of
// the PUBLIC entry points alone: nothing here reaches into a handle.  (run_gate.hip's loop has another
// shape -- a synchronous gate call, a writev writer, every block recorded -- and is not built on this.)
//
// What the two loops do differently, on purpose or by history; each is what its callers see today:
//   stats.blocks      detect: every collected batch counts whole, also one collected after the formatter
//                     has stopped.  extraction: the blocks before the index-error block, and no batch
//                     behind the end of the run.  (Sink::take returns the count; the front end adds it.)
//   stats.detections  the THR_FLAG_CORR records before the end of the run, kept or not: the extraction
//                     counts with no sink at all, the detect loop refuses to run without one.
//   error sentences   prefixed `thr_run:` / `thr_run_extract:` (Run::who); the index-error sentence ends
//                     "detections before it were written" / "blocks behind it were already folded: reset
//                     the extraction" (Run::index_tail).
//   precedence        the same in both: sink error, index error, collect error, framing / submit error.
//   timing            frame_s, submit_s and wait_s are the calling thread's.  format_s / write_s are the
//                     formatter thread's in the detect loop, the calling thread's in the extraction loop.
//                     format_s is ONE rule now, where the two files had two: it runs from the start of the
//                     record scan (the detect loop's rule; the extraction loop started it behind the scan)
//                     and is added whether thr_format_toad succeeds or not (the extraction loop's rule; the
//                     detect loop dropped it on failure).
//   records per block the handle's n_templates; an extraction's handle has one.
#pragma once
#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include <time.h>
#include <unistd.h>

#include "../../include/thrifty_hip.h"

namespace thr {
int fail_msg(int code, const char* fmt, ...);
int on_exception(const char* who) noexcept;

namespace run {

using Clock = std::chrono::steady_clock;
inline double secs(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }

inline double wall_clock() {
    timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    return double(ts.tv_sec) + 1e-9 * double(ts.tv_nsec);
}

struct Batch {
    std::vector<double> ts;           // one stamp per block (.card), or ONE for the whole batch (raw stream)
    std::vector<int64_t> idx, off;    // per block (off: .card payload offsets); raw stream: idx[0] = first block
    std::vector<thr_record> recs;     // [nb][T], filled by thr_collect
    size_t nb = 0;
    size_t first = 0;                 // ordinal of the batch's first block in this run
    uint64_t ticket = 0;
    double stamp(size_t block) const { return ts.size() == 1 ? ts[0] : ts[block]; }
};

struct Run {
    const char* who;                  // prefix of the loop's own error sentences
    const char* index_tail;           // how its index-error sentence ends
    thr_handle* h = nullptr;
    thr_run_opts o{};
    thr_run_stats st{};
    int T = 1, block_len = 0;
    int64_t new_len = 0;
    size_t max_batch = 0;
};

// `need_sink`: refuse a run with neither an output descriptor nor a record array.  `owner`: the handle
// the caller's extraction belongs to (no extraction: `h` itself).
inline int check(const char* who, thr_handle* h, const thr_run_opts* o, thr_run_stats* st, bool need_sink,
                 const thr_handle* owner, Run& R) {
    if (!h || !o || !st || !owner) return fail_msg(THR_ERR_ARG, "%s: null argument", who);
    if (o->struct_bytes != sizeof(thr_run_opts))
        return fail_msg(THR_ERR_ARG, "%s: thr_run_opts.struct_bytes %u, this library's is %zu", who, o->struct_bytes,
                        sizeof(thr_run_opts));
    if (need_sink && o->out_fd < 0 && !o->rec_out)
        return fail_msg(THR_ERR_ARG, "%s: neither an output descriptor nor a record array", who);
    if (owner != h) return fail_msg(THR_ERR_ARG, "%s: the extraction belongs to another handle", who);
    thr_settings cfg;
    const int rc = thr_get_settings(h, &cfg);
    if (rc != THR_OK) return rc;
    if (o->batch_blocks < 0 || o->batch_blocks > cfg.max_batch)
        return fail_msg(THR_ERR_ARG, "%s: batch_blocks %d exceeds the handle's max_batch %d", who, o->batch_blocks,
                        cfg.max_batch);
    std::memset(st, 0, sizeof *st);
    st->index_error_at = UINT64_MAX;
    st->index_error_block = -1;
    R.h = h;
    R.o = *o;
    R.T = cfg.n_templates;
    R.max_batch = size_t(o->batch_blocks ? o->batch_blocks : cfg.max_batch);
    R.block_len = cfg.block_len;
    R.new_len = int64_t(cfg.block_len) - cfg.history_len;
    R.st = *st;
    return THR_OK;
}

// next(batch) of .card text: up to max_batch lines, stamps and indices the lines' own; `pos` = bytes consumed
struct CardFramer {
    const Run& R;
    const char* text;
    size_t text_len, pos = 0;
    int operator()(Batch& b) {
        b.ts.resize(R.max_batch);
        b.idx.resize(R.max_batch);
        b.off.resize(R.max_batch);
        while (pos < text_len) {
            size_t n = 0, used = 0;
            const int frc = thr_frame_card(text + pos, text_len - pos, R.block_len, 1, R.max_batch, b.ts.data(),
                                           b.idx.data(), b.off.data(), &n, &used);
            if (frc != THR_OK) return frc;
            for (size_t i = 0; i < n; ++i) b.off[i] += int64_t(pos);
            pos += used;
            if (n) {
                b.nb = n;
                return THR_OK;
            }
            if (used == 0) break;      // (nothing framed, nothing skipped: the end)
        }
        b.nb = 0;
        return THR_OK;
    }
};

// next(batch) of a raw stream of `n_bytes`: batch k is blocks [idx[0], idx[0] + nb) of the stream
struct StreamFramer {
    const Run& R;
    size_t blk, stride, total, done = 0;
    StreamFramer(const Run& r, size_t n_bytes)
        : R(r), blk(size_t(r.block_len) * 2), stride(size_t(r.new_len) * 2),
          total(n_bytes < blk ? 0 : (n_bytes - blk) / stride + 1) {}
    int operator()(Batch& b) {
        b.nb = std::min(R.max_batch, total - done);
        if (b.nb == 0) return THR_OK;
        // the reference stamps a block when its read returns (block_data.py:86-98); of a mapped file
        // every block of a batch is "read" at once: one stamp
        b.ts.assign(1, std::isnan(R.o.timestamp) ? wall_clock() : R.o.timestamp);
        b.idx.assign(1, int64_t(done));
        done += b.nb;
        return THR_OK;
    }
    size_t offset(const Batch& b) const { return size_t(b.idx[0]) * stride; }
    size_t bytes(const Batch& b) const { return (b.nb - 1) * stride + blk; }
    size_t bytes_in() const { return done ? (done - 1) * stride + blk : 0; }
};

// Where a collected batch goes: the run ends at the first THR_FLAG_INDEX_ERROR record (the reference's
// loop raises there), the detected records before it are formatted and written when there is an output
// descriptor, and appended to the record array when there is one.  One thread at a time.
struct Sink {
    Run& R;
    int rc = THR_OK;                  // the first output error
    std::string err;
    size_t rec_n = 0;
    std::vector<thr_record> keep;
    std::vector<double> keep_ts;
    std::vector<char> text;
    explicit Sink(Run& r) : R(r) {}

    bool ended() const { return rc != THR_OK || R.st.index_error_at != UINT64_MAX; }

    int write_all(const char* p, size_t n) {
        while (n) {
            const ssize_t w = ::write(R.o.out_fd, p, n);
            if (w < 0) {
                if (errno == EINTR) continue;
                err = std::string("write() to the .toad output failed: ") + strerror(errno);
                return THR_ERR_STATE;
            }
            p += w;
            n -= size_t(w);
        }
        return THR_OK;
    }

    // -> the blocks of `b` before the end of the run: b.nb unless it holds the index-error block
    size_t take(const Batch& b) {
        const auto t0 = Clock::now();
        const thr_run_opts& o = R.o;
        thr_run_stats& st = R.st;
        const bool want = o.out_fd >= 0 || o.rec_out;
        const size_t T = size_t(R.T);
        keep.clear();
        keep_ts.clear();
        size_t end = b.nb;
        for (size_t block = 0; block < end; ++block) {
            for (size_t t = 0; t < T; ++t) {
                const thr_record& r = b.recs[block * T + t];
                if (r.flags & THR_FLAG_INDEX_ERROR) {   // carrier_sync.py:187: the reference's loop dies here
                    st.index_error_block = r.block_idx;
                    st.index_error_bin = r.carrier_bin;
                    st.index_error_at = uint64_t(b.first + block);
                    end = block;                        // (ends the outer loop too)
                    break;
                }
                if (r.flags & THR_FLAG_CORR) {
                    st.detections += 1;
                    if (want) {
                        keep.push_back(r);
                        keep_ts.push_back(b.stamp(block));
                    }
                }
            }
        }
        if (!keep.empty() && o.out_fd >= 0) {
            text.resize(keep.size() * size_t(THR_TOAD_LINE_MAX));
            size_t used = 0;
            rc = thr_format_toad(keep.data(), keep_ts.data(), keep.size(), R.new_len, o.with_rxid, o.rxid, o.with_txid,
                                 o.carrier_offset_mode, text.data(), text.size(), &used);
            const auto t1 = Clock::now();
            st.format_s += secs(t0, t1);
            if (rc != THR_OK) {
                err = thr_last_error();                 // (this thread's message)
            } else {
                rc = write_all(text.data(), used);
                st.write_s += secs(t1, Clock::now());
                st.text_bytes += used;
            }
        }
        if (!keep.empty() && o.rec_out && rc == THR_OK) {
            if (rec_n + keep.size() > o.rec_capacity) {
                rc = THR_ERR_ARG;
                err = std::string(R.who) + ": more detections than rec_capacity";
            } else {
                for (size_t i = 0; i < keep.size(); ++i) {      // the timestamp travels in `reserved`
                    thr_record r = keep[i];
                    std::memcpy(&r.reserved, &keep_ts[i], sizeof(double));
                    o.rec_out[rec_n + i] = r;
                }
                rec_n += keep.size();
            }
        }
        return end;
    }
};

// The calling thread's loop: `next(batch)` frames the next batch (nb = 0 at the end of the input), `submit`
// hands it to the engine, up to THR_MAX_IN_FLIGHT stay open, the oldest is collected and delivered.  `D`
// owns the batches and the sink:
//   D.ring[s]      the batches           D.acquire() -> s   a free one (may wait for it)
//   D.release(s)   unused, or dropped    D.deliver(s)       collected: through the sink, then free again
//   D.ended()      the sink has seen the end of the run: nothing more is framed
//   D.finish()     everything delivered has been through D.sink
// (D is made here: its batches, and the detect loop's thread start, are inside total_s)
template <class Delivery, class Next, class Submit>
int drive(Run& R, Next&& next, Submit&& submit) {
    const auto t_start = Clock::now();
    Delivery D(R);
    std::deque<int> flight;
    bool input_done = false;
    size_t ordinal = 0;
    // the first error of THIS thread, by where it lies in the input: a batch that fails at collect
    // (invalid base64) was submitted before whatever stopped the framing / submitting
    int in_rc = THR_OK, col_rc = THR_OK;
    std::string in_err, col_err;
    bool dead = false;        // a collect failed: what was submitted after it is waited for and dropped
    try {
        for (;;) {
            if (!input_done && !dead && !D.ended() && flight.size() < size_t(THR_MAX_IN_FLIGHT)) {
                const int s = D.acquire();
                Batch& b = D.ring[size_t(s)];
                const auto t0 = Clock::now();
                b.nb = 0;
                b.ticket = 0;
                int frc = next(b);
                const auto t1 = Clock::now();
                R.st.frame_s += secs(t0, t1);
                if (frc == THR_OK && b.nb != 0) {
                    b.first = ordinal;
                    b.recs.resize(b.nb * size_t(R.T));
                    frc = submit(b);
                    R.st.submit_s += secs(t1, Clock::now());
                }
                if (frc != THR_OK || b.nb == 0) {
                    if (frc != THR_OK) {
                        in_rc = frc;
                        in_err = thr_last_error();
                    }
                    input_done = true;
                    D.release(s);
                    continue;
                }
                ordinal += b.nb;
                R.st.batches += 1;
                flight.push_back(s);
                continue;
            }
            if (flight.empty()) break;
            const int s = flight.front();
            flight.pop_front();
            const auto t0 = Clock::now();
            const int crc = thr_collect(R.h, D.ring[size_t(s)].ticket);
            R.st.wait_s += secs(t0, Clock::now());
            if (crc != THR_OK && !dead) {
                col_rc = crc;
                col_err = thr_last_error();
                dead = true;
            }
            // (after a framing / submit error the batches submitted BEFORE it still go out: the
            // reference's per-line loop had emitted everything ahead of the bad input)
            if (dead) D.release(s);
            else D.deliver(s);
        }
    } catch (...) {
        // (host memory): the handle must not be left with open tickets
        in_rc = on_exception(R.who);
        in_err = thr_last_error();
        for (int s : flight) (void)thr_collect(R.h, D.ring[size_t(s)].ticket);
    }
    D.finish();
    R.st.total_s = secs(t_start, Clock::now());
    if (D.sink.rc != THR_OK) return fail_msg(D.sink.rc, "%s", D.sink.err.c_str());
    if (R.st.index_error_at != UINT64_MAX)
        return fail_msg(THR_ERR_INDEX,
                        "block %lld: carrier bin %d + fit reach >= block_len -- the reference raises IndexError "
                        "here (carrier_sync.py:187); %s",
                        (long long)R.st.index_error_block, R.st.index_error_bin, R.index_tail);
    if (col_rc != THR_OK) return fail_msg(col_rc, "%s", col_err.c_str());
    if (in_rc != THR_OK) return fail_msg(in_rc, "%s", in_err.c_str());
    return THR_OK;
}

}  // namespace run
}  // namespace thr
