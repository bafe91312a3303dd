// thr_run_extract_card / thr_run_extract_stream: the whole-capture loop of a template extraction in one
// call -- thr_run_card / thr_run_stream (run_file.hip) with the extraction's fold and keep enqueued
// behind every batch (thr_extract_submit_card / thr_extract_submit_stream) and nothing else per batch:
// the calling thread frames, keeps up to THR_MAX_IN_FLIGHT batches submitted and collects them in order.
// What a collected batch is looked at for is the reference's IndexError block (the run ends there) and
// the detection count; .toad text is formatted only when an output descriptor was given, records are
// appended only when an array was.  Like run_file.hip this file is built on the public entry points; all
// it reads of an extraction is the handle it belongs to.
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include <time.h>
#include <unistd.h>

#include "template_extract.hpp"

namespace thr {
int fail_msg(int code, const char* fmt, ...);
int on_exception(const char* who) noexcept;
}

namespace {

using Clock = std::chrono::steady_clock;
inline double secs(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }

double wall_clock() {
    timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    return double(ts.tv_sec) + 1e-9 * double(ts.tv_nsec);
}

struct Batch {
    std::vector<double> ts;
    std::vector<int64_t> idx, off;
    std::vector<thr_record> recs;
    size_t nb = 0, first = 0;
    uint64_t ticket = 0;
};

struct Run {
    thr_handle* h = nullptr;
    thr_run_opts o{};
    thr_run_stats st{};
    int block_len = 0;
    int64_t new_len = 0;
    size_t max_batch = 0, rec_n = 0;
    bool stopped = false;             // the index-error block, or an output error: nothing more is submitted
    int out_rc = THR_OK;
    std::string out_err;
    std::vector<thr_record> keep;
    std::vector<double> keep_ts;
    std::vector<char> text;

    int write_all(const char* p, size_t n) {
        while (n) {
            const ssize_t w = ::write(o.out_fd, p, n);
            if (w < 0) {
                if (errno == EINTR) continue;
                out_err = std::string("write() to the .toad output failed: ") + strerror(errno);
                return THR_ERR_STATE;
            }
            p += w;
            n -= size_t(w);
        }
        return THR_OK;
    }

    // a collected batch: where the run ends, how many detections, the outputs that were asked for
    void take(const Batch& b) {
        size_t end = b.nb;
        const bool want = o.out_fd >= 0 || o.rec_out;
        keep.clear();
        keep_ts.clear();
        for (size_t i = 0; i < b.nb; ++i) {
            const thr_record& r = b.recs[i];
            if (r.flags & THR_FLAG_INDEX_ERROR) {     // carrier_sync.py:187: the reference's loop dies here
                end = i;
                st.index_error_block = r.block_idx;
                st.index_error_bin = r.carrier_bin;
                st.index_error_at = uint64_t(b.first + i);
                break;
            }
            if (r.flags & THR_FLAG_CORR) {
                st.detections += 1;
                if (want) {
                    keep.push_back(r);
                    keep_ts.push_back(b.ts.size() == 1 ? b.ts[0] : b.ts[i]);
                }
            }
        }
        st.blocks += end;
        if (!keep.empty() && o.out_fd >= 0) {
            const auto t0 = Clock::now();
            text.resize(keep.size() * size_t(THR_TOAD_LINE_MAX));
            size_t used = 0;
            const int rc = thr_format_toad(keep.data(), keep_ts.data(), keep.size(), new_len, o.with_rxid, o.rxid,
                                           o.with_txid, o.carrier_offset_mode, text.data(), text.size(), &used);
            const auto t1 = Clock::now();
            st.format_s += secs(t0, t1);
            if (rc != THR_OK) {
                out_rc = rc;
                out_err = thr_last_error();
            } else {
                out_rc = write_all(text.data(), used);
                st.write_s += secs(t1, Clock::now());
                st.text_bytes += used;
            }
        }
        if (!keep.empty() && o.rec_out && out_rc == THR_OK) {
            if (rec_n + keep.size() > o.rec_capacity) {
                out_rc = THR_ERR_ARG;
                out_err = "thr_run_extract: more detections than rec_capacity";
            } else {
                for (size_t i = 0; i < keep.size(); ++i) {      // the timestamp travels in `reserved`
                    thr_record r = keep[i];
                    std::memcpy(&r.reserved, &keep_ts[i], sizeof(double));
                    o.rec_out[rec_n + i] = r;
                }
                rec_n += keep.size();
            }
        }
        if (end != b.nb || out_rc != THR_OK) stopped = true;
    }
};

template <class Next, class Submit>
int drive(Run& R, Next&& next, Submit&& submit) {
    const auto t_start = Clock::now();
    std::vector<Batch> ring(size_t(THR_MAX_IN_FLIGHT));
    std::deque<int> flight, spare;
    for (int i = 0; i < THR_MAX_IN_FLIGHT; ++i) spare.push_back(i);
    bool input_done = false, dead = false;
    size_t ordinal = 0;
    int in_rc = THR_OK, col_rc = THR_OK;
    std::string in_err, col_err;
    try {
        for (;;) {
            if (!input_done && !dead && !R.stopped && !spare.empty()) {
                const int s = spare.front();
                Batch& b = ring[size_t(s)];
                const auto t0 = Clock::now();
                b.nb = 0;
                b.ticket = 0;
                int frc = next(b);
                const auto t1 = Clock::now();
                R.st.frame_s += secs(t0, t1);
                if (frc == THR_OK && b.nb != 0) {
                    b.first = ordinal;
                    b.recs.resize(b.nb);
                    frc = submit(b);
                    R.st.submit_s += secs(t1, Clock::now());
                } else if (frc == THR_OK) {
                    input_done = true;
                    continue;
                }
                if (frc != THR_OK) {
                    in_rc = frc;
                    in_err = thr_last_error();
                    input_done = true;
                    continue;
                }
                ordinal += b.nb;
                R.st.batches += 1;
                spare.pop_front();
                flight.push_back(s);
                continue;
            }
            if (flight.empty()) break;
            const int s = flight.front();
            flight.pop_front();
            spare.push_back(s);
            Batch& b = ring[size_t(s)];
            const auto t0 = Clock::now();
            const int crc = thr_collect(R.h, b.ticket);
            R.st.wait_s += secs(t0, Clock::now());
            if (crc != THR_OK && !dead) {
                col_rc = crc;
                col_err = thr_last_error();
                dead = true;
            }
            if (!dead && !R.stopped) R.take(b);      // (behind the end of the run: waited for and dropped)
        }
    } catch (...) {
        in_rc = thr::on_exception("thr_run_extract");
        in_err = thr_last_error();
        for (int s : flight) (void)thr_collect(R.h, ring[size_t(s)].ticket);    // no ticket stays open
    }
    R.st.total_s = secs(t_start, Clock::now());
    if (R.out_rc != THR_OK) return thr::fail_msg(R.out_rc, "%s", R.out_err.c_str());
    if (R.st.index_error_at != UINT64_MAX)
        return thr::fail_msg(THR_ERR_INDEX,
                             "block %lld: carrier bin %d + fit reach >= block_len -- the reference raises IndexError "
                             "here (carrier_sync.py:187); blocks behind it were already folded: reset the extraction",
                             (long long)R.st.index_error_block, R.st.index_error_bin);
    if (col_rc != THR_OK) return thr::fail_msg(col_rc, "%s", col_err.c_str());
    if (in_rc != THR_OK) return thr::fail_msg(in_rc, "%s", in_err.c_str());
    return THR_OK;
}

int check(const char* who, thr_handle* h, const thr_run_opts* o, thr_extract* x, thr_run_stats* st, Run& R) {
    if (!h || !o || !x || !st) return thr::fail_msg(THR_ERR_ARG, "%s: null argument", who);
    if (o->struct_bytes != sizeof(thr_run_opts))
        return thr::fail_msg(THR_ERR_ARG, "%s: thr_run_opts.struct_bytes %u, this library's is %zu", who,
                             o->struct_bytes, sizeof(thr_run_opts));
    if (x->h != h) return thr::fail_msg(THR_ERR_ARG, "%s: the extraction belongs to another handle", who);
    thr_settings cfg;
    const int rc = thr_get_settings(h, &cfg);
    if (rc != THR_OK) return rc;
    if (o->batch_blocks < 0 || o->batch_blocks > cfg.max_batch)
        return thr::fail_msg(THR_ERR_ARG, "%s: batch_blocks %d exceeds the handle's max_batch %d", who,
                             o->batch_blocks, cfg.max_batch);
    std::memset(st, 0, sizeof *st);
    st->index_error_at = UINT64_MAX;
    st->index_error_block = -1;
    R.h = h;
    R.o = *o;
    R.max_batch = size_t(o->batch_blocks ? o->batch_blocks : cfg.max_batch);
    R.block_len = cfg.block_len;
    R.new_len = int64_t(cfg.block_len) - cfg.history_len;
    R.st = *st;
    return THR_OK;
}

}  // namespace

extern "C" {

int thr_run_extract_card(thr_handle* h, const char* text, size_t text_len, const thr_run_opts* opts,
                         thr_extract* x, thr_run_stats* stats) try {
    Run R;
    int rc = check("thr_run_extract_card", h, opts, x, stats, R);
    if (rc != THR_OK) return rc;
    if (!text && text_len) return thr::fail_msg(THR_ERR_ARG, "thr_run_extract_card: null text");
    size_t pos = 0;
    auto next = [&](Batch& b) -> int {
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
            if (used == 0) break;
        }
        b.nb = 0;
        return THR_OK;
    };
    auto submit = [&](Batch& b) -> int {
        return thr_extract_submit_card(x, text, text_len, b.off.data(), b.idx.data(), b.ts.data(), b.nb,
                                       b.recs.data(), &b.ticket);
    };
    rc = drive(R, next, submit);
    R.st.bytes_in = pos;
    *stats = R.st;
    return rc;
} catch (...) {
    return thr::on_exception("thr_run_extract_card");
}

int thr_run_extract_stream(thr_handle* h, const uint8_t* stream, size_t n_bytes, int64_t first_block_idx,
                           const thr_run_opts* opts, thr_extract* x, thr_run_stats* stats) try {
    Run R;
    int rc = check("thr_run_extract_stream", h, opts, x, stats, R);
    if (rc != THR_OK) return rc;
    if (!stream && n_bytes) return thr::fail_msg(THR_ERR_ARG, "thr_run_extract_stream: null stream");
    const size_t blk = size_t(R.block_len) * 2, stride = size_t(R.new_len) * 2;
    const size_t total = n_bytes < blk ? 0 : (n_bytes - blk) / stride + 1;
    size_t done = 0;
    auto next = [&](Batch& b) -> int {
        b.nb = std::min(R.max_batch, total - done);
        if (b.nb == 0) return THR_OK;
        // (of a mapped file every block of a batch is "read" at once: one stamp, like thr_run_stream)
        b.ts.assign(1, std::isnan(R.o.timestamp) ? wall_clock() : R.o.timestamp);
        b.idx.assign(1, int64_t(done));
        done += b.nb;
        return THR_OK;
    };
    auto submit = [&](Batch& b) -> int {
        const size_t at = size_t(b.idx[0]);
        size_t got = 0;
        const int src = thr_extract_submit_stream(x, stream + at * stride, (b.nb - 1) * stride + blk,
                                                  first_block_idx + int64_t(at), b.ts[0], b.recs.data(), b.nb, &got,
                                                  &b.ticket);
        if (src == THR_OK && got != b.nb)
            return thr::fail_msg(THR_ERR_STATE, "thr_run_extract_stream: framed %zu blocks, engine took %zu", b.nb, got);
        return src;
    };
    rc = drive(R, next, submit);
    R.st.bytes_in = done ? (done - 1) * stride + blk : 0;
    *stats = R.st;
    return rc;
} catch (...) {
    return thr::on_exception("thr_run_extract_stream");
}

}  // extern "C"
