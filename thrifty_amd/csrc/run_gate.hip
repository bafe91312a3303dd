// thr_run_gate_stream / thr_run_gate_card: the whole `fastcard -i <file> [--card] -o <out.card>` loop in one
// call (fastcard_cli.c:143-196), the twin of run_file.hip's file -> .toad loop.  Built on the public entry
// points and nothing else (thr_gate / thr_gate_stream / thr_gate_card, thr_frame_card): the calling thread
// frames a batch and gates it; a thread of the library assembles the .card lines of the batches handed to
// it -- "<sec>.<usec> <index> " in front of each payload slot -- and writev()s them to `out_fd`, so the text
// of batch i leaves while batch i + 1 is on the device.  kRing batches may be in flight between the two.
#include <sys/uio.h>
#include <unistd.h>

#include <cerrno>
#include <deque>

#include "host_internal.hpp"

namespace {

constexpr int kRing = 3;

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
double wall_s() { return std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count(); }

struct Batch {
    std::vector<char> slots;
    std::vector<thr_record> rec;
    std::vector<double> ts;              // per block
    std::vector<const char*> line;       // .card input: the input line of each block (copied when it passes)
    std::vector<size_t> line_len;
    size_t n = 0, passed = 0;
};

struct Writer {
    int fd;
    size_t stride, chars;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Batch*> todo, spare;
    bool closing = false;
    int err = 0;                          // errno of a failed write
    double format_s = 0, write_s = 0;
    uint64_t text_bytes = 0;
    std::thread th;

    int write_all(std::vector<iovec>& iov) {
        size_t at = 0;
        while (at < iov.size()) {
            const int cnt = int(std::min<size_t>(iov.size() - at, 512));
            ssize_t w = ::writev(fd, iov.data() + at, cnt);
            if (w < 0) {
                if (errno == EINTR) continue;
                return errno;
            }
            text_bytes += uint64_t(w);
            while (w > 0 && at < iov.size()) {          // a short write: go on behind what was taken
                if (size_t(w) >= iov[at].iov_len) {
                    w -= ssize_t(iov[at].iov_len);
                    ++at;
                } else {
                    iov[at].iov_base = static_cast<char*>(iov[at].iov_base) + w;
                    iov[at].iov_len -= size_t(w);
                    w = 0;
                }
            }
        }
        return 0;
    }

    void emit(Batch& b) {
        if (fd < 0 || b.passed == 0) return;
        const double t0 = now_s();
        std::vector<iovec> iov;
        std::vector<char> heads;
        if (!b.line.empty()) {            // .card input: the passed blocks' input lines, unchanged
            static char nl = '\n';
            for (size_t i = 0; i < b.n; ++i)
                if (b.rec[i].flags & THR_FLAG_CARRIER) {
                    iov.push_back(iovec{const_cast<char*>(b.line[i]), b.line_len[i]});
                    iov.push_back(iovec{&nl, 1});
                }
        } else {
            heads.resize(b.passed * THR_CARD_HEADER_MAX);
            std::vector<size_t> head_len(b.passed);
            size_t k = 0;
            for (size_t i = 0; i < b.n; ++i)
                if (b.rec[i].flags & THR_FLAG_CARRIER) {
                    size_t len = 0;
                    // (the header alone: a line without payload ends in "<index> \n"; the newline is dropped)
                    thr_format_card(&b.ts[i], &b.rec[i].block_idx, b.slots.data(), 0, 0, 1,
                                    heads.data() + k * THR_CARD_HEADER_MAX, THR_CARD_HEADER_MAX + 1, &len);
                    head_len[k++] = len ? len - 1 : 0;
                }
            for (size_t s = 0; s < b.passed; ++s) {
                iov.push_back(iovec{heads.data() + s * THR_CARD_HEADER_MAX, head_len[s]});
                iov.push_back(iovec{b.slots.data() + s * stride, chars + 1});
            }
        }
        const double t1 = now_s();
        const int e = write_all(iov);
        const double t2 = now_s();
        std::lock_guard<std::mutex> lk(mu);
        format_s += t1 - t0;
        write_s += t2 - t1;
        if (e && !err) err = e;
    }

    void run() {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv.wait(lk, [&] { return closing || !todo.empty(); });
            if (todo.empty()) return;
            Batch* b = todo.front();
            todo.pop_front();
            const bool skip = err != 0;
            lk.unlock();
            if (!skip) emit(*b);
            lk.lock();
            spare.push_back(b);
            cv.notify_all();
        }
    }

    Batch* take(double* waited) {        // a free batch buffer (waits for the writer when all are in flight)
        std::unique_lock<std::mutex> lk(mu);
        if (spare.empty()) {
            const double t0 = now_s();
            cv.wait(lk, [&] { return !spare.empty(); });
            *waited += now_s() - t0;
        }
        Batch* b = spare.front();
        spare.pop_front();
        return b;
    }
    void give(Batch* b) {
        {
            std::lock_guard<std::mutex> lk(mu);
            todo.push_back(b);
        }
        cv.notify_all();
    }
    void put_back(Batch* b) {
        std::lock_guard<std::mutex> lk(mu);
        spare.push_back(b);
    }
    void finish() {
        {
            std::lock_guard<std::mutex> lk(mu);
            closing = true;
        }
        cv.notify_all();
        if (th.joinable()) th.join();
    }
    ~Writer() { finish(); }      // (an exception between start and finish must not leave the thread joinable)
};

struct Run {
    thr_handle* h;
    const thr_gate_run_opts* o;
    thr_gate_run_stats* st;
    thr_settings cfg{};
    size_t stride = 0, chars = 0, batch = 0;
    Batch ring[kRing];
    Writer w;
    size_t rec_used = 0;

    int start(const char* who) {
        if (!h || !o || !st) return fail(THR_ERR_ARG, "%s: null argument", who);
        std::memset(st, 0, sizeof(*st));
        if (o->struct_bytes != sizeof(thr_gate_run_opts))
            return fail(THR_ERR_ARG, "%s: thr_gate_run_opts of %u bytes, this library's has %zu", who, o->struct_bytes,
                        sizeof(thr_gate_run_opts));
        if (o->skip < 0 || o->batch_blocks < 0) return fail(THR_ERR_ARG, "%s: negative skip or batch_blocks", who);
        if (o->rec_capacity && !o->rec_out) return fail(THR_ERR_ARG, "%s: rec_capacity without rec_out", who);
        int rc = thr_get_settings(h, &cfg);
        if (rc != THR_OK) return rc;
        if ((rc = thr_gate_slot_stride(h, &stride, &chars)) != THR_OK) return rc;
        if (cfg.n_templates != 0) return fail(THR_ERR_STATE, "%s: the handle is not a carrier gate (THR_VARIANT_GATE)", who);
        batch = size_t(o->batch_blocks ? std::min(o->batch_blocks, cfg.max_batch) : cfg.max_batch);
        // (a batch's payload slots: at most about 64 MiB of input's worth)
        batch = std::max<size_t>(1, std::min(batch, (size_t(64) << 20) / (size_t(cfg.block_len) * 2) + 1));
        w.fd = o->out_fd;
        w.stride = stride;
        w.chars = chars;
        for (auto& b : ring) w.spare.push_back(&b);
        w.th = std::thread([this] { w.run(); });
        return THR_OK;
    }

    Batch* next_batch(size_t nb) {
        Batch* b = w.take(&st->wait_s);
        b->slots.resize(nb * stride);
        b->rec.resize(nb);
        b->ts.assign(nb, 0.0);
        b->line.clear();
        b->line_len.clear();
        b->n = nb;
        b->passed = 0;
        return b;
    }

    int done_batch(Batch* b, int rc) {
        if (rc != THR_OK) {
            w.put_back(b);
            return rc;
        }
        st->blocks += b->n;
        st->passed += b->passed;
        st->batches += 1;
        if (o->rec_out) {
            if (rec_used + b->n > o->rec_capacity) {
                w.put_back(b);
                return fail(THR_ERR_ARG, "thr_run_gate: rec_out holds %zu records, the input has more blocks", o->rec_capacity);
            }
            std::memcpy(o->rec_out + rec_used, b->rec.data(), b->n * sizeof(thr_record));
            rec_used += b->n;
        }
        w.give(b);
        std::lock_guard<std::mutex> lk(w.mu);
        return w.err ? fail(THR_ERR_DEVICE, "thr_run_gate: write to descriptor %d failed: %s", w.fd, std::strerror(w.err))
                     : THR_OK;
    }

    int finish(int rc, double t_start) {
        w.finish();
        st->format_s = w.format_s;
        st->write_s = w.write_s;
        st->text_bytes = w.text_bytes;
        st->total_s = now_s() - t_start;
        if (rc == THR_OK && w.err)
            rc = fail(THR_ERR_DEVICE, "thr_run_gate: write to descriptor %d failed: %s", w.fd, std::strerror(w.err));
        return rc;
    }
};

}  // namespace

extern "C" {

int thr_run_gate_stream(thr_handle* h, const uint8_t* stream, size_t n_bytes, int64_t first_block_idx,
                        const thr_gate_run_opts* opts, thr_gate_run_stats* stats) try {
    const double t_start = now_s();
    Run r{h, opts, stats};
    int rc = r.start("thr_run_gate_stream");
    if (rc != THR_OK) return rc;
    if (!stream && n_bytes) return r.finish(fail(THR_ERR_ARG, "thr_run_gate_stream: null stream"), t_start);
    const size_t n = size_t(r.cfg.block_len), hist = size_t(r.cfg.history_len);
    const size_t step = 2 * (n - hist), blk = 2 * n;
    if (step % 4 != 0)
        return r.finish(fail(THR_ERR_ARG, "raw-stream framing needs an even block_len - history_len (got %zu)", n - hist),
                        t_start);
    // raw_reader.c:15-46 + fastcard_cli.c:151-169: the reader takes `step` new bytes per block, the first
    // `skip` blocks are dropped; kept block i starts step * (i + skip) - 2 * history bytes into the stream
    const size_t skip = size_t(opts->skip);
    const size_t read = n_bytes / step, total = read > skip ? read - skip : 0;
    stats->bytes_in = n_bytes;
    size_t i = 0;
    while (i < total && rc == THR_OK) {
        double t0 = now_s();
        const long long off = (long long)(step * (i + skip)) - (long long)(2 * hist);
        size_t nb;
        Batch* b;
        if (off < 0) {
            // blocks that start in front of the stream: the missing history is zero bytes, packed on the host
            nb = 0;
            while (i + nb < total && nb < r.batch && (long long)(step * (i + nb + skip)) < (long long)(2 * hist)) ++nb;
            std::vector<uint8_t> lead(nb * blk, 0);
            for (size_t k = 0; k < nb; ++k) {
                const size_t pad = 2 * hist - step * (i + k + skip);
                std::memcpy(lead.data() + k * blk + pad, stream, blk - pad);
            }
            std::vector<int64_t> idx(nb);
            for (size_t k = 0; k < nb; ++k) idx[k] = first_block_idx + int64_t(i + k);
            b = r.next_batch(nb);
            b->ts.assign(nb, std::isnan(opts->timestamp) ? wall_s() : opts->timestamp);
            stats->frame_s += now_s() - t0;
            t0 = now_s();
            rc = thr_gate(h, lead.data(), idx.data(), nb, b->rec.data(), &b->passed, b->slots.data(), b->slots.size());
        } else {
            nb = std::min(r.batch, total - i);
            b = r.next_batch(nb);
            b->ts.assign(nb, std::isnan(opts->timestamp) ? wall_s() : opts->timestamp);
            stats->frame_s += now_s() - t0;
            t0 = now_s();
            size_t got = 0;
            rc = thr_gate_stream(h, stream + off, (nb - 1) * step + blk, first_block_idx + int64_t(i), b->rec.data(), nb,
                                 &got, &b->passed, b->slots.data(), b->slots.size());
            if (rc == THR_OK && got != nb) rc = fail(THR_ERR_STATE, "thr_run_gate_stream: framed %zu blocks, gated %zu", nb, got);
        }
        stats->gate_s += now_s() - t0;
        rc = r.done_batch(b, rc);
        i += nb;
    }
    return r.finish(rc, t_start);
} catch (...) {
    return thr::on_exception("thr_run_gate_stream");
}

int thr_run_gate_card(thr_handle* h, const char* text, size_t text_len, const thr_gate_run_opts* opts,
                      thr_gate_run_stats* stats) try {
    const double t_start = now_s();
    Run r{h, opts, stats};
    int rc = r.start("thr_run_gate_card");
    if (rc != THR_OK) return rc;
    if (!text && text_len) return r.finish(fail(THR_ERR_ARG, "thr_run_gate_card: null text"), t_start);
    stats->bytes_in = text_len;
    size_t pos = 0, skip = size_t(opts->skip);
    std::vector<double> ts(r.batch);
    std::vector<int64_t> idx(r.batch), off(r.batch);
    while (pos < text_len && rc == THR_OK) {
        double t0 = now_s();
        size_t nrec = 0, used = 0;
        rc = thr_frame_card(text + pos, text_len - pos, r.cfg.block_len, 1, r.batch, ts.data(), idx.data(), off.data(),
                            &nrec, &used);
        if (rc != THR_OK) break;
        if (used == 0 && nrec == 0) break;
        const size_t drop = std::min(skip, nrec);       // (the first `skip` blocks are read and dropped)
        skip -= drop;
        const size_t nb = nrec - drop;
        if (nb == 0) {
            pos += used;
            stats->frame_s += now_s() - t0;
            continue;
        }
        Batch* b = r.next_batch(nb);
        b->line.resize(nb);
        b->line_len.resize(nb);
        for (size_t k = 0; k < nb; ++k) {
            const char* pay = text + pos + off[drop + k];
            const char* ls = pay;
            while (ls > text && ls[-1] != '\n') --ls;    // (the two short header fields in front of the payload)
            b->line[k] = ls;
            b->line_len[k] = size_t(pay - ls) + r.chars;
            b->ts[k] = ts[drop + k];
        }
        stats->frame_s += now_s() - t0;
        t0 = now_s();
        rc = thr_gate_card(h, text + pos, text_len - pos, off.data() + drop, idx.data() + drop, nb, b->rec.data(),
                           &b->passed, b->slots.data(), b->slots.size());
        stats->gate_s += now_s() - t0;
        rc = r.done_batch(b, rc);
        pos += used;
    }
    return r.finish(rc, t_start);
} catch (...) {
    return thr::on_exception("thr_run_gate_card");
}

}  // extern "C"
