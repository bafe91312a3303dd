// thr_run_extract_card / thr_run_extract_stream: the whole-capture loop of a template extraction in one
// call -- thr_run_card / thr_run_stream (run_file.hip) with the extraction's fold and keep enqueued
// behind every batch (thr_extract_submit_card / thr_extract_submit_stream) and nothing else per batch:
// the calling thread frames, keeps up to THR_MAX_IN_FLIGHT batches submitted and collects them in order.
// What a collected batch is looked at for is the reference's IndexError block (the run ends there) and
// the detection count; .toad text is formatted only when an output descriptor was given, records are
// appended only when an array was.  The loop, the framers and the sink are run_loop.hpp's, shared with
// run_file.hip; like that file this one is built on the public entry points: all it reads of an extraction
// is the handle it belongs to.
#include "run_loop.hpp"
#include "template_extract.hpp"

namespace {

using namespace thr::run;

// drive()'s `D` (run_loop.hpp): a collected batch goes through the sink on the calling thread, so as many
// batches as may be in flight are enough
struct Inline {
    Run& R;
    Sink sink;
    std::vector<Batch> ring;
    std::deque<int> spare;

    explicit Inline(Run& r) : R(r), sink(r), ring(size_t(THR_MAX_IN_FLIGHT)) {
        for (int i = 0; i < THR_MAX_IN_FLIGHT; ++i) spare.push_back(i);
    }
    bool ended() const { return sink.ended(); }      // the index-error block, or an output error
    int acquire() {
        const int s = spare.front();
        spare.pop_front();
        return s;
    }
    void release(int s) { spare.push_back(s); }
    void deliver(int s) {                            // (behind the end of the run: waited for and dropped)
        if (!sink.ended()) R.st.blocks += sink.take(ring[size_t(s)]);
        release(s);
    }
    void finish() {}
};

const char* const INDEX_TAIL = "blocks behind it were already folded: reset the extraction";

}  // namespace

extern "C" {

int thr_run_extract_card(thr_handle* h, const char* text, size_t text_len, const thr_run_opts* opts,
                         thr_extract* x, thr_run_stats* stats) try {
    Run R{"thr_run_extract", INDEX_TAIL};
    int rc = check("thr_run_extract_card", h, opts, stats, false, x ? x->h : nullptr, R);
    if (rc != THR_OK) return rc;
    if (!text && text_len) return thr::fail_msg(THR_ERR_ARG, "thr_run_extract_card: null text");
    CardFramer next{R, text, text_len};
    rc = drive<Inline>(R, next, [&](Batch& b) -> int {
        return thr_extract_submit_card(x, text, text_len, b.off.data(), b.idx.data(), b.ts.data(), b.nb,
                                       b.recs.data(), &b.ticket);
    });
    R.st.bytes_in = next.pos;
    *stats = R.st;
    return rc;
} catch (...) {
    return thr::on_exception("thr_run_extract_card");
}

int thr_run_extract_stream(thr_handle* h, const uint8_t* stream, size_t n_bytes, int64_t first_block_idx,
                           const thr_run_opts* opts, thr_extract* x, thr_run_stats* stats) try {
    Run R{"thr_run_extract", INDEX_TAIL};
    int rc = check("thr_run_extract_stream", h, opts, stats, false, x ? x->h : nullptr, R);
    if (rc != THR_OK) return rc;
    if (!stream && n_bytes) return thr::fail_msg(THR_ERR_ARG, "thr_run_extract_stream: null stream");
    StreamFramer next(R, n_bytes);
    rc = drive<Inline>(R, next, [&](Batch& b) -> int {
        size_t got = 0;
        const int src = thr_extract_submit_stream(x, stream + next.offset(b), next.bytes(b), first_block_idx + b.idx[0],
                                                  b.ts[0], b.recs.data(), b.nb, &got, &b.ticket);
        if (src == THR_OK && got != b.nb)
            return thr::fail_msg(THR_ERR_STATE, "thr_run_extract_stream: framed %zu blocks, engine took %zu", b.nb, got);
        return src;
    });
    R.st.bytes_in = next.bytes_in();
    *stats = R.st;
    return rc;
} catch (...) {
    return thr::on_exception("thr_run_extract_stream");
}

}  // extern "C"
