// tk_capi_window.cpp -- overlapping windows for long documents (include/tekken_hip.h tk_window_from_ids_device and the entries
// around it; csrc/tk_window.hip): every document longer than max_length split into windows that overlap by stride ids, with the
// mapping back to the documents.
#include "tk_capi_layout.h"

#define TK_WINDOW_ALL_FLAGS (TK_WINDOW_FIXED | TK_WINDOW_I64 | TK_WINDOW_MASK | TK_WINDOW_SPANS)

// the options that can be refused before anything is enqueued (step 8 of the definition)
static int window_check_opts(tk_ctx* c, const tk_window_opts* o) {
    if (!o) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    if (o->flags & ~(uint32_t)TK_WINDOW_ALL_FLAGS) { c->err = "unknown window flag"; return TK_ERR_INVALID_ARG; }
    const int rc = rowfill_check_opts(c, "windows", o);
    if (rc != TK_OK) return rc;
    if (o->stride >= o->max_length - o->keep_head - o->keep_tail) {
        c->err = "stride " + std::to_string(o->stride) + " is not below the " + std::to_string(o->max_length - o->keep_head - o->keep_tail) +
                 " body ids of a window";
        return TK_ERR_INVALID_ARG;
    }
    return TK_OK;
}

// The window pass over ids on the device into the context's c->window buffers; *out gets the device pointers.  The tensor is sized
// by the three steps of tk_capi_layout.h (ONE read: W, the longest document, n_split), and only once the sizes are accepted is
// anything of an earlier result touched (rowfill_outputs).  One wait ends the call.  The caller holds c->mu.
static int run_window(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t n_ids,
                      const uint32_t* d_spans, const tk_window_opts* o, hipStream_t s, tk_window* out) {
    int rc = window_check_opts(c, o);
    if (rc != TK_OK) return rc;
    if ((rc = check_n_docs(c, n_docs)) != TK_OK) return rc;
    if (n_docs == 0 && n_ids) { c->err = "windows: ids without a document"; return TK_ERR_INVALID_ARG; }
    const bool fixed = (o->flags & TK_WINDOW_FIXED) != 0, i64 = (o->flags & TK_WINDOW_I64) != 0, mask = (o->flags & TK_WINDOW_MASK) != 0,
               spans = (o->flags & TK_WINDOW_SPANS) != 0;
    if (spans && !d_spans) { c->err = "TK_WINDOW_SPANS needs a spans buffer"; return TK_ERR_INVALID_ARG; }
    if ((rc = layout_check_fixed_len(c, "windows", fixed, o->max_length, o->multiple_of)) != TK_OK) return rc;
    WindowBufs& b = c->window;
    TkWindowArgs a;
    memset(&a, 0, sizeof(a));
    rowfill_inputs(a, d_ids, d_id_offs, d_spans, n_docs, o);
    a.step = o->max_length - o->keep_head - o->keep_tail - o->stride;
    unsigned long long stat[2];                     // the longest document | the split ones
    uint64_t W, L;
    rc = layout_count_rows(c, n_docs, b.stat, b.cnt, b.dw_next, b.bsum, stat, 2, s, [&](uint32_t* counts, unsigned long long* d_stat) {
        a.counts = counts;
        a.stat = d_stat;
        return tk_launch_window_counts(a, s);
    }, &W);
    if (rc != TK_OK) return rc;
    if (stat[0] >= 0xFFFFFFFFull) { c->err = "windows: a document reaches 2^32 - 1 ids (window_start is uint32)"; return TK_ERR_INVALID_ARG; }
    rc = layout_row_len(c, "windows", fixed, stat[0] < o->max_length ? stat[0] : o->max_length, o->max_length, o->multiple_of, W, &L);
    if (rc != TK_OK) return rc;
    if ((rc = rowfill_outputs(c, b, a, W, L, i64, mask, spans)) != TK_OK) return rc;
    TK_HIP(c, tk_launch_window(a, i64, s));
    TK_HIP(c, hipStreamSynchronize(s));
    rowfill_result(a, stat[1], out);
    return TK_OK;
}

namespace {
struct WindowPass : LayoutPass<WindowPass> {
    typedef tk_window_opts Opts;
    typedef tk_window Result;
    static constexpr const char* name = "window";
    static uint64_t esz(const Opts& o) { return (o.flags & TK_WINDOW_I64) ? 8 : 4; }
    static constexpr auto encode_opts = rowfill_encode_opts<tk_window_opts, window_check_opts>;
    static constexpr auto run = run_window;
    // behind an encode the spans are the spans pass's own, which runs in front where they are asked for
    static int run_encoded(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t n_ids, const Opts* o, hipStream_t s,
                           Result* out) {
        if (o->flags & TK_WINDOW_SPANS) {
            int rc = run_spans(c, d_ids, d_id_offs, n_docs, n_ids, nullptr, nullptr, 0, s, nullptr);
            if (rc != TK_OK) return rc;
        }
        return run_window(c, d_ids, d_id_offs, n_docs, n_ids, (const uint32_t*)c->spans.spans.p, o, s, out);
    }
};
}  // namespace

extern "C" int tk_window_from_ids_device(tk_ctx* c, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                                         const void* d_spans, const tk_window_opts* opts, void* hip_stream, tk_window* out) {
    return layout_from_ids_device<WindowPass>(c, d_ids, d_id_offsets, n_docs, n_ids, opts, hip_stream, out, (const uint32_t*)d_spans);
}
extern "C" int tk_encode_batch_device_window(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs,
                                             uint64_t n_bytes, int add_bos, int add_eos, int checks, const tk_window_opts* opts,
                                             void* hip_stream, void** d_ids, void** d_out_offsets, uint64_t* n_ids, tk_window* out) {
    return layout_encode_device<WindowPass>(c, d_bytes, d_doc_offsets, n_docs, n_bytes, add_bos, add_eos, checks, opts, hip_stream, d_ids,
                                            d_out_offsets, n_ids, out);
}
extern "C" int tk_encode_batch_window(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos,
                                      int add_eos, int validate_utf8, const tk_window_opts* opts, tk_window* out) {
    return layout_encode_host<WindowPass>(c, bytes, doc_offsets, n_docs, add_bos, add_eos, validate_utf8, opts, out);
}
extern "C" void tk_free_window(tk_window* r) { layout_free(r); }
