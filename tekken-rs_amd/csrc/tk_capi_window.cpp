// tk_capi_window.cpp -- overlapping windows for long documents (include/tekken_hip.h tk_window_from_ids_device and the entries
// around it; csrc/tk_window.hip): every document longer than max_length split into windows that overlap by stride ids, with the
// mapping back to the documents.
#include "tk_capi_layout.h"

#define TK_WINDOW_ALL_FLAGS (TK_WINDOW_FIXED | TK_WINDOW_I64 | TK_WINDOW_MASK | TK_WINDOW_SPANS)

// the options that can be refused before anything is enqueued (step 8 of the definition)
static int window_check_opts(tk_ctx* c, const tk_window_opts* o) {
    if (!o) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    if (o->flags & ~(uint32_t)TK_WINDOW_ALL_FLAGS) { c->err = "unknown window flag"; return TK_ERR_INVALID_ARG; }
    if (o->max_length == 0) { c->err = "windows need a max_length"; return TK_ERR_INVALID_ARG; }
    if (o->max_length > TK_LAYOUT_MAX_ROW) { c->err = "max_length " + std::to_string(o->max_length) + " is beyond 2^31 - 1"; return TK_ERR_INVALID_ARG; }
    if ((uint64_t)o->keep_head + o->keep_tail >= o->max_length) {
        c->err = "keep_head + keep_tail leave no room for text in max_length " + std::to_string(o->max_length);
        return TK_ERR_INVALID_ARG;
    }
    if (o->stride >= o->max_length - o->keep_head - o->keep_tail) {
        c->err = "stride " + std::to_string(o->stride) + " is not below the " + std::to_string(o->max_length - o->keep_head - o->keep_tail) +
                 " body ids of a window";
        return TK_ERR_INVALID_ARG;
    }
    return TK_OK;
}
// the options of an entry that encodes first: BOS / EOS are what every window repeats
static int window_encode_opts(tk_ctx* c, const tk_window_opts* opts, int add_bos, int add_eos, tk_window_opts* o) {
    *o = *opts;
    o->keep_head = add_bos ? 1u : 0u;
    o->keep_tail = add_eos ? 1u : 0u;
    return window_check_opts(c, o);
}
static uint64_t round_up(uint64_t L, uint64_t m) { return m ? (L + m - 1) / m * m : L; }

// The window pass over ids on the device into the context's c->window buffers; *out gets the device pointers.  The per-document counts
// and their scan go to work buffers; ONE read (W, the longest document, n_split) sizes the tensor, and only once the sizes are
// accepted is anything of an earlier result touched (the scan becomes doc_windows by a swap of the two buffers).  One wait ends
// the call.  The caller holds c->mu.
static int run_window(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t n_ids,
                      const uint32_t* d_spans, const tk_window_opts* o, hipStream_t s, tk_window* out) {
    int rc = window_check_opts(c, o);
    if (rc != TK_OK) return rc;
    if ((rc = check_n_docs(c, n_docs)) != TK_OK) return rc;
    if (n_docs == 0 && n_ids) { c->err = "windows: ids without a document"; return TK_ERR_INVALID_ARG; }
    const bool fixed = (o->flags & TK_WINDOW_FIXED) != 0, i64 = (o->flags & TK_WINDOW_I64) != 0, mask = (o->flags & TK_WINDOW_MASK) != 0,
               spans = (o->flags & TK_WINDOW_SPANS) != 0;
    if (spans && !d_spans) { c->err = "TK_WINDOW_SPANS needs a spans buffer"; return TK_ERR_INVALID_ARG; }
    if (fixed && round_up(o->max_length, o->multiple_of) > TK_LAYOUT_MAX_ROW) {
        c->err = "windows: max_length rounded up to a multiple of " + std::to_string(o->multiple_of) + " is beyond 2^31 - 1";
        return TK_ERR_INVALID_ARG;
    }
    TK_HIP(c, c->window.stat.reserve(64));
    TK_HIP(c, c->window.cnt.reserve(n_docs * 4 + 16));
    TK_HIP(c, c->window.dw_next.reserve((n_docs + 1) * 8));
    TK_HIP(c, c->window.bsum.reserve(scan_workspace_bytes(n_docs)));
    TkWindowArgs a;
    memset(&a, 0, sizeof(a));
    a.ids = d_ids;
    a.id_offs = d_id_offs;
    a.in_spans = d_spans;
    a.n_docs = n_docs;
    a.max_len = o->max_length;
    a.step = o->max_length - o->keep_head - o->keep_tail - o->stride;
    a.keep_head = o->keep_head;
    a.keep_tail = o->keep_tail;
    a.pad_id = o->pad_id;
    a.counts = (uint32_t*)c->window.cnt.p;
    a.stat = (unsigned long long*)c->window.stat.p;
    unsigned long long stat[2] = {0, 0};            // the longest document | the split ones
    uint64_t W = 0;
    if (n_docs == 0) {
        TK_HIP(c, hipMemsetAsync(c->window.dw_next.p, 0, 8, s));
    } else {
        TK_HIP(c, hipMemsetAsync(a.stat, 0, 16, s));
        TK_HIP(c, tk_launch_window_counts(a, s));
        if ((rc = scan_u32(c, c->window.bsum, a.counts, n_docs, (uint64_t*)c->window.dw_next.p, s)) != TK_OK) return rc;
        TK_HIP(c, hipMemcpyAsync(&W, (const uint64_t*)c->window.dw_next.p + n_docs, 8, hipMemcpyDeviceToHost, s));
        TK_HIP(c, hipMemcpyAsync(stat, a.stat, 16, hipMemcpyDeviceToHost, s));
    }
    TK_HIP(c, hipStreamSynchronize(s));
    if (stat[0] >= 0xFFFFFFFFull) { c->err = "windows: a document reaches 2^32 - 1 ids (window_start is uint32)"; return TK_ERR_INVALID_ARG; }
    const uint64_t L = round_up(fixed || stat[0] > o->max_length ? o->max_length : stat[0], o->multiple_of);
    if (L > TK_LAYOUT_MAX_ROW || W >= (1ull << 32) || (W && L > TK_LAYOUT_MAX_ELEMS / W)) {
        c->err = "windows: " + std::to_string(W) + " rows of " + std::to_string(L) + " elements are beyond what one tensor can hold";
        return TK_ERR_INVALID_ARG;
    }
    const uint64_t elems = W * L;
    TK_HIP(c, c->window.ids.reserve(elems * (i64 ? 8 : 4) + 16));
    if (mask) TK_HIP(c, c->window.mask.reserve(elems + 16));
    if (spans) TK_HIP(c, c->window.spans.reserve(elems * 8 + 16));
    TK_HIP(c, c->window.len.reserve(W * 4 + 16));
    TK_HIP(c, c->window.doc.reserve(W * 4 + 16));
    TK_HIP(c, c->window.start.reserve(W * 4 + 16));
    std::swap(c->window.dw, c->window.dw_next);
    a.row_len = (uint32_t)L;
    a.n_rows = W;
    a.doc_windows = (const uint64_t*)c->window.dw.p;
    a.out = c->window.ids.p;
    a.mask = mask ? (uint8_t*)c->window.mask.p : nullptr;
    a.out_spans = spans ? (uint32_t*)c->window.spans.p : nullptr;
    a.lengths = (uint32_t*)c->window.len.p;
    a.window_doc = (uint32_t*)c->window.doc.p;
    a.window_start = (uint32_t*)c->window.start.p;
    TK_HIP(c, tk_launch_window(a, i64, s));
    TK_HIP(c, hipStreamSynchronize(s));
    out->input_ids = c->window.ids.p;
    out->mask = a.mask;
    out->lengths = a.lengths;
    out->window_doc = a.window_doc;
    out->window_start = a.window_start;
    out->doc_windows = (uint64_t*)c->window.dw.p;
    out->spans = a.out_spans;
    out->n_docs = n_docs;
    out->n_windows = W;
    out->row_len = L;
    out->n_split = stat[1];
    return TK_OK;
}

namespace {
struct WindowPass : LayoutPass<WindowPass> {
    typedef tk_window_opts Opts;
    typedef tk_window Result;
    static constexpr const char* name = "window";
    static uint64_t esz(const Opts& o) { return (o.flags & TK_WINDOW_I64) ? 8 : 4; }
    static constexpr auto encode_opts = window_encode_opts;
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
