// tk_capi_pair.cpp -- sentence-pair rows (include/tekken_hip.h tk_pair_from_ids_device and the entries around it; csrc/tk_pair.hip):
// the ids of two texts a pair put into rows head + A + sep + B + tail, cut by one of three strategies, the windowed side split into
// overlapping windows, with type ids, sequence ids and the mapping back to the pairs.
#include "tk_capi_layout.h"

#define TK_PAIR_ALL_FLAGS (TK_PAIR_FIXED | TK_PAIR_I64 | TK_PAIR_MASK | TK_PAIR_SPANS | TK_PAIR_TYPE_IDS | TK_PAIR_SEQUENCE_IDS | TK_PAIR_OVERFLOW)

// the options that can be refused before anything is enqueued (step 8 of the definition)
static int pair_check_opts(tk_ctx* c, const tk_pair_opts* o) {
    if (!o) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    if (o->flags & ~(uint32_t)TK_PAIR_ALL_FLAGS) { c->err = "unknown pair flag"; return TK_ERR_INVALID_ARG; }
    if (o->strategy > TK_PAIR_ONLY_SECOND) { c->err = "unknown pair strategy " + std::to_string(o->strategy); return TK_ERR_INVALID_ARG; }
    if (o->n_head > 4 || o->n_sep > 4 || o->n_tail > 4) { c->err = "pairs: head, sep and tail hold at most 4 ids each"; return TK_ERR_INVALID_ARG; }
    if (o->max_length == 0) { c->err = "pairs need a max_length"; return TK_ERR_INVALID_ARG; }
    if (o->max_length > TK_LAYOUT_MAX_ROW) { c->err = "max_length " + std::to_string(o->max_length) + " is beyond 2^31 - 1"; return TK_ERR_INVALID_ARG; }
    const uint32_t x = o->n_head + o->n_sep + o->n_tail;
    if (o->max_length < x + 2u) {
        c->err = "the " + std::to_string(x) + " fixed ids leave fewer than 2 ids for the texts in max_length " + std::to_string(o->max_length);
        return TK_ERR_INVALID_ARG;
    }
    const uint32_t cap = o->max_length - x;
    if (o->strategy == TK_PAIR_LONGEST_FIRST) {
        if ((o->flags & TK_PAIR_OVERFLOW) || o->stride) { c->err = "pairs: overflow and stride need only_first or only_second"; return TK_ERR_INVALID_ARG; }
        return TK_OK;
    }
    if (o->max_fixed > cap - 1u) {
        c->err = "max_fixed " + std::to_string(o->max_fixed) + " leaves no room for the windowed side in " + std::to_string(cap) + " ids";
        return TK_ERR_INVALID_ARG;
    }
    const uint32_t F = o->max_fixed ? o->max_fixed : cap - 1u;
    if (o->stride >= cap - F) {
        c->err = "stride " + std::to_string(o->stride) + " is not below the " + std::to_string(cap - F) + " ids a window has at least";
        return TK_ERR_INVALID_ARG;
    }
    return TK_OK;
}
// the options of the entries that encode first: the parts are encoded without BOS / EOS, the template is all in opts
static int pair_encode_opts(tk_ctx* c, const tk_pair_opts* opts, int, int, tk_pair_opts* o) {
    const int rc = pair_check_opts(c, opts);
    if (rc == TK_OK) *o = *opts;
    return rc;
}

// The pair pass over ids on the device into the context's c->pair buffers; *out gets the device pointers.  The tensors are sized by
// the three steps of tk_capi_layout.h (ONE read: W and the statistics words), and only once the sizes are accepted is anything of an
// earlier result touched (the scan becomes pair_windows by a swap of the two buffers).  One wait ends the call.  The caller holds
// c->mu.
static int run_pair(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_parts, uint64_t n_ids, const uint32_t* d_spans,
                    const tk_pair_opts* o, hipStream_t s, tk_pair* out) {
    int rc = pair_check_opts(c, o);
    if (rc != TK_OK) return rc;
    if (n_parts & 1u) { c->err = "pairs: " + std::to_string(n_parts) + " parts are not pairs"; return TK_ERR_INVALID_ARG; }
    if ((rc = check_n_docs(c, n_parts)) != TK_OK) return rc;
    if (n_parts == 0 && n_ids) { c->err = "pairs: ids without a part"; return TK_ERR_INVALID_ARG; }
    const uint32_t fl = o->flags;
    const bool fixed = (fl & TK_PAIR_FIXED) != 0, i64 = (fl & TK_PAIR_I64) != 0, spans = (fl & TK_PAIR_SPANS) != 0;
    if (spans && !d_spans) { c->err = "TK_PAIR_SPANS needs a spans buffer"; return TK_ERR_INVALID_ARG; }
    if ((rc = layout_check_fixed_len(c, "pairs", fixed, o->max_length, o->multiple_of)) != TK_OK) return rc;
    const uint64_t P = n_parts / 2;
    TkPairArgs a;
    memset(&a, 0, sizeof(a));
    a.ids = d_ids;
    a.id_offs = d_id_offs;
    a.in_spans = d_spans;
    a.n_pairs = P;
    a.max_len = o->max_length;
    a.n_head = o->n_head; a.n_sep = o->n_sep; a.n_tail = o->n_tail;
    memcpy(a.head, o->head, sizeof(a.head));
    memcpy(a.sep, o->sep, sizeof(a.sep));
    memcpy(a.tail, o->tail, sizeof(a.tail));
    a.cap = o->max_length - o->n_head - o->n_sep - o->n_tail;
    a.strategy = o->strategy;
    a.overflow = (fl & TK_PAIR_OVERFLOW) ? 1u : 0u;
    a.stride = o->stride;
    a.max_fixed = o->max_fixed ? o->max_fixed : a.cap - 1u;
    a.pad_id = o->pad_id;
    unsigned long long stat[5];                     // the longest row | truncated | split | fixed side cut | the longest part
    uint64_t W, L;
    rc = layout_count_rows(c, P, c->pair.stat, c->pair.cnt, c->pair.pw_next, c->pair.bsum, stat, 5, s, [&](uint32_t* counts, unsigned long long* d_stat) {
        a.counts = counts;
        a.stat = d_stat;
        return tk_launch_pair_counts(a, s);
    }, &W);
    if (rc != TK_OK) return rc;
    if (stat[4] >= 0xFFFFFFFFull) { c->err = "pairs: a part reaches 2^32 - 1 ids (window_start is uint32)"; return TK_ERR_INVALID_ARG; }
    if ((rc = layout_row_len(c, "pairs", fixed, stat[0], o->max_length, o->multiple_of, W, &L)) != TK_OK) return rc;
    const uint64_t elems = W * L;
    TK_HIP(c, c->pair.ids.reserve(elems * (i64 ? 8 : 4) + 16));
    if (fl & TK_PAIR_MASK) TK_HIP(c, c->pair.mask.reserve(elems + 16));
    if (fl & TK_PAIR_TYPE_IDS) TK_HIP(c, c->pair.type.reserve(elems + 16));
    if (fl & TK_PAIR_SEQUENCE_IDS) TK_HIP(c, c->pair.seq.reserve(elems + 16));
    if (spans) TK_HIP(c, c->pair.spans.reserve(elems * 8 + 16));
    TK_HIP(c, c->pair.len.reserve(W * 4 + 16));
    TK_HIP(c, c->pair.pair.reserve(W * 4 + 16));
    TK_HIP(c, c->pair.start.reserve(W * 4 + 16));
    TK_HIP(c, c->pair.second.reserve(W * 4 + 16));
    std::swap(c->pair.pw, c->pair.pw_next);
    a.row_len = (uint32_t)L;
    a.n_rows = W;
    a.pair_windows = (const uint64_t*)c->pair.pw.p;
    a.out = c->pair.ids.p;
    a.mask = (fl & TK_PAIR_MASK) ? (uint8_t*)c->pair.mask.p : nullptr;
    a.type_ids = (fl & TK_PAIR_TYPE_IDS) ? (uint8_t*)c->pair.type.p : nullptr;
    a.seq_ids = (fl & TK_PAIR_SEQUENCE_IDS) ? (uint8_t*)c->pair.seq.p : nullptr;
    a.out_spans = spans ? (uint32_t*)c->pair.spans.p : nullptr;
    a.lengths = (uint32_t*)c->pair.len.p;
    a.window_pair = (uint32_t*)c->pair.pair.p;
    a.window_start = (uint32_t*)c->pair.start.p;
    a.second_start = (uint32_t*)c->pair.second.p;
    TK_HIP(c, tk_launch_pair(a, i64, s));
    TK_HIP(c, hipStreamSynchronize(s));
    out->input_ids = c->pair.ids.p;
    out->mask = a.mask;
    out->type_ids = a.type_ids;
    out->sequence_ids = a.seq_ids;
    out->lengths = a.lengths;
    out->window_pair = a.window_pair;
    out->window_start = a.window_start;
    out->second_start = a.second_start;
    out->spans = a.out_spans;
    out->pair_windows = (uint64_t*)c->pair.pw.p;
    out->n_pairs = P;
    out->n_windows = W;
    out->row_len = L;
    out->n_truncated = stat[1];
    out->n_split = stat[2];
    out->n_fixed_cut = stat[3];
    return TK_OK;
}

namespace {
struct PairPass : LayoutPass<PairPass> {
    typedef tk_pair_opts Opts;
    typedef tk_pair Result;
    static constexpr const char* name = "pair";
    static uint64_t esz(const Opts& o) { return (o.flags & TK_PAIR_I64) ? 8 : 4; }
    static constexpr auto encode_opts = pair_encode_opts;
    static constexpr auto run = run_pair;
    // behind an encode the spans are the spans pass's own, which runs in front where they are asked for
    static int run_encoded(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_parts, uint64_t n_ids, const Opts* o, hipStream_t s,
                           Result* out) {
        if (o->flags & TK_PAIR_SPANS) {
            int rc = run_spans(c, d_ids, d_id_offs, n_parts, n_ids, nullptr, nullptr, 0, s, nullptr);
            if (rc != TK_OK) return rc;
        }
        return run_pair(c, d_ids, d_id_offs, n_parts, n_ids, (const uint32_t*)c->spans.spans.p, o, s, out);
    }
};
}  // namespace

extern "C" int tk_pair_from_ids_device(tk_ctx* c, const void* d_ids, const void* d_id_offsets, uint64_t n_parts, uint64_t n_ids,
                                       const void* d_spans, const tk_pair_opts* opts, void* hip_stream, tk_pair* out) {
    return layout_from_ids_device<PairPass>(c, d_ids, d_id_offsets, n_parts, n_ids, opts, hip_stream, out, (const uint32_t*)d_spans);
}
extern "C" int tk_encode_pairs_device(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_parts, uint64_t n_bytes, int checks,
                                      const tk_pair_opts* opts, void* hip_stream, void** d_ids, void** d_out_offsets, uint64_t* n_ids,
                                      tk_pair* out) {
    return layout_encode_device<PairPass>(c, d_bytes, d_doc_offsets, n_parts, n_bytes, 0, 0, checks, opts, hip_stream, d_ids, d_out_offsets, n_ids,
                                          out);
}
extern "C" int tk_encode_pairs(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_parts, int validate_utf8,
                               const tk_pair_opts* opts, tk_pair* out) {
    return layout_encode_host<PairPass>(c, bytes, doc_offsets, n_parts, 0, 0, validate_utf8, opts, out);
}
extern "C" void tk_free_pair(tk_pair* r) { layout_free(r); }
