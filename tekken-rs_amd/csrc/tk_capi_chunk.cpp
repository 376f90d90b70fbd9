// tk_capi_chunk.cpp -- boundary-aware token-budget chunks (include/tekken_hip.h tk_chunk_from_ids_device and the entries around it;
// csrc/tk_chunk.hip): every document longer than max_length cut at the strongest break of the text that a chunk can end at, with the
// mapping back to the documents.  The from-ids entry is the scaffold's (tk_capi_layout.h); the entries that encode first are this
// pass's own: they take the text a second time, for the levels.
#include "tk_capi_layout.h"

#define TK_CHUNK_ALL_FLAGS (TK_CHUNK_FIXED | TK_CHUNK_I64 | TK_CHUNK_MASK | TK_CHUNK_SPANS | TK_CHUNK_BYTES)

static int chunk_check_levels(tk_ctx* c, uint32_t levels) {
    if (levels & ~(uint32_t)TK_CHUNK_LEVELS_ALL) { c->err = "chunks: a levels bit outside 1 << 2 .. 1 << 5"; return TK_ERR_INVALID_ARG; }
    return TK_OK;
}
// the options that can be refused before anything is enqueued
static int chunk_check_opts(tk_ctx* c, const tk_chunk_opts* o) {
    if (!o) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    if (o->flags & ~(uint32_t)TK_CHUNK_ALL_FLAGS) { c->err = "unknown chunk flag"; return TK_ERR_INVALID_ARG; }
    const int rc = rowfill_check_opts(c, "chunks", o);
    if (rc != TK_OK) return rc;
    const uint32_t cap = o->max_length - o->keep_head - o->keep_tail;
    if (o->min_length == 0 || o->min_length > cap) {
        c->err = "min_length " + std::to_string(o->min_length) + " is not in 1 .. " + std::to_string(cap) + ", the body ids of a chunk";
        return TK_ERR_INVALID_ARG;
    }
    if (o->overlap >= o->min_length) {
        c->err = "overlap " + std::to_string(o->overlap) + " is not below min_length " + std::to_string(o->min_length);
        return TK_ERR_INVALID_ARG;
    }
    return chunk_check_levels(c, o->levels);
}
static constexpr auto chunk_encode_opts = rowfill_encode_opts<tk_chunk_opts, chunk_check_opts>;

static hipError_t chunk_events(tk_ctx* c) {
    for (Event& ev : c->chunk.ev) {
        const hipError_t e = ev.h ? hipSuccess : hipEventCreate(&ev.h);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The level bytes of ids on the device into c->chunk.lev, on s (one wait).  The caller holds c->mu; the mask is known.
static int run_levels(tk_ctx* c, const uint32_t* d_spans, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t n_ids, const uint8_t* d_bytes,
                      const uint64_t* d_doc_offs, uint32_t levels, hipStream_t s) {
    ChunkBufs& b = c->chunk;
    b.ms[0] = 0.f;
    int rc = check_n_docs(c, n_docs);
    if (rc != TK_OK) return rc;
    if (n_docs == 0 && n_ids) { c->err = "chunks: ids without a document"; return TK_ERR_INVALID_ARG; }
    TK_HIP(c, b.lev.reserve(n_ids + 16));
    TK_HIP(c, chunk_events(c));
    if (n_docs == 0 || n_ids == 0) return TK_OK;
    TkChunkArgs a;
    memset(&a, 0, sizeof(a));
    a.in_spans = d_spans;
    a.id_offs = d_id_offs;
    a.n_docs = n_docs;
    a.bytes = d_bytes;
    a.doc_offs = d_doc_offs;
    a.lev_out = (uint8_t*)b.lev.p;
    // what every level becomes under the mask: the highest enabled level at or below it, or TOKEN
    uint32_t to = TK_CHUNK_LEVEL_TOKEN;
    a.demote = TK_CHUNK_LEVEL_TOKEN << 4;
    for (uint32_t l = TK_CHUNK_LEVEL_WORD; l <= TK_CHUNK_LEVEL_PARAGRAPH; ++l) {
        if (levels & (1u << l)) to = l;
        a.demote |= to << (4u * l);
    }
    TK_HIP(c, hipEventRecord(b.ev[0], s));
    TK_HIP(c, tk_launch_chunk_levels(a, s));
    TK_HIP(c, hipEventRecord(b.ev[1], s));
    TK_HIP(c, hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&b.ms[0], b.ev[0], b.ev[1]);
    return TK_OK;
}

// The chunk pass over ids and level bytes on the device into the context's c->chunk buffers; *out gets the device pointers.  The
// tensors are sized by the three steps of tk_capi_layout.h, the first walk being the counts kernel (ONE read: W, the longest document,
// n_split, the level counts), and only once the sizes are accepted is anything of an earlier result touched (rowfill_outputs).  One
// wait ends the call.  The caller holds c->mu.
static int run_chunk(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t n_ids, const uint8_t* d_lev,
                     const uint32_t* d_spans, const tk_chunk_opts* o, hipStream_t s, tk_chunk* out) {
    ChunkBufs& b = c->chunk;
    b.ms[1] = b.ms[2] = 0.f;
    int rc = chunk_check_opts(c, o);
    if (rc != TK_OK) return rc;
    if ((rc = check_n_docs(c, n_docs)) != TK_OK) return rc;
    if (n_docs == 0 && n_ids) { c->err = "chunks: ids without a document"; return TK_ERR_INVALID_ARG; }
    const bool fixed = (o->flags & TK_CHUNK_FIXED) != 0, i64 = (o->flags & TK_CHUNK_I64) != 0, mask = (o->flags & TK_CHUNK_MASK) != 0,
               spans = (o->flags & TK_CHUNK_SPANS) != 0, bytes = (o->flags & TK_CHUNK_BYTES) != 0;
    if ((spans || bytes) && !d_spans) { c->err = "TK_CHUNK_SPANS and TK_CHUNK_BYTES need a spans buffer"; return TK_ERR_INVALID_ARG; }
    if (n_ids && !d_lev) { c->err = "chunks: ids without a level buffer"; return TK_ERR_INVALID_ARG; }
    if ((rc = layout_check_fixed_len(c, "chunks", fixed, o->max_length, o->multiple_of)) != TK_OK) return rc;
    TkChunkArgs a;
    memset(&a, 0, sizeof(a));
    rowfill_inputs(a, d_ids, d_id_offs, d_spans, n_docs, o);
    a.lev = d_lev;
    a.min_len = o->min_length;
    a.overlap = o->overlap;
    unsigned long long stat[8];                     // the longest document | the split ones | the cuts at levels 0 .. 5
    uint64_t W, L;
    rc = layout_count_rows(c, n_docs, b.stat, b.cnt, b.dw_next, b.bsum, stat, 8, s, [&](uint32_t* counts, unsigned long long* d_stat) {
        a.counts = counts;
        a.stat = d_stat;
        hipError_t e = chunk_events(c);             // (behind the work buffers, as every resource of the call)
        if (e == hipSuccess) e = hipEventRecord(b.ev[2], s);
        return e != hipSuccess ? e : tk_launch_chunk_walk(a, 0, s);
    }, &W, &b.ev[3].h);
    if (rc != TK_OK) return rc;
    if (stat[0] >= 0xFFFFFFFFull) { c->err = "chunks: a document reaches 2^32 - 1 ids (window_start is uint32)"; return TK_ERR_INVALID_ARG; }
    rc = layout_row_len(c, "chunks", fixed, stat[0] < o->max_length ? stat[0] : o->max_length, o->max_length, o->multiple_of, W, &L);
    if (rc != TK_OK) return rc;
    TK_HIP(c, b.cut.reserve(W + 16));
    if (bytes) TK_HIP(c, b.cbytes.reserve(W * 8 + 16));
    TK_HIP(c, b.lcounts.reserve(64));
    TK_HIP(c, b.rec.reserve(W * sizeof(TkChunkRec) + 16));
    if ((rc = rowfill_outputs(c, b, a, W, L, i64, mask, spans)) != TK_OK) return rc;
    a.rec = (TkChunkRec*)b.rec.p;
    a.cut_level = (uint8_t*)b.cut.p;
    a.chunk_bytes = bytes ? (uint32_t*)b.cbytes.p : nullptr;
    if (n_docs == 0) {
        TK_HIP(c, hipMemsetAsync(b.lcounts.p, 0, 48, s));
    } else {
        TK_HIP(c, hipMemcpyAsync(b.lcounts.p, a.stat + 2, 48, hipMemcpyDeviceToDevice, s));
        TK_HIP(c, hipEventRecord(b.ev[4], s));
        TK_HIP(c, tk_launch_chunk_walk(a, 1, s));
        TK_HIP(c, hipEventRecord(b.ev[5], s));
        TK_HIP(c, tk_launch_chunk(a, i64, s));
        TK_HIP(c, hipEventRecord(b.ev[6], s));
    }
    TK_HIP(c, hipStreamSynchronize(s));
    if (n_docs) {
        float first = 0.f, second = 0.f;
        (void)hipEventElapsedTime(&first, b.ev[2], b.ev[3]);
        (void)hipEventElapsedTime(&second, b.ev[4], b.ev[5]);
        (void)hipEventElapsedTime(&b.ms[2], b.ev[5], b.ev[6]);
        b.ms[1] = first + second;
    }
    rowfill_result(a, stat[1], out);
    out->cut_level = a.cut_level;
    out->chunk_bytes = a.chunk_bytes;
    out->level_counts = (uint64_t*)b.lcounts.p;
    return TK_OK;
}

// the spans (into the pass's own buffer), the levels and the chunks of ids that were encoded from text on the device
static int run_chunk_encoded(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t n_ids, const uint8_t* d_bytes,
                             const uint64_t* d_doc_offs, const tk_chunk_opts* o, hipStream_t s, tk_chunk* out) {
    int rc = run_spans(c, d_ids, d_id_offs, n_docs, n_ids, nullptr, nullptr, 0, s, nullptr, &c->chunk.in_spans);
    if (rc != TK_OK) return rc;
    const uint32_t* sp = (const uint32_t*)c->chunk.in_spans.p;
    if ((rc = run_levels(c, sp, d_id_offs, n_docs, n_ids, d_bytes, d_doc_offs, o->levels, s)) != TK_OK) return rc;
    return run_chunk(c, d_ids, d_id_offs, n_docs, n_ids, (const uint8_t*)c->chunk.lev.p, sp, o, s, out);
}

namespace {
struct ChunkPass : LayoutPass<ChunkPass> {
    typedef tk_chunk_opts Opts;
    typedef tk_chunk Result;
    static constexpr const char* name = "chunk";
    static uint64_t esz(const Opts& o) { return (o.flags & TK_CHUNK_I64) ? 8 : 4; }
    static constexpr auto run = run_chunk;
};
}  // namespace

extern "C" int tk_chunk_levels_device(tk_ctx* c, const void* d_spans, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                                      const void* d_bytes, const void* d_doc_offsets, uint64_t n_bytes, uint32_t levels, void* hip_stream,
                                      void** d_levels) {
    TK_ENTRY(c);
    int rc = chunk_check_levels(c, levels);
    if (rc != TK_OK) return rc;
    if (!d_id_offsets || (!d_spans && n_ids) || !d_doc_offsets || (!d_bytes && n_bytes) || !d_levels) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    TK_HIP(c, hipSetDevice(c->device));
    rc = run_levels(c, (const uint32_t*)d_spans, (const uint64_t*)d_id_offsets, n_docs, n_ids, (const uint8_t*)d_bytes,
                    (const uint64_t*)d_doc_offsets, levels, (hipStream_t)hip_stream);
    if (rc != TK_OK) return rc;
    *d_levels = c->chunk.lev.p;
    return TK_OK;
}
extern "C" int tk_chunk_from_ids_device(tk_ctx* c, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                                        const void* d_levels, const void* d_spans, const tk_chunk_opts* opts, void* hip_stream, tk_chunk* out) {
    return layout_from_ids_device<ChunkPass>(c, d_ids, d_id_offsets, n_docs, n_ids, opts, hip_stream, out, (const uint8_t*)d_levels,
                                             (const uint32_t*)d_spans);
}
extern "C" int tk_encode_batch_device_chunk(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                            int add_bos, int add_eos, int checks, const tk_chunk_opts* opts, void* hip_stream, void** d_ids,
                                            void** d_out_offsets, uint64_t* n_ids, tk_chunk* out) {
    TK_ENTRY(c);
    int rc = check_flags_and_args(c, checks, TK_CHECK_OFFSETS | TK_CHECK_UTF8, !opts || !out);
    if (rc != TK_OK) return rc;
    tk_chunk_opts o;
    if ((rc = chunk_encode_opts(c, opts, add_bos, add_eos, &o)) != TK_OK) return rc;
    rc = encode_device_checked(c, d_bytes, d_doc_offsets, n_docs, n_bytes, add_bos, add_eos, checks, hip_stream, d_ids, d_out_offsets, n_ids);
    if (rc != TK_OK) return rc;
    return run_chunk_encoded(c, (const uint32_t*)*d_ids, (const uint64_t*)*d_out_offsets, n_docs, *n_ids, (const uint8_t*)d_bytes,
                             (const uint64_t*)d_doc_offsets, &o, (hipStream_t)hip_stream, out);
}
// host in / host out.  *out is zeroed once the arguments are there, and filled only by a call that went through
extern "C" int tk_encode_batch_chunk(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos, int add_eos,
                                     int validate_utf8, const tk_chunk_opts* opts, tk_chunk* out) {
    TK_ENTRY(c);
    if (!opts || !out) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    memset(out, 0, sizeof(*out));
    tk_chunk_opts o;
    int rc = chunk_encode_opts(c, opts, add_bos, add_eos, &o);
    if (rc != TK_OK) return rc;
    DevBatch dev;
    uint64_t n_ids;
    if ((rc = encode_batch_for_layout(c, bytes, doc_offsets, n_docs, add_bos, add_eos, validate_utf8, &dev, &n_ids)) != TK_OK) return rc;
    // (the small path's text, ids and offsets are mapped pinned memory: the kernels of the pass read them there)
    tk_chunk r;
    if ((rc = run_chunk_encoded(c, dev.ids, dev.id_offs, n_docs, n_ids, dev.bytes, dev.doc_offs, &o, c->stream, &r)) != TK_OK) return rc;
    return layout_copy_out(c, r, ChunkPass::esz(o), n_docs, ChunkPass::name, out);
}
extern "C" void tk_free_chunk(tk_chunk* r) { layout_free(r); }

extern "C" void tk_last_chunk_ms(const tk_ctx* c, float ms[3]) {
    std::unique_lock<std::mutex> lock;
    if (c) lock = std::unique_lock<std::mutex>(const_cast<tk_ctx*>(c)->mu);   // (a call on another thread writes them under it)
    for (int i = 0; ms && i < 3; ++i) ms[i] = c ? c->chunk.ms[i] : 0.f;
}
