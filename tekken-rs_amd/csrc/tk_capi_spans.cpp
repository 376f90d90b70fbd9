// tk_capi_spans.cpp -- per-token byte spans (include/tekken_hip.h tk_token_spans_device and the entries around it;
// csrc/tk_spans.hip): where in its document every id's bytes lie, with the per-document checks.
#include "tk_ctx.h"

// the first document whose id range holds id index idx: binary search on the device offsets (error path only; the offsets may be
// mapped pinned memory -- the small path's)
int doc_of_id(tk_ctx* c, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t idx, uint64_t* out) {
    uint64_t lo = 0, hi = n_docs;
    while (lo < hi) {
        uint64_t mid = (lo + hi) / 2, v = 0;
        TK_HIP(c, hipMemcpy(&v, d_id_offs + mid + 1, 8, hipMemcpyDefault));
        if (v <= idx) lo = mid + 1; else hi = mid;
    }
    *out = lo;
    return TK_OK;
}

// The spans pass over ids on the device: (start, end) of every id into c->spans.spans, the checks of `checks` (TK_SPANS_CHECK_*
// only) in the same pass, one host wait for the error words.  The caller holds c->mu.  (Also the window entries' spans pass, and
// -- into its own buffer -- the units pass in bytes.)
int run_spans(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t n_ids,
              const uint64_t* d_doc_offs, const uint8_t* d_bytes, int checks, hipStream_t s, uint64_t* bad_doc, DevBuf* into) {
    DevBuf& spans = into ? *into : c->spans.spans;
    if (checks & TK_SPANS_CHECK_BYTES) checks |= TK_SPANS_CHECK_COVER;
    if (((checks & TK_SPANS_CHECK_COVER) && !d_doc_offs) || ((checks & TK_SPANS_CHECK_BYTES) && !d_bytes)) {
        c->err = "the spans checks need the document offsets (COVER) and the text (BYTES)";
        return TK_ERR_INVALID_ARG;
    }
    int rc = token_tables(c);
    if (rc != TK_OK) return rc;
    TK_HIP(c, spans.reserve(n_ids * 8 + 16));
    TK_HIP(c, c->spans.err.reserve(64));
    TkSpansArgs a;
    memset(&a, 0, sizeof(a));
    a.ids = d_ids;
    a.id_offs = d_id_offs;
    a.n_docs = n_docs;
    a.doc_offs = d_doc_offs;
    a.bytes = d_bytes;
    a.spans = (uint32_t*)spans.p;
    a.err = (unsigned long long*)c->spans.err.p;
    token_args(c, a);
    unsigned long long err[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    TK_HIP(c, hipMemsetAsync(c->spans.err.p, 0xFF, 32, s));
    TK_HIP(c, tk_launch_spans(a, checks, s));
    TK_HIP(c, hipMemcpyAsync(err, c->spans.err.p, 32, hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipStreamSynchronize(s));
    if (err[0] == ~0ull && err[1] == ~0ull && err[2] == ~0ull && err[3] == ~0ull) return TK_OK;
    // error path: name the first document that fails and say why
    const TkHostTables& h = c->host;
    uint64_t first = err[0];
    for (int k = 1; k < 4; ++k) {
        if (err[k] == ~0ull) continue;
        uint64_t d = 0;
        if ((rc = doc_of_id(c, d_id_offs, n_docs, err[k], &d)) != TK_OK) return rc;
        if (k >= 2 || d < first) first = d;
        if (k == 2) {
            uint32_t id = 0;
            TK_HIP(c, hipMemcpy(&id, d_ids + err[2], 4, hipMemcpyDefault));
            if (bad_doc) *bad_doc = d;
            c->err = "spans: id " + std::to_string(id) + " (document " + std::to_string(d) + ") is outside the vocabulary";
            return TK_ERR_RUNTIME;
        }
        if (k == 3) {
            if (bad_doc) *bad_doc = d;
            c->err = "spans: document " + std::to_string(d) + " reaches 2^32 bytes (spans are uint32 offsets)";
            return TK_ERR_INVALID_ARG;
        }
    }
    if (bad_doc) *bad_doc = first;
    // the two lengths: what the ids of the document cover, and the document itself
    uint64_t range[2] = {0, 0}, text[2] = {0, 0};
    TK_HIP(c, hipMemcpy(range, d_id_offs + first, 16, hipMemcpyDefault));
    TK_HIP(c, hipMemcpy(text, d_doc_offs + first, 16, hipMemcpyDefault));
    std::vector<uint32_t> hid((size_t)(range[1] - range[0]));
    if (!hid.empty()) TK_HIP(c, hipMemcpy(hid.data(), d_ids + range[0], hid.size() * 4, hipMemcpyDefault));
    uint64_t covered = 0;
    for (uint32_t id : hid)
        if (id >= h.num_special) covered += h.offs[id - h.num_special + 1] - h.offs[id - h.num_special];
    const std::string lens = "the ids cover " + std::to_string(covered) + " bytes, the document has " + std::to_string(text[1] - text[0]);
    if (err[0] == first) c->err = "spans: document " + std::to_string(first) + " is not covered by its ids: " + lens;
    else c->err = "spans: in document " + std::to_string(first) + " the token bytes of id index " + std::to_string(err[1] - range[0]) +
                  " differ from the text under its span (" + lens + ")";
    return TK_ERR_RUNTIME;
}

extern "C" int tk_token_spans_device(tk_ctx* c, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                                     const void* d_doc_offsets, const void* d_bytes, int checks, void* hip_stream, void** d_spans,
                                     uint64_t* bad_doc) {
    TK_ENTRY(c);
    if (checks & ~(TK_SPANS_CHECK_COVER | TK_SPANS_CHECK_BYTES)) { c->err = "unknown check flag"; return TK_ERR_INVALID_ARG; }
    if (!d_id_offsets || (!d_ids && n_ids) || !d_spans) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    TK_HIP(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;  // NULL = HIP's null stream: ordered after the caller's own work on it
    int rc = run_spans(c, (const uint32_t*)d_ids, (const uint64_t*)d_id_offsets, n_docs, n_ids, (const uint64_t*)d_doc_offsets,
                       (const uint8_t*)d_bytes, checks, s, bad_doc);
    if (rc != TK_OK) return rc;
    *d_spans = c->spans.spans.p;
    return TK_OK;
}

extern "C" int tk_encode_batch_device_spans(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs,
                                            uint64_t n_bytes, int add_bos, int add_eos, int checks, void* hip_stream, void** d_ids,
                                            void** d_out_offsets, void** d_spans, uint64_t* n_ids, uint64_t* bad_doc) {
    TK_ENTRY(c);
    const int enc = TK_CHECK_OFFSETS | TK_CHECK_UTF8, sp = TK_SPANS_CHECK_COVER | TK_SPANS_CHECK_BYTES;
    if (checks & ~(enc | sp)) { c->err = "unknown check flag"; return TK_ERR_INVALID_ARG; }
    if (!d_spans) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    int rc = encode_device_checked(c, d_bytes, d_doc_offsets, n_docs, n_bytes, add_bos, add_eos, checks & enc, hip_stream, d_ids,
                                   d_out_offsets, n_ids);
    if (rc != TK_OK) return rc;
    rc = run_spans(c, (const uint32_t*)*d_ids, (const uint64_t*)*d_out_offsets, n_docs, *n_ids, (const uint64_t*)d_doc_offsets,
                   (const uint8_t*)d_bytes, checks & sp, (hipStream_t)hip_stream, bad_doc);
    if (rc != TK_OK) return rc;
    *d_spans = c->spans.spans.p;
    return TK_OK;
}

extern "C" int tk_encode_batch_spans(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos,
                                     int add_eos, int validate_utf8, int checks, tk_result* out, uint32_t** spans, uint64_t* bad_doc) {
    TK_ENTRY(c);
    if (checks & ~(TK_SPANS_CHECK_COVER | TK_SPANS_CHECK_BYTES)) { c->err = "unknown check flag"; return TK_ERR_INVALID_ARG; }
    if (!spans) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    *spans = nullptr;
    DevBatch dev;
    int rc = encode_batch(c, bytes, doc_offsets, n_docs, add_bos, add_eos, validate_utf8, out, &dev);
    if (rc != TK_OK) return rc;
    // (the small path's ids, offsets and text are mapped pinned memory: the spans kernel reads them there)
    rc = run_spans(c, dev.ids, dev.id_offs, n_docs, out->n_ids, dev.doc_offs, dev.bytes, checks, c->stream, bad_doc);
    CopyOut h = {c->spans.spans.p, out->n_ids * 8, nullptr};
    if (rc != TK_OK || (rc = copy_out(c, &h, 1, "spans")) != TK_OK) {
        tk_free_result(out);
        return rc;
    }
    *spans = (uint32_t*)h.host;
    return TK_OK;
}

extern "C" void tk_free_spans(uint32_t* spans) { tk_pinned_put(spans); }
