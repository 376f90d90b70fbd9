// tk_capi_spans_units.cpp -- per-token spans in code points / UTF-16 units and the annotation -> token range look-up
// (include/tekken_hip.h tk_token_spans_units_device, tk_spans_locate_device and the entries around them; csrc/tk_spans_units.hip).
#include "tk_ctx.h"
#include "tk_units_table.h"

// the per-rank entries of the units kernel, built at the first units call on the context
static int units_table(tk_ctx* c) {
    if (c->units.table.p) return TK_OK;
    const TkHostTables& h = c->host;
    std::vector<uint16_t> tab((size_t)h.n_ranks + 8, 0);
    tk_units_table_build(h.blob.data(), h.offs.data(), h.n_ranks, tab.data());
    const int rc = upload(c, c->units.table, tab.data(), tab.size() * 2);
    if (rc != TK_OK) c->units.table.release();             // (the pointer is the "built" flag: a failed copy must not leave it set)
    return rc;
}

static int check_unit(tk_ctx* c, int unit) {
    if (unit == TK_UNIT_BYTE || unit == TK_UNIT_CHAR || unit == TK_UNIT_UTF16) return TK_OK;
    c->err = "unknown unit " + std::to_string(unit);
    return TK_ERR_INVALID_ARG;
}

// The units pass over ids on the device: (start, end) of every id in `unit` into c->units.spans, one host wait for the error words.
// TK_UNIT_BYTE is the byte kernel into the same buffer.  The caller holds c->mu.
static int run_spans_units(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t n_ids, int unit,
                           hipStream_t s) {
    if (unit == TK_UNIT_BYTE) return run_spans(c, d_ids, d_id_offs, n_docs, n_ids, nullptr, nullptr, 0, s, nullptr, &c->units.spans);
    int rc = units_table(c);
    if (rc != TK_OK) return rc;
    TK_HIP(c, c->units.spans.reserve(n_ids * 8 + 16));
    TK_HIP(c, c->units.err.reserve(64));
    TkSpansUnitsArgs a;
    memset(&a, 0, sizeof(a));
    a.ids = d_ids;
    a.id_offs = d_id_offs;
    a.n_docs = n_docs;
    a.spans = (uint32_t*)c->units.spans.p;
    a.err = (unsigned long long*)c->units.err.p;
    a.tok_blob = (const uint8_t*)c->t_blob.p;
    a.tok_offs = (const uint32_t*)c->t_offs.p;
    a.tok_units = (const uint16_t*)c->units.table.p;
    a.n_ranks = c->host.n_ranks;
    a.num_special = c->host.num_special;
    unsigned long long err[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    TK_HIP(c, hipMemsetAsync(c->units.err.p, 0xFF, 32, s));
    TK_HIP(c, tk_launch_spans_units(a, unit, s));
    TK_HIP(c, hipMemcpyAsync(err, c->units.err.p, 32, hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipStreamSynchronize(s));
    for (int k = 2; k < 4; ++k) {
        if (err[k] == ~0ull) continue;
        uint64_t d = 0;
        if ((rc = doc_of_id(c, d_id_offs, n_docs, err[k], &d)) != TK_OK) return rc;
        if (k == 2) {
            uint32_t id = 0;
            TK_HIP(c, hipMemcpy(&id, d_ids + err[2], 4, hipMemcpyDefault));
            c->err = "spans: id " + std::to_string(id) + " (document " + std::to_string(d) + ") is outside the vocabulary";
            return TK_ERR_RUNTIME;
        }
        c->err = "spans: document " + std::to_string(d) + " reaches 2^32 units (spans are uint32 offsets)";
        return TK_ERR_INVALID_ARG;
    }
    return TK_OK;
}

extern "C" int tk_token_spans_units_device(tk_ctx* c, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                                           int unit, void* hip_stream, void** d_spans) {
    TK_ENTRY(c);
    int rc = check_unit(c, unit);
    if (rc != TK_OK) return rc;
    if (!d_id_offsets || (!d_ids && n_ids) || !d_spans) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    TK_HIP(c, hipSetDevice(c->device));
    rc = run_spans_units(c, (const uint32_t*)d_ids, (const uint64_t*)d_id_offsets, n_docs, n_ids, unit, (hipStream_t)hip_stream);
    if (rc != TK_OK) return rc;
    *d_spans = c->units.spans.p;
    return TK_OK;
}

extern "C" int tk_encode_batch_device_spans_units(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs,
                                                  uint64_t n_bytes, int add_bos, int add_eos, int checks, int unit, void* hip_stream,
                                                  void** d_ids, void** d_out_offsets, void** d_spans, uint64_t* n_ids) {
    TK_ENTRY(c);
    // (a TK_SPANS_CHECK_* bit is an unknown flag here: those checks belong to the byte pass)
    int rc = check_flags_and_args(c, checks, TK_CHECK_OFFSETS | TK_CHECK_UTF8, !d_spans);
    if (rc != TK_OK || (rc = check_unit(c, unit)) != TK_OK) return rc;
    rc = encode_device_checked(c, d_bytes, d_doc_offsets, n_docs, n_bytes, add_bos, add_eos, checks, hip_stream, d_ids, d_out_offsets, n_ids);
    if (rc != TK_OK) return rc;
    rc = run_spans_units(c, (const uint32_t*)*d_ids, (const uint64_t*)*d_out_offsets, n_docs, *n_ids, unit, (hipStream_t)hip_stream);
    if (rc != TK_OK) return rc;
    *d_spans = c->units.spans.p;
    return TK_OK;
}

extern "C" int tk_encode_batch_spans_units(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos,
                                           int add_eos, int validate_utf8, int unit, tk_result* out, uint32_t** spans) {
    TK_ENTRY(c);
    int rc = check_unit(c, unit);
    if (rc != TK_OK) return rc;
    if (!spans) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    *spans = nullptr;
    DevBatch dev;
    if ((rc = encode_batch(c, bytes, doc_offsets, n_docs, add_bos, add_eos, validate_utf8, out, &dev)) != TK_OK) return rc;
    // (the small path's ids and offsets are mapped pinned memory: the units kernel reads them there)
    rc = run_spans_units(c, dev.ids, dev.id_offs, n_docs, out->n_ids, unit, c->stream);
    CopyOut h = {c->units.spans.p, out->n_ids * 8, nullptr};
    if (rc != TK_OK || (rc = copy_out(c, &h, 1, "spans")) != TK_OK) {
        tk_free_result(out);
        return rc;
    }
    *spans = (uint32_t*)h.host;
    return TK_OK;
}

extern "C" int tk_spans_locate_device(tk_ctx* c, const void* d_spans, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                                      const void* d_ann_doc, const void* d_ann, uint64_t n_ann, void* hip_stream, void** d_tok_range,
                                      uint64_t* bad_ann) {
    TK_ENTRY(c);
    if (!d_id_offsets || (!d_spans && n_ids) || ((!d_ann_doc || !d_ann) && n_ann) || !d_tok_range) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    if (n_ann >= (1ull << 32)) { c->err = "locate: " + std::to_string(n_ann) + " annotations are beyond 2^32 - 1"; return TK_ERR_INVALID_ARG; }
    TK_HIP(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;
    // the ranges go to the work buffer; it becomes the result (a swap of the two) only once every annotation is accepted
    TK_HIP(c, c->units.next.reserve(n_ann * 8 + 16));
    TK_HIP(c, c->units.range_err.reserve(64));
    TkLocateArgs a;
    memset(&a, 0, sizeof(a));
    a.spans = (const uint32_t*)d_spans;
    a.id_offs = (const uint64_t*)d_id_offsets;
    a.n_docs = n_docs;
    a.n_ids = n_ids;
    a.ann_doc = (const uint32_t*)d_ann_doc;
    a.ann = (const uint32_t*)d_ann;
    a.n_ann = n_ann;
    a.out = (uint32_t*)c->units.next.p;
    a.err = (unsigned long long*)c->units.range_err.p;
    unsigned long long err = ~0ull;
    TK_HIP(c, hipMemsetAsync(c->units.range_err.p, 0xFF, 8, s));
    TK_HIP(c, tk_launch_spans_locate(a, s));
    TK_HIP(c, hipMemcpyAsync(&err, c->units.range_err.p, 8, hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipStreamSynchronize(s));
    if (err != ~0ull) {
        if (bad_ann) *bad_ann = err;
        c->err = "locate: annotation " + std::to_string(err) + " names a document beyond n_docs or starts behind its end";
        return TK_ERR_INVALID_ARG;
    }
    std::swap(c->units.range, c->units.next);
    *d_tok_range = c->units.range.p;
    return TK_OK;
}
