// tk_capi_dense.cpp -- model-ready dense batches (include/tekken_hip.h tk_dense_from_ids_device and the entries around it;
// csrc/tk_dense.hip): truncation, padding, mask and lengths, and back to the ragged form.
#include "tk_capi_layout.h"

#define TK_DENSE_ALL_FLAGS (TK_DENSE_PAD_LEFT | TK_DENSE_TRUNC_LEFT | TK_DENSE_FIXED | TK_DENSE_I64 | TK_DENSE_MASK)

// the options that can be refused before anything is enqueued (step 5 of the definition)
static int dense_check_opts(tk_ctx* c, const tk_dense_opts* o) {
    if (!o) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    if (o->flags & ~(uint32_t)TK_DENSE_ALL_FLAGS) { c->err = "unknown dense flag"; return TK_ERR_INVALID_ARG; }
    if ((o->flags & TK_DENSE_FIXED) && o->max_length == 0) { c->err = "TK_DENSE_FIXED needs a max_length"; return TK_ERR_INVALID_ARG; }
    if (o->max_length) {
        const bool left = (o->flags & TK_DENSE_TRUNC_LEFT) != 0;
        if (left ? o->keep_head > o->max_length : o->keep_tail > o->max_length) {
            c->err = std::string(left ? "keep_head" : "keep_tail") + " exceeds max_length " + std::to_string(o->max_length);
            return TK_ERR_INVALID_ARG;
        }
    }
    return TK_OK;
}
// the options of an entry that encodes first: BOS / EOS are what truncation keeps
static int dense_encode_opts(tk_ctx* c, const tk_dense_opts* opts, int add_bos, int add_eos, tk_dense_opts* o) {
    *o = *opts;
    o->keep_head = add_bos ? 1u : 0u;
    o->keep_tail = add_eos ? 1u : 0u;
    int rc = dense_check_opts(c, o);
    if (rc != TK_OK) return rc;
    if (o->max_length && o->keep_head + o->keep_tail > o->max_length) {
        c->err = "BOS / EOS do not fit into max_length " + std::to_string(o->max_length);
        return TK_ERR_INVALID_ARG;
    }
    return TK_OK;
}

// The dense pass over ids on the device into the context's c->dense buffers; *out gets the device pointers.  Longest-row mode: one
// reduction over the id offsets and one 8-byte read size the tensor; FIXED: no read before the launch.  One wait at the end
// (the truncated count).  Nothing of an earlier result is touched before every argument has been accepted.  The caller holds c->mu.
static int run_dense(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_docs, const tk_dense_opts* o,
                     hipStream_t s, tk_dense* out) {
    int rc = dense_check_opts(c, o);
    if (rc != TK_OK) return rc;
    if ((rc = check_n_docs(c, n_docs)) != TK_OK) return rc;
    const bool fixed = (o->flags & TK_DENSE_FIXED) != 0, i64 = (o->flags & TK_DENSE_I64) != 0, mask = (o->flags & TK_DENSE_MASK) != 0;
    TK_HIP(c, c->dense.stat.reserve(64));
    unsigned long long* d_stat = (unsigned long long*)c->dense.stat.p;
    TK_HIP(c, hipMemsetAsync(d_stat, 0, 16, s));
    uint64_t L = o->max_length;
    if (!fixed) {
        unsigned long long longest = 0;
        TK_HIP(c, tk_launch_dense_maxlen(d_id_offs, n_docs, d_stat, s));
        TK_HIP(c, hipMemcpyAsync(&longest, d_stat, 8, hipMemcpyDeviceToHost, s));
        TK_HIP(c, hipStreamSynchronize(s));
        L = o->max_length && longest > o->max_length ? o->max_length : longest;
    }
    L = round_up(L, o->multiple_of);
    if (L > TK_LAYOUT_MAX_ROW || (n_docs && L > TK_LAYOUT_MAX_ELEMS / n_docs)) return layout_too_large(c, "dense", n_docs, L);
    const uint64_t elems = n_docs * L;
    TK_HIP(c, c->dense.ids.reserve(elems * (i64 ? 8 : 4) + 16));
    if (mask) TK_HIP(c, c->dense.mask.reserve(elems + 16));
    TK_HIP(c, c->dense.len.reserve(n_docs * 4 + 16));
    TkDenseArgs a;
    memset(&a, 0, sizeof(a));
    a.ids = d_ids;
    a.id_offs = d_id_offs;
    a.n_docs = n_docs;
    a.row_len = (uint32_t)L;
    a.lim = o->max_length ? o->max_length : 0xFFFFFFFFu;
    a.keep_head = o->keep_head;
    a.keep_tail = o->keep_tail;
    a.pad_id = o->pad_id;
    a.trunc_left = (o->flags & TK_DENSE_TRUNC_LEFT) != 0;
    a.pad_left = (o->flags & TK_DENSE_PAD_LEFT) != 0;
    a.out = c->dense.ids.p;
    a.mask = mask ? (uint8_t*)c->dense.mask.p : nullptr;
    a.lengths = (uint32_t*)c->dense.len.p;
    a.stat = d_stat;
    unsigned long long n_trunc = 0;
    if (L == 0 && n_docs) TK_HIP(c, hipMemsetAsync(c->dense.len.p, 0, n_docs * 4, s));   // (no document has an id: nothing to launch)
    TK_HIP(c, tk_launch_dense(a, i64, s));
    TK_HIP(c, hipMemcpyAsync(&n_trunc, d_stat + 1, 8, hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipStreamSynchronize(s));
    out->ids = c->dense.ids.p;
    out->mask = mask ? (uint8_t*)c->dense.mask.p : nullptr;
    out->lengths = (uint32_t*)c->dense.len.p;
    out->n_docs = n_docs;
    out->row_len = L;
    out->n_truncated = n_trunc;
    return TK_OK;
}

namespace {
struct DensePass : LayoutPass<DensePass> {
    typedef tk_dense_opts Opts;
    typedef tk_dense Result;
    static constexpr const char* name = "dense";
    static uint64_t esz(const Opts& o) { return (o.flags & TK_DENSE_I64) ? 8 : 4; }
    static constexpr auto encode_opts = dense_encode_opts;
    static int run(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t, const Opts* o, hipStream_t s, Result* out) {
        return run_dense(c, d_ids, d_id_offs, n_docs, o, s, out);   // (the offsets say how many ids there are)
    }
};
}  // namespace

extern "C" int tk_dense_from_ids_device(tk_ctx* c, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                                        const tk_dense_opts* opts, void* hip_stream, tk_dense* out) {
    return layout_from_ids_device<DensePass>(c, d_ids, d_id_offsets, n_docs, n_ids, opts, hip_stream, out);
}
extern "C" int tk_encode_batch_device_dense(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs,
                                            uint64_t n_bytes, int add_bos, int add_eos, int checks, const tk_dense_opts* opts,
                                            void* hip_stream, void** d_ids, void** d_out_offsets, uint64_t* n_ids, tk_dense* out) {
    return layout_encode_device<DensePass>(c, d_bytes, d_doc_offsets, n_docs, n_bytes, add_bos, add_eos, checks, opts, hip_stream, d_ids,
                                           d_out_offsets, n_ids, out);
}
extern "C" int tk_encode_batch_dense(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos,
                                     int add_eos, int validate_utf8, const tk_dense_opts* opts, tk_dense* out) {
    return layout_encode_host<DensePass>(c, bytes, doc_offsets, n_docs, add_bos, add_eos, validate_utf8, opts, out);
}
extern "C" void tk_free_dense(tk_dense* r) { layout_free(r); }

extern "C" int tk_ragged_from_dense_device(tk_ctx* c, const void* d_dense, uint64_t n_docs, uint64_t row_len, int flags,
                                           const void* d_lengths, uint32_t pad_id, void* hip_stream, void** d_ids,
                                           void** d_id_offsets, uint64_t* n_ids) {
    TK_ENTRY(c);
    if (flags & ~(TK_DENSE_I64 | TK_DENSE_PAD_LEFT)) { c->err = "unknown dense flag"; return TK_ERR_INVALID_ARG; }
    if ((!d_dense && n_docs && row_len) || !d_ids || !d_id_offsets || !n_ids) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    if (n_docs >= 0xFFFFFFF0ull || row_len > TK_LAYOUT_MAX_ROW || (n_docs && row_len > TK_LAYOUT_MAX_ELEMS / n_docs)) return layout_too_large(c, "dense", n_docs, row_len);
    TK_HIP(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;
    const int i64 = (flags & TK_DENSE_I64) != 0;
    // (the ids are sized by the tensor, an upper bound of what the rows hold: no host read between the scan and the copy)
    TK_HIP(c, c->dense.rids.reserve(n_docs * row_len * 4 + 16));
    TK_HIP(c, c->dense.roffs.reserve((n_docs + 1) * 8));
    TK_HIP(c, c->dense.rlens.reserve(n_docs * 4 + 16));
    TK_HIP(c, c->block_sums.reserve(scan_workspace_bytes(n_docs)));
    TkRaggedArgs a;
    memset(&a, 0, sizeof(a));
    a.dense = d_dense;
    a.n_docs = n_docs;
    a.row_len = (uint32_t)row_len;
    a.pad_id = pad_id;
    a.pad_left = (flags & TK_DENSE_PAD_LEFT) != 0;
    a.given = (const uint32_t*)d_lengths;
    a.lens = (uint32_t*)c->dense.rlens.p;
    a.offs = (const uint64_t*)c->dense.roffs.p;
    a.out_ids = (uint32_t*)c->dense.rids.p;
    uint64_t total = 0;
    if (n_docs == 0) {
        TK_HIP(c, hipMemsetAsync(c->dense.roffs.p, 0, 8, s));
    } else {
        if (row_len == 0) TK_HIP(c, hipMemsetAsync(c->dense.rlens.p, 0, n_docs * 4, s));
        else TK_HIP(c, tk_launch_ragged_rowlen(a, i64, s));
        int rc = scan_u32(c, c->block_sums, a.lens, n_docs, (uint64_t*)c->dense.roffs.p, s);
        if (rc != TK_OK) return rc;
        TK_HIP(c, tk_launch_ragged_copy(a, i64, s));
        TK_HIP(c, hipMemcpyAsync(&total, (const uint64_t*)c->dense.roffs.p + n_docs, 8, hipMemcpyDeviceToHost, s));
    }
    TK_HIP(c, hipStreamSynchronize(s));
    *d_ids = c->dense.rids.p;
    *d_id_offsets = c->dense.roffs.p;
    *n_ids = total;
    return TK_OK;
}
