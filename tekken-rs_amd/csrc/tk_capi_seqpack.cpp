// tk_capi_seqpack.cpp -- packed fixed-length training rows (include/tekken_hip.h tk_seqpack_from_ids_device and the entries
// around it; csrc/tk_seqpack.hip): the stream of all ids cut into rows of seq_len, with position_ids, segment_ids and cu_seqlens.
#include "tk_ctx.h"

#define TK_SEQPACK_ALL_FLAGS (TK_SEQPACK_I64 | TK_SEQPACK_POSITIONS | TK_SEQPACK_SEGMENTS | TK_SEQPACK_CU_SEQLENS | TK_SEQPACK_DROP_LAST)

// the options that can be refused before the number of ids is known (step 8 of the definition)
static int seqpack_check_opts(tk_ctx* c, const tk_seqpack_opts* o) {
    if (!o) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    if (o->flags & ~(uint32_t)TK_SEQPACK_ALL_FLAGS) { c->err = "unknown seqpack flag"; return TK_ERR_INVALID_ARG; }
    if (o->seq_len == 0) { c->err = "seqpack needs a seq_len"; return TK_ERR_INVALID_ARG; }
    if (o->seq_len > TK_LAYOUT_MAX_ROW) { c->err = "seq_len " + std::to_string(o->seq_len) + " is beyond 2^31 - 1"; return TK_ERR_INVALID_ARG; }
    return TK_OK;
}

// The packed pass over ids on the device into the context's sp_* buffers; *out gets the device pointers.  n_rows, n_used and
// n_left follow from n_ids on the host, so nothing is read before the launches; ONE wait at the end (n_segments, max_seqlen).
// Nothing of an earlier result is touched before every argument has been accepted.  The caller holds c->mu.
static int run_seqpack(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t n_ids,
                       const tk_seqpack_opts* o, hipStream_t s, tk_seqpack* out) {
    int rc = seqpack_check_opts(c, o);
    if (rc != TK_OK) return rc;
    if ((rc = check_n_docs(c, n_docs)) != TK_OK) return rc;
    if (n_docs == 0 && n_ids) { c->err = "seqpack: ids without a document"; return TK_ERR_INVALID_ARG; }
    const uint64_t L = o->seq_len;
    const bool i64 = (o->flags & TK_SEQPACK_I64) != 0, want_pos = (o->flags & TK_SEQPACK_POSITIONS) != 0,
               want_seg = (o->flags & TK_SEQPACK_SEGMENTS) != 0, want_cu = (o->flags & TK_SEQPACK_CU_SEQLENS) != 0;
    const uint64_t n_rows = (o->flags & TK_SEQPACK_DROP_LAST) ? n_ids / L : n_ids / L + (n_ids % L != 0);
    const uint64_t n_used = n_ids < n_rows * L ? n_ids : n_rows * L;
    if (n_rows > TK_LAYOUT_MAX_ELEMS / L) {
        c->err = "seqpack: " + std::to_string(n_rows) + " rows of " + std::to_string(L) + " elements are beyond what one tensor can hold";
        return TK_ERR_INVALID_ARG;
    }
    if (want_cu && n_used >= (1ull << 31)) {
        c->err = "seqpack: cu_seqlens is int32 and " + std::to_string(n_used) + " ids do not fit";
        return TK_ERR_INVALID_ARG;
    }
    const uint64_t elems = n_rows * L, esz = i64 ? 8 : 4;
    TK_HIP(c, c->sp_stat.reserve(64));
    TK_HIP(c, c->sp_ids.reserve(elems * esz + 16));
    if (want_pos) TK_HIP(c, c->sp_pos.reserve(elems * esz + 16));
    if (want_seg) TK_HIP(c, c->sp_seg.reserve(elems * esz + 16));
    if (want_cu) TK_HIP(c, c->sp_cu.reserve((n_docs + n_rows + 2) * 4));
    unsigned long long stat[2] = {0, 0};
    if (n_used == 0) {                          // (no row: cu_seqlens = [0], nothing to launch)
        if (want_cu) TK_HIP(c, hipMemsetAsync(c->sp_cu.p, 0, 4, s));
    } else {
        TK_HIP(c, c->sp_flags.reserve(n_docs * 4 + 16));
        TK_HIP(c, c->sp_aflags.reserve(n_docs * 4 + 16));
        TK_HIP(c, c->sp_fpos.reserve((n_docs + 1) * 8));
        TK_HIP(c, c->sp_apos.reserve((n_docs + 1) * 8));
        TK_HIP(c, c->sp_starts.reserve((n_docs + 1) * 8));
        TK_HIP(c, c->sp_aligned.reserve((n_docs + 1) * 8));
        TK_HIP(c, c->sp_bsum.reserve(scan_workspace_bytes(n_docs)));
        TkSeqpackArgs a;
        memset(&a, 0, sizeof(a));
        a.ids = d_ids;
        a.id_offs = d_id_offs;
        a.n_docs = n_docs;
        a.row_len = o->seq_len;
        a.pad_id = o->pad_id;
        a.n_rows = n_rows;
        a.n_used = n_used;
        a.flags = (uint32_t*)c->sp_flags.p;
        a.aflags = (uint32_t*)c->sp_aflags.p;
        a.fpos = (const uint64_t*)c->sp_fpos.p;
        a.apos = (const uint64_t*)c->sp_apos.p;
        a.starts = (uint64_t*)c->sp_starts.p;
        a.n_aligned = (uint64_t*)c->sp_aligned.p;
        a.out_ids = c->sp_ids.p;
        a.out_pos = want_pos ? c->sp_pos.p : nullptr;
        a.out_seg = want_seg ? c->sp_seg.p : nullptr;
        a.cu = want_cu ? (int32_t*)c->sp_cu.p : nullptr;
        a.stat = (unsigned long long*)c->sp_stat.p;
        TK_HIP(c, hipMemsetAsync(a.stat, 0, 16, s));
        TK_HIP(c, tk_launch_seqpack_flags(a, s));
        if ((rc = scan_u32(c, c->sp_bsum, a.flags, n_docs, (uint64_t*)c->sp_fpos.p, s)) != TK_OK) return rc;
        if ((rc = scan_u32(c, c->sp_bsum, a.aflags, n_docs, (uint64_t*)c->sp_apos.p, s)) != TK_OK) return rc;
        TK_HIP(c, tk_launch_seqpack_starts(a, s));
        TK_HIP(c, tk_launch_seqpack(a, i64, s));
        TK_HIP(c, tk_launch_seqpack_cu(a, s));
        TK_HIP(c, hipMemcpyAsync(stat, a.stat, 16, hipMemcpyDeviceToHost, s));
    }
    TK_HIP(c, hipStreamSynchronize(s));
    out->input_ids = c->sp_ids.p;
    out->position_ids = want_pos ? c->sp_pos.p : nullptr;
    out->segment_ids = want_seg ? c->sp_seg.p : nullptr;
    out->cu_seqlens = want_cu ? (int32_t*)c->sp_cu.p : nullptr;
    out->n_rows = n_rows;
    out->row_len = L;
    out->n_used = n_used;
    out->n_left = n_ids - n_used;
    out->n_segments = stat[0];
    out->max_seqlen = stat[1];
    return TK_OK;
}

extern "C" int tk_seqpack_from_ids_device(tk_ctx* c, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                                          const tk_seqpack_opts* opts, void* hip_stream, tk_seqpack* out) {
    TK_ENTRY(c);
    if (!d_id_offsets || (!d_ids && n_ids) || !opts || !out) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    TK_HIP(c, hipSetDevice(c->device));
    return run_seqpack(c, (const uint32_t*)d_ids, (const uint64_t*)d_id_offsets, n_docs, n_ids, opts, (hipStream_t)hip_stream, out);
}

extern "C" int tk_encode_batch_device_seqpack(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs,
                                              uint64_t n_bytes, int add_bos, int add_eos, int checks, const tk_seqpack_opts* opts,
                                              void* hip_stream, void** d_ids, void** d_out_offsets, uint64_t* n_ids, tk_seqpack* out) {
    TK_ENTRY(c);
    int rc = check_flags_and_args(c, checks, TK_CHECK_OFFSETS | TK_CHECK_UTF8, !opts || !out);
    if (rc != TK_OK || (rc = seqpack_check_opts(c, opts)) != TK_OK) return rc;
    rc = encode_device_checked(c, d_bytes, d_doc_offsets, n_docs, n_bytes, add_bos, add_eos, checks, hip_stream, d_ids, d_out_offsets, n_ids);
    if (rc != TK_OK) return rc;
    return run_seqpack(c, (const uint32_t*)*d_ids, (const uint64_t*)*d_out_offsets, n_docs, *n_ids, opts, (hipStream_t)hip_stream, out);
}

extern "C" void tk_free_seqpack(tk_seqpack* r) {
    if (!r) return;
    tk_pinned_put(r->input_ids);
    tk_pinned_put(r->position_ids);
    tk_pinned_put(r->segment_ids);
    tk_pinned_put(r->cu_seqlens);
    memset(r, 0, sizeof(*r));
}

extern "C" int tk_encode_batch_seqpack(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos,
                                       int add_eos, int validate_utf8, const tk_seqpack_opts* opts, tk_seqpack* out) {
    TK_ENTRY(c);
    if (!opts || !out) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    memset(out, 0, sizeof(*out));
    int rc = seqpack_check_opts(c, opts);
    if (rc != TK_OK) return rc;
    DevBatch dev;
    uint64_t n_ids;
    if ((rc = encode_batch_for_layout(c, bytes, doc_offsets, n_docs, add_bos, add_eos, validate_utf8, &dev, &n_ids)) != TK_OK) return rc;
    tk_seqpack p;
    rc = run_seqpack(c, dev.ids, dev.id_offs, n_docs, n_ids, opts, c->stream, &p);
    if (rc != TK_OK) return rc;
    const uint64_t bytes_t = p.n_rows * p.row_len * ((opts->flags & TK_SEQPACK_I64) ? 8 : 4);
    CopyOut h[4] = {{p.input_ids, bytes_t, nullptr}, {p.position_ids, bytes_t, nullptr, p.position_ids != nullptr},
                    {p.segment_ids, bytes_t, nullptr, p.segment_ids != nullptr},
                    {p.cu_seqlens, (p.n_segments + 1) * 4, nullptr, p.cu_seqlens != nullptr}};
    if ((rc = copy_out(c, h, 4, "seqpack")) != TK_OK) return rc;
    *out = p;
    out->input_ids = h[0].host;
    out->position_ids = h[1].host;
    out->segment_ids = h[2].host;
    out->cu_seqlens = (int32_t*)h[3].host;
    return TK_OK;
}
