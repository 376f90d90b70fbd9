// tk_capi_seqpack.cpp -- packed fixed-length training rows (include/tekken_hip.h tk_seqpack_from_ids_device and the entries
// around it; csrc/tk_seqpack.hip): the stream of all ids cut into rows of seq_len, with position_ids, segment_ids and cu_seqlens.
#include "tk_capi_layout.h"

#define TK_SEQPACK_ALL_FLAGS (TK_SEQPACK_I64 | TK_SEQPACK_POSITIONS | TK_SEQPACK_SEGMENTS | TK_SEQPACK_CU_SEQLENS | TK_SEQPACK_DROP_LAST)

// the options that can be refused before the number of ids is known (step 8 of the definition)
static int seqpack_check_opts(tk_ctx* c, const tk_seqpack_opts* o) {
    if (!o) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    if (o->flags & ~(uint32_t)TK_SEQPACK_ALL_FLAGS) { c->err = "unknown seqpack flag"; return TK_ERR_INVALID_ARG; }
    if (o->seq_len == 0) { c->err = "seqpack needs a seq_len"; return TK_ERR_INVALID_ARG; }
    if (o->seq_len > TK_LAYOUT_MAX_ROW) { c->err = "seq_len " + std::to_string(o->seq_len) + " is beyond 2^31 - 1"; return TK_ERR_INVALID_ARG; }
    return TK_OK;
}

// The packed pass over ids on the device into the context's c->seqpack buffers; *out gets the device pointers.  n_rows, n_used and
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
    if (n_rows > TK_LAYOUT_MAX_ELEMS / L) return layout_too_large(c, "seqpack", n_rows, L);
    if (want_cu && n_used >= (1ull << 31)) {
        c->err = "seqpack: cu_seqlens is int32 and " + std::to_string(n_used) + " ids do not fit";
        return TK_ERR_INVALID_ARG;
    }
    const uint64_t elems = n_rows * L, esz = i64 ? 8 : 4;
    TK_HIP(c, c->seqpack.stat.reserve(64));
    TK_HIP(c, c->seqpack.ids.reserve(elems * esz + 16));
    if (want_pos) TK_HIP(c, c->seqpack.pos.reserve(elems * esz + 16));
    if (want_seg) TK_HIP(c, c->seqpack.seg.reserve(elems * esz + 16));
    if (want_cu) TK_HIP(c, c->seqpack.cu.reserve((n_docs + n_rows + 2) * 4));
    unsigned long long stat[2] = {0, 0};
    if (n_used == 0) {                          // (no row: cu_seqlens = [0], nothing to launch)
        if (want_cu) TK_HIP(c, hipMemsetAsync(c->seqpack.cu.p, 0, 4, s));
    } else {
        TK_HIP(c, c->seqpack.flags.reserve(n_docs * 4 + 16));
        TK_HIP(c, c->seqpack.aflags.reserve(n_docs * 4 + 16));
        TK_HIP(c, c->seqpack.fpos.reserve((n_docs + 1) * 8));
        TK_HIP(c, c->seqpack.apos.reserve((n_docs + 1) * 8));
        TK_HIP(c, c->seqpack.starts.reserve((n_docs + 1) * 8));
        TK_HIP(c, c->seqpack.aligned.reserve((n_docs + 1) * 8));
        TK_HIP(c, c->seqpack.bsum.reserve(scan_workspace_bytes(n_docs)));
        TkSeqpackArgs a;
        memset(&a, 0, sizeof(a));
        a.ids = d_ids;
        a.id_offs = d_id_offs;
        a.n_docs = n_docs;
        a.row_len = o->seq_len;
        a.pad_id = o->pad_id;
        a.n_rows = n_rows;
        a.n_used = n_used;
        a.flags = (uint32_t*)c->seqpack.flags.p;
        a.aflags = (uint32_t*)c->seqpack.aflags.p;
        a.fpos = (const uint64_t*)c->seqpack.fpos.p;
        a.apos = (const uint64_t*)c->seqpack.apos.p;
        a.starts = (uint64_t*)c->seqpack.starts.p;
        a.n_aligned = (uint64_t*)c->seqpack.aligned.p;
        a.out_ids = c->seqpack.ids.p;
        a.out_pos = want_pos ? c->seqpack.pos.p : nullptr;
        a.out_seg = want_seg ? c->seqpack.seg.p : nullptr;
        a.cu = want_cu ? (int32_t*)c->seqpack.cu.p : nullptr;
        a.stat = (unsigned long long*)c->seqpack.stat.p;
        TK_HIP(c, hipMemsetAsync(a.stat, 0, 16, s));
        TK_HIP(c, tk_launch_seqpack_flags(a, s));
        if ((rc = scan_u32(c, c->seqpack.bsum, a.flags, n_docs, (uint64_t*)c->seqpack.fpos.p, s)) != TK_OK) return rc;
        if ((rc = scan_u32(c, c->seqpack.bsum, a.aflags, n_docs, (uint64_t*)c->seqpack.apos.p, s)) != TK_OK) return rc;
        TK_HIP(c, tk_launch_seqpack_starts(a, s));
        TK_HIP(c, tk_launch_seqpack(a, i64, s));
        TK_HIP(c, tk_launch_seqpack_cu(a, s));
        TK_HIP(c, hipMemcpyAsync(stat, a.stat, 16, hipMemcpyDeviceToHost, s));
    }
    TK_HIP(c, hipStreamSynchronize(s));
    out->input_ids = c->seqpack.ids.p;
    out->position_ids = want_pos ? c->seqpack.pos.p : nullptr;
    out->segment_ids = want_seg ? c->seqpack.seg.p : nullptr;
    out->cu_seqlens = want_cu ? (int32_t*)c->seqpack.cu.p : nullptr;
    out->n_rows = n_rows;
    out->row_len = L;
    out->n_used = n_used;
    out->n_left = n_ids - n_used;
    out->n_segments = stat[0];
    out->max_seqlen = stat[1];
    return TK_OK;
}

namespace {
struct SeqpackPass : LayoutPass<SeqpackPass> {
    typedef tk_seqpack_opts Opts;
    typedef tk_seqpack Result;
    static constexpr const char* name = "seqpack";
    static uint64_t esz(const Opts& o) { return (o.flags & TK_SEQPACK_I64) ? 8 : 4; }
    // the options of an entry that encodes first are the caller's
    static int encode_opts(tk_ctx* c, const Opts* opts, int, int, Opts* o) { *o = *opts; return seqpack_check_opts(c, o); }
    static constexpr auto run = run_seqpack;
};
}  // namespace

extern "C" int tk_seqpack_from_ids_device(tk_ctx* c, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                                          const tk_seqpack_opts* opts, void* hip_stream, tk_seqpack* out) {
    return layout_from_ids_device<SeqpackPass>(c, d_ids, d_id_offsets, n_docs, n_ids, opts, hip_stream, out);
}
extern "C" int tk_encode_batch_device_seqpack(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs,
                                              uint64_t n_bytes, int add_bos, int add_eos, int checks, const tk_seqpack_opts* opts,
                                              void* hip_stream, void** d_ids, void** d_out_offsets, uint64_t* n_ids, tk_seqpack* out) {
    return layout_encode_device<SeqpackPass>(c, d_bytes, d_doc_offsets, n_docs, n_bytes, add_bos, add_eos, checks, opts, hip_stream, d_ids,
                                             d_out_offsets, n_ids, out);
}
extern "C" int tk_encode_batch_seqpack(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos,
                                       int add_eos, int validate_utf8, const tk_seqpack_opts* opts, tk_seqpack* out) {
    return layout_encode_host<SeqpackPass>(c, bytes, doc_offsets, n_docs, add_bos, add_eos, validate_utf8, opts, out);
}
extern "C" void tk_free_seqpack(tk_seqpack* r) { layout_free(r); }
