// tk_capi_rowfit.cpp -- whole documents packed into rows without cutting them (include/tekken_hip.h tk_rowfit_from_ids_device and
// the entries around it; csrc/tk_rowfit.hip): next-fit placement in the caller's order, with labels, position_ids, segment_ids,
// cu_seqlens and doc_start.
#include "tk_capi_layout.h"

#define TK_ROWFIT_ALL_FLAGS (TK_ROWFIT_I64 | TK_ROWFIT_POSITIONS | TK_ROWFIT_SEGMENTS | TK_ROWFIT_CU_SEQLENS | TK_ROWFIT_LABELS | TK_ROWFIT_DOC_START)

// the options that can be refused before the number of ids is known (step 9 of the definition)
static int rowfit_check_opts(tk_ctx* c, const tk_rowfit_opts* o) {
    if (!o) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    if (o->flags & ~(uint32_t)TK_ROWFIT_ALL_FLAGS) { c->err = "unknown rowfit flag"; return TK_ERR_INVALID_ARG; }
    if (o->seq_len == 0) { c->err = "rowfit needs a seq_len"; return TK_ERR_INVALID_ARG; }
    if (o->seq_len > TK_LAYOUT_MAX_ROW) { c->err = "seq_len " + std::to_string(o->seq_len) + " is beyond 2^31 - 1"; return TK_ERR_INVALID_ARG; }
    if (o->keep_tail > o->seq_len) {
        c->err = "keep_tail " + std::to_string(o->keep_tail) + " is beyond seq_len " + std::to_string(o->seq_len);
        return TK_ERR_INVALID_ARG;
    }
    return TK_OK;
}

// ... of the entries that encode text first: text has no labels stream, and that is refused before anything is encoded
static int rowfit_encode_opts(tk_ctx* c, const tk_rowfit_opts* opts, int, int, tk_rowfit_opts* o) {
    *o = *opts;
    int rc = rowfit_check_opts(c, o);
    if (rc == TK_OK && (o->flags & TK_ROWFIT_LABELS)) { c->err = "TK_ROWFIT_LABELS: encoded text has no labels stream"; rc = TK_ERR_INVALID_ARG; }
    return rc;
}

// The rowfit pass over ids on the device into the context's c->rowfit buffers; *out gets the device pointers.  The placement goes to
// work buffers; ONE read (48 bytes: n_truncated, n_rows, sum e, where the offsets end) sizes the tensors, and only once the sizes are
// accepted is anything of an earlier result touched.  One wait ends the call.  The caller holds c->mu.
static int run_rowfit(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t n_ids, const int32_t* d_lab,
                      const tk_rowfit_opts* o, hipStream_t s, tk_rowfit* out) {
    int rc = rowfit_check_opts(c, o);
    if (rc != TK_OK) return rc;
    if ((rc = check_n_docs(c, n_docs)) != TK_OK) return rc;
    if (n_docs == 0 && n_ids) { c->err = "rowfit: ids without a document"; return TK_ERR_INVALID_ARG; }
    const uint64_t L = o->seq_len, D = n_docs;
    const bool i64 = (o->flags & TK_ROWFIT_I64) != 0, want_pos = (o->flags & TK_ROWFIT_POSITIONS) != 0,
               want_seg = (o->flags & TK_ROWFIT_SEGMENTS) != 0, want_cu = (o->flags & TK_ROWFIT_CU_SEQLENS) != 0,
               want_lab = (o->flags & TK_ROWFIT_LABELS) != 0, want_ds = (o->flags & TK_ROWFIT_DOC_START) != 0;
    if (want_lab && !d_lab && n_ids) { c->err = "TK_ROWFIT_LABELS needs a labels buffer"; return TK_ERR_INVALID_ARG; }
    const uint64_t esz = i64 ? 8 : 4;
    uint64_t n_rows = 0, sum_e = 0;
    unsigned long long stat[6] = {0, 0, 0, 0, 0, 0};   // n_truncated | n_segments | max_seqlen | n_rows | sum e | id_offs[D]
    bool staged = false;
    c->rowfit.ms[0] = c->rowfit.ms[1] = c->rowfit.ms[2] = 0.f;
    if (n_ids == 0) {                           // (no row: cu_seqlens = [0], doc_start = [0] * D, nothing to launch)
        TK_HIP(c, c->rowfit.ids.reserve(16));
        if (want_lab) TK_HIP(c, c->rowfit.lab.reserve(16));
        if (want_pos) TK_HIP(c, c->rowfit.pos.reserve(16));
        if (want_seg) TK_HIP(c, c->rowfit.seg.reserve(16));
        TK_HIP(c, c->rowfit.cu.reserve(16));
        TK_HIP(c, c->rowfit.dstart.reserve((D + 1) * 8));
        TK_HIP(c, hipMemsetAsync(c->rowfit.cu.p, 0, 4, s));
        TK_HIP(c, hipMemsetAsync(c->rowfit.dstart.p, 0, (D + 1) * 8, s));
    } else {
        TK_HIP(c, c->rowfit.stat.reserve(64));
        TK_HIP(c, c->rowfit.e.reserve(D * 4 + 16));
        TK_HIP(c, c->rowfit.nz.reserve(D * 4 + 16));
        TK_HIP(c, c->rowfit.E.reserve((D + 1) * 8));
        TK_HIP(c, c->rowfit.nzp.reserve((D + 1) * 8));
        TK_HIP(c, c->rowfit.ja.reserve((D + 1) * 8));
        TK_HIP(c, c->rowfit.jb.reserve((D + 1) * 8));
        TK_HIP(c, c->rowfit.row.reserve((D + 1) * 4 + 16));
        TK_HIP(c, c->rowfit.open.reserve((D + 2) * 8));
        TK_HIP(c, c->rowfit.segno.reserve(D * 4 + 16));
        TK_HIP(c, c->rowfit.bsum.reserve(scan_workspace_bytes(D)));
        TkRowfitArgs a;
        memset(&a, 0, sizeof(a));
        a.ids = d_ids;
        a.lab = want_lab ? d_lab : nullptr;
        a.id_offs = d_id_offs;
        a.n_docs = D;
        a.row_len = o->seq_len;
        a.pad_id = o->pad_id;
        a.keep_tail = o->keep_tail;
        a.ignore = o->ignore_index;
        a.e = (uint32_t*)c->rowfit.e.p;
        a.nz = (uint32_t*)c->rowfit.nz.p;
        a.E = (const uint64_t*)c->rowfit.E.p;
        a.nzp = (const uint64_t*)c->rowfit.nzp.p;
        a.jump_a = (uint64_t*)c->rowfit.ja.p;
        a.jump_b = (uint64_t*)c->rowfit.jb.p;
        a.row = (uint32_t*)c->rowfit.row.p;
        a.open = (uint64_t*)c->rowfit.open.p;
        a.segno = (uint32_t*)c->rowfit.segno.p;
        a.stat = (unsigned long long*)c->rowfit.stat.p;
        // Two neighbouring rows hold more than L ids together (the second one's first document did not fit the first), so
        // n_rows <= 2 * floor(N / (L + 1)) + 1, and a row holds a document: the rounds after which the chain's end is marked
        uint64_t r_max = 2 * (n_ids / (L + 1)) + 1;
        if (r_max > D) r_max = D;
        uint32_t rounds = 0;
        while ((1ull << rounds) <= r_max) ++rounds;
        for (Event& ev : c->rowfit.ev)
            if (!ev.h) TK_HIP(c, hipEventCreate(&ev.h));
        TK_HIP(c, hipMemsetAsync(a.stat, 0, 24, s));
        TK_HIP(c, hipEventRecord(c->rowfit.ev[0], s));
        TK_HIP(c, tk_launch_rowfit_len(a, s));
        if ((rc = scan_u32(c, c->rowfit.bsum, a.e, D, (uint64_t*)c->rowfit.E.p, s)) != TK_OK) return rc;
        if ((rc = scan_u32(c, c->rowfit.bsum, a.nz, D, (uint64_t*)c->rowfit.nzp.p, s)) != TK_OK) return rc;
        TK_HIP(c, tk_launch_rowfit_chain(a, rounds, s));
        TK_HIP(c, hipEventRecord(c->rowfit.ev[1], s));
        TK_HIP(c, hipMemcpyAsync(stat, a.stat, 48, hipMemcpyDeviceToHost, s));
        TK_HIP(c, hipStreamSynchronize(s));
        const uint64_t end = stat[5];
        sum_e = stat[4];
        (void)hipEventElapsedTime(&c->rowfit.ms_chain, c->rowfit.ev[0], c->rowfit.ev[1]);
        if (end != n_ids) {
            c->err = "rowfit: id_offsets end at " + std::to_string(end) + ", not at n_ids = " + std::to_string(n_ids);
            return TK_ERR_INVALID_ARG;
        }
        n_rows = stat[3];
        if (n_rows > TK_LAYOUT_MAX_ELEMS / L) return layout_too_large(c, "rowfit", n_rows, L);
        if (want_cu && n_rows * L >= (1ull << 31)) {
            c->err = "rowfit: cu_seqlens is int32 and " + std::to_string(n_rows) + " rows of " + std::to_string(L) + " elements do not fit";
            return TK_ERR_INVALID_ARG;
        }
        const uint64_t elems = n_rows * L;
        TK_HIP(c, c->rowfit.ids.reserve(elems * esz + 16));
        if (want_lab) TK_HIP(c, c->rowfit.lab.reserve(elems * 4 + 16));
        if (want_pos) TK_HIP(c, c->rowfit.pos.reserve(elems * esz + 16));
        if (want_seg) TK_HIP(c, c->rowfit.seg.reserve(elems * esz + 16));
        TK_HIP(c, c->rowfit.cu.reserve((D + n_rows + 2) * 4));
        TK_HIP(c, c->rowfit.dstart.reserve((D + 1) * 8));
        TK_HIP(c, c->rowfit.padf.reserve(n_rows * 4 + 16));
        TK_HIP(c, c->rowfit.padp.reserve((n_rows + 1) * 8));
        TK_HIP(c, c->rowfit.bsum.reserve(scan_workspace_bytes(n_rows)));
        a.n_rows = n_rows;
        a.padf = (uint32_t*)c->rowfit.padf.p;
        a.padp = (const uint64_t*)c->rowfit.padp.p;
        a.dstart = (uint64_t*)c->rowfit.dstart.p;
        a.out_ids = c->rowfit.ids.p;
        a.out_lab = want_lab ? (int32_t*)c->rowfit.lab.p : nullptr;
        a.out_pos = want_pos ? c->rowfit.pos.p : nullptr;
        a.out_seg = want_seg ? c->rowfit.seg.p : nullptr;
        a.cu = want_cu ? (int32_t*)c->rowfit.cu.p : nullptr;
        TK_HIP(c, hipEventRecord(c->rowfit.ev[2], s));
        TK_HIP(c, tk_launch_rowfit_place(a, s));
        if ((rc = scan_u32(c, c->rowfit.bsum, a.padf, n_rows, (uint64_t*)c->rowfit.padp.p, s)) != TK_OK) return rc;
        TK_HIP(c, hipEventRecord(c->rowfit.ev[3], s));
        TK_HIP(c, tk_launch_rowfit(a, i64, s));
        TK_HIP(c, hipEventRecord(c->rowfit.ev[4], s));
        TK_HIP(c, tk_launch_rowfit_cu(a, s));
        TK_HIP(c, hipEventRecord(c->rowfit.ev[0], s));   // (its first record has been waited for: the host read)
        staged = true;
        TK_HIP(c, hipMemcpyAsync(stat + 1, a.stat + 1, 16, hipMemcpyDeviceToHost, s));
    }
    TK_HIP(c, hipStreamSynchronize(s));
    if (staged) {
        float t = 0.f;
        (void)hipEventElapsedTime(&c->rowfit.ms[0], c->rowfit.ev[2], c->rowfit.ev[3]);
        c->rowfit.ms[0] += c->rowfit.ms_chain;
        (void)hipEventElapsedTime(&c->rowfit.ms[1], c->rowfit.ev[3], c->rowfit.ev[4]);
        (void)hipEventElapsedTime(&t, c->rowfit.ev[4], c->rowfit.ev[0]);
        c->rowfit.ms[2] = t;
    }
    out->input_ids = c->rowfit.ids.p;
    out->labels = want_lab ? (int32_t*)c->rowfit.lab.p : nullptr;
    out->position_ids = want_pos ? c->rowfit.pos.p : nullptr;
    out->segment_ids = want_seg ? c->rowfit.seg.p : nullptr;
    out->cu_seqlens = want_cu ? (int32_t*)c->rowfit.cu.p : nullptr;
    out->doc_start = want_ds ? (uint64_t*)c->rowfit.dstart.p : nullptr;
    out->n_rows = n_rows;
    out->row_len = L;
    out->n_segments = stat[1];
    out->max_seqlen = stat[2];
    out->n_truncated = stat[0];
    out->n_pad = n_rows * L - sum_e;
    return TK_OK;
}

namespace {
struct RowfitPass : LayoutPass<RowfitPass> {
    typedef tk_rowfit_opts Opts;
    typedef tk_rowfit Result;
    static constexpr const char* name = "rowfit";
    static uint64_t esz(const Opts& o) { return (o.flags & TK_ROWFIT_I64) ? 8 : 4; }
    static constexpr auto encode_opts = rowfit_encode_opts;
    static constexpr auto run = run_rowfit;
    // (encoded text has no labels stream)
    static int run_encoded(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t n_ids, const Opts* o, hipStream_t s,
                           Result* out) {
        return run_rowfit(c, d_ids, d_id_offs, n_docs, n_ids, nullptr, o, s, out);
    }
};
}  // namespace

extern "C" int tk_rowfit_from_ids_device(tk_ctx* c, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                                         const void* d_labels, const tk_rowfit_opts* opts, void* hip_stream, tk_rowfit* out) {
    return layout_from_ids_device<RowfitPass>(c, d_ids, d_id_offsets, n_docs, n_ids, opts, hip_stream, out, (const int32_t*)d_labels);
}
extern "C" int tk_encode_batch_device_rowfit(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs,
                                             uint64_t n_bytes, int add_bos, int add_eos, int checks, const tk_rowfit_opts* opts,
                                             void* hip_stream, void** d_ids, void** d_out_offsets, uint64_t* n_ids, tk_rowfit* out) {
    return layout_encode_device<RowfitPass>(c, d_bytes, d_doc_offsets, n_docs, n_bytes, add_bos, add_eos, checks, opts, hip_stream, d_ids,
                                            d_out_offsets, n_ids, out);
}
extern "C" int tk_encode_batch_rowfit(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos,
                                      int add_eos, int validate_utf8, const tk_rowfit_opts* opts, tk_rowfit* out) {
    return layout_encode_host<RowfitPass>(c, bytes, doc_offsets, n_docs, add_bos, add_eos, validate_utf8, opts, out);
}
extern "C" void tk_free_rowfit(tk_rowfit* r) { layout_free(r); }

extern "C" int tk_encode_parts_device_rowfit(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_parts, uint64_t n_bytes,
                                             const void* d_part_ctrl, const void* d_part_flags, const void* d_conv_offsets, uint64_t n_convs,
                                             int checks, const tk_join_opts* join_opts, const tk_rowfit_opts* opts, void* hip_stream,
                                             tk_join* joined, tk_rowfit* out) {
    TK_ENTRY(c);
    if (!joined || !out || !join_opts) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    int rc = rowfit_check_opts(c, opts);
    if (rc != TK_OK) return rc;
    if ((opts->flags & TK_ROWFIT_LABELS) && !(join_opts->flags & TK_JOIN_LABELS)) {   // (before anything is encoded or joined)
        c->err = "TK_ROWFIT_LABELS needs the join's labels: TK_JOIN_LABELS";
        return TK_ERR_INVALID_ARG;
    }
    rc = encode_parts_device_join(c, d_bytes, d_doc_offsets, n_parts, n_bytes, d_part_ctrl, d_part_flags, d_conv_offsets, n_convs, checks,
                                  join_opts, hip_stream, joined);
    if (rc != TK_OK) return rc;
    return run_rowfit(c, joined->ids, joined->offsets, n_convs, joined->n_ids, joined->labels, opts, (hipStream_t)hip_stream, out);
}

extern "C" void tk_last_rowfit_ms(const tk_ctx* c, float* placement_ms, float* fill_ms, float* cu_ms) {
    std::unique_lock<std::mutex> lock;
    if (c) lock = std::unique_lock<std::mutex>(const_cast<tk_ctx*>(c)->mu);   // (a call on another thread writes them under it)
    if (placement_ms) *placement_ms = c ? c->rowfit.ms[0] : 0.f;
    if (fill_ms) *fill_ms = c ? c->rowfit.ms[1] : 0.f;
    if (cu_ms) *cu_ms = c ? c->rowfit.ms[2] : 0.f;
}
