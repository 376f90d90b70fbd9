// tk_capi_fim.cpp -- fill-in-the-middle rows (include/tekken_hip.h tk_fim_split_device and the entries around it; csrc/tk_fim.hip):
// packed text or ids in; every chosen document cut in two places and written back in the new order inside its own range, with
// the part tables that tk_encode_parts_device_join / tk_join_from_ids_device take.  The composite entries run split -> join.
#include "tk_capi_layout.h"

#define TK_FIM_ALL_FLAGS (TK_FIM_SNAP | TK_FIM_BOS | TK_FIM_EOS | TK_FIM_PART_SRC | TK_FIM_LABEL_MIDDLE)

// step 8 of the definition: what is refused before any launch
static int fim_check_opts(tk_ctx* c, const tk_fim_opts* o, int unit_bytes, uint64_t n_docs) {
    if (!o) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    if (o->flags & ~(uint32_t)TK_FIM_ALL_FLAGS) { c->err = "unknown fim flag"; return TK_ERR_INVALID_ARG; }
    if (unit_bytes == 4 && (o->flags & (TK_FIM_BOS | TK_FIM_EOS))) {
        c->err = "fim: TK_FIM_BOS / TK_FIM_EOS belong to the text entries (stored ids carry theirs: head / tail)";
        return TK_ERR_INVALID_ARG;
    }
    if (o->rate_q32 > (1ull << 32) || o->spm_q32 > (1ull << 32)) { c->err = "fim: rate_q32 / spm_q32 above 2^32"; return TK_ERR_INVALID_ARG; }
    if (unit_bytes == 1 && (o->head || o->tail)) { c->err = "fim: head / tail belong to the ids entries"; return TK_ERR_INVALID_ARG; }
    const uint32_t ids[3] = {o->prefix_id, o->suffix_id, o->middle_id};
    for (uint32_t id : ids)
        if (id != TK_JOIN_NONE && id >= c->host.num_special) {
            c->err = "fim: control id " + std::to_string(id) + " is neither TK_JOIN_NONE nor below num_special_tokens (" +
                     std::to_string(c->host.num_special) + ")";
            return TK_ERR_INVALID_ARG;
        }
    return check_n_docs(c, n_docs);
}

// The FIM pass over units on the device into the context's c->fim buffers; *out gets the device pointers.  Everything that can be
// refused has been refused by the caller (fim_check_opts, the checks of the text); nothing is read before the launches, ONE wait at
// the end fetches the three counters.  The caller holds c->mu.
static int run_fim(tk_ctx* c, const void* d_units, const void* d_offs, uint64_t n_docs, uint64_t n_units, const void* d_cuts, int unit_bytes,
                   const tk_fim_opts* o, hipStream_t s, tk_fim* out) {
    FimBufs& b = c->fim;
    const uint64_t D = n_docs, P = 5u * D;
    const bool want_src = (o->flags & TK_FIM_PART_SRC) != 0;
    const bool copy = d_cuts != nullptr || o->rate_q32 != 0;   // (nothing can be transformed: the caller's own units, not copied)
    b.ms[0] = b.ms[1] = 0.f;
    for (Event& ev : b.ev)
        if (!ev.h) TK_HIP(c, hipEventCreate(&ev.h));
    TK_HIP(c, b.stat.reserve(64));
    TK_HIP(c, b.poffs.reserve((P + 1) * 8));
    TK_HIP(c, b.ctrl.reserve(P * 4 + 16));
    TK_HIP(c, b.pflags.reserve(P * 4 + 16));
    TK_HIP(c, b.conv.reserve((D + 1) * 8));
    TK_HIP(c, b.cuts.reserve(D * 16 + 16));
    TK_HIP(c, b.mode.reserve(D + 16));
    if (want_src) TK_HIP(c, b.psrc.reserve(P * 8 + 16));
    if (copy) TK_HIP(c, b.units.reserve(n_units * unit_bytes + 16));
    TkFimArgs a;
    memset(&a, 0, sizeof(a));
    a.units = d_units;
    a.offs = (const uint64_t*)d_offs;
    a.n_docs = D;
    a.n_units = n_units;
    a.in_cuts = (const uint64_t*)d_cuts;
    a.rate = o->rate_q32;
    a.spm = o->spm_q32;
    for (uint32_t k = 0; k < 4; ++k) a.s[k] = tki_hash(o->seed, TKI_SEED_BASE + k);
    a.ctrl[0] = o->prefix_id; a.ctrl[1] = o->suffix_id; a.ctrl[2] = o->middle_id;
    a.head = o->head; a.tail = o->tail; a.min_units = o->min_units; a.flags = o->flags;
    a.bos = (o->flags & TK_FIM_BOS) ? c->host.bos_id : TK_JOIN_NONE;
    a.eos = (o->flags & TK_FIM_EOS) ? c->host.eos_id : TK_JOIN_NONE;
    a.out_units = b.units.p;
    a.part_offs = (uint64_t*)b.poffs.p;
    a.part_ctrl = (uint32_t*)b.ctrl.p;
    a.part_flags = (uint32_t*)b.pflags.p;
    a.conv_offs = (uint64_t*)b.conv.p;
    a.part_src = want_src ? (uint64_t*)b.psrc.p : nullptr;
    a.cuts = (uint64_t*)b.cuts.p;
    a.mode = (uint8_t*)b.mode.p;
    a.stat = (unsigned long long*)b.stat.p;
    unsigned long long got[3] = {0, 0, 0};              // n_transformed, n_spm, n_skipped
    TK_HIP(c, hipMemsetAsync(a.stat, 0, 24, s));
    TK_HIP(c, hipEventRecord(b.ev[0], s));
    TK_HIP(c, tk_launch_fim_cut(a, unit_bytes, s));
    TK_HIP(c, hipEventRecord(b.ev[1], s));
    if (copy) TK_HIP(c, tk_launch_fim_permute(a, unit_bytes, s));
    TK_HIP(c, hipEventRecord(b.ev[2], s));
    TK_HIP(c, hipMemcpyAsync(got, a.stat, 24, hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&b.ms[0], b.ev[0], b.ev[1]);
    if (copy) (void)hipEventElapsedTime(&b.ms[1], b.ev[1], b.ev[2]);
    out->units = copy ? b.units.p : const_cast<void*>(d_units);
    out->part_offsets = a.part_offs;
    out->part_ctrl = a.part_ctrl;
    out->part_flags = a.part_flags;
    out->conv_offsets = a.conv_offs;
    out->part_src = a.part_src;
    out->cuts = a.cuts;
    out->mode = a.mode;
    out->n_docs = D;
    out->n_parts = P;
    out->n_units = n_units;
    out->n_transformed = got[0];
    out->n_spm = got[1];
    out->n_skipped = got[2];
    return TK_OK;
}

// the text split behind its checks
static int fim_split_text(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes, const void* d_cuts,
                          int checks, const tk_fim_opts* opts, hipStream_t s, tk_fim* out) {
    int rc = fim_check_opts(c, opts, 1, n_docs);
    if (rc != TK_OK) return rc;
    TK_HIP(c, hipSetDevice(c->device));
    if (checks && (rc = check_text_device(c, d_bytes, d_doc_offsets, n_docs, n_bytes, checks, s)) != TK_OK) return rc;
    return run_fim(c, d_bytes, d_doc_offsets, n_docs, n_bytes, d_cuts, 1, opts, s, out);
}

extern "C" int tk_fim_split_device(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                   const void* d_cuts, int checks, const tk_fim_opts* opts, void* hip_stream, tk_fim* out) {
    TK_ENTRY(c);
    int rc = check_flags_and_args(c, checks, TK_CHECK_OFFSETS | TK_CHECK_UTF8, !d_doc_offsets || (!d_bytes && n_bytes) || !opts || !out);
    if (rc != TK_OK) return rc;
    return fim_split_text(c, d_bytes, d_doc_offsets, n_docs, n_bytes, d_cuts, checks, opts, (hipStream_t)hip_stream, out);
}

extern "C" int tk_fim_split_ids_device(tk_ctx* c, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                                       const void* d_cuts, const tk_fim_opts* opts, void* hip_stream, tk_fim* out) {
    TK_ENTRY(c);
    if (!d_id_offsets || (!d_ids && n_ids) || !opts || !out) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    int rc = fim_check_opts(c, opts, 4, n_docs);
    if (rc != TK_OK) return rc;
    TK_HIP(c, hipSetDevice(c->device));
    return run_fim(c, d_ids, d_id_offsets, n_docs, n_ids, d_cuts, 4, opts, (hipStream_t)hip_stream, out);
}

// (the body of tk_encode_batch_device_fim; the caller holds c->mu.  parts: optional)
static int encode_device_fim(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes, const void* d_cuts,
                             int checks, const tk_fim_opts* opts, const tk_join_opts* jopts, void* hip_stream, tk_fim* parts, tk_join* out) {
    int rc = check_flags_and_args(c, checks, TK_CHECK_OFFSETS | TK_CHECK_UTF8, !d_doc_offsets || (!d_bytes && n_bytes) || !opts || !jopts || !out);
    if (rc != TK_OK) return rc;
    // (the join's options are refused before the text is split; 5 parts a document: D < (2^32 - 16) / 5 goes through)
    if ((rc = fim_check_opts(c, opts, 1, n_docs)) != TK_OK || (rc = join_check_args(c, 5u * n_docs, n_docs, jopts)) != TK_OK) return rc;
    tk_fim f;
    if ((rc = fim_split_text(c, d_bytes, d_doc_offsets, n_docs, n_bytes, d_cuts, checks, opts, (hipStream_t)hip_stream, &f)) != TK_OK) return rc;
    if (parts) *parts = f;
    return encode_parts_device_join(c, f.units, f.part_offsets, f.n_parts, f.n_units, f.part_ctrl, f.part_flags, f.conv_offsets, n_docs, 0,
                                    jopts, hip_stream, out);
}

extern "C" int tk_encode_batch_device_fim(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                          const void* d_cuts, int checks, const tk_fim_opts* opts, const tk_join_opts* jopts, void* hip_stream,
                                          tk_fim* parts, tk_join* out) {
    TK_ENTRY(c);
    return encode_device_fim(c, d_bytes, d_doc_offsets, n_docs, n_bytes, d_cuts, checks, opts, jopts, hip_stream, parts, out);
}

extern "C" int tk_fim_from_ids_device(tk_ctx* c, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids, const void* d_cuts,
                                      const tk_fim_opts* opts, const tk_join_opts* jopts, void* hip_stream, tk_fim* parts, tk_join* out) {
    TK_ENTRY(c);
    if (!d_id_offsets || (!d_ids && n_ids) || !opts || !jopts || !out) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    int rc;
    if ((rc = fim_check_opts(c, opts, 4, n_docs)) != TK_OK || (rc = join_check_args(c, 5u * n_docs, n_docs, jopts)) != TK_OK) return rc;
    TK_HIP(c, hipSetDevice(c->device));
    tk_fim f;
    if ((rc = run_fim(c, d_ids, d_id_offsets, n_docs, n_ids, d_cuts, 4, opts, (hipStream_t)hip_stream, &f)) != TK_OK) return rc;
    if (parts) *parts = f;
    return run_join(c, (const uint32_t*)f.units, f.part_offsets, f.n_parts, n_ids, f.part_ctrl, f.part_flags, f.conv_offsets, n_docs, false, jopts,
                    (hipStream_t)hip_stream, out);
}

extern "C" int tk_encode_batch_fim(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, const uint64_t* cuts,
                                   int validate_utf8, const tk_fim_opts* opts, const tk_join_opts* jopts, tk_fim* parts, tk_join* out) {
    TK_ENTRY(c);
    if (!opts || !jopts || !out || !doc_offsets || (!bytes && doc_offsets[n_docs])) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    memset(out, 0, sizeof(*out));
    if (parts) memset(parts, 0, sizeof(*parts));
    int rc = fim_check_opts(c, opts, 1, n_docs);
    if (rc != TK_OK || (rc = check_offsets(c, doc_offsets, n_docs)) != TK_OK) return rc;
    TK_HIP(c, hipSetDevice(c->device));
    FimBufs& b = c->fim;
    const uint64_t n_bytes = doc_offsets[n_docs];
    TK_HIP(c, b.in_units.reserve(n_bytes + 64));
    TK_HIP(c, b.in_offs.reserve((n_docs + 1) * 8));
    if (cuts) TK_HIP(c, b.in_cuts.reserve(n_docs * 16 + 16));
    if (n_bytes) TK_HIP(c, hipMemcpyAsync(b.in_units.p, bytes, n_bytes, hipMemcpyHostToDevice, c->stream));
    TK_HIP(c, hipMemcpyAsync(b.in_offs.p, doc_offsets, (n_docs + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (cuts && n_docs) TK_HIP(c, hipMemcpyAsync(b.in_cuts.p, cuts, n_docs * 16, hipMemcpyHostToDevice, c->stream));
    tk_fim f;
    tk_join j;
    rc = encode_device_fim(c, b.in_units.p, b.in_offs.p, n_docs, n_bytes, cuts ? b.in_cuts.p : nullptr, validate_utf8 ? TK_CHECK_UTF8 : 0, opts, jopts,
                           c->stream, &f, &j);
    if (rc != TK_OK) { (void)hipStreamSynchronize(c->stream); return rc; }   // (the copies of the caller's arrays have ended when the call returns)
    if ((rc = layout_copy_out(c, j, 4, n_docs, "join", out)) != TK_OK) return rc;
    if (parts && (rc = layout_copy_out(c, f, 1, n_docs, "fim", parts)) != TK_OK) { layout_free(out); return rc; }
    return TK_OK;
}

extern "C" void tk_free_fim(tk_fim* r) { layout_free(r); }

extern "C" void tk_last_fim_ms(const tk_ctx* c, float ms[2]) {
    std::unique_lock<std::mutex> lock;
    if (c) lock = std::unique_lock<std::mutex>(const_cast<tk_ctx*>(c)->mu);   // (a call on another thread writes them under it)
    for (int i = 0; ms && i < 2; ++i) ms[i] = c ? c->fim.ms[i] : 0.f;
}

extern "C" uint32_t tk_fim_tile(int unit_bytes) { return unit_bytes == 1 ? TKI_TILE1 : unit_bytes == 4 ? TKI_TILE4 : 0u; }
