// tk_capi_decode_lossy.cpp -- the lossy decode entries of the C ABI (include/tekken_hip.h; csrc/tk_decode_lossy.hip): the repair
// pass behind the strict pipeline of tk_capi_decode.cpp, and the stream step for generation.
#include "tk_ctx.h"

// The strict pipeline, then -- only where the validation found an invalid run -- the repair pass over its raw text.  *bytes / *offs:
// where the result lives (the strict pipeline's own buffers on the fast path).
static int run_decode_lossy(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t n_ids, int policy,
                            hipStream_t s, uint64_t* n_bytes, uint64_t* bad_doc, uint64_t* first_bad, void** bytes, void** offs) {
    DecodeLossyBufs& L = c->lossy;
    L.strict_ms = L.repair_ms = 0.f;
    L.n_replaced = L.n_bad_docs = 0;
    L.repair_launches = 0;
    uint64_t raw = 0, u8bad = ~0ull;
    int rc = run_decode(c, d_ids, d_id_offs, n_docs, n_ids, policy, s, &raw, bad_doc, &u8bad);
    if (rc != TK_OK) return rc;
    L.strict_ms = c->pipeline_ms;
    if (first_bad) *first_bad = u8bad;
    *bytes = c->dec_bytes.p;
    *offs = c->dec_offs.p;
    *n_bytes = raw;
    if (u8bad == ~0ull) return TK_OK;                  // every run is valid: the raw buffers are the result
    const uint64_t n_tiles = (raw + TK_LOSSY_TILE - 1) / TK_LOSSY_TILE;
    TK_HIP(c, L.tcnt.reserve((n_tiles + 1) * 4));
    TK_HIP(c, L.toffs.reserve((n_tiles + 2) * 8));
    TK_HIP(c, L.flags.reserve((n_docs + 1) * 4));
    TK_HIP(c, L.stat.reserve(16));
    TK_HIP(c, L.offs.reserve((n_docs + 1) * 8));
    TK_HIP(c, L.bsum.reserve(scan_workspace_bytes(n_tiles)));
    for (Event& ev : L.ev)
        if (!ev.h) TK_HIP(c, hipEventCreate(&ev.h));
    TkLossyArgs a;
    memset(&a, 0, sizeof(a));
    a.bytes = (const uint8_t*)c->dec_bytes.p;
    a.n_bytes = raw;
    a.offs = (const uint64_t*)c->dec_offs.p;
    a.n_docs = n_docs;
    a.run_bits = (const uint32_t*)c->dec_bits.p;
    a.tile_cnt = (uint32_t*)L.tcnt.p;
    a.tile_offs = (const uint64_t*)L.toffs.p;
    a.out_offs = (uint64_t*)L.offs.p;
    a.bad_flags = (uint32_t*)L.flags.p;
    a.stat = (unsigned long long*)L.stat.p;
    TK_HIP(c, hipEventRecord(L.ev[0], s));
    TK_HIP(c, hipMemsetAsync(L.flags.p, 0, (n_docs + 1) * 4, s));
    TK_HIP(c, hipMemsetAsync(L.stat.p, 0, 16, s));
    TK_HIP(c, tk_launch_decode_lossy_counts(a, s));
    if ((rc = scan_u32(c, L.bsum, a.tile_cnt, n_tiles, (uint64_t*)L.toffs.p, s)) != TK_OK) return rc;
    uint64_t total = 0;
    TK_HIP(c, hipMemcpyAsync(&total, (uint64_t*)L.toffs.p + n_tiles, 8, hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipStreamSynchronize(s));
    TK_HIP(c, L.bytes.reserve(total + 64));
    a.out_bytes = (uint8_t*)L.bytes.p;
    TK_HIP(c, tk_launch_decode_lossy_write(a, s));
    TK_HIP(c, hipEventRecord(L.ev[1], s));
    unsigned long long stat[2] = {0, 0};
    TK_HIP(c, hipMemcpyAsync(stat, L.stat.p, 16, hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&L.repair_ms, L.ev[0], L.ev[1]);
    L.n_replaced = stat[0];
    L.n_bad_docs = stat[1];
    L.repair_launches = 5;                             // counts, the scan's three, write
    *bytes = L.bytes.p;
    *offs = L.offs.p;
    *n_bytes = total;
    return TK_OK;
}

extern "C" int tk_decode_batch_device_lossy(tk_ctx* c, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                                            int policy, void* hip_stream, void** d_bytes, void** d_out_offsets, uint64_t* n_bytes,
                                            uint64_t* bad_doc, uint64_t* n_replaced, uint64_t* first_bad_doc) {
    TK_ENTRY(c);
    if (!d_id_offsets || (!d_ids && n_ids) || !d_bytes || !d_out_offsets || !n_bytes) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    TK_HIP(c, hipSetDevice(c->device));
    int rc = run_decode_lossy(c, (const uint32_t*)d_ids, (const uint64_t*)d_id_offsets, n_docs, n_ids, policy, (hipStream_t)hip_stream,
                              n_bytes, bad_doc, first_bad_doc, d_bytes, d_out_offsets);
    if (rc != TK_OK) return rc;
    if (n_replaced) *n_replaced = c->lossy.n_replaced;
    return TK_OK;
}

extern "C" int tk_decode_batch_lossy(tk_ctx* c, const uint32_t* ids, const uint64_t* id_offsets, uint64_t n_docs, int policy,
                                     tk_text_result* out, uint64_t* bad_doc, uint64_t* n_replaced, uint64_t* first_bad_doc) {
    TK_ENTRY(c);
    if (!id_offsets || !out || (!ids && id_offsets[n_docs])) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    memset(out, 0, sizeof(*out));
    int rc = check_offsets(c, id_offsets, n_docs);
    if (rc != TK_OK) return rc;
    TK_HIP(c, hipSetDevice(c->device));
    const uint64_t n_ids = id_offsets[n_docs];
    TK_HIP(c, c->dec_in_ids.reserve((n_ids + 1) * 4));
    TK_HIP(c, c->dec_in_offs.reserve((n_docs + 1) * 8));
    if (n_ids) TK_HIP(c, hipMemcpyAsync(c->dec_in_ids.p, ids, n_ids * 4, hipMemcpyHostToDevice, c->stream));
    TK_HIP(c, hipMemcpyAsync(c->dec_in_offs.p, id_offsets, (n_docs + 1) * 8, hipMemcpyHostToDevice, c->stream));
    uint64_t n_bytes = 0;
    void* d_bytes = nullptr;
    void* d_offs = nullptr;
    rc = run_decode_lossy(c, (const uint32_t*)c->dec_in_ids.p, (const uint64_t*)c->dec_in_offs.p, n_docs, n_ids, policy, c->stream,
                          &n_bytes, bad_doc, first_bad_doc, &d_bytes, &d_offs);
    if (rc != TK_OK) return rc;
    CopyOut h[2] = {{d_bytes, n_bytes, nullptr}, {d_offs, (n_docs + 1) * 8, nullptr}};
    if ((rc = copy_out(c, h, 2, "result")) != TK_OK) return rc;
    out->bytes = (uint8_t*)h[0].host;
    out->offsets = (uint64_t*)h[1].host;
    out->n_bytes = n_bytes;
    out->n_docs = n_docs;
    if (n_replaced) *n_replaced = c->lossy.n_replaced;
    return TK_OK;
}

// One step over ids and states on the device.  Count kernel, scan, ONE host read (the total and the two error words behind it),
// write kernel -- which alone touches the states, and is not launched when the count kernel flagged an error.
static int run_stream_step(tk_ctx* c, uint32_t* d_state, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_seqs, int policy,
                           int flags, hipStream_t s, uint64_t* n_bytes, uint64_t* bad_seq) {
    if (policy < TK_POLICY_IGNORE || policy > TK_POLICY_RAISE) { c->err = "invalid policy"; return TK_ERR_INVALID_ARG; }
    if (policy == TK_POLICY_KEEP && !c->have_specials) { c->err = "TK_POLICY_KEEP needs tk_ctx_set_special_tokens first"; return TK_ERR_INVALID_ARG; }
    if (flags & ~TK_STREAM_FINAL) { c->err = "unknown stream flag"; return TK_ERR_INVALID_ARG; }
    DecodeLossyBufs& L = c->lossy;
    TK_HIP(c, L.s_lens.reserve((n_seqs + 1) * 4));
    TK_HIP(c, L.s_offs.reserve((n_seqs + 3) * 8));
    TK_HIP(c, L.s_stat.reserve(8));
    TK_HIP(c, L.s_bsum.reserve(scan_workspace_bytes(n_seqs)));
    TkStreamArgs a;
    memset(&a, 0, sizeof(a));
    a.state = d_state;
    a.ids = d_ids;
    a.id_offs = d_id_offs;
    a.n_seqs = n_seqs;
    a.lens = (uint32_t*)L.s_lens.p;
    a.out_offs = (const uint64_t*)L.s_offs.p;
    a.err = (unsigned long long*)L.s_offs.p + n_seqs + 1;
    a.stat = (unsigned long long*)L.s_stat.p;
    a.tok_blob = (const uint8_t*)c->t_blob.p;
    a.tok_offs = (const uint32_t*)c->t_offs.p;
    a.sp_blob = (const uint8_t*)c->t_spblob.p;
    a.sp_offs = (const uint32_t*)c->t_spoffs.p;
    a.n_ranks = c->host.n_ranks;
    a.num_special = c->host.num_special;
    a.policy = policy;
    a.flags = flags;
    TK_HIP(c, hipMemsetAsync(a.err, 0xFF, 16, s));
    TK_HIP(c, hipMemsetAsync(a.stat, 0, 8, s));
    TK_HIP(c, tk_launch_decode_stream_count(a, s));
    int rc = scan_u32(c, L.s_bsum, a.lens, n_seqs, (uint64_t*)L.s_offs.p, s);
    if (rc != TK_OK) return rc;
    unsigned long long head[3] = {0, ~0ull, ~0ull};    // total | first RAISE special | first id outside the vocabulary
    TK_HIP(c, hipMemcpyAsync(head, (uint64_t*)L.s_offs.p + n_seqs, 24, hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipStreamSynchronize(s));
    if (head[1] != ~0ull || head[2] != ~0ull) {
        // the first offending id decides (id indices run with the sequences); the states were only read
        const bool special = head[1] < head[2];
        uint64_t q = 0;
        if ((rc = doc_of_id(c, d_id_offs, n_seqs, special ? head[1] : head[2], &q)) != TK_OK) return rc;
        if (bad_seq) *bad_seq = q;
        if (special) {
            c->err = "Decoding tokens that contain special tokens is not allowed (sequence " + std::to_string(q) + ")";
            return TK_ERR_SPECIAL_POLICY;
        }
        c->err = "DecodeKeyError: invalid token for decoding (sequence " + std::to_string(q) + ")";
        return TK_ERR_RUNTIME;
    }
    TK_HIP(c, L.s_bytes.reserve(head[0] + 64));
    a.out_bytes = (uint8_t*)L.s_bytes.p;
    TK_HIP(c, tk_launch_decode_stream_write(a, s));
    TK_HIP(c, hipStreamSynchronize(s));
    *n_bytes = head[0];
    return TK_OK;
}

extern "C" int tk_decode_stream_step_device(tk_ctx* c, void* d_state, const void* d_ids, const void* d_id_offsets, uint64_t n_seqs,
                                            uint64_t n_ids, int policy, int flags, void* hip_stream, void** d_bytes,
                                            void** d_out_offsets, uint64_t* n_bytes, uint64_t* bad_seq) {
    TK_ENTRY(c);
    if (!d_id_offsets || (!d_state && n_seqs) || (!d_ids && n_ids) || !d_bytes || !d_out_offsets || !n_bytes) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    TK_HIP(c, hipSetDevice(c->device));
    int rc = run_stream_step(c, (uint32_t*)d_state, (const uint32_t*)d_ids, (const uint64_t*)d_id_offsets, n_seqs, policy, flags,
                             (hipStream_t)hip_stream, n_bytes, bad_seq);
    if (rc != TK_OK) return rc;
    *d_bytes = c->lossy.s_bytes.p;
    *d_out_offsets = c->lossy.s_offs.p;
    return TK_OK;
}

extern "C" int tk_decode_stream_step(tk_ctx* c, uint32_t* state, const uint32_t* ids, const uint64_t* id_offsets, uint64_t n_seqs,
                                     int policy, int flags, tk_text_result* out, uint64_t* bad_seq) {
    TK_ENTRY(c);
    if (!id_offsets || !out || (!state && n_seqs) || (!ids && id_offsets[n_seqs])) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    memset(out, 0, sizeof(*out));
    int rc = check_offsets(c, id_offsets, n_seqs);
    if (rc != TK_OK) return rc;
    TK_HIP(c, hipSetDevice(c->device));
    DecodeLossyBufs& L = c->lossy;
    const uint64_t n_ids = id_offsets[n_seqs];
    TK_HIP(c, L.s_in_ids.reserve((n_ids + 1) * 4));
    TK_HIP(c, L.s_in_offs.reserve((n_seqs + 1) * 8));
    TK_HIP(c, L.s_state.reserve((n_seqs + 1) * 4));
    if (n_ids) TK_HIP(c, hipMemcpyAsync(L.s_in_ids.p, ids, n_ids * 4, hipMemcpyHostToDevice, c->stream));
    TK_HIP(c, hipMemcpyAsync(L.s_in_offs.p, id_offsets, (n_seqs + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (n_seqs) TK_HIP(c, hipMemcpyAsync(L.s_state.p, state, n_seqs * 4, hipMemcpyHostToDevice, c->stream));
    uint64_t n_bytes = 0;
    rc = run_stream_step(c, (uint32_t*)L.s_state.p, (const uint32_t*)L.s_in_ids.p, (const uint64_t*)L.s_in_offs.p, n_seqs, policy, flags,
                         c->stream, &n_bytes, bad_seq);
    if (rc != TK_OK) return rc;
    CopyOut h[3] = {{L.s_bytes.p, n_bytes, nullptr}, {L.s_offs.p, (n_seqs + 1) * 8, nullptr}, {L.s_state.p, n_seqs * 4, nullptr}};
    if ((rc = copy_out(c, h, 3, "result")) != TK_OK) return rc;
    if (n_seqs) memcpy(state, h[2].host, n_seqs * 4);
    tk_pinned_put(h[2].host);
    out->bytes = (uint8_t*)h[0].host;
    out->offsets = (uint64_t*)h[1].host;
    out->n_bytes = n_bytes;
    out->n_docs = n_seqs;
    return TK_OK;
}

extern "C" void tk_last_decode_lossy_ms(const tk_ctx* c, float* strict_ms, float* repair_ms) {
    std::unique_lock<std::mutex> lock;
    if (c) lock = std::unique_lock<std::mutex>(const_cast<tk_ctx*>(c)->mu);   // (a call on another thread writes them under it)
    if (strict_ms) *strict_ms = c ? c->lossy.strict_ms : 0.f;
    if (repair_ms) *repair_ms = c ? c->lossy.repair_ms : 0.f;
}

extern "C" void tk_last_decode_lossy_stats(const tk_ctx* c, uint64_t* n_replaced, uint64_t* n_bad_docs, uint64_t* n_repair_launches) {
    std::unique_lock<std::mutex> lock;
    if (c) lock = std::unique_lock<std::mutex>(const_cast<tk_ctx*>(c)->mu);
    if (n_replaced) *n_replaced = c ? c->lossy.n_replaced : 0;
    if (n_bad_docs) *n_bad_docs = c ? c->lossy.n_bad_docs : 0;
    if (n_repair_launches) *n_repair_launches = c ? c->lossy.repair_launches : 0;
}
