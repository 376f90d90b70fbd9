// tk_capi_decode.cpp -- the decode entries of the C ABI (include/tekken_hip.h; csrc/tk_decode.hip): ids -> text with the
// reference's special-token policies and its errors (reference src/tekkenizer.rs:463-560).
#include "tk_ctx.h"

// The decode kernels' tables, built at the first decode or spans call on the context: by rank, the token's bytes and length in
// ONE 16-byte entry (tokens of up to 15 bytes), and the length alone in a byte
int token_tables(tk_ctx* c) {
    if (c->t_inline.p) return TK_OK;
    const TkHostTables& h = c->host;
    std::vector<uint8_t> inl((size_t)h.n_ranks * 16 + 16, 0), l8((size_t)h.n_ranks + 16, 0);
    for (uint32_t r = 0; r < h.n_ranks; ++r) {
        const uint32_t len = h.offs[r + 1] - h.offs[r];
        l8[r] = (uint8_t)(len < 255u ? len : 255u);
        if (len <= 15u) {
            memcpy(&inl[(size_t)r * 16], h.blob.data() + h.offs[r], len);
            inl[(size_t)r * 16 + 15] = (uint8_t)len;
        } else {
            inl[(size_t)r * 16 + 15] = 0xFFu;
        }
    }
    const int rc = upload(c, c->t_inline, inl.data(), inl.size());
    return rc != TK_OK ? rc : upload(c, c->t_len8, l8.data(), l8.size());
}

int run_decode(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t n_ids, int policy,
               hipStream_t s, uint64_t* n_bytes, uint64_t* bad_doc, uint64_t* utf8_bad) {
    if (policy < TK_POLICY_IGNORE || policy > TK_POLICY_RAISE) { c->err = "invalid policy"; return TK_ERR_INVALID_ARG; }
    if (policy == TK_POLICY_KEEP && !c->have_specials) { c->err = "TK_POLICY_KEEP needs tk_ctx_set_special_tokens first"; return TK_ERR_INVALID_ARG; }
    TK_HIP(c, c->dec_lens.reserve((n_docs + 1) * 4));
    TK_HIP(c, c->dec_offs.reserve((n_docs + 1) * 8));
    TK_HIP(c, c->dec_err.reserve(64));
    TK_HIP(c, c->dec_hi.reserve((n_docs + 1) * 4));
    TK_HIP(c, c->block_sums.reserve((n_docs / 2048 + 4) * 8));
    int rct = token_tables(c);
    if (rct != TK_OK) return rct;
    TkDecodeArgs a;
    memset(&a, 0, sizeof(a));
    a.ids = d_ids;
    a.id_offs = d_id_offs;
    a.n_ids = n_ids;
    a.n_docs = n_docs;
    a.lens = (uint32_t*)c->dec_lens.p;
    a.out_offs = (uint64_t*)c->dec_offs.p;
    a.err = (unsigned long long*)c->dec_err.p;
    a.doc_hi = (uint32_t*)c->dec_hi.p;
    token_args(c, a);
    a.sp_blob = (const uint8_t*)c->t_spblob.p;
    a.sp_offs = (const uint32_t*)c->t_spoffs.p;
    a.policy = policy;
    // Lengths by GROUPS of 16 documents (tk_decode_grouplen_kernel): the emit kernel only needs to know where a group's text begins
    // and writes the documents' offsets itself.  A group whose text reaches 4 GiB (err[3]) sends the call through the per-document
    // length pass instead.
    const uint64_t n_groups = (n_docs + TK_DECODE_GROUP_DOCS - 1) / TK_DECODE_GROUP_DOCS;
    TK_HIP(c, c->dec_glens.reserve((n_groups + 1) * 4));
    TK_HIP(c, c->dec_goffs.reserve((n_groups + 2) * 8));
    a.glens = (uint32_t*)c->dec_glens.p;
    a.group_limit = c->knobs.decode_group_limit;
    TK_HIP(c, hipMemsetAsync(c->dec_err.p, 0xFF, 32, s));
    TK_HIP(c, hipEventRecord(c->ev[0], s));
    uint64_t total = 0;
    unsigned long long err[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    const bool by_groups = !c->knobs.no_decode_groups;
    if (by_groups) {
        TK_HIP(c, tk_launch_decode_grouplen(a, s));
        TK_HIP(c, tk_launch_scan(a.glens, n_groups, (uint64_t*)c->dec_goffs.p, (uint64_t*)c->block_sums.p, s));
        TK_HIP(c, hipMemcpyAsync(&total, (uint64_t*)c->dec_goffs.p + n_groups, 8, hipMemcpyDeviceToHost, s));
        TK_HIP(c, hipMemcpyAsync(err, c->dec_err.p, 32, hipMemcpyDeviceToHost, s));
        TK_HIP(c, hipStreamSynchronize(s));
        if (n_docs == 0) total = 0;
    }
    if (by_groups && err[3] == ~0ull) {
        a.goffs = (const uint64_t*)c->dec_goffs.p;
    } else {
        TK_HIP(c, tk_launch_decode_doclen(a, s));
        TK_HIP(c, tk_launch_scan(a.lens, n_docs, (uint64_t*)c->dec_offs.p, (uint64_t*)c->block_sums.p, s));
        TK_HIP(c, hipMemcpyAsync(&total, (uint64_t*)c->dec_offs.p + n_docs, 8, hipMemcpyDeviceToHost, s));
        TK_HIP(c, hipMemcpyAsync(err, c->dec_err.p, 16, hipMemcpyDeviceToHost, s));
        TK_HIP(c, hipStreamSynchronize(s));
    }
    TK_HIP(c, c->dec_bytes.reserve(total + 64));
    TK_HIP(c, c->dec_bits.reserve((total / 32 + 4) * 4));
    a.out_bytes = (uint8_t*)c->dec_bytes.p;
    a.run_bits = (uint32_t*)c->dec_bits.p;
    TK_HIP(c, hipMemsetAsync(c->dec_bits.p, 0, (total / 32 + 4) * 4, s));
    if (n_docs == 0) TK_HIP(c, hipMemsetAsync(c->dec_offs.p, 0, 8, s));   // (no group writes the offsets' one entry: the total, 0)
    TK_HIP(c, tk_launch_decode_emit(a, s));
    TK_HIP(c, tk_launch_decode_validate(a, s));
    TK_HIP(c, hipEventRecord(c->ev[2], s));
    TK_HIP(c, hipMemcpyAsync(err, c->dec_err.p, 24, hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&c->pipeline_ms, c->ev[0], c->ev[2]);
    c->encode_ms = 0.f;
    if (utf8_bad) {                // the lossy entries: an invalid run is theirs to repair
        *utf8_bad = err[2];
        err[2] = ~0ull;
    }
    if (err[0] != ~0ull || err[1] != ~0ull || err[2] != ~0ull) {
        // Some document makes the reference return Err.  The GPU found WHICH documents; the class of the
        // error of the first one is decided by walking that single document's groups in the reference's
        // order (src/tekkenizer.rs:463-560) -- error classification only, no result is computed here.
        uint64_t first = err[2];
        for (int k = 0; k < 2; ++k) {
            if (err[k] == ~0ull) continue;
            uint64_t d = 0;
            int rc = doc_of_id(c, d_id_offs, n_docs, err[k], &d);
            if (rc != TK_OK) return rc;
            if (d < first) first = d;
        }
        if (bad_doc) *bad_doc = first;
        uint64_t range[2] = {0, 0};
        TK_HIP(c, hipMemcpy(range, d_id_offs + first, 16, hipMemcpyDeviceToHost));
        std::vector<uint32_t> hid((size_t)(range[1] - range[0]));
        if (!hid.empty()) TK_HIP(c, hipMemcpy(hid.data(), d_ids + range[0], hid.size() * 4, hipMemcpyDeviceToHost));
        const TkHostTables& h = c->host;
        size_t g0 = 0;
        while (g0 < hid.size()) {
            const bool sp = hid[g0] < h.num_special;
            size_t g1 = g0 + 1;
            while (g1 < hid.size() && (hid[g1] < h.num_special) == sp) ++g1;
            if (sp) {
                if (policy == TK_POLICY_RAISE) {
                    c->err = "Decoding tokens that contain special tokens is not allowed (document " + std::to_string(first) + ")";
                    return TK_ERR_SPECIAL_POLICY;
                }
            } else {
                std::string run;
                for (size_t k = g0; k < g1; ++k) {
                    const uint32_t r = hid[k] - h.num_special;
                    if (r >= h.n_ranks) {
                        c->err = "DecodeKeyError: invalid token for decoding: " + std::to_string(r) + " (document " + std::to_string(first) + ")";
                        return TK_ERR_RUNTIME;
                    }
                    run.append((const char*)h.blob.data() + h.offs[r], h.offs[r + 1] - h.offs[r]);
                }
                if (!utf8_bad && !tekken::utf8_valid((const uint8_t*)run.data(), run.size())) {
                    c->err = "FromUtf8Error: invalid utf-8 sequence (document " + std::to_string(first) + ")";
                    return TK_ERR_RUNTIME;
                }
            }
            g0 = g1;
        }
        c->err = "decode: device flagged document " + std::to_string(first) + " but the host walk found no error";
        return TK_ERR_RUNTIME;
    }
    *n_bytes = total;
    return TK_OK;
}

extern "C" int tk_decode_batch_device(tk_ctx* c, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                                      int policy, void* hip_stream, void** d_bytes, void** d_out_offsets, uint64_t* n_bytes,
                                      uint64_t* bad_doc) {
    TK_ENTRY(c);
    if (!d_id_offsets || (!d_ids && n_ids) || !d_bytes || !d_out_offsets || !n_bytes) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    TK_HIP(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;  // NULL = HIP's null stream: ordered after the caller's own work on it
    int rc = run_decode(c, (const uint32_t*)d_ids, (const uint64_t*)d_id_offsets, n_docs, n_ids, policy, s, n_bytes, bad_doc);
    if (rc != TK_OK) return rc;
    *d_bytes = c->dec_bytes.p;
    *d_out_offsets = c->dec_offs.p;
    return TK_OK;
}

extern "C" int tk_decode_batch(tk_ctx* c, const uint32_t* ids, const uint64_t* id_offsets, uint64_t n_docs, int policy,
                               tk_text_result* out, uint64_t* bad_doc) {
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
    rc = run_decode(c, (const uint32_t*)c->dec_in_ids.p, (const uint64_t*)c->dec_in_offs.p, n_docs, n_ids, policy, c->stream,
                    &n_bytes, bad_doc);
    if (rc != TK_OK) return rc;
    CopyOut h[2] = {{c->dec_bytes.p, n_bytes, nullptr}, {c->dec_offs.p, (n_docs + 1) * 8, nullptr}};
    if ((rc = copy_out(c, h, 2, "result")) != TK_OK) return rc;
    out->bytes = (uint8_t*)h[0].host;
    out->offsets = (uint64_t*)h[1].host;
    out->n_bytes = n_bytes;
    out->n_docs = n_docs;
    return TK_OK;
}

extern "C" void tk_free_text_result(tk_text_result* r) {
    if (!r) return;
    tk_pinned_put(r->bytes);
    tk_pinned_put(r->offsets);
    memset(r, 0, sizeof(*r));
}
