// tk_capi_words.cpp -- word ids (include/tekken_hip.h tk_words_from_ids_device and the entries around it; csrc/tk_words.hip):
// the pre-tokenization piece every id came from.  The three entries are this pass's own (they take the text, as join's do);
// tk_free_words and the host copy-out are made from the one description of tk_words in tk_capi_layout.h.
#include "tk_capi_layout.h"

// The piece-start flags of text on the device into c->words.flags, on s.  The hard-coded pattern: the split-only launch of the
// per-document encode kernel, as tk_split_batch makes it -- it overwrites encode's temporaries (staging, counts, defer_list, the
// work counters) and none of its outputs; documents with malformed UTF-8 are split again behind it.  The JSON pattern: the pass's own kernel over the sequential matcher (the split-only
// instantiation knows the hard-coded pattern alone).
static int split_flags(tk_ctx* c, const uint8_t* d_bytes, const uint64_t* d_doc_offs, uint64_t n_docs, uint64_t n_bytes, hipStream_t s) {
    WordsBufs& b = c->words;
    TK_HIP(c, hipMemsetAsync(b.flags.p, 0, n_bytes + 64, s));
    if (n_docs == 0 || n_bytes == 0) return TK_OK;
    if (c->pattern == 1) {
        TK_HIP(c, tk_launch_words_split_json(c->dview, d_bytes, d_doc_offs, n_docs, (uint8_t*)b.flags.p, s));
        return TK_OK;
    }
    TK_HIP(c, c->staging.reserve((n_bytes + 2 * n_docs + 64) * 4));
    TK_HIP(c, c->counts.reserve((n_docs + 1) * 4));
    TK_HIP(c, c->defer_list.reserve((n_docs + 1) * 4));
    TkEncodeArgs a = encode_args(c, d_bytes, d_doc_offs, n_docs, 0, 0);
    a.dbg_starts = (uint8_t*)b.flags.p;
    a.split_only = 1;
    TK_HIP(c, hipMemsetAsync(c->ctr(TKC_WORK), 0, TKC_CLEARED * 4, s));
    const uint64_t want = (n_docs + 7) / 8;
    TK_HIP(c, tk_launch_encode(a, 2, (uint32_t)(want < 8192 ? (want ? want : 1) : 8192), s));
    // (the windows of that kernel and the sequential matcher part on malformed UTF-8: such documents are split again)
    TK_HIP(c, tk_launch_words_resplit(c->dview, d_bytes, d_doc_offs, n_docs, (uint8_t*)b.flags.p, s));
    return TK_OK;
}

// The words pass over ids and text on the device (the caller holds c->mu; checks: TK_WORDS_CHECK_ALIGNED or 0; the flags of o
// are known).  Two host waits: the error words and n_words behind the scan, the end of the call.
int run_words(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t n_ids, const uint8_t* d_bytes,
              const uint64_t* d_doc_offs, uint64_t n_bytes, int checks, const tk_words_opts* o, hipStream_t s, tk_words* out, uint64_t* bad) {
    WordsBufs& b = c->words;
    for (float& m : b.ms) m = 0.f;
    int rc = token_tables(c);
    if (rc != TK_OK) return rc;
    const bool want_first = (o->flags & TK_WORDS_FIRST) != 0;
    TK_HIP(c, b.ids.reserve(n_ids * 4 + 16));
    TK_HIP(c, b.dw.reserve((n_docs + 1) * 8));
    TK_HIP(c, b.cnt.reserve(n_docs * 4 + 16));
    TK_HIP(c, b.flags.reserve(n_bytes + 64));
    TK_HIP(c, b.bsum.reserve(scan_workspace_bytes(n_docs)));
    TK_HIP(c, b.err.reserve(64));
    for (Event& ev : b.ev)
        if (!ev.h) TK_HIP(c, hipEventCreate(&ev.h));
    uint64_t n_words = 0;
    if (n_docs == 0) {
        TK_HIP(c, hipMemsetAsync(b.dw.p, 0, 8, s));
    } else {
        TkWordsArgs a;
        memset(&a, 0, sizeof(a));
        a.ids = d_ids;
        a.id_offs = d_id_offs;
        a.n_docs = n_docs;
        a.doc_offs = d_doc_offs;
        a.flags = (const uint8_t*)b.flags.p;
        a.word_ids = (uint32_t*)b.ids.p;
        a.n_words = (uint32_t*)b.cnt.p;
        a.doc_words = (const uint64_t*)b.dw.p;
        a.err = (unsigned long long*)b.err.p;
        token_args(c, a);
        unsigned long long err[5] = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull};
        TK_HIP(c, hipMemsetAsync(b.err.p, 0xFF, 40, s));
        TK_HIP(c, hipEventRecord(b.ev[0], s));
        if ((rc = split_flags(c, d_bytes, d_doc_offs, n_docs, n_ids ? n_bytes : 0, s)) != TK_OK) return rc;
        TK_HIP(c, hipEventRecord(b.ev[1], s));
        TK_HIP(c, tk_launch_words(a, (checks & TK_WORDS_CHECK_ALIGNED) != 0, s));
        TK_HIP(c, hipEventRecord(b.ev[2], s));
        if ((rc = scan_u32(c, b.bsum, a.n_words, n_docs, (uint64_t*)b.dw.p, s)) != TK_OK) return rc;
        TK_HIP(c, hipEventRecord(b.ev[3], s));
        TK_HIP(c, hipMemcpyAsync(err, b.err.p, 40, hipMemcpyDeviceToHost, s));
        TK_HIP(c, hipMemcpyAsync(&n_words, (const uint64_t*)b.dw.p + n_docs, 8, hipMemcpyDeviceToHost, s));
        TK_HIP(c, hipStreamSynchronize(s));
        (void)hipEventElapsedTime(&b.ms[0], b.ev[0], b.ev[1]);
        (void)hipEventElapsedTime(&b.ms[1], b.ev[1], b.ev[2]);
        (void)hipEventElapsedTime(&b.ms[2], b.ev[2], b.ev[3]);
        // ---- error paths: name the first document that fails and say why
        if (err[4] != ~0ull) {
            if (bad) *bad = err[4];
            c->err = "words: document " + std::to_string(err[4]) + " reaches 2^32 bytes";
            return TK_ERR_INVALID_ARG;
        }
        for (int k = 2; k < 4; ++k) {
            if (err[k] == ~0ull) continue;
            uint64_t d = 0;
            if ((rc = doc_of_id(c, d_id_offs, n_docs, err[k], &d)) != TK_OK) return rc;
            if (bad) *bad = d;
            if (k == 3) { c->err = "words: document " + std::to_string(d) + " reaches 2^32 bytes (spans are uint32 offsets)"; return TK_ERR_INVALID_ARG; }
            uint32_t id = 0;
            TK_HIP(c, hipMemcpy(&id, d_ids + err[2], 4, hipMemcpyDefault));
            c->err = "words: id " + std::to_string(id) + " (document " + std::to_string(d) + ") is outside the vocabulary";
            return TK_ERR_RUNTIME;
        }
        if (err[0] != ~0ull || err[1] != ~0ull) {
            uint64_t first = err[0], d1 = ~0ull;
            if (err[1] != ~0ull) {
                if ((rc = doc_of_id(c, d_id_offs, n_docs, err[1], &d1)) != TK_OK) return rc;
                if (d1 < first) first = d1;
            }
            if (bad) *bad = first;
            uint64_t range[2] = {0, 0}, text[2] = {0, 0};
            TK_HIP(c, hipMemcpy(range, d_id_offs + first, 16, hipMemcpyDefault));
            TK_HIP(c, hipMemcpy(text, d_doc_offs + first, 16, hipMemcpyDefault));
            if (err[0] == first) {
                const TkHostTables& h = c->host;
                std::vector<uint32_t> hid((size_t)(range[1] - range[0]));
                if (!hid.empty()) TK_HIP(c, hipMemcpy(hid.data(), d_ids + range[0], hid.size() * 4, hipMemcpyDefault));
                uint64_t covered = 0;
                for (uint32_t id : hid)
                    if (id >= h.num_special) covered += h.offs[id - h.num_special + 1] - h.offs[id - h.num_special];
                c->err = "words: document " + std::to_string(first) + " is not aligned with its ids: the ids cover " + std::to_string(covered) +
                         " bytes, the document has " + std::to_string(text[1] - text[0]);
            } else {
                c->err = "words: in document " + std::to_string(first) + " a piece starts inside the span of id index " +
                         std::to_string(err[1] - range[0]);
            }
            return TK_ERR_RUNTIME;
        }
        if (want_first) {
            TK_HIP(c, b.first.reserve(n_words * 4 + 16));
            a.word_first = (uint32_t*)b.first.p;
            TK_HIP(c, hipEventRecord(b.ev[4], s));
            if (n_words) TK_HIP(c, tk_launch_words_first(a, s));
            TK_HIP(c, hipEventRecord(b.ev[5], s));
        }
    }
    if (want_first && n_docs == 0) TK_HIP(c, b.first.reserve(16));
    TK_HIP(c, hipStreamSynchronize(s));
    if (want_first && n_docs) (void)hipEventElapsedTime(&b.ms[3], b.ev[4], b.ev[5]);
    out->word_ids = (uint32_t*)b.ids.p;
    out->doc_words = (uint64_t*)b.dw.p;
    out->word_first = want_first ? (uint32_t*)b.first.p : nullptr;
    out->n_docs = n_docs;
    out->n_ids = n_ids;
    out->n_words = n_words;
    return TK_OK;
}

// how the three entries open: an unknown flag or check bit is refused first, then a null argument
static int words_open(tk_ctx* c, int checks, int known, const tk_words_opts* opts, bool null_arg) {
    if ((checks & ~known) || (opts && (opts->flags & ~TK_WORDS_FIRST))) { c->err = "unknown flag"; return TK_ERR_INVALID_ARG; }
    if (!opts || null_arg) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    return TK_OK;
}

extern "C" int tk_words_from_ids_device(tk_ctx* c, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                                        const void* d_bytes, const void* d_doc_offsets, uint64_t n_bytes, int checks,
                                        const tk_words_opts* opts, void* hip_stream, tk_words* out, uint64_t* bad) {
    TK_ENTRY(c);
    int rc = words_open(c, checks, TK_WORDS_CHECK_ALIGNED, opts,
                        !d_id_offsets || (!d_ids && n_ids) || !d_doc_offsets || (!d_bytes && n_bytes) || !out);
    if (rc != TK_OK) return rc;
    if ((rc = enter_device(c, n_docs)) != TK_OK) return rc;
    return run_words(c, (const uint32_t*)d_ids, (const uint64_t*)d_id_offsets, n_docs, n_ids, (const uint8_t*)d_bytes,
                     (const uint64_t*)d_doc_offsets, n_bytes, checks, opts, (hipStream_t)hip_stream, out, bad);
}

extern "C" int tk_encode_batch_device_words(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                            int add_bos, int add_eos, int checks, const tk_words_opts* opts, void* hip_stream,
                                            void** d_ids, void** d_out_offsets, uint64_t* n_ids, tk_words* out, uint64_t* bad) {
    TK_ENTRY(c);
    const int enc = TK_CHECK_OFFSETS | TK_CHECK_UTF8;
    int rc = words_open(c, checks, enc | TK_WORDS_CHECK_ALIGNED, opts, !out);
    if (rc != TK_OK) return rc;
    rc = encode_device_checked(c, d_bytes, d_doc_offsets, n_docs, n_bytes, add_bos, add_eos, checks & enc, hip_stream, d_ids, d_out_offsets, n_ids);
    if (rc != TK_OK) return rc;
    return run_words(c, (const uint32_t*)*d_ids, (const uint64_t*)*d_out_offsets, n_docs, *n_ids, (const uint8_t*)d_bytes,
                     (const uint64_t*)d_doc_offsets, n_bytes, checks & TK_WORDS_CHECK_ALIGNED, opts, (hipStream_t)hip_stream, out, bad);
}

extern "C" int tk_encode_batch_words(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos,
                                     int add_eos, int validate_utf8, int checks, const tk_words_opts* opts, tk_result* ids_out,
                                     tk_words* out, uint64_t* bad) {
    TK_ENTRY(c);
    int rc = words_open(c, checks, TK_WORDS_CHECK_ALIGNED, opts, !out);
    if (rc != TK_OK) return rc;
    memset(out, 0, sizeof(*out));
    DevBatch dev;
    if ((rc = encode_batch(c, bytes, doc_offsets, n_docs, add_bos, add_eos, validate_utf8, ids_out, &dev)) != TK_OK) return rc;
    const uint64_t n_bytes = doc_offsets[n_docs];
    auto fail = [&](int code) { tk_free_result(ids_out); return code; };
    if (dev.bytes == (const uint8_t*)c->ds_in) {
        // the one-launch small path read the text from mapped pinned memory: the split launch gets a copy on the device (the ids
        // and their offsets stay where they are: the words kernel reads them there, as the spans kernel does)
        WordsBufs& b = c->words;
        hipError_t e = b.text.reserve(n_bytes + 64);
        if (e == hipSuccess) e = b.toffs.reserve((n_docs + 1) * 8);
        if (e == hipSuccess && n_bytes) e = hipMemcpyAsync(b.text.p, bytes, n_bytes, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(b.toffs.p, doc_offsets, (n_docs + 1) * 8, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) { c->err = std::string("words: staging the text failed: ") + hipGetErrorString(e); return fail(TK_ERR_RUNTIME); }
        dev.bytes = (const uint8_t*)b.text.p;
        dev.doc_offs = (const uint64_t*)b.toffs.p;
    }
    tk_words r;
    if ((rc = run_words(c, dev.ids, dev.id_offs, n_docs, ids_out->n_ids, dev.bytes, dev.doc_offs, n_bytes, checks, opts, c->stream, &r, bad)) != TK_OK)
        return fail(rc);
    if ((rc = layout_copy_out(c, r, 4, n_docs, "words", out)) != TK_OK) return fail(rc);
    return TK_OK;
}

extern "C" void tk_free_words(tk_words* r) { layout_free(r); }

extern "C" void tk_last_words_ms(const tk_ctx* c, float ms[4]) {
    std::unique_lock<std::mutex> lock;
    if (c) lock = std::unique_lock<std::mutex>(const_cast<tk_ctx*>(c)->mu);   // (a call on another thread writes them under it)
    for (int i = 0; ms && i < 4; ++i) ms[i] = c ? c->words.ms[i] : 0.f;
}
