// tk_capi_specials.cpp -- special-token strings parsed out of text (include/tekken_hip.h tk_specials_split_device and the entries
// around it; csrc/tk_specials.hip): packed text in; the text without the matched strings, cut into parts, and the part tables that
// tk_encode_parts_device_join takes out.  The composite entries run text -> parts -> encode -> join.
#include <map>

#include "tk_capi_layout.h"

#define TK_SPECIALS_ALL_FLAGS (TK_SPECIALS_BOS | TK_SPECIALS_EOS | TK_SPECIALS_PART_SRC)

// The byte trie over the context's strings, built once behind tk_ctx_set_special_tokens: a string that is empty or longer than
// TKS_MAXLEN is left out (str_of = TKS_NONE: an error only where a call puts it into its match set).  The modes are not in it:
// a terminal names its distinct string, and the per-call eff words say which id, if any, that string stands for.
static int specials_trie(tk_ctx* c) {
    SpecialsBufs& b = c->specials;
    if (b.trie_ready) return TK_OK;
    const uint32_t n = (uint32_t)(b.h_offs.empty() ? 0 : b.h_offs.size() - 1);
    std::map<uint32_t, uint32_t> edge;                  // node << 8 | byte -> child
    std::vector<uint32_t> term(1, TKS_NONE);
    b.str_of.assign(n, TKS_NONE);
    b.n_distinct = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t o = b.h_offs[i], len = b.h_offs[i + 1] - o;
        if (len == 0 || len > TKS_MAXLEN) continue;
        uint32_t node = 0;
        for (uint32_t k = 0; k < len; ++k) {
            const uint32_t key = node << 8 | b.h_blob[o + k];
            auto it = edge.find(key);
            if (it == edge.end()) {
                it = edge.emplace(key, (uint32_t)term.size()).first;
                term.push_back(TKS_NONE);
            }
            node = it->second;
        }
        if (term[node] == TKS_NONE) term[node] = b.n_distinct++;
        b.str_of[i] = term[node];
    }
    if (term.size() >= (1u << 24)) { c->err = "special token strings: too many bytes for the trie"; return TK_ERR_INVALID_ARG; }
    uint32_t size = 16;
    while (size < 2 * edge.size()) size <<= 1;          // at most half full: an empty entry ends every probe
    std::vector<uint64_t> table(size, 0);
    for (const auto& e : edge) {
        uint32_t slot = tks_edge_slot(e.first, size - 1);
        while (table[slot]) slot = (slot + 1) & (size - 1);
        table[slot] = (uint64_t)(e.first + 1u) << 32 | e.second;
    }
    int rc;
    if ((rc = upload(c, b.edges, table.data(), table.size() * 8)) || (rc = upload(c, b.term, term.data(), term.size() * 4))) return rc;
    b.edge_mask = size - 1;
    b.trie_ready = true;
    return TK_OK;
}

// Step 1 of the definition: what is refused before any work.  On TK_OK the eff words and the first-byte mask of this call's match
// set are in c->specials.h_eff / first, and *any says whether the set has a string at all.
static int specials_check_opts(tk_ctx* c, const tk_specials_opts* o, uint32_t first[8], bool* any) {
    if (!o) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    if (o->flags & ~(uint32_t)TK_SPECIALS_ALL_FLAGS) { c->err = "unknown specials flag"; return TK_ERR_INVALID_ARG; }
    if (!c->have_specials) { c->err = "the specials pass needs tk_ctx_set_special_tokens first"; return TK_ERR_INVALID_ARG; }
    const uint32_t n = c->host.num_special;
    if (n >= (1u << 23)) { c->err = "specials: 2^23 special tokens or more"; return TK_ERR_INVALID_ARG; }   // (a candidate's id and length share a word)
    if (o->modes && o->n_modes != n) {
        c->err = "specials: n_modes is " + std::to_string(o->n_modes) + ", num_special_tokens " + std::to_string(n);
        return TK_ERR_INVALID_ARG;
    }
    for (uint32_t i = 0; o->modes && i < n; ++i)
        if (o->modes[i] > TK_SPECIAL_RAISE) { c->err = "specials: unknown mode " + std::to_string(o->modes[i]) + " of id " + std::to_string(i); return TK_ERR_INVALID_ARG; }
    SpecialsBufs& b = c->specials;
    for (uint32_t i = 0; i < n; ++i) {                  // (known without the trie: a refused call builds nothing)
        const uint32_t len = b.h_offs[i + 1] - b.h_offs[i];
        if ((!o->modes || o->modes[i] != TK_SPECIAL_TEXT) && (len == 0 || len > TKS_MAXLEN)) {
            c->err = "specials: the string of id " + std::to_string(i) + " has " + std::to_string(len) + " bytes (1 .. " + std::to_string(TKS_MAXLEN) + " can be matched)";
            return TK_ERR_INVALID_ARG;
        }
    }
    TK_HIP(c, hipSetDevice(c->device));
    int rc = specials_trie(c);
    if (rc != TK_OK) return rc;
    b.h_eff.assign(b.n_distinct ? b.n_distinct : 1, TKS_NONE);
    memset(first, 0, 32);
    *any = false;
    for (uint32_t i = 0; i < n; ++i) {                  // (ascending: the lower id stands for equal strings)
        const uint32_t m = o->modes ? o->modes[i] : TK_SPECIAL_PARSE;
        if (m == TK_SPECIAL_TEXT) continue;
        uint32_t& e = b.h_eff[b.str_of[i]];
        if (e != TKS_NONE) continue;
        e = i | (m == TK_SPECIAL_RAISE ? TKS_RAISE : 0u);
        const uint8_t f = b.h_blob[b.h_offs[i]];
        first[f >> 5] |= 1u << (f & 31);
        *any = true;
    }
    return TK_OK;
}

// step 3: the message of a RAISE match, from the candidate the mark kernel reported
static int specials_raise(tk_ctx* c, const TkSpecialsArgs& a, uint64_t cand, uint64_t* bad) {
    uint64_t pos = 0, start = 0;
    uint32_t id = 0, doc = 0;
    TK_HIP(c, hipMemcpy(&pos, a.cpos + cand, 8, hipMemcpyDeviceToHost));
    TK_HIP(c, hipMemcpy(&id, a.cid + cand, 4, hipMemcpyDeviceToHost));
    TK_HIP(c, hipMemcpy(&doc, a.cdoc + cand, 4, hipMemcpyDeviceToHost));
    TK_HIP(c, hipMemcpy(&start, a.doc_offs + doc, 8, hipMemcpyDeviceToHost));
    if (bad) *bad = doc;
    c->err = "document " + std::to_string(doc) + ", byte " + std::to_string(pos - start) + ": the string of special token id " +
             std::to_string(id & ~TKS_RAISE) + " is not allowed in text (TK_SPECIAL_RAISE)";
    return TK_ERR_SPECIAL_POLICY;
}

// The specials pass over text on the device into the context's c->specials buffers; *out gets the device pointers.  The candidates,
// the chain and the marks go to work buffers; TWO reads (the number of candidates; M, n_removed and the RAISE word) size what
// follows, and only once the call is accepted is anything of an earlier result touched.  One wait ends the call.  The caller
// holds c->mu.
static int run_specials(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes, int checks,
                        const tk_specials_opts* o, hipStream_t s, tk_specials* out, uint64_t* bad) {
    uint32_t first[8];
    bool any = false;
    int rc = specials_check_opts(c, o, first, &any);
    if (rc != TK_OK) return rc;
    if ((rc = check_n_docs(c, n_docs)) != TK_OK) return rc;
    if (checks && (rc = check_text_device(c, d_bytes, d_doc_offsets, n_docs, n_bytes, checks, s)) != TK_OK) return rc;
    SpecialsBufs& b = c->specials;
    const uint64_t D = n_docs;
    const bool want_src = (o->flags & TK_SPECIALS_PART_SRC) != 0;
    b.ms[0] = b.ms[1] = b.ms[2] = b.ms[3] = 0.f;
    for (Event& ev : b.ev)
        if (!ev.h) TK_HIP(c, hipEventCreate(&ev.h));
    TkSpecialsArgs a;
    memset(&a, 0, sizeof(a));
    a.bytes = (const uint8_t*)d_bytes;
    a.doc_offs = (const uint64_t*)d_doc_offsets;
    a.n_docs = D;
    a.n_bytes = n_bytes;
    a.bos = (o->flags & TK_SPECIALS_BOS) ? c->host.bos_id : TK_JOIN_NONE;
    a.eos = c->host.eos_id;
    a.eos_part = (o->flags & TK_SPECIALS_EOS) ? 1u : 0u;
    memcpy(a.first, first, 32);
    uint64_t NC = 0, M = 0, removed = 0;
    bool counted = false, chained = false;
    if (any && n_bytes) {
        a.n_tiles = (n_bytes + TKS_TILE - 1) / TKS_TILE;
        TK_HIP(c, b.stat.reserve(256));
        TK_HIP(c, b.eff.reserve(b.h_eff.size() * 4));
        TK_HIP(c, b.tcnt.reserve(a.n_tiles * 4 + 16));
        TK_HIP(c, b.tpos.reserve((a.n_tiles + 1) * 8));
        TK_HIP(c, b.bsum.reserve(scan_workspace_bytes(a.n_tiles)));
        a.edges = (const uint64_t*)b.edges.p;
        a.edge_mask = b.edge_mask;
        a.term = (const uint32_t*)b.term.p;
        a.eff = (const uint32_t*)b.eff.p;
        a.tile_cnt = (uint32_t*)b.tcnt.p;
        a.tile_pos = (const uint64_t*)b.tpos.p;
        a.stat = (unsigned long long*)b.stat.p;
        // (h_eff belongs to the context: it outlives the copy, which the wait below ends)
        TK_HIP(c, hipMemcpyAsync(b.eff.p, b.h_eff.data(), b.h_eff.size() * 4, hipMemcpyHostToDevice, s));
        TK_HIP(c, hipMemsetAsync(a.stat, 0, 128, s));
        TK_HIP(c, hipMemsetAsync(a.stat + 1, 0xFF, 8, s));
        TK_HIP(c, hipEventRecord(b.ev[0], s));
        TK_HIP(c, tk_launch_specials_cand(a, 0, s));
        if ((rc = scan_u32(c, b.bsum, a.tile_cnt, a.n_tiles, (uint64_t*)b.tpos.p, s)) != TK_OK) return rc;
        TK_HIP(c, tk_launch_specials_count_end(a, s));
        TK_HIP(c, hipEventRecord(b.ev[1], s));
        unsigned long long nc = 0;
        TK_HIP(c, hipMemcpyAsync(&nc, a.stat, 8, hipMemcpyDeviceToHost, s));
        TK_HIP(c, hipStreamSynchronize(s));
        counted = true;
        NC = nc;
        if (NC >= 0xFFFFFFF0ull) { c->err = "specials: " + std::to_string(NC) + " candidates in one batch (the chain holds fewer than 2^32 - 16)"; return TK_ERR_INVALID_ARG; }
    }
    if (NC) {
        TK_HIP(c, b.cpos.reserve((NC + 1) * 8));
        TK_HIP(c, b.clen.reserve(NC * 4 + 16));
        TK_HIP(c, b.cid.reserve(NC * 4 + 16));
        TK_HIP(c, b.cdoc.reserve(NC * 4 + 16));
        TK_HIP(c, b.ja.reserve((NC + 1) * 8));
        TK_HIP(c, b.jb.reserve((NC + 1) * 8));
        TK_HIP(c, b.row.reserve((NC + 1) * 4 + 16));
        TK_HIP(c, b.open.reserve((NC + 2) * 8));
        TK_HIP(c, b.flen.reserve(NC * 4 + 16));
        TK_HIP(c, b.remc.reserve((NC + 1) * 8));
        TK_HIP(c, b.bsum.reserve(scan_workspace_bytes(NC)));
        a.n_cand = NC;
        a.cpos = (uint64_t*)b.cpos.p;
        a.clen = (uint32_t*)b.clen.p;
        a.cid = (uint32_t*)b.cid.p;
        a.cdoc = (uint32_t*)b.cdoc.p;
        a.jump = (uint64_t*)b.ja.p;
        a.row = (uint32_t*)b.row.p;
        a.open = (const uint64_t*)b.open.p;
        a.flen = (uint32_t*)b.flen.p;
        a.remc = (const uint64_t*)b.remc.p;
        TkRowfitArgs ch;                                // the chain, as the doubling rounds of the rowfit pass take it: a match is a row
        memset(&ch, 0, sizeof(ch));
        ch.n_docs = NC;
        ch.jump_a = a.jump;
        ch.jump_b = (uint64_t*)b.jb.p;
        ch.row = a.row;
        ch.open = (uint64_t*)b.open.p;
        ch.E = ch.id_offs = a.cpos;
        ch.stat = a.stat + 8;
        uint32_t rounds = 0;                            // (a match holds a candidate: at most NC links)
        while ((1ull << rounds) <= NC) ++rounds;
        TK_HIP(c, hipEventRecord(b.ev[2], s));
        TK_HIP(c, tk_launch_specials_cand(a, 1, s));
        TK_HIP(c, hipEventRecord(b.ev[3], s));
        TK_HIP(c, tk_launch_specials_nxt(a, s));
        TK_HIP(c, tk_launch_chain_rounds(ch, rounds, s));
        TK_HIP(c, tk_launch_specials_mark(a, s));
        if ((rc = scan_u32(c, b.bsum, a.flen, NC, (uint64_t*)b.remc.p, s)) != TK_OK) return rc;
        TK_HIP(c, hipEventRecord(b.ev[4], s));
        unsigned long long got[3] = {0, 0, 0};          // M, the first RAISE match, n_removed
        TK_HIP(c, hipMemcpyAsync(got, a.stat + 11, 8, hipMemcpyDeviceToHost, s));
        TK_HIP(c, hipMemcpyAsync(got + 1, a.stat + 1, 8, hipMemcpyDeviceToHost, s));
        TK_HIP(c, hipMemcpyAsync(got + 2, a.remc + NC, 8, hipMemcpyDeviceToHost, s));
        TK_HIP(c, hipStreamSynchronize(s));
        chained = true;
        if (got[1] != ~0ull) return specials_raise(c, a, got[1], bad);
        M = got[0];
        removed = got[2];
        if (M > NC || removed > n_bytes) { c->err = "specials: the chain did not report"; return TK_ERR_RUNTIME; }
    }
    // ---- accepted: the outputs
    const uint64_t per = 1u + a.eos_part, P = D * per + M, n_out = n_bytes - removed;
    TK_HIP(c, b.poffs.reserve((P + 1) * 8));
    TK_HIP(c, b.ctrl.reserve(P * 4 + 16));
    TK_HIP(c, b.conv.reserve((D + 1) * 8));
    if (want_src) TK_HIP(c, b.psrc.reserve(P * 8 + 16));
    if (M) {
        TK_HIP(c, b.mpos.reserve(M * 8 + 16));
        TK_HIP(c, b.sout.reserve((M + 1) * 8));
        TK_HIP(c, b.ssrc.reserve((M + 1) * 8));
        TK_HIP(c, b.bytes.reserve(n_out + 16));
    }
    a.n_matches = M;
    a.n_removed = removed;
    a.mpos = (uint64_t*)b.mpos.p;
    a.seg_out = (uint64_t*)b.sout.p;
    a.seg_src = (uint64_t*)b.ssrc.p;
    a.out_bytes = (uint8_t*)b.bytes.p;
    a.part_offs = (uint64_t*)b.poffs.p;
    a.part_ctrl = (uint32_t*)b.ctrl.p;
    a.conv_offs = (uint64_t*)b.conv.p;
    a.part_src = want_src ? (uint64_t*)b.psrc.p : nullptr;
    TK_HIP(c, hipEventRecord(b.ev[5], s));
    if (M) TK_HIP(c, tk_launch_specials_matches(a, s));
    TK_HIP(c, tk_launch_specials_docs(a, s));
    TK_HIP(c, hipEventRecord(b.ev[6], s));
    if (M) TK_HIP(c, tk_launch_specials_compact(a, s));
    TK_HIP(c, hipEventRecord(b.ev[7], s));
    TK_HIP(c, hipStreamSynchronize(s));
    float ms = 0.f;
    if (counted) (void)hipEventElapsedTime(&b.ms[0], b.ev[0], b.ev[1]);
    if (chained) {
        (void)hipEventElapsedTime(&ms, b.ev[2], b.ev[3]);
        b.ms[0] += ms;
        (void)hipEventElapsedTime(&b.ms[1], b.ev[3], b.ev[4]);
    }
    (void)hipEventElapsedTime(&b.ms[2], b.ev[5], b.ev[6]);
    (void)hipEventElapsedTime(&b.ms[3], b.ev[6], b.ev[7]);
    out->bytes = M ? (uint8_t*)b.bytes.p : (uint8_t*)d_bytes;   // (no match: the caller's own text, not copied)
    out->part_offsets = (uint64_t*)b.poffs.p;
    out->part_ctrl = (uint32_t*)b.ctrl.p;
    out->conv_offsets = (uint64_t*)b.conv.p;
    out->part_src = want_src ? (uint64_t*)b.psrc.p : nullptr;
    out->n_docs = D;
    out->n_parts = P;
    out->n_bytes = n_out;
    out->n_matches = M;
    out->n_removed = removed;
    return TK_OK;
}

extern "C" int tk_specials_split_device(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                        int checks, const tk_specials_opts* opts, void* hip_stream, tk_specials* out, uint64_t* bad) {
    TK_ENTRY(c);
    int rc = check_flags_and_args(c, checks, TK_CHECK_OFFSETS | TK_CHECK_UTF8, !d_doc_offsets || (!d_bytes && n_bytes) || !opts || !out);
    if (rc != TK_OK) return rc;
    return run_specials(c, d_bytes, d_doc_offsets, n_docs, n_bytes, checks, opts, (hipStream_t)hip_stream, out, bad);
}

// (the body of tk_encode_batch_device_parsed; the caller holds c->mu.  parts: optional)
static int encode_device_parsed(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes, int checks,
                                const tk_specials_opts* opts, const tk_join_opts* jopts, void* hip_stream, tk_specials* parts, tk_join* out,
                                uint64_t* bad) {
    int rc = check_flags_and_args(c, checks, TK_CHECK_OFFSETS | TK_CHECK_UTF8, !d_doc_offsets || (!d_bytes && n_bytes) || !opts || !jopts || !out);
    if (rc != TK_OK) return rc;
    // (the join's options are refused before the text is split, the number of parts before it is encoded)
    if ((rc = join_check_args(c, 0, n_docs, jopts)) != TK_OK) return rc;
    tk_specials sp;
    if ((rc = run_specials(c, d_bytes, d_doc_offsets, n_docs, n_bytes, checks, opts, (hipStream_t)hip_stream, &sp, bad)) != TK_OK) return rc;
    if (parts) *parts = sp;
    return encode_parts_device_join(c, sp.bytes, sp.part_offsets, sp.n_parts, sp.n_bytes, sp.part_ctrl, nullptr, sp.conv_offsets, n_docs, 0,
                                    jopts, hip_stream, out);
}

extern "C" int tk_encode_batch_device_parsed(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                             int checks, const tk_specials_opts* opts, const tk_join_opts* jopts, void* hip_stream,
                                             tk_specials* parts, tk_join* out, uint64_t* bad) {
    TK_ENTRY(c);
    return encode_device_parsed(c, d_bytes, d_doc_offsets, n_docs, n_bytes, checks, opts, jopts, hip_stream, parts, out, bad);
}

extern "C" int tk_encode_batch_parsed(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int validate_utf8,
                                      const tk_specials_opts* opts, const tk_join_opts* jopts, tk_specials* parts, tk_join* out, uint64_t* bad) {
    TK_ENTRY(c);
    if (!opts || !jopts || !out || !doc_offsets || (!bytes && doc_offsets[n_docs])) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    memset(out, 0, sizeof(*out));
    if (parts) memset(parts, 0, sizeof(*parts));
    int rc = check_n_docs(c, n_docs);
    if (rc != TK_OK || (rc = check_offsets(c, doc_offsets, n_docs)) != TK_OK) return rc;
    TK_HIP(c, hipSetDevice(c->device));
    SpecialsBufs& b = c->specials;
    const uint64_t n_bytes = doc_offsets[n_docs];
    TK_HIP(c, b.in_bytes.reserve(n_bytes + 64));
    TK_HIP(c, b.in_offs.reserve((n_docs + 1) * 8));
    if (n_bytes) TK_HIP(c, hipMemcpyAsync(b.in_bytes.p, bytes, n_bytes, hipMemcpyHostToDevice, c->stream));
    TK_HIP(c, hipMemcpyAsync(b.in_offs.p, doc_offsets, (n_docs + 1) * 8, hipMemcpyHostToDevice, c->stream));
    tk_specials sp;
    tk_join j;
    rc = encode_device_parsed(c, b.in_bytes.p, b.in_offs.p, n_docs, n_bytes, validate_utf8 ? TK_CHECK_UTF8 : 0, opts, jopts, c->stream, &sp, &j, bad);
    if (rc != TK_OK) { (void)hipStreamSynchronize(c->stream); return rc; }   // (the copies of the caller's arrays have ended when the call returns)
    if ((rc = layout_copy_out(c, j, 4, n_docs, "join", out)) != TK_OK) return rc;
    if (parts && (rc = layout_copy_out(c, sp, 1, n_docs, "specials", parts)) != TK_OK) { layout_free(out); return rc; }
    return TK_OK;
}

// One document through the same kernels (here and not in tekkenizer.cpp: the host-only builds of that file have no engine entries)
extern "C" int tk_tokenizer_encode_parsed(tk_tokenizer* t, const char* text, size_t len, int add_bos, int add_eos, const uint8_t* modes,
                                          uint32_t n_modes, uint32_t** ids, size_t* n_ids) {
    if (!t || !ids || !n_ids || (!text && len)) return TK_ERR_INVALID_ARG;
    tk_ctx* c = tk_tokenizer_ctx(t);
    if (!c) return tk_tokenizer_fail(t, TK_ERR_NO_DEVICE, "tokenizer was created without a device (host-only object)");
    const uint64_t offs[2] = {0, (uint64_t)len};
    const tk_specials_opts o = {modes, n_modes, (add_bos ? TK_SPECIALS_BOS : 0u) | (add_eos ? TK_SPECIALS_EOS : 0u)};
    const tk_join_opts jo = {0, 0};
    tk_join j;
    const int rc = tk_encode_batch_parsed(c, (const uint8_t*)(text ? text : ""), offs, 1, 0, &o, &jo, nullptr, &j, nullptr);
    if (rc != TK_OK) return tk_tokenizer_fail(t, rc, tk_last_error(c));
    *ids = (uint32_t*)malloc((j.n_ids ? j.n_ids : 1) * sizeof(uint32_t));
    if (!*ids) { tk_free_join(&j); return tk_tokenizer_fail(t, TK_ERR_RUNTIME, "out of memory"); }
    memcpy(*ids, j.ids, j.n_ids * sizeof(uint32_t));
    *n_ids = j.n_ids;
    tk_free_join(&j);
    return TK_OK;
}

extern "C" void tk_free_specials(tk_specials* r) { layout_free(r); }

extern "C" void tk_last_specials_ms(const tk_ctx* c, float ms[4]) {
    std::unique_lock<std::mutex> lock;
    if (c) lock = std::unique_lock<std::mutex>(const_cast<tk_ctx*>(c)->mu);   // (a call on another thread writes them under it)
    for (int i = 0; ms && i < 4; ++i) ms[i] = c ? c->specials.ms[i] : 0.f;
}

extern "C" uint32_t tk_specials_tile(void) { return TKS_TILE; }
