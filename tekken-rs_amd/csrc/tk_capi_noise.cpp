// tk_capi_noise.cpp -- masked-LM and span-corruption rows (include/tekken_hip.h tk_noise_replace_device / tk_noise_spans_device and
// the entries around them; csrc/tk_noise.hip): a hash-drawn or caller-given choice of tokens, words or spans of every document,
// and the ids with the chosen ones masked (replace mode) or every chosen run behind a sentinel (spans mode).  The composite entries
// run encode -> words (word unit) -> noise.
#include "tk_capi_layout.h"

#define TKN_STAT_BYTES ((TKN_STAT_DROP + 1u) * 8u)   /* TkNoiseArgs.stat */
#define TK_NOISE_ALL_FLAGS (TK_NOISE_SELECTED | TK_NOISE_DESC | TK_NOISE_SPLIT | TK_NOISE_JOINED)

// step 5 of the definition: what is refused before any launch.  have_words: word ids are given, or will be made (the composites)
static int noise_check_opts(tk_ctx* c, const tk_noise_opts* o, bool spans, bool have_words, bool have_sel, uint64_t n_docs) {
    if (!o) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    const uint64_t one = 1ull << 32, S0 = c->host.num_special, V = S0 + c->host.n_ranks;
    if (o->flags & ~(uint32_t)TK_NOISE_ALL_FLAGS) { c->err = "unknown noise flag"; return TK_ERR_INVALID_ARG; }
    if (o->unit != TK_NOISE_UNIT_TOKEN && o->unit != TK_NOISE_UNIT_WORD) { c->err = "unknown noise unit"; return TK_ERR_INVALID_ARG; }
    if (o->span_min < 1 || o->span_min > o->span_max || o->span_max > TK_NOISE_SPAN_LIMIT) {
        c->err = "noise: 1 <= span_min <= span_max <= " + std::to_string(TK_NOISE_SPAN_LIMIT) + " does not hold";
        return TK_ERR_INVALID_ARG;
    }
    if (o->start_q32 > one || o->mask_q32 > one || o->random_q32 > one || o->mask_q32 + o->random_q32 > one) {
        c->err = "noise: a rate above 2^32 (or mask_q32 + random_q32 above it)";
        return TK_ERR_INVALID_ARG;
    }
    if (o->unit == TK_NOISE_UNIT_WORD && !have_words && !have_sel) { c->err = "noise: TK_NOISE_UNIT_WORD needs word_ids"; return TK_ERR_INVALID_ARG; }
    if (!spans) {
        if (o->mask_id >= V) { c->err = "noise: mask_id " + std::to_string(o->mask_id) + " is outside the vocabulary"; return TK_ERR_INVALID_ARG; }
    } else {
        if (!(o->flags & (TK_NOISE_SPLIT | TK_NOISE_JOINED))) { c->err = "noise: neither TK_NOISE_SPLIT nor TK_NOISE_JOINED"; return TK_ERR_INVALID_ARG; }
        if (o->final_id != TK_JOIN_NONE && o->final_id >= S0) {
            c->err = "noise: final_id " + std::to_string(o->final_id) + " is neither TK_JOIN_NONE nor below num_special_tokens (" + std::to_string(S0) + ")";
            return TK_ERR_INVALID_ARG;
        }
        // the sentinels the options can produce: first .. first + n - 1, or first - (n - 1) .. first
        const uint64_t n = o->n_sentinels, first = o->sentinel_first;
        const bool ok = n == 0 || ((o->flags & TK_NOISE_DESC) ? first < S0 && n - 1 <= first : first + n - 1 < S0);
        if (!ok) { c->err = "noise: a sentinel of the options is not below num_special_tokens (" + std::to_string(S0) + ")"; return TK_ERR_INVALID_ARG; }
    }
    return check_n_docs(c, n_docs);
}

// what the kernels take of the options
static void noise_args(const tk_ctx* c, const void* d_ids, const void* d_offs, uint64_t n_docs, uint64_t n_ids, const void* d_word_ids,
                       const void* d_sel, const tk_noise_opts* o, TkNoiseArgs* a) {
    memset(a, 0, sizeof(*a));
    a->ids = (const uint32_t*)d_ids;
    a->offs = (const uint64_t*)d_offs;
    a->word_ids = (const uint32_t*)d_word_ids;
    a->sel = (const uint8_t*)d_sel;
    a->n_docs = n_docs;
    a->n_ids = n_ids;
    for (uint32_t k = 0; k < 4; ++k) a->s[k] = tki_hash(o->seed, TKN_SEED_BASE + k);
    a->start_q32 = o->start_q32;
    a->mask_q32 = o->mask_q32;
    a->mask_random_q32 = o->mask_q32 + o->random_q32;
    a->unit = o->unit; a->span_min = o->span_min; a->span_max = o->span_max;
    a->mask_id = o->mask_id;
    a->num_special = c->host.num_special;
    a->n_ordinary = c->host.n_ranks;
    a->ignore = o->ignore_index;
    a->n_sentinels = o->n_sentinels; a->sentinel_first = o->sentinel_first; a->final_id = o->final_id;
    a->desc = (o->flags & TK_NOISE_DESC) != 0;
    a->split = (o->flags & TK_NOISE_SPLIT) != 0;
    a->joined = (o->flags & TK_NOISE_JOINED) != 0;
    a->n_tiles = (n_ids + TKN_TILE - 1) / TKN_TILE;
}

// A document of `limit` ids or more is refused.  Fewer ids than that in all: no document can have them, and nothing is asked of
// the device; else one small kernel (the dense pass's longest document) and one wait.
static int noise_check_longest(tk_ctx* c, const uint64_t* d_offs, uint64_t n_docs, uint64_t n_ids, uint64_t limit, hipStream_t s) {
    if (n_ids < limit || n_docs == 0) return TK_OK;
    NoiseBufs& b = c->noise;
    unsigned long long longest = 0;
    TK_HIP(c, b.stat.reserve(TKN_STAT_BYTES));
    TK_HIP(c, hipMemsetAsync(b.stat.p, 0, 8, s));
    TK_HIP(c, tk_launch_dense_maxlen(d_offs, n_docs, (unsigned long long*)b.stat.p, s));
    TK_HIP(c, hipMemcpyAsync(&longest, b.stat.p, 8, hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipStreamSynchronize(s));
    if (longest >= limit) { c->err = "noise: a document of " + std::to_string(longest) + " ids (the limit is " + std::to_string(limit) + ")"; return TK_ERR_INVALID_ARG; }
    return TK_OK;
}

// the counters of a call from the copies the blocks added to (TkNoiseArgs.stat)
static void noise_sum(const unsigned long long* slots, unsigned long long* got) {
    for (uint32_t k = 0; k < TKN_STATS; ++k) got[k] = 0;
    for (uint32_t i = 0; i < TKN_SLOTS * TKN_STATS; ++i) got[i % TKN_STATS] += slots[i];
}

static int noise_events(tk_ctx* c) {
    NoiseBufs& b = c->noise;
    for (float& m : b.ms) m = 0.f;
    for (Event& ev : b.ev)
        if (!ev.h) TK_HIP(c, hipEventCreate(&ev.h));
    return TK_OK;
}

// Replace mode over ids on the device into the context's c->noise buffers.  Everything that can be refused has been refused by the
// caller (noise_check_opts); ONE kernel, ONE wait at the end, which fetches the three counters.  The caller holds c->mu.
static int run_noise_replace(tk_ctx* c, const void* d_ids, const void* d_offs, uint64_t n_docs, uint64_t n_ids, const void* d_word_ids,
                             const void* d_sel, const tk_noise_opts* o, hipStream_t s, tk_noise_replace* out) {
    NoiseBufs& b = c->noise;
    int rc = noise_check_longest(c, (const uint64_t*)d_offs, n_docs, n_ids, 0xFFFFFFFFull, s);
    if (rc != TK_OK || (rc = noise_events(c)) != TK_OK) return rc;
    const bool want_sel = (o->flags & TK_NOISE_SELECTED) != 0;
    TK_HIP(c, b.stat.reserve(TKN_STAT_BYTES));
    TK_HIP(c, b.ids.reserve(n_ids * 4 + 16));
    TK_HIP(c, b.lab.reserve(n_ids * 4 + 16));
    if (want_sel) TK_HIP(c, b.sel.reserve(n_ids + 16));
    TkNoiseArgs a;
    noise_args(c, d_ids, d_offs, n_docs, n_ids, d_word_ids, d_sel, o, &a);
    a.out_ids = (uint32_t*)b.ids.p;
    a.labels = (int32_t*)b.lab.p;
    a.selected = want_sel ? (uint8_t*)b.sel.p : nullptr;
    a.stat = (unsigned long long*)b.stat.p;
    unsigned long long slots[TKN_STAT_DROP + 1], got[TKN_STATS];   // n_selected, n_masked, n_random
    TK_HIP(c, hipMemsetAsync(a.stat, 0, TKN_STAT_BYTES, s));
    TK_HIP(c, hipEventRecord(b.ev[0], s));
    TK_HIP(c, tk_launch_noise_replace(a, s));
    TK_HIP(c, hipEventRecord(b.ev[1], s));
    TK_HIP(c, hipMemcpyAsync(slots, a.stat, TKN_STAT_BYTES, hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipStreamSynchronize(s));
    noise_sum(slots, got);
    (void)hipEventElapsedTime(&b.ms[0], b.ev[0], b.ev[1]);
    out->input_ids = a.out_ids;
    out->labels = a.labels;
    out->selected = a.selected;
    out->n_docs = n_docs;
    out->n_ids = n_ids;
    out->n_selected = got[0];
    out->n_masked = got[1];
    out->n_random = got[2];
    return TK_OK;
}

// Spans mode.  Two waits: the sizes of the outputs and the counters behind the document scans, the end of the call.
static int run_noise_spans(tk_ctx* c, const void* d_ids, const void* d_offs, uint64_t n_docs, uint64_t n_ids, const void* d_word_ids,
                           const void* d_sel, const tk_noise_opts* o, hipStream_t s, tk_noise_spans* out) {
    NoiseBufs& b = c->noise;
    const uint64_t D = n_docs;
    int rc = noise_check_longest(c, (const uint64_t*)d_offs, D, n_ids, 0xFFFFFFFFull - 1u - o->n_sentinels, s);
    if (rc != TK_OK || (rc = noise_events(c)) != TK_OK) return rc;
    TkNoiseArgs a;
    noise_args(c, d_ids, d_offs, D, n_ids, d_word_ids, d_sel, o, &a);
    const uint64_t T = a.n_tiles;
    TK_HIP(c, b.stat.reserve(TKN_STAT_BYTES));
    TK_HIP(c, b.sel.reserve(n_ids + 16));
    TK_HIP(c, b.tsel.reserve(T * 4 + 16));
    TK_HIP(c, b.trs.reserve(T * 4 + 16));
    TK_HIP(c, b.tS.reserve((T + 1) * 8));
    TK_HIP(c, b.tR.reserve((T + 1) * 8));
    TK_HIP(c, b.dsel0.reserve(D * 4 + 16));
    TK_HIP(c, b.drs0.reserve(D * 4 + 16));
    TK_HIP(c, b.SB.reserve((D + 1) * 8));
    TK_HIP(c, b.RB.reserve((D + 1) * 8));
    TK_HIP(c, b.KS.reserve(D * 4 + 16));
    TK_HIP(c, b.in_len.reserve(D * 4 + 16));
    TK_HIP(c, b.tg_len.reserve(D * 4 + 16));
    TK_HIP(c, b.in_off.reserve((D + 1) * 8));
    TK_HIP(c, b.tg_off.reserve((D + 1) * 8));
    TK_HIP(c, b.bsum.reserve(scan_workspace_bytes(D > T ? D : T)));
    a.selected = (uint8_t*)b.sel.p;
    a.tile_sel = (uint32_t*)b.tsel.p; a.tile_rs = (uint32_t*)b.trs.p;
    a.tile_S = (const uint64_t*)b.tS.p; a.tile_R = (const uint64_t*)b.tR.p;
    a.doc_sel0 = (uint32_t*)b.dsel0.p; a.doc_rs0 = (uint32_t*)b.drs0.p;
    a.SB = (uint64_t*)b.SB.p; a.RB = (uint64_t*)b.RB.p; a.KS = (uint32_t*)b.KS.p;
    a.in_len = (uint32_t*)b.in_len.p; a.tg_len = (uint32_t*)b.tg_len.p;
    a.in_off = (const uint64_t*)b.in_off.p; a.tg_off = (const uint64_t*)b.tg_off.p;
    a.stat = (unsigned long long*)b.stat.p;
    unsigned long long slots[TKN_STAT_DROP + 1], got[TKN_STATS];   // n_selected, n_runs, n_runs_dropped
    uint64_t n_in = 0, n_tg = 0;
    TK_HIP(c, hipMemsetAsync(a.stat, 0, TKN_STAT_BYTES, s));
    if (D) {
        TK_HIP(c, hipMemsetAsync(a.doc_sel0, 0, D * 4, s));
        TK_HIP(c, hipMemsetAsync(a.doc_rs0, 0, D * 4, s));
    }
    TK_HIP(c, hipEventRecord(b.ev[0], s));
    TK_HIP(c, tk_launch_noise_select(a, s));
    TK_HIP(c, hipEventRecord(b.ev[1], s));
    if (D == 0 || n_ids == 0) {                         // (no tile was counted: nothing is selected)
        TK_HIP(c, hipMemsetAsync(b.tS.p, 0, (T + 1) * 8, s));
        TK_HIP(c, hipMemsetAsync(b.tR.p, 0, (T + 1) * 8, s));
    } else {
        TK_HIP(c, tk_launch_noise_count(a, s));
        if ((rc = scan_u32(c, b.bsum, a.tile_sel, T, (uint64_t*)b.tS.p, s)) != TK_OK) return rc;
        if ((rc = scan_u32(c, b.bsum, a.tile_rs, T, (uint64_t*)b.tR.p, s)) != TK_OK) return rc;
    }
    TK_HIP(c, tk_launch_noise_docs(a, s));
    TK_HIP(c, tk_launch_noise_drop(a, s));
    TK_HIP(c, tk_launch_noise_lens(a, s));
    if ((rc = scan_u32(c, b.bsum, a.in_len, D, (uint64_t*)b.in_off.p, s)) != TK_OK) return rc;
    if ((rc = scan_u32(c, b.bsum, a.tg_len, D, (uint64_t*)b.tg_off.p, s)) != TK_OK) return rc;
    TK_HIP(c, hipEventRecord(b.ev[2], s));
    TK_HIP(c, hipMemcpyAsync(slots, a.stat, TKN_STAT_BYTES, hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipMemcpyAsync(&n_in, a.in_off + D, 8, hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipMemcpyAsync(&n_tg, a.tg_off + D, 8, hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipStreamSynchronize(s));
    noise_sum(slots, got);
    // what a well-formed batch can give: anything else is offsets that mean nothing, and no buffer is sized by it
    const uint64_t most = n_ids + 2u * (uint64_t)o->n_sentinels * D + D;
    if (n_in > n_ids + (uint64_t)o->n_sentinels * D || n_in + n_tg > most) { c->err = "noise: id_offsets are not well-formed"; return TK_ERR_INVALID_ARG; }
    a.n_inputs = n_in;
    a.n_targets = n_tg;
    if (a.split) {
        TK_HIP(c, b.inputs.reserve(n_in * 4 + 16));
        TK_HIP(c, b.targets.reserve(n_tg * 4 + 16));
        a.inputs = (uint32_t*)b.inputs.p;
        a.targets = (uint32_t*)b.targets.p;
    }
    if (a.joined) {
        TK_HIP(c, b.joined.reserve((n_in + n_tg) * 4 + 16));
        TK_HIP(c, b.jlab.reserve((n_in + n_tg) * 4 + 16));
        TK_HIP(c, b.joffs.reserve((D + 1) * 8));
        a.joined_ids = (uint32_t*)b.joined.p;
        a.joined_labels = (int32_t*)b.jlab.p;
        a.joined_offs = (uint64_t*)b.joffs.p;
    }
    TK_HIP(c, tk_launch_noise_fill(a, s));
    TK_HIP(c, hipEventRecord(b.ev[3], s));
    TK_HIP(c, hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&b.ms[0], b.ev[0], b.ev[1]);
    (void)hipEventElapsedTime(&b.ms[1], b.ev[1], b.ev[2]);
    (void)hipEventElapsedTime(&b.ms[2], b.ev[2], b.ev[3]);
    out->inputs = a.inputs;
    out->input_offsets = a.split ? (uint64_t*)b.in_off.p : nullptr;
    out->targets = a.targets;
    out->target_offsets = a.split ? (uint64_t*)b.tg_off.p : nullptr;
    out->joined = a.joined_ids;
    out->joined_offsets = a.joined_offs;
    out->joined_labels = a.joined_labels;
    out->n_docs = D;
    out->n_selected = got[0];
    out->n_runs = got[1];
    out->n_runs_dropped = got[2];
    out->n_inputs = n_in;
    out->n_targets = n_tg;
    return TK_OK;
}

// ---- the entries, written once for the two modes ----
struct NoiseReplace {
    typedef tk_noise_replace Result;
    static constexpr bool spans = false;
    static constexpr const char* name = "noise_replace";
    static int run(tk_ctx* c, const void* ids, const void* offs, uint64_t D, uint64_t N, const void* w, const void* sel, const tk_noise_opts* o,
                   hipStream_t s, Result* out) { return run_noise_replace(c, ids, offs, D, N, w, sel, o, s, out); }
};
struct NoiseSpans {
    typedef tk_noise_spans Result;
    static constexpr bool spans = true;
    static constexpr const char* name = "noise_spans";
    static int run(tk_ctx* c, const void* ids, const void* offs, uint64_t D, uint64_t N, const void* w, const void* sel, const tk_noise_opts* o,
                   hipStream_t s, Result* out) { return run_noise_spans(c, ids, offs, D, N, w, sel, o, s, out); }
};

template <class P>
static int noise_from_ids(tk_ctx* c, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids, const void* d_word_ids,
                          const void* d_sel, const tk_noise_opts* opts, void* hip_stream, typename P::Result* out) {
    TK_ENTRY(c);
    if (!d_id_offsets || (!d_ids && n_ids) || !opts || !out) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    int rc = noise_check_opts(c, opts, P::spans, d_word_ids != nullptr, d_sel != nullptr, n_docs);
    if (rc != TK_OK) return rc;
    TK_HIP(c, hipSetDevice(c->device));
    return P::run(c, d_ids, d_id_offsets, n_docs, n_ids, d_word_ids, d_sel, opts, (hipStream_t)hip_stream, out);
}

// the words pass (word unit only) and the noise pass behind an encode on s; the caller holds c->mu
template <class P>
static int noise_encoded(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t n_ids, const uint8_t* d_bytes,
                         const uint64_t* d_doc_offs, uint64_t n_bytes, const tk_noise_opts* o, hipStream_t s, typename P::Result* out) {
    const void* words = nullptr;
    if (o->unit == TK_NOISE_UNIT_WORD) {
        const tk_words_opts wo = {0u};
        tk_words w;
        const int rc = run_words(c, d_ids, d_id_offs, n_docs, n_ids, d_bytes, d_doc_offs, n_bytes, 0, &wo, s, &w, nullptr);
        if (rc != TK_OK) return rc;
        words = w.word_ids;
    }
    return P::run(c, d_ids, d_id_offs, n_docs, n_ids, words, nullptr, o, s, out);
}

template <class P>
static int noise_encode_device(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes, int add_bos,
                               int add_eos, int checks, const tk_noise_opts* opts, void* hip_stream, void** d_ids, void** d_out_offsets,
                               uint64_t* n_ids, typename P::Result* out) {
    TK_ENTRY(c);
    int rc = check_flags_and_args(c, checks, TK_CHECK_OFFSETS | TK_CHECK_UTF8, !opts || !out);
    if (rc != TK_OK || (rc = noise_check_opts(c, opts, P::spans, true, false, n_docs)) != TK_OK) return rc;
    rc = encode_device_checked(c, d_bytes, d_doc_offsets, n_docs, n_bytes, add_bos, add_eos, checks, hip_stream, d_ids, d_out_offsets, n_ids);
    if (rc != TK_OK) return rc;
    return noise_encoded<P>(c, (const uint32_t*)*d_ids, (const uint64_t*)*d_out_offsets, n_docs, *n_ids, (const uint8_t*)d_bytes,
                            (const uint64_t*)d_doc_offsets, n_bytes, opts, (hipStream_t)hip_stream, out);
}

template <class P>
static int noise_encode_host(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos, int add_eos,
                             int validate_utf8, const tk_noise_opts* opts, tk_result* ids_out, typename P::Result* out) {
    TK_ENTRY(c);
    if (!opts || !out || !ids_out) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    memset(out, 0, sizeof(*out));
    int rc = noise_check_opts(c, opts, P::spans, true, false, n_docs);
    if (rc != TK_OK) return rc;
    DevBatch dev;
    if ((rc = encode_batch(c, bytes, doc_offsets, n_docs, add_bos, add_eos, validate_utf8, ids_out, &dev)) != TK_OK) return rc;
    const uint64_t n_bytes = doc_offsets[n_docs];
    auto fail = [&](int code) { tk_free_result(ids_out); return code; };
    if (opts->unit == TK_NOISE_UNIT_WORD && dev.bytes == (const uint8_t*)c->ds_in) {
        // (the one-launch small path read the text from mapped pinned memory: the words pass's split launch gets a copy on the
        // device, as in tk_encode_batch_words)
        NoiseBufs& b = c->noise;
        hipError_t e = b.text.reserve(n_bytes + 64);
        if (e == hipSuccess) e = b.toffs.reserve((n_docs + 1) * 8);
        if (e == hipSuccess && n_bytes) e = hipMemcpyAsync(b.text.p, bytes, n_bytes, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(b.toffs.p, doc_offsets, (n_docs + 1) * 8, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) { c->err = std::string("noise: staging the text failed: ") + hipGetErrorString(e); return fail(TK_ERR_RUNTIME); }
        dev.bytes = (const uint8_t*)b.text.p;
        dev.doc_offs = (const uint64_t*)b.toffs.p;
    }
    typename P::Result r;
    if ((rc = noise_encoded<P>(c, dev.ids, dev.id_offs, n_docs, ids_out->n_ids, dev.bytes, dev.doc_offs, n_bytes, opts, c->stream, &r)) != TK_OK)
        return fail(rc);
    if ((rc = layout_copy_out(c, r, 4, n_docs, P::name, out)) != TK_OK) return fail(rc);
    return TK_OK;
}

extern "C" int tk_noise_replace_device(tk_ctx* c, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                                       const void* d_word_ids, const void* d_sel, const tk_noise_opts* opts, void* hip_stream,
                                       tk_noise_replace* out) {
    return noise_from_ids<NoiseReplace>(c, d_ids, d_id_offsets, n_docs, n_ids, d_word_ids, d_sel, opts, hip_stream, out);
}
extern "C" int tk_noise_spans_device(tk_ctx* c, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                                     const void* d_word_ids, const void* d_sel, const tk_noise_opts* opts, void* hip_stream, tk_noise_spans* out) {
    return noise_from_ids<NoiseSpans>(c, d_ids, d_id_offsets, n_docs, n_ids, d_word_ids, d_sel, opts, hip_stream, out);
}
extern "C" int tk_encode_batch_device_noise_replace(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                                    int add_bos, int add_eos, int checks, const tk_noise_opts* opts, void* hip_stream,
                                                    void** d_ids, void** d_out_offsets, uint64_t* n_ids, tk_noise_replace* out) {
    return noise_encode_device<NoiseReplace>(c, d_bytes, d_doc_offsets, n_docs, n_bytes, add_bos, add_eos, checks, opts, hip_stream, d_ids,
                                             d_out_offsets, n_ids, out);
}
extern "C" int tk_encode_batch_device_noise_spans(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                                  int add_bos, int add_eos, int checks, const tk_noise_opts* opts, void* hip_stream, void** d_ids,
                                                  void** d_out_offsets, uint64_t* n_ids, tk_noise_spans* out) {
    return noise_encode_device<NoiseSpans>(c, d_bytes, d_doc_offsets, n_docs, n_bytes, add_bos, add_eos, checks, opts, hip_stream, d_ids,
                                           d_out_offsets, n_ids, out);
}
extern "C" int tk_encode_batch_noise_replace(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos,
                                             int add_eos, int validate_utf8, const tk_noise_opts* opts, tk_result* ids_out, tk_noise_replace* out) {
    return noise_encode_host<NoiseReplace>(c, bytes, doc_offsets, n_docs, add_bos, add_eos, validate_utf8, opts, ids_out, out);
}
extern "C" int tk_encode_batch_noise_spans(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos,
                                           int add_eos, int validate_utf8, const tk_noise_opts* opts, tk_result* ids_out, tk_noise_spans* out) {
    return noise_encode_host<NoiseSpans>(c, bytes, doc_offsets, n_docs, add_bos, add_eos, validate_utf8, opts, ids_out, out);
}

extern "C" void tk_free_noise_replace(tk_noise_replace* r) { layout_free(r); }
extern "C" void tk_free_noise_spans(tk_noise_spans* r) { layout_free(r); }

extern "C" void tk_last_noise_ms(const tk_ctx* c, float ms[3]) {
    std::unique_lock<std::mutex> lock;
    if (c) lock = std::unique_lock<std::mutex>(const_cast<tk_ctx*>(c)->mu);   // (a call on another thread writes them under it)
    for (int i = 0; ms && i < 3; ++i) ms[i] = c ? c->noise.ms[i] : 0.f;
}

extern "C" uint32_t tk_noise_tile(void) { return TKN_TILE; }
