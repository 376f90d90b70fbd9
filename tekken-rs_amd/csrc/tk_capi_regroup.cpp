// tk_capi_regroup.cpp -- encoded documents selected, reordered and cut into batches (include/tekken_hip.h tk_regroup_from_ids_device
// and the entries around it; csrc/tk_regroup.hip): ragged ids in, ragged ids out, with the permutation and the batch boundaries.
#include "tk_capi_layout.h"

#define TK_REGROUP_ALL_FLAGS (TK_REGROUP_DESC | TK_REGROUP_LABELS | TK_REGROUP_PERM | TK_REGROUP_BATCHES | TK_REGROUP_BATCH_OFFSETS | TK_REGROUP_BATCH_ROWLEN)

// the options that can be refused before anything is enqueued (step 5 of the definition)
static int regroup_check_opts(tk_ctx* c, const tk_regroup_opts* o) {
    if (!o) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    if (o->order > TK_REGROUP_ORDER_GROUPED) { c->err = "unknown regroup order"; return TK_ERR_INVALID_ARG; }
    if (o->flags & ~(uint32_t)TK_REGROUP_ALL_FLAGS) { c->err = "unknown regroup flag"; return TK_ERR_INVALID_ARG; }
    if (o->order == TK_REGROUP_ORDER_GROUPED && o->window == 0) { c->err = "TK_REGROUP_ORDER_GROUPED needs a window"; return TK_ERR_INVALID_ARG; }
    if ((o->flags & TK_REGROUP_BATCHES) && o->max_tokens == 0) { c->err = "TK_REGROUP_BATCHES needs max_tokens"; return TK_ERR_INVALID_ARG; }
    if (o->max_length && o->min_length > o->max_length) {
        c->err = "min_length " + std::to_string(o->min_length) + " is beyond max_length " + std::to_string(o->max_length);
        return TK_ERR_INVALID_ARG;
    }
    return TK_OK;
}

// ... of the entries that encode text first: text has no labels stream, and that is refused before anything is encoded
static int regroup_encode_opts(tk_ctx* c, const tk_regroup_opts* opts, int, int, tk_regroup_opts* o) {
    *o = *opts;
    int rc = regroup_check_opts(c, o);
    if (rc == TK_OK && (o->flags & TK_REGROUP_LABELS)) { c->err = "TK_REGROUP_LABELS: encoded text has no labels stream"; rc = TK_ERR_INVALID_ARG; }
    return rc;
}

// 8-bit radix passes that a sort of keys up to `largest` needs: none above its highest set bit
static uint32_t radix_passes(uint64_t largest) {
    uint32_t n = 0;
    while (largest) { ++n; largest >>= 8; }
    return n;
}

// The regroup pass over ids on the device into the context's c->regroup buffers; *out gets the device pointers.  The selection
// goes to work buffers; ONE read (64 bytes: the drop counts, K, the kept ids, the longest kept document, where the offsets end)
// sizes the outputs, and only once it is accepted is anything of an earlier result touched.  One wait ends the call.  The
// caller holds c->mu.
static int run_regroup(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t n_ids, const int32_t* d_lab,
                       const uint8_t* d_keep, const tk_regroup_opts* o, hipStream_t s, tk_regroup* out) {
    int rc = regroup_check_opts(c, o);
    if (rc != TK_OK) return rc;
    if ((rc = check_n_docs(c, n_docs)) != TK_OK) return rc;
    if (n_docs == 0 && n_ids) { c->err = "regroup: ids without a document"; return TK_ERR_INVALID_ARG; }
    const uint64_t D = n_docs;
    const bool want_lab = (o->flags & TK_REGROUP_LABELS) != 0, want_perm = (o->flags & TK_REGROUP_PERM) != 0,
               batches = (o->flags & TK_REGROUP_BATCHES) != 0, want_bo = batches && (o->flags & TK_REGROUP_BATCH_OFFSETS),
               want_brl = batches && (o->flags & TK_REGROUP_BATCH_ROWLEN);
    if (want_lab && !d_lab && n_ids) { c->err = "TK_REGROUP_LABELS needs a labels buffer"; return TK_ERR_INVALID_ARG; }
    RegroupBufs& b = c->regroup;
    unsigned long long stat[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    b.ms[0] = b.ms[1] = b.ms[2] = b.ms[3] = 0.f;
    uint64_t K = 0, n_out = 0;
    bool staged = false;
    if (D) {
        TK_HIP(c, b.stat.reserve(256));
        TK_HIP(c, b.flag.reserve(D * 4 + 16));
        TK_HIP(c, b.fpos.reserve((D + 1) * 8));
        TK_HIP(c, b.kept.reserve(D * 4 + 16));
        TK_HIP(c, b.bsum.reserve(scan_workspace_bytes(D)));
        TkRegroupArgs a;
        memset(&a, 0, sizeof(a));
        a.ids = d_ids;
        a.lab = want_lab ? d_lab : nullptr;
        a.id_offs = d_id_offs;
        a.keep = d_keep;
        a.n_docs = D;
        a.max_tokens = o->max_tokens;
        a.min_len = o->min_length;
        a.max_len = o->max_length;
        a.order = o->order;
        a.seed = o->seed;
        a.window = o->window;
        a.max_docs = o->max_docs;
        a.desc = (o->flags & TK_REGROUP_DESC) != 0;
        a.flag = (uint32_t*)b.flag.p;
        a.fpos = (const uint64_t*)b.fpos.p;
        a.kept = (uint32_t*)b.kept.p;
        a.stat = (unsigned long long*)b.stat.p;
        for (Event& ev : b.ev)
            if (!ev.h) TK_HIP(c, hipEventCreate(&ev.h));
        TK_HIP(c, hipMemsetAsync(a.stat, 0, 128, s));
        TK_HIP(c, hipEventRecord(b.ev[0], s));
        TK_HIP(c, tk_launch_regroup_select(a, s));
        if ((rc = scan_u32(c, b.bsum, a.flag, D, (uint64_t*)b.fpos.p, s)) != TK_OK) return rc;
        TK_HIP(c, tk_launch_regroup_compact(a, s));
        TK_HIP(c, hipEventRecord(b.ev[1], s));
        TK_HIP(c, hipMemcpyAsync(stat, a.stat, 64, hipMemcpyDeviceToHost, s));
        TK_HIP(c, hipStreamSynchronize(s));
        (void)hipEventElapsedTime(&b.ms[0], b.ev[0], b.ev[1]);
        if (stat[5] != n_ids) {
            c->err = "regroup: id_offsets end at " + std::to_string(stat[5]) + ", not at n_ids = " + std::to_string(n_ids);
            return TK_ERR_INVALID_ARG;
        }
        if (stat[7]) { c->err = "regroup: " + std::to_string(stat[7]) + " documents of 2^32 ids or more (or decreasing id_offsets)"; return TK_ERR_INVALID_ARG; }
        K = stat[4];
        n_out = stat[3];
        a.n_kept = K;
        a.n_out = n_out;
        a.longest = (uint32_t)stat[6];
        // ---- accepted: the outputs
        TK_HIP(c, b.ids.reserve(n_out * 4 + 16));
        if (want_lab) TK_HIP(c, b.lab.reserve(n_out * 4 + 16));
        TK_HIP(c, b.offs.reserve((K + 1) * 8));
        TK_HIP(c, b.perm.reserve(K * 4 + 16));
        TK_HIP(c, b.len.reserve(K * 4 + 16));
        TK_HIP(c, b.src.reserve(K * 8 + 16));
        a.perm = (uint32_t*)b.perm.p;
        a.len = (uint32_t*)b.len.p;
        a.src = (uint64_t*)b.src.p;
        a.out_offs = (uint64_t*)b.offs.p;
        a.out_ids = (uint32_t*)b.ids.p;
        a.out_lab = want_lab ? (int32_t*)b.lab.p : nullptr;
        // ---- the order: `cur` is the buffer of the pairs' documents (KEEP: the kept documents as they are)
        TK_HIP(c, hipEventRecord(b.ev[2], s));
        const uint32_t* val = a.kept;
        if (o->order != TK_REGROUP_ORDER_KEEP && K > 1) {
            const uint32_t blocks = tk_regroup_sort_blocks(K);
            for (DevBuf& k : b.key) TK_HIP(c, k.reserve(K * 4 + 16));
            for (DevBuf& v : b.val) TK_HIP(c, v.reserve(K * 4 + 16));
            TK_HIP(c, b.hist.reserve((uint64_t)blocks * 256 * 4 + 16));
            TK_HIP(c, b.hpos.reserve(((uint64_t)blocks * 256 + 1) * 8));
            TK_HIP(c, b.bsum.reserve(scan_workspace_bytes((uint64_t)blocks * 256)));
            a.hist = (uint32_t*)b.hist.p;
            a.hpos = (const uint64_t*)b.hpos.p;
            int kc = 0, vc = 0, vo = 1;                 // the key / document buffers that hold the pairs, and where a pass puts the documents
            auto set_out = [&] { a.key_out = (uint32_t*)b.key[kc].p; a.val_out = (uint32_t*)b.val[vc].p; };
            auto sort = [&](uint32_t passes) -> int {   // the pairs in key[kc] / val[vc], by the low `passes` digits of the key
                for (uint32_t p = 0; p < passes; ++p) {
                    a.key_in = (const uint32_t*)b.key[kc].p; a.val_in = (const uint32_t*)b.val[vc].p;
                    a.key_out = (uint32_t*)b.key[kc ^ 1].p; a.val_out = (uint32_t*)b.val[vo].p;
                    TK_HIP(c, tk_launch_regroup_hist(a, 8 * p, s));
                    const int r = scan_u32(c, b.bsum, a.hist, (uint64_t)blocks * 256, (uint64_t*)b.hpos.p, s);
                    if (r != TK_OK) return r;
                    TK_HIP(c, tk_launch_regroup_scatter(a, 8 * p, s));
                    kc ^= 1;
                    std::swap(vc, vo);
                }
                return TK_OK;
            };
            set_out();
            TK_HIP(c, tk_launch_regroup_keys(a, 0, s));
            if ((rc = sort(o->order == TK_REGROUP_ORDER_LENGTH ? radix_passes(a.longest) : 4)) != TK_OK) return rc;
            if (o->order == TK_REGROUP_ORDER_GROUPED) { // val[vc]: the shuffled documents, which stay where they are
                const int sh = vc;
                a.shuf = (const uint32_t*)b.val[sh].p;
                a.val_in = a.shuf;
                vc = vo; vo = 3 - sh - vc;
                set_out();
                TK_HIP(c, tk_launch_regroup_keys(a, 1, s));                  // (length key, shuffle rank)
                if ((rc = sort(radix_passes(a.longest))) != TK_OK) return rc;
                const uint32_t gp = radix_passes((K - 1) / o->window);
                if (gp) {
                    a.val_in = (const uint32_t*)b.val[vc].p;
                    kc ^= 1; std::swap(vc, vo);         // (the keys kernel is a pass of its own: from the pairs' buffers into the others)
                    set_out();
                    TK_HIP(c, tk_launch_regroup_keys(a, 2, s));              // (group, shuffle rank)
                    if ((rc = sort(gp)) != TK_OK) return rc;
                }
            }
            val = (const uint32_t*)b.val[vc].p;
        }
        a.val_in = val;
        TK_HIP(c, tk_launch_regroup_perm(a, s));
        if ((rc = scan_u32(c, b.bsum, a.len, K, a.out_offs, s)) != TK_OK) return rc;
        TK_HIP(c, hipEventRecord(b.ev[3], s));
        TK_HIP(c, tk_launch_regroup_gather(a, s));
        TK_HIP(c, hipEventRecord(b.ev[4], s));
        if (batches && K) {
            uint32_t levels = 0;
            while (levels < TKG_MAX_LEVELS && (1ull << (6 * levels)) < K) ++levels;
            uint64_t at = 0;
            for (uint32_t l = 1; l <= levels; ++l) { a.pyr_at[l] = at; at += (K + (1ull << (6 * l)) - 1) >> (6 * l); }
            a.n_levels = levels;
            TK_HIP(c, b.pyr.reserve(at * 4 + 16));
            TK_HIP(c, b.ja.reserve((K + 1) * 8));
            TK_HIP(c, b.jb.reserve((K + 1) * 8));
            TK_HIP(c, b.row.reserve((K + 1) * 4 + 16));
            TK_HIP(c, b.open.reserve((K + 2) * 8));
            TK_HIP(c, b.bmax.reserve(K * 4 + 16));
            if (want_bo) TK_HIP(c, b.bo.reserve((K + 1) * 8));
            if (want_brl) TK_HIP(c, b.brl.reserve(K * 4 + 16));
            a.pyr = (uint32_t*)b.pyr.p;
            a.jump = (uint64_t*)b.ja.p;
            a.row = (uint32_t*)b.row.p;
            a.bmax = (uint32_t*)b.bmax.p;
            a.open = (const uint64_t*)b.open.p;
            a.batch_offs = want_bo ? (uint64_t*)b.bo.p : nullptr;
            a.batch_rowlen = want_brl ? (uint32_t*)b.brl.p : nullptr;
            TkRowfitArgs ch;                            // the chain, as the doubling rounds of the rowfit pass take it: a batch is a row
            memset(&ch, 0, sizeof(ch));
            ch.n_docs = K;
            ch.jump_a = a.jump;
            ch.jump_b = (uint64_t*)b.jb.p;
            ch.row = a.row;
            ch.open = (uint64_t*)b.open.p;
            ch.E = ch.id_offs = a.out_offs;
            ch.stat = a.stat + 12;
            uint32_t rounds = 0;                        // (a batch holds a document: at most K links)
            while ((1ull << rounds) <= K) ++rounds;
            TK_HIP(c, tk_launch_regroup_pyramid(a, s));
            TK_HIP(c, tk_launch_regroup_nxt(a, s));
            TK_HIP(c, tk_launch_chain_rounds(ch, rounds, s));
            TK_HIP(c, tk_launch_regroup_batches(a, s));
            TK_HIP(c, hipMemcpyAsync(stat + 8, a.stat + 8, 24, hipMemcpyDeviceToHost, s));
        }
        TK_HIP(c, hipEventRecord(b.ev[5], s));
        staged = true;
    } else {
        TK_HIP(c, b.ids.reserve(16));
        if (want_lab) TK_HIP(c, b.lab.reserve(16));
        TK_HIP(c, b.offs.reserve(16));
        TK_HIP(c, b.perm.reserve(16));
        TK_HIP(c, hipMemsetAsync(b.offs.p, 0, 8, s));
    }
    if (batches && K == 0 && want_bo) {                 // (no batch: batch_offsets = [0])
        TK_HIP(c, b.bo.reserve(16));
        TK_HIP(c, hipMemsetAsync(b.bo.p, 0, 8, s));
    }
    if (batches && K == 0 && want_brl) TK_HIP(c, b.brl.reserve(16));
    TK_HIP(c, hipStreamSynchronize(s));
    if (staged) {
        (void)hipEventElapsedTime(&b.ms[1], b.ev[2], b.ev[3]);
        (void)hipEventElapsedTime(&b.ms[2], b.ev[3], b.ev[4]);
        (void)hipEventElapsedTime(&b.ms[3], b.ev[4], b.ev[5]);
    }
    out->ids = (uint32_t*)b.ids.p;
    out->offsets = (uint64_t*)b.offs.p;
    out->labels = want_lab ? (int32_t*)b.lab.p : nullptr;
    out->perm = want_perm ? (uint32_t*)b.perm.p : nullptr;
    out->batch_offsets = want_bo ? (uint64_t*)b.bo.p : nullptr;
    out->batch_rowlen = want_brl ? (uint32_t*)b.brl.p : nullptr;
    out->n_docs = K;
    out->n_ids = n_out;
    out->n_masked = stat[0];
    out->n_short = stat[1];
    out->n_long = stat[2];
    out->n_batches = stat[10];
    out->n_oversize = stat[8];
    out->n_batch_pad = stat[10] ? stat[9] - n_out : 0;
    return TK_OK;
}

namespace {
struct RegroupPass : LayoutPass<RegroupPass> {
    typedef tk_regroup_opts Opts;
    typedef tk_regroup Result;
    static constexpr const char* name = "regroup";
    static uint64_t esz(const Opts&) { return 4; }
    static constexpr auto encode_opts = regroup_encode_opts;
    static constexpr auto run = run_regroup;
    // (encoded text has neither a labels stream nor a keep mask)
    static int run_encoded(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t n_ids, const Opts* o, hipStream_t s,
                           Result* out) {
        return run_regroup(c, d_ids, d_id_offs, n_docs, n_ids, nullptr, nullptr, o, s, out);
    }
};
}  // namespace

extern "C" int tk_regroup_from_ids_device(tk_ctx* c, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                                          const void* d_labels, const void* d_keep, const tk_regroup_opts* opts, void* hip_stream,
                                          tk_regroup* out) {
    return layout_from_ids_device<RegroupPass>(c, d_ids, d_id_offsets, n_docs, n_ids, opts, hip_stream, out, (const int32_t*)d_labels,
                                               (const uint8_t*)d_keep);
}
extern "C" int tk_encode_batch_device_regroup(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs,
                                              uint64_t n_bytes, int add_bos, int add_eos, int checks, const tk_regroup_opts* opts,
                                              void* hip_stream, void** d_ids, void** d_out_offsets, uint64_t* n_ids, tk_regroup* out) {
    return layout_encode_device<RegroupPass>(c, d_bytes, d_doc_offsets, n_docs, n_bytes, add_bos, add_eos, checks, opts, hip_stream, d_ids,
                                             d_out_offsets, n_ids, out);
}
extern "C" int tk_encode_batch_regroup(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos,
                                       int add_eos, int validate_utf8, const tk_regroup_opts* opts, tk_regroup* out) {
    return layout_encode_host<RegroupPass>(c, bytes, doc_offsets, n_docs, add_bos, add_eos, validate_utf8, opts, out);
}
extern "C" void tk_free_regroup(tk_regroup* r) { layout_free(r); }

extern "C" void tk_last_regroup_ms(const tk_ctx* c, float ms[4]) {
    std::unique_lock<std::mutex> lock;
    if (c) lock = std::unique_lock<std::mutex>(const_cast<tk_ctx*>(c)->mu);   // (a call on another thread writes them under it)
    for (int i = 0; ms && i < 4; ++i) ms[i] = c ? c->regroup.ms[i] : 0.f;
}
