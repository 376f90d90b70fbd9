// tk_pipeline.cpp -- the batch pipeline over text on the device:  encode(pass 1) -> scan -> compact [-> pass 2 -> scan -> compact],
// in its flat (default), per-document and sequential (JSON pattern) forms, and the policy of the memo of merged pieces.
//
// Replaces CoreBPE::encode at reference src/tekkenizer.rs:384-386 and fuses the id shift / BOS / EOS of :390-402.  The device
// counters every step here reads and writes are named in tk_counters.h.
#include <algorithm>

#include "tk_ctx.h"

// The knobs tools set between calls: read at the start of every call of the pipeline
static TkCallKnobs call_knobs() {
    TkCallKnobs k;
    k.log = getenv("TK_DEBUG_LOG") != nullptr;
    k.marks = getenv("TK_DEBUG_MARKS") != nullptr;
    k.skip_pass2 = getenv("TK_DEBUG_SKIP_PASS2") != nullptr;
    if (const char* ll = getenv("TK_MEMO_LOG_LOG2")) { const int v = atoi(ll); if (v >= 8 && v <= 24) k.memo_log_log2 = v; }
#ifdef TK_ABLATE   /* `make ablate` builds only */
    if (const char* ab = getenv("TK_DEBUG_ABLATE")) k.ablate = atoi(ab);  // timing-only experiments
#endif
    return k;
}

static uint64_t cu_count(const tk_ctx* c) {
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device);
    return (uint64_t)cus;
}

TkEncodeArgs encode_args(tk_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offs, uint64_t n_docs, int add_bos, int add_eos) {
    TkEncodeArgs a;
    memset(&a, 0, sizeof(a));
    a.bytes = d_bytes;
    a.doc_offs = d_offs;
    a.n_docs = n_docs;
    a.staging = (uint32_t*)c->staging.p;
    a.counts = (uint32_t*)c->counts.p;
    a.work_counter = c->ctr(TKC_WORK);
    a.defer_count = c->ctr(TKC_DEFERRED);
    a.defer_list = (uint32_t*)c->defer_list.p;
    a.add_bos = add_bos;
    a.add_eos = add_eos;
    a.t = c->dview;
    return a;
}

// How pass 2 and the round-based kernels behind it are sized for n documents of at most maxlen bytes.  A scratch slice holds
// nodes (4 words per byte) | block minima | successor tokens (1 word per byte), 16-byte aligned; the grid of pass 2 is launched
// in blocks of 4 waves and EVERY launched wave owns a slice; the slices stay within 8 GiB.
struct Pass2Plan {
    uint64_t words;        // of a scratch slice
    uint64_t waves;        // pass 2 (mode 1)
    uint64_t walk_waves;   // the walk: one wave per document
    uint64_t blocks;       // the merges: one 16-wave block per CU (158 KB of LDS)
    uint64_t job_cap;      // a job is a piece of at least long_min bytes: no more of them than every document's share
};
static Pass2Plan pass2_plan(uint64_t maxlen, uint64_t n, uint64_t max_waves, uint64_t cus, uint32_t long_min) {
    Pass2Plan p;
    p.words = ((5 * maxlen + 2 * ((maxlen + 63) / 64) + 64 + 3) / 4) * 4;
    const uint64_t budget_words = (8ull << 30) / 4;
    const uint64_t fit = budget_words / p.words >= 4 ? budget_words / p.words : 4;   // scratch slices the budget allows
    p.waves = (std::min(std::min(n, max_waves), fit) + 3) / 4 * 4;
    if (p.waves == 0) p.waves = 4;
    p.walk_waves = std::min((std::min<uint64_t>(n, 1024u) + 3) / 4 * 4, fit / 4 * 4);
    p.blocks = std::min(cus, fit);
    p.job_cap = maxlen / (long_min ? long_min : 1) * n + n + 16;
    return p;
}

static void long_args(const tk_ctx* c, TkEncodeArgs& a) {
    a.long_min = c->knobs.long_min < 65u ? 65u : c->knobs.long_min;
    a.long_lazy_mul = c->knobs.long_lazy_mul;
    a.long_force = c->knobs.long_force;
}

// walk (one wave per document of a.todo_list; long pieces become jobs) -> merge the jobs in rounds (one workgroup each) ->
// squeeze the holes out.  No host sync in between: the merge grid is persistent and reads the job count itself.
static int enqueue_rounds(tk_ctx* c, const TkEncodeArgs& a, const Pass2Plan& p, uint64_t job_cap, uint64_t n, hipStream_t s) {
    TK_HIP(c, c->long_jobs.reserve(job_cap * sizeof(TkLongJob)));
    TkEncodeArgs b = a;
    b.long_list = nullptr;
    b.long_jobs = (TkLongJob*)c->long_jobs.p;
    b.long_job_count = c->ctr(TKC_LONG_JOBS);
    b.long_job_cap = (uint32_t)(job_cap > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : job_cap);
    TK_HIP(c, tk_launch_encode_long(b, (uint32_t)p.walk_waves, 0, s));
    TK_HIP(c, hipMemsetAsync(c->ctr(TKC_WORK), 0, 4, s));                   // the job queue's ticket counter
    const uint64_t cblocks = std::min<uint64_t>((n + 3) / 4, 4096);
    TK_HIP(c, tk_launch_encode_long_merge(b, (uint32_t)p.blocks, (uint32_t)cblocks, s));
    return TK_OK;
}

// Pass 2 over the n_def documents of c->defer_list: documents with a long piece that missed the vocabulary need the
// scratch-backed cooperative merge.  The scratch is sized from the longest deferred document.
static int run_pass2(tk_ctx* c, TkEncodeArgs& a, const uint64_t* d_offs, uint32_t n_def, hipStream_t s, uint64_t max_waves = 1024) {
    const bool dbg = c->call.log;
    uint32_t maxlen32 = 0;
    TK_HIP(c, hipMemsetAsync(c->ctr(TKC_DEFER_MAXLEN), 0, 4, s));
    TK_HIP(c, tk_launch_defer_maxlen((const uint32_t*)c->defer_list.p, n_def, d_offs, c->ctr(TKC_DEFER_MAXLEN), s));
    TK_HIP(c, hipMemcpyAsync(&maxlen32, c->ctr(TKC_DEFER_MAXLEN), 4, hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipStreamSynchronize(s));
    const uint64_t maxlen = maxlen32;
    if (dbg) fprintf(stderr, "[tk] pass2: n_def=%u maxlen=%llu\n", n_def, (unsigned long long)maxlen);
    const Pass2Plan p = pass2_plan(maxlen, n_def, max_waves, 0, 0);
    TK_HIP(c, c->scratch.reserve(p.waves * p.words * 4));
    a.todo_list = (const uint32_t*)c->defer_list.p;
    a.n_todo = n_def;
    a.scratch = (uint32_t*)c->scratch.p;
    a.scratch_words_per_wave = p.words;
    // documents with a LONG piece that is not a vocabulary key are handed on to the workgroup-per-document kernel
    // (tk_long.hip: the piece is merged in rounds by 16 waves instead of step by step by one)
    if (c->knobs.long_min) {
        TK_HIP(c, c->long_list.reserve(((size_t)n_def + 1) * 4));
        a.long_list = (uint32_t*)c->long_list.p;
        a.long_count = c->ctr(TKC_LONG_LIST);
        long_args(c, a);
    }
    TK_HIP(c, hipMemsetAsync(c->ctr(TKC_WORK), 0, 8, s));                    // (and TKC_DEFERRED)
    TK_HIP(c, hipMemsetAsync(c->ctr(TKC_LONG_LIST), 0, 4, s));
    TK_HIP(c, tk_launch_encode(a, 1, (uint32_t)p.waves, s));
    if (dbg) { TK_HIP(c, hipStreamSynchronize(s)); fprintf(stderr, "[tk] pass2 kernel done\n"); }
    if (!c->knobs.long_min) return TK_OK;
    TK_HIP(c, hipMemcpyAsync(c->h_pin + TKC_LONG_LIST, c->ctr(TKC_LONG_LIST), 4, hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipStreamSynchronize(s));
    const uint32_t n_long = c->h_pin[TKC_LONG_LIST];
    c->n_round_docs += n_long;
    if (!n_long) return TK_OK;
    const Pass2Plan q = pass2_plan(maxlen, n_long, max_waves, cu_count(c), a.long_min);
    TK_HIP(c, c->scratch.reserve(std::max(q.walk_waves, q.blocks) * q.words * 4));   // (pass 2 is complete: its slices are free)
    TkEncodeArgs b = a;
    b.todo_list = (const uint32_t*)c->long_list.p;
    b.n_todo = n_long;
    b.scratch = (uint32_t*)c->scratch.p;
    TK_HIP(c, hipMemsetAsync(c->ctr(TKC_WORK), 0, 4, s));
    TK_HIP(c, hipMemsetAsync(c->ctr(TKC_LONG_JOBS), 0, 4, s));
    int rc = enqueue_rounds(c, b, q, q.job_cap, n_long, s);
    if (rc != TK_OK) return rc;
    if (dbg) { TK_HIP(c, hipStreamSynchronize(s)); fprintf(stderr, "[tk] round-based kernels done: %u documents\n", n_long); }
    return TK_OK;
}

// The same passes WITHOUT a host sync, for the flat pipeline's tail: the documents are a.todo_list = `list`, their number lives
// in device memory (count_dev; NULL: n_bound is exact), n_bound and maxlen bound it and every document's length from above.
// Walk (one wave per document, piece by piece; long pieces become jobs), round-based merges of the jobs, compaction
// (tk_long.hip); TK_LONG_MIN=0: pass 2 alone.
static int enqueue_pass2(tk_ctx* c, TkEncodeArgs a, const uint32_t* list, const uint32_t* count_dev, uint32_t n_bound,
                         uint64_t maxlen, uint64_t n_bytes, hipStream_t s, uint64_t max_waves = 1024) {
    if (c->knobs.long_min) long_args(c, a);
    const Pass2Plan p = pass2_plan(maxlen, n_bound, max_waves, cu_count(c), a.long_min);
    // (with the round-based merges on -- the default -- the mode-1 pass-2 kernel is never launched: only the walk's waves and the
    // merging workgroups own a slice.  Sizing for p.waves as well allocated up to 5.4 GB on the JSON-pattern path, where max_waves
    // is 8192, for a batch with many handed-back 32 KiB documents)
    const uint64_t slices = c->knobs.long_min ? std::max(p.walk_waves, p.blocks) : p.waves;
    TK_HIP(c, c->scratch.reserve(slices * p.words * 4));
    a.todo_list = list;
    a.n_todo = n_bound;
    a.n_todo_dev = count_dev;
    a.defer_count = c->ctr(TKC_PASS2_SPARE);                               // (pass 2 defers nothing; count_dev may be TKC_DEFERRED)
    a.scratch = (uint32_t*)c->scratch.p;
    a.scratch_words_per_wave = p.words;
    TK_HIP(c, hipMemsetAsync(c->ctr(TKC_WORK), 0, 4, s));
    TK_HIP(c, hipMemsetAsync(c->ctr(TKC_LONG_LIST), 0, 8, s));             // (unused on this path) and TKC_LONG_JOBS
    if (!c->knobs.long_min) {                                              // (no round-based merges -- pass 2 does it all)
        TK_HIP(c, tk_launch_encode(a, 1, (uint32_t)p.waves, s));
        return TK_OK;
    }
    // The walk takes EVERY document of the list (the first form ran pass 2 first and walked only the documents in which it
    // met a long piece: two kernels in a row, each as long as its slowest document, the second redoing what the first
    // had done of its documents).  No more jobs than the text holds, either
    return enqueue_rounds(c, a, p, std::min(p.job_cap, n_bytes / a.long_min + n_bound + 16), n_bound, s);
}

// scan of the per-document counts and compaction of the staging rows into c->out_ids (the per-document and sequential pipelines)
static int scan_compact(tk_ctx* c, const TkEncodeArgs& a, hipStream_t s) {
    TK_HIP(c, tk_launch_scan(a.counts, a.n_docs, (uint64_t*)c->out_offs.p, (uint64_t*)c->block_sums.p, s));
    TK_HIP(c, tk_launch_compact(a.staging, a.doc_offs, a.counts, (const uint64_t*)c->out_offs.p, a.n_docs, (uint32_t*)c->out_ids.p, s));
    TK_HIP(c, hipEventRecord(c->ev[2], s));
    return TK_OK;
}
static int reserve_doc_buffers(tk_ctx* c, uint64_t n_docs, uint64_t n_bytes) {
    const uint64_t cap = n_bytes + 2 * n_docs + 64;
    TK_HIP(c, c->staging.reserve(cap * 4));
    TK_HIP(c, c->out_ids.reserve(cap * 4));
    TK_HIP(c, c->counts.reserve((n_docs + 1) * 4));
    TK_HIP(c, c->out_offs.reserve((n_docs + 1) * 8));
    TK_HIP(c, c->block_sums.reserve((n_docs / 2048 + 4) * 8));
    TK_HIP(c, c->defer_list.reserve((n_docs + 1) * 4));
    return TK_OK;
}

static int run_pipeline_doc(tk_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offs, uint64_t n_docs, uint64_t n_bytes,
                            int add_bos, int add_eos, hipStream_t s, uint64_t* n_ids) {
    int rc = reserve_doc_buffers(c, n_docs, n_bytes);
    if (rc != TK_OK) return rc;
    TkEncodeArgs a = encode_args(c, d_bytes, d_offs, n_docs, add_bos, add_eos);
    a.dbg_ablate = c->call.ablate;
    if (c->call.marks && !c->dbg_mark) {
        TK_HIP(c, c->dbg_mark.alloc(256, hipHostMallocMapped));
        memset(c->dbg_mark, 0, 256);
    }
    if (c->call.marks) a.dbg_mark = c->dbg_mark;
    TK_HIP(c, hipMemsetAsync(c->ctr(TKC_WORK), 0, TKC_CLEARED * 4, s));
    TK_HIP(c, hipEventRecord(c->ev[0], s));
    uint64_t want = (n_docs + 7) / 8;
    uint32_t n_waves = (uint32_t)(want < 8192 ? (want ? want : 1) : 8192);
    TK_HIP(c, tk_launch_encode(a, 0, n_waves, s));
    TK_HIP(c, hipEventRecord(c->ev[1], s));
    if ((rc = scan_compact(c, a, s)) != TK_OK) return rc;
    uint32_t head[TKC_DEFER_MAXLEN + 1] = {0, 0, 0, 0};
    uint64_t total = 0;
    TK_HIP(c, hipMemcpyAsync(head, c->ctr(TKC_WORK), sizeof(head), hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipMemcpyAsync(&total, (uint64_t*)c->out_offs.p + n_docs, 8, hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipStreamSynchronize(s));
    const uint32_t n_def = head[TKC_DEFERRED];
    c->n_long_docs = n_def;
    if (c->call.log) fprintf(stderr, "[tk] pass1 done: docs=%llu deferred=%u total=%llu\n", (unsigned long long)n_docs, n_def, (unsigned long long)total);
    if (n_def != 0 && !c->call.skip_pass2) {
        if ((rc = run_pass2(c, a, d_offs, n_def, s)) != TK_OK || (rc = scan_compact(c, a, s)) != TK_OK) return rc;
        TK_HIP(c, hipMemcpyAsync(&total, (uint64_t*)c->out_offs.p + n_docs, 8, hipMemcpyDeviceToHost, s));
        TK_HIP(c, hipStreamSynchronize(s));
    }
    (void)hipEventElapsedTime(&c->encode_ms, c->ev[0], c->ev[1]);
    (void)hipEventElapsedTime(&c->pipeline_ms, c->ev[0], c->ev[2]);
    *n_ids = total;
    return TK_OK;
}

// MEMO (tk_hash.h): the table is allocated at the first flat-pipeline call that wants it.  Adaptive policy (memo_account): a call's
// hit rate = hits / (hits + pieces of 2..16 bytes the narrow merge kernel still had to merge); on text whose unknown pieces do not
// come back (random code points: BASELINE configs[2]) or that has few of them (a vocabulary fitted to the text), the look-ups cost
// more than the hits return, so after two such calls in a row the table is left alone for 30 calls, then tried again.
// Whatever the policy does, ids never depend on it: an entry is the exact key and the pure merge of its bytes.
static int memo_prepare(tk_ctx* c, TkFlatArgs& fa, hipStream_t s, uint64_t n_bytes) {
    TkKnobs& k = c->knobs;
    c->memo_active_last = false;           // (fa's memo fields are zero: the table is off for this call unless all of this goes through)
    if (k.memo_log2 == 0) return TK_OK;
    // adaptive policy: a call of under 1 MB leaves the table alone (and a context that only ever sees such calls never allocates
    // its 576 MB): memo_account cannot judge a call that small, and its two extra launches are a tenth of its time
    if (k.memo_policy == 0 && n_bytes < (1u << 20)) return TK_OK;
    if (k.memo_policy == 0 && c->memo_pause) { --c->memo_pause; return TK_OK; }
    const size_t bytes = ((size_t)1 << k.memo_log2) * sizeof(tk_memo_entry);
    if (c->memo_have_log2 != k.memo_log2) {
        c->t_memo.release();
        if (c->t_memo.reserve(bytes) != hipSuccess) {      // no room: the memo is an optimisation, the call goes on without it
            (void)hipGetLastError();
            k.memo_log2 = 0; c->memo_have_log2 = 0;
            return TK_OK;
        }
        TK_HIP(c, hipMemsetAsync(c->t_memo.p, 0, bytes, s));
        c->memo_have_log2 = k.memo_log2;
        c->memo_epoch = 0;
    }
    if (c->memo_epoch >= 0xFFFFFFF0u) {                     // the claim word would wrap: start over
        TK_HIP(c, hipMemsetAsync(c->t_memo.p, 0, bytes, s));
        c->memo_epoch = 0;
    }
    // the log of a call's new entries: one stretch per wave of the narrow merge kernel's grid (at most 16 waves on each CU), a
    // quarter of the table in all, at most 2^21 records (what does not fit is dropped and comes again)
    const uint32_t log_waves = (uint32_t)cu_count(c) * 16u;
    // (TK_MEMO_LOG_LOG2: records of the log, all waves together; measured on the held-out shape: what bounds the hit rate of a table
    // of 2^22 entries is how many new entries a call can log, not the table)
    const uint32_t log_log2 = c->call.memo_log_log2 ? (uint32_t)c->call.memo_log_log2 : k.memo_log2 > 23 ? 21 : k.memo_log2 - 2;
    const uint32_t log_cap = 1u << log_log2;
    const uint32_t per_wave = log_cap / log_waves > 0 ? log_cap / log_waves : 1u;
    if (c->t_memo_log.reserve((size_t)per_wave * log_waves * sizeof(tk_memo_entry) + (size_t)log_waves * 4) != hipSuccess) {
        (void)hipGetLastError();
        c->t_memo.release();
        k.memo_log2 = 0; c->memo_have_log2 = 0;
        return TK_OK;
    }
    fa.memo_tab = (tk_memo_entry*)c->t_memo.p;
    fa.memo_mask = (1u << k.memo_log2) - 1u;
    fa.memo_log = (tk_memo_entry*)c->t_memo_log.p;
    fa.memo_log_counts = (uint32_t*)(fa.memo_log + (size_t)per_wave * log_waves);
    fa.memo_log_per_wave = per_wave;
    fa.memo_log_waves = log_waves;
    TK_HIP(c, hipMemsetAsync(fa.memo_log_counts, 0, (size_t)log_waves * 4, s));   // (waves the grid does not launch log nothing)
    fa.memo_epoch = ++c->memo_epoch;
    fa.memo_probe = c->memo_epoch > 1 ? 1 : 0;            // (the first call on an empty table: nothing to find, only to fill)
    fa.memo_hits = c->ctr(TKC_MEMO_HITS);
    c->memo_active_last = true;
    return TK_OK;
}
static void memo_account(tk_ctx* c, const uint32_t* final_ctr, uint64_t n_bytes) {
    c->memo_hits_last = c->memo_lookups_last = 0;
    if (!c->memo_active_last) return;
    c->memo_hits_last = final_ctr[TKC_MEMO_HITS];
    c->memo_lookups_last = (uint64_t)final_ctr[TKC_MEMO_HITS] + final_ctr[TKC_NARROW_LEFT];
    c->memo_hits_total += c->memo_hits_last;
    c->memo_lookups_total += c->memo_lookups_last;
    if (c->knobs.memo_policy != 0 || c->memo_epoch < 2 || n_bytes < (1u << 20)) return;   // (the first call fills an empty table)
    // does it pay?  A look-up is one more dependent load in the flat kernel's miss path (measured on the 1 M x 512-byte shapes:
    // +0.15 .. 0.18 ms whatever the number of look-ups), a hit saves a merge (~0.075 ms per million): under one hit per 160 bytes of
    // text, or under three hits in ten look-ups (the mixed UTF-8 shape at 28 %: no gain, no loss), the table is left alone for 30 calls.
    const bool pays = c->memo_hits_last * 10 >= c->memo_lookups_last * 3 && c->memo_hits_last * 160 >= n_bytes;
    if (pays) c->memo_low_streak = 0;
    else if (++c->memo_low_streak >= 2) { c->memo_pause = 30; c->memo_low_streak = 0; }
}

// ---- The flat pipeline (tk_flat.hip): one wave per 2048-byte region of the packed stream, documents the fast path cannot take
// (non-ASCII, very long runs / pieces) redone by the per-document kernels.  One call is a FlatRun taken through the steps below
// by run_pipeline_flat. ----
struct FlatRun {
    tk_ctx* c;
    const uint8_t* d_bytes;
    const uint64_t* d_offs;
    uint64_t n_docs, n_bytes, n_chunks;
    int add_bos, add_eos;
    hipStream_t s, sb;             // stream A (the caller's) and B (the tail; A itself with TK_TAIL=serial)
    bool serial;
    uint64_t wf_narrow;            // entries of f_wfirst for the narrow classes (the wide ones lie behind them)
    uint64_t total;                // ids of the batch, once a finish() has been waited for
    TkFlatArgs fa;
    bool fold_miss, fold_doc;      // the folded forms of the two scans (flat_fold_choice)
    bool merge_one;                // both merge kernels in one launch (tk_merge_all_kernel)
};

// The folded forms (tk_flat_tail_impl.h) run where there is something to scan and the partial sums are few: every consumer adds
// them up itself, (partial sums)^2 loads in all.  TK_TAIL_FOLD=0 / 1 forces either form (1: wherever it can run).
static void flat_fold_choice(FlatRun& r) {
    const TkKnobs& k = r.c->knobs;
    const uint64_t miss_sums = (5 * r.n_chunks + TKF_FOLD_TILE - 1) / TKF_FOLD_TILE, doc_blocks = (r.n_docs + TKF_FOLD_DOC_BLOCK - 1) / TKF_FOLD_DOC_BLOCK;
    r.fold_miss = r.n_chunks != 0 && k.tail_fold != 0 && (k.tail_fold == 1 || miss_sums <= k.fold_miss_max);
    r.fold_doc = r.n_docs != 0 && k.tail_fold != 0 && (k.tail_fold == 1 || doc_blocks <= k.fold_doc_max);
    r.merge_one = k.tail_fold != 0 && k.fold_merge;
}

static int flat_reserve(FlatRun& r) {
    tk_ctx* c = r.c;
    const uint64_t n_chunks = r.n_chunks, n_docs = r.n_docs;
    TK_HIP(c, c->f_first.reserve((n_chunks + 1) * 4));
    TK_HIP(c, c->f_tmp.reserve((n_chunks * TKF_STRIDE + 64) * 4));
    TK_HIP(c, c->f_lstart.reserve((n_docs + 1) * 4));
    TK_HIP(c, c->f_flags.reserve(2 * (n_docs + 1) * 4));   // flags | holes (one memset)
    TK_HIP(c, c->f_todo.reserve((n_docs + 1) * 4));
    TK_HIP(c, c->f_miss.reserve((n_chunks * TKF_MISSCAP + 64) * 4));  // worst case; only the used records are ever touched
    TK_HIP(c, c->f_mcnt.reserve((5 * n_chunks + 1) * 4));   // 4 C miss counts (class-major) | C slot counts (one scan)
    TK_HIP(c, c->f_mpfx.reserve((5 * n_chunks + 2) * 8));
    TK_HIP(c, c->f_info.reserve((n_docs + 1) * 16));
    // one entry per 64 queued pieces: the narrow classes (2..16 bytes), then the wide ones (17..64 bytes)
    r.wf_narrow = n_chunks * (TKF_MISSOFF2 / 64 + 1) + 64;
    const uint64_t wf_wide = n_chunks * ((TKF_MISSCAP - TKF_MISSOFF2) / 64 + 1) + 64;
    TK_HIP(c, c->f_wfirst.reserve((r.wf_narrow + wf_wide) * 4));
    TK_HIP(c, c->counts.reserve((n_docs + 1) * 4));
    TK_HIP(c, c->out_offs.reserve((n_docs + 1) * 8));
    const uint64_t scan_n = n_docs > 5 * n_chunks ? n_docs : 5 * n_chunks;
    TK_HIP(c, c->block_sums.reserve((scan_n / 2048 + 4) * 8));
    if (r.fold_doc) TK_HIP(c, c->f_gsum.reserve(((n_docs + 63) / 64 + (n_docs + TKF_FOLD_DOC_BLOCK - 1) / TKF_FOLD_DOC_BLOCK + 2) * 8));   // group sums | block sums
    return TK_OK;
}

static void flat_args(FlatRun& r) {
    tk_ctx* c = r.c;
    TkFlatArgs& fa = r.fa;
    memset(&fa, 0, sizeof(fa));
    fa.bytes = r.d_bytes;
    fa.doc_offs = r.d_offs;
    fa.n_docs = r.n_docs;
    fa.n_bytes = r.n_bytes;
    fa.n_chunks = r.n_chunks;
    fa.first_doc = (const uint32_t*)c->f_first.p;
    fa.tmp = (uint32_t*)c->f_tmp.p;
    fa.kcount = (uint32_t*)c->f_mcnt.p + 4 * r.n_chunks;
    fa.lstart = (uint32_t*)c->f_lstart.p;
    fa.flags = (uint32_t*)c->f_flags.p;
    fa.miss_list = (uint32_t*)c->f_miss.p;
    fa.miss_count = (uint32_t*)c->f_mcnt.p;
    fa.miss_prefix = (const uint64_t*)c->f_mpfx.p;
    fa.holes = (uint32_t*)c->f_flags.p + (r.n_docs + 1);
    fa.wave_first = (uint32_t*)c->f_wfirst.p;
    fa.wave_first_wide = (uint32_t*)c->f_wfirst.p + r.wf_narrow;
    fa.t = c->dview;
    fa.pattern = c->pattern;
    fa.dbg_ablate = c->call.ablate;
}

// Pieces of 65..TKF_LONGCAP bytes stay on the flat path as records (TKC_LONG_RECS), and the chunks that hold a piece of more
// than 64 bytes go on a list (TKC_CUT_CHUNKS) for tk_flat_cut_kernel.  The flat kernel finds both through the control words
// behind the counters (not touched by the pre-pass): written when a buffer changes, i.e. a handful of times in a context's life.
// TK_FLAT_LONG=0: such pieces hand their documents back; TK_FLAT_CUT=0 or the JSON pattern: a null list, no cuts.
static int flat_control_words(FlatRun& r) {
    tk_ctx* c = r.c;
    TkFlatArgs& fa = r.fa;
    if (c->knobs.no_flat_long) return TK_OK;
    TK_HIP(c, c->f_long.reserve((r.n_bytes / 65 + 1024) * sizeof(TkFlatLongRec)));
    fa.long_recs = (TkFlatLongRec*)c->f_long.p;
    fa.long_count = c->ctr(TKC_LONG_RECS);
    fa.long_cap = (uint32_t)std::min<uint64_t>(c->f_long.cap / sizeof(TkFlatLongRec), 0xFFFFFFF0ull);
    fa.long_ctl = c->ctr(TKC_LONG_CTL);
    if (c->long_ctl_ptr != c->f_long.p || c->long_ctl_cap != fa.long_cap) {
        const uint64_t pv = (uint64_t)reinterpret_cast<uintptr_t>(c->f_long.p);
        const uint32_t words[] = {(uint32_t)pv, (uint32_t)(pv >> 32), fa.long_cap};   // TKC_LONG_CTL, _HI, _CAP
        TK_HIP(c, hipMemcpyAsync(c->ctr(TKC_LONG_CTL), words, sizeof(words), hipMemcpyHostToDevice, r.s));
        TK_HIP(c, hipStreamSynchronize(r.s));
        c->long_ctl_ptr = c->f_long.p;
        c->long_ctl_cap = fa.long_cap;
    }
    void* want_cut = nullptr;
    if (!c->knobs.no_flat_cut && c->pattern == 0) {
        TK_HIP(c, c->f_cut.reserve((r.n_chunks + 1) * 4));
        want_cut = c->f_cut.p;
        fa.cut_list = (uint32_t*)c->f_cut.p;
        fa.cut_count = c->ctr(TKC_CUT_CHUNKS);
    }
    if (c->cut_ctl_ptr != want_cut) {
        const uint64_t pv = (uint64_t)reinterpret_cast<uintptr_t>(want_cut);
        const uint32_t words[] = {(uint32_t)pv, (uint32_t)(pv >> 32)};                // TKC_CUT_CTL, _HI
        TK_HIP(c, hipMemcpyAsync(c->ctr(TKC_CUT_CTL), words, sizeof(words), hipMemcpyHostToDevice, r.s));
        TK_HIP(c, hipStreamSynchronize(r.s));
        c->cut_ctl_ptr = want_cut;
    }
    return TK_OK;
}

// The list of the handed-back documents is made on a second stream (B) right behind the flat kernel, beside the merge
// kernels, and comes to the host first (the early copy): if there are such documents, the per-document passes over them run on B
// while stream A is still merging -- the tail of a batch (Zipf shape: pass 2, walk, round-based merges, compaction; each as long
// as its longest document) is hidden instead of appended.
static int flat_fork_todo(FlatRun& r) {
    tk_ctx* c = r.c;
    if (!r.serial) {
        TK_HIP(c, hipEventRecord(c->ev_b[0], r.s));
        TK_HIP(c, hipStreamWaitEvent(r.sb, c->ev_b[0], 0));
    }
    TK_HIP(c, tk_launch_flat_todo(r.fa.flags, r.d_offs, r.n_docs, (uint32_t*)c->f_todo.p, c->ctr(TKC_TODO), c->ctr(TKC_TODO_MAXLEN), r.sb));
    if (!r.serial) {
        TK_HIP(c, hipMemcpyAsync(c->h_pin + TKC_EARLY_MIRROR, c->ctr(TKC_WORK), TKC_EARLY_WORDS * 4, hipMemcpyDeviceToHost, r.sb));
        TK_HIP(c, hipEventRecord(c->ev_b[1], r.sb));
    }
    return TK_OK;
}

// counts -> scan -> assembly -> every counter of the batch with one copy into pinned memory (TKC_TOTAL: left there by the
// assembly).  final_pass = 0 is the optimistic pass: if nothing was handed back and no long-piece record waits, it IS the result
// (the assembly copies nothing otherwise).
static int flat_finish(FlatRun& r, int final_pass, bool wait) {
    tk_ctx* c = r.c;
    const TkFlatArgs& fa = r.fa;
    const uint32_t extra = (uint32_t)((r.add_bos ? 1 : 0) + (r.add_eos ? 1 : 0));
    // chunk slot prefix sums: behind those of the 4 C miss counts (offset by the miss total: only differences are used)
    const uint64_t* d_P = (const uint64_t*)c->f_mpfx.p + 4 * r.n_chunks;
    if (r.fold_doc) {   // two launches: the counts kernel leaves sums, the assembly makes its own offsets
        uint64_t* gsum = (uint64_t*)c->f_gsum.p;
        uint64_t* bsum = gsum + (r.n_docs + 63) / 64;
        TK_HIP(c, tk_launch_flat_counts_sums(r.d_offs, r.n_docs, r.n_bytes, r.n_chunks, d_P, fa.lstart, fa.flags, fa.holes, extra,
                                             (uint32_t*)c->counts.p, c->f_info.p, final_pass, c->ctr(TKC_HANDED_BACK), gsum, bsum, r.s));
        TK_HIP(c, tk_launch_flat_assemble_fold(r.n_docs, c->f_info.p, fa.kcount, (const uint32_t*)c->counts.p, gsum, bsum,
                                               (uint64_t*)c->out_offs.p, fa.tmp, (const uint32_t*)c->staging.p, (uint32_t*)c->out_ids.p,
                                               c->host.bos_id, c->host.eos_id, r.add_bos, r.add_eos, (uint64_t*)c->ctr(TKC_TOTAL),
                                               final_pass ? nullptr : c->ctr(TKC_HANDED_BACK), r.s));
    } else {
        TK_HIP(c, tk_launch_flat_counts(r.d_offs, r.n_docs, r.n_bytes, r.n_chunks, d_P, fa.lstart, fa.flags, fa.holes, extra,
                                        (uint32_t*)c->counts.p, c->f_info.p, final_pass, c->ctr(TKC_HANDED_BACK), r.s));
        TK_HIP(c, tk_launch_scan((const uint32_t*)c->counts.p, r.n_docs, (uint64_t*)c->out_offs.p, (uint64_t*)c->block_sums.p, r.s));
        TK_HIP(c, tk_launch_flat_assemble(r.n_docs, c->f_info.p, fa.kcount, (const uint64_t*)c->out_offs.p, fa.tmp,
                                          (const uint32_t*)c->staging.p, (uint32_t*)c->out_ids.p, c->host.bos_id,
                                          c->host.eos_id, r.add_bos, r.add_eos, (uint64_t*)c->ctr(TKC_TOTAL),
                                          final_pass ? nullptr : c->ctr(TKC_HANDED_BACK), r.s));
    }
    TK_HIP(c, hipEventRecord(c->ev[2], r.s));
    TK_HIP(c, hipMemcpyAsync(c->h_pin, c->ctr(TKC_WORK), TKC_FINAL_WORDS * 4, hipMemcpyDeviceToHost, r.s));
    if (wait) {
        TK_HIP(c, hipStreamSynchronize(r.s));
        ++c->host_syncs;
        memcpy(&r.total, c->h_pin + TKC_TOTAL, 8);
    }
    return TK_OK;
}

// Pass 1 (mode 3) over the n documents of a.todo_list on stream s
static int enqueue_pass1_todo(tk_ctx* c, const TkEncodeArgs& a, uint32_t n, hipStream_t s) {
    TK_HIP(c, hipMemsetAsync(c->ctr(TKC_WORK), 0, 8, s));                    // (and TKC_DEFERRED)
    const uint64_t want = ((uint64_t)n + 7) / 8;
    TK_HIP(c, tk_launch_encode(a, 3, (uint32_t)(want < 8192 ? want : 8192), s));
    return TK_OK;
}

// What the optimistic pass could not finish.  Stream A: the n_lrec long-piece records, one wave each (lookup / merge into the
// reserved slots); a piece that turns out longer than TKF_LONGCAP flags its document and puts it on the late list (TKC_LATE).
// Stream B: the per-document path over the n_todo handed-back documents -- pass 1 (mode 3), then, for what it defers (the count
// stays on the device), pass 2 and the round-based kernels; the JSON pattern's go straight to the piece-by-piece path with its
// sequential matcher.  A waits for B.
static int flat_enqueue_tail(FlatRun& r, TkEncodeArgs& a, uint32_t n_lrec, uint32_t n_todo, uint64_t maxlen) {
    tk_ctx* c = r.c;
    TkFlatArgs& fa = r.fa;
    if (n_lrec) {
        fa.long_merge128 = c->knobs.no_flat_long128 ? 0 : 1;
        const uint32_t lwaves = ((n_lrec < 8192u ? n_lrec : 8192u) + 3u) / 4u * 4u;
        TK_HIP(c, c->scratch_rec.reserve((size_t)lwaves * TKF_LONG_SCRATCH_WORDS * 4));
        TK_HIP(c, c->f_late.reserve((r.n_docs + 1) * 4));
        fa.late_list = (uint32_t*)c->f_late.p;
        fa.late_count = c->ctr(TKC_LATE);
        TK_HIP(c, tk_launch_flat_long(fa, c->ctr(TKC_WORK), (uint32_t*)c->scratch_rec.p, TKF_LONG_SCRATCH_WORDS, lwaves, r.s));
    }
    if (!n_todo) return TK_OK;
    int rc;
    a.todo_list = (const uint32_t*)c->f_todo.p;
    a.n_todo = n_todo;
    if (c->pattern == 1) {
        rc = enqueue_pass2(c, a, (const uint32_t*)c->f_todo.p, nullptr, n_todo, maxlen, r.n_bytes, r.sb, 8192);
    } else {
        if ((rc = enqueue_pass1_todo(c, a, n_todo, r.sb)) != TK_OK) return rc;
        rc = enqueue_pass2(c, a, (const uint32_t*)c->defer_list.p, c->ctr(TKC_DEFERRED), n_todo, maxlen, r.n_bytes, r.sb);
    }
    if (rc != TK_OK) return rc;
    if (!r.serial) {
        TK_HIP(c, hipEventRecord(c->ev_b[2], r.sb));
        TK_HIP(c, hipStreamWaitEvent(r.s, c->ev_b[2], 0));
    }
    return TK_OK;
}

// rare: documents that a long-piece record flagged (an open piece of more than TKF_LONGCAP bytes without a cut) after the list was
// made -- the same passes over the late list, in sequence on stream A, and the result is assembled again
static int flat_redo_late(FlatRun& r, TkEncodeArgs& a, uint32_t n_late) {
    tk_ctx* c = r.c;
    int rc;
    c->n_flagged += n_late;
    a.todo_list = (const uint32_t*)c->f_late.p;
    a.n_todo = n_late;
    a.n_todo_dev = nullptr;
    a.defer_count = c->ctr(TKC_DEFERRED);
    if (c->pattern == 1) {
        TK_HIP(c, hipMemcpyAsync(c->defer_list.p, c->f_late.p, (size_t)n_late * 4, hipMemcpyDeviceToDevice, r.s));
        if ((rc = run_pass2(c, a, r.d_offs, n_late, r.s, 8192)) != TK_OK) return rc;
        c->n_long_docs += n_late;
    } else {
        if ((rc = enqueue_pass1_todo(c, a, n_late, r.s)) != TK_OK) return rc;
        uint32_t n_def = 0;
        TK_HIP(c, hipMemcpyAsync(&n_def, c->ctr(TKC_DEFERRED), 4, hipMemcpyDeviceToHost, r.s));
        TK_HIP(c, hipStreamSynchronize(r.s));
        c->n_long_docs += n_def;
        if (n_def && (rc = run_pass2(c, a, r.d_offs, n_def, r.s)) != TK_OK) return rc;
    }
    return flat_finish(r, 1, true);
}

// Everything behind the early copy: the plain case (the optimistic pass was the result), or the tail and the final passes
static int flat_complete(FlatRun& r, const uint32_t* early) {
    tk_ctx* c = r.c;
    const uint32_t n_todo = early[TKC_TODO];
    uint32_t n_lrec = early[TKC_LONG_RECS];
    const uint64_t maxlen = early[TKC_TODO_MAXLEN];
    c->n_cut_chunks = early[TKC_CUT_CHUNKS];
    c->n_flagged = n_todo;
    c->n_long_docs = 0;
    c->n_long_recs = 0;
    if (c->call.log) fprintf(stderr, "[tk] flat: docs=%llu chunks=%llu handed back=%u (longest %llu bytes) long-piece records=%u cut chunks=%u\n",
                             (unsigned long long)r.n_docs, (unsigned long long)r.n_chunks, n_todo, (unsigned long long)maxlen, n_lrec, early[TKC_CUT_CHUNKS]);
    if (n_todo == 0 && n_lrec == 0) {
        if (!r.serial) {
            TK_HIP(c, hipStreamSynchronize(r.s));
            ++c->host_syncs;
            memcpy(&r.total, c->h_pin + TKC_TOTAL, 8);
        }
        return TK_OK;
    }
    TK_HIP(c, c->staging.reserve((r.n_bytes + 2 * r.n_docs + 64) * 4));
    TK_HIP(c, c->defer_list.reserve((r.n_docs + 1) * 4));
    TkEncodeArgs a = encode_args(c, r.d_bytes, r.d_offs, r.n_docs, r.add_bos, r.add_eos);
    a.pattern = c->pattern;
    if (n_lrec > r.fa.long_cap) n_lrec = r.fa.long_cap;
    c->n_long_recs = n_lrec;
    int rc = flat_enqueue_tail(r, a, n_lrec, n_todo, maxlen);
    if (rc != TK_OK || (rc = flat_finish(r, 1, true)) != TK_OK) return rc;
    if (c->h_pin[TKC_PASS2_SPARE] == TKC_OVERFLOW) { c->err = "internal: the long-piece job list overflowed"; return TK_ERR_RUNTIME; }   // (set by tk_long_walk_kernel)
    c->n_long_docs = c->pattern == 1 ? n_todo : c->h_pin[TKC_DEFERRED];
    c->n_round_docs += n_todo && c->knobs.long_min ? c->h_pin[TKC_LONG_JOBS] : 0;   // (here: long pieces merged in rounds)
    const uint32_t n_late = n_lrec ? c->h_pin[TKC_LATE] : 0;
    return n_late ? flat_redo_late(r, a, n_late) : TK_OK;
}

// One host sync per batch on stream A in the common case, and one for the early copy of stream B.  Everything that depends on
// device-side counts stays on the device: the merge kernels are persistent, the output buffer takes its upper bound (a document
// cannot produce more ids than bytes + 2), and the handed-back documents are only COUNTED at first -- if there are any, the
// per-document kernels run afterwards and counts / scan / assembly are redone.
static int run_pipeline_flat(tk_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offs, uint64_t n_docs, uint64_t n_bytes,
                             int add_bos, int add_eos, hipStream_t s, uint64_t* n_ids) {
    const bool serial = c->knobs.serial_tail;
    FlatRun r = {c, d_bytes, d_offs, n_docs, n_bytes, (n_bytes + TKF_COMMIT - 1) / TKF_COMMIT, add_bos, add_eos,
                 s, serial ? s : (hipStream_t)c->stream_b, serial, 0, 0, {}, false, false, false};
    flat_fold_choice(r);
    int rc = flat_reserve(r);
    if (rc != TK_OK) return rc;
    flat_args(r);
    if ((rc = flat_control_words(r)) != TK_OK) return rc;
    TK_HIP(c, c->out_ids.reserve((n_bytes + 2 * n_docs + 64) * 4));
    if ((rc = memo_prepare(c, r.fa, s, n_bytes)) != TK_OK) return rc;
    TK_HIP(c, hipEventRecord(c->ev[3], s));
    // (the pre-pass also clears the per-document flags / holes and the TKC_CLEARED counter words: no memset launches)
    TK_HIP(c, tk_launch_flat_firstdoc(d_offs, n_docs, r.n_chunks, (uint32_t*)c->f_first.p, r.fa.flags, r.fa.holes, c->ctr(TKC_WORK), s));
    TK_HIP(c, hipEventRecord(c->ev[0], s));
    TK_HIP(c, tk_launch_flat(r.fa, s));
    TK_HIP(c, hipEventRecord(c->ev[1], s));
    if (r.fa.dbg_ablate & 24) {  // timing-only runs that stop inside the flat kernel: nothing downstream has valid input
        TK_HIP(c, hipEventRecord(c->ev[2], s));
        TK_HIP(c, hipStreamSynchronize(s));
        (void)hipEventElapsedTime(&c->encode_ms, c->ev[0], c->ev[1]);
        (void)hipEventElapsedTime(&c->pipeline_ms, c->ev[3], c->ev[2]);
        c->n_flagged = 0;
        *n_ids = 0;
        return TK_OK;
    }
    c->host_syncs = 0;
    // From here on work is queued on TWO streams.  Whatever way this function is left on an error -- a failed reserve, a failed
    // launch --, both have drained before the caller sees it: the next call's pre-pass runs on `s` alone and would otherwise race
    // the tail of this batch (pass 1, the walk, the merges) for counts, staging and the counters.
    struct JoinStreams {
        hipStream_t a, b;
        bool armed;
        ~JoinStreams() { if (armed) { (void)hipStreamSynchronize(b); (void)hipStreamSynchronize(a); } }
    } join_guard{s, r.sb, true};
    if ((rc = flat_fork_todo(r)) != TK_OK) return rc;
    if (r.fold_miss) {  // block sums -> apply (prefix sums, wave_first*, TKC_NARROW_LEFT in one pass)
        TK_HIP(c, tk_launch_fold_apply(r.fa.miss_count, 5 * r.n_chunks, r.n_chunks, (uint64_t*)c->f_mpfx.p, (uint64_t*)c->block_sums.p,
                                       r.fa.wave_first, r.fa.wave_first_wide, c->ctr(TKC_NARROW_LEFT), s));
    } else {
        TK_HIP(c, tk_launch_scan(r.fa.miss_count, 5 * r.n_chunks, (uint64_t*)c->f_mpfx.p, (uint64_t*)c->block_sums.p, s));
        TK_HIP(c, tk_launch_merge_wavefirst(r.fa.miss_prefix, r.n_chunks, r.fa.wave_first, r.fa.wave_first_wide, c->ctr(TKC_NARROW_LEFT), s));
    }
    // the single merge launch has nothing to do with the fold's bound: it is taken behind either scan form (TK_TAIL_FOLD=0: the two kernels)
    TK_HIP(c, r.merge_one ? tk_launch_merge_all(r.fa, s) : tk_launch_merge_kernels(r.fa, s));
    TK_HIP(c, hipEventRecord(c->ev[4], s));
    if ((rc = flat_finish(r, 0, r.serial)) != TK_OK) return rc;
    const uint32_t* early = c->h_pin;
    if (!r.serial) {
        TK_HIP(c, hipEventSynchronize(c->ev_b[1]));
        ++c->host_syncs;
        early = c->h_pin + TKC_EARLY_MIRROR;
    }
    if ((rc = flat_complete(r, early)) != TK_OK) return rc;
    (void)hipEventElapsedTime(&c->encode_ms, c->ev[0], c->ev[1]);
    (void)hipEventElapsedTime(&c->pipeline_ms, c->ev[3], c->ev[2]);
    (void)hipEventElapsedTime(&c->merge_ms, c->ev[1], c->ev[4]);
    memo_account(c, c->h_pin, n_bytes);
    *n_ids = r.total;
    join_guard.armed = false;      // (every path to here has waited for both streams already)
    return TK_OK;
}

// Row f-3, opt-in (tk_ctx_set_pattern(ctx, 1)) with TK_PIPELINE=doc: EVERY document takes the piece-by-piece path of
// pass 2 with the sequential matcher tk_match_end2 (one wave per document).  The default route for the JSON pattern is
// the flat pipeline with tk_flat_json_kernel; this is what its handed-back documents use, and the A / B form.
static int run_pipeline_seq(tk_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offs, uint64_t n_docs, uint64_t n_bytes,
                            int add_bos, int add_eos, hipStream_t s, uint64_t* n_ids) {
    int rc = reserve_doc_buffers(c, n_docs, n_bytes);
    if (rc != TK_OK) return rc;
    TkEncodeArgs a = encode_args(c, d_bytes, d_offs, n_docs, add_bos, add_eos);
    a.pattern = 1;
    c->n_flagged = 0;
    c->n_long_docs = n_docs;
    uint64_t total = 0;
    TK_HIP(c, hipEventRecord(c->ev[0], s));
    TK_HIP(c, hipEventRecord(c->ev[3], s));
    if (n_docs) {
        TK_HIP(c, tk_launch_iota((uint32_t*)c->defer_list.p, n_docs, s));
        if ((rc = run_pass2(c, a, d_offs, (uint32_t)n_docs, s, 8192)) != TK_OK) return rc;
    }
    TK_HIP(c, hipEventRecord(c->ev[1], s));
    if ((rc = scan_compact(c, a, s)) != TK_OK) return rc;
    TK_HIP(c, hipMemcpyAsync(&total, (uint64_t*)c->out_offs.p + n_docs, 8, hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&c->encode_ms, c->ev[0], c->ev[1]);
    (void)hipEventElapsedTime(&c->pipeline_ms, c->ev[0], c->ev[2]);
    *n_ids = total;
    return TK_OK;
}

// Pipeline choice: the flat pipeline, unless TK_PIPELINE=doc asks for the per-document kernels alone (tests / A-B runs).
int run_pipeline(tk_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offs, uint64_t n_docs, uint64_t n_bytes, int add_bos,
                 int add_eos, hipStream_t s, uint64_t* n_ids) {
    c->call = call_knobs();
    // (row f-3: TK_PIPELINE=doc selects the purely sequential form of the opt-in; the per-document window kernels only
    // know the hard-coded pattern)
    if (c->pattern == 1 && c->knobs.pipeline_forced == 2) return run_pipeline_seq(c, d_bytes, d_offs, n_docs, n_bytes, add_bos, add_eos, s, n_ids);
    c->use_flat = c->knobs.pipeline_forced != 2;
    if (c->use_flat) return run_pipeline_flat(c, d_bytes, d_offs, n_docs, n_bytes, add_bos, add_eos, s, n_ids);
    c->n_flagged = 0;
    return run_pipeline_doc(c, d_bytes, d_offs, n_docs, n_bytes, add_bos, add_eos, s, n_ids);
}
