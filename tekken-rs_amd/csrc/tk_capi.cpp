// tk_capi.cpp -- engine-level C ABI (include/tekken_hip.h): the context, its device tables, settings and diagnostics; the pinned
// pool of the result blocks.  The batch pipeline is tk_pipeline.cpp, the entries are tk_capi_encode / _decode / _spans / _dense.cpp.
//
// Replaces CoreBPE::new at reference src/tekkenizer.rs:125.  There is NO CPU fallback in the engine: without a HIP device
// every entry point fails with TK_ERR_NO_DEVICE.
#include <unordered_map>

#include "tk_ctx.h"

static thread_local std::string g_tls_err;

void tk_set_tls_error(const std::string& e) { g_tls_err = e; }
const std::string& tk_get_tls_error() { return g_tls_err; }

namespace {

// Pinned result buffers of tk_encode_batch / tk_decode_batch: a process-wide pool.  hipHostMalloc / hipHostFree cost
// hundreds of microseconds each (they map the pages into every device); a caller that encodes batch after batch gets the
// same blocks back from tk_free_result instead.  Bounded: at most 8 free blocks / 1 GiB are kept.
struct PinPool {
    std::mutex mu;
    std::unordered_map<void*, size_t> live;            // handed out
    std::vector<std::pair<void*, size_t>> free_blocks;
    size_t free_bytes = 0;
    void* get(size_t bytes) {
        if (bytes == 0) bytes = 1;
        {
            std::lock_guard<std::mutex> lock(mu);
            size_t best = free_blocks.size();
            for (size_t i = 0; i < free_blocks.size(); ++i)
                if (free_blocks[i].second >= bytes && free_blocks[i].second <= 4 * bytes + (1u << 16) &&
                    (best == free_blocks.size() || free_blocks[i].second < free_blocks[best].second))
                    best = i;
            if (best != free_blocks.size()) {
                std::pair<void*, size_t> b = free_blocks[best];
                free_blocks.erase(free_blocks.begin() + (long)best);
                free_bytes -= b.second;
                live[b.first] = b.second;
                return b.first;
            }
        }
        const size_t want = bytes < 4096 ? 4096 : bytes + bytes / 8;
        void* p = nullptr;
        if (hipHostMalloc(&p, want, hipHostMallocPortable) != hipSuccess) return nullptr;
        std::lock_guard<std::mutex> lock(mu);
        live[p] = want;
        return p;
    }
    void put(void* p) {
        if (!p) return;
        size_t sz = 0;
        {
            std::lock_guard<std::mutex> lock(mu);
            auto it = live.find(p);
            if (it == live.end()) { sz = 0; }
            else {
                sz = it->second;
                live.erase(it);
                if (free_blocks.size() < 8 && free_bytes + sz <= (1ull << 30)) {
                    free_blocks.push_back({p, sz});
                    free_bytes += sz;
                    return;
                }
            }
        }
        (void)hipHostFree(p);
    }
};
PinPool g_pin_pool;

}  // namespace

void* tk_pinned_get(size_t bytes) { return g_pin_pool.get(bytes); }
void tk_pinned_put(void* p) { g_pin_pool.put(p); }

int upload(tk_ctx* c, DevBuf& b, const void* src, size_t bytes) {
    TK_HIP(c, b.reserve(bytes ? bytes : 16));
    if (bytes) TK_HIP(c, hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    return TK_OK;
}

int check_n_docs(tk_ctx* c, uint64_t n_docs) {
    if (n_docs >= 0xFFFFFFF0ull) { c->err = "too many documents in one batch"; return TK_ERR_INVALID_ARG; }
    return TK_OK;
}
int enter_device(tk_ctx* c, uint64_t n_docs) {
    int rc = check_n_docs(c, n_docs);
    if (rc != TK_OK) return rc;
    TK_HIP(c, hipSetDevice(c->device));
    return TK_OK;
}

static int copy_out_fail(tk_ctx* c, CopyOut* a, int n, const std::string& err) {
    for (int i = 0; i < n; ++i) { tk_pinned_put(a[i].host); a[i].host = nullptr; }
    c->err = err;
    return TK_ERR_RUNTIME;
}
int pinned_blocks(tk_ctx* c, CopyOut* a, int n) {
    bool ok = true;
    for (int i = 0; i < n; ++i)
        if (a[i].selected) ok = (a[i].host = tk_pinned_get(a[i].bytes)) != nullptr && ok;
    return ok ? TK_OK : copy_out_fail(c, a, n, "hipHostMalloc failed");
}
int copy_out(tk_ctx* c, CopyOut* a, int n, const char* what) {
    int rc = pinned_blocks(c, a, n);
    if (rc != TK_OK) return rc;
    hipError_t e = hipSuccess;
    for (int i = 0; i < n && e == hipSuccess; ++i)
        if (a[i].selected && a[i].dev && a[i].bytes) e = hipMemcpyAsync(a[i].host, a[i].dev, a[i].bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? TK_OK : copy_out_fail(c, a, n, std::string(what) + " copy failed: " + hipGetErrorString(e));
}

int check_flags_and_args(tk_ctx* c, int checks, int known, bool null_arg) {
    if (checks & ~known) { c->err = "unknown check flag"; return TK_ERR_INVALID_ARG; }
    if (null_arg) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    return TK_OK;
}
int scan_u32(tk_ctx* c, DevBuf& workspace, const uint32_t* counts, uint64_t n, uint64_t* offs, hipStream_t s) {
    TK_HIP(c, workspace.reserve(scan_workspace_bytes(n)));
    TK_HIP(c, tk_launch_scan(counts, n, offs, (uint64_t*)workspace.p, s));
    return TK_OK;
}
int encode_batch_for_layout(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos, int add_eos,
                            int validate_utf8, DevBatch* dev, uint64_t* n_ids) {
    tk_result res;
    int rc = encode_batch(c, bytes, doc_offsets, n_docs, add_bos, add_eos, validate_utf8, &res, dev);
    if (rc != TK_OK) return rc;
    *n_ids = res.n_ids;
    tk_free_result(&res);
    return TK_OK;
}

// The environment knobs of a context, read once at its creation (the per-call ones: call_knobs, tk_pipeline.cpp)
static void read_knobs(TkKnobs& k) {
    if (const char* tl = getenv("TK_TAIL")) k.serial_tail = strcmp(tl, "serial") == 0;
    if (const char* dg = getenv("TK_DECODE_GROUPS")) k.no_decode_groups = strcmp(dg, "0") == 0;
    if (const char* gl = getenv("TK_DECODE_GROUP_LIMIT")) { const long long v = atoll(gl); if (v > 0 && v < 0x7FFFFF00ll) k.decode_group_limit = (uint32_t)v; }
    if (const char* fl = getenv("TK_FLAT_LONG")) k.no_flat_long = atoi(fl) == 0;
    if (const char* fl = getenv("TK_FLAT_LONG128")) k.no_flat_long128 = atoi(fl) == 0;
    if (const char* fl = getenv("TK_FLAT_CUT")) k.no_flat_cut = atoi(fl) == 0;
    if (const char* lm = getenv("TK_LONG_MIN")) k.long_min = (uint32_t)atoi(lm);
    if (const char* lz = getenv("TK_LONG_LAZY_MUL")) k.long_lazy_mul = (uint32_t)atoi(lz);
    if (const char* lf = getenv("TK_LONG_FORCE")) k.long_force = (uint32_t)atoi(lf);
    if (const char* ml = getenv("TK_MEMO_LOG2")) { const int v = atoi(ml); k.memo_log2 = v <= 0 ? 0u : (uint32_t)(v < 10 ? 10 : v > 26 ? 26 : v); }
    if (const char* mp = getenv("TK_MEMO_POLICY")) k.memo_policy = strcmp(mp, "always") == 0 ? 1 : 0;
    if (const char* tf = getenv("TK_TAIL_FOLD")) k.tail_fold = atoi(tf) != 0 ? 1 : 0;
    if (const char* fg = getenv("TK_TAIL_FOLD_MERGE")) k.fold_merge = atoi(fg) != 0;
    if (const char* fm = getenv("TK_TAIL_FOLD_MISS_MAX")) k.fold_miss_max = (uint32_t)atoll(fm);
    if (const char* fd = getenv("TK_TAIL_FOLD_DOC_MAX")) k.fold_doc_max = (uint32_t)atoll(fd);
    if (const char* pl = getenv("TK_PIPELINE"))  // "doc": per-document kernels only, "flat": chunk-per-wave kernel always
        k.pipeline_forced = strcmp(pl, "doc") == 0 ? 2 : strcmp(pl, "flat") == 0 ? 1 : 0;
}

extern "C" int tk_ctx_create(const uint8_t* token_bytes, const uint32_t* token_offsets, uint32_t n_ranks,
                             uint32_t num_special_tokens, uint32_t bos_id, uint32_t eos_id, int device_id,
                             tk_ctx** out_ctx) {
    if (!out_ctx) { g_tls_err = "out_ctx is NULL"; return TK_ERR_INVALID_ARG; }
    *out_ctx = nullptr;
    tk_ctx* c = new tk_ctx();
    std::string err;
    bool from_cache = false;   // TK_TABLE_CACHE_DIR: derived tables from a side file keyed by the rank table (row f-2)
    int rc = tk_build_tables_cached(token_bytes, token_offsets, n_ranks, num_special_tokens, bos_id, eos_id, c->host, err, &from_cache);
    if (rc != TK_OK) { g_tls_err = err; delete c; return rc; }

    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0) {
        g_tls_err = "no HIP device available (the tokenization path has no CPU fallback)";
        delete c;
        return TK_ERR_NO_DEVICE;
    }
    if (device_id < 0 || device_id >= n_dev) {
        g_tls_err = "device_id out of range";
        delete c;
        return TK_ERR_INVALID_ARG;
    }
    c->device = device_id;
    auto fail = [&](int code) {
        g_tls_err = c->err;
        tk_ctx_destroy(c);
        return code;
    };
    auto fail_msg = [&](const char* msg) { c->err = msg; return fail(TK_ERR_RUNTIME); };
    if (hipSetDevice(device_id) != hipSuccess) return fail_msg("hipSetDevice failed");
    if (hipStreamCreateWithFlags(&c->stream.h, hipStreamNonBlocking) != hipSuccess) return fail_msg("hipStreamCreate failed");
    for (Event& ev : c->ev)
        if (hipEventCreate(&ev.h) != hipSuccess) return fail_msg("hipEventCreate failed");
    if (hipStreamCreateWithFlags(&c->stream_b.h, hipStreamNonBlocking) != hipSuccess) return fail_msg("hipStreamCreate failed");
    for (Event& ev : c->ev_b)
        if (hipEventCreateWithFlags(&ev.h, hipEventDisableTiming) != hipSuccess) return fail_msg("hipEventCreate failed");
    read_knobs(c->knobs);
    if (c->h_pin.alloc(TKC_PIN_WORDS * 4, hipHostMallocDefault) != hipSuccess) return fail_msg("hipHostMalloc failed");

    const TkHostTables& h = c->host;
    if (getenv("TK_DEBUG_LOG"))
        fprintf(stderr, "[tk] tables%s: KEY8 %u slots, KEY16 %u slots (hash mode %u, %llu keys, %llu in their second slot, %llu slots flagged), PAIR %u buckets (%llu pairs)\n",
                from_cache ? " (from cache)" : "", h.key8_mask + 1, h.key_mask + 1, h.key_hash_mode, (unsigned long long)h.n_key, (unsigned long long)h.n_key_second,
                (unsigned long long)h.n_key_spill_slots, h.pair_mask + 1, (unsigned long long)h.n_pairs);
    // every table goes up and the device view points at it (the first failure stops the rest)
    c->dview = h.host_view();
    auto up = [&](DevBuf& b, const auto& v, auto*& view) {
        if (rc == TK_OK && (rc = upload(c, b, v.data(), v.size() * sizeof(v[0]))) == TK_OK) view = (std::remove_reference_t<decltype(view)>)b.p;
    };
    TkTablesView& dv = c->dview;
    up(c->t_uc1, h.uc_stage1, dv.uc_stage1);    up(c->t_uc2, h.uc_stage2, dv.uc_stage2);
    up(c->t_uc2a, h.uc2_stage1, dv.uc2_stage1); up(c->t_uc2b, h.uc2_stage2, dv.uc2_stage2);
    up(c->t_key8, h.key8_tab, dv.key8_tab);     up(c->t_key, h.key_tab, dv.key_tab);
    up(c->t_long, h.long_tab, dv.long_tab);     up(c->t_pair, h.pair_tab, dv.pair_tab);
    up(c->t_pair2, h.pair2, dv.pair2);          up(c->t_pairf, h.pair_filter, dv.pair_filter);
    up(c->t_ucbmp, h.uc_bmp, dv.uc_bmp);        up(c->t_key64, h.key64_tab, dv.key64_tab);
    up(c->t_cutk2, h.cut_k2, dv.cut_k2);        up(c->t_cutg3, h.cut_g3, dv.cut_g3);
    up(c->t_blob, h.blob, dv.blob);
    if (rc != TK_OK || (rc = upload(c, c->t_offs, h.offs.data(), h.offs.size() * 4)) != TK_OK) return fail(rc);

    if (c->counters.reserve(TKC_DEVICE_WORDS * 4) != hipSuccess) return fail_msg("hipMalloc(counters) failed");
    // the wave primitives (DPP wave shifts, bpermute) are checked once on the real device
    uint32_t bad = 1;
    if (hipMemsetAsync(c->ctr(TKC_WORK), 0, TKC_DEVICE_WORDS * 4, c->stream) != hipSuccess ||   // (the counters and the control words behind them)
        tk_launch_wave_selftest(c->ctr(TKC_WORK), c->stream) != hipSuccess ||
        hipMemcpyAsync(&bad, c->ctr(TKC_WORK), 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        c->err = std::string("wave self-test launch failed: ") + hipGetErrorString(hipGetLastError());
        return fail(TK_ERR_RUNTIME);
    }
    if (bad != 0) {
        c->err = "wave primitive self-test failed on this device (mask " + std::to_string(bad) + ")";
        return fail(TK_ERR_RUNTIME);
    }
    *out_ctx = c;
    return TK_OK;
}

extern "C" void tk_ctx_destroy(tk_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;                      // (every buffer, pinned block, stream and event of the context releases itself: tk_ctx.h)
}

extern "C" int tk_ctx_set_pattern(tk_ctx* c, int mode) {
    TK_ENTRY(c);
    if (mode != 0 && mode != 1) { c->err = "pattern mode must be 0 (hard-coded pattern) or 1 (tekken.json pattern)"; return TK_ERR_INVALID_ARG; }
    c->pattern = mode;
    return TK_OK;
}

extern "C" const char* tk_last_error(const tk_ctx* c) { return c ? c->err.c_str() : g_tls_err.c_str(); }

const TkHostTables* tk_ctx_host_tables(const tk_ctx* c) { return c ? &c->host : nullptr; }

extern "C" const uint32_t* tk_debug_marks(const tk_ctx* c) { return c ? c->dbg_mark.p : nullptr; }

extern "C" float tk_last_merge_ms(const tk_ctx* c) { return c ? c->merge_ms : 0.f; }

extern "C" int tk_last_timing(const tk_ctx* c, float* pipeline_ms, float* encode_kernel_ms) {
    if (!c) return TK_ERR_INVALID_ARG;
    if (pipeline_ms) *pipeline_ms = c->pipeline_ms;
    if (encode_kernel_ms) *encode_kernel_ms = c->encode_ms;
    return TK_OK;
}

extern "C" int tk_ctx_set_memo(tk_ctx* c, int log2_entries, int policy) {
    TK_ENTRY(c);
    if (log2_entries != 0 && (log2_entries < 10 || log2_entries > 26)) { c->err = "memo size: log2_entries must be 0 (off) or 10..26"; return TK_ERR_INVALID_ARG; }
    if (policy != 0 && policy != 1) { c->err = "memo policy must be 0 (adaptive) or 1 (always)"; return TK_ERR_INVALID_ARG; }
    c->knobs.memo_log2 = (uint32_t)log2_entries;
    c->knobs.memo_policy = policy;
    c->memo_pause = 0; c->memo_low_streak = 0;
    if (log2_entries == 0) {
        TK_HIP(c, hipSetDevice(c->device));
        TK_HIP(c, hipDeviceSynchronize());
        c->t_memo.release();
        c->t_memo_log.release();
        c->memo_have_log2 = 0;
    }
    return TK_OK;
}
extern "C" int tk_ctx_memo_clear(tk_ctx* c) {
    TK_ENTRY(c);
    c->memo_have_log2 = 0;         // (the next call that wants the table clears it on its own stream)
    c->memo_pause = 0; c->memo_low_streak = 0;
    return TK_OK;
}
extern "C" int tk_memo_stats(const tk_ctx* c, uint64_t* lookups_last, uint64_t* hits_last, uint64_t* lookups_total, uint64_t* hits_total, int* active_last) {
    if (!c) return TK_ERR_INVALID_ARG;
    if (lookups_last) *lookups_last = c->memo_lookups_last;
    if (hits_last) *hits_last = c->memo_hits_last;
    if (lookups_total) *lookups_total = c->memo_lookups_total;
    if (hits_total) *hits_total = c->memo_hits_total;
    if (active_last) *active_last = c->memo_active_last ? 1 : 0;
    return TK_OK;
}

extern "C" uint64_t tk_small_path_calls(const tk_ctx* c) { return c ? c->n_small_calls : 0; }
extern "C" uint64_t tk_round_path_docs(const tk_ctx* c) { return c ? c->n_round_docs : 0; }
extern "C" uint64_t tk_long_piece_records(const tk_ctx* c) { return c ? c->n_long_recs : 0; }
extern "C" uint64_t tk_cut_chunks(const tk_ctx* c) { return c ? c->n_cut_chunks : 0; }
extern "C" uint64_t tk_last_host_syncs(const tk_ctx* c) { return c ? c->host_syncs : 0; }

extern "C" int tk_last_stats(const tk_ctx* c, uint64_t* n_long_docs, uint64_t* reserved) {
    if (!c) return TK_ERR_INVALID_ARG;
    if (n_long_docs) *n_long_docs = c->n_long_docs;
    if (reserved) *reserved = c->n_flagged;  // documents the flat path handed back to the per-document kernels
    return TK_OK;
}

extern "C" int tk_ctx_set_special_tokens(tk_ctx* c, const uint8_t* blob, const uint32_t* offs, uint32_t n) {
    TK_ENTRY(c);
    if (!offs || n != c->host.num_special || (!blob && n && offs[n])) {
        c->err = "special token strings: need exactly num_special_tokens entries";
        return TK_ERR_INVALID_ARG;
    }
    TK_HIP(c, hipSetDevice(c->device));
    int rc;
    if ((rc = upload(c, c->t_spblob, blob, n ? offs[n] : 0)) || (rc = upload(c, c->t_spoffs, offs, ((size_t)n + 1) * 4))) return rc;
    c->have_specials = true;
    // (the host copy the specials pass builds its byte trie from, at its first call behind this one)
    c->specials.h_blob.assign(blob, blob + (n ? offs[n] : 0));
    c->specials.h_offs.assign(offs, offs + n + 1);
    c->specials.trie_ready = false;
    return TK_OK;
}
