// tk_capi_encode.cpp -- the encode entries of the C ABI (include/tekken_hip.h): text on the device or on the host, one string,
// small batches in one launch, pipelined ingestion, the 18-bit wire format of ids, tk_split_batch.  The pipeline they run is
// tk_pipeline.cpp.  Replaces Tekkenizer::encode at reference src/tekkenizer.rs:378-405.
#include "tk_ctx.h"

// (the body of tk_encode_batch_device; the caller holds c->mu)
static int encode_device(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes, int add_bos,
                         int add_eos, void* hip_stream, void** d_ids, void** d_out_offsets, uint64_t* n_ids) {
    if (!d_doc_offsets || (!d_bytes && n_bytes) || !d_ids || !d_out_offsets || !n_ids) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    int rc = enter_device(c, n_docs);
    if (rc != TK_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;  // NULL = HIP's null stream: ordered after the caller's own work on it
    rc = run_pipeline(c, (const uint8_t*)d_bytes, (const uint64_t*)d_doc_offsets, n_docs, n_bytes, add_bos, add_eos, s, n_ids);
    if (rc != TK_OK) return rc;
    *d_ids = c->out_ids.p;
    *d_out_offsets = c->out_offs.p;
    return TK_OK;
}

extern "C" int tk_encode_batch_device(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs,
                                      uint64_t n_bytes, int add_bos, int add_eos, void* hip_stream, void** d_ids,
                                      void** d_out_offsets, uint64_t* n_ids) {
    TK_ENTRY(c);
    return encode_device(c, d_bytes, d_doc_offsets, n_docs, n_bytes, add_bos, add_eos, hip_stream, d_ids, d_out_offsets, n_ids);
}

// The same entry with the checks a host caller gets from tk_encode_batch ("C callers get a `validate` flag"):
// TK_CHECK_OFFSETS -- d_doc_offsets[0] == 0, non-decreasing, [n_docs] == n_bytes, or TK_ERR_INVALID_ARG (without it a bad offset
// array is out-of-bounds indexing on the device); TK_CHECK_UTF8 -- every document is well-formed UTF-8 on its own (which includes:
// no document starts inside a code point), or TK_ERR_INVALID_UTF8; implies the offsets check.  One small kernel and one host wait
// each, before anything else runs.
extern "C" int tk_encode_batch_device_ex(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs,
                                         uint64_t n_bytes, int add_bos, int add_eos, int checks, void* hip_stream, void** d_ids,
                                         void** d_out_offsets, uint64_t* n_ids) {
    TK_ENTRY(c);
    if (checks & ~(TK_CHECK_OFFSETS | TK_CHECK_UTF8)) { c->err = "unknown check flag"; return TK_ERR_INVALID_ARG; }
    return encode_device_checked(c, d_bytes, d_doc_offsets, n_docs, n_bytes, add_bos, add_eos, checks, hip_stream, d_ids, d_out_offsets, n_ids);
}

// one check kernel over the batch on stream s: the number of documents it refuses, through TKC_INVALID and ONE host wait
template <class Launch> static int count_invalid(tk_ctx* c, hipStream_t s, uint32_t* bad, Launch launch) {
    uint32_t* d_bad = c->ctr(TKC_INVALID);
    TK_HIP(c, hipMemsetAsync(d_bad, 0, 4, s));
    TK_HIP(c, launch(d_bad));
    TK_HIP(c, hipMemcpyAsync(bad, d_bad, 4, hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipStreamSynchronize(s));
    return TK_OK;
}
static int validate_utf8_device(tk_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offs, uint64_t n_docs, hipStream_t s) {
    uint32_t bad = 0;
    int rc = count_invalid(c, s, &bad, [&](uint32_t* d_bad) { return tk_launch_validate(d_bytes, d_offs, n_docs, d_bad, s); });
    if (rc != TK_OK) return rc;
    if (bad) { c->err = std::to_string(bad) + " document(s) are not valid UTF-8"; return TK_ERR_INVALID_UTF8; }
    return TK_OK;
}

int check_text_device(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes, int checks, void* hip_stream) {
    if (!d_doc_offsets || (!d_bytes && n_bytes)) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    int rc = enter_device(c, n_docs);
    if (rc != TK_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    uint32_t bad = 0;
    rc = count_invalid(c, s, &bad, [&](uint32_t* d_bad) { return tk_launch_check_offsets((const uint64_t*)d_doc_offsets, n_docs, n_bytes, d_bad, s); });
    if (rc != TK_OK) return rc;
    if (bad) { c->err = "doc_offsets must start at 0, be non-decreasing and end at n_bytes (" + std::to_string(bad) + " violation(s))"; return TK_ERR_INVALID_ARG; }
    if ((checks & TK_CHECK_UTF8) && (rc = validate_utf8_device(c, (const uint8_t*)d_bytes, (const uint64_t*)d_doc_offsets, n_docs, s)) != TK_OK) return rc;
    return TK_OK;
}

// (the body of tk_encode_batch_device_ex; the caller holds c->mu and has refused unknown flags)
int encode_device_checked(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes, int add_bos,
                          int add_eos, int checks, void* hip_stream, void** d_ids, void** d_out_offsets, uint64_t* n_ids) {
    if (checks) {
        const int rc = check_text_device(c, d_bytes, d_doc_offsets, n_docs, n_bytes, checks, hip_stream);
        if (rc != TK_OK) return rc;
    }
    return encode_device(c, d_bytes, d_doc_offsets, n_docs, n_bytes, add_bos, add_eos, hip_stream, d_ids, d_out_offsets, n_ids);
}

int check_offsets(tk_ctx* c, const uint64_t* doc_offsets, uint64_t n_docs) {
    if (doc_offsets[0] != 0) { c->err = "doc_offsets[0] must be 0"; return TK_ERR_INVALID_ARG; }
    for (uint64_t d = 0; d < n_docs; ++d)
        if (doc_offsets[d + 1] < doc_offsets[d]) { c->err = "doc_offsets must be non-decreasing"; return TK_ERR_INVALID_ARG; }
    return TK_OK;
}

static int stage_input(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs) {
    const uint64_t n_bytes = doc_offsets[n_docs];
    TK_HIP(c, c->in_bytes.reserve(n_bytes + 64));
    TK_HIP(c, c->in_offs.reserve((n_docs + 1) * 8));
    if (n_bytes) TK_HIP(c, hipMemcpyAsync(c->in_bytes.p, bytes, n_bytes, hipMemcpyHostToDevice, c->stream));
    TK_HIP(c, hipMemcpyAsync(c->in_offs.p, doc_offsets, (n_docs + 1) * 8, hipMemcpyHostToDevice, c->stream));
    return TK_OK;
}

// ---- small batches in ONE launch (tk_small_kernel).  The reference's own signature is one &str per call
// (src/tekkenizer.rs:378-405): through the batch pipeline that is about ten launches, two copies and a host sync. ----
static bool small_eligible(const tk_ctx* c, uint64_t n_docs, uint64_t n_bytes) {
    static const bool off = getenv("TK_NO_SMALL_PATH") != nullptr;
    return !off && c->pattern == 0 && c->knobs.pipeline_forced == 0 && n_docs >= 1 && n_docs <= TK_SMALL_MAX_DOCS && n_bytes <= TK_SMALL_MAX_BYTES;
}

static int small_prepare(tk_ctx* c) {
    if (c->small_ready) return TK_OK;
    // (ready only once EVERY step below went through: a call that fails half-way leaves the flag clear, and the next call
    // starts over with what is still missing instead of running on null pointers)
    const size_t in_bytes = TK_SMALL_MAX_BYTES + (TK_SMALL_MAX_DOCS + 1) * 8;
    const size_t out_bytes = (size_t)(TK_SMALL_STATUS_WORD + 4) * 4;
    if (!c->hs_in) TK_HIP(c, c->hs_in.alloc(in_bytes, hipHostMallocMapped));
    if (!c->hs_out) TK_HIP(c, c->hs_out.alloc(out_bytes, hipHostMallocMapped));
    TK_HIP(c, hipHostGetDevicePointer(&c->ds_in, c->hs_in, 0));
    TK_HIP(c, hipHostGetDevicePointer(&c->ds_out, c->hs_out, 0));
    TK_HIP(c, c->staging.reserve((size_t)(TK_SMALL_IDS_CAP + 64) * 4));
    TK_HIP(c, c->counts.reserve((TK_SMALL_MAX_DOCS + 1) * 4));
    TK_HIP(c, c->in_bytes.reserve(TK_SMALL_MAX_BYTES + 64));
    TK_HIP(c, c->s_offs.reserve((TK_SMALL_MAX_DOCS + 1) * 8));
    c->small_ready = true;
    return TK_OK;
}

// hs_in holds the text and (behind it) the document offsets.  *fallback = true: a document needs pass 2 (a piece that
// does not fit a window) -- nothing was produced, the caller takes the batch pipeline.  Otherwise the ids are in
// hs_out[0 .. *n_ids) and the id offsets at hs_out + TK_SMALL_OUT_OFFS_WORD when this returns.
static int run_small(tk_ctx* c, uint64_t n_docs, uint64_t n_bytes, int add_bos, int add_eos, uint64_t* n_ids, bool* fallback) {
    uint64_t* h_offs = (uint64_t*)(c->hs_in + TK_SMALL_MAX_BYTES);
    volatile uint32_t* status = (volatile uint32_t*)(c->hs_out + TK_SMALL_STATUS_WORD);
    TkEncodeArgs a = encode_args(c, nullptr, nullptr, n_docs, add_bos, add_eos);
    a.work_counter = a.defer_count = a.defer_list = nullptr;   // (one workgroup, nothing deferred: status[0] says so instead)
    // A few short strings are read by the kernel straight from pinned host memory (one PCIe round trip per window); beyond
    // that the copy engine is the better reader.
    if (n_bytes <= 4096 && n_docs <= 16) {
        a.bytes = (const uint8_t*)c->ds_in;
        a.doc_offs = (const uint64_t*)((const uint8_t*)c->ds_in + TK_SMALL_MAX_BYTES);
    } else {
        if (n_bytes) TK_HIP(c, hipMemcpyAsync(c->in_bytes.p, c->hs_in, n_bytes, hipMemcpyHostToDevice, c->stream));
        TK_HIP(c, hipMemcpyAsync(c->s_offs.p, h_offs, (n_docs + 1) * 8, hipMemcpyHostToDevice, c->stream));
        a.bytes = (const uint8_t*)c->in_bytes.p;
        a.doc_offs = (const uint64_t*)c->s_offs.p;
    }
    status[0] = 0xFFFFFFFFu;
    uint32_t* d_out = (uint32_t*)c->ds_out;
    TK_HIP(c, tk_launch_small(a, d_out, (uint64_t*)(d_out + TK_SMALL_OUT_OFFS_WORD), d_out + TK_SMALL_STATUS_WORD, c->stream));
    TK_HIP(c, hipStreamSynchronize(c->stream));
    if (status[0] == 0xFFFFFFFFu) { c->err = "the small-batch kernel did not report"; return TK_ERR_RUNTIME; }
    *fallback = status[0] != 0u;
    *n_ids = status[1];
    if (!*fallback) {
        c->n_small_calls++;
        c->n_flagged = 0; c->n_long_docs = 0; c->pipeline_ms = 0.f; c->encode_ms = 0.f;
    }
    return TK_OK;
}

/* Tekkenizer::encode for ONE &str with a caller-owned output (the reference's own call shape): no allocation, and for
 * texts of up to 64 KiB one kernel launch.  ids_capacity >= len + 2 always suffices. */
extern "C" int tk_encode_one(tk_ctx* c, const uint8_t* text, uint64_t len, int add_bos, int add_eos, uint32_t* ids_out,
                             uint64_t ids_capacity, uint64_t* n_ids_out) {
    TK_ENTRY(c);
    if ((!text && len) || !n_ids_out || (!ids_out && ids_capacity)) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    *n_ids_out = 0;
    TK_HIP(c, hipSetDevice(c->device));
    uint64_t n_ids = 0;
    if (small_eligible(c, 1, len)) {
        int rc = small_prepare(c);
        if (rc != TK_OK) return rc;
        if (len) memcpy(c->hs_in, text, len);
        uint64_t* h_offs = (uint64_t*)(c->hs_in + TK_SMALL_MAX_BYTES);
        h_offs[0] = 0; h_offs[1] = len;
        bool fallback = false;
        if ((rc = run_small(c, 1, len, add_bos, add_eos, &n_ids, &fallback)) != TK_OK) return rc;
        if (!fallback) {
            *n_ids_out = n_ids;
            if (n_ids > ids_capacity) { c->err = "ids_out is too small"; return TK_ERR_INVALID_ARG; }
            if (n_ids) memcpy(ids_out, c->hs_out, n_ids * 4);
            return TK_OK;
        }
    }
    const uint64_t offs[2] = {0, len};
    int rc = stage_input(c, text, offs, 1);
    if (rc != TK_OK) return rc;
    rc = run_pipeline(c, (const uint8_t*)c->in_bytes.p, (const uint64_t*)c->in_offs.p, 1, len, add_bos, add_eos, c->stream, &n_ids);
    if (rc != TK_OK) return rc;
    *n_ids_out = n_ids;
    if (n_ids > ids_capacity) { c->err = "ids_out is too small"; return TK_ERR_INVALID_ARG; }
    if (n_ids) TK_HIP(c, hipMemcpy(ids_out, c->out_ids.p, n_ids * 4, hipMemcpyDeviceToHost));
    return TK_OK;
}

// (the body of tk_encode_batch; the caller holds c->mu.  dev: optional)
int encode_batch(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos, int add_eos,
                 int validate_utf8, tk_result* out, DevBatch* dev) {
    if (!doc_offsets || !out || (!bytes && doc_offsets[n_docs])) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    int rc = check_n_docs(c, n_docs);
    if (rc != TK_OK) return rc;
    memset(out, 0, sizeof(*out));
    if ((rc = check_offsets(c, doc_offsets, n_docs)) != TK_OK) return rc;
    TK_HIP(c, hipSetDevice(c->device));
    const uint64_t n_bytes = doc_offsets[n_docs];
    if (small_eligible(c, n_docs, n_bytes)) {
        // one launch for the whole batch; UTF-8 is validated on the host (same RFC 3629 rules as tk_validate_kernel)
        if (validate_utf8) {
            uint64_t bad = 0;
            for (uint64_t d = 0; d < n_docs; ++d)
                if (!tekken::utf8_valid(bytes + doc_offsets[d], doc_offsets[d + 1] - doc_offsets[d])) ++bad;
            if (bad) { c->err = std::to_string(bad) + " document(s) are not valid UTF-8"; return TK_ERR_INVALID_UTF8; }
        }
        if ((rc = small_prepare(c)) != TK_OK) return rc;
        if (n_bytes) memcpy(c->hs_in, bytes, n_bytes);
        memcpy(c->hs_in + TK_SMALL_MAX_BYTES, doc_offsets, (n_docs + 1) * 8);
        uint64_t n_ids = 0;
        bool fallback = false;
        if ((rc = run_small(c, n_docs, n_bytes, add_bos, add_eos, &n_ids, &fallback)) != TK_OK) return rc;
        if (!fallback) {
            CopyOut h[2] = {{nullptr, (n_ids ? n_ids : 1) * 4, nullptr}, {nullptr, (n_docs + 1) * 8, nullptr}};
            if ((rc = pinned_blocks(c, h, 2)) != TK_OK) return rc;
            if (n_ids) memcpy(h[0].host, c->hs_out, n_ids * 4);
            memcpy(h[1].host, c->hs_out + TK_SMALL_OUT_OFFS_WORD, (n_docs + 1) * 8);
            out->ids = (uint32_t*)h[0].host; out->offsets = (uint64_t*)h[1].host; out->n_ids = n_ids; out->n_docs = n_docs;
            if (dev) *dev = DevBatch{(const uint8_t*)c->ds_in, (const uint64_t*)((const uint8_t*)c->ds_in + TK_SMALL_MAX_BYTES),
                                     (const uint32_t*)c->ds_out, (const uint64_t*)((const uint32_t*)c->ds_out + TK_SMALL_OUT_OFFS_WORD)};
            return TK_OK;
        }
    }
    if ((rc = stage_input(c, bytes, doc_offsets, n_docs)) != TK_OK) return rc;
    if (validate_utf8 && (rc = validate_utf8_device(c, (const uint8_t*)c->in_bytes.p, (const uint64_t*)c->in_offs.p, n_docs, c->stream)) != TK_OK) return rc;
    uint64_t n_ids = 0;
    rc = run_pipeline(c, (const uint8_t*)c->in_bytes.p, (const uint64_t*)c->in_offs.p, n_docs, n_bytes, add_bos,
                      add_eos, c->stream, &n_ids);
    if (rc != TK_OK) return rc;
    // (pinned buffers from the process-wide pool: no hipHostMalloc per call once the pool is warm)
    CopyOut h[2] = {{n_ids ? c->out_ids.p : nullptr, (n_ids ? n_ids : 1) * 4, nullptr}, {c->out_offs.p, (n_docs + 1) * 8, nullptr}};
    if ((rc = copy_out(c, h, 2, "result")) != TK_OK) return rc;
    out->ids = (uint32_t*)h[0].host;
    out->offsets = (uint64_t*)h[1].host;
    out->n_ids = n_ids;
    out->n_docs = n_docs;
    if (dev) *dev = DevBatch{(const uint8_t*)c->in_bytes.p, (const uint64_t*)c->in_offs.p, (const uint32_t*)c->out_ids.p, (const uint64_t*)c->out_offs.p};
    return TK_OK;
}

extern "C" int tk_encode_batch(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs,
                               int add_bos, int add_eos, int validate_utf8, tk_result* out) {
    TK_ENTRY(c);
    return encode_batch(c, bytes, doc_offsets, n_docs, add_bos, add_eos, validate_utf8, out, nullptr);
}

// ---- pipelined ingestion (row f-4) ----
extern "C" void* tk_host_alloc(size_t bytes) {
    void* p = nullptr;
    return hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}
extern "C" void tk_host_free(void* p) { if (p) (void)hipHostFree(p); }

extern "C" int tk_encode_batch_pipelined(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs,
                                         int add_bos, int add_eos, uint64_t slice_bytes, uint32_t* ids_out, uint64_t ids_capacity,
                                         uint64_t* offsets_out, uint64_t* n_ids_out) {
    TK_ENTRY(c);
    if (!doc_offsets || !offsets_out || !n_ids_out || (!ids_out && ids_capacity) || (!bytes && doc_offsets[n_docs])) {
        c->err = "null argument";
        return TK_ERR_INVALID_ARG;
    }
    int rc = check_n_docs(c, n_docs);
    if (rc != TK_OK) return rc;
    *n_ids_out = 0;
    if ((rc = check_offsets(c, doc_offsets, n_docs)) != TK_OK) return rc;
    TK_HIP(c, hipSetDevice(c->device));
    if (!c->s_in) {
        TK_HIP(c, hipStreamCreateWithFlags(&c->s_in.h, hipStreamNonBlocking));
        TK_HIP(c, hipStreamCreateWithFlags(&c->s_out.h, hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) {
            TK_HIP(c, hipEventCreateWithFlags(&c->ev_in[i].h, hipEventDisableTiming));
            TK_HIP(c, hipEventCreateWithFlags(&c->ev_out[i].h, hipEventDisableTiming));
        }
    }
    if (slice_bytes == 0) slice_bytes = 32ull << 20;
    // slices of whole documents: [cut[k], cut[k + 1])
    std::vector<uint64_t> cut(1, 0);
    uint64_t max_bytes = 0, max_docs = 0;
    for (uint64_t d = 0; d < n_docs;) {
        const uint64_t b0 = doc_offsets[d];
        uint64_t e = d + 1;                               // at least one document per slice, however long it is
        while (e < n_docs && doc_offsets[e + 1] - b0 <= slice_bytes && e - d < (1ull << 22)) ++e;
        cut.push_back(e);
        if (doc_offsets[e] - b0 > max_bytes) max_bytes = doc_offsets[e] - b0;
        if (e - d > max_docs) max_docs = e - d;
        d = e;
    }
    const size_t n_slices = cut.size() - 1;
    offsets_out[0] = 0;
    if (n_slices == 0) return TK_OK;
    // staging: two input sets, two output sets (run_pipeline writes c->out_ids / c->out_offs: the sets are swapped per slice)
    DevBuf* inb[2] = {&c->in_bytes, &c->in_bytes2};
    DevBuf* ino[2] = {&c->in_offs, &c->in_offs2};
    for (int i = 0; i < 2; ++i) {
        TK_HIP(c, inb[i]->reserve(max_bytes + 64));
        TK_HIP(c, ino[i]->reserve((max_docs + 1) * 8));
    }
    TK_HIP(c, c->out_ids.reserve((max_bytes + 2 * max_docs + 64) * 4));
    TK_HIP(c, c->out_ids2.reserve((max_bytes + 2 * max_docs + 64) * 4));
    TK_HIP(c, c->out_offs.reserve((max_docs + 1) * 8));
    TK_HIP(c, c->out_offs2.reserve((max_docs + 1) * 8));
    if (c->h_offs_cap < max_docs + 1) {
        for (int i = 0; i < 2; ++i) TK_HIP(c, c->h_offs_stage[i].alloc((max_docs + 1) * 8, hipHostMallocDefault));
        c->h_offs_cap = max_docs + 1;
    }
    auto upload_slice = [&](size_t k) -> int {            // host -> device of slice k on the input stream
        const int b = (int)(k & 1);
        const uint64_t d0 = cut[k], d1 = cut[k + 1], b0 = doc_offsets[d0], nb = doc_offsets[d1] - b0;
        uint64_t* ho = c->h_offs_stage[b];
        for (uint64_t d = d0; d <= d1; ++d) ho[d - d0] = doc_offsets[d] - b0;
        if (nb) TK_HIP(c, hipMemcpyAsync(inb[b]->p, bytes + b0, nb, hipMemcpyHostToDevice, c->s_in));
        TK_HIP(c, hipMemcpyAsync(ino[b]->p, ho, (d1 - d0 + 1) * 8, hipMemcpyHostToDevice, c->s_in));
        TK_HIP(c, hipEventRecord(c->ev_in[b], c->s_in));
        return TK_OK;
    };
    uint64_t id_base = 0;
    std::vector<uint64_t> slice_ids(n_slices, 0);
    float pipe_ms = 0.f, enc_ms = 0.f;
    uint64_t flagged = 0, longd = 0;
    // the offsets staging of slice k is rewritten by upload_slice(k + 2): that copy must have been consumed -- it has, the
    // kernels of slice k (which waited for it) are complete when run_pipeline returns
    // (inside the loop a failing HIP call sets rc and leaves the loop: the drain below must run whatever happened)
#define TK_HIP_BRK(call) { hipError_t _e = (call); if (_e != hipSuccess) { c->err = std::string(#call) + ": " + hipGetErrorString(_e); rc = TK_ERR_RUNTIME; break; } }
    rc = upload_slice(0);
    for (size_t k = 0; rc == TK_OK && k < n_slices; ++k) {
        const int b = (int)(k & 1);
        if (k + 1 < n_slices && (rc = upload_slice(k + 1)) != TK_OK) break;
        const uint64_t d0 = cut[k], d1 = cut[k + 1], nb = doc_offsets[d1] - doc_offsets[d0];
        TK_HIP_BRK(hipStreamWaitEvent(c->stream, c->ev_in[b], 0));
        if (k >= 2) TK_HIP_BRK(hipStreamWaitEvent(c->stream, c->ev_out[b], 0));   // the ids of slice k - 2 have left this output set
        uint64_t n_ids = 0;
        rc = run_pipeline(c, (const uint8_t*)inb[b]->p, (const uint64_t*)ino[b]->p, d1 - d0, nb, add_bos, add_eos, c->stream, &n_ids);
        if (rc != TK_OK) break;
        pipe_ms += c->pipeline_ms; enc_ms += c->encode_ms; flagged += c->n_flagged; longd += c->n_long_docs;
        slice_ids[k] = n_ids;
        if (id_base + n_ids > ids_capacity) {
            *n_ids_out = id_base + n_ids;
            c->err = "ids_out is too small";
            rc = TK_ERR_INVALID_ARG;
            break;
        }
        // device -> host on the output stream (run_pipeline returned after its stream drained: the ids are complete)
        if (n_ids) TK_HIP_BRK(hipMemcpyAsync(ids_out + id_base, c->out_ids.p, n_ids * 4, hipMemcpyDeviceToHost, c->s_out));
        TK_HIP_BRK(hipMemcpyAsync(offsets_out + d0 + 1, (const uint64_t*)c->out_offs.p + 1, (d1 - d0) * 8, hipMemcpyDeviceToHost, c->s_out));
        TK_HIP_BRK(hipEventRecord(c->ev_out[b], c->s_out));
        std::swap(c->out_ids, c->out_ids2);
        std::swap(c->out_offs, c->out_offs2);
        id_base += n_ids;
    }
#undef TK_HIP_BRK
    // drain the copy streams whatever happened (buffers must not be in flight when the call returns)
    (void)hipStreamSynchronize(c->s_in);
    hipError_t e = hipStreamSynchronize(c->s_out);
    if (rc != TK_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    if (e != hipSuccess) { c->err = std::string("result copy failed: ") + hipGetErrorString(e); return TK_ERR_RUNTIME; }
    // slice-relative id offsets -> batch offsets
    uint64_t base = 0;
    for (size_t k = 0; k < n_slices; ++k) {
        if (base)
            for (uint64_t d = cut[k] + 1; d <= cut[k + 1]; ++d) offsets_out[d] += base;
        base += slice_ids[k];
    }
    c->pipeline_ms = pipe_ms; c->encode_ms = enc_ms; c->n_flagged = flagged; c->n_long_docs = longd;
    *n_ids_out = id_base;
    return TK_OK;
}

// ---- 18-bit wire format of ids (multi-GPU gather) ----
extern "C" uint64_t tk_ids18_bytes(uint64_t n_ids) { return ((2 * n_ids + 3) & ~3ull) + 4 * ((n_ids + 15) / 16); }

extern "C" int tk_pack_ids18_device(tk_ctx* c, const void* d_ids, uint64_t n_ids, void* d_packed, void* hip_stream) {
    TK_ENTRY(c);
    if ((!d_ids || !d_packed) && n_ids) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    TK_HIP(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;
    uint32_t* d_bad = c->ctr(TKC_PACK_BAD);
    TK_HIP(c, hipMemsetAsync(d_bad, 0, 4, s));
    TK_HIP(c, tk_launch_pack18((const uint32_t*)d_ids, n_ids, d_packed, d_bad, s));
    TK_HIP(c, hipMemcpyAsync(c->h_pin + TKC_PACK_BAD, d_bad, 4, hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipStreamSynchronize(s));
    if (c->h_pin[TKC_PACK_BAD]) { c->err = "an id does not fit 18 bits"; return TK_ERR_INVALID_ARG; }
    return TK_OK;
}

extern "C" int tk_unpack_ids18_device(tk_ctx* c, const void* d_packed, uint64_t n_ids, void* d_ids, void* hip_stream) {
    TK_ENTRY(c);
    if ((!d_ids || !d_packed) && n_ids) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    TK_HIP(c, hipSetDevice(c->device));
    TK_HIP(c, tk_launch_unpack18(d_packed, n_ids, (uint32_t*)d_ids, (hipStream_t)hip_stream));
    return TK_OK;
}

extern "C" void tk_free_result(tk_result* r) {
    if (!r) return;
    tk_pinned_put(r->ids);
    tk_pinned_put(r->offsets);
    memset(r, 0, sizeof(*r));
}

extern "C" int tk_split_batch(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs,
                              uint8_t* out_is_start) {
    TK_ENTRY(c);
    if (!doc_offsets || (!bytes && doc_offsets[n_docs]) || !out_is_start) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    int rc = check_offsets(c, doc_offsets, n_docs);
    if (rc != TK_OK) return rc;
    TK_HIP(c, hipSetDevice(c->device));
    const uint64_t n_bytes = doc_offsets[n_docs];
    if ((rc = stage_input(c, bytes, doc_offsets, n_docs)) != TK_OK) return rc;
    TK_HIP(c, c->dbg.reserve(n_bytes + 64));
    TK_HIP(c, c->staging.reserve((n_bytes + 2 * n_docs + 64) * 4));
    TK_HIP(c, c->counts.reserve((n_docs + 1) * 4));
    TK_HIP(c, c->defer_list.reserve((n_docs + 1) * 4));
    TkEncodeArgs a = encode_args(c, (const uint8_t*)c->in_bytes.p, (const uint64_t*)c->in_offs.p, n_docs, 0, 0);
    a.dbg_starts = (uint8_t*)c->dbg.p;
    a.split_only = 1;
    TK_HIP(c, hipMemsetAsync(c->ctr(TKC_WORK), 0, TKC_CLEARED * 4, c->stream));
    TK_HIP(c, hipMemsetAsync(c->dbg.p, 0, n_bytes + 64, c->stream));
    uint64_t want = (n_docs + 7) / 8;
    TK_HIP(c, tk_launch_encode(a, 2, (uint32_t)(want < 8192 ? (want ? want : 1) : 8192), c->stream));
    if (n_bytes) TK_HIP(c, hipMemcpyAsync(out_is_start, c->dbg.p, n_bytes, hipMemcpyDeviceToHost, c->stream));
    TK_HIP(c, hipStreamSynchronize(c->stream));
    return TK_OK;
}
