// tk_capi_join.cpp -- chat batches (include/tekken_hip.h tk_join_from_ids_device and the entries around it; csrc/tk_join.hip):
// the ids of text parts, encoded one by one, joined with control ids into one stream per conversation, with labels and the part
// index of every element.
#include "tk_capi_layout.h"

#define TK_JOIN_ALL_FLAGS (TK_JOIN_LABELS | TK_JOIN_PART_INDEX)

// what can be refused before anything is on the device (step 6 of the definition)
int join_check_args(tk_ctx* c, uint64_t n_parts, uint64_t n_convs, const tk_join_opts* o) {
    if (!o) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    if (o->flags & ~(uint32_t)TK_JOIN_ALL_FLAGS) { c->err = "unknown join flag"; return TK_ERR_INVALID_ARG; }
    int rc = check_n_docs(c, n_parts);
    if (rc != TK_OK) return rc;
    if ((rc = check_n_docs(c, n_convs)) != TK_OK) return rc;
    if (n_convs == 0 && n_parts) { c->err = "join: parts without a conversation"; return TK_ERR_INVALID_ARG; }
    return TK_OK;
}

// the two messages of TK_CHECK_PARTS, the same from the host and the device check
static int bad_conv(tk_ctx* c, uint64_t conv, uint64_t n_parts) {
    c->err = "conv_offsets must start at 0, be non-decreasing and end at n_parts (" + std::to_string(n_parts) +
             "): first violation at conversation " + std::to_string(conv);
    return TK_ERR_INVALID_ARG;
}
static int bad_ctrl(tk_ctx* c, uint64_t part, uint32_t id) {
    c->err = "part " + std::to_string(part) + ": control id " + std::to_string(id) + " is neither TK_JOIN_NONE nor below num_special_tokens (" +
             std::to_string(c->host.num_special) + ")";
    return TK_ERR_INVALID_ARG;
}

static int check_parts_host(tk_ctx* c, const uint32_t* ctrl, const uint64_t* conv, uint64_t P, uint64_t C) {
    for (uint64_t i = 0; i <= C; ++i)
        if ((i == 0 && conv[0] != 0) || (i < C && conv[i + 1] < conv[i]) || (i == C && conv[C] != P)) return bad_conv(c, i, P);
    for (uint64_t p = 0; p < P; ++p)
        if (ctrl[p] != TK_JOIN_NONE && ctrl[p] >= c->host.num_special) return bad_ctrl(c, p, ctrl[p]);
    return TK_OK;
}

// TK_CHECK_PARTS on the device: one small kernel and one wait, before any buffer of an earlier result is given up
static int check_parts_device(tk_ctx* c, const uint32_t* d_ctrl, const uint64_t* d_conv, uint64_t P, uint64_t C, hipStream_t s) {
    TK_HIP(c, c->join.stat.reserve(64));
    TkJoinArgs a;
    memset(&a, 0, sizeof(a));
    a.n_parts = P; a.n_convs = C; a.ctrl = d_ctrl; a.conv_offs = d_conv; a.num_special = c->host.num_special;
    a.stat = (unsigned long long*)c->join.stat.p;
    unsigned long long bad[2] = {0, 0};
    TK_HIP(c, hipMemsetAsync(a.stat + 1, 0xFF, 16, s));
    TK_HIP(c, tk_launch_join_check(a, s));
    TK_HIP(c, hipMemcpyAsync(bad, a.stat + 1, 16, hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipStreamSynchronize(s));
    if (bad[0] != ~0ull) return bad_conv(c, bad[0], P);
    if (bad[1] != ~0ull) {
        uint32_t id = 0;
        TK_HIP(c, hipMemcpy(&id, d_ctrl + bad[1], 4, hipMemcpyDeviceToHost));
        return bad_ctrl(c, bad[1], id);
    }
    return TK_OK;
}

// The join over ids on the device into the context's c->join buffers; *out gets the device pointers.  The outputs are sized for
// n_ids + n_parts elements, so nothing is read before the launches; ONE wait at the end (N, n_ctrl, n_labelled).  Nothing of an
// earlier result is touched before every argument has been accepted.  The caller holds c->mu.
int run_join(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t P, uint64_t n_ids, const uint32_t* d_ctrl,
             const uint32_t* d_pflags, const uint64_t* d_conv, uint64_t C, bool check_parts, const tk_join_opts* o, hipStream_t s,
             tk_join* out) {
    int rc = join_check_args(c, P, C, o);
    if (rc != TK_OK) return rc;
    if (P == 0 && n_ids) { c->err = "join: ids without a part"; return TK_ERR_INVALID_ARG; }
    if (check_parts && (rc = check_parts_device(c, d_ctrl, d_conv, P, C, s)) != TK_OK) return rc;
    const bool want_lab = (o->flags & TK_JOIN_LABELS) != 0, want_pi = (o->flags & TK_JOIN_PART_INDEX) != 0;
    const uint64_t cap = n_ids + P;
    TK_HIP(c, c->join.stat.reserve(64));
    TK_HIP(c, c->join.ids.reserve(cap * 4 + 16));
    TK_HIP(c, c->join.offs.reserve((C + 1) * 8));
    if (want_lab) TK_HIP(c, c->join.labels.reserve(cap * 4 + 16));
    if (want_pi) TK_HIP(c, c->join.pidx.reserve(cap * 4 + 16));
    unsigned long long got[3] = {0, 0, 0};      // N, n_ctrl, n_labelled
    if (P == 0) {                               // (no part: offsets = [0] * (C + 1), nothing to launch)
        TK_HIP(c, hipMemsetAsync(c->join.offs.p, 0, (C + 1) * 8, s));
    } else {
        TK_HIP(c, c->join.has.reserve(P * 4 + 16));
        TK_HIP(c, c->join.cb.reserve((P + 1) * 8));
        TK_HIP(c, c->join.start.reserve((P + 1) * 8));
        if (want_pi) TK_HIP(c, c->join.plocal.reserve(P * 4 + 16));
        TK_HIP(c, c->join.bsum.reserve(scan_workspace_bytes(P)));
        TkJoinArgs a;
        memset(&a, 0, sizeof(a));
        a.ids = d_ids;
        a.id_offs = d_id_offs;
        a.n_parts = P;
        a.n_convs = C;
        a.ctrl = d_ctrl;
        a.pflags = d_pflags;
        a.conv_offs = d_conv;
        a.cap = cap;
        a.num_special = c->host.num_special;
        a.ignore = o->ignore_index;
        a.has = (uint32_t*)c->join.has.p;
        a.cb = (const uint64_t*)c->join.cb.p;
        a.start = (uint64_t*)c->join.start.p;
        a.plocal = (uint32_t*)c->join.plocal.p;
        a.out_ids = (uint32_t*)c->join.ids.p;
        a.out_offs = (uint64_t*)c->join.offs.p;
        a.labels = want_lab ? (int32_t*)c->join.labels.p : nullptr;
        a.part_index = want_pi ? (uint32_t*)c->join.pidx.p : nullptr;
        a.stat = (unsigned long long*)c->join.stat.p;
        TK_HIP(c, hipMemsetAsync(a.stat, 0, 8, s));
        TK_HIP(c, tk_launch_join_has(a, s));
        if ((rc = scan_u32(c, c->join.bsum, a.has, P, (uint64_t*)c->join.cb.p, s)) != TK_OK) return rc;
        TK_HIP(c, tk_launch_join_parts(a, s));
        TK_HIP(c, tk_launch_join(a, s));
        TK_HIP(c, hipMemcpyAsync(got, a.start + P, 8, hipMemcpyDeviceToHost, s));
        TK_HIP(c, hipMemcpyAsync(got + 1, a.cb + P, 8, hipMemcpyDeviceToHost, s));
        TK_HIP(c, hipMemcpyAsync(got + 2, a.stat, 8, hipMemcpyDeviceToHost, s));
    }
    TK_HIP(c, hipStreamSynchronize(s));
    if (got[0] > cap) {
        c->err = "join: id_offsets end at " + std::to_string(got[0] - got[1]) + ", beyond n_ids = " + std::to_string(n_ids);
        return TK_ERR_INVALID_ARG;
    }
    out->ids = (uint32_t*)c->join.ids.p;
    out->offsets = (uint64_t*)c->join.offs.p;
    out->labels = want_lab ? (int32_t*)c->join.labels.p : nullptr;
    out->part_index = want_pi ? (uint32_t*)c->join.pidx.p : nullptr;
    out->n_convs = C;
    out->n_parts = P;
    out->n_ids = got[0];
    out->n_ctrl = got[1];
    out->n_labelled = got[2];
    return TK_OK;
}

extern "C" int tk_join_from_ids_device(tk_ctx* c, const void* d_ids, const void* d_id_offsets, uint64_t n_parts, uint64_t n_ids,
                                       const void* d_part_ctrl, const void* d_part_flags, const void* d_conv_offsets, uint64_t n_convs,
                                       int checks, const tk_join_opts* opts, void* hip_stream, tk_join* out) {
    TK_ENTRY(c);
    int rc = check_flags_and_args(c, checks, TK_CHECK_PARTS, !d_id_offsets || (!d_ids && n_ids) || (!d_part_ctrl && n_parts) || !d_conv_offsets || !opts || !out);
    if (rc != TK_OK) return rc;
    TK_HIP(c, hipSetDevice(c->device));
    return run_join(c, (const uint32_t*)d_ids, (const uint64_t*)d_id_offsets, n_parts, n_ids, (const uint32_t*)d_part_ctrl,
                    (const uint32_t*)d_part_flags, (const uint64_t*)d_conv_offsets, n_convs, (checks & TK_CHECK_PARTS) != 0, opts,
                    (hipStream_t)hip_stream, out);
}

int encode_parts_device_join(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_parts, uint64_t n_bytes,
                             const void* d_part_ctrl, const void* d_part_flags, const void* d_conv_offsets, uint64_t n_convs,
                             int checks, const tk_join_opts* opts, void* hip_stream, tk_join* out) {
    int rc = check_flags_and_args(c, checks, TK_CHECK_OFFSETS | TK_CHECK_UTF8 | TK_CHECK_PARTS,
                                  !d_doc_offsets || (!d_bytes && n_bytes) || (!d_part_ctrl && n_parts) || !d_conv_offsets || !opts || !out);
    if (rc != TK_OK || (rc = join_check_args(c, n_parts, n_convs, opts)) != TK_OK) return rc;
    TK_HIP(c, hipSetDevice(c->device));
    // (the parts are checked before the text is encoded: a refused call costs one small kernel)
    if ((checks & TK_CHECK_PARTS) && (rc = check_parts_device(c, (const uint32_t*)d_part_ctrl, (const uint64_t*)d_conv_offsets, n_parts, n_convs,
                                                               (hipStream_t)hip_stream)) != TK_OK) return rc;
    void *d_ids = nullptr, *d_oo = nullptr;
    uint64_t n_ids = 0;
    rc = encode_device_checked(c, d_bytes, d_doc_offsets, n_parts, n_bytes, 0, 0, checks & (TK_CHECK_OFFSETS | TK_CHECK_UTF8), hip_stream,
                               &d_ids, &d_oo, &n_ids);
    if (rc != TK_OK) return rc;
    return run_join(c, (const uint32_t*)d_ids, (const uint64_t*)d_oo, n_parts, n_ids, (const uint32_t*)d_part_ctrl, (const uint32_t*)d_part_flags,
                    (const uint64_t*)d_conv_offsets, n_convs, false, opts, (hipStream_t)hip_stream, out);
}

extern "C" int tk_encode_parts_device_join(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_parts, uint64_t n_bytes,
                                           const void* d_part_ctrl, const void* d_part_flags, const void* d_conv_offsets, uint64_t n_convs,
                                           int checks, const tk_join_opts* opts, void* hip_stream, tk_join* out) {
    TK_ENTRY(c);
    return encode_parts_device_join(c, d_bytes, d_doc_offsets, n_parts, n_bytes, d_part_ctrl, d_part_flags, d_conv_offsets, n_convs, checks,
                                    opts, hip_stream, out);
}

extern "C" void tk_free_join(tk_join* r) { layout_free(r); }

extern "C" int tk_encode_parts_join(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_parts, const uint32_t* part_ctrl,
                                    const uint32_t* part_flags, const uint64_t* conv_offsets, uint64_t n_convs, int validate_utf8,
                                    const tk_join_opts* opts, tk_join* out) {
    TK_ENTRY(c);
    if (!opts || !out || !doc_offsets || !conv_offsets || (!part_ctrl && n_parts)) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    memset(out, 0, sizeof(*out));
    int rc = join_check_args(c, n_parts, n_convs, opts);
    if (rc != TK_OK) return rc;
    if ((rc = check_parts_host(c, part_ctrl, conv_offsets, n_parts, n_convs)) != TK_OK) return rc;
    DevBatch dev;
    uint64_t n_ids;
    if ((rc = encode_batch_for_layout(c, bytes, doc_offsets, n_parts, 0, 0, validate_utf8, &dev, &n_ids)) != TK_OK) return rc;
    TK_HIP(c, c->join.in_ctrl.reserve(n_parts * 4 + 16));
    TK_HIP(c, c->join.in_flags.reserve(n_parts * 4 + 16));
    TK_HIP(c, c->join.in_conv.reserve((n_convs + 1) * 8));
    if (n_parts) TK_HIP(c, hipMemcpyAsync(c->join.in_ctrl.p, part_ctrl, n_parts * 4, hipMemcpyHostToDevice, c->stream));
    if (n_parts && part_flags) TK_HIP(c, hipMemcpyAsync(c->join.in_flags.p, part_flags, n_parts * 4, hipMemcpyHostToDevice, c->stream));
    TK_HIP(c, hipMemcpyAsync(c->join.in_conv.p, conv_offsets, (n_convs + 1) * 8, hipMemcpyHostToDevice, c->stream));
    tk_join j;
    rc = run_join(c, dev.ids, dev.id_offs, n_parts, n_ids, (const uint32_t*)c->join.in_ctrl.p, part_flags ? (const uint32_t*)c->join.in_flags.p : nullptr,
                  (const uint64_t*)c->join.in_conv.p, n_convs, false, opts, c->stream, &j);
    if (rc != TK_OK) return rc;
    return layout_copy_out(c, j, 4, n_convs, "join", out);
}
