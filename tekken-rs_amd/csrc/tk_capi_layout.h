// tk_capi_layout.h -- what the host files of the layout passes (tk_capi_dense / _seqpack / _join / _window / _chunk / _rowfit / _regroup / _pair.cpp) share, and
// only they include: ONE description of the outputs of each result struct, from which tk_free_<pass> and the copy-out of the host
// entries are made, the sizing of a tensor of rows (the refusals, and the counts / scan / one read of the window, chunk and pair
// passes), what the window and chunk passes share beyond that, and the three entries around a pass (ids on the device | text on the
// device | text on the host) written once.
// (tk_capi_words.cpp, tk_capi_specials.cpp, tk_capi_fim.cpp, tk_capi_noise.cpp and tk_capi_audio.cpp take the descriptions of
// tk_words / tk_specials / tk_fim / tk_noise_replace / tk_noise_spans / tk_logmel / tk_ragged from here
// and have entries of their own: they take the text, or stand in front of encode.)
#ifndef TK_CAPI_LAYOUT_H
#define TK_CAPI_LAYOUT_H
#include <type_traits>

#include "tk_ctx.h"

// ---- the outputs of a result.  layout_outputs(r, esz, n_docs, f) calls f(field, bytes, selected) for every pointer field of r, in
// the order of the struct.  esz: the bytes of an element of the tensors that the pass's I64 flag widens; n_docs: what a size needs
// and r does not carry (rowfit's doc_start).  selected: false for an output the caller did not ask for, which is null in the
// result of the pass.  An output added to a struct is added here, and nowhere else in the host code.
template <class F> static inline void layout_outputs(tk_dense& r, uint64_t esz, uint64_t, F&& f) {
    const uint64_t elems = r.n_docs * r.row_len;
    f(r.ids, elems * esz, true);
    f(r.mask, elems, r.mask != nullptr);
    f(r.lengths, r.n_docs * 4, true);
}
template <class F> static inline void layout_outputs(tk_seqpack& r, uint64_t esz, uint64_t, F&& f) {
    const uint64_t bytes = r.n_rows * r.row_len * esz;
    f(r.input_ids, bytes, true);
    f(r.position_ids, bytes, r.position_ids != nullptr);
    f(r.segment_ids, bytes, r.segment_ids != nullptr);
    f(r.cu_seqlens, (r.n_segments + 1) * 4, r.cu_seqlens != nullptr);
}
template <class F> static inline void layout_outputs(tk_join& r, uint64_t, uint64_t, F&& f) {
    const uint64_t n4 = r.n_ids * 4;            // (no id: 0 bytes, which is the block alone and nothing copied)
    f(r.ids, n4, true);
    f(r.offsets, (r.n_convs + 1) * 8, true);
    f(r.labels, n4, r.labels != nullptr);
    f(r.part_index, n4, r.part_index != nullptr);
}
template <class F> static inline void layout_outputs(tk_window& r, uint64_t esz, uint64_t, F&& f) {
    const uint64_t elems = r.n_windows * r.row_len;
    f(r.input_ids, elems * esz, true);
    f(r.mask, elems, r.mask != nullptr);
    f(r.lengths, r.n_windows * 4, true);
    f(r.window_doc, r.n_windows * 4, true);
    f(r.window_start, r.n_windows * 4, true);
    f(r.doc_windows, (r.n_docs + 1) * 8, true);
    f(r.spans, elems * 8, r.spans != nullptr);
}
template <class F> static inline void layout_outputs(tk_chunk& r, uint64_t esz, uint64_t, F&& f) {
    const uint64_t elems = r.n_windows * r.row_len;
    f(r.input_ids, elems * esz, true);
    f(r.mask, elems, r.mask != nullptr);
    f(r.lengths, r.n_windows * 4, true);
    f(r.window_doc, r.n_windows * 4, true);
    f(r.window_start, r.n_windows * 4, true);
    f(r.doc_windows, (r.n_docs + 1) * 8, true);
    f(r.spans, elems * 8, r.spans != nullptr);
    f(r.cut_level, r.n_windows, true);
    f(r.chunk_bytes, r.n_windows * 8, r.chunk_bytes != nullptr);
    f(r.level_counts, 6 * 8, true);
}
template <class F> static inline void layout_outputs(tk_pair& r, uint64_t esz, uint64_t, F&& f) {
    const uint64_t elems = r.n_windows * r.row_len;
    f(r.input_ids, elems * esz, true);
    f(r.mask, elems, r.mask != nullptr);
    f(r.type_ids, elems, r.type_ids != nullptr);
    f(r.sequence_ids, elems, r.sequence_ids != nullptr);
    f(r.lengths, r.n_windows * 4, true);
    f(r.window_pair, r.n_windows * 4, true);
    f(r.window_start, r.n_windows * 4, true);
    f(r.second_start, r.n_windows * 4, true);
    f(r.spans, elems * 8, r.spans != nullptr);
    f(r.pair_windows, (r.n_pairs + 1) * 8, true);
}
template <class F> static inline void layout_outputs(tk_rowfit& r, uint64_t esz, uint64_t n_docs, F&& f) {
    const uint64_t elems = r.n_rows * r.row_len;
    f(r.input_ids, elems * esz, true);
    f(r.labels, elems * 4, r.labels != nullptr);
    f(r.position_ids, elems * esz, r.position_ids != nullptr);
    f(r.segment_ids, elems * esz, r.segment_ids != nullptr);
    f(r.cu_seqlens, (r.n_segments + 1) * 4, r.cu_seqlens != nullptr);
    f(r.doc_start, n_docs * 8, r.doc_start != nullptr);
}
template <class F> static inline void layout_outputs(tk_regroup& r, uint64_t, uint64_t, F&& f) {
    const uint64_t n4 = r.n_ids * 4;            // (r.n_docs: the kept documents)
    f(r.ids, n4, true);
    f(r.offsets, (r.n_docs + 1) * 8, true);
    f(r.labels, n4, r.labels != nullptr);
    f(r.perm, r.n_docs * 4, r.perm != nullptr);
    f(r.batch_offsets, (r.n_batches + 1) * 8, r.batch_offsets != nullptr);
    f(r.batch_rowlen, r.n_batches * 4, r.batch_rowlen != nullptr);
}
template <class F> static inline void layout_outputs(tk_specials& r, uint64_t, uint64_t, F&& f) {
    f(r.bytes, r.n_bytes, true);                // (no byte: the block alone, as a join's ids)
    f(r.part_offsets, (r.n_parts + 1) * 8, true);
    f(r.part_ctrl, r.n_parts * 4, true);
    f(r.conv_offsets, (r.n_docs + 1) * 8, true);
    f(r.part_src, r.n_parts * 8, r.part_src != nullptr);
}
template <class F> static inline void layout_outputs(tk_fim& r, uint64_t esz, uint64_t, F&& f) {
    f(r.units, r.n_units * esz, true);          // (esz: the bytes of a unit, 1 for text and 4 for ids)
    f(r.part_offsets, (r.n_parts + 1) * 8, true);
    f(r.part_ctrl, r.n_parts * 4, true);
    f(r.part_flags, r.n_parts * 4, true);
    f(r.conv_offsets, (r.n_docs + 1) * 8, true);
    f(r.part_src, r.n_parts * 8, r.part_src != nullptr);
    f(r.cuts, r.n_docs * 16, true);
    f(r.mode, r.n_docs, true);
}
template <class F> static inline void layout_outputs(tk_noise_replace& r, uint64_t, uint64_t, F&& f) {
    f(r.input_ids, r.n_ids * 4, true);
    f(r.labels, r.n_ids * 4, true);
    f(r.selected, r.n_ids, r.selected != nullptr);
}
template <class F> static inline void layout_outputs(tk_noise_spans& r, uint64_t, uint64_t, F&& f) {
    const uint64_t offs = (r.n_docs + 1) * 8, nj = (r.n_inputs + r.n_targets) * 4;
    f(r.inputs, r.n_inputs * 4, r.inputs != nullptr);           // (TK_NOISE_SPLIT: the first four)
    f(r.input_offsets, offs, r.input_offsets != nullptr);
    f(r.targets, r.n_targets * 4, r.targets != nullptr);
    f(r.target_offsets, offs, r.target_offsets != nullptr);
    f(r.joined, nj, r.joined != nullptr);                       // (TK_NOISE_JOINED: the last three)
    f(r.joined_offsets, offs, r.joined_offsets != nullptr);
    f(r.joined_labels, nj, r.joined_labels != nullptr);
}
template <class F> static inline void layout_outputs(tk_words& r, uint64_t, uint64_t, F&& f) {
    f(r.word_ids, r.n_ids * 4, true);
    f(r.doc_words, (r.n_docs + 1) * 8, true);
    f(r.word_first, r.n_words * 4, r.word_first != nullptr);
}
template <class F> static inline void layout_outputs(tk_logmel& r, uint64_t, uint64_t, F&& f) {
    f(r.features, r.n_mel * r.n_frames * 4, true);
    f(r.frame_off, (r.n_segments + 1) * 8, true);
    f(r.clip_seg, (r.n_clips + 1) * 8, true);
}
template <class F> static inline void layout_outputs(tk_ragged& r, uint64_t, uint64_t, F&& f) {
    f(r.ids, r.n_ids * 4, true);
    f(r.offsets, (r.n_parts + 1) * 8, true);
}

// tk_free_<pass>: every block back to the pinned pool, the struct zeroed
template <class R> static inline void layout_free(R* r) {
    if (!r) return;
    layout_outputs(*r, 0, 0, [](auto*& p, uint64_t, bool) { tk_pinned_put(p); });
    memset(r, 0, sizeof(*r));
}

// The result of a pass (device pointers) to the host: *out = dev with every selected output in a pinned block of its own, an
// unselected one null.  On a failure *out is untouched (copy_out, tk_ctx.h: every block is back in the pool).
template <class R> static inline int layout_copy_out(tk_ctx* c, const R& dev, uint64_t esz, uint64_t n_docs, const char* what, R* out) {
    R r = dev;
    std::vector<CopyOut> h;
    layout_outputs(r, esz, n_docs, [&](auto*& p, uint64_t bytes, bool selected) { h.push_back(CopyOut{p, bytes, nullptr, selected}); });
    const int rc = copy_out(c, h.data(), (int)h.size(), what);
    if (rc != TK_OK) return rc;
    size_t n = 0;
    layout_outputs(r, esz, n_docs, [&](auto*& p, uint64_t, bool) { p = (std::remove_reference_t<decltype(p)>)h[n++].host; });
    *out = r;
    return TK_OK;
}

// ---- the sizing of a tensor of rows ----
static inline uint64_t round_up(uint64_t L, uint64_t m) { return m ? (L + m - 1) / m * m : L; }
// what every pass says of a tensor it cannot make; noun: "dense", "windows", ...
static inline int layout_too_large(tk_ctx* c, const char* noun, uint64_t n_rows, uint64_t row_len) {
    c->err = std::string(noun) + ": " + std::to_string(n_rows) + " rows of " + std::to_string(row_len) + " elements are beyond what one tensor can hold";
    return TK_ERR_INVALID_ARG;
}
// The passes in which an owner (a document, a pair) gives w rows -- window, chunk, pair -- size their tensors in three steps, and
// touch nothing of an earlier result before the third has gone through (the pass then swaps `next` in as its doc_windows):
// 1. before anything is enqueued: a fixed row length that cannot be
static inline int layout_check_fixed_len(tk_ctx* c, const char* noun, bool fixed, uint64_t max_length, uint64_t multiple_of) {
    if (!fixed || round_up(max_length, multiple_of) <= TK_LAYOUT_MAX_ROW) return TK_OK;
    c->err = std::string(noun) + ": max_length rounded up to a multiple of " + std::to_string(multiple_of) + " is beyond 2^31 - 1";
    return TK_ERR_INVALID_ARG;
}
// 2. the work buffers, the pass's counts kernel -- counts_kernel(counts, d_stat) enqueues it on s: counts[n] and n_stat statistics
// words, zeroed here --, the scan of the counts into `next`, and ONE read with one wait: *W = next[n], the rows, and stat[0 .. n_stat).
// No owner: nothing is launched, next[0] = 0 and everything read is 0.  scanned: an event recorded behind the scan (one that
// counts_kernel may have created), or null
template <class K>
static inline int layout_count_rows(tk_ctx* c, uint64_t n, DevBuf& d_stat, DevBuf& cnt, DevBuf& next, DevBuf& bsum, unsigned long long* stat,
                                    size_t n_stat, hipStream_t s, K counts_kernel, uint64_t* W, const hipEvent_t* scanned = nullptr) {
    TK_HIP(c, d_stat.reserve(64));
    TK_HIP(c, cnt.reserve(n * 4 + 16));
    TK_HIP(c, next.reserve((n + 1) * 8));
    TK_HIP(c, bsum.reserve(scan_workspace_bytes(n)));
    *W = 0;
    memset(stat, 0, n_stat * 8);
    if (n == 0) {
        TK_HIP(c, hipMemsetAsync(next.p, 0, 8, s));
    } else {
        TK_HIP(c, hipMemsetAsync(d_stat.p, 0, n_stat * 8, s));
        TK_HIP(c, counts_kernel((uint32_t*)cnt.p, (unsigned long long*)d_stat.p));
        const int rc = scan_u32(c, bsum, (const uint32_t*)cnt.p, n, (uint64_t*)next.p, s);
        if (rc != TK_OK) return rc;
        if (scanned) TK_HIP(c, hipEventRecord(*scanned, s));
        TK_HIP(c, hipMemcpyAsync(W, (const uint64_t*)next.p + n, 8, hipMemcpyDeviceToHost, s));
        TK_HIP(c, hipMemcpyAsync(stat, d_stat.p, n_stat * 8, hipMemcpyDeviceToHost, s));
    }
    TK_HIP(c, hipStreamSynchronize(s));
    return TK_OK;
}
// 3. the row length: max_length where `fixed`, else the longest row (window and chunk pass the longest document, clamped to
// max_length; a pair's row never exceeds it), rounded up to multiple_of; refused where W rows of it are more than a tensor holds
static inline int layout_row_len(tk_ctx* c, const char* noun, bool fixed, uint64_t longest, uint64_t max_length, uint64_t multiple_of, uint64_t W,
                                 uint64_t* L) {
    *L = round_up(fixed ? max_length : longest, multiple_of);
    if (*L > TK_LAYOUT_MAX_ROW || W >= (1ull << 32) || (W && *L > TK_LAYOUT_MAX_ELEMS / W)) return layout_too_large(c, noun, W, *L);
    return TK_OK;
}

// ---- what the window and chunk passes share beyond that (their rows are head | a run of the body | tail of a document:
// TkRowFillArgs, WindowBufs; O: tk_window_opts / tk_chunk_opts, R: tk_window / tk_chunk) ----
// the option tests both have, behind the null and flag tests of each; noun: "windows" / "chunks"
template <class O> static inline int rowfill_check_opts(tk_ctx* c, const char* noun, const O* o) {
    if (o->max_length == 0) { c->err = std::string(noun) + " need a max_length"; return TK_ERR_INVALID_ARG; }
    if (o->max_length > TK_LAYOUT_MAX_ROW) { c->err = "max_length " + std::to_string(o->max_length) + " is beyond 2^31 - 1"; return TK_ERR_INVALID_ARG; }
    if ((uint64_t)o->keep_head + o->keep_tail >= o->max_length) {
        c->err = "keep_head + keep_tail leave no room for text in max_length " + std::to_string(o->max_length);
        return TK_ERR_INVALID_ARG;
    }
    return TK_OK;
}
// the options of an entry that encodes first: BOS / EOS are what every row repeats
template <class O, int (*check_opts)(tk_ctx*, const O*)>
static int rowfill_encode_opts(tk_ctx* c, const O* opts, int add_bos, int add_eos, O* o) {
    *o = *opts;
    o->keep_head = add_bos ? 1u : 0u;
    o->keep_tail = add_eos ? 1u : 0u;
    return check_opts(c, o);
}
template <class O>
static inline void rowfill_inputs(TkRowFillArgs& a, const uint32_t* d_ids, const uint64_t* d_id_offs, const uint32_t* d_spans, uint64_t n_docs, const O* o) {
    a.ids = d_ids;
    a.id_offs = d_id_offs;
    a.in_spans = d_spans;
    a.n_docs = n_docs;
    a.max_len = o->max_length;
    a.keep_head = o->keep_head;
    a.keep_tail = o->keep_tail;
    a.pad_id = o->pad_id;
}
// The seven outputs both have, for W rows of L elements: reserved, then -- the last thing that can fail is behind -- the scan
// swapped in as doc_windows, and the fill's arguments point at them.  (The chunk pass reserves its own outputs in front.)
static inline int rowfill_outputs(tk_ctx* c, WindowBufs& b, TkRowFillArgs& a, uint64_t W, uint64_t L, bool i64, bool mask, bool spans) {
    const uint64_t elems = W * L;
    TK_HIP(c, b.ids.reserve(elems * (i64 ? 8 : 4) + 16));
    if (mask) TK_HIP(c, b.mask.reserve(elems + 16));
    if (spans) TK_HIP(c, b.spans.reserve(elems * 8 + 16));
    TK_HIP(c, b.len.reserve(W * 4 + 16));
    TK_HIP(c, b.doc.reserve(W * 4 + 16));
    TK_HIP(c, b.start.reserve(W * 4 + 16));
    std::swap(b.dw, b.dw_next);
    a.row_len = (uint32_t)L;
    a.n_rows = W;
    a.doc_windows = (const uint64_t*)b.dw.p;
    a.out = b.ids.p;
    a.mask = mask ? (uint8_t*)b.mask.p : nullptr;
    a.out_spans = spans ? (uint32_t*)b.spans.p : nullptr;
    a.lengths = (uint32_t*)b.len.p;
    a.window_doc = (uint32_t*)b.doc.p;
    a.window_start = (uint32_t*)b.start.p;
    return TK_OK;
}
template <class R> static inline void rowfill_result(const TkRowFillArgs& a, uint64_t n_split, R* out) {
    out->input_ids = a.out;
    out->mask = a.mask;
    out->lengths = a.lengths;
    out->window_doc = a.window_doc;
    out->window_start = a.window_start;
    out->doc_windows = (uint64_t*)a.doc_windows;
    out->spans = a.out_spans;
    out->n_docs = a.n_docs;
    out->n_windows = a.n_rows;
    out->row_len = a.row_len;
    out->n_split = n_split;
}

// ---- the three entries around a pass, for the passes whose entries take the same arguments (dense, seqpack, window, rowfit, regroup;
// join has its own).  A pass is a struct P with
//   Opts, Result    the option and result structs of the C ABI
//   name            what a failed copy-out is called in the message
//   esz(o)          the bytes of an element of the tensors
//   encode_opts(c, opts, add_bos, add_eos, &o)   the options of an entry that encodes first, checked: what can be refused is refused
//                   before anything is encoded
//   run(c, d_ids, d_id_offs, n_docs, n_ids, [d_extra,] o, s, out)   the pass (it checks its options itself); d_extra: the second
//                   input of the passes that have one (window: the spans, rowfit: the labels, regroup: the labels and the keep mask)
//   run_encoded(c, d_ids, d_id_offs, n_docs, n_ids, o, s, out)      the pass behind an encode on s; LayoutPass<P> has it for a pass
//                   without a second input, the others say what stands in for theirs
// What a bad call reports first is behaviour (check_n_docs, tk_ctx.h): an unknown check flag, a null argument, the options of the
// pass, then encode, then the pass.  Nothing below asks which pass it serves: what differs is in P.
template <class P> struct LayoutPass {
    template <class O, class R>
    static int run_encoded(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t n_ids, const O* o, hipStream_t s, R* out) {
        return P::run(c, d_ids, d_id_offs, n_docs, n_ids, o, s, out);
    }
};
template <class P, class... Extra>
static inline int layout_from_ids_device(tk_ctx* c, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                                         const typename P::Opts* opts, void* hip_stream, typename P::Result* out, Extra... d_extra) {
    TK_ENTRY(c);
    if (!d_id_offsets || (!d_ids && n_ids) || !opts || !out) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    TK_HIP(c, hipSetDevice(c->device));
    return P::run(c, (const uint32_t*)d_ids, (const uint64_t*)d_id_offsets, n_docs, n_ids, d_extra..., opts, (hipStream_t)hip_stream, out);
}
template <class P>
static inline int layout_encode_device(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                       int add_bos, int add_eos, int checks, const typename P::Opts* opts, void* hip_stream, void** d_ids,
                                       void** d_out_offsets, uint64_t* n_ids, typename P::Result* out) {
    TK_ENTRY(c);
    int rc = check_flags_and_args(c, checks, TK_CHECK_OFFSETS | TK_CHECK_UTF8, !opts || !out);
    if (rc != TK_OK) return rc;
    typename P::Opts o;
    if ((rc = P::encode_opts(c, opts, add_bos, add_eos, &o)) != TK_OK) return rc;
    rc = encode_device_checked(c, d_bytes, d_doc_offsets, n_docs, n_bytes, add_bos, add_eos, checks, hip_stream, d_ids, d_out_offsets, n_ids);
    if (rc != TK_OK) return rc;
    return P::run_encoded(c, (const uint32_t*)*d_ids, (const uint64_t*)*d_out_offsets, n_docs, *n_ids, &o, (hipStream_t)hip_stream, out);
}
// host in / host out.  *out is zeroed once the arguments are there, and filled only by a call that went through
template <class P>
static inline int layout_encode_host(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos,
                                     int add_eos, int validate_utf8, const typename P::Opts* opts, typename P::Result* out) {
    TK_ENTRY(c);
    if (!opts || !out) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    memset(out, 0, sizeof(*out));
    typename P::Opts o;
    int rc = P::encode_opts(c, opts, add_bos, add_eos, &o);
    if (rc != TK_OK) return rc;
    DevBatch dev;
    uint64_t n_ids;
    if ((rc = encode_batch_for_layout(c, bytes, doc_offsets, n_docs, add_bos, add_eos, validate_utf8, &dev, &n_ids)) != TK_OK) return rc;
    // (the small path's ids and offsets are mapped pinned memory: the kernels of the pass read them there)
    typename P::Result r;
    if ((rc = P::run_encoded(c, dev.ids, dev.id_offs, n_docs, n_ids, &o, c->stream, &r)) != TK_OK) return rc;
    return layout_copy_out(c, r, P::esz(o), n_docs, P::name, out);
}

#endif
