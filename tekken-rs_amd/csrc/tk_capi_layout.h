// tk_capi_layout.h -- what the host files of the layout passes (tk_capi_dense / _seqpack / _join / _window / _chunk / _rowfit / _regroup / _pair.cpp) share, and
// only they include: ONE description of the outputs of each result struct, from which tk_free_<pass> and the copy-out of the host
// entries are made, and the three entries around a pass (ids on the device | text on the device | text on the host) written once.
// (tk_capi_words.cpp, tk_capi_specials.cpp, tk_capi_fim.cpp and tk_capi_noise.cpp take the descriptions of tk_words / tk_specials /
// tk_fim / tk_noise_replace / tk_noise_spans from here
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
