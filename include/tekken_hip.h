/*
 * tekken_hip.h -- C ABI of the MI355X-native batch tokenization path for tekken-rs.
 *
 * The reference has no FFI seam today; this boundary is inserted at its single call into
 * the third-party BPE engine:
 *
 *     let (tokens, _) = self.tekkenizer.encode(text, &HashSet::new());   src/tekkenizer.rs:384-386
 *     CoreBPE::new(mergeable_ranks.clone(), special_tokens, pattern)      src/tekkenizer.rs:125
 *
 * plus the id shift and BOS/EOS insertion of src/tekkenizer.rs:390-402, which are fused
 * into the device emit.  Everything is plain pointers and sizes; no C++ or torch types.
 * The Rust binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Threading: a context serialises its calls internally (one HIP stream + mutex), so it can
 * back the reference's `&self` / `Sync` Tekkenizer (tests/test_tokenizer_output.rs:5-12).
 */
#ifndef TEKKEN_HIP_H
#define TEKKEN_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes; the Rust shim maps them onto TokenizerError (src/errors.rs:23-59) ---- */
#define TK_OK 0
#define TK_ERR_INVALID_CONFIG (-1)   /* -> TokenizerError::InvalidConfig   (errors.rs:45-46) */
#define TK_ERR_RUNTIME (-2)          /* -> TokenizerError::Tokenizers(msg) (errors.rs:37-38) */
#define TK_ERR_INVALID_UTF8 (-3)     /* -> TokenizerError::Tokenizers(msg); &str can never trigger it */
#define TK_ERR_NO_DEVICE (-4)        /* -> TokenizerError::Tokenizers(msg): no gfx950 device / HIP missing */
#define TK_ERR_INVALID_ARG (-5)      /* -> TokenizerError::InvalidConfig */
#define TK_ERR_IO (-6)               /* -> TokenizerError::Io              (errors.rs:25-26) */
#define TK_ERR_JSON (-7)             /* -> TokenizerError::Json            (errors.rs:29-30) */
#define TK_ERR_BASE64 (-8)           /* -> TokenizerError::Base64          (errors.rs:33-34) */
#define TK_ERR_TOKEN_NOT_FOUND (-9)  /* -> TokenizerError::TokenNotFound   (errors.rs:49-50) */
#define TK_ERR_SPECIAL_POLICY (-10)  /* -> TokenizerError::SpecialTokenPolicy (errors.rs:53-54) */
#define TK_ERR_AUDIO (-11)           /* -> TokenizerError::Audio           (errors.rs; src/audio.rs:421, src/tekkenizer.rs:731) */

#define TK_POLICY_IGNORE 0  /* SpecialTokenPolicy::Ignore  (src/special_tokens.rs:128-136) */
#define TK_POLICY_KEEP 1    /* SpecialTokenPolicy::Keep  */
#define TK_POLICY_RAISE 2   /* SpecialTokenPolicy::Raise */

typedef struct tk_ctx tk_ctx;

/* ------------------------------------------------------------------------------------------
 * Engine level: replaces CoreBPE::new / CoreBPE::encode.
 * ---------------------------------------------------------------------------------------- */

/* Replaces `CoreBPE::new(mergeable_ranks, {}, pattern)` (src/tekkenizer.rs:122-126).
 * token_bytes/token_offsets: rank i has bytes token_bytes[token_offsets[i] .. token_offsets[i+1]);
 * the table must already satisfy the checks of reload_mergeable_ranks (src/tekkenizer.rs:776-816)
 * -- the checks are repeated and TK_ERR_INVALID_CONFIG is returned if they fail.
 * bos_id/eos_id are the FINAL ids of "<s>" / "</s>" (src/tekkenizer.rs:286-297).
 * The split pattern is the literal of src/tekkenizer.rs:123 (the JSON `pattern` is ignored by the
 * reference, :74).  Inputs are copied.  device_id: HIP device ordinal. */
int tk_ctx_create(const uint8_t* token_bytes, const uint32_t* token_offsets, uint32_t n_ranks,
                  uint32_t num_special_tokens, uint32_t bos_id, uint32_t eos_id, int device_id,
                  tk_ctx** out_ctx);

/* Frees device and host state.  NULL is a no-op. */
void tk_ctx_destroy(tk_ctx* ctx);

/* Message of the last failing call on this context (or of the last failing tk_ctx_create /
 * tk_tokenizer_* constructor on this thread when ctx == NULL).  Never NULL. */
const char* tk_last_error(const tk_ctx* ctx);

typedef struct tk_result {
    uint32_t* ids;      /* n_ids final token ids (shifted, BOS/EOS in place), document order */
    uint64_t* offsets;  /* n_docs + 1 entries: document d owns ids[offsets[d] .. offsets[d+1]) */
    uint64_t n_ids;
    uint64_t n_docs;
} tk_result;

/* Batch form of `Tekkenizer::encode(text, add_bos, add_eos)` (src/tekkenizer.rs:378-405):
 * document d = bytes[doc_offsets[d] .. doc_offsets[d+1]), for every d exactly what the reference
 * returns for that &str.  Host buffers in, host buffers out (pinned, owned by the library until
 * tk_free_result).  Each document must be valid UTF-8 (a Rust &str always is); pass
 * validate_utf8 != 0 to have that checked (TK_ERR_INVALID_UTF8). */
int tk_encode_batch(tk_ctx* ctx, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs,
                    int add_bos, int add_eos, int validate_utf8, tk_result* out);
void tk_free_result(tk_result* r);

/* `Tekkenizer::encode(text, add_bos, add_eos)` for ONE document with a caller-owned output -- the reference's own call shape
 * (src/tekkenizer.rs:378-405: one &str in, one Vec<u32> out).  No allocation; a text of up to 64 KiB is ONE kernel launch
 * (a single workgroup splits, looks up, merges, and packs; the kernel reads the text from, and writes the ids to, mapped
 * pinned host memory), longer ones take the batch pipeline.  ids_capacity >= len + 2 always suffices;
 * TK_ERR_INVALID_ARG if the ids do not fit (*n_ids then holds the count needed).  Batches of up to 1024 documents / 64 KiB
 * handed to tk_encode_batch take the same one-launch path. */
int tk_encode_one(tk_ctx* ctx, const uint8_t* text, uint64_t len, int add_bos, int add_eos, uint32_t* ids_out,
                  uint64_t ids_capacity, uint64_t* n_ids);
/* Calls on this context served by the one-launch path so far (diagnostics / tests). */
uint64_t tk_small_path_calls(const tk_ctx* ctx);
/* Documents so far whose long piece (>= 1 KiB, not a vocabulary key) was merged in rounds by a whole workgroup
 * (csrc/tk_long.hip) instead of step by step by one wave (diagnostics / tests; TK_LONG_MIN overrides the threshold). */
uint64_t tk_round_path_docs(const tk_ctx* ctx);
/* Pieces of 65..256 bytes of the LAST batch that stayed on the flat path as records (csrc/tk_flat_chunk_impl.h step 6) instead of
 * handing their documents to the per-document kernels (diagnostics / tests; TK_FLAT_LONG=0 at context creation switches
 * the path off, TK_FLAT_LONG128=0 its one-lane-per-piece merge). */
uint64_t tk_long_piece_records(const tk_ctx* ctx);
/* 2048-byte regions of the LAST batch that held a piece of more than 64 bytes and went through the CUT instantiation of the
 * flat kernel (csrc/tk_flat_chunk_impl.h step 4b: such a piece is cut into fragments wherever no vocabulary token can span the
 * boundary, and the fragments merge independently -- exact; diagnostics / tests; TK_FLAT_CUT=0 switches the cuts off). */
uint64_t tk_cut_chunks(const tk_ctx* ctx);
/* Host waits of the LAST batch on the flat pipeline: 2 -- the list of the documents the flat kernel handed back (made on a
 * second stream beside the merge kernels), then the result; 3 only when a long-piece record flagged a document late
 * (diagnostics / tests; TK_TAIL=serial at context creation runs the tail behind the merge kernels on the one stream). */
uint64_t tk_last_host_syncs(const tk_ctx* ctx);

/* Memo of merged pieces (no reference equivalent; `encode` is a pure function of the text, src/tekkenizer.rs:384-386, and stays
 * one): a device table {piece of 2..16 bytes that is no vocabulary key -> the <= 5 ids the byte-pair merge gives it}, read by the
 * split + look-up kernel, filled behind the merge kernel, visible from the NEXT call on the context.  Text repeats its unknown
 * words; a hit costs one 32-byte gather instead of a chain of ~20 dependent PAIR probes.  An entry holds the exact key and the
 * exact result: the table can change how long a call takes, never an id (tests/test_gpu_parity.py::test_memo_*).
 *   log2_entries  0 = off (the table is freed); 10..26: 2^n entries of 32 bytes (default 24 = 512 MB of a 288 GB part, plus 64 MB for the log of a call's new entries; TK_MEMO_LOG2 --
 *                 measured on the held-out shape: 2^20 entries 0.66 of the look-ups hit, 2^22 0.77, 2^24 0.85: the table is direct-mapped)
 *   policy        0 = adaptive: after two calls in a row that hit less than once per 160 bytes of text or less than three times in
 *                 ten look-ups (text with few unknown pieces, or whose unknown pieces never come back) the table is left
 *                 alone for 30 calls; a call of under 1 MB of text never uses it (a context that only sees such calls never
 *                 allocates it).  1 = always on (TK_MEMO_POLICY=always)
 * tk_ctx_memo_clear empties the table.  tk_memo_stats: look-ups (pieces of 2..16 bytes that missed the vocabulary) and hits of
 * the last call and since the context was created, and whether the last call used the table. */
int tk_ctx_set_memo(tk_ctx* ctx, int log2_entries, int policy);
int tk_ctx_memo_clear(tk_ctx* ctx);
int tk_memo_stats(const tk_ctx* ctx, uint64_t* lookups_last, uint64_t* hits_last, uint64_t* lookups_total, uint64_t* hits_total,
                  int* active_last);

/* Opt-in: honour the `pattern` of Mistral's tekken.json -- case-aware words
 * (`HelloWorld` -> `Hello`, `World`), single digits, `/` absorbed after punctuation; literal in reference
 * tests/test_small_vocab.rs:62 -- instead of the pattern the reference hard-codes and always uses
 * (src/tekkenizer.rs:74,123).  mode 0 (default) = the reference's behaviour, 1 = the JSON pattern, on its own
 * instantiation of the same kernels (ASCII text at the default pipeline's rate). */
int tk_ctx_set_pattern(tk_ctx* ctx, int mode);

/* Streaming / pipelined ingestion (same results as tk_encode_batch, which is what the reference's
 * `encode` returns per document).  The batch is cut into slices of whole documents (about slice_bytes of text each,
 * 0 = default 32 MiB) that go through a three-stage pipeline on three HIP streams: host->device copy of slice k+1, the
 * kernels of slice k, device->host copy of the ids of slice k-1 (double-buffered device staging).  The caller owns all
 * four host buffers; when they come from tk_host_alloc (pinned memory) every copy is an asynchronous DMA and the three
 * stages overlap -- pageable buffers work too, at the runtime's staged-copy rate.
 *   ids_out       capacity ids_capacity; doc_offsets[n_docs] + 2 * n_docs always suffices (a document produces at most
 *                 one id per byte, plus BOS / EOS)
 *   offsets_out   n_docs + 1 entries
 * TK_ERR_INVALID_ARG if the ids do not fit (*n_ids then holds the count reached when it was noticed). */
void* tk_host_alloc(size_t bytes);      /* pinned host memory (NULL on failure) */
void tk_host_free(void* p);
int tk_encode_batch_pipelined(tk_ctx* ctx, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs,
                              int add_bos, int add_eos, uint64_t slice_bytes, uint32_t* ids_out, uint64_t ids_capacity,
                              uint64_t* offsets_out, uint64_t* n_ids);

/* Same computation with inputs already resident in HBM (hipMalloc'ed on the context's device):
 * d_bytes = n_bytes packed text bytes, d_doc_offsets = n_docs+1 uint64 (non-decreasing, [0] = 0, [n_docs] = n_bytes:
 * not checked on this entry -- tk_encode_batch_device_ex checks).  Work is enqueued on
 * `hip_stream` (a hipStream_t; NULL = HIP's null stream, so the work is ordered after whatever the
 * caller already enqueued there) and the call returns after the stream has drained.  *d_ids / *d_out_offsets are device buffers owned by the context, valid
 * until the next call on it; *n_ids = total ids. */
int tk_encode_batch_device(tk_ctx* ctx, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs,
                           uint64_t n_bytes, int add_bos, int add_eos, void* hip_stream, void** d_ids,
                           void** d_out_offsets, uint64_t* n_ids);

/* The same with the checks tk_encode_batch makes for host callers, on the device (one small kernel and one host wait each, before
 * anything else runs): TK_CHECK_OFFSETS -- d_doc_offsets[0] == 0, non-decreasing, [n_docs] == n_bytes, else TK_ERR_INVALID_ARG;
 * TK_CHECK_UTF8 -- every document is well-formed UTF-8 on its own (a Rust &str always is; this includes "no document starts inside
 * a code point"), else TK_ERR_INVALID_UTF8; implies the offsets check.  checks = 0 is tk_encode_batch_device. */
#define TK_CHECK_OFFSETS 1
#define TK_CHECK_UTF8 2
int tk_encode_batch_device_ex(tk_ctx* ctx, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                              int add_bos, int add_eos, int checks, void* hip_stream, void** d_ids, void** d_out_offsets,
                              uint64_t* n_ids);

/* ---- per-token byte spans (HF tokenizers' offset_mapping; no reference equivalent -- decode_all, src/tekkenizer.rs:463-560,
 * gives per-segment strings, not positions in the input) ----
 * For each output id i of document d, the span is spans[2i], spans[2i+1] = (start, end).  Both are uint32 byte offsets
 * relative to the start of document d.
 *   - A non-special id covers end - start = len(token bytes), and bytes[doc_start+start : doc_start+end] equals those token
 *     bytes.
 *   - BOS is (0, 0).  EOS is (doc_len, doc_len).  In general a special id gets a zero-length span at the current position.
 *   - A document of 2^32 bytes or more makes the spans entries fail with TK_ERR_INVALID_ARG.  The encode entries are not
 *     affected.
 *   - Offsets are in BYTES, not characters: a token can end inside a UTF-8 character (the byte-fallback tokens of an emoji or a
 *     rare CJK character do).  Code-point and UTF-16 offsets come from the units entries below (tk_token_spans_units_device),
 *     the tokens an annotated range covers from tk_spans_locate_device.
 * Encode is lossless (byte-level BPE tiles the text; the only specials it emits are BOS / EOS), so the spans of encode's ids
 * are a per-document exclusive prefix sum of the ids' byte lengths (a special id: 0) -- a separate pass behind the encode
 * pipeline (csrc/tk_spans.hip), which can check the ids against the text in the same pass.  `checks` is a bit field that sits
 * above TK_CHECK_OFFSETS / TK_CHECK_UTF8, so one word can carry all four:
 *   TK_SPANS_CHECK_COVER  the last end of every document equals doc_offsets[d+1] - doc_offsets[d] (a document without ids:
 *                         doc_len == 0)
 *   TK_SPANS_CHECK_BYTES  implies COVER; the token bytes of every non-special id equal the text under its span -- the round
 *                         trip decode(encode(x)) == x, id by id
 * A failed check returns TK_ERR_RUNTIME (the message names the document and the two lengths) and writes the first failing
 * document to *bad_doc (optional); an id outside the vocabulary is TK_ERR_RUNTIME too. */
#define TK_SPANS_CHECK_COVER 4
#define TK_SPANS_CHECK_BYTES 8
/* Spans of ids already on the device (any ids: encode's own outputs, or the caller's).  d_doc_offsets (n_docs + 1 uint64,
 * well-formed) is needed only for a check, d_bytes only for TK_SPANS_CHECK_BYTES (NULL otherwise).  *d_spans (2 * n_ids uint32)
 * is a device buffer owned by the context, valid until the next spans call on it, and SEPARATE from the encode outputs: the
 * d_ids / d_out_offsets the previous encode call on the same context returned stay valid through this call.  The work is
 * enqueued on hip_stream and the call returns after the stream has drained. */
int tk_token_spans_device(tk_ctx* ctx, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                          const void* d_doc_offsets, const void* d_bytes, int checks, void* hip_stream, void** d_spans,
                          uint64_t* bad_doc);
/* tk_encode_batch_device_ex + the spans pass on the same stream.  checks may combine TK_CHECK_OFFSETS / TK_CHECK_UTF8 (encode's
 * input checks) with TK_SPANS_CHECK_COVER / TK_SPANS_CHECK_BYTES.  *d_ids / *d_out_offsets as tk_encode_batch_device, *d_spans
 * as tk_token_spans_device. */
int tk_encode_batch_device_spans(tk_ctx* ctx, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                 int add_bos, int add_eos, int checks, void* hip_stream, void** d_ids, void** d_out_offsets,
                                 void** d_spans, uint64_t* n_ids, uint64_t* bad_doc);
/* Host in / host out: tk_encode_batch + spans (batches of the one-launch small path included).  *spans is pinned, 2 * n_ids
 * entries, free with tk_free_spans; out as tk_encode_batch (tk_free_result). */
int tk_encode_batch_spans(tk_ctx* ctx, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos,
                          int add_eos, int validate_utf8, int checks, tk_result* out, uint32_t** spans, uint64_t* bad_doc);
void tk_free_spans(uint32_t* spans);

/* ---- spans in code points or UTF-16 units, and annotation -> token range (HF's offset_mapping over a str, char_to_token; no
 * reference equivalent) ----
 * The unit a caller's strings are indexed in: a Python str by code point, a JavaScript / Java / LSP string by UTF-16 unit.  The
 * definition is by BYTES, so it holds for any input, valid UTF-8 or not.
 *   - A document's text T is the concatenation of the token bytes of its non-special ids (for encode's output: the document).
 *   - The weight of a byte b is u(b) = ((b & 0xC0) != 0x80); TK_UNIT_UTF16 adds 1 more when b >= 0xF0; TK_UNIT_BYTE: u = 1.
 *   - U(p) = the sum of u(T[q]) over q < p.
 *   - lead(p) = the largest q <= p with (T[q] & 0xC0) != 0x80, or 0 if there is none; TK_UNIT_BYTE: lead(p) = p.
 * The unit span of an id with byte span (s, e):
 *   - s == e (a special id): (U(s), U(s)).
 *   - otherwise (U(lead(s)), U(e)): a token that begins or ends inside a character is widened to that whole character.  The four
 *     byte-fallback tokens of an emoji at character c are all (c, c + 1) in code points and (c, c + 2) in UTF-16 units.
 *   - Nothing carries across a document boundary: a document that begins with continuation bytes has lead = 0 there.
 * Starts and ends are non-decreasing along a document.  A document of 2^32 units or more is TK_ERR_INVALID_ARG, an id outside
 * the vocabulary TK_ERR_RUNTIME, as in the byte pass.  The pass reads no text: a per-rank table and two wave scans
 * (csrc/tk_spans_units.hip). */
#define TK_UNIT_BYTE 0
#define TK_UNIT_CHAR 1    /* Unicode code points: the index of a Python str */
#define TK_UNIT_UTF16 2   /* UTF-16 code units */
/* Unit spans of ids already on the device (any ids).  *d_spans (2 * n_ids uint32) is a device buffer owned by the context, valid
 * until the next units call on it, and a buffer of its OWN: the byte spans of an earlier tk_token_spans_device call and every
 * encode output stay valid through this call.  TK_UNIT_BYTE gives what tk_token_spans_device gives.  An unknown unit is
 * TK_ERR_INVALID_ARG.  The work is enqueued on hip_stream and the call returns after the stream has drained. */
int tk_token_spans_units_device(tk_ctx* ctx, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids, int unit,
                                void* hip_stream, void** d_spans);
/* tk_encode_batch_device_ex + the units pass on the same stream.  checks takes TK_CHECK_OFFSETS / TK_CHECK_UTF8 only: a
 * TK_SPANS_CHECK_* bit is TK_ERR_INVALID_ARG (those checks belong to the byte pass, which the caller can run as well). */
int tk_encode_batch_device_spans_units(tk_ctx* ctx, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                       int add_bos, int add_eos, int checks, int unit, void* hip_stream, void** d_ids,
                                       void** d_out_offsets, void** d_spans, uint64_t* n_ids);
/* Host in / host out: tk_encode_batch + the units pass (batches of the one-launch small path included).  *spans is pinned,
 * 2 * n_ids entries, free with tk_free_spans; out as tk_encode_batch (tk_free_result). */
int tk_encode_batch_spans_units(tk_ctx* ctx, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos,
                                int add_eos, int validate_utf8, int unit, tk_result* out, uint32_t** spans);
/* Which ids does an annotated range cover?  d_spans: 2 * n_ids uint32 spans in any unit whose starts and ends are non-decreasing
 * along a document (the byte or the units pass); d_ann_doc: uint32[n_ann], the document of every annotation; d_ann: uint32[n_ann, 2],
 * (as, ae) in the unit of d_spans.  With (S_i, E_i) the spans of document d:
 *     lo = #{i : E_i <= as},  hi = #{i : S_i < ae},  d_tok_range[a] = (lo, max(lo, hi))
 * -- a pair of document-relative id indices (uint32[n_ann, 2], owned by the context, valid until the next locate call on it, apart
 * from every other output).  For encode's output the ids whose span overlaps [as, ae) are exactly lo .. hi - 1; HF's
 * char_to_token(c) is the annotation (c, c + 1); BOS and EOS are never inside a non-empty range.  One lane per annotation, two
 * binary searches; every probe stays inside [id_offsets[d], id_offsets[d + 1]), whatever the spans hold.
 * ann_doc >= n_docs or as > ae is TK_ERR_INVALID_ARG: the first such annotation is written to *bad_ann (optional), nothing else is
 * checked, and the result of an earlier call stays readable.  n_ann == 0 and documents without ids are valid. */
int tk_spans_locate_device(tk_ctx* ctx, const void* d_spans, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                           const void* d_ann_doc, const void* d_ann, uint64_t n_ann, void* hip_stream, void** d_tok_range,
                           uint64_t* bad_ann);

/* ---- model-ready dense batches: truncation, padding, mask, and back (no reference equivalent: pad_id(), src/tekkenizer.rs:304,
 * is all the reference has) ----
 * Input: the ragged ids R_d = ids[oo[d] : oo[d+1]], n_d = len(R_d), d < D; options max_length T (0 = no limit), multiple_of m
 * (0 = none), pad_id, keep_head h, keep_tail t and the flags below.
 *   1. lim = T if T > 0, else unbounded.
 *   2. Kept ids K_d: n_d <= lim: K_d = R_d.  Otherwise, truncating on the right (default), K_d = R_d[: lim - t] + R_d[n_d - t :];
 *      with TK_DENSE_TRUNC_LEFT, K_d = R_d[: h] + R_d[n_d - (lim - h) :].  len(K_d) = min(n_d, lim); the first h / last t ids of a
 *      document survive truncation (the fused encode entries set h = add_bos, t = add_eos: BOS and EOS are kept and the text
 *      between them is cut, as HF tokenizers does).
 *   3. Row length: L = T with TK_DENSE_FIXED (which needs T > 0), else L = min(max_d n_d, lim) (0 for an empty batch or all-empty
 *      documents); then, if m > 0, L is rounded up to a multiple of m.  Truncation is to lim, never to the rounded L.
 *   4. Row d of dense[D, L] is K_d followed by pad_id, or with TK_DENSE_PAD_LEFT pad_id first and K_d flush right.  mask[D, L]
 *      (uint8, only with TK_DENSE_MASK, else NULL) is 1 under K_d, 0 under padding.  lengths[d] = len(K_d) (uint32, always).
 *      n_truncated = number of documents with n_d > lim.  Elements are int32, or int64 with TK_DENSE_I64 (ids are < 2^31).
 *   5. TK_ERR_INVALID_ARG, nothing written, an earlier dense result stays readable: T > 0 and (t > T truncating right, h > T
 *      truncating left; in the fused entries add_bos + add_eos > T); TK_DENSE_FIXED with T == 0; an unknown flag; a tensor
 *      beyond the bounds L < 2^31 and D * L <= 2^36 elements.  A failed allocation is TK_ERR_RUNTIME.
 * The layout is a separate pass behind the unchanged encode pipeline (csrc/tk_dense.hip): every element is written once, pad
 * included, in 16-byte stores where L is a multiple of 4 (element stores otherwise: pad to a multiple of 4 for the fast form).
 * The longest-row mode reads max_d n_d back (8 bytes) before it can size the tensor; TK_DENSE_FIXED needs no read before the
 * launch. */
#define TK_DENSE_PAD_LEFT 1
#define TK_DENSE_TRUNC_LEFT 2
#define TK_DENSE_FIXED 4
#define TK_DENSE_I64 8
#define TK_DENSE_MASK 16
typedef struct tk_dense_opts { uint32_t max_length, multiple_of, pad_id, keep_head, keep_tail, flags; } tk_dense_opts;
typedef struct tk_dense { void* ids; uint8_t* mask; uint32_t* lengths; uint64_t n_docs, row_len, n_truncated; } tk_dense;
/* ids already on the device (encode's own outputs or the caller's; d_id_offsets: n_docs + 1 uint64, well-formed) -> dense.
 * out's buffers are device buffers owned by the context, valid until the next dense call on it, and SEPARATE from the encode
 * and spans outputs: an earlier encode's d_ids / d_out_offsets stay valid through this call.  The work is enqueued on hip_stream
 * and the call returns after the stream has drained.  This entry does NOT check d_id_offsets (the fused entry below takes
 * TK_CHECK_OFFSETS for its text offsets; the id offsets it passes on are encode's own): a decreasing pair or an offset beyond
 * n_ids is out-of-bounds indexing on the device. */
int tk_dense_from_ids_device(tk_ctx* ctx, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                             const tk_dense_opts* opts, void* hip_stream, tk_dense* out);
/* tk_encode_batch_device_ex + the dense pass on the same stream.  keep_head / keep_tail of opts are ignored and set from
 * add_bos / add_eos; the ragged outputs (*d_ids / *d_out_offsets / *n_ids as tk_encode_batch_device) are returned as well. */
int tk_encode_batch_device_dense(tk_ctx* ctx, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                 int add_bos, int add_eos, int checks, const tk_dense_opts* opts, void* hip_stream,
                                 void** d_ids, void** d_out_offsets, uint64_t* n_ids, tk_dense* out);
/* Host in / host out: tk_encode_batch + the dense pass (batches of the one-launch small path included).  out's buffers are
 * pinned host memory, released with tk_free_dense (out->mask is NULL without TK_DENSE_MASK). */
int tk_encode_batch_dense(tk_ctx* ctx, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos,
                          int add_eos, int validate_utf8, const tk_dense_opts* opts, tk_dense* out);
void tk_free_dense(tk_dense* out);
/* The inverse: dense rows on the device -> ragged ids + offsets.  flags: TK_DENSE_I64 (the element type), TK_DENSE_PAD_LEFT.
 * lengths[d] comes from d_lengths (n_docs uint32, clamped to row_len), or, when d_lengths is NULL, is row_len minus the maximal
 * run of pad_id at the padded end of the row (the right end, or the left with TK_DENSE_PAD_LEFT); R_d is the lengths[d] ids at
 * the unpadded end, the offsets their exclusive prefix sum.  ragged(dense(x)) == x whenever nothing was truncated and pad_id does
 * not end (begin) a document -- encode never emits <pad>.  *d_ids (uint32) / *d_id_offsets (n_docs + 1 uint64) are owned by the
 * context and apart from the decode buffers: valid through a following tk_decode_batch_device on the same context, until the
 * next call of this entry. */
int tk_ragged_from_dense_device(tk_ctx* ctx, const void* d_dense, uint64_t n_docs, uint64_t row_len, int flags,
                                const void* d_lengths, uint32_t pad_id, void* hip_stream, void** d_ids,
                                void** d_id_offsets, uint64_t* n_ids);

/* ---- packed fixed-length training rows: input_ids, position_ids, segment_ids, cu_seqlens (no reference equivalent: pad_id(),
 * src/tekkenizer.rs:304, is all the reference has) ----
 * Pre-training does not pad documents: it concatenates them, BOS / EOS included, into one stream and cuts the stream into rows
 * of seq_len.  Input: the ragged ids R_d = ids[oo[d] : oo[d+1]], d < D; N = oo[D]; options seq_len = L (required, > 0), pad_id
 * and the flags below.
 *   1. The stream is S = R_0 + R_1 + ... + R_{D-1}: the ids are already concatenated, S[g] = ids[g].  n_rows = ceil(N / L), or
 *      floor(N / L) with TK_SEQPACK_DROP_LAST; n_used = min(N, n_rows * L); n_left = N - n_used.  The ids ids[n_used :] are left
 *      for the caller to carry into its next batch (carrying them across calls is the caller's business).
 *   2. input_ids[r, c] = ids[g] with g = r * L + c, if g < n_used, else pad_id.  Only the last row can hold pads, and only
 *      without DROP_LAST.
 *   3. A segment is a maximal run of positions g < n_used that lie in one document and in one row.  Its starts are
 *      B = sorted({oo[d] : n_d > 0, oo[d] < n_used} u {r * L : r * L < n_used}), without duplicates: empty documents make no
 *      segment, a document that crosses a row boundary is split there.  n_segments = |B|.
 *   4. position_ids[r, c] = g - (start of g's segment); a pad gets 0.  Positions restart at a document start and at a row
 *      start: the continued part of a document cannot see its head in the previous row.
 *   5. segment_ids[r, c] = 1 + the number of segment starts in (r * L, g]: segments are numbered 1, 2, 3, ... within a row; a
 *      pad gets 0.
 *   6. cu_seqlens (int32, n_segments + 1 entries) is B followed by n_used: offsets into the flattened [n_rows * L] tensor, pads
 *      lie beyond its last entry.  max_seqlen = max diff(cu_seqlens); 0 when n_used == 0, where cu_seqlens = [0].  n_segments
 *      and max_seqlen are filled whether or not cu_seqlens is selected.
 *   7. input_ids, position_ids and segment_ids are int32, or int64 with TK_SEQPACK_I64; cu_seqlens is always int32.
 *      TK_SEQPACK_POSITIONS, TK_SEQPACK_SEGMENTS and TK_SEQPACK_CU_SEQLENS select the optional outputs; an unselected output is
 *      NULL.
 *   8. TK_ERR_INVALID_ARG, nothing written, an earlier packed result stays readable: L == 0; L >= 2^31; an unknown flag;
 *      n_rows * L > 2^36; TK_SEQPACK_CU_SEQLENS with n_used >= 2^31; n_docs == 0 with n_ids > 0.  A failed allocation is TK_ERR_RUNTIME.  D == 0 or N == 0
 *      is valid and gives n_rows == 0.
 * The layout is a separate pass behind the unchanged encode pipeline (csrc/tk_seqpack.hip): every element is written once, pad
 * included, in 16-byte stores where L is a multiple of 4 (element stores otherwise).  n_rows, n_used and n_left follow from
 * n_ids on the host: nothing is read before the launches, and one wait at the end reads n_segments and max_seqlen. */
#define TK_SEQPACK_I64 1
#define TK_SEQPACK_POSITIONS 2
#define TK_SEQPACK_SEGMENTS 4
#define TK_SEQPACK_CU_SEQLENS 8
#define TK_SEQPACK_DROP_LAST 16
typedef struct tk_seqpack_opts { uint32_t seq_len, pad_id, flags; } tk_seqpack_opts;
typedef struct tk_seqpack { void *input_ids, *position_ids, *segment_ids; int32_t* cu_seqlens;
                            uint64_t n_rows, row_len, n_used, n_left, n_segments, max_seqlen; } tk_seqpack;
/* ids already on the device (encode's own outputs or the caller's; d_id_offsets: n_docs + 1 uint64, [0] = 0, non-decreasing,
 * [n_docs] = n_ids -- NOT checked, as in tk_dense_from_ids_device: anything else is out-of-bounds indexing on the device) ->
 * packed rows.  out's buffers are device buffers owned by the context, valid until the next packed call on it, and SEPARATE from
 * the encode, spans, dense and decode outputs.  The work is enqueued on hip_stream and the call returns after the stream has
 * drained. */
int tk_seqpack_from_ids_device(tk_ctx* ctx, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                               const tk_seqpack_opts* opts, void* hip_stream, tk_seqpack* out);
/* tk_encode_batch_device_ex + the packed pass on the same stream; the ragged outputs (*d_ids / *d_out_offsets / *n_ids as
 * tk_encode_batch_device) are returned as well: ids[out->n_used :] is what the caller carries on. */
int tk_encode_batch_device_seqpack(tk_ctx* ctx, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                   int add_bos, int add_eos, int checks, const tk_seqpack_opts* opts, void* hip_stream,
                                   void** d_ids, void** d_out_offsets, uint64_t* n_ids, tk_seqpack* out);
/* Host in / host out: tk_encode_batch + the packed pass (batches of the one-launch small path included).  out's buffers are
 * pinned host memory, released with tk_free_seqpack (an unselected output is NULL). */
int tk_encode_batch_seqpack(tk_ctx* ctx, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos, int add_eos,
                            int validate_utf8, const tk_seqpack_opts* opts, tk_seqpack* out);
void tk_free_seqpack(tk_seqpack* out);

/* ---- overlapping windows for long documents: max_length, stride, mapping (no reference equivalent: pad_id(),
 * src/tekkenizer.rs:304, is all the reference has; HF tokenizers calls this return_overflowing_tokens with a stride and
 * overflow_to_sample_mapping) ----
 * A document that is longer than the model's context and must not be cut is split into windows of max_length ids that overlap by
 * stride ids; every window carries the document's own head and tail (BOS / EOS).  Input: the ragged ids R_d = ids[oo[d] : oo[d+1]],
 * n_d = len(R_d), d < D; options max_length T (required, > 0), stride s, multiple_of m (0 = none), pad_id, keep_head h, keep_tail t
 * and the flags below.
 *   1. Body capacity c = T - h - t; the step between windows is step = c - s.  c >= 1 and 0 <= s < c are required.
 *   2. A document with n_d <= T gives ONE window: R_d as it lies (empty documents too: every document has at least one window).
 *   3. A document with n_d > T is split.  Its body is B = R_d[h : n_d - t], b = n_d - h - t; it has w_d = 1 + ceil((b - c) / step)
 *      windows, and window k is R_d[:h] + B[k * step : min(k * step + c, b)] + R_d[n_d - t :].  Consecutive windows share s body
 *      ids; the last window may be shorter (it is not right-aligned, as in HF tokenizers).  The first h and last t ids are repeated
 *      in every window (the fused entries set h = add_bos, t = add_eos).
 *   4. Windows are numbered document by document: doc_windows (uint64, D + 1 entries) is the exclusive prefix sum of w_d, strictly
 *      increasing, and W = doc_windows[D].
 *   5. Row length: L = T with TK_WINDOW_FIXED, else L = min(max_d n_d, T) (0 for an empty batch or all-empty documents); then, if
 *      m > 0, L is rounded up to a multiple of m.
 *   6. Outputs, elements int32 or int64 with TK_WINDOW_I64: input_ids[W, L] is the window followed by pad_id (padding on the right
 *      only); mask[W, L] (uint8, only with TK_WINDOW_MASK, else NULL) is 1 under the window; lengths[W] (uint32); window_doc[W]
 *      (uint32) the document of every window (overflow_to_sample_mapping); window_start[W] (uint32) = min(h + k * step, n_d), the
 *      index in R_d of the window's first body id; doc_windows as in 4; n_windows = W; n_split = the documents with w_d > 1.
 *   7. With TK_WINDOW_SPANS, spans[W, L, 2] (uint32) holds the (start, end) byte span of the id under every element, taken from a
 *      spans buffer with the layout of tk_token_spans_device's output (2 * n_ids uint32); a pad gets (0, 0).
 *   8. TK_ERR_INVALID_ARG, nothing written, an earlier window result stays readable: T == 0; h + t >= T (in the fused entries
 *      add_bos + add_eos >= T); s >= c; an unknown flag; T or the rounded L beyond 2^31 - 1; W >= 2^32; W * L > 2^36;
 *      TK_WINDOW_SPANS without a spans buffer in the from-ids entry; n_docs == 0 with n_ids > 0; a document of 2^32 - 1 ids or more
 *      (window_start is uint32).  A failed allocation is TK_ERR_RUNTIME.  D == 0 is valid and gives W == 0.
 * The layout is a separate pass behind the unchanged encode pipeline (csrc/tk_window.hip): every element of every selected output is
 * written once, pad included, in 16-byte stores where L is a multiple of 4 (element stores otherwise).  W is not known before the
 * per-document counts have been summed: one small read (W and max_d n_d) sizes the tensor, and one wait ends the call. */
#define TK_WINDOW_FIXED 1
#define TK_WINDOW_I64 2
#define TK_WINDOW_MASK 4
#define TK_WINDOW_SPANS 8
typedef struct tk_window_opts { uint32_t max_length, stride, multiple_of, pad_id, keep_head, keep_tail, flags; } tk_window_opts;
typedef struct tk_window { void* input_ids; uint8_t* mask; uint32_t *lengths, *window_doc, *window_start; uint64_t* doc_windows;
                           uint32_t* spans; uint64_t n_docs, n_windows, row_len, n_split; } tk_window;
/* ids already on the device (encode's own outputs or the caller's; d_id_offsets: n_docs + 1 uint64, [0] = 0, non-decreasing,
 * [n_docs] = n_ids -- NOT checked, as in tk_dense_from_ids_device: anything else is out-of-bounds indexing on the device) ->
 * windows.  d_spans: 2 * n_ids uint32 as tk_token_spans_device returns them, NULL without TK_WINDOW_SPANS.  out's buffers are
 * device buffers owned by the context, valid until the next window call on it, and SEPARATE from the encode, spans, dense, packed,
 * join and decode outputs.  The work is enqueued on hip_stream and the call returns after the stream has drained. */
int tk_window_from_ids_device(tk_ctx* ctx, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                              const void* d_spans, const tk_window_opts* opts, void* hip_stream, tk_window* out);
/* tk_encode_batch_device_ex + (with TK_WINDOW_SPANS) the spans pass + the window pass on the same stream.  keep_head / keep_tail
 * of opts are ignored and set from add_bos / add_eos; checks: TK_CHECK_OFFSETS / TK_CHECK_UTF8 as in tk_encode_batch_device_dense;
 * the ragged outputs (*d_ids / *d_out_offsets / *n_ids as tk_encode_batch_device) are returned as well. */
int tk_encode_batch_device_window(tk_ctx* ctx, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                  int add_bos, int add_eos, int checks, const tk_window_opts* opts, void* hip_stream,
                                  void** d_ids, void** d_out_offsets, uint64_t* n_ids, tk_window* out);
/* Host in / host out: tk_encode_batch + the window pass (batches of the one-launch small path included).  out's buffers are
 * pinned host memory, released with tk_free_window (an unselected output is NULL). */
int tk_encode_batch_window(tk_ctx* ctx, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos, int add_eos,
                           int validate_utf8, const tk_window_opts* opts, tk_window* out);
void tk_free_window(tk_window* out);

/* ---- boundary-aware token-budget chunks: long documents cut at breaks of the text (no reference equivalent: pad_id(),
 * src/tekkenizer.rs:304, is all the reference has; the definition is this project's own -- what LangChain's
 * RecursiveCharacterTextSplitter.from_tiktoken_encoder, LlamaIndex's SentenceSplitter and semchunk do by calling a tokenizer over
 * and over on the host) ----
 * The window pass cuts every `step` ids wherever that falls; this pass cuts a document of more than max_length ids at the strongest
 * break of the text that a chunk of at least min_length body ids can end at.  Input: the ragged ids R_d = ids[oo[d] : oo[d+1]],
 * n_d = len(R_d), d < D; one LEVEL byte per id; optionally the spans buffer of tk_token_spans_device (2 * n_ids uint32); options
 * max_length T (required, > 0), min_length m, overlap o, multiple_of (0 = none), pad_id, keep_head h, keep_tail t, levels (a bit
 * mask, for tk_chunk_levels_device and the entries that encode first) and the flags below.  Let c = T - h - t; c >= 1 and
 * 0 <= o < m <= c are required.
 *   Levels.  lev[i] (uint8) is the strength of the break in front of id i: 0 NONE (inside a character), 1 TOKEN, 2 WORD, 3 SENTENCE,
 *   4 LINE, 5 PARAGRAPH (a byte above 5 reads as 5).  Either the caller gives the bytes (how a syntax-aware choice comes in, as with
 *   the FIM cuts), or tk_chunk_levels_device makes them from text and spans, a total function of bytes only: with text the bytes of
 *   document d, len their number, p the span start of id i and WS the six ASCII bytes 0x09 .. 0x0D and 0x20, first match wins:
 *     1. p >= len or p == 0: TOKEN.
 *     2. (text[p] & 0xC0) == 0x80: NONE.
 *     3. Walk back from p over WS bytes to q: the walk ends in front of the first byte that is not WS, at byte 0, or after 16 bytes
 *        -- then it was stopped by the bound, whatever lies further in front.  nl = the 0x0A among text[q : p]: nl >= 2 PARAGRAPH,
 *        nl == 1 LINE.
 *     4. gap = (q < p) or text[p] in WS.  If the walk was not stopped by the bound and q > 0: SENTENCE if gap and text[q - 1] is one
 *        of . ! ?; SENTENCE also if q >= 3 and text[q - 3 : q] is one of E3 80 82, EF BC 81, EF BC 9F (the ideographic full stop,
 *        the fullwidth ! and ?; no white space needed).
 *     5. Otherwise WORD if gap, else TOKEN.
 *   Then the mask: a level in 2 .. 5 whose bit 1 << level is not in `levels` is demoted to the highest enabled level below it, or
 *   to TOKEN; NONE and TOKEN cannot be disabled.  No read leaves text[0 : len].
 *   Walk, per document.
 *     1. n_d <= T gives ONE chunk: R_d as it lies (empty documents too, as rule 2 of the window pass).
 *     2. Otherwise the body is B = R_d[h : n_d - t], b = n_d - h - t, and L(j) = lev[oo[d] + h + j].  Start at a = 0.
 *     3. b - a <= c: the last chunk is [a, b).  Otherwise the candidates are the j in [a + m, a + c], best = max L(j) over them, the
 *        cut e is the LARGEST candidate with L(e) == best, and the chunk is [a, e) with cut_level = best.
 *     4. The next start is the smallest j in [max(a + 1, e - o), e) with L(j) >= WORD; if there is none, the smallest there with
 *        L(j) >= TOKEN; if there is none, e.  Go to 3.
 *     5. Row k of the document is R_d[:h] + B[a_k : e_k] + R_d[n_d - t :].
 *   It follows that a_k < a_{k+1} <= e_k < e_{k+1}, e_k - a_{k+1} <= o, m <= e_k - a_k <= c for all but the last chunk, a_0 = 0,
 *   e_last = b and w_d <= 1 + ceil((b - c) / (m - o)); with every level equal the chunks are the window pass's windows at
 *   stride = o, for any valid m.
 *   Outputs.  input_ids[W, L], mask, lengths, window_doc, window_start = min(h + a_k, n_d), doc_windows and spans[W, L, 2] (with
 *   TK_CHUNK_SPANS) mean exactly what they mean in tk_window, and so do the row-length rules (TK_CHUNK_FIXED, multiple_of, int32 or
 *   int64 with TK_CHUNK_I64, TK_CHUNK_MASK).  cut_level[W] (uint8): the level of the cut that ended the chunk, TK_CHUNK_CUT_LAST
 *   (255) for a document's last chunk.  chunk_bytes[W, 2] (uint32, with TK_CHUNK_BYTES, which needs spans): the span start of the
 *   chunk's first body id and the span end of its last; for an unsplit document from its first id's start to its last id's end,
 *   (0, 0) for one without ids.  level_counts (uint64[6]): the cuts made at every level -- the quality figure: a high count at
 *   NONE or TOKEN says min_length is too close to max_length.  Counts: n_docs, n_windows = W, row_len = L, n_split.
 *   TK_ERR_INVALID_ARG, nothing written, an earlier chunk result stays readable: the window pass's list with stride read as
 *   overlap; m == 0, m > c or o >= m; a levels bit outside 2 .. 5; TK_CHUNK_BYTES or TK_CHUNK_SPANS without a spans buffer; ids
 *   without a level buffer in the from-ids entry.  A failed allocation is TK_ERR_RUNTIME.  D == 0 is valid and gives W == 0.
 * A separate pass behind the unchanged encode pipeline (csrc/tk_chunk.hip): the levels kernel; the walk, run twice (the counts, then
 * -- behind their scan and ONE small read that sizes the tensors -- the windows' records); the fill kernel, the window pass's with
 * one more load a row.  One wait ends the call. */
#define TK_CHUNK_FIXED 1
#define TK_CHUNK_I64 2
#define TK_CHUNK_MASK 4
#define TK_CHUNK_SPANS 8
#define TK_CHUNK_BYTES 16
#define TK_CHUNK_LEVEL_NONE 0
#define TK_CHUNK_LEVEL_TOKEN 1
#define TK_CHUNK_LEVEL_WORD 2
#define TK_CHUNK_LEVEL_SENTENCE 3
#define TK_CHUNK_LEVEL_LINE 4
#define TK_CHUNK_LEVEL_PARAGRAPH 5
#define TK_CHUNK_LEVELS_ALL 60
#define TK_CHUNK_CUT_LAST 255
typedef struct tk_chunk_opts { uint32_t max_length, min_length, overlap, multiple_of, pad_id, keep_head, keep_tail, levels, flags; } tk_chunk_opts;
typedef struct tk_chunk { void* input_ids; uint8_t* mask; uint32_t *lengths, *window_doc, *window_start; uint64_t* doc_windows;
                          uint32_t* spans; uint8_t* cut_level; uint32_t* chunk_bytes; uint64_t* level_counts;
                          uint64_t n_docs, n_windows, row_len, n_split; } tk_chunk;
/* The level bytes of ids whose spans are on the device (d_spans: 2 * n_ids uint32 as tk_token_spans_device returns them;
 * d_id_offsets as below; d_bytes / d_doc_offsets: the text the ids were encoded from) under the mask `levels` (bits 1 << 2 ..
 * 1 << 5; another bit: TK_ERR_INVALID_ARG) -> *d_levels, n_ids uint8 in a device buffer owned by the context, valid until the next
 * call that makes levels on it. */
int tk_chunk_levels_device(tk_ctx* ctx, const void* d_spans, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                           const void* d_bytes, const void* d_doc_offsets, uint64_t n_bytes, uint32_t levels, void* hip_stream,
                           void** d_levels);
/* ids and their level bytes already on the device (d_id_offsets: n_docs + 1 uint64, [0] = 0, non-decreasing, [n_docs] = n_ids -- NOT
 * checked, as in tk_window_from_ids_device: anything else is out-of-bounds indexing on the device) -> chunks.  d_levels: n_ids
 * uint8, the caller's or tk_chunk_levels_device's; d_spans: NULL without TK_CHUNK_SPANS and TK_CHUNK_BYTES; opts->levels is checked
 * and not used.  out's buffers are device buffers owned by the context, valid until the next chunk call on it, and SEPARATE from
 * every other pass's outputs.  The work is enqueued on hip_stream and the call returns after the stream has drained. */
int tk_chunk_from_ids_device(tk_ctx* ctx, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                             const void* d_levels, const void* d_spans, const tk_chunk_opts* opts, void* hip_stream, tk_chunk* out);
/* tk_encode_batch_device_ex + the spans pass (into a buffer of the chunk pass: tk_token_spans_device's result stays as it is) + the
 * levels + the chunk pass on the same stream.  keep_head / keep_tail of opts are ignored and set from add_bos / add_eos; checks:
 * TK_CHECK_OFFSETS / TK_CHECK_UTF8 as in tk_encode_batch_device_dense; the ragged outputs (*d_ids / *d_out_offsets / *n_ids as
 * tk_encode_batch_device) are returned as well. */
int tk_encode_batch_device_chunk(tk_ctx* ctx, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                 int add_bos, int add_eos, int checks, const tk_chunk_opts* opts, void* hip_stream,
                                 void** d_ids, void** d_out_offsets, uint64_t* n_ids, tk_chunk* out);
/* Host in / host out: tk_encode_batch + the same passes (batches of the one-launch small path included).  out's buffers are pinned
 * host memory, released with tk_free_chunk (an unselected output is NULL). */
int tk_encode_batch_chunk(tk_ctx* ctx, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos, int add_eos,
                          int validate_utf8, const tk_chunk_opts* opts, tk_chunk* out);
void tk_free_chunk(tk_chunk* out);
/* Milliseconds of the stages of the last chunk call on the context: [0] the levels kernel (of the last call that made levels),
 * [1] the two walks and the scan, [2] the fill kernel. */
void tk_last_chunk_ms(const tk_ctx* ctx, float ms[3]);

/* ---- chat batches: text parts joined with control ids, plus labels (no reference equivalent: the reference never makes a
 * control token out of text -- "[INST]" in the input stays plain text -- and get_control_token, src/tekkenizer.rs:331-341, only
 * hands out the id) ----
 * A batch has C conversations over P parts.  Conversation c owns parts conv_offsets[c] .. conv_offsets[c+1] (C + 1 uint64,
 * [0] = 0, [C] = P, non-decreasing).  Part p has a text -- document p of the usual packed bytes / doc_offsets[P + 1], possibly
 * empty --, part_ctrl[p] (uint32: a control id, or TK_JOIN_NONE) and part_flags[p] (uint32: TK_PART_LABEL_CTRL |
 * TK_PART_LABEL_TEXT; a NULL part_flags means all zero; other bits are ignored).
 *   1. E_p = the encoding of part p's text alone, without BOS / EOS: what tk_encode_batch_device returns for document p, so no
 *      token spans a part boundary.  T_p = [part_ctrl[p]] (only if it is not TK_JOIN_NONE) followed by E_p.  J_c = the
 *      concatenation of T_p over the parts of c, in order.
 *   2. ids (uint32, N = sum |T_p|) = J_0 + J_1 + ...; offsets (uint64, C + 1) = the exclusive prefix sum of |J_c|.  n_ctrl = the
 *      number of parts with a control id: N = n_text_ids + n_ctrl.
 *   3. labels (int32, N, only with TK_JOIN_LABELS, else NULL): the element of a control id is that id if part_flags &
 *      TK_PART_LABEL_CTRL, else ignore_index; the element of a text id is that id if part_flags & TK_PART_LABEL_TEXT, else
 *      ignore_index (callers pass -100).  n_labelled = the number of elements that are not ignored by these rules; it is filled
 *      whether or not labels is selected.
 *   4. part_index (uint32, N, only with TK_JOIN_PART_INDEX, else NULL) = p - conv_offsets[c] of the part the element came from.
 *   5. Valid and empty: C == 0 (conv_offsets = [0]; P must be 0), conversations without parts, parts with neither a control id
 *      nor text, P == 0.
 *   6. TK_ERR_INVALID_ARG, nothing written, an earlier join result stays readable: an unknown flag (opts or checks); a NULL
 *      required argument; C == 0 with P > 0; P == 0 with ids; and, with TK_CHECK_PARTS (a bit of the `checks` word beside
 *      TK_CHECK_OFFSETS / TK_CHECK_UTF8), conv_offsets that do not start at 0, decrease or do not end at P, or a control id that is
 *      neither TK_JOIN_NONE nor < num_special_tokens -- the message names the first bad conversation or part.  The host entry
 *      always makes these checks, on the host.  Without the check on a device entry a control id is copied as given, and
 *      malformed offsets are out-of-bounds indexing on the device, as in tk_dense_from_ids_device.  A failed allocation is
 *      TK_ERR_RUNTIME.
 *   7. out's buffers are owned by the context, valid until the next join call on it, and SEPARATE from the encode, spans, dense,
 *      packed and decode buffers: ids / offsets can be passed straight to tk_dense_from_ids_device, tk_seqpack_from_ids_device,
 *      tk_token_spans_device (without checks) or tk_decode_batch_device.
 * The join is a separate pass behind the unchanged encode pipeline (csrc/tk_join.hip): every element is written once, in 16-byte
 * stores but for the last N % 4 elements; an unselected output is not touched.  The buffers are sized for n_ids + P elements, so
 * nothing is read before the launches, and one wait at the end reads N, n_ctrl and n_labelled.  TK_CHECK_PARTS on a device entry
 * costs one small kernel and one more wait in front: the earlier result can only be given up once the arguments are accepted. */
#define TK_CHECK_PARTS 16
#define TK_JOIN_NONE 0xFFFFFFFFu
#define TK_PART_LABEL_CTRL 1
#define TK_PART_LABEL_TEXT 2
#define TK_JOIN_LABELS 1
#define TK_JOIN_PART_INDEX 2
typedef struct tk_join_opts { int32_t ignore_index; uint32_t flags; } tk_join_opts;
typedef struct tk_join { uint32_t* ids; uint64_t* offsets; int32_t* labels; uint32_t* part_index;
                         uint64_t n_convs, n_parts, n_ids, n_ctrl, n_labelled; } tk_join;
/* ids already on the device (encode's own outputs for add_bos = add_eos = 0, or the caller's; d_id_offsets: n_parts + 1 uint64,
 * [0] = 0, non-decreasing, [n_parts] = n_ids -- NOT checked) -> the joined stream.  d_part_ctrl: n_parts uint32; d_part_flags:
 * n_parts uint32 or NULL; d_conv_offsets: n_convs + 1 uint64.  checks: 0 | TK_CHECK_PARTS.  The work is enqueued on hip_stream
 * and the call returns after the stream has drained. */
int tk_join_from_ids_device(tk_ctx* ctx, const void* d_ids, const void* d_id_offsets, uint64_t n_parts, uint64_t n_ids,
                            const void* d_part_ctrl, const void* d_part_flags, const void* d_conv_offsets, uint64_t n_convs,
                            int checks, const tk_join_opts* opts, void* hip_stream, tk_join* out);
/* tk_encode_batch_device_ex(add_bos = 0, add_eos = 0) over the part texts + the join on the same stream.  checks may combine
 * TK_CHECK_OFFSETS / TK_CHECK_UTF8 (the text) with TK_CHECK_PARTS. */
int tk_encode_parts_device_join(tk_ctx* ctx, const void* d_bytes, const void* d_doc_offsets, uint64_t n_parts, uint64_t n_bytes,
                                const void* d_part_ctrl, const void* d_part_flags, const void* d_conv_offsets, uint64_t n_convs,
                                int checks, const tk_join_opts* opts, void* hip_stream, tk_join* out);
/* Host in / host out: tk_encode_batch + the join (batches of the one-launch small path included).  out's buffers are pinned host
 * memory, released with tk_free_join (an unselected output is NULL). */
int tk_encode_parts_join(tk_ctx* ctx, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_parts, const uint32_t* part_ctrl,
                         const uint32_t* part_flags, const uint64_t* conv_offsets, uint64_t n_convs, int validate_utf8,
                         const tk_join_opts* opts, tk_join* out);
void tk_free_join(tk_join* out);

/* ---- whole documents packed into rows without cutting them (next-fit), with labels (no reference equivalent: pad_id(),
 * src/tekkenizer.rs:304, is all the reference has) ----
 * Supervised fine-tuning packs conversations into rows of seq_len but never cuts one: labels, position_ids and the attention
 * segments must all describe one whole sample.  Input: the ragged ids R_d = ids[oo[d] : oo[d+1]] with n_d ids each, d < D;
 * N = oo[D]; optionally a second int32 stream lab with the SAME offsets; options seq_len = L (required, > 0), pad_id,
 * ignore_index, keep_tail and the flags below.
 *   1. e_d = min(n_d, L).  A document with n_d > L is truncated on the right to L elements of which the last keep_tail are its
 *      last ids: element k of the placed document is R_d[k] for k < L - keep_tail and R_d[n_d - (L - k)] for k >= L - keep_tail.
 *      Documents that fit are never changed.  n_truncated = the documents with n_d > L.  lab is truncated the same way.
 *   2. Next-fit in the caller's order: r = -1, fill = L; for d = 0 .. D-1: if e_d > 0 and fill + e_d > L then r += 1, fill = 0;
 *      doc_start[d] = r * L + fill; fill += e_d.  n_rows = r + 1.  An empty document opens no row and takes no space; its
 *      doc_start is where the next id would go (possibly (r + 1) * L; 0 before the first row).  row = doc_start / L and
 *      col = doc_start % L for every non-empty document; documents keep their order, doc_start is non-decreasing.
 *   3. input_ids[n_rows, L]: document d occupies the flattened positions doc_start[d] .. doc_start[d] + e_d, every other
 *      position holds pad_id.  n_pad = n_rows * L - sum(e_d).
 *   4. labels[n_rows, L] (TK_ROWFIT_LABELS, needs lab; always int32): lab in the same positions, ignore_index under pads.
 *   5. position_ids (TK_ROWFIT_POSITIONS): the distance to the document's start, 0 under pads.  segment_ids
 *      (TK_ROWFIT_SEGMENTS): 1, 2, 3, ... over the non-empty documents of a row, 0 under pads.
 *   6. cu_seqlens (TK_ROWFIT_CU_SEQLENS, int32): the sorted starts of every non-empty document and of every row's pad run
 *      (where the row has pads), followed by n_rows * L.  It tiles the whole flattened tensor: a variable-length attention call
 *      takes the tensor as it is, every pad run a segment of its own.  n_segments = its length - 1; max_seqlen = max diff, pad
 *      runs included (an attention kernel needs a bound over every segment).  n_rows == 0: [0], n_segments = max_seqlen = 0.
 *      n_segments and max_seqlen are filled whether or not the array is selected.
 *   7. doc_start (TK_ROWFIT_DOC_START): uint64 [D], as defined in 2.
 *   8. input_ids, position_ids and segment_ids are int32, or int64 with TK_ROWFIT_I64; labels and cu_seqlens are int32.  An
 *      unselected output is NULL.
 *   9. TK_ERR_INVALID_ARG, nothing written, an earlier rowfit result stays readable: L == 0; L >= 2^31; an unknown flag;
 *      keep_tail > L; TK_ROWFIT_LABELS without a labels pointer when N > 0; n_docs == 0 with n_ids > 0; n_rows * L > 2^36;
 *      TK_ROWFIT_CU_SEQLENS with n_rows * L >= 2^31.  The last two are known once n_rows is, behind the placement and before
 *      any output buffer is touched (offsets that do not end at n_ids are refused at the same point).  A failed allocation is
 *      TK_ERR_RUNTIME.  D == 0 or N == 0 is valid and gives n_rows == 0.
 * Next-fit trades padding for order and parallelism: best-fit-decreasing packs tighter, but it reorders the samples and is
 * sequential.  A caller who wants less padding puts the documents into length order first, on the device:
 * tk_regroup_from_ids_device below, whose ids / offsets this entry takes as they are; n_pad makes the cost visible.
 * The layout is a separate pass behind the unchanged encode pipeline (csrc/tk_rowfit.hip).  The placement is not sequential
 * either: with E the exclusive prefix sum of e, the row opened at document i ends in front of nxt(i), the largest j with
 * E[j] <= E[i] + L; pointer doubling over the chain 0, nxt(0), nxt(nxt(0)), ... marks the row openers and numbers the rows in
 * ceil(log2(n_rows)) + 1 rounds.  One host read (48 bytes: n_rows, n_truncated, sum e, the end of the offsets) sizes the tensors; every element is then written
 * once, pad included, in 16-byte stores where L is a multiple of 4, and one more wait ends the call. */
#define TK_ROWFIT_I64 1
#define TK_ROWFIT_POSITIONS 2
#define TK_ROWFIT_SEGMENTS 4
#define TK_ROWFIT_CU_SEQLENS 8
#define TK_ROWFIT_LABELS 16
#define TK_ROWFIT_DOC_START 32
typedef struct tk_rowfit_opts { uint32_t seq_len, pad_id, keep_tail, flags; int32_t ignore_index; } tk_rowfit_opts;
typedef struct tk_rowfit { void* input_ids; int32_t* labels; void *position_ids, *segment_ids; int32_t* cu_seqlens; uint64_t* doc_start;
                           uint64_t n_rows, row_len, n_segments, max_seqlen, n_truncated, n_pad; } tk_rowfit;
/* ids already on the device (encode's own outputs, a join's ids / offsets, or the caller's; d_id_offsets: n_docs + 1 uint64,
 * [0] = 0, non-decreasing, [n_docs] = n_ids -- only the last is checked) -> whole-document rows.  d_labels: NULL or int32[n_ids]
 * (a join's labels).  out's buffers are device buffers owned by the context, valid until the next rowfit call on it, and
 * SEPARATE from the encode, spans, dense, packed, join, window and decode outputs.  The work is enqueued on hip_stream and the
 * call returns after the stream has drained. */
int tk_rowfit_from_ids_device(tk_ctx* ctx, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                              const void* d_labels, const tk_rowfit_opts* opts, void* hip_stream, tk_rowfit* out);
/* tk_encode_batch_device_ex + the rowfit pass on the same stream (text has no labels stream: TK_ROWFIT_LABELS is refused before
 * anything is encoded, here and in tk_encode_batch_rowfit); the ragged outputs (*d_ids / *d_out_offsets / *n_ids as tk_encode_batch_device) are returned as well. */
int tk_encode_batch_device_rowfit(tk_ctx* ctx, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                  int add_bos, int add_eos, int checks, const tk_rowfit_opts* opts, void* hip_stream,
                                  void** d_ids, void** d_out_offsets, uint64_t* n_ids, tk_rowfit* out);
/* tk_encode_parts_device_join + the rowfit pass over the conversations' ids, labels (with TK_JOIN_LABELS) and offsets on the same
 * stream: a conversation is a document of the placement.  *joined is the join's result, as tk_encode_parts_device_join gives it.
 * TK_ROWFIT_LABELS without TK_JOIN_LABELS is refused before anything is encoded. */
int tk_encode_parts_device_rowfit(tk_ctx* ctx, const void* d_bytes, const void* d_doc_offsets, uint64_t n_parts, uint64_t n_bytes,
                                  const void* d_part_ctrl, const void* d_part_flags, const void* d_conv_offsets, uint64_t n_convs,
                                  int checks, const tk_join_opts* join_opts, const tk_rowfit_opts* opts, void* hip_stream,
                                  tk_join* joined, tk_rowfit* out);
/* Host in / host out: tk_encode_batch + the rowfit pass (batches of the one-launch small path included).  out's buffers are
 * pinned host memory, released with tk_free_rowfit (an unselected output is NULL). */
int tk_encode_batch_rowfit(tk_ctx* ctx, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos, int add_eos,
                           int validate_utf8, const tk_rowfit_opts* opts, tk_rowfit* out);
void tk_free_rowfit(tk_rowfit* out);
/* Not in the list of entries the pass was asked to have: the measurement needs the placement and the fill kernel apart
 * (tools/rowfit_time.py), and only the library sees the boundary between them.  It costs six event records a call.
 * GPU time of the stages of the context's last rowfit pass, from events on its stream: the placement (lengths, scans, nxt,
 * doubling rounds, doc_start; the host read between them is not counted), the fill kernel, the cu_seqlens kernel.  All 0 when
 * the pass launched nothing (n_ids == 0) or was refused.  A NULL pointer is skipped. */
void tk_last_rowfit_ms(const tk_ctx* ctx, float* placement_ms, float* fill_ms, float* cu_ms);

/* ---- special-token strings parsed out of text on the device (tiktoken's allowed_special / disallowed_special; no reference
 * equivalent: the reference calls CoreBPE::encode with an empty allowed set, src/tekkenizer.rs:384-386, and so does every encode
 * entry above) ----
 * A chat template renders a conversation to one string ("<s>[INST] ... [/INST] ...</s>"), a pre-training shard carries "</s>"
 * between documents: this pass finds the occurrences of special-token strings in the packed text of D documents, takes them out and
 * returns what tk_encode_parts_device_join needs.  Inputs: bytes / doc_offsets[D + 1] as encode takes them; the context's special
 * strings S_0 .. S_{n-1} (tk_ctx_set_special_tokens; n = num_special_tokens): S_i is the string of id i, the one decode prints
 * for id i under TK_POLICY_KEEP; modes, uint8[n] or NULL, with modes[i] one of TK_SPECIAL_TEXT (never matched: the string stays text,
 * which is what every other entry does), TK_SPECIAL_PARSE, TK_SPECIAL_RAISE.  NULL means PARSE for every string.
 *   1. Match set.  A = { i : modes[i] != TEXT }.  TK_ERR_INVALID_ARG before any work: a string of A that is empty or longer than
 *      255 bytes; no strings set on the context; n_modes != num_special_tokens (with modes != NULL); an unknown mode value.  Where
 *      two strings of A are equal bytes, the lower id stands for both.
 *   2. Matches, per document, alone.  p = 0; while p < len: among the i in A with doc[p : p + |S_i|] == S_i (wholly inside the
 *      document) the longest wins: emit (p, |S_i|, i) and continue at p + |S_i|; none: continue at p + 1.  Leftmost-longest,
 *      non-overlapping, on bytes; a match never crosses a document boundary.  It is tiktoken's and HF's result whenever no string
 *      of A is a prefix of another, which holds for every Tekken vocabulary.  On valid UTF-8 a match begins and ends on a
 *      character boundary.
 *   3. Raise.  An emitted match whose id has mode RAISE fails the call as a whole with TK_ERR_SPECIAL_POLICY; nothing of an
 *      earlier result is touched.  *bad (optional) receives the first such document; the message names the document, the
 *      document-relative byte position and the id.
 *   4. Parts.  Document d with matches (s_1, l_1, i_1) .. (s_m, l_m, i_m): part 0 has part_ctrl = the context's BOS id with
 *      TK_SPECIALS_BOS, else TK_JOIN_NONE, and the text doc[0 : s_1) (the whole document if m == 0); part j (1 <= j <= m) has
 *      part_ctrl = i_j and the text doc[s_j + l_j : s_{j+1}), s_{m+1} = len; with TK_SPECIALS_EOS one more part, the EOS id and
 *      empty text.  conv_offsets (uint64, D + 1) = the exclusive prefix sum of the parts per document; n_parts = P =
 *      conv_offsets[D].  part_offsets (uint64, P + 1) and bytes: the parts' texts concatenated in order, which is the input with
 *      exactly the matched strings removed.  n_matches = sum m, n_removed = sum l, n_bytes = the input's n_bytes - n_removed.
 *      part_src (uint64, P, only with TK_SPECIALS_PART_SRC, else NULL): the offset in the INPUT buffer at which part p's text
 *      begins, so a byte span inside part p maps back to the caller's document by one addition.
 *   5. The encoding it defines.  J_d = the join of document d's parts (steps 1-2 of the join above) = [bos] + enc(seg_0) + [i_1] +
 *      enc(seg_1) + .. + [i_m] + enc(seg_m) + [eos].  With every mode TEXT, or on text that holds no string of A, J_d is bit for
 *      bit what tk_encode_batch returns for the same add_bos / add_eos.
 *   6. Valid and empty: D == 0; empty documents (one part, empty text); a document that is one special string and nothing else;
 *      n_bytes == 0; A empty (no device work beyond the part tables).  When n_removed == 0, out->bytes may be the caller's own
 *      d_bytes (no copy): it is then valid as long as the caller keeps that buffer.
 *   7. TK_ERR_INVALID_ARG beside step 1: an unknown flag (opts or checks), a NULL required argument, D >= 2^32 - 16, 2^32 - 16
 *      candidates or more.  checks: TK_CHECK_OFFSETS / TK_CHECK_UTF8 as in tk_encode_batch_device_ex, on the INPUT, before the
 *      split.  Without TK_CHECK_OFFSETS malformed offsets give parts that mean nothing but are never out-of-bounds indexing in
 *      this pass.  A failed allocation is TK_ERR_RUNTIME.
 *   8. out's buffers are device buffers owned by the context, valid until the next specials call on it, and SEPARATE from every
 *      other pass's; an earlier result stays readable when a call is refused.
 * A separate pass in front of the unchanged encode pipeline (csrc/tk_specials.hip).  Candidates: every text byte is
 * read once; a byte outside the 256-bit first-byte mask of A costs one test, any other a walk of a byte trie over the strings that
 * is bounded by the longest string, not by their number.  The matches are the candidates reachable from the first one under
 * nxt(c) = the first candidate at or behind c's end -- one chain over the whole batch, marked by the pointer doubling that the
 * rowfit and regroup passes have.  The part tables need one search per document and no scan; the text is compacted in 16-byte
 * stores.  Two host reads (the number of candidates; n_matches, n_removed and the RAISE word) and one more wait; without a
 * candidate the pass ends behind the first read with the part tables alone. */
#define TK_SPECIAL_TEXT 0
#define TK_SPECIAL_PARSE 1
#define TK_SPECIAL_RAISE 2
#define TK_SPECIALS_BOS 1
#define TK_SPECIALS_EOS 2
#define TK_SPECIALS_PART_SRC 4
typedef struct tk_specials_opts { const uint8_t* modes; uint32_t n_modes; uint32_t flags; } tk_specials_opts;
typedef struct tk_specials { uint8_t* bytes; uint64_t* part_offsets; uint32_t* part_ctrl; uint64_t* conv_offsets; uint64_t* part_src;
                             uint64_t n_docs, n_parts, n_bytes, n_matches, n_removed; } tk_specials;
/* Text on the device -> the parts.  opts->modes is a HOST pointer, copied per call.  The work is enqueued on hip_stream and the
 * call returns after the stream has drained. */
int tk_specials_split_device(tk_ctx* ctx, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes, int checks,
                             const tk_specials_opts* opts, void* hip_stream, tk_specials* out, uint64_t* bad);
/* The split + tk_encode_parts_device_join over its parts on the same stream: *out is J (step 5), *parts the split's result.
 * Everything that can be refused (opts, jopts, the checks, RAISE) is refused before anything is encoded.  jopts' labels and part_index
 * work as in the join; part_flags is NULL: a caller who wants labels per part calls the two halves. */
int tk_encode_batch_device_parsed(tk_ctx* ctx, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                  int checks, const tk_specials_opts* opts, const tk_join_opts* jopts, void* hip_stream,
                                  tk_specials* parts, tk_join* out, uint64_t* bad);
/* Host in / host out.  out's (and, where parts is not NULL, parts') buffers are pinned host memory, released with tk_free_join /
 * tk_free_specials (an unselected output is NULL). */
int tk_encode_batch_parsed(tk_ctx* ctx, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int validate_utf8,
                           const tk_specials_opts* opts, const tk_join_opts* jopts, tk_specials* parts, tk_join* out, uint64_t* bad);
void tk_free_specials(tk_specials* out);
/* As tk_last_regroup_ms, for tools/specials_time.py: GPU time of the stages of the context's last specials pass, from events on
 * its stream: ms[0] the candidates (both launches and the scan; the host read between them is not counted), ms[1] the chain
 * (nxt, the doubling rounds, the marks and their scan), ms[2] the part tables, ms[3] the text compaction.  All 0 where the pass
 * was refused; a stage that launched nothing is 0 or the cost of two event records. */
void tk_last_specials_ms(const tk_ctx* ctx, float ms[4]);
/* The text bytes of a tile of the candidate kernel (tests place matches across its boundaries). */
uint32_t tk_specials_tile(void);

/* ---- fill-in-the-middle rows: documents cut in two places and reordered on the device (no reference equivalent; the
 * [PREFIX] / [SUFFIX] / [MIDDLE] control tokens of a Tekken vocabulary are what it is for) ----
 * A document is cut at two random places into prefix P, middle M and suffix S and becomes "[SUFFIX] S [PREFIX] P M" (SPM without
 * a middle id: Mistral / Codestral) or "[PREFIX] P [SUFFIX] S [MIDDLE] M" (PSM).  This pass makes the cuts, the part tables that
 * tk_encode_parts_device_join / tk_join_from_ids_device take, and the text (or the ids) copied once in the new order; no token
 * spans a part boundary, which is the seam as inference sees it.  ONE definition over units: a unit is a byte for the text
 * entries and an id (uint32) for the ids entries.  Inputs: units, offsets[D + 1] (uint64, as encode takes them), tk_fim_opts, and
 * optionally cuts, uint64[D][2], document-relative; TK_FIM_NO_CUT in slot 0 means "leave this document alone".
 *   1. Body.  Text entries: head = tail = 0 (refused otherwise); the body is the whole document, n = len.  Ids entries: the first
 *      `head` and last `tail` ids (a stored BOS / EOS) stay in place, the body is what lies between, n = len - head - tail.  A
 *      document with len < head + tail is never transformed: its body is the whole document, its head and tail are empty.
 *   2. Draws, all arithmetic mod 2^32, h exactly as at TK_REGROUP_ORDER_SHUFFLE below:  s_k = h(seed, 0x46494D00 + k),
 *      u_k = h(s_k, d), k = 0..3 (epoch e and e + 1 share no draw).  Without cuts document d is a candidate iff u_0 < rate_q32; a
 *      candidate is transformed iff len >= head + tail and n >= max(min_units, 1) and n < 2^32 - 1; its cuts are
 *      c_i = (uint64(u_{2+i}) * (n + 1)) >> 32, uniform over 0..n.  With cuts every document whose slot 0 is not TK_FIM_NO_CUT is a
 *      candidate, transformed iff len >= head + tail and n < 2^32 - 1; its cuts are the two given values, each clamped to n;
 *      rate_q32 and min_units play no part.  n_skipped = the candidates that are not transformed.  Order: SPM iff
 *      u_1 < spm_q32, else PSM.
 *   3. Snap (text entries with TK_FIM_SNAP only).  For each cut c, at most 3 times: while 0 < c < n and (byte[c] & 0xC0) == 0x80:
 *      c -= 1.  Defined on bytes, so total on malformed UTF-8; on valid UTF-8 every cut lands on a character start.  Then
 *      lo = min, hi = max; P = body[0 : lo), M = body[lo : hi), S = body[hi : n).
 *   4. Parts.  Every document gives exactly 5 parts: conv_offsets[d] = 5 d, n_parts = 5 D.
 *          part      untransformed                 PSM                 SPM
 *          0 head    text entries: no text, ctrl = the BOS id with TK_FIM_BOS, else TK_JOIN_NONE; ids entries: the head ids, no ctrl
 *          1         (NONE, body)                  (prefix_id, P)      (suffix_id, S)
 *          2         (NONE, empty)                 (suffix_id, S)      (prefix_id, P)
 *          3         (NONE, empty)                 (middle_id, M)      (middle_id, M)
 *          4 tail    the mirror of part 0: the EOS id with TK_FIM_EOS, or the tail ids
 *      Each of the three ids may be TK_JOIN_NONE (Mistral: SPM with middle_id = NONE).  units holds the parts' units in part
 *      order: document d keeps its range [offsets[d], offsets[d+1]), permuted; n_units is the input's.  part_offsets
 *      (uint64, 5 D + 1) are the parts' starts in units; part_src (uint64, 5 D, only with TK_FIM_PART_SRC, else NULL) is where
 *      each part's first unit lies in the INPUT buffer (an empty part: where its text would begin; the empty parts 2 and 3 of an
 *      untransformed document: the body's end).
 *   5. Labels.  part_flags (uint32, 5 D) = TK_PART_LABEL_CTRL | TK_PART_LABEL_TEXT on every part; with TK_FIM_LABEL_MIDDLE a
 *      transformed document's parts 0..2 get 0, part 3 TK_PART_LABEL_TEXT alone, part 4 both.  Untransformed documents stay fully
 *      labelled.
 *   6. Also out: cuts (uint64 [D][2]) = (lo, hi) behind the snap, or TK_FIM_NO_CUT twice; mode (uint8 [D]): 0 none, 1 PSM, 2 SPM;
 *      n_transformed, n_spm, n_skipped.
 *   7. The encoding it defines.  J_d = the join of the document's five parts.  For an untransformed document it is bit for bit
 *      what tk_encode_batch returns with the same BOS / EOS (text), or the input ids (ids).  With rate_q32 == 0 and no cuts
 *      out->units may be the caller's own buffer, not copied.
 *   8. Valid and empty: D == 0, empty documents, n_units == 0.  TK_ERR_INVALID_ARG, nothing written, an earlier result stays
 *      readable: an unknown flag (opts or checks); TK_FIM_BOS / TK_FIM_EOS on an ids entry; rate_q32 or spm_q32 above 2^32; head or
 *      tail non-zero on a text entry; an id that is neither TK_JOIN_NONE nor < num_special_tokens; D >= 2^32 - 16; a NULL required
 *      argument.  checks (text entries): TK_CHECK_OFFSETS / TK_CHECK_UTF8 as in tk_encode_batch_device_ex, on the INPUT.  Without
 *      TK_CHECK_OFFSETS malformed offsets give parts that mean nothing, but nothing outside [units, units + n_units) is read.
 *      out's buffers are device buffers owned by the context, SEPARATE from every other pass's and valid until the next FIM call.
 * A separate pass in front of the unchanged encode pipeline (csrc/tk_fim.hip): one thread a document makes the
 * draws, the snap (at most 3 byte reads a cut) and the five part records; the permute kernel has the shape of the join, regroup
 * and compaction kernels -- a block takes tiles of output units, two wave searches over offsets, the tile's documents' cuts in
 * LDS, a thread resolves 16 bytes: one 16-byte load at any byte and one 16-byte store where they lie in one of the document's
 * shifted ranges, unit by unit over the seams.  No scan, no host read before the last wait, which fetches the three counters. */
#define TK_FIM_NO_CUT (~0ull)
#define TK_FIM_SNAP 1
#define TK_FIM_BOS 2
#define TK_FIM_EOS 4
#define TK_FIM_PART_SRC 8
#define TK_FIM_LABEL_MIDDLE 16
typedef struct tk_fim_opts { uint64_t rate_q32, spm_q32; uint32_t seed, prefix_id, suffix_id, middle_id, head, tail, min_units, flags; } tk_fim_opts;
typedef struct tk_fim { void* units; uint64_t* part_offsets; uint32_t* part_ctrl; uint32_t* part_flags; uint64_t* conv_offsets;
                        uint64_t* part_src; uint64_t* cuts; uint8_t* mode;
                        uint64_t n_docs, n_parts, n_units, n_transformed, n_spm, n_skipped; } tk_fim;
/* Text on the device -> the parts (units: uint8).  d_cuts: uint64[n_docs][2] on the device, or NULL.  The work is enqueued on
 * hip_stream and the call returns after the stream has drained. */
int tk_fim_split_device(tk_ctx* ctx, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes, const void* d_cuts,
                        int checks, const tk_fim_opts* opts, void* hip_stream, tk_fim* out);
/* Ids on the device (encode's own output, or stored ids) -> the parts (units: uint32); part_offsets are then the d_id_offsets of
 * tk_join_from_ids_device. */
int tk_fim_split_ids_device(tk_ctx* ctx, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids, const void* d_cuts,
                            const tk_fim_opts* opts, void* hip_stream, tk_fim* out);
/* The text split + tk_encode_parts_device_join over its parts (part_flags included) on the same stream: *out is J (step 7),
 * *parts (optional) the split's result.  Everything that can be refused is refused before anything is encoded. */
int tk_encode_batch_device_fim(tk_ctx* ctx, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                               const void* d_cuts, int checks, const tk_fim_opts* opts, const tk_join_opts* jopts, void* hip_stream,
                               tk_fim* parts, tk_join* out);
/* The ids split + tk_join_from_ids_device: a new draw every epoch over documents tokenised once (cuts at token boundaries). */
int tk_fim_from_ids_device(tk_ctx* ctx, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids, const void* d_cuts,
                           const tk_fim_opts* opts, const tk_join_opts* jopts, void* hip_stream, tk_fim* parts, tk_join* out);
/* Host in / host out (cuts: a host array or NULL).  out's (and, where parts is not NULL, parts') buffers are pinned host memory,
 * released with tk_free_join / tk_free_fim (an unselected output is NULL). */
int tk_encode_batch_fim(tk_ctx* ctx, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, const uint64_t* cuts,
                        int validate_utf8, const tk_fim_opts* opts, const tk_join_opts* jopts, tk_fim* parts, tk_join* out);
void tk_free_fim(tk_fim* out);
/* GPU time of the context's last FIM pass from events on its stream: ms[0] the cut kernel, ms[1] the permute kernel (0 where
 * nothing was copied).  Both 0 where the pass was refused. */
void tk_last_fim_ms(const tk_ctx* ctx, float ms[2]);
/* The output units of a tile of the permute kernel for units of unit_bytes (1 or 4; anything else: 0): tests place seams on its
 * borders. */
uint32_t tk_fim_tile(int unit_bytes);

/* ---- masked-LM and span-corruption rows: a noise pass over encoded ids (no reference equivalent; HF's
 * DataCollatorForLanguageModeling(mlm=True) / DataCollatorForWholeWordMask, SpanBERT's spans, MNTP; T5 / UL2 span corruption) ----
 * One hash-drawn (or caller-given) choice of tokens, words or spans per document, and two things made of it: the ids with the
 * chosen ones masked and the labels (replace mode), or the documents with every chosen run replaced by one sentinel and the
 * targets that spell the runs out (spans mode).  A new draw every epoch over documents tokenised once: the seed is the epoch.
 * Inputs: ids (uint32 [N]), id_offsets (uint64 [D + 1]), optionally word_ids (uint32 [N], exactly as tk_words_from_ids_device
 * writes them), optionally sel (uint8 [N]), tk_noise_opts.  V = the context's vocabulary size (ranks + special tokens),
 * S0 = num_special_tokens.
 *   1. Eligibility and unit.  Id i sits in document d at document-relative position p.  It is eligible iff ids[i] >= S0 and, under
 *      TK_NOISE_UNIT_WORD, word_ids[i] != TK_WORD_NONE.  Its unit index x_i is p under TK_NOISE_UNIT_TOKEN and word_ids[i] under
 *      TK_NOISE_UNIT_WORD (which needs word_ids, unless sel is given).
 *   2. Draws, all arithmetic mod 2^32, h exactly as at TK_REGROUP_ORDER_SHUFFLE below:  s_k = h(seed, 0x4E4F4900 + k), k = 0..3;
 *      t_k = h(s_k, d).  Per unit index x of document d:
 *          start(x)   iff h(t_0, x) < start_q32
 *          len(x)     = span_min + ((uint64(h(t_1, x)) * (span_max - span_min + 1)) >> 32)
 *          covered(x) iff some q with x - span_max < q <= x, q >= 0, has start(q) and q + len(q) > x
 *      The draws are over indices and do not look at eligibility: a special id's position can start a span.
 *      selected(i) = eligible(i) and covered(x_i).  With sel: selected(i) = eligible(i) and sel[i] != 0; start_q32 and the span
 *      lengths then play no part.  1 <= span_min <= span_max <= TK_NOISE_SPAN_LIMIT; start_q32 <= 2^32.
 *   3. Replace mode (tk_noise_replace_device).  The offsets are the input's.  r = h(t_2, p), v = h(t_3, p), and
 *          input_ids[i] = ids[i]                                   if not selected
 *                       = mask_id                                  if r < mask_q32
 *                       = S0 + ((uint64(v) * (V - S0)) >> 32)      if r < mask_q32 + random_q32   (64-bit; the sum <= 2^32)
 *                       = ids[i]                                   otherwise
 *      labels (int32 [N]) = ids[i] where selected, else ignore_index; selected (uint8 [N], 0 / 1) only with TK_NOISE_SELECTED, else
 *      NULL.  mask_id is any id < V (Tekken has no [MASK]: a <SPECIAL_n> control id or an ordinary token).  n_selected, n_masked,
 *      n_random count the three.  n_sentinels, sentinel_first, final_id and the other flags play no part.
 *   4. Spans mode (tk_noise_spans_device).  A run is a maximal sequence of consecutive selected ids inside one document: runs
 *      never join across a document boundary, and an ineligible id inside a covered stretch splits a run.  Run k, numbered from
 *      0 in its document, is kept iff k < n_sentinels; the ids of a dropped run count as not selected (n_runs_dropped counts the
 *      runs).  The sentinel of run k is sentinel_first + k, with TK_NOISE_DESC sentinel_first - k; every sentinel the options can
 *      produce must be < S0.  Per document: inputs_d = the document's ids in order with every kept run replaced by its sentinel;
 *      targets_d = for every kept run in order its sentinel followed by its ids, then final_id unless that is TK_JOIN_NONE.
 *      TK_NOISE_SPLIT: inputs / input_offsets (uint64 [D + 1]) and targets / target_offsets, two ragged batches that feed the
 *      dense pass as they are.  TK_NOISE_JOINED: joined / joined_offsets / joined_labels with joined_d = inputs_d ++ targets_d
 *      and joined_labels (int32) the id on the targets' elements, ignore_index on the inputs' (the decoder-only form).  At least
 *      one of the two; an unselected output is NULL.  n_selected (behind the drop), n_runs (kept), n_runs_dropped, n_inputs,
 *      n_targets.  A document without a kept run: inputs_d is the document, targets_d is empty or final_id alone.  mask_id, the
 *      two rates of step 3 and TK_NOISE_SELECTED play no part.
 *   5. Valid and empty: D == 0, empty documents, N == 0, start_q32 == 0, n_sentinels == 0 (everything dropped).
 *      TK_ERR_INVALID_ARG, nothing written, an earlier result stays readable: an unknown flag or unit; the span limits violated; a
 *      rate above 2^32, or mask_q32 + random_q32 above it; mask_id >= V; a sentinel that the options can produce, or a final_id
 *      other than TK_JOIN_NONE, that is not < S0; neither TK_NOISE_SPLIT nor TK_NOISE_JOINED (spans mode); TK_NOISE_UNIT_WORD
 *      without word_ids and without sel; D >= 2^32 - 16; a document of 2^32 - 1 ids or more (spans mode: of 2^32 - 2 -
 *      n_sentinels or more, so that the lengths of inputs_d and targets_d stay in 32 bits); a NULL required argument.  Without
 *      well-formed id_offsets the outputs mean nothing, but nothing outside [ids, ids + N) (and the same range of word_ids and sel)
 *      is read and nothing outside the outputs written.  out's buffers are device buffers owned by the context, SEPARATE from
 *      every other pass's, and valid until the next noise call (replace and spans share them).
 * A separate pass behind the unchanged encode pipeline (csrc/tk_noise.hip).  Replace mode is one kernel: tiles of
 * ids, every thread the hashes of its own 4 positions, covered from a prefix maximum over the tile with a halo of span_max - 1
 * positions recomputed from their hashes (word unit: from the at most span_max candidate starts of the id's word); 16-byte loads
 * and stores, no scan launch, no host read before the last wait.  Spans mode: the selection, per-tile and per-document counts of
 * selected ids and run starts, two scans over tiles and two over documents, one host read that sizes the outputs, and a fill
 * kernel in which every id computes where it goes. */
#define TK_NOISE_UNIT_TOKEN 0
#define TK_NOISE_UNIT_WORD 1
#define TK_NOISE_SELECTED 1
#define TK_NOISE_DESC 2
#define TK_NOISE_SPLIT 4
#define TK_NOISE_JOINED 8
#define TK_NOISE_SPAN_LIMIT 64
typedef struct tk_noise_opts { uint64_t start_q32, mask_q32, random_q32; uint32_t seed, unit, span_min, span_max, mask_id, n_sentinels,
                               sentinel_first, final_id, flags; int32_t ignore_index; } tk_noise_opts;
typedef struct tk_noise_replace { uint32_t* input_ids; int32_t* labels; uint8_t* selected;
                                  uint64_t n_docs, n_ids, n_selected, n_masked, n_random; } tk_noise_replace;
typedef struct tk_noise_spans { uint32_t* inputs; uint64_t* input_offsets; uint32_t* targets; uint64_t* target_offsets; uint32_t* joined;
                                uint64_t* joined_offsets; int32_t* joined_labels;
                                uint64_t n_docs, n_selected, n_runs, n_runs_dropped, n_inputs, n_targets; } tk_noise_spans;
/* ids already on the device (encode's own outputs, or stored ids).  d_word_ids: NULL or uint32 [n_ids]; d_sel: NULL or uint8
 * [n_ids].  The work is enqueued on hip_stream and the call returns after the stream has drained. */
int tk_noise_replace_device(tk_ctx* ctx, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids, const void* d_word_ids,
                            const void* d_sel, const tk_noise_opts* opts, void* hip_stream, tk_noise_replace* out);
int tk_noise_spans_device(tk_ctx* ctx, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids, const void* d_word_ids,
                          const void* d_sel, const tk_noise_opts* opts, void* hip_stream, tk_noise_spans* out);
/* tk_encode_batch_device_ex, with TK_NOISE_UNIT_WORD the words pass, and the noise pass on the same stream.  Everything that can
 * be refused is refused before anything is encoded.  *d_ids / *d_out_offsets / *n_ids as tk_encode_batch_device: with
 * start_q32 == 0 (replace mode) out->input_ids holds the same ids bit for bit. */
int tk_encode_batch_device_noise_replace(tk_ctx* ctx, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                         int add_bos, int add_eos, int checks, const tk_noise_opts* opts, void* hip_stream, void** d_ids,
                                         void** d_out_offsets, uint64_t* n_ids, tk_noise_replace* out);
int tk_encode_batch_device_noise_spans(tk_ctx* ctx, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                       int add_bos, int add_eos, int checks, const tk_noise_opts* opts, void* hip_stream, void** d_ids,
                                       void** d_out_offsets, uint64_t* n_ids, tk_noise_spans* out);
/* Host in / host out: tk_encode_batch + the passes above.  ids_out as tk_encode_batch (tk_free_result): the ids in front of the
 * noise and their offsets, which are replace mode's.  out's buffers are pinned host memory, released with tk_free_noise_replace /
 * tk_free_noise_spans (an unselected output is NULL). */
int tk_encode_batch_noise_replace(tk_ctx* ctx, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos, int add_eos,
                                  int validate_utf8, const tk_noise_opts* opts, tk_result* ids_out, tk_noise_replace* out);
int tk_encode_batch_noise_spans(tk_ctx* ctx, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos, int add_eos,
                                int validate_utf8, const tk_noise_opts* opts, tk_result* ids_out, tk_noise_spans* out);
void tk_free_noise_replace(tk_noise_replace* out);
void tk_free_noise_spans(tk_noise_spans* out);
/* GPU time of the stages of the context's last noise pass, from events on its stream: ms[0] the selection (replace mode: the whole
 * pass), ms[1] the counts and scans of spans mode (the host read behind them is not counted), ms[2] its fill kernel.  All 0 where
 * the pass was refused. */
void tk_last_noise_ms(const tk_ctx* ctx, float ms[3]);
/* The input ids of a tile of the noise kernels: tests place runs, spans and document boundaries on its borders. */
uint32_t tk_noise_tile(void);

/* ---- encoded documents selected, reordered and cut into batches on the device (no reference equivalent) ----
 * What a data pipeline does between "encode" and "batch": drop documents, put the rest into another order (shuffled, by length, by
 * length within shuffled groups), cut that order into batches under a padded-token budget.  Ragged in, ragged out: the result's
 * ids / offsets feed tk_dense_from_ids_device, tk_rowfit_from_ids_device, tk_seqpack_from_ids_device and the spans entries as
 * they are.  Input: the ragged ids R_d = ids[oo[d] : oo[d+1]] with n_d ids each, d < D; N = oo[D]; optionally lab, int32[N], with
 * the SAME offsets (a join's labels); optionally keep, uint8[D]; the options and flags below.
 *   1. Selection.  Document d is kept iff (keep is NULL or keep[d] != 0) and n_d >= min_length and (max_length == 0 or
 *      n_d <= max_length).  A dropped document is counted once, under the first test it fails: n_masked, then n_short, then
 *      n_long.  K = n_docs is the number kept; c_0 < ... < c_{K-1} are the kept indices.
 *   2. Order.  perm[k] is the source document of output document k.
 *      TK_REGROUP_ORDER_KEEP: perm = c.
 *      TK_REGROUP_ORDER_LENGTH: ascending n_d, stable (equal lengths stay in ascending d); with TK_REGROUP_DESC descending n_d,
 *      still stable in d.
 *      TK_REGROUP_ORDER_SHUFFLE: ascending h(seed, d), all arithmetic mod 2^32:
 *          x = d * 0x9E3779B1 + seed;  x ^= x >> 16;  x *= 0x85EBCA6B;  x ^= x >> 13;  x *= 0xC2B2AE35;  x ^= x >> 16
 *      h is a bijection of the 32-bit d: no ties, and the order of two documents does not depend on what else was dropped.
 *      TK_REGROUP_ORDER_GROUPED (needs window = w > 0): the SHUFFLE order cut into consecutive groups of w (the last may be
 *      shorter), each group sorted by length (ascending; descending with TK_REGROUP_DESC), stable with respect to the shuffled
 *      order.  TK_REGROUP_DESC means nothing to KEEP and SHUFFLE.
 *   3. Ragged outputs.  offsets (uint64, K + 1) is the exclusive prefix sum of n_perm[k]; ids[offsets[k] : offsets[k+1]] =
 *      R_perm[k]; n_ids = offsets[K].  labels (TK_REGROUP_LABELS, needs lab): lab moved the same way.  perm (TK_REGROUP_PERM):
 *      uint32 [K].
 *   4. Batches (TK_REGROUP_BATCHES, needs max_tokens = T > 0; max_docs == 0: no limit).  With m_k = n_perm[k]:
 *          bo = [0]; start = 0; mx = 0
 *          for k in 0 .. K-1:
 *              m = max(mx, m_k); cnt = k - start + 1
 *              if cnt > 1 and (cnt * m > T or (max_docs and cnt > max_docs)): bo.append(k); start = k; m = m_k
 *              mx = m
 *          if K > 0: bo.append(K)
 *      batch_offsets = bo (TK_REGROUP_BATCH_OFFSETS, uint64 [n_batches + 1]; [0] and n_batches = 0 when K = 0).  batch_rowlen[b]
 *      (TK_REGROUP_BATCH_ROWLEN, uint32 [n_batches]) is the longest document of batch b: the L of a dense call over the batch.
 *      n_oversize = the batches with cnt * rowlen > T (such a batch is one document on its own; max_length <= T rules it out).
 *      n_batch_pad = sum_b cnt_b * rowlen_b - n_ids.  The three counts are filled whether or not the arrays are selected, as
 *      long as TK_REGROUP_BATCHES is set; without it the two array flags select nothing and the counts are 0.
 *   5. TK_ERR_INVALID_ARG, nothing written, an earlier regroup result stays readable: an unknown order or flag; D >= 2^32;
 *      TK_REGROUP_ORDER_GROUPED with window == 0; TK_REGROUP_BATCHES with max_tokens == 0; TK_REGROUP_LABELS without lab when
 *      N > 0; min_length > max_length > 0; n_docs == 0 with n_ids > 0; and, known behind the selection and before any output
 *      buffer is touched: offsets that do not end at n_ids, a document of 2^32 ids or more (which is also what offsets that
 *      decrease look like).  A failed allocation is TK_ERR_RUNTIME.  D = 0, N = 0 and "everything dropped" are valid: K = 0.
 * A separate pass behind the unchanged encode pipeline (csrc/tk_regroup.hip): the selection and its scan, one host
 * read (K, n_ids, the drop counts, the longest kept document), a stable least-significant-digit radix sort of (key, document)
 * pairs, 8 bits a pass, which skips the digits above the largest key, the gather of every id in 16-byte stores, and the batch
 * boundaries by one search per document and the pointer doubling that the rowfit pass has.  One more wait ends the call. */
#define TK_REGROUP_ORDER_KEEP 0
#define TK_REGROUP_ORDER_LENGTH 1
#define TK_REGROUP_ORDER_SHUFFLE 2
#define TK_REGROUP_ORDER_GROUPED 3
#define TK_REGROUP_DESC 1
#define TK_REGROUP_LABELS 2
#define TK_REGROUP_PERM 4
#define TK_REGROUP_BATCHES 8
#define TK_REGROUP_BATCH_OFFSETS 16
#define TK_REGROUP_BATCH_ROWLEN 32
typedef struct tk_regroup_opts { uint64_t max_tokens; uint32_t min_length, max_length, order, seed, window, max_docs, flags; } tk_regroup_opts;
typedef struct tk_regroup { uint32_t* ids; uint64_t* offsets; int32_t* labels; uint32_t* perm; uint64_t* batch_offsets; uint32_t* batch_rowlen;
                            uint64_t n_docs, n_ids, n_masked, n_short, n_long, n_batches, n_oversize, n_batch_pad; } tk_regroup;
/* ids already on the device (encode's own outputs, a join's ids / offsets / labels, or the caller's; d_id_offsets: n_docs + 1
 * uint64) -> the regrouped documents.  d_labels: NULL or int32[n_ids]; d_keep: NULL or uint8[n_docs].  out's buffers are device
 * buffers owned by the context, valid until the next regroup call on it, and SEPARATE from the encode, spans, dense, packed, join,
 * window, rowfit and decode outputs: out->ids / out->offsets (and out->offsets + first_doc for one batch: the passes index
 * ids[offsets[d] + j]) are meant to go into those passes next.  The work is enqueued on hip_stream and the call returns after
 * the stream has drained. */
int tk_regroup_from_ids_device(tk_ctx* ctx, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                               const void* d_labels, const void* d_keep, const tk_regroup_opts* opts, void* hip_stream, tk_regroup* out);
/* tk_encode_batch_device_ex + the regroup pass on the same stream.  Text has neither a labels stream nor a keep mask:
 * TK_REGROUP_LABELS is refused before anything is encoded, here and in tk_encode_batch_regroup.  The ragged outputs of encode
 * (*d_ids / *d_out_offsets / *n_ids as tk_encode_batch_device) are returned as well. */
int tk_encode_batch_device_regroup(tk_ctx* ctx, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                   int add_bos, int add_eos, int checks, const tk_regroup_opts* opts, void* hip_stream,
                                   void** d_ids, void** d_out_offsets, uint64_t* n_ids, tk_regroup* out);
/* Host in / host out: tk_encode_batch + the regroup pass.  out's buffers are pinned host memory, released with tk_free_regroup (an
 * unselected output is NULL). */
int tk_encode_batch_regroup(tk_ctx* ctx, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos, int add_eos,
                            int validate_utf8, const tk_regroup_opts* opts, tk_regroup* out);
void tk_free_regroup(tk_regroup* out);
/* As tk_last_rowfit_ms, for tools/regroup_time.py: GPU time of the stages of the context's last regroup pass, from events on its
 * stream: ms[0] the selection and its compaction (the host read behind it is not counted), ms[1] the sort (keys, radix passes,
 * the new offsets), ms[2] the gather kernel, ms[3] the batches.  All 0 where the pass was refused; a stage that launched nothing
 * is 0 or the cost of two event records. */
void tk_last_regroup_ms(const tk_ctx* ctx, float ms[4]);

/* ---- word ids: the pre-tokenization piece every id came from (HF tokenizers' word_ids(), word_to_tokens(), token_to_word();
 * no reference equivalent: the reference splits inside CoreBPE::encode, src/tekkenizer.rs:384-386, and keeps no trace of it) ----
 * Inputs, all for the same documents: the text (bytes, doc_offsets) and the ids (ids, id_offsets: encode's own output or the
 * caller's).  Per document d:
 *   - F_d is the set of document-relative piece starts of the document's text under the pattern the context is set to: the
 *     hard-coded pattern, or the JSON pattern after tk_tokenizer_set_honour_pattern / tk_ctx_set_pattern(ctx, 1).  The
 *     document is split alone.  0 is in F_d iff the document is not empty.
 *   - (s_i, e_i) is the byte span of id i, as tk_token_spans_device defines it.  A special id has s == e.
 *   - begins(i) holds iff all three of these hold: s_i < e_i, s_i < doc_len(d), and s_i is in F_d.
 *   - word_ids[i] (uint32) is TK_WORD_NONE (HF's None) if s_i == e_i.  Otherwise it is #{ j <= i in document d : begins(j) } - 1.
 *     An id in front of the document's first begins wraps to TK_WORD_NONE.
 *   - n_words(d) = #{ i in d : begins(i) }.
 *   - doc_words (uint64, n_docs + 1) is the exclusive prefix sum of n_words.
 *   - word_first[doc_words[d] + w] (uint32, only with TK_WORDS_FIRST) is i - id_offsets[d] for the id with begins(i) and
 *     word_ids[i] == w.  The ids of word w are the non-special ids from there up to word_first of the document's next word.
 *     For the last word, they run up to the document's last id.
 * For encode's own output every piece is a run of whole tokens.  Then word_ids[i] is the index of the piece that holds token i
 * (what HF returns), and n_words(d) = |F_d|.
 * The definition is total.  It holds for any ids.  No read leaves the buffers (s_i < doc_len(d) is tested before the flag is
 * read).  Every word_first index lies in [doc_words[d], doc_words[d + 1]) by construction.
 * A document of 2^32 bytes or more is TK_ERR_INVALID_ARG.  An id outside the vocabulary is TK_ERR_RUNTIME.  Both are as in the
 * spans pass.
 * One check flag sits above the existing check bits, so one word can carry it with TK_CHECK_OFFSETS / TK_CHECK_UTF8:
 *   TK_WORDS_CHECK_ALIGNED  per document, the ids' text is exactly as long as the document; and no piece start lies strictly
 *                           inside a token's span (the invariant of encode that no token crosses a pre-token boundary)
 * A failed check returns TK_ERR_RUNTIME; the message names the document (and the document-relative id index of a token that
 * crosses a piece start), and *bad (optional) receives the first failing document.
 * A separate pass behind the unchanged encode pipeline (csrc/tk_words.hip): the piece-start flags of the text by
 * the split-only launch of the per-document encode kernel, which overwrites encode's temporaries and none of its outputs (a
 * document with malformed UTF-8 is split again piece by piece: every byte outside a well-formed sequence is a character of its
 * own there; the JSON pattern: a per-document kernel over the sequential matcher); the words kernel; the scan of the per-document
 * counts and one 8-byte read (n_words); with TK_WORDS_FIRST the same walk once more. */
#define TK_WORD_NONE 0xFFFFFFFFu
#define TK_WORDS_FIRST 1u                 /* opts.flags: also the document-relative first id of every word */
#define TK_WORDS_CHECK_ALIGNED 32
typedef struct tk_words_opts { uint32_t flags; } tk_words_opts;
typedef struct tk_words { uint32_t* word_ids; uint64_t* doc_words; uint32_t* word_first;
                          uint64_t n_docs, n_ids, n_words; } tk_words;
/* ids and text already on the device.  checks: 0 or TK_WORDS_CHECK_ALIGNED.  out's buffers are device buffers owned by the
 * context, valid until the next words call on it, and SEPARATE from the encode, spans, units and layout outputs: what earlier
 * calls on the context returned stays valid through this call.  d_doc_offsets must be well-formed (n_docs + 1 uint64 that end
 * at n_bytes).  The work is enqueued on hip_stream and the call returns after the stream has drained. */
int tk_words_from_ids_device(tk_ctx* ctx, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                             const void* d_bytes, const void* d_doc_offsets, uint64_t n_bytes, int checks, const tk_words_opts* opts,
                             void* hip_stream, tk_words* out, uint64_t* bad);
/* tk_encode_batch_device_ex + the words pass on the same stream.  checks may combine TK_CHECK_OFFSETS / TK_CHECK_UTF8 with
 * TK_WORDS_CHECK_ALIGNED.  *d_ids / *d_out_offsets / *n_ids as tk_encode_batch_device. */
int tk_encode_batch_device_words(tk_ctx* ctx, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                 int add_bos, int add_eos, int checks, const tk_words_opts* opts, void* hip_stream, void** d_ids,
                                 void** d_out_offsets, uint64_t* n_ids, tk_words* out, uint64_t* bad);
/* Host in / host out: tk_encode_batch + the words pass (batches of the one-launch small path included).  checks: 0 or
 * TK_WORDS_CHECK_ALIGNED.  ids_out as tk_encode_batch (tk_free_result); out's buffers are pinned host memory, released with
 * tk_free_words (word_first is NULL without TK_WORDS_FIRST). */
int tk_encode_batch_words(tk_ctx* ctx, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos, int add_eos,
                          int validate_utf8, int checks, const tk_words_opts* opts, tk_result* ids_out, tk_words* out, uint64_t* bad);
void tk_free_words(tk_words* out);
/* As tk_last_regroup_ms, for tools/words_time.py: GPU time of the stages of the context's last words pass, from events on its
 * stream: ms[0] the split launch (with the memset of the flags), ms[1] the words kernel, ms[2] the scan of the counts (the
 * 8-byte read behind it is not counted), ms[3] the word_first kernel.  All 0 where the pass was refused. */
void tk_last_words_ms(const tk_ctx* ctx, float ms[4]);

/* ---- sentence-pair rows: templates, truncation strategies, overflow (no reference equivalent: the reference encodes one text,
 * src/tekkenizer.rs:378; this is the text_pair half of HF tokenizers' call: truncation = longest_first / only_first / only_second,
 * stride, return_overflowing_tokens, token_type_ids, sequence_ids) ----
 * Input: P pairs as 2P parts, encoded without BOS / EOS as for the join pass.  Part 2p is the first text A_p (a ids), part 2p + 1
 * the second text B_p (b ids); d_ids and d_id_offsets[2P + 1] are as in tk_join_from_ids_device.  Options (tk_pair_opts):
 * max_length T, strategy (TK_PAIR_LONGEST_FIRST / TK_PAIR_ONLY_FIRST / TK_PAIR_ONLY_SECOND), stride s, max_fixed F, multiple_of m
 * (0 = none), pad_id, three fixed id lists head / sep / tail of n_head / n_sep / n_tail = 0..4 ids each ([BOS], [] or [EOS, BOS],
 * [EOS]) and the flags below.
 *   1. x = n_head + n_sep + n_tail ids of every row are fixed; c = T - x is left for the two texts.  c >= 2 is required.
 *   2. TK_PAIR_LONGEST_FIRST: one row per pair, both sides cut on the right: A' = A[:a'], B' = B[:b'].  a + b <= c: nothing is
 *      cut.  Otherwise, a <= b: a' = min(a, c / 2), b' = min(b, c - a'); a > b: b' = min(b, c / 2), a' = min(a, c - b') (c / 2
 *      rounded down): the shorter side keeps up to half of c, the longer one what is left.  Modelled after HF's longest_first
 *      (which removes one id at a time from the longer side); on ties with an odd c the two can differ by which side keeps
 *      the odd id.
 *   3. TK_PAIR_ONLY_SECOND: the fixed side is X = A, the windowed side V = B; TK_PAIR_ONLY_FIRST: X = B, V = A.  F == 0 reads as
 *      c - 1, otherwise 1 <= F <= c - 1 is required.  f = min(|X|, F) and X' = X[:f]; cw = c - f, v = |V|.  v <= cw: one row, V
 *      whole.  v > cw without TK_PAIR_OVERFLOW: one row with V[:cw].  v > cw with TK_PAIR_OVERFLOW: step = cw - s, the pair has
 *      w = 1 + ceil((v - cw) / step) windows and window k holds V[k * step : min(k * step + cw, v)]; the last window may be
 *      shorter (it is not right-aligned, as in the window pass).  s < c - F is required, so step >= 1 whatever the pair.
 *   4. Every row is head + A-part + sep + B-part + tail; the fixed ids and X' are repeated in every window of a pair.
 *   5. Rows are numbered pair by pair: pair_windows (uint64, P + 1 entries) is the exclusive prefix sum of w_p (w_p = 1 but for
 *      3.), strictly increasing, and W = pair_windows[P].
 *   6. Row length: L = T with TK_PAIR_FIXED, else L = min(the longest row, T) (x where every pair is empty, 0 for P == 0); then,
 *      if m > 0, L is rounded up to a multiple of m.
 *   7. Outputs, elements int32 or int64 with TK_PAIR_I64: input_ids[W, L] is the row followed by pad_id; mask[W, L] (uint8,
 *      TK_PAIR_MASK) is 1 under the row; type_ids[W, L] (uint8, TK_PAIR_TYPE_IDS) is 0 from the head through the sep, 1 from the
 *      first B id through the tail, 0 under a pad; sequence_ids[W, L] (uint8, TK_PAIR_SEQUENCE_IDS) is 0 under an id of A, 1
 *      under an id of B and TK_PAIR_SEQ_NONE under a fixed id or a pad; lengths[W] (uint32); window_pair[W] (uint32) the pair of
 *      every row (overflow_to_sample_mapping); window_start[W] (uint32) the index in V of the row's first id of V (k * step), 0
 *      where nothing is windowed; second_start[W] (uint32) the column of the row's first B id = n_head + the row's A ids + n_sep;
 *      spans[W, L, 2] (uint32, TK_PAIR_SPANS) the part-relative (start, end) of the id under every element, from a buffer with
 *      the layout of tk_token_spans_device's output over the 2P parts, (0, 0) under a fixed id or a pad; pair_windows as in 5.
 *      An unselected output is NULL.  Counts, filled always: n_pairs = P; n_windows = W; row_len = L; n_truncated = the pairs
 *      with a row that lacks an id of A or of B (a + b > c in 2.; |X| > F or v > cw in 3., split pairs included); n_split = the
 *      pairs with w_p > 1; n_fixed_cut = the pairs with |X| > F.
 *   8. TK_ERR_INVALID_ARG, nothing written, an earlier pair result stays readable: c < 2 (T == 0 included: T == 0 is invalid with
 *      and without TK_PAIR_FIXED); an unknown strategy or flag; a list count above 4; TK_PAIR_OVERFLOW or s > 0 with
 *      TK_PAIR_LONGEST_FIRST; F > c - 1; s >= c - F; an odd number of parts; TK_PAIR_SPANS without a spans buffer in the from-ids
 *      entry; T or the rounded L beyond 2^31 - 1; W >= 2^32; W * L > 2^36; a part of 2^32 - 1 ids or more; no part with
 *      n_ids > 0.  A failed allocation is TK_ERR_RUNTIME.  P == 0 is valid and gives W == 0.
 * The layout is a separate pass behind the unchanged encode pipeline (csrc/tk_pair.hip): every element of every
 * selected output is written once, pad included, in 16-byte stores where L is a multiple of 4 (element stores otherwise).  W is not
 * known before the per-pair counts have been summed: one small read (W, the longest row, the counts) sizes the tensors, and one
 * wait ends the call. */
#define TK_PAIR_LONGEST_FIRST 0
#define TK_PAIR_ONLY_FIRST 1
#define TK_PAIR_ONLY_SECOND 2
#define TK_PAIR_FIXED 1
#define TK_PAIR_I64 2
#define TK_PAIR_MASK 4
#define TK_PAIR_SPANS 8
#define TK_PAIR_TYPE_IDS 16
#define TK_PAIR_SEQUENCE_IDS 32
#define TK_PAIR_OVERFLOW 64
#define TK_PAIR_SEQ_NONE 255
typedef struct tk_pair_opts { uint32_t max_length, strategy, stride, max_fixed, multiple_of, pad_id, n_head, n_sep, n_tail;
                              uint32_t head[4], sep[4], tail[4]; uint32_t flags; } tk_pair_opts;
typedef struct tk_pair { void* input_ids; uint8_t *mask, *type_ids, *sequence_ids; uint32_t *lengths, *window_pair, *window_start,
                         *second_start, *spans; uint64_t* pair_windows;
                         uint64_t n_pairs, n_windows, row_len, n_truncated, n_split, n_fixed_cut; } tk_pair;
/* ids already on the device (encode's own outputs for add_bos = add_eos = 0, or the caller's; d_id_offsets: n_parts + 1 uint64,
 * [0] = 0, non-decreasing, [n_parts] = n_ids -- NOT checked, as in tk_window_from_ids_device: anything else is out-of-bounds
 * indexing on the device) -> rows.  n_parts = 2P.  d_spans: 2 * n_ids uint32 as tk_token_spans_device returns them, NULL without
 * TK_PAIR_SPANS.  out's buffers are device buffers owned by the context, valid until the next pair call on it, and SEPARATE from
 * the outputs of every other pass.  The work is enqueued on hip_stream and the call returns after the stream has drained. */
int tk_pair_from_ids_device(tk_ctx* ctx, const void* d_ids, const void* d_id_offsets, uint64_t n_parts, uint64_t n_ids,
                            const void* d_spans, const tk_pair_opts* opts, void* hip_stream, tk_pair* out);
/* tk_encode_batch_device_ex(add_bos = 0, add_eos = 0) over the 2P part texts + (with TK_PAIR_SPANS) the spans pass + the pair pass
 * on the same stream.  checks: TK_CHECK_OFFSETS / TK_CHECK_UTF8; the ragged outputs (*d_ids / *d_out_offsets / *n_ids as
 * tk_encode_batch_device) are returned as well. */
int tk_encode_pairs_device(tk_ctx* ctx, const void* d_bytes, const void* d_doc_offsets, uint64_t n_parts, uint64_t n_bytes, int checks,
                           const tk_pair_opts* opts, void* hip_stream, void** d_ids, void** d_out_offsets, uint64_t* n_ids,
                           tk_pair* out);
/* Host in / host out: tk_encode_batch over the part texts + the pair pass (batches of the one-launch small path included).  out's
 * buffers are pinned host memory, released with tk_free_pair (an unselected output is NULL). */
int tk_encode_pairs(tk_ctx* ctx, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_parts, int validate_utf8,
                    const tk_pair_opts* opts, tk_pair* out);
void tk_free_pair(tk_pair* out);

/* ---- decode: batch form of Tekkenizer::decode (src/tekkenizer.rs:436-560) ----
 * The engine needs the special-token strings for TK_POLICY_KEEP: entry i is the string of the special token
 * at POSITION i of the reference's all_special_tokens vector (src/tekkenizer.rs:108-116, 536-540);
 * n must equal num_special_tokens.  Copied. */
int tk_ctx_set_special_tokens(tk_ctx* ctx, const uint8_t* strings_blob, const uint32_t* string_offsets, uint32_t n);

typedef struct tk_text_result {
    uint8_t* bytes;     /* concatenated UTF-8 text of all documents */
    uint64_t* offsets;  /* n_docs + 1: document d is bytes[offsets[d] .. offsets[d+1]) */
    uint64_t n_bytes;
    uint64_t n_docs;
} tk_text_result;

/* For every document d (ids[id_offsets[d] .. id_offsets[d+1])) exactly the String that
 * Tekkenizer::decode(ids_d, policy) returns.  If ANY document would make the reference return Err, the call
 * fails as a whole and *bad_doc (optional) receives the first such document:
 *   TK_ERR_SPECIAL_POLICY  a special id under TK_POLICY_RAISE          (src/tekkenizer.rs:531-535)
 *   TK_ERR_RUNTIME         an id outside the vocabulary, or a non-special run that is not valid UTF-8
 *                          (CoreBPE::decode -> TokenizerError::Tokenizers, src/tekkenizer.rs:552-555) */
int tk_decode_batch(tk_ctx* ctx, const uint32_t* ids, const uint64_t* id_offsets, uint64_t n_docs, int policy,
                    tk_text_result* out, uint64_t* bad_doc);
void tk_free_text_result(tk_text_result* r);
/* Same with ids resident in HBM; outputs are context-owned device buffers valid until the next call. */
int tk_decode_batch_device(tk_ctx* ctx, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                           int policy, void* hip_stream, void** d_bytes, void** d_out_offsets, uint64_t* n_bytes,
                           uint64_t* bad_doc);

/* ---- lossy decode: invalid UTF-8 becomes U+FFFD instead of failing the call (no reference equivalent for whole documents; the
 * reference uses String::from_utf8_lossy for pieces, src/tekkenizer.rs:150) ----
 * Lossy text of a run of bytes: what python's bytes.decode("utf-8", "replace").encode() and Rust's from_utf8_lossy return
 * (WHATWG / Unicode "substitution of maximal subparts").  From the left: an ASCII byte is copied; a byte that cannot begin a
 * sequence (80..BF, C0, C1, F5..FF) becomes EF BF BD; a lead C2..F4 takes the longest prefix of its sequence that is still well
 * formed (second byte bounded by the lead -- E0: A0..BF, ED: 80..9F, F0: 90..BF, F4: 80..8F, otherwise 80..BF --, later bytes
 * 80..BF, never past the end of the run), a complete sequence is copied, a truncated prefix of 1..3 bytes becomes ONE EF BF BD,
 * and the scan goes on behind the prefix.
 * Lossy decode of a document follows the grouping of tk_decode_batch: every maximal run of non-special ids is lossy-decoded on its
 * own -- a character never spans a special id, not even one dropped under TK_POLICY_IGNORE, and never a document boundary --,
 * special runs are handled by the policy as in tk_decode_batch.  A special id under TK_POLICY_RAISE and an id outside the
 * vocabulary remain errors of the whole call, with the codes and *bad_doc of tk_decode_batch; only the UTF-8 error class is gone.
 * *n_replaced (optional): U+FFFD written; *first_bad_doc (optional): the first document with one, ~0 for none.
 * Where every run is valid the strict pipeline's buffers are the result: no kernel is added, no byte moved. */
int tk_decode_batch_lossy(tk_ctx* ctx, const uint32_t* ids, const uint64_t* id_offsets, uint64_t n_docs, int policy,
                          tk_text_result* out, uint64_t* bad_doc, uint64_t* n_replaced, uint64_t* first_bad_doc);
/* Same with ids resident in HBM; outputs are context-owned device buffers valid until the next call on the context. */
int tk_decode_batch_device_lossy(tk_ctx* ctx, const void* d_ids, const void* d_id_offsets, uint64_t n_docs, uint64_t n_ids,
                                 int policy, void* hip_stream, void** d_bytes, void** d_out_offsets, uint64_t* n_bytes,
                                 uint64_t* bad_doc, uint64_t* n_replaced, uint64_t* first_bad_doc);

/* Streaming decode for generation: all running sequences at once, a few new ids per sequence and step.  Every sequence carries a
 * uint32 state: bytes 0..2 hold up to three pending bytes, byte 3 their count 0..3; 0 is a fresh sequence (to reuse a slot the
 * caller zeroes its word).  A step takes a ragged batch of new ids (a sequence may have none) and returns for every sequence the
 * lossy text of `pending ++ bytes of the new ids` under the grouping above, except that a truncated prefix that reaches the end of
 * the step's bytes behind a non-special last id is not written: it becomes the new state.  A special id (a dropped one too)
 * writes an open prefix as one U+FFFD, in front of its own string under TK_POLICY_KEEP.  flags: TK_STREAM_FINAL writes every open
 * prefix as U+FFFD and leaves the states 0.  For any split of an id sequence into steps, the steps' texts plus the final flush are
 * the lossy decode of the whole sequence.
 * d_state (uint32[n_seqs]) is the caller's device memory, rewritten by the step; d_ids / d_id_offsets (uint64[n_seqs + 1]) as in
 * tk_decode_batch_device.  Outputs: context-owned device buffers, valid until the next stream step or lossy decode on the context.
 * Errors as tk_decode_batch (TK_ERR_SPECIAL_POLICY, TK_ERR_RUNTIME for an id outside the vocabulary), *bad_seq (optional) the
 * first such sequence; the state buffer is then untouched.  One lane walks one sequence: a long step is correct and slow --
 * prefill-sized input belongs in tk_decode_batch_device_lossy. */
#define TK_STREAM_FINAL 1
int tk_decode_stream_step_device(tk_ctx* ctx, void* d_state, const void* d_ids, const void* d_id_offsets, uint64_t n_seqs,
                                 uint64_t n_ids, int policy, int flags, void* hip_stream, void** d_bytes, void** d_out_offsets,
                                 uint64_t* n_bytes, uint64_t* bad_seq);
/* Host convenience: state (uint32[n_seqs], read and rewritten), ids and offsets in host memory; release with tk_free_text_result. */
int tk_decode_stream_step(tk_ctx* ctx, uint32_t* state, const uint32_t* ids, const uint64_t* id_offsets, uint64_t n_seqs, int policy,
                          int flags, tk_text_result* out, uint64_t* bad_seq);
/* As tk_last_rowfit_ms, for tools/decode_lossy_time.py: GPU time of the context's last lossy batch decode, from events on its
 * stream -- the strict pipeline in front, and the repair pass (0 where every run was valid). */
void tk_last_decode_lossy_ms(const tk_ctx* ctx, float* strict_ms, float* repair_ms);
/* ... and its counters: U+FFFD written, documents with one, kernels launched behind the strict pipeline (0: the fast path). */
void tk_last_decode_lossy_stats(const tk_ctx* ctx, uint64_t* n_replaced, uint64_t* n_bad_docs, uint64_t* n_repair_launches);

/* 18-bit wire format of token ids for the multi-GPU gather (no reference equivalent: the reference is one process on a
 * CPU; BASELINE north_star asks for "a single RCCL gather of token-id buffers over xGMI").  The link into the
 * gathering GPU bounds the job, and an id below 2^18 -- every Tekken vocabulary -- travels as 2.25 bytes instead of 4.
 * All pointers are device memory of the context's device; the work is enqueued on hip_stream and NOT waited for
 * (tk_pack_ids18_device returns after the stream has drained only because it has to report an id >= 2^18 as
 * TK_ERR_INVALID_ARG).  tk_ids18_bytes(n) = size of the packed form of n ids. */
uint64_t tk_ids18_bytes(uint64_t n_ids);
int tk_pack_ids18_device(tk_ctx* ctx, const void* d_ids, uint64_t n_ids, void* d_packed, void* hip_stream);
int tk_unpack_ids18_device(tk_ctx* ctx, const void* d_packed, uint64_t n_ids, void* d_ids, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * Node level: every GPU of one node behind ONE call (no reference equivalent: the reference is one thread on a CPU;
 * BASELINE north_star "shards ... across the 8xMI355X node with a single RCCL gather of token-id buffers over xGMI";
 * SURVEY section 8b `ctx_create(.., device_ids[], n_devices, ..)`).  One process; per device one context (tables
 * replicated), one stream, one host thread for the life of the node.  tk_node_encode_batch cuts the batch into contiguous runs of WHOLE
 * documents with balanced bytes, every device tokenizes its run, and the id buffers are gathered on device_ids[0] with
 * direct peer -> root RCCL transfers inside one ncclGroupStart / ncclGroupEnd (18 bits per id on the wire when every id
 * fits) -- for every document exactly what Tekkenizer::encode returns (src/tekkenizer.rs:378-405), in document order.
 * device_ids must be distinct (TK_ERR_INVALID_ARG otherwise).  RCCL is opened with dlopen only when n_devices > 1.
 * The result is released with tk_free_result. */
typedef struct tk_node tk_node;
int tk_node_create(const uint8_t* token_bytes, const uint32_t* token_offsets, uint32_t n_ranks, uint32_t num_special_tokens,
                   uint32_t bos_id, uint32_t eos_id, const int* device_ids, int n_devices, tk_node** out_node);
void tk_node_destroy(tk_node* node);
/* node == NULL: the last failing tk_node_create on this thread */
const char* tk_node_last_error(const tk_node* node);
int tk_node_encode_batch(tk_node* node, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos,
                         int add_eos, tk_result* out);
/* The same with CALLER-OWNED host buffers: ids_out[ids_capacity], offsets_out[n_docs + 1]; *n_ids_out = ids written (also set
 * when ids_capacity is too small: TK_ERR_INVALID_ARG, nothing written).  With every buffer from tk_host_alloc (pinned) the
 * copies up and down are asynchronous DMAs and nothing is allocated, pinned or copied on the host per call -- the form a
 * host that encodes batch after batch should use (the Rust shim's encode_batch_into). */
int tk_node_encode_batch_pinned(tk_node* node, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos,
                                int add_eos, uint32_t* ids_out, uint64_t ids_capacity, uint64_t* offsets_out, uint64_t* n_ids_out);
int tk_node_n_devices(const tk_node* node);
/* Device timings of the last tk_node_encode_batch: the slowest device's tokenization pipeline, and the exchange on the root
 * (first receive posted .. offsets rebased), milliseconds. */
int tk_node_last_timing(const tk_node* node, float* kernels_ms_max, float* gather_ms);
/* How the last batch was cut: text bytes and ids of every device's run (up to `cap` entries each; either pointer may be NULL).
 * Returns the number of devices.  Runs are contiguous whole documents with balanced BYTES: no run exceeds the mean by more than
 * one document. */
int tk_node_last_shards(const tk_node* node, uint64_t* shard_bytes, uint64_t* shard_ids, int cap);

/* Device timings of the last tk_encode_batch* call, from HIP events on the stream the kernels
 * ran on: whole pipeline and the dominant encode kernel alone (milliseconds). */
int tk_last_timing(const tk_ctx* ctx, float* pipeline_ms, float* encode_kernel_ms);
/* ... and the span from the end of that kernel to the end of the merge kernels (the scans in between included): on text with
 * many pieces outside the vocabulary (BASELINE configs[2]) the merge kernels, not the encode kernel, are the longest part. */
float tk_last_merge_ms(const tk_ctx* ctx);

/* Counters of the last call: documents handled by the long-piece path (pass 2), and documents the flat
 * chunk-per-wave kernel handed back to the per-document kernels (non-ASCII, very long runs / pieces). */
int tk_last_stats(const tk_ctx* ctx, uint64_t* n_long_docs, uint64_t* n_handed_back);

/* Pre-tokenization split only (vocab-free): out_is_start[i] = 1 iff a piece starts at byte i of
 * the packed buffer (host in / host out).  Debug / parity entry for the split rules. */
int tk_split_batch(tk_ctx* ctx, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs,
                   uint8_t* out_is_start);

/* ---- audio: the ids of a clip, and the log-mel features its [AUDIO] positions stand for (src/audio.rs, src/tekkenizer.rs:697-760) ----
 * The reference turns a clip into [BEGIN_AUDIO] [AUDIO]*N by integer frame arithmetic and executes no DSP; the features are the
 * Whisper-style log-mel spectrogram that Voxtral's preprocessing computes from the same configuration fields.
 * Config A = (sampling_rate sr, frame_rate fr, num_mel_bins M, hop_length H, window_size W, chunk_length_s: optional).
 *   1. Padding (audio.rs:439-463), a clip of n samples: with chunk_length_s, cf = (usize)(chunk_length_s * sr) and
 *      n' = ceil_div(n, cf) * cf (n = 0 stays 0); without, n' = max(n, W).  The padding is zeros at the end.
 *   2. Frames (audio.rs:562-577): T = n' / H where H divides n', else ceil(n' as f64 / H as f64 - 1.0), evaluated in double as the
 *      reference writes it (it equals floor(n' / H) wherever both were compared).
 *   3. Tokens: per = (usize)(sr as f64 / fr / H as f64), N = ceil(T as f64 / per as f64); the ids are [BEGIN_AUDIO] + [AUDIO] * N.
 *      per == 0 is TK_ERR_INVALID_CONFIG (the reference would divide by zero), and so is cf == 0.
 *   4. Segments: with chunks a segment is one chunk of cf samples and has T_s = T(cf) frames; without, the whole padded clip is
 *      the one segment.  Each segment is transformed on its own: reflection never reaches into a neighbour.
 *   5. Features of a segment x[0 .. L), L > W / 2: the centred STFT torch.stft(x, W, H, window=hann_window(W), center=True,
 *      pad_mode="reflect") with the last frame dropped.  w[i] = 0.5 - 0.5 cos(2 pi i / W) (periodic Hann); frame t < T_s reads
 *      p[tH + i], i < W, p[j] = x[r(j - W/2)], r(q) = -q for q < 0, 2(L-1) - q for q >= L, q otherwise; power = |X_k|^2, k < F =
 *      W/2 + 1; mel[m] = sum_k FB[k][m] power[k] with FB the reference's mel_filter_bank(F, M, 0, sr/2, sr) (audio.rs:684-748:
 *      Slaney scale and normalisation, built in double, kept as f32); Lg = log10(max(mel, 1e-10)); Lg = max(Lg, Lmax - 8), Lmax
 *      the maximum of Lg over the segment, or opts.log_mel_max where that is finite; feature = (Lg + 4) / 4, float32.
 *   6. Layout: the segments of all clips back to back in clip order; segment s is [M][T_s] row-major at element M * frame_off[s]
 *      (under a chunked config the whole output is a dense [S, M, T]).  clip_seg[c] .. clip_seg[c+1]: the segments of clip c.
 *   7. The zero padding is never materialised.  NaN / Inf samples propagate as IEEE arithmetic makes them (a NaN that reaches a
 *      segment's maximum is dropped by the maximum, as fmaxf does).  The transform is an exact-f32 product: no bf16 / fp16 operand.
 *      A clip's features do not depend on what else is in the batch, nor on the stream.
 *   8. tk_audio_set_config refuses (TK_ERR_INVALID_CONFIG) what the transform cannot do -- the loader keeps accepting what the
 *      reference accepts --: W odd, W < 4, W > 2048, H == 0, H > W, M == 0, M > 256, sr == 0, fr <= 0, chunk_length_s <= 0, per == 0,
 *      cf == 0 and a chunked config with cf <= W / 2.  The log-mel entries refuse (TK_ERR_INVALID_ARG, nothing written, an earlier
 *      result stays readable) an unknown flag (checks or opts), a NULL required argument, sample offsets that do not start at 0,
 *      decrease or do not end at n_samples (they are read on the host, which sizes the output from them: TK_CHECK_OFFSETS is
 *      accepted and changes nothing), more than 2^32 - 16 clips or segments, an output beyond 2^36 elements; and with TK_ERR_AUDIO
 *      a context without an audio config ("Audio encoder not configured").  A failed allocation is TK_ERR_RUNTIME.
 *      n_clips == 0 and clips without a segment are valid. */
typedef struct tk_audio_config {
    uint64_t sampling_rate;
    double frame_rate;
    uint64_t num_mel_bins, hop_length, window_size;
    double chunk_length_s;         /* valid where has_chunk_length != 0 */
    uint32_t has_chunk_length, pad;
} tk_audio_config;
/* Steps 1-4 for n_clips clips of n_samples[c] samples: padded[c] = n', n_frames[c] = the sum of T_s over the clip's segments,
 * n_tokens[c] = N, n_segments[c].  Any output may be NULL.  Pure host arithmetic, which the other audio entries use too.
 * TK_ERR_INVALID_CONFIG: sr == 0, H == 0, W == 0, M == 0, fr <= 0, chunk_length_s <= 0 (what the reference's constructors refuse),
 * per == 0, cf == 0. */
int tk_audio_layout(const tk_audio_config* cfg, const uint64_t* n_samples, uint64_t n_clips, uint64_t* padded, uint64_t* n_frames,
                    uint64_t* n_tokens, uint64_t* n_segments);
/* Builds the transform's tables for cfg -- the [W][2F] matrix of w[i] cos(2 pi i k / W) | -w[i] sin(2 pi i k / W), computed in double
 * and rounded once, and the filter bank as one (first_bin, n_bins, weights) run per mel filter -- and uploads them.  A refused
 * config leaves the context's earlier one in place. */
int tk_audio_set_config(tk_ctx* ctx, const tk_audio_config* cfg);
typedef struct tk_logmel_opts { float log_mel_max; /* NaN (or +-Inf): the per-segment maximum */ uint32_t flags; /* none defined: 0 */ } tk_logmel_opts;
typedef struct tk_logmel { float* features; uint64_t* frame_off; /* n_segments + 1 */ uint64_t* clip_seg; /* n_clips + 1 */
                           uint64_t n_clips, n_segments, n_frames, n_mel; } tk_logmel;
/* d_samples: float32, the clips back to back, unpadded; d_sample_offsets: n_clips + 1 uint64.  opts may be NULL (the per-segment
 * maximum).  out: device pointers of buffers the context owns, apart from every other pass's, valid until the next log-mel call
 * on the context.  The work is enqueued on hip_stream and the call returns after the stream has drained. */
int tk_audio_logmel_device(tk_ctx* ctx, const void* d_samples, const void* d_sample_offsets, uint64_t n_clips, uint64_t n_samples,
                           int checks, const tk_logmel_opts* opts, void* hip_stream, tk_logmel* out);
/* Host in / host out: out's buffers are pinned host memory, released with tk_free_logmel. */
int tk_audio_logmel(tk_ctx* ctx, const float* samples, const uint64_t* sample_offsets, uint64_t n_clips, const tk_logmel_opts* opts,
                    tk_logmel* out);
void tk_free_logmel(tk_logmel* out);
/* The frames of a tile of the product kernel: tests place segment lengths around its multiples. */
uint32_t tk_audio_frame_tile(void);
/* GPU time of the context's last log-mel call from events on its stream: ms[0] the product kernel, ms[1] the clamp kernel (0
 * with a fixed log_mel_max: it is not launched).  Both 0 where the call was refused. */
void tk_last_logmel_ms(const tk_ctx* ctx, float ms[2]);

/* ---- audio parts in chat rows: the ragged input of the join pass, built on the device ----
 * The join pass treats a part as "control id, then ids", so an audio part is control id [BEGIN_AUDIO] in front of N times [AUDIO].
 * Per part p the splice emits the part's own ids ids[offs[p] .. offs[p+1]) followed by part_tokens[p] copies of fill_id, with
 * new offsets: counts, one scan and a fill kernel.  d_part_tokens: n_parts uint32 (0 for a text part).  d_id_offsets is NOT
 * checked.  TK_ERR_INVALID_ARG, nothing written, an earlier result stays readable: a NULL required argument, n_parts >= 2^32 - 16.
 * out: device pointers of buffers the context owns, apart from every other pass's, valid until the next splice on the context. */
typedef struct tk_ragged { uint32_t* ids; uint64_t* offsets; uint64_t n_parts, n_ids; } tk_ragged;
int tk_audio_splice_device(tk_ctx* ctx, const void* d_ids, const void* d_id_offsets, uint64_t n_parts, uint64_t n_ids,
                           const void* d_part_tokens, uint32_t fill_id, void* hip_stream, tk_ragged* out);
/* How many splice calls on the context got as far as their buffers (tests: a batch without audio never does). */
uint64_t tk_audio_splice_calls(const tk_ctx* ctx);

/* ------------------------------------------------------------------------------------------
 * Tokenizer level: the host-side mirror of tekken::tekkenizer::Tekkenizer, exported so that
 * non-C++ hosts (the Rust shim, Python tests) can drive loader + encode + decode.
 * ---------------------------------------------------------------------------------------- */
typedef struct tk_tokenizer tk_tokenizer;

/* Tekkenizer::from_file (src/tekkenizer.rs:222-248).  device_id < 0 => host-only object
 * (loader, decode and accessors work; encode returns TK_ERR_NO_DEVICE). */
int tk_tokenizer_from_file(const char* path, int device_id, tk_tokenizer** out);
/* Same, from an in-memory tekken.json document. */
int tk_tokenizer_from_json(const char* json, size_t json_len, int device_id, tk_tokenizer** out);
void tk_tokenizer_destroy(tk_tokenizer* t);
/* Error text of the last failing call on t (t == NULL: last failing constructor on this thread). */
const char* tk_tokenizer_last_error(const tk_tokenizer* t);

/* Tekkenizer::encode (src/tekkenizer.rs:378-405) for one document; *ids is malloc'ed, free with
 * tk_free_ids. */
int tk_tokenizer_encode(tk_tokenizer* t, const char* text, size_t len, int add_bos, int add_eos,
                        uint32_t** ids, size_t* n_ids);
/* Batch addition (no reference equivalent; see tk_encode_batch). */
int tk_tokenizer_encode_batch(tk_tokenizer* t, const uint8_t* bytes, const uint64_t* doc_offsets,
                              uint64_t n_docs, int add_bos, int add_eos, tk_result* out);
void tk_free_ids(uint32_t* ids);
/* tk_encode_batch_parsed for one document (the specials pass above, through the same kernels): modes as tk_specials_opts.modes
 * (NULL: every special string is parsed), n_modes = num_special_tokens; *ids is malloc'ed, free with tk_free_ids. */
int tk_tokenizer_encode_parsed(tk_tokenizer* t, const char* text, size_t len, int add_bos, int add_eos, const uint8_t* modes,
                               uint32_t n_modes, uint32_t** ids, size_t* n_ids);
/* Tekkenizer::encode + the byte span of every id (see tk_token_spans_device for the definition); *ids and *spans (2 * n_ids
 * entries) are malloc'ed, free both with tk_free_ids.  The spans are computed on the host from the ids and the rank table (no
 * second launch); they equal what the spans kernel gives for the same ids. */
int tk_tokenizer_encode_with_spans(tk_tokenizer* t, const char* text, size_t len, int add_bos, int add_eos,
                                   uint32_t** ids, uint32_t** spans, size_t* n_ids);
/* Opt-in (row f-3): honour the `pattern` of the loaded tekken.json instead of ignoring it like the reference does
 * (src/tekkenizer.rs:74).  Only Mistral's pattern string is known; any other is refused with TK_ERR_INVALID_CONFIG.
 * See tk_ctx_set_pattern. */
int tk_tokenizer_set_honour_pattern(tk_tokenizer* t, int honour);

/* Batch decode on the GPU (needs a device-backed tokenizer); see tk_decode_batch. */
int tk_tokenizer_decode_batch(tk_tokenizer* t, const uint32_t* ids, const uint64_t* id_offsets, uint64_t n_docs,
                              int policy, tk_text_result* out, uint64_t* bad_doc);

/* Tekkenizer::decode (src/tekkenizer.rs:436-443); *text is malloc'ed (not NUL terminated beyond
 * *len, but a trailing NUL is added for convenience), free with tk_free_text. */
int tk_tokenizer_decode(tk_tokenizer* t, const uint32_t* ids, size_t n_ids, int policy, char** text,
                        size_t* len);
void tk_free_text(char* text);
/* Tekkenizer::decode_all (src/tekkenizer.rs:463-560): the segments decode() joins, one per run of special / non-special
 * ids -- *text holds them back to back (tk_free_text), seg_ends[i] (tk_free_offsets) is the END of segment i in *text. */
int tk_tokenizer_decode_all(tk_tokenizer* t, const uint32_t* ids, size_t n_ids, int policy, char** text, uint64_t** seg_ends,
                            size_t* n_segments);
void tk_free_offsets(uint64_t* offsets);
/* Tekkenizer::vocab (src/tekkenizer.rs:348-350): the piece string of every id, specials included, back to back in *text;
 * ends[id] is where the piece of `id` ends (vocab_size entries). */
int tk_tokenizer_vocab(tk_tokenizer* t, char** text, uint64_t** ends, size_t* n_pieces);

/* Accessors (src/tekkenizer.rs:260-350, 574-600, 617-695). */
uint32_t tk_tokenizer_vocab_size(const tk_tokenizer* t);
uint32_t tk_tokenizer_num_special_tokens(const tk_tokenizer* t);
const char* tk_tokenizer_version(const tk_tokenizer* t); /* "v3" | "v7" | "v11" | "v13" */
int tk_tokenizer_control_token(tk_tokenizer* t, const char* name, uint32_t* id); /* get_control_token */
int tk_tokenizer_is_special(const tk_tokenizer* t, uint32_t id);
int tk_tokenizer_is_byte(const tk_tokenizer* t, uint32_t id);
int tk_tokenizer_id_to_piece(tk_tokenizer* t, uint32_t id, char** text, size_t* len);
int tk_tokenizer_id_to_byte_piece(tk_tokenizer* t, uint32_t id, int policy, uint8_t** bytes, size_t* len);
/* config.pattern of the loaded tekken.json (src/config.rs:38-49; the reference parses and ignores it, src/tekkenizer.rs:74),
 * and whether the object came from a TK_TABLE_CACHE_DIR side file (row f-2) rather than from parsing the JSON. */
const char* tk_tokenizer_json_pattern(const tk_tokenizer* t);
int tk_tokenizer_from_cache(const tk_tokenizer* t);
/* Audio (src/tekkenizer.rs:697-760).  has_audio: the tekken.json carried an `audio` object (has_audio_support).  audio_config /
 * audio_ids: TK_ERR_AUDIO "Audio encoder not configured" without one.  encode_audio is the reference's signature minus the
 * waveform copy: a clip of n_samples samples at clip_rate -> *ids = [BEGIN_AUDIO] + [AUDIO] * N (malloc'ed, tk_free_ids) and
 * *padded_samples = n' (optional); a clip_rate other than the config's is TK_ERR_AUDIO "Resampling not yet implemented", as in
 * the reference (audio.rs:415-424).  A device-backed tokenizer has its engine context configured (tk_audio_set_config) at
 * construction where the transform can do the config. */
int tk_tokenizer_has_audio(const tk_tokenizer* t);
int tk_tokenizer_audio_config(tk_tokenizer* t, tk_audio_config* out);
int tk_tokenizer_audio_ids(tk_tokenizer* t, uint32_t* audio_id, uint32_t* begin_audio_id);
int tk_tokenizer_encode_audio(tk_tokenizer* t, uint64_t n_samples, uint64_t clip_rate, uint32_t** ids, size_t* n_ids,
                              uint64_t* padded_samples);
/* The engine context behind the tokenizer (NULL for host-only objects). */
tk_ctx* tk_tokenizer_ctx(tk_tokenizer* t);
/* The validated rank table (for building an oracle beside it in tests). */
int tk_tokenizer_rank_table(const tk_tokenizer* t, const uint8_t** blob, const uint32_t** offsets,
                            uint32_t* n_ranks);

#ifdef __cplusplus
}
#endif
#endif
