// tk_kernels.h -- host-callable launchers of the gfx950 kernels (tk_kernels.hip).
#ifndef TK_KERNELS_H
#define TK_KERNELS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tekken_hip.h"
#include "tk_encode_impl_args.h"
#include "tk_flat_args.h"
#include "tk_rows.h"

// mode 0: pass 1; mode 1: pass 2 (scratch-backed, every launched wave owns a scratch slice);
// mode 2: split only; mode 3: pass 1 over args.todo_list.  n_waves = waves launched (rounded up to whole 4-wave blocks)
hipError_t tk_launch_encode(const TkEncodeArgs& args, int mode, uint32_t n_waves, hipStream_t s);

// One launch for a small batch (<= TK_SMALL_MAX_DOCS documents): encode + scan + pack by a single workgroup.  bytes /
// out_ids / out_offs / status may be mapped pinned host memory.  status[0] != 0: a document needs pass 2, nothing usable
// was written; status[1] = total ids.
#define TK_SMALL_MAX_DOCS 1024
#define TK_SMALL_MAX_BYTES (64u << 10)
#define TK_SMALL_THREADS 1024
hipError_t tk_launch_small(const TkEncodeArgs& args, uint32_t* out_ids, uint64_t* out_offs, uint32_t* status, hipStream_t s);

// Workgroup-per-document pass over args.todo_list (documents with a long piece that is not a vocabulary key, handed on by
// pass 2): the long piece is merged in rounds by 16 waves (tk_long.hip).  Every block owns a scratch slice of
// args.scratch_words_per_wave words.
hipError_t tk_launch_encode_long(const TkEncodeArgs& args, uint32_t n_walk_waves, uint32_t n_merge_blocks, hipStream_t s);
hipError_t tk_launch_encode_long_merge(const TkEncodeArgs& args, uint32_t n_merge_blocks, uint32_t n_compact_blocks, hipStream_t s);

// counts[n] (u32) -> offs[n+1] (u64, exclusive prefix sum); block_sums: workspace of
// ceil(n/2048)+1 u64.  offs[n] (= total) is also what the host reads back.
hipError_t tk_launch_scan(const uint32_t* counts, uint64_t n, uint64_t* offs, uint64_t* block_sums, hipStream_t s);

// out_ids[out_offs[d] + k] = staging[doc_offs[d] + 2*d + k] for k < counts[d]
hipError_t tk_launch_compact(const uint32_t* staging, const uint64_t* doc_offs, const uint32_t* counts,
                             const uint64_t* out_offs, uint64_t n_docs, uint32_t* out_ids, hipStream_t s);

// UTF-8 validation of every document; *d_bad receives the number of invalid documents
hipError_t tk_launch_check_offsets(const uint64_t* doc_offs, uint64_t n_docs, uint64_t n_bytes, uint32_t* d_bad, hipStream_t s);
hipError_t tk_launch_validate(const uint8_t* bytes, const uint64_t* doc_offs, uint64_t n_docs, uint32_t* d_bad,
                              hipStream_t s);

// ---- flat path (tk_flat.hip, tk_flat_impl.h): one wave per 2048-byte region of the packed stream ----
// (counters16: the context's counter block, words by name in tk_counters.h; the pre-pass clears TKC_CLEARED words and TKC_MEMO_HITS)
hipError_t tk_launch_flat_firstdoc(const uint64_t* doc_offs, uint64_t n_docs, uint64_t n_chunks, uint32_t* first_doc,
                                   uint32_t* flags, uint32_t* holes, uint32_t* counters16, hipStream_t s);
hipError_t tk_launch_flat(const TkFlatArgs& a, hipStream_t s);
// the long-piece records of the flat kernel (65..TKF_LONGCAP bytes): n_waves persistent waves, scratch_words words of scratch each
#define TKF_LONG_SCRATCH_WORDS 2048u
hipError_t tk_launch_flat_long(const TkFlatArgs& a, uint32_t* work_counter, uint32_t* scratch, uint32_t scratch_words, uint32_t n_waves,
                               hipStream_t s);
// flagged documents -> todo list (count in *n_todo), the longest of them in *maxlen (atomicMax: zero it first)
hipError_t tk_launch_flat_todo(const uint32_t* flags, const uint64_t* doc_offs, uint64_t n_docs, uint32_t* todo, uint32_t* n_todo,
                               uint32_t* maxlen, hipStream_t s);
// doc_info: [n_docs] 16-byte records (TkFlatDocInfo, tk_flat_tail_impl.h) written by counts, read by assemble
hipError_t tk_launch_flat_counts(const uint64_t* doc_offs, uint64_t n_docs, uint64_t n_bytes, uint64_t n_chunks,
                                 const uint64_t* P, const uint32_t* lstart, const uint32_t* flags, const uint32_t* holes,
                                 uint32_t extra, uint32_t* counts, void* doc_info, int final_pass, uint32_t* n_flagged, hipStream_t s);
hipError_t tk_launch_flat_assemble(uint64_t n_docs, const void* doc_info, const uint32_t* kcount, const uint64_t* out_offs,
                                   const uint32_t* tmp, const uint32_t* staging, uint32_t* out_ids, uint32_t bos_id,
                                   uint32_t eos_id, int add_bos, int add_eos, uint64_t* total_out, const uint32_t* skip_if, hipStream_t s);
// the first launch of tk_launch_merge on its own: which sub-queue holds the first item of every merge wave
hipError_t tk_launch_merge_wavefirst(const uint64_t* prefix, uint64_t n_chunks, uint32_t* wave_first, uint32_t* wave_first_wide,
                                     uint32_t* narrow_left_out, hipStream_t s);
hipError_t tk_launch_merge_kernels(const TkFlatArgs& a, hipStream_t s);   // both merge kernels, persistent grids (behind the wave-first launch or the folded apply)
hipError_t tk_launch_merge_all(const TkFlatArgs& a, hipStream_t s);       // ... as one launch: narrow loop, then the wide loops on the same LDS

// ---- the folded tail of the flat path (tk_flat_tail_impl.h): the same arrays from fewer launches; for n_chunks, n_docs >= 1 ----
// the first kernel of tk_launch_scan alone: raw (not scanned) sums of 2048 counts each
hipError_t tk_launch_scan_block_sums(const uint32_t* counts, uint64_t n, uint64_t* block_sums, hipStream_t s);
// tk_launch_scan(counts, n, prefix, ...) + tk_launch_merge_wavefirst in two launches; n >= 4 n_chunks (the sub-queue counts first)
hipError_t tk_launch_fold_apply(const uint32_t* counts, uint64_t n, uint64_t n_chunks, uint64_t* prefix, uint64_t* block_sums,
                                uint32_t* wave_first, uint32_t* wave_first_wide, uint32_t* narrow_left_out, hipStream_t s);
// tk_launch_flat_counts, and the counts' sums per 64 documents (group_sums[ceil(n_docs / 64)]) and per 4096 (doc_block_sums)
hipError_t tk_launch_flat_counts_sums(const uint64_t* doc_offs, uint64_t n_docs, uint64_t n_bytes, uint64_t n_chunks, const uint64_t* P,
                                      const uint32_t* lstart, const uint32_t* flags, const uint32_t* holes, uint32_t extra,
                                      uint32_t* counts, void* doc_info, int final_pass, uint32_t* n_flagged, uint64_t* group_sums,
                                      uint64_t* doc_block_sums, hipStream_t s);
// tk_launch_scan of the counts + tk_launch_flat_assemble in one launch: out_offs[0 .. n_docs] is WRITTEN here
hipError_t tk_launch_flat_assemble_fold(uint64_t n_docs, const void* doc_info, const uint32_t* kcount, const uint32_t* counts,
                                        const uint64_t* group_sums, const uint64_t* doc_block_sums, uint64_t* out_offs,
                                        const uint32_t* tmp, const uint32_t* staging, uint32_t* out_ids, uint32_t bos_id, uint32_t eos_id,
                                        int add_bos, int add_eos, uint64_t* total_out, const uint32_t* skip_if, hipStream_t s);

hipError_t tk_launch_iota(uint32_t* out, uint64_t n, hipStream_t s);   // out[i] = i
hipError_t tk_launch_add_u64(uint64_t* p, uint64_t n, uint64_t add, hipStream_t s);   // p[i] += add

// ---- 18-bit wire format of ids for the multi-GPU gather (tk_kernels.hip) ----
hipError_t tk_launch_pack18(const uint32_t* ids, uint64_t n, void* packed, uint32_t* d_bad, hipStream_t s);
hipError_t tk_launch_unpack18(const void* packed, uint64_t n, uint32_t* ids, hipStream_t s);

// ---- decode path (tk_decode.hip) ----
#define TK_DECODE_GROUP_DOCS 16u   /* consecutive documents the decode kernels take as one stream of ids */
struct TkDecodeArgs {
    const uint32_t* ids;       // [n_ids] packed token ids of all documents
    const uint64_t* id_offs;   // [n_docs + 1]
    uint64_t n_ids, n_docs;
    uint32_t* lens;            // [n_docs] text bytes of every document (per-document length pass: the fall-back form)
    uint32_t* glens;           // [ceil(n_docs / 16)] text bytes of every group of 16 consecutive documents (tk_decode_grouplen_kernel)
    const uint64_t* goffs;     // [groups + 1] exclusive scan of glens; non-NULL: the emit kernel starts a group there and writes out_offs itself
    uint32_t group_limit;      // a group with this many ids or text bytes (< 2^31) raises err[3]: the call takes the per-document pass
    uint8_t* out_bytes;        // [total bytes]
    uint64_t* out_offs;        // [n_docs + 1] exclusive scan of lens
    uint32_t* run_bits;        // bitmap over output bytes: 1 = a run starts here (hard UTF-8 boundary)
    uint32_t* doc_hi;          // [n_docs] written by emit: the document's text holds a byte >= 0x80 (only those are validated)
    unsigned long long* err;   // [3] see tk_decode.hip
    const uint8_t* tok_blob;   // token bytes by rank
    const uint32_t* tok_offs;  // [n_ranks + 1]
    const uint8_t* tok_inline; // [n_ranks] 16-byte entries: the token's bytes (<= 15) and its length in byte 15; 0xFF there = longer, see tok_offs
    const uint8_t* tok_len8;   // [n_ranks] length of the token, 0xFF = 255 bytes or more (see tok_offs)
    const uint8_t* sp_blob;    // special token strings by POSITION (reference src/tekkenizer.rs:536-540)
    const uint32_t* sp_offs;   // [num_special + 1]
    uint32_t n_ranks, num_special;
    int policy;                // TK_POLICY_*
};
hipError_t tk_launch_decode_doclen(const TkDecodeArgs& a, hipStream_t s);
hipError_t tk_launch_decode_grouplen(const TkDecodeArgs& a, hipStream_t s);   // err[3] != ~0: a group's text reaches 4 GiB, use the per-document pass
hipError_t tk_launch_decode_emit(const TkDecodeArgs& a, hipStream_t s);
hipError_t tk_launch_decode_validate(const TkDecodeArgs& a, hipStream_t s);

// ---- lossy decode (tk_decode_lossy.hip): the repair pass behind the strict pipeline, and the stream step ----
#define TK_LOSSY_TILE 4096u        /* raw text bytes of a block's tile */
#define TK_LOSSY_MAX_BLOCKS 2048u  /* grid cap of the two repair kernels (grid-stride beyond) */
struct TkLossyArgs {
    const uint8_t* bytes;      // the raw text of the batch (the emit kernel's output; readable 64 bytes past n_bytes)
    uint64_t n_bytes;
    const uint64_t* offs;      // [n_docs + 1] the raw text's document offsets
    uint64_t n_docs;
    const uint32_t* run_bits;  // the emit kernel's run starts, (n_bytes / 32 + 4) words
    uint32_t* tile_cnt;        // [n_tiles] written by the counts kernel
    const uint64_t* tile_offs; // [n_tiles + 1] their exclusive scan
    uint8_t* out_bytes;        // the lossy text
    uint64_t* out_offs;        // [n_docs + 1] its document offsets
    uint32_t* bad_flags;       // [n_docs] zeroed: set for a document with a replacement
    unsigned long long* stat;  // [0] U+FFFD written, [1] documents with one
};
hipError_t tk_launch_decode_lossy_counts(const TkLossyArgs& a, hipStream_t s);
hipError_t tk_launch_decode_lossy_write(const TkLossyArgs& a, hipStream_t s);
struct TkStreamArgs {
    uint32_t* state;           // [n_seqs] the open prefix of every sequence (include/tekken_hip.h), rewritten by the write kernel
    const uint32_t* ids;       // the step's new ids, ragged
    const uint64_t* id_offs;   // [n_seqs + 1]
    uint64_t n_seqs;
    uint32_t* lens;            // [n_seqs] text bytes of the step, written by the count kernel
    const uint64_t* out_offs;  // [n_seqs + 1] their exclusive scan
    uint8_t* out_bytes;
    unsigned long long* err;   // [0] first id index with a Raise-policy special token (or ~0), [1] first one outside the vocabulary
    unsigned long long* stat;  // [0] U+FFFD written
    const uint8_t* tok_blob;
    const uint32_t* tok_offs;
    const uint8_t* sp_blob;
    const uint32_t* sp_offs;
    uint32_t n_ranks, num_special;
    int policy, flags;         // TK_POLICY_*, TK_STREAM_*
};
hipError_t tk_launch_decode_stream_count(const TkStreamArgs& a, hipStream_t s);
hipError_t tk_launch_decode_stream_write(const TkStreamArgs& a, hipStream_t s);

// ---- per-token byte spans (tk_spans.hip) ----
struct TkSpansArgs {
    const uint32_t* ids;       // [n_ids] packed token ids of all documents
    const uint64_t* id_offs;   // [n_docs + 1]
    uint64_t n_docs;
    const uint64_t* doc_offs;  // [n_docs + 1] text offsets (TK_SPANS_CHECK_COVER / _BYTES only)
    const uint8_t* bytes;      // the packed text (TK_SPANS_CHECK_BYTES only)
    uint32_t* spans;           // [2 * n_ids] (start, end) per id, relative to the start of its document
    unsigned long long* err;   // [4] see tk_spans.hip
    const uint8_t* tok_blob;   // token bytes by rank
    const uint32_t* tok_offs;  // [n_ranks + 1]
    const uint8_t* tok_inline; // [n_ranks] 16-byte entries (TkDecodeArgs::tok_inline)
    const uint8_t* tok_len8;   // [n_ranks] one-byte lengths (TkDecodeArgs::tok_len8)
    uint32_t n_ranks, num_special;
};
hipError_t tk_launch_spans(const TkSpansArgs& a, int checks, hipStream_t s);

// ---- word ids: the pre-tokenization piece of every id (tk_words.hip) ----
struct TkWordsArgs {
    const uint32_t* ids;       // [n_ids] packed token ids of all documents
    const uint64_t* id_offs;   // [n_docs + 1]
    uint64_t n_docs;
    const uint64_t* doc_offs;  // [n_docs + 1] text offsets
    const uint8_t* flags;      // one byte per text byte: a piece starts here (the pass's own buffer, 64 zeroed bytes behind the text)
    uint32_t* word_ids;        // [n_ids] the word of every id, TK_WORD_NONE for a special id
    uint32_t* n_words;         // [n_docs] ids that begin a word
    const uint64_t* doc_words; // [n_docs + 1] exclusive scan of n_words (tk_launch_words_first)
    uint32_t* word_first;      // [n_words] the document-relative first id of every word (tk_launch_words_first)
    unsigned long long* err;   // [5] see tk_words.hip
    const uint8_t* tok_blob;   // token bytes by rank
    const uint32_t* tok_offs;  // [n_ranks + 1]
    const uint8_t* tok_inline; // [n_ranks] 16-byte entries (TkDecodeArgs::tok_inline; not read)
    const uint8_t* tok_len8;   // [n_ranks] one-byte lengths (TkDecodeArgs::tok_len8)
    uint32_t n_ranks, num_special;
};
hipError_t tk_launch_words(const TkWordsArgs& a, int check_aligned, hipStream_t s);   // word_ids, n_words, err
hipError_t tk_launch_words_first(const TkWordsArgs& a, hipStream_t s);                // word_first (behind the scan of n_words)
// behind the split-only launch of the encode kernel (hard-coded pattern): a document that holds a malformed UTF-8 byte is split
// again with the sequential matcher, which takes such a byte as a character of its own (as the oracle does)
hipError_t tk_launch_words_resplit(const TkTablesView& t, const uint8_t* bytes, const uint64_t* doc_offs, uint64_t n_docs, uint8_t* flags,
                                   hipStream_t s);
// flags[p] = 1 where a piece starts under the JSON pattern, every document split alone (flags zeroed by the caller)
hipError_t tk_launch_words_split_json(const TkTablesView& t, const uint8_t* bytes, const uint64_t* doc_offs, uint64_t n_docs, uint8_t* flags,
                                      hipStream_t s);

// ---- per-token spans in code points / UTF-16 units, annotation -> token range (tk_spans_units.hip) ----
struct TkSpansUnitsArgs {
    const uint32_t* ids;       // [n_ids] packed token ids of all documents
    const uint64_t* id_offs;   // [n_docs + 1]
    uint64_t n_docs;
    uint32_t* spans;           // [2 * n_ids] (start, end) per id in the unit, relative to the start of its document
    unsigned long long* err;   // [4] see tk_spans_units.hip ([2] and [3], as the byte pass numbers them)
    const uint8_t* tok_blob;   // token bytes by rank
    const uint32_t* tok_offs;  // [n_ranks + 1]
    const uint16_t* tok_units; // [n_ranks] the entries of tk_units_table.h
    uint32_t n_ranks, num_special;
};
hipError_t tk_launch_spans_units(const TkSpansUnitsArgs& a, int unit, hipStream_t s);   // unit: TK_UNIT_CHAR or TK_UNIT_UTF16
struct TkLocateArgs {
    const uint32_t* spans;     // [2 * n_ids] (start, end) per id, non-decreasing along a document
    const uint64_t* id_offs;   // [n_docs + 1]
    uint64_t n_docs, n_ids;
    const uint32_t* ann_doc;   // [n_ann] the document of every annotation
    const uint32_t* ann;       // [2 * n_ann] (as, ae) in the unit of spans
    uint64_t n_ann;
    uint32_t* out;             // [2 * n_ann] (lo, hi) document-relative id indices
    unsigned long long* err;   // [1] first annotation with ann_doc >= n_docs or as > ae (atomicMin: ~0 from the caller)
};
hipError_t tk_launch_spans_locate(const TkLocateArgs& a, hipStream_t s);   // n_ann == 0: nothing is launched

// ---- model-ready dense layout (tk_dense.hip) ----
struct TkDenseArgs {
    const uint32_t* ids;       // [n_ids] packed token ids of all documents
    const uint64_t* id_offs;   // [n_docs + 1]
    uint64_t n_docs;
    uint32_t row_len;          // L (< 2^31)
    uint32_t lim;              // max_length, 0xFFFFFFFF = none
    uint32_t keep_head, keep_tail, pad_id;
    uint32_t trunc_left, pad_left;
    void* out;                 // [n_docs * row_len] int32 or int64
    uint8_t* mask;             // [n_docs * row_len] or NULL
    uint32_t* lengths;         // [n_docs] kept ids of every row
    unsigned long long* stat;  // [0] longest document (tk_launch_dense_maxlen), [1] += truncated documents (tk_launch_dense)
    TkyRows rows;              // the launch shape (tk_rows.h; set by the launcher)
};
// row_len == 0 or n_docs == 0: nothing is launched (the caller zeroes lengths)
hipError_t tk_launch_dense(const TkDenseArgs& a, int i64, hipStream_t s);
hipError_t tk_launch_dense_maxlen(const uint64_t* id_offs, uint64_t n_docs, unsigned long long* stat, hipStream_t s);
struct TkRaggedArgs {
    const void* dense;         // [n_docs * row_len] int32 or int64
    uint64_t n_docs;
    uint32_t row_len, pad_id, pad_left;
    const uint32_t* given;     // [n_docs] the caller's lengths, or NULL: trim pad_id
    uint32_t* lens;            // [n_docs] out of tk_launch_ragged_rowlen (<= row_len), in of tk_launch_ragged_copy
    const uint64_t* offs;      // [n_docs + 1] exclusive scan of lens
    uint32_t* out_ids;
};
hipError_t tk_launch_ragged_rowlen(const TkRaggedArgs& a, int i64, hipStream_t s);
hipError_t tk_launch_ragged_copy(const TkRaggedArgs& a, int i64, hipStream_t s);

// ---- packed fixed-length training rows (tk_seqpack.hip) ----
struct TkSeqpackArgs {
    const uint32_t* ids;       // [n_ids] packed token ids of all documents: the stream
    const uint64_t* id_offs;   // [n_docs + 1]
    uint64_t n_docs;
    uint32_t row_len, pad_id;  // L (0 < L < 2^31)
    uint64_t n_rows, n_used;   // rows of the tensor; ids that go into it (the rest of the last row is pad)
    uint32_t* flags;           // [n_docs] the document has ids
    uint32_t* aflags;          // [n_docs] ... and starts at a multiple of L
    const uint64_t* fpos;      // [n_docs + 1] exclusive scan of flags; [n_docs] = M, the non-empty documents
    const uint64_t* apos;      // [n_docs + 1] exclusive scan of aflags
    uint64_t* starts;          // [M + 1] starts of the non-empty documents, strictly increasing; [M] = n_ids
    uint64_t* n_aligned;       // [M + 1] apos of the same documents: aligned starts before each
    void* out_ids;             // [n_rows * L] int32 or int64
    void* out_pos;             // the same shape, or NULL
    void* out_seg;             // the same shape, or NULL
    int32_t* cu;               // [n_segments + 1] (at most n_docs + n_rows + 1), or NULL
    unsigned long long* stat;  // [0] = n_segments, [1] = max_seqlen (atomicMax: zeroed by the caller)
    uint32_t ids_al16;         // ids is 16-byte aligned (set by the launcher)
};
hipError_t tk_launch_seqpack_flags(const TkSeqpackArgs& a, hipStream_t s);    // flags, aflags
hipError_t tk_launch_seqpack_starts(const TkSeqpackArgs& a, hipStream_t s);   // starts, n_aligned (behind the two scans)
hipError_t tk_launch_seqpack(const TkSeqpackArgs& a, int i64, hipStream_t s); // the tensors; n_rows == 0: nothing is launched
hipError_t tk_launch_seqpack_cu(const TkSeqpackArgs& a, hipStream_t s);       // cu_seqlens (a.cu != NULL), n_segments, max_seqlen

// ---- what the arguments of the window and chunk passes share: their rows are head | a run of the body | tail of a document ----
struct TkRowFillArgs {
    const uint32_t* ids;       // [n_ids] packed token ids of all documents
    const uint64_t* id_offs;   // [n_docs + 1]
    const uint32_t* in_spans;  // [2 * n_ids] (start, end) per id, or NULL (the chunk pass's levels kernel: its input)
    uint64_t n_docs;
    uint32_t max_len;          // T
    uint32_t keep_head, keep_tail, pad_id;
    uint32_t row_len;          // L (< 2^31; 0: only the per-row outputs are written)
    uint64_t n_rows;           // W (< 2^32)
    uint32_t* counts;          // [n_docs] w_d
    const uint64_t* doc_windows;   // [n_docs + 1] exclusive scan of counts, strictly increasing
    void* out;                 // [W * L] int32 or int64
    uint8_t* mask;             // [W * L] or NULL
    uint32_t* out_spans;       // [W * L * 2] or NULL
    uint32_t* lengths;         // [W]
    uint32_t* window_doc;      // [W]
    uint32_t* window_start;    // [W]
    // zeroed by the caller: [0] longest document, clamped to 2^32 - 1 (atomicMax), [1] += documents with w_d > 1; the chunk pass:
    // [2 .. 8) += the cuts made at level 0 .. 5
    unsigned long long* stat;
    TkyRows rows;              // the launch shape (tk_rows.h; set by the launcher)
};

// ---- overlapping windows for long documents (tk_window.hip) ----
struct TkWindowArgs : TkRowFillArgs {
    uint32_t step;             // c - s
};
hipError_t tk_launch_window_counts(const TkWindowArgs& a, hipStream_t s);   // counts, stat
hipError_t tk_launch_window(const TkWindowArgs& a, int i64, hipStream_t s); // the outputs; n_rows == 0: nothing is launched

// ---- boundary-aware token-budget chunks (tk_chunk.hip) ----
struct TkChunkRec { uint32_t start, len, level, pad; };   // a chunk's body run B[start : start + len] and the level of the cut behind it
struct TkChunkArgs : TkRowFillArgs {
    const uint8_t* lev;        // [n_ids] the level of the break in front of every id (a byte above 5 reads as 5)
    uint32_t min_len, overlap; // m; o (0 <= o < m <= c = T - h - t)
    uint32_t group;            // documents a wave of the walk takes (a power of two <= 64; set by the launcher)
    TkChunkRec* rec;           // [W] out of the second walk, in of the fill kernel
    uint8_t* cut_level;        // [W]
    uint32_t* chunk_bytes;     // [W * 2] or NULL
    // the levels kernel alone
    const uint8_t* bytes;      // the text
    const uint64_t* doc_offs;  // [n_docs + 1]
    uint32_t demote;           // 4 bits a level: what level L becomes under the caller's mask
    uint8_t* lev_out;          // [n_ids]
};
hipError_t tk_launch_chunk_levels(const TkChunkArgs& a, hipStream_t s);         // lev_out
hipError_t tk_launch_chunk_walk(const TkChunkArgs& a, int records, hipStream_t s);   // 0: counts, stat; 1: rec (behind the scan)
hipError_t tk_launch_chunk(const TkChunkArgs& a, int i64, hipStream_t s);       // the outputs; n_rows == 0: nothing is launched

// ---- sentence-pair rows (tk_pair.hip) ----
struct TkPairArgs {
    const uint32_t* ids;       // [n_ids] packed token ids of the 2P parts, encoded without BOS / EOS
    const uint64_t* id_offs;   // [2 * n_pairs + 1]
    const uint32_t* in_spans;  // [2 * n_ids] (start, end) per id, or NULL
    uint64_t n_pairs;
    uint32_t max_len, cap;     // T; c = T - x
    uint32_t strategy;         // TK_PAIR_LONGEST_FIRST / _ONLY_FIRST / _ONLY_SECOND
    uint32_t overflow;         // TK_PAIR_OVERFLOW: a windowed side longer than its room gives several rows
    uint32_t stride, max_fixed;    // s; F (resolved: never 0 with an ONLY_ strategy)
    uint32_t n_head, n_sep, n_tail;
    uint32_t head[4], sep[4], tail[4];
    uint32_t pad_id;
    uint32_t row_len;          // L (< 2^31; 0: only the per-row outputs are written)
    uint64_t n_rows;           // W (< 2^32)
    uint32_t* counts;          // [n_pairs] w_p
    const uint64_t* pair_windows;  // [n_pairs + 1] exclusive scan of counts, strictly increasing
    void* out;                 // [W * L] int32 or int64
    uint8_t* mask;             // [W * L] or NULL
    uint8_t* type_ids;         // [W * L] or NULL
    uint8_t* seq_ids;          // [W * L] or NULL
    uint32_t* out_spans;       // [W * L * 2] or NULL
    uint32_t* lengths;         // [W]
    uint32_t* window_pair;     // [W]
    uint32_t* window_start;    // [W]
    uint32_t* second_start;    // [W]
    // zeroed by the caller: [0] the longest row and [4] the longest part, clamped to 2^32 - 1 (atomicMax); [1] += pairs that lost
    // an id, [2] += pairs with w_p > 1, [3] += pairs whose fixed side was cut
    unsigned long long* stat;
    TkyRows rows;              // the launch shape (tk_rows.h; set by the launcher)
};
hipError_t tk_launch_pair_counts(const TkPairArgs& a, hipStream_t s);     // counts, stat
hipError_t tk_launch_pair(const TkPairArgs& a, int i64, hipStream_t s);   // the outputs; n_rows == 0: nothing is launched

// ---- chat batches: parts joined with control ids, plus labels (tk_join.hip) ----
struct TkJoinArgs {
    const uint32_t* ids;       // [n_ids] packed token ids of all parts, encoded without BOS / EOS
    const uint64_t* id_offs;   // [n_parts + 1]
    uint64_t n_parts, n_convs;
    const uint32_t* ctrl;      // [n_parts] a control id or TK_JOIN_NONE
    const uint32_t* pflags;    // [n_parts] TK_PART_LABEL_* or NULL (all zero)
    const uint64_t* conv_offs; // [n_convs + 1]
    uint64_t cap;              // elements the outputs hold (n_ids + n_parts): nothing is written at or beyond it
    uint32_t num_special;      // (the check kernel)
    int32_t ignore;            // ignore_index
    uint32_t* has;             // [n_parts] the part has a control id
    const uint64_t* cb;        // [n_parts + 1] exclusive scan of has: control ids before the part; [n_parts] = n_ctrl
    uint64_t* start;           // [n_parts + 1] id_offs + cb: where the part starts in the output, non-decreasing; [n_parts] = N
    uint32_t* plocal;          // [n_parts] the part's index inside its conversation (only with part_index)
    uint32_t* out_ids;         // [N]
    uint64_t* out_offs;        // [n_convs + 1]
    int32_t* labels;           // [N] or NULL
    uint32_t* part_index;      // [N] or NULL
    unsigned long long* stat;  // [0] += n_labelled; [1], [2]: the first bad conversation / part (atomicMin: ~0 from the caller)
};
hipError_t tk_launch_join_check(const TkJoinArgs& a, hipStream_t s);   // TK_CHECK_PARTS: stat[1], stat[2]
hipError_t tk_launch_join_has(const TkJoinArgs& a, hipStream_t s);     // has
hipError_t tk_launch_join_parts(const TkJoinArgs& a, hipStream_t s);   // start, plocal, out_offs, n_labelled (behind the scan of has)
hipError_t tk_launch_join(const TkJoinArgs& a, hipStream_t s);         // ids, labels, part_index; n_parts == 0: nothing is launched

// ---- whole documents placed next-fit into rows, never cut (tk_rowfit.hip) ----
struct TkRowfitArgs {
    const uint32_t* ids;       // [n_ids] packed token ids of all documents
    const int32_t* lab;        // [n_ids] a second stream with the same offsets, or NULL
    const uint64_t* id_offs;   // [n_docs + 1]
    uint64_t n_docs;
    uint32_t row_len, pad_id;  // L (0 < L < 2^31)
    uint32_t keep_tail;        // ids of an over-long document's end that survive (<= L)
    int32_t ignore;            // ignore_index
    uint64_t n_rows;           // known behind the chain: tk_launch_rowfit_place and later
    uint32_t* e;               // [n_docs] min(n_d, L)
    uint32_t* nz;              // [n_docs] the document has ids
    const uint64_t* E;         // [n_docs + 1] exclusive scan of e
    const uint64_t* nzp;       // [n_docs + 1] exclusive scan of nz
    uint64_t *jump_a, *jump_b; // [n_docs + 1] the jump table and its square: target | steps << 32
    uint32_t* row;             // [n_docs + 1] the row a document opens, 0xFFFFFFFF = none; [n_docs] = n_rows
    uint64_t* open;            // [n_rows + 1] (at most n_docs + 1) the documents that open a row, increasing; [n_rows] = n_docs
    uint32_t* padf;            // [n_rows] the row has pads
    const uint64_t* padp;      // [n_rows + 1] exclusive scan of padf
    uint64_t* dstart;          // [n_docs + 1] doc_start, non-decreasing; [n_docs] = n_rows * L
    uint32_t* segno;           // [n_docs] the document's number inside its row, from 1
    void* out_ids;             // [n_rows * L] int32 or int64
    int32_t* out_lab;          // the same shape, int32, or NULL
    void* out_pos;             // the shape and type of out_ids, or NULL
    void* out_seg;             // the shape and type of out_ids, or NULL
    int32_t* cu;               // [n_segments + 1] (at most n_docs + n_rows + 1), or NULL
    unsigned long long* stat;  // [0] += n_truncated, [1] = n_segments, [2] = max_seqlen (atomicMax): zeroed by the caller;
                               // [3] = n_rows, [4] = sum e, [5] = id_offs[n_docs] (tk_launch_rowfit_chain)
};
hipError_t tk_launch_rowfit_len(const TkRowfitArgs& a, hipStream_t s);     // e, nz, n_truncated (n_docs > 0)
hipError_t tk_launch_rowfit_chain(const TkRowfitArgs& a, uint32_t rounds, hipStream_t s);   // jump, row, open (behind the scan of e)
// the doubling rounds and the openers alone, over a chain whose first links the caller has written (jump_a[v] = nxt(v) | 1 << 32,
// jump_a[n_docs] = n_docs, row[v] = v ? 0xFFFFFFFF : 0): what tk_launch_rowfit_chain runs behind its own nxt kernel, and the
// regroup pass behind its.  Reads E[n_docs] and id_offs[n_docs] into stat[4], stat[5] and writes stat[3] = the links of the chain
hipError_t tk_launch_chain_rounds(const TkRowfitArgs& a, uint32_t rounds, hipStream_t s);
hipError_t tk_launch_rowfit_place(const TkRowfitArgs& a, hipStream_t s);   // dstart, segno, padf (n_rows known)
hipError_t tk_launch_rowfit(const TkRowfitArgs& a, int i64, hipStream_t s);   // the tensors; n_rows == 0: nothing is launched
hipError_t tk_launch_rowfit_cu(const TkRowfitArgs& a, hipStream_t s);      // cu_seqlens (a.cu != NULL), n_segments, max_seqlen (behind the scan of padf)

// ---- documents selected, reordered and cut into batches (tk_regroup.hip) ----
#define TKG_CHUNK 2048u        /* (key, document) pairs of a block of a radix pass */
#define TKG_FAN 64u            /* entries of a level of the maximum pyramid under one entry of the next */
#define TKG_MAX_LEVELS 6       /* 64^6 > 2^32 */
struct TkRegroupArgs {
    const uint32_t* ids;       // [n_ids] packed token ids of all documents
    const int32_t* lab;        // [n_ids] a second stream with the same offsets, or NULL
    const uint64_t* id_offs;   // [n_docs + 1]
    const uint8_t* keep;       // [n_docs] or NULL
    uint64_t n_docs;           // D (< 2^32)
    uint64_t n_kept;           // K: known behind the host read
    uint64_t n_out;            // ids of the kept documents: known behind the host read
    uint64_t max_tokens;
    uint32_t min_len, max_len, order, seed, window, max_docs, desc;
    uint32_t longest;          // the longest kept document: known behind the host read
    uint32_t* flag;            // [n_docs] the document is kept
    const uint64_t* fpos;      // [n_docs + 1] exclusive scan of flag
    uint32_t* kept;            // [K] c: the kept documents, increasing
    const uint32_t *key_in, *val_in;   // [K] the pairs of a radix pass ...
    uint32_t *key_out, *val_out;       // ... and where it puts them
    uint32_t* hist;            // [256 * blocks] digit-major counts of a radix pass
    const uint64_t* hpos;      // [256 * blocks + 1] exclusive scan of hist
    const uint32_t* shuf;      // [K] GROUPED: the documents in shuffled order (val is the rank in it)
    uint32_t* perm;            // [K]
    uint32_t* len;             // [K] m_k = n_perm[k]
    uint64_t* src;             // [K] id_offs[perm[k]]
    uint64_t* out_offs;        // [K + 1] exclusive scan of len
    uint32_t* out_ids;         // [n_out]
    int32_t* out_lab;          // [n_out] or NULL
    uint32_t* pyr;             // the maximum pyramid over len: level l (from 1) at pyr + pyr_at[l], ceil(K / 64^l) entries
    uint64_t pyr_at[TKG_MAX_LEVELS + 1];
    uint32_t n_levels;         // levels above len
    uint64_t* jump;            // [K + 1] the chain's first links (TkRowfitArgs.jump_a)
    uint32_t* row;             // [K + 1] the batch a document opens, 0xFFFFFFFF = none; [K] = n_batches
    uint32_t* bmax;            // [K] the longest document of the batch that would open at k
    const uint64_t* open;      // [n_batches + 1] the documents that open a batch; [n_batches] = K
    uint64_t* batch_offs;      // [n_batches + 1] or NULL
    uint32_t* batch_rowlen;    // [n_batches] or NULL
    unsigned long long* stat;  // [0..2] += n_masked, n_short, n_long; [3] += ids of the kept documents; [4] = K; [5] = id_offs[D];
                               // [6] = the longest kept document (atomicMax); [7] += documents of 2^32 ids or more: zeroed by the
                               // caller.  [8] += n_oversize; [9] += sum cnt * rowlen; [10] = n_batches.  [12..15]: the chain's own
};
hipError_t tk_launch_regroup_select(const TkRegroupArgs& a, hipStream_t s);    // flag, stat[0..3], [6], [7] (n_docs > 0)
hipError_t tk_launch_regroup_compact(const TkRegroupArgs& a, hipStream_t s);   // kept, stat[4], stat[5] (behind the scan of flag)
hipError_t tk_launch_regroup_keys(const TkRegroupArgs& a, int what, hipStream_t s);   // key_out / val_out of K pairs: what = 0 the order's key of kept[k] | 1 GROUPED's length key of rank k | 2 GROUPED's group of val_in[k]
uint32_t tk_regroup_sort_blocks(uint64_t n_kept);
hipError_t tk_launch_regroup_hist(const TkRegroupArgs& a, uint32_t shift, hipStream_t s);      // hist of digit (key_in >> shift) & 255
hipError_t tk_launch_regroup_scatter(const TkRegroupArgs& a, uint32_t shift, hipStream_t s);   // key_out, val_out (behind the scan of hist)
hipError_t tk_launch_regroup_perm(const TkRegroupArgs& a, hipStream_t s);      // perm (GROUPED: shuf[val_in]; else a copy of val_in where they differ), len, src
hipError_t tk_launch_regroup_gather(const TkRegroupArgs& a, hipStream_t s);    // out_ids, out_lab; n_out == 0: nothing is launched
hipError_t tk_launch_regroup_pyramid(const TkRegroupArgs& a, hipStream_t s);   // pyr
hipError_t tk_launch_regroup_nxt(const TkRegroupArgs& a, hipStream_t s);       // jump, row, bmax
hipError_t tk_launch_regroup_batches(const TkRegroupArgs& a, hipStream_t s);   // batch_offs, batch_rowlen, stat[8..10] (behind tk_launch_chain_rounds)

// ---- special-token strings parsed out of text: matches, parts, the text without them (tk_specials.hip) ----
#define TKS_TILE 4096u         /* text bytes of a block's tile of the candidate kernel (16 a thread) */
#define TKS_MAXLEN 255u        /* the longest string that can be matched: the look-ahead behind a tile is TKS_MAXLEN - 1 bytes */
#define TKS_NONE 0xFFFFFFFFu
#define TKS_RAISE 0x80000000u  /* the bit of a candidate's id that says its mode is TK_SPECIAL_RAISE */
// the automaton's transition table: open addressing, an entry is (key + 1) << 32 | child with key = node << 8 | byte, 0 = empty
static inline __host__ __device__ uint32_t tks_edge_slot(uint32_t key, uint32_t mask) {
    uint32_t h = key * 0x9E3779B1u;
    h ^= h >> 15;
    return h & mask;
}
struct TkSpecialsArgs {
    const uint8_t* bytes;      // [n_bytes] the text
    const uint64_t* doc_offs;  // [n_docs + 1]
    uint64_t n_docs, n_bytes;
    const uint64_t* edges;     // [edge_mask + 1] the byte trie over the context's strings (node 0: the root)
    uint32_t edge_mask;
    const uint32_t* term;      // [n_nodes] the distinct string that ends at the node, or TKS_NONE
    const uint32_t* eff;       // [n_distinct] per call: the lowest id of the match set with that string (| TKS_RAISE), or TKS_NONE
    uint32_t first[8];         // 256 bits: the first bytes of the match set
    uint32_t bos, eos;         // part 0's control id or TK_JOIN_NONE | the id of the closing part (eos_part != 0)
    uint32_t eos_part;         // 1 with TK_SPECIALS_EOS
    uint64_t n_tiles;          // ceil(n_bytes / TKS_TILE)
    uint32_t* tile_cnt;        // [n_tiles] candidates that start in the tile
    const uint64_t* tile_pos;  // [n_tiles + 1] exclusive scan of tile_cnt
    uint64_t n_cand;           // NC: known behind the first host read
    uint64_t* cpos;            // [NC + 1] where candidate c starts in the text, increasing; [NC] = n_bytes
    uint32_t* clen;            // [NC] the length of the longest string of the match set there (inside the document)
    uint32_t* cid;             // [NC] its id | TKS_RAISE
    uint32_t* cdoc;            // [NC] its document
    uint64_t* jump;            // [NC + 1] the chain's first links (TkRowfitArgs.jump_a)
    uint32_t* row;             // [NC + 1] the number of the match a candidate is, 0xFFFFFFFF = none; [NC] = n_matches
    const uint64_t* open;      // [n_matches + 1] the candidates that are matches, increasing; [n_matches] = NC
    uint32_t* flen;            // [NC] clen of a match, 0 of any other candidate
    const uint64_t* remc;      // [NC + 1] exclusive scan of flen: the bytes removed in front of candidate c; [NC] = n_removed
    uint64_t n_matches, n_removed;   // M, sum l: known behind the second host read
    uint64_t* mpos;            // [M] where match r starts in the text
    uint64_t* seg_out;         // [M + 1] where the text behind match r - 1 (r = 0: the head of the text) starts in the output, non-decreasing
    uint64_t* seg_src;         // [M + 1] ... and in the input
    uint8_t* out_bytes;        // [n_bytes - n_removed]
    uint64_t* part_offs;       // [P + 1], P = n_docs * (1 + eos_part) + M
    uint32_t* part_ctrl;       // [P]
    uint64_t* conv_offs;       // [n_docs + 1]
    uint64_t* part_src;        // [P] or NULL
    unsigned long long* stat;  // [0] = NC (tk_launch_specials_count_end); [1]: the first candidate that is a RAISE match (atomicMin: ~0 from
                               // the caller); [8..13]: the chain's own ([11] = M)
};
hipError_t tk_launch_specials_cand(const TkSpecialsArgs& a, int write, hipStream_t s);   // write = 0: tile_cnt | 1: cpos, clen, cid, cdoc (behind the scan of tile_cnt)
hipError_t tk_launch_specials_count_end(const TkSpecialsArgs& a, hipStream_t s);   // stat[0] = tile_pos[n_tiles]
hipError_t tk_launch_specials_nxt(const TkSpecialsArgs& a, hipStream_t s);         // jump, row (then tk_launch_chain_rounds)
hipError_t tk_launch_specials_mark(const TkSpecialsArgs& a, hipStream_t s);        // flen, stat[1] (behind the chain)
hipError_t tk_launch_specials_matches(const TkSpecialsArgs& a, hipStream_t s);     // mpos, seg_out, seg_src, the parts behind the matches (M known)
hipError_t tk_launch_specials_docs(const TkSpecialsArgs& a, hipStream_t s);        // conv_offs, the first and the closing part of every document, part_offs[P]
hipError_t tk_launch_specials_compact(const TkSpecialsArgs& a, hipStream_t s);     // out_bytes; nothing left: nothing is launched

// ---- fill-in-the-middle rows: documents cut in two places and reordered (tk_fim.hip) ----
#define TKI_TILE1 16384u       /* output bytes of a block's tile of the permute kernel over text: 64 a thread */
#define TKI_TILE4 4096u        /* output ids of a block's tile of the permute kernel over ids: 16 a thread */
#define TKI_SEED_BASE 0x46494D00u
#define TKI_HT 4u              /* the bit of a staged mode word that says the document has its head and tail */
// h(seed, d) of the regroup pass (include/tekken_hip.h TK_REGROUP_ORDER_SHUFFLE); the host makes the four s_k with it
static inline __host__ __device__ uint32_t tki_hash(uint32_t seed, uint32_t d) {
    uint32_t x = d * 0x9E3779B1u + seed;
    x ^= x >> 16; x *= 0x85EBCA6Bu;
    x ^= x >> 13; x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}
struct TkFimArgs {
    const void* units;         // [n_units] bytes or ids
    const uint64_t* offs;      // [n_docs + 1]
    uint64_t n_docs, n_units;
    const uint64_t* in_cuts;   // [n_docs][2] the caller's cuts, or NULL: drawn
    uint64_t rate, spm;        // rate_q32, spm_q32
    uint32_t s[4];             // s_k = h(seed, TKI_SEED_BASE + k)
    uint32_t ctrl[3];          // prefix_id, suffix_id, middle_id
    uint32_t head, tail, min_units, flags;
    uint32_t bos, eos;         // the control ids of parts 0 and 4 (TK_JOIN_NONE: none)
    void* out_units;           // [n_units]
    uint64_t* part_offs;       // [5 n_docs + 1]
    uint32_t* part_ctrl;       // [5 n_docs]
    uint32_t* part_flags;      // [5 n_docs]
    uint64_t* conv_offs;       // [n_docs + 1]
    uint64_t* part_src;        // [5 n_docs] or NULL
    uint64_t* cuts;            // [n_docs][2] (lo, hi) behind the snap, or TK_FIM_NO_CUT twice
    uint8_t* mode;             // [n_docs] 0 none | 1 PSM | 2 SPM
    unsigned long long* stat;  // [0] n_transformed, [1] n_spm, [2] n_skipped (zeroed by the caller)
};
hipError_t tk_launch_fim_cut(const TkFimArgs& a, int unit_bytes, hipStream_t s);       // everything but out_units
hipError_t tk_launch_fim_permute(const TkFimArgs& a, int unit_bytes, hipStream_t s);   // out_units (behind tk_launch_fim_cut); no unit: nothing is launched

// ---- masked-LM and span-corruption rows: a noise pass over encoded ids (tk_noise.hip) ----
#define TKN_TILE 4096u         /* input ids of a block's tile of the noise kernels: 4 rounds of 4 a thread */
#define TKN_ROUND 1024u        /* ids of one round of a block: TKY_BLOCK threads, 4 consecutive ids each */
#define TKN_SEED_BASE 0x4E4F4900u
#define TKN_SLOTS 64u          /* copies of every counter of a call: a block adds to copy blockIdx % TKN_SLOTS, the host adds them up */
#define TKN_STATS 4u           /* counters of a copy */
#define TKN_STAT_DROP (TKN_SLOTS * TKN_STATS)   /* the word behind the copies: a document drops a run */
struct TkNoiseArgs {
    const uint32_t* ids;       // [n_ids] packed token ids of all documents
    const uint64_t* offs;      // [n_docs + 1]
    const uint32_t* word_ids;  // [n_ids] or NULL (needed by TK_NOISE_UNIT_WORD)
    const uint8_t* sel;        // [n_ids] the caller's choice, or NULL: drawn
    uint64_t n_docs, n_ids;
    uint32_t s[4];             // s_k = h(seed, TKN_SEED_BASE + k)
    uint64_t start_q32, mask_q32, mask_random_q32;   // (the third: mask_q32 + random_q32)
    uint32_t unit, span_min, span_max;
    uint32_t mask_id, num_special, n_ordinary;   // S0; V - S0
    int32_t ignore;            // ignore_index
    // replace mode
    uint32_t* out_ids;         // [n_ids]
    int32_t* labels;           // [n_ids]
    uint8_t* selected;         // [n_ids]: replace mode: the output or NULL; spans mode: selected(i) in front of the drop (a work array)
    // spans mode
    uint32_t n_sentinels, sentinel_first, desc, final_id, split, joined;
    uint64_t n_tiles;          // ceil(n_ids / TKN_TILE)
    uint32_t *tile_sel, *tile_rs;          // [n_tiles] selected ids | run starts of the tile
    const uint64_t *tile_S, *tile_R;       // [n_tiles + 1] their exclusive scans
    uint32_t *doc_sel0, *doc_rs0;          // [n_docs] of a document that starts inside a tile: the tile's selected ids | run starts in front of it (else 0: zeroed by the caller)
    uint64_t *SB, *RB;         // [n_docs + 1] selected ids | run starts in front of the document
    uint32_t* KS;              // [n_docs] the document's selected ids behind the drop
    uint32_t *in_len, *tg_len; // [n_docs] the ids of inputs_d | targets_d
    const uint64_t *in_off, *tg_off;       // [n_docs + 1] their exclusive scans: input_offsets | target_offsets
    uint64_t n_inputs, n_targets;          // known behind the host read: nothing is written at or beyond them
    uint32_t *inputs, *targets, *joined_ids;
    uint64_t* joined_offs;     // [n_docs + 1]
    int32_t* joined_labels;
    // TKN_SLOTS copies of TKN_STATS counters -- replace: [0] n_selected, [1] n_masked, [2] n_random; spans: [0] n_selected behind
    // the drop, [1] n_runs, [2] n_runs_dropped -- and [TKN_STAT_DROP]: not 0 where a document drops a run (tk_launch_noise_docs;
    // tk_launch_noise_drop returns at once where it is 0).  Zeroed by the caller
    unsigned long long* stat;
};
hipError_t tk_launch_noise_replace(const TkNoiseArgs& a, hipStream_t s);   // out_ids, labels, selected, stat[0..2]; no id: nothing is launched
hipError_t tk_launch_noise_select(const TkNoiseArgs& a, hipStream_t s);    // spans mode: selected
hipError_t tk_launch_noise_count(const TkNoiseArgs& a, hipStream_t s);     // tile_sel, tile_rs, doc_sel0, doc_rs0
hipError_t tk_launch_noise_docs(const TkNoiseArgs& a, hipStream_t s);      // SB, RB, KS without a drop, stat[TKN_STAT_DROP] (behind the two tile scans)
hipError_t tk_launch_noise_drop(const TkNoiseArgs& a, hipStream_t s);      // KS of the documents with a dropped run
hipError_t tk_launch_noise_lens(const TkNoiseArgs& a, hipStream_t s);      // in_len, tg_len, stat[0..2]
hipError_t tk_launch_noise_fill(const TkNoiseArgs& a, hipStream_t s);      // the outputs (behind the two document scans and the host read)

// ---- audio: log-mel features and the splice of audio parts (tk_audio.hip) ----
#define TKA_BLOCK 256
#define TKA_FRAMES 64u         /* frames of a block's tile: two 32-frame MFMA tiles a wave */
#define TKA_ROUND_BINS 128u    /* bins of a round: 32 a wave */
struct TkaSegment {            // one segment, as the host lays it out (tk_audio_layout's arithmetic)
    uint64_t start;            // its first sample in the packed clips
    uint64_t valid;            // the samples of it the clip has; the rest, up to len, are zero padding that is never read
    uint64_t len;              // L: its samples with the padding (reflection is about L - 1)
    uint64_t out;              // its first element in the features: M * frame_off[s]
    uint32_t frames, pad;      // T_s
};
struct TkaTile { uint32_t seg, t0; };   // a block's tile: frames t0 .. t0 + TKA_FRAMES of segment seg
struct TkLogmelArgs {
    const float* samples;      // the clips back to back, unpadded
    const TkaSegment* segs;    // [n_segs]
    const TkaTile* tiles;      // [n_tiles]
    uint32_t n_tiles, n_segs;
    uint32_t W, H, F, M;       // window, hop, bins W / 2 + 1, mel filters
    const float* dft;          // [W][2 F]: tk_audio_tables.h
    const uint32_t *fb_first, *fb_count, *fb_start;   // [M]
    const float* fb_weights;
    float* out;                // the features
    uint32_t* seg_max;         // [n_segs] bit patterns of the largest max(mel, 1e-10) (zeroed by the caller); null with a fixed maximum
    float fixed_max;           // log_mel_max where seg_max is null
    uint32_t staged;           // the tile's samples go to LDS (set by the launcher: they fit)
    uint32_t lds_samples;      // floats of LDS for them (set by the launcher)
    // the clamp kernel
    const uint64_t* frame_off; // [n_segs + 1]
    uint64_t n_elems;          // M * frame_off[n_segs]
};
hipError_t tk_launch_logmel(const TkLogmelArgs& a, hipStream_t s);         // L = log10(max(mel, 1e-10)), or the feature with a fixed maximum; no tile: nothing is launched
hipError_t tk_launch_logmel_clamp(const TkLogmelArgs& a, hipStream_t s);   // (max(L, Lmax - 8) + 4) / 4 in place
struct TkSpliceArgs {
    const uint32_t* ids;       // [n_ids]
    const uint64_t* id_offs;   // [n_parts + 1]
    const uint32_t* part_tokens;   // [n_parts] copies of fill_id behind the part's ids
    uint64_t n_parts, n_ids;
    uint32_t fill_id;
    uint32_t* counts;          // [n_parts] the new lengths, clamped to 2^32 - 1 (tk_launch_splice_counts)
    const uint64_t* out_offs;  // [n_parts + 1] their exclusive scan
    uint32_t* out_ids;
    uint64_t n_out;
};
hipError_t tk_launch_splice_counts(const TkSpliceArgs& a, hipStream_t s);
hipError_t tk_launch_splice_fill(const TkSpliceArgs& a, hipStream_t s);    // n_out == 0: nothing is launched

// max document length over the deferred documents (atomicMax into *d_out, which must be zeroed)
hipError_t tk_launch_defer_maxlen(const uint32_t* defer_list, uint32_t n, const uint64_t* doc_offs, uint32_t* d_out,
                                  hipStream_t s);

// self-test of the wave primitives (DPP shifts, bpermute); writes 0 to *d_fail when all pass
hipError_t tk_launch_wave_selftest(uint32_t* d_fail, hipStream_t s);

#endif
