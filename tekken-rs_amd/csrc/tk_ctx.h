// tk_ctx.h -- the engine's context and what the host files of the C ABI (tk_capi*.cpp, tk_pipeline.cpp) share.  Internal: only
// they include it (tekkenizer.cpp sees tk_engine.h, tk_node.cpp the public C ABI).  Every buffer and handle of the context
// releases itself: `delete c` is the whole of tk_ctx_destroy.
#ifndef TK_CTX_H
#define TK_CTX_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/tekken_hip.h"
#include "tekkenizer.hpp"
#include "tk_counters.h"
#include "tk_engine.h"
#include "tk_kernels.h"
#include "tk_tables.h"

struct DevBuf {                    // device memory that only grows; movable (the pipelined entry swaps its output sets)
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~DevBuf() { release(); }
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        release();
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
    }
};

struct NoCopy { NoCopy() = default; NoCopy(const NoCopy&) = delete; NoCopy& operator=(const NoCopy&) = delete; };

template <class T> struct PinBuf : NoCopy {   // a pinned host block the context owns; reads as the T* it holds
    T* p = nullptr;
    ~PinBuf() { release(); }
    hipError_t alloc(size_t bytes, unsigned flags) { release(); return hipHostMalloc((void**)&p, bytes, flags); }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; }
    operator T*() const { return p; }
};

template <class H, hipError_t (*Destroy)(H)> struct Handle : NoCopy {   // a stream or an event; reads as the handle
    H h = nullptr;
    ~Handle() { if (h) (void)Destroy(h); }
    operator H() const { return h; }
};
typedef Handle<hipStream_t, hipStreamDestroy> Stream;
typedef Handle<hipEvent_t, hipEventDestroy> Event;

// Environment knobs read ONCE, when the context is created (read_knobs, tk_capi.cpp); tk_ctx_set_memo overrides the memo pair
struct TkKnobs {
    bool serial_tail = false;      // TK_TAIL=serial: the tail behind the merge kernels on the one stream (A / B, tests)
    bool no_decode_groups = false; // TK_DECODE_GROUPS=0: the per-document length pass (A / B and tests of the fall-back)
    uint32_t decode_group_limit = 0x7FFFFF00u;   // ids / text bytes of a group from which the call falls back (TK_DECODE_GROUP_LIMIT: tests)
    bool no_flat_long = false;     // TK_FLAT_LONG=0: pieces of 65..TKF_LONGCAP bytes hand their documents back (the round-1 behaviour; A / B and tests)
    bool no_flat_long128 = false;  // TK_FLAT_LONG128=0: every long-piece record takes the single-wave merge
    bool no_flat_cut = false;      // TK_FLAT_CUT=0: no cut decomposition (pieces of more than 256 bytes hand their documents back; A / B and tests)
    uint32_t long_min = 256;       // shortest piece (bytes) merged in rounds by a workgroup (TK_LONG_MIN; 0 = never)
    uint32_t long_lazy_mul = 0;    // TK_LONG_LAZY_MUL (0 = the default of tk_piece_is_long)
    uint32_t long_force = 0;       // TK_LONG_FORCE (tests): 1 = every long piece through the compacting rounds, 2 = through the lazy rounds
    uint32_t memo_log2 = 24;       // entries = 2^memo_log2 (32 bytes each: 512 MB of a 288 GB part), 0 = off; TK_MEMO_LOG2
    int memo_policy = 0;           // 0 adaptive (pause while the hit rate is low), 1 always on; TK_MEMO_POLICY=always
    int pipeline_forced = 0;       // TK_PIPELINE: 0 / 1 flat (default), 2 per-document kernels only
    int tail_fold = -1;            // TK_TAIL_FOLD: the folded scans of the flat tail: -1 by the two bounds below, 0 never, 1 wherever they can run (A / B, tests)
    // the folded forms cost (partial sums)^2 loads: the largest counts of partial sums at which they were not slower than the
    // three-kernel scans (profiles/tail_fold_time.json); TK_TAIL_FOLD_MISS_MAX / TK_TAIL_FOLD_DOC_MAX
    bool fold_merge = true;        // TK_TAIL_FOLD_MERGE=0: two merge kernels instead of tk_merge_all_kernel (the A / B that isolates it)
    uint32_t fold_miss_max = 1300; // miss side: block sums of 2048 entries (5 n_chunks entries)
    uint32_t fold_doc_max = 512;   // document side: blocks of 4096 documents
};
// ... and the ones read on EVERY call of the batch pipeline (call_knobs, tk_pipeline.cpp): tools set them between calls
struct TkCallKnobs {
    bool log = false;              // TK_DEBUG_LOG
    bool marks = false;            // TK_DEBUG_MARKS
    bool skip_pass2 = false;       // TK_DEBUG_SKIP_PASS2
    int memo_log_log2 = 0;         // TK_MEMO_LOG_LOG2 (8..24; 0: the default)
    int ablate = 0;                // TK_DEBUG_ABLATE (`make ablate` builds only)
};

// ---- the buffers of the passes behind encode, one struct per pass and one member of tk_ctx each.  The buffers of a pass are apart
// from those of every other pass and from every encode / decode buffer (a result stays valid through the calls of the other
// passes), only grow, and are allocated at the first call of the pass.
struct SpansBufs { DevBuf spans, err; };   // tk_token_spans_device: (start, end) per id, the error words
// the units pass and the annotation look-up (tk_spans_units.hip): the per-rank entries of tk_units_table.h (built at the first
// units call), the spans in the unit and their error words; the token ranges (next: written first, swapped in once the call is
// accepted) and their error words
struct UnitsBufs { DevBuf table, spans, err, range, next, range_err; };
// the dense layout (tk_dense.hip): the tensor, its mask, lengths and the two statistics words; the ragged ids / offsets / row
// lengths of the inverse
struct DenseBufs { DevBuf ids, mask, len, stat, rids, roffs, rlens; };
// the packed training rows (tk_seqpack.hip): the three tensors, cu_seqlens and the two statistics words; the work arrays
// (flags and their scans, the compacted starts, the scan workspace)
struct SeqpackBufs { DevBuf ids, pos, seg, cu, stat, flags, aflags, fpos, apos, starts, aligned, bsum; };
// the chat batches (tk_join.hip): the joined ids, their per-conversation offsets, labels, part indices and the statistics
// words; the work arrays (has-a-control-id and its scan, the parts' output starts and local indices, the scan workspace); the
// host entry's copies of part_ctrl / part_flags / conv_offsets
struct JoinBufs { DevBuf ids, offs, labels, pidx, stat, has, cb, start, plocal, bsum, in_ctrl, in_flags, in_conv; };
// the overlapping windows (tk_window.hip): the tensor, its mask and spans, the per-window arrays, doc_windows; the work arrays
// (dw_next: the scan that becomes doc_windows once the call is accepted, the counts, the scan workspace, the statistics words)
struct WindowBufs { DevBuf ids, mask, spans, len, doc, start, dw, dw_next, cnt, bsum, stat; };
// the boundary-aware chunks (tk_chunk.hip): the window pass's outputs and work arrays, and its own: cut_level, chunk_bytes and
// level_counts; the windows' records; the level bytes of tk_chunk_levels_device and the spans of the entries that encode first
struct ChunkBufs : WindowBufs {
    DevBuf cut, cbytes, lcounts, rec, lev, in_spans;
    Event ev[7];                   // the stages of the last chunk call (tk_last_chunk_ms), created at the first one
    float ms[3] = {0.f, 0.f, 0.f}; // levels | walks and scan | fill
};
// the sentence-pair rows (tk_pair.hip): the tensor, its mask, type ids, sequence ids and spans, the per-row arrays, pair_windows;
// the work arrays (pw_next: the scan that becomes pair_windows once the call is accepted, the counts, the scan workspace, the
// statistics words)
struct PairBufs { DevBuf ids, mask, type, seq, spans, len, pair, start, second, pw, pw_next, cnt, bsum, stat; };
// the whole-document rows (tk_rowfit.hip): the four tensors, cu_seqlens, doc_start and the statistics words; the work arrays
// (lengths and their scans, the jump tables, the row marks, the row openers, the per-document segment numbers, the per-row
// pad flags and their scan, the scan workspace)
struct RowfitBufs {
    DevBuf ids, lab, pos, seg, cu, dstart, stat, e, nz, E, nzp, ja, jb, row, open, segno, padf, padp, bsum;
    Event ev[5];                   // the stages of the last rowfit call (tk_last_rowfit_ms), created at the first one
    float ms[3] = {0.f, 0.f, 0.f};   // placement | fill kernel | cu_seqlens kernel
    float ms_chain = 0.f;          // the placement's part in front of the host read
};
// the regrouped documents (tk_regroup.hip): the ragged outputs, perm, the batch arrays and the statistics words; the work arrays
// (the kept flags, their scan and the kept documents, two key and three document buffers of the radix sort, its digit counts and
// their scan, the documents' lengths and source starts, the maximum pyramid, the jump tables, the batch marks, openers and row
// lengths, the scan workspace)
struct RegroupBufs {
    DevBuf ids, offs, lab, perm, bo, brl, stat, flag, fpos, kept, key[2], val[3], hist, hpos, len, src, pyr, ja, jb, row, open, bmax, bsum;
    Event ev[6];                   // the stages of the last regroup call (tk_last_regroup_ms), created at the first one
    float ms[4] = {0.f, 0.f, 0.f, 0.f};   // selection | sort | gather kernel | batches
};
// the word ids (tk_words.hip): word_ids, doc_words, word_first; the work arrays (the piece-start flags of the text, the
// per-document counts, the scan workspace, the error words; the text and offsets of a batch the one-launch small path encoded)
struct WordsBufs {
    DevBuf ids, dw, first, flags, cnt, bsum, err, text, toffs;
    Event ev[6];                   // the stages of the last words call (tk_last_words_ms), created at the first one
    float ms[4] = {0.f, 0.f, 0.f, 0.f};   // split launch | words kernel | scan | word_first
};
// the special-token strings parsed out of text (tk_specials.hip): the text without them, the part tables; the host copy of the
// context's strings and the byte trie over them (built at the first call behind tk_ctx_set_special_tokens: edges, term; str_of:
// the distinct string of every id, TKS_NONE for one that is empty or too long), the per-call eff words; the work arrays (the
// tile counts and their scan, the candidates, the jump tables, the marks, the matches, the match lengths and their scan, the
// matches' positions, the segments, the scan workspace, the statistics words); the host entry's copies of the text and its offsets
struct SpecialsBufs {
    DevBuf bytes, poffs, ctrl, conv, psrc;
    std::vector<uint8_t> h_blob;
    std::vector<uint32_t> h_offs, str_of, h_eff;
    uint32_t n_distinct = 0, edge_mask = 0;
    bool trie_ready = false;
    DevBuf edges, term, eff;
    DevBuf tcnt, tpos, cpos, clen, cid, cdoc, ja, jb, row, open, flen, remc, mpos, sout, ssrc, bsum, stat, in_bytes, in_offs;
    Event ev[8];                   // the stages of the last specials call (tk_last_specials_ms), created at the first one
    float ms[4] = {0.f, 0.f, 0.f, 0.f};   // candidates | chain | part tables | text compaction
};
// the fill-in-the-middle pass (tk_fim.hip): the units in the new order, the part tables, cuts and mode, the three counters; the
// host entry's copies of the text, its offsets and the caller's cuts
struct FimBufs {
    DevBuf units, poffs, ctrl, pflags, conv, psrc, cuts, mode, stat, in_units, in_offs, in_cuts;
    Event ev[3];                   // the stages of the last FIM call (tk_last_fim_ms), created at the first one
    float ms[2] = {0.f, 0.f};      // cut kernel | permute kernel
};
// the noise pass (tk_noise.hip): replace mode's ids, labels and selected bytes (spans mode: its work flags); spans mode's five
// outputs (the two split offsets are the document scans themselves) and joined_offsets; the statistics words; the work arrays
// (the tiles' counts and their scans, the documents' counts in front of them, kept ids and lengths, the scan workspace); the host
// entries' copies of a small batch's text and offsets
struct NoiseBufs {
    DevBuf ids, lab, sel, inputs, targets, joined, jlab, joffs, in_off, tg_off, stat;
    DevBuf tsel, trs, tS, tR, dsel0, drs0, SB, RB, KS, in_len, tg_len, bsum, text, toffs;
    Event ev[4];                   // the stages of the last noise call (tk_last_noise_ms), created at the first one
    float ms[3] = {0.f, 0.f, 0.f}; // selection | counts and scans | fill kernel
};

// lossy decode (tk_decode_lossy.hip).  The repair pass: the lossy text and its offsets, the tiles' counts and their scan, the
// per-document "has a replacement" flags, the two counters, the scan workspace.  The stream step: the step's text, its offsets
// (n_seqs + 1 words, and the two error words right behind them: ONE host read), the lengths, the counter; the host entry's copies of
// the state, the ids and their offsets.
struct DecodeLossyBufs {
    DevBuf bytes, offs, tcnt, toffs, flags, stat, bsum;
    DevBuf s_bytes, s_offs, s_lens, s_stat, s_bsum, s_state, s_in_ids, s_in_offs;
    Event ev[2];                   // around the repair pass of the last lossy call (tk_last_decode_lossy_ms), created at the first one
    float strict_ms = 0.f, repair_ms = 0.f;
    uint64_t n_replaced = 0, n_bad_docs = 0;
    uint32_t repair_launches = 0;  // kernels the last lossy call launched behind the strict pipeline (0: the fast path)
};

// the audio pass (tk_audio.hip).  The config and its device tables (tk_audio_set_config: the DFT matrix, the filter bank's runs);
// the log-mel outputs (features, frame_off, clip_seg), the segments, tiles and per-segment maxima, the host entry's copies of
// the samples and their offsets; the splice's outputs (ids, offsets) and its counts and scan workspace
struct AudioBufs {
    bool have_config = false;
    tk_audio_config cfg = {};
    uint32_t W = 0, F = 0, M = 0;
    DevBuf dft, fb_first, fb_count, fb_start, fb_weights;
    DevBuf feat, frame_off, clip_seg, segs, tiles, seg_max, in_samples, in_offs;
    DevBuf sp_ids, sp_offs, sp_cnt, sp_bsum;
    uint64_t n_splice_calls = 0;
    Event ev[3];                   // the stages of the last log-mel call (tk_last_logmel_ms), created at the first one
    float ms[2] = {0.f, 0.f};      // product kernel | clamp kernel
};

struct tk_ctx {
    int device = 0;
    std::mutex mu;
    std::string err;
    TkKnobs knobs;
    TkCallKnobs call;
    TkHostTables host;
    TkTablesView dview;
    // streams: the context's own; B: the tail of a batch (documents handed back by the flat kernel) beside the merge kernels;
    // s_in / s_out: the copy streams of tk_encode_batch_pipelined, created at its first call
    Stream stream, stream_b, s_in, s_out;
    Event ev[5];                   // [4]: behind the merge kernels (tk_last_merge_ms)
    Event ev_b[3];                 // flat kernel done (A) | list of handed-back documents on the host (B) | tail done (B)
    Event ev_in[2], ev_out[2];
    DevBuf t_uc1, t_uc2, t_key8, t_key, t_long, t_pair, t_pair2, t_pairf, t_blob, t_offs, t_spblob, t_spoffs, t_uc2a, t_uc2b;
    DevBuf t_key64;                // whole pieces of 17..64 bytes by the flat kernel's dword hash
    DevBuf t_cutk2, t_cutg3, t_ucbmp;   // the cut rule's bit maps, the class trie flattened for the BMP (tk_tables.cpp make_cut_tables)
    int pattern = 0;               // tk_ctx_set_pattern: 0 the reference's hard-coded pattern, 1 the JSON pattern (row f-3)
    bool have_specials = false;
    DevBuf dec_lens, dec_bytes, dec_offs, dec_bits, dec_err, dec_in_ids, dec_in_offs, dec_hi, dec_glens, dec_goffs;
    DevBuf t_inline, t_len8;   // decode: 16-byte inline entries and one-byte lengths by rank (built at the first decode / spans call)
    // the passes behind encode, one member each (the structs above tk_ctx)
    SpansBufs spans;
    UnitsBufs units;
    DenseBufs dense;
    SeqpackBufs seqpack;
    JoinBufs join;
    WindowBufs window;
    ChunkBufs chunk;
    PairBufs pair;
    RowfitBufs rowfit;
    RegroupBufs regroup;
    WordsBufs words;
    SpecialsBufs specials;
    FimBufs fim;
    NoiseBufs noise;
    DecodeLossyBufs lossy;
    AudioBufs audio;
    DevBuf staging, counts, out_ids, out_offs, block_sums, defer_list, scratch, in_bytes, in_offs, dbg;
    DevBuf counters;               // TKC_DEVICE_WORDS words: tk_counters.h
    PinBuf<uint32_t> h_pin;        // TKC_PIN_WORDS pinned host words: the per-batch device counters land here with ONE copy
    PinBuf<uint32_t> dbg_mark;     // mapped pinned memory, only with TK_DEBUG_MARKS
    DevBuf long_jobs;              // tk_long.hip: the long pieces of the long-list documents
    DevBuf long_list;              // pass 2 -> tk_long.hip: documents with a long piece that is not a vocabulary key
    // flat path (tk_flat.hip)
    DevBuf f_first, f_tmp, f_lstart, f_flags, f_todo, f_miss, f_mcnt, f_mpfx, f_wfirst, f_info, f_gsum;
    DevBuf f_long;                 // records of the pieces of 65..TKF_LONGCAP bytes
    DevBuf f_cut;                  // chunks left to the CUT instantiation (tk_flat_cut_kernel)
    DevBuf f_late;                 // documents a long-piece record flagged after the list of handed-back documents was made
    DevBuf scratch_rec;            // scratch of the long-piece record kernels (stream A; c->scratch belongs to the tail on stream B)
    void* long_ctl_ptr = nullptr;  // what the control words at TKC_LONG_CTL describe
    uint32_t long_ctl_cap = 0;
    void* cut_ctl_ptr = nullptr;   // what the control words at TKC_CUT_CTL describe
    bool use_flat = true;
    // diagnostics of the last call
    uint64_t n_flagged = 0, n_long_docs = 0;
    uint64_t n_round_docs = 0;     // documents the round-based kernel took
    uint64_t n_long_recs = 0;      // pieces of 65..TKF_LONGCAP bytes the flat path kept
    uint64_t n_cut_chunks = 0;     // regions that went through the CUT instantiation
    uint32_t host_syncs = 0;       // host waits of the last flat-pipeline call
    float pipeline_ms = 0.f, encode_ms = 0.f, merge_ms = 0.f;
    // pipelined ingestion (tk_encode_batch_pipelined): the second set of staging buffers
    DevBuf in_bytes2, in_offs2, out_ids2, out_offs2;
    PinBuf<uint64_t> h_offs_stage[2];   // slice-relative document offsets going up
    uint64_t h_offs_cap = 0;
    // small batches in one launch (tk_small_kernel): mapped pinned host buffers the kernel reads / writes directly
    PinBuf<uint8_t> hs_in;         // [TK_SMALL_MAX_BYTES] text | [TK_SMALL_MAX_DOCS + 1] u64 offsets
    PinBuf<uint32_t> hs_out;       // [TK_SMALL_MAX_BYTES + 2 * TK_SMALL_MAX_DOCS] ids | [TK_SMALL_MAX_DOCS + 1] u64 offsets | [4] status
    void* ds_in = nullptr, *ds_out = nullptr;   // the same buffers as the device sees them
    DevBuf s_offs;
    uint64_t n_small_calls = 0;    // calls served by the one-launch path (tk_last_stats_ex)
    bool small_ready = false;      // small_prepare() went through completely
    // memo of merged pieces (tk_hash.h MEMO; include/tekken_hip.h tk_ctx_set_memo)
    DevBuf t_memo, t_memo_log;
    uint32_t memo_have_log2 = 0;   // size of the table that is allocated (0: none yet)
    uint32_t memo_epoch = 0;       // calls that used the table so far
    uint32_t memo_low_streak = 0, memo_pause = 0;
    bool memo_active_last = false;
    uint64_t memo_hits_last = 0, memo_lookups_last = 0, memo_hits_total = 0, memo_lookups_total = 0;

    uint32_t* ctr(int word) const { return (uint32_t*)counters.p + word; }   // a word of the device counter block (TkCounter)
};

#define TK_SMALL_IDS_CAP (TK_SMALL_MAX_BYTES + 2 * TK_SMALL_MAX_DOCS)
#define TK_SMALL_OUT_OFFS_WORD (TK_SMALL_IDS_CAP)                          /* u32 index of the u64 offsets in hs_out (8-byte aligned) */
#define TK_SMALL_STATUS_WORD (TK_SMALL_OUT_OFFS_WORD + 2 * (TK_SMALL_MAX_DOCS + 1) + 2)

#define TK_HIP(ctx, call)                                                                          \
    do {                                                                                           \
        hipError_t _e = (call);                                                                    \
        if (_e != hipSuccess) { (ctx)->err = std::string(#call) + ": " + hipGetErrorString(_e); return TK_ERR_RUNTIME; } \
    } while (0)

// how every entry of the C ABI opens: a null context is refused, the context is locked for the call
#define TK_ENTRY(c)                                                                                \
    if (!(c)) return TK_ERR_INVALID_ARG;                                                           \
    std::lock_guard<std::mutex> lock((c)->mu)

// ---- what the files need from one another (every function below expects c->mu held and the device set) ----
#pragma GCC visibility push(hidden)
// tk_capi.cpp
int upload(tk_ctx* c, DevBuf& b, const void* src, size_t bytes);
// the checks that open an entry, in the order every entry had them: the batch limit, then the device.  (What a bad call reports
// first is behaviour: entries with a check between the two call the halves themselves.)
int check_n_docs(tk_ctx* c, uint64_t n_docs);
int enter_device(tk_ctx* c, uint64_t n_docs);
// Result copy-out: pinned blocks from the process-wide pool for n arrays (an array of 0 bytes gets a block too; dev == nullptr: the
// block alone; !selected -- an output the caller did not ask for --: no block, host stays null), the device -> host copies on
// c->stream, ONE wait.  On a failure every block is back in the pool, c->err is "hipHostMalloc failed" or
// "<what> copy failed: ..." and host[] is all null.
struct CopyOut { const void* dev; size_t bytes; void* host; bool selected = true; };
int pinned_blocks(tk_ctx* c, CopyOut* a, int n);
int copy_out(tk_ctx* c, CopyOut* a, int n, const char* what);
// ---- what the layout passes share (tk_capi_dense / _seqpack / _join / _window / _chunk / _pair / _rowfit / _regroup.cpp; tk_capi_layout.h is theirs alone) ----
#define TK_LAYOUT_MAX_ROW 0x7FFFFFFFull         /* a row of a tensor stays below 2^31 elements */
#define TK_LAYOUT_MAX_ELEMS (1ull << 36)        /* rows * row length: 256 GiB of int32, more than the part holds */
// how an entry with check flags opens: an unknown flag is refused first, then a null argument
int check_flags_and_args(tk_ctx* c, int checks, int known, bool null_arg);
// offs[0 .. n] = the exclusive prefix sums of counts[0 .. n) on s.  `workspace` is sized for it here, which allocates only where
// the caller has not reserved scan_workspace_bytes(n) with its other buffers, before its first launch
static inline size_t scan_workspace_bytes(uint64_t n) { return (n / 2048 + 4) * 8; }
int scan_u32(tk_ctx* c, DevBuf& workspace, const uint32_t* counts, uint64_t n, uint64_t* offs, hipStream_t s);
// tk_pipeline.cpp: the batch pipeline over text on the device; the ids end in c->out_ids, their offsets in c->out_offs
int run_pipeline(tk_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offs, uint64_t n_docs, uint64_t n_bytes, int add_bos,
                 int add_eos, hipStream_t s, uint64_t* n_ids);
// what every TkEncodeArgs of the context holds (per-document kernels over c->staging / c->counts, TKC_WORK / TKC_DEFERRED, no pattern)
TkEncodeArgs encode_args(tk_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offs, uint64_t n_docs, int add_bos, int add_eos);
// tk_capi_encode.cpp
int check_offsets(tk_ctx* c, const uint64_t* doc_offsets, uint64_t n_docs);
// TK_CHECK_OFFSETS / TK_CHECK_UTF8 over text on the device (checks != 0: one small kernel and one host wait each)
int check_text_device(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes, int checks, void* hip_stream);
int encode_device_checked(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_docs, uint64_t n_bytes, int add_bos,
                          int add_eos, int checks, void* hip_stream, void** d_ids, void** d_out_offsets, uint64_t* n_ids);
// Where the device copy of a host batch and of its result lives once encode_batch returns (the spans and dense passes read them):
// the context's staging buffers, or -- one-launch small path -- the mapped pinned buffers the small kernel read and wrote.
struct DevBatch {
    const uint8_t* bytes = nullptr; const uint64_t* doc_offs = nullptr;
    const uint32_t* ids = nullptr;  const uint64_t* id_offs = nullptr;
};
int encode_batch(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos, int add_eos,
                 int validate_utf8, tk_result* out, DevBatch* dev);
// tk_capi.cpp: encode_batch for a layout pass, which reads the ids where *dev says (the small path's are mapped pinned memory: the
// kernels read them there) and whose result does not hold the ragged ids: their host copy is freed, their number kept
int encode_batch_for_layout(tk_ctx* c, const uint8_t* bytes, const uint64_t* doc_offsets, uint64_t n_docs, int add_bos, int add_eos,
                            int validate_utf8, DevBatch* dev, uint64_t* n_ids);
// tk_capi_join.cpp: the body of tk_encode_parts_device_join (tk_capi_rowfit.cpp runs the rowfit pass behind it under one lock)
int encode_parts_device_join(tk_ctx* c, const void* d_bytes, const void* d_doc_offsets, uint64_t n_parts, uint64_t n_bytes,
                             const void* d_part_ctrl, const void* d_part_flags, const void* d_conv_offsets, uint64_t n_convs,
                             int checks, const tk_join_opts* opts, void* hip_stream, tk_join* out);
// ... and what it refuses before anything is on the device (tk_capi_specials.cpp and tk_capi_fim.cpp ask before they split the text)
int join_check_args(tk_ctx* c, uint64_t n_parts, uint64_t n_convs, const tk_join_opts* o);
// ... and the join itself over ids on the device (tk_capi_fim.cpp runs it behind the ids split under one lock)
int run_join(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t P, uint64_t n_ids, const uint32_t* d_ctrl,
             const uint32_t* d_pflags, const uint64_t* d_conv, uint64_t C, bool check_parts, const tk_join_opts* o, hipStream_t s,
             tk_join* out);
// tk_capi_words.cpp: the words pass over ids and text on the device (tk_capi_noise.cpp runs it between encode and the noise pass
// under one lock); checks: TK_WORDS_CHECK_ALIGNED or 0
int run_words(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t n_ids, const uint8_t* d_bytes,
              const uint64_t* d_doc_offs, uint64_t n_bytes, int checks, const tk_words_opts* o, hipStream_t s, tk_words* out, uint64_t* bad);
// tk_capi_decode.cpp: the decode kernels' tables (also what the spans kernel reads), built at the first call that needs them
int token_tables(tk_ctx* c);
// ... and the strict decode pipeline over ids on the device: the text ends in c->dec_bytes, its offsets in c->dec_offs, the run
// starts in c->dec_bits.  utf8_bad (the lossy entries): a run that is not valid UTF-8 is no error; the first document with one
// goes to *utf8_bad (~0: none), every other error is reported as without it
int run_decode(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t n_ids, int policy,
               hipStream_t s, uint64_t* n_bytes, uint64_t* bad_doc, uint64_t* utf8_bad = nullptr);
template <class A> static inline void token_args(const tk_ctx* c, A& a) {   // ... as the decode and spans kernels take them
    a.tok_blob = (const uint8_t*)c->t_blob.p; a.tok_offs = (const uint32_t*)c->t_offs.p;
    a.tok_inline = (const uint8_t*)c->t_inline.p; a.tok_len8 = (const uint8_t*)c->t_len8.p;
    a.n_ranks = c->host.n_ranks; a.num_special = c->host.num_special;
}
// tk_capi_spans.cpp: the spans pass over ids on the device into c->spans.spans, with the TK_SPANS_CHECK_* of `checks`
// (into: the buffer the spans go to instead -- the units pass with TK_UNIT_BYTE)
int run_spans(tk_ctx* c, const uint32_t* d_ids, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t n_ids, const uint64_t* d_doc_offs,
              const uint8_t* d_bytes, int checks, hipStream_t s, uint64_t* bad_doc, DevBuf* into = nullptr);
// tk_capi_spans.cpp: the document whose id range holds id index idx (error paths)
int doc_of_id(tk_ctx* c, const uint64_t* d_id_offs, uint64_t n_docs, uint64_t idx, uint64_t* out);
#pragma GCC visibility pop

#endif
