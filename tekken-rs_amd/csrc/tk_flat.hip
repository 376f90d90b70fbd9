// tk_flat.hip -- gfx950 kernels of the flat (chunk-per-wave) tokenization path, see tk_flat_impl.h.
//
//   tk_flat_firstdoc_kernel   per chunk: how many documents start below its loaded region
//   tk_flat_kernel            split + lookup of one region (64 x TKF_W bytes) per wave, ids chunk-dense
//   tk_flat_mode1_kernel      the same for tables built with the strong key hash; tk_flat_json_kernel: the split rules of the
//                             JSON pattern of tekken.json (opt-in); tk_flat_split_kernel: the per-byte
//                             piece-start flags of tk_split_batch compiled in (`make ablate`: the timing ablations too)
//   tk_merge_kernel           byte-pair merge of the queued pieces (2..16 bytes) that missed the vocabulary, one lane per piece
//   tk_merge_wide_kernel      the same for pieces of 17..64 bytes (32- and 64-entry LDS columns)
//   tk_flat_long_kernel       the records of pieces of 65..256 bytes: end of the piece where the chunk did not see it, whole-piece
//                             lookup; tk_flat_long128_kernel: 65..128 bytes, one lane per piece; tk_flat_long_coop_kernel:
//                             129..256 bytes, one wave per piece with the parts in registers
//   tk_flat_todo_kernel       flagged documents -> list for the per-document kernel
//   tk_flat_counts_kernel     ids per document from the chunk prefix sums and the document-start ranks
//   tk_flat_assemble_kernel   chunk-dense ids -> packed ids in document order with BOS / EOS
//                             (reference src/tekkenizer.rs:390-402)
//
// The bodies of firstdoc, wavefirst, todo, counts and assemble are in tk_flat_tail_impl.h (shared with the CPU wave emulator).
//
// Integer / byte work, no MFMA; roofline: HBM by the byte accounting of DESIGN.md, in practice VALU issue (section 6).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "tk_kernels.h"
#include "tk_wave_hip.h"
#include "tk_flat_impl.h"
#include "tk_flat_tail_impl.h"

#define TKF_BLOCK 256
#ifndef TKF_OCC
#define TKF_OCC __attribute__((amdgpu_waves_per_eu(7, 7)))  /* the LDS slices of 28 waves fill the CU: 7 waves per SIMD, <= 72 VGPRs */
#endif

__global__ __launch_bounds__(TKF_BLOCK) void tk_flat_firstdoc_kernel(const uint64_t* __restrict__ doc_offs, uint64_t n_docs,
                                                                      uint64_t n_chunks, uint32_t* __restrict__ first_doc,
                                                                      uint32_t* __restrict__ flags, uint32_t* __restrict__ holes,
                                                                      uint32_t* __restrict__ counters16) {
    tkf_firstdoc_body((uint64_t)blockIdx.x * TKF_BLOCK + threadIdx.x, doc_offs, n_docs, n_chunks, first_doc, flags, holes, counters16);
}

template <int DBG, int MODE, int PAT = 0, int MEMO = 1>
__device__ __forceinline__ void tk_flat_kernel_body(const TkFlatArgs& a, uint32_t* lds_all) {
    const int lane = wv_lane();
    // the wave number is wave-uniform: say so, and the chunk index and everything addressed by it stay in scalar registers
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t* lds = lds_all + wv * TKF_LDS_WORDS;
    tk_flat_init_lds(a, lds, lane);
    uint64_t c_begin = (uint64_t)blockIdx.x * (TKF_BLOCK / 64) + wv, c_end = a.n_chunks, c_step = (uint64_t)gridDim.x * (TKF_BLOCK / 64);
    if (gridDim.x >= 8) {
        // XCD-aware: blocks b and b + 8 share an XCD (and its L2), so the blocks of one residue class take ONE contiguous
        // eighth of the chunks -- neighbouring chunks share their halo bytes and the cache lines of the per-chunk /
        // per-document arrays they read and write.  (Placement is a speed matter only.)
        const uint64_t label = blockIdx.x & 7u, nb = (gridDim.x - label + 7u) / 8u;
        c_begin = a.n_chunks * label / 8 + (uint64_t)(blockIdx.x >> 3) * (TKF_BLOCK / 64) + wv;
        c_end = a.n_chunks * (label + 1) / 8;
        c_step = nb * (TKF_BLOCK / 64);
    }
    for (uint64_t c = c_begin; c < c_end; c += c_step) tk_flat_chunk<DBG, MODE, PAT, 0, MEMO>(a, c, lane, lds);
    if (MEMO) tk_flat_flush_memo_hits(a, lds, lane);
}

__global__ __launch_bounds__(TKF_BLOCK) TKF_OCC void tk_flat_kernel(TkFlatArgs a) {
    __shared__ uint32_t lds_all[(TKF_BLOCK / 64) * TKF_LDS_WORDS];
    tk_flat_kernel_body<0, 0, 0, 0>(a, lds_all);
}
// the same with the look-up in the memo of merged pieces (launched when the call uses the table: a.memo_tab != NULL)
__global__ __launch_bounds__(TKF_BLOCK) TKF_OCC void tk_flat_memo_kernel(TkFlatArgs a) {
    __shared__ uint32_t lds_all[(TKF_BLOCK / 64) * TKF_LDS_WORDS];
    tk_flat_kernel_body<0, 0, 0, 1>(a, lds_all);
}

// the tables were built with the strong key hash (mode 1: the cheap one could not place the vocabulary)
__global__ __launch_bounds__(TKF_BLOCK) TKF_OCC void tk_flat_mode1_kernel(TkFlatArgs a) {
    __shared__ uint32_t lds_all[(TKF_BLOCK / 64) * TKF_LDS_WORDS];
    tk_flat_kernel_body<0, 1>(a, lds_all);
}

// opt-in (row f-3): the split rules of the JSON pattern of Mistral's tekken.json
__global__ __launch_bounds__(TKF_BLOCK) TKF_OCC void tk_flat_json_kernel(TkFlatArgs a) {
    __shared__ uint32_t lds_all[(TKF_BLOCK / 64) * TKF_LDS_WORDS];
    if (a.t.key_hash_mode == 0u) tk_flat_kernel_body<0, 0, 1>(a, lds_all);
    else tk_flat_kernel_body<0, 1, 1>(a, lds_all);
}

// the same kernels with the per-byte piece-start flags of tk_split_batch compiled in (and, in a `make ablate` build, TK_DEBUG_ABLATE)
__global__ __launch_bounds__(TKF_BLOCK) TKF_OCC void tk_flat_split_kernel(TkFlatArgs a) {
    __shared__ uint32_t lds_all[(TKF_BLOCK / 64) * TKF_LDS_WORDS];
    if (a.t.key_hash_mode == 0u) tk_flat_kernel_body<1, 0>(a, lds_all);
    else tk_flat_kernel_body<1, 1>(a, lds_all);
}

// The chunks tk_flat_kernel left alone because they hold a piece of more than 64 bytes (a.cut_list): the same chunk work
// with the CUT step -- such pieces are cut into fragments wherever no vocabulary token can span the boundary
// (tk_flat_chunk_impl.h step 4b), so that a 32 KiB letter run becomes thousands of independent short merges instead of one chain
// and its document stays on the flat path.  Persistent waves over the list; the count never leaves the device.
template <int DBG>
__device__ __forceinline__ void tk_flat_cut_body(const TkFlatArgs& a, uint32_t* lds_all) {
    const uint32_t n = *a.cut_count;
    if (n == 0u) return;                                     // (grid-uniform)
    const int lane = wv_lane();
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t* lds = lds_all + wv * TKF_LDS_WORDS_CUT;
    tk_flat_init_lds(a, lds, lane);
    const uint64_t n_waves = (uint64_t)gridDim.x * (TKF_BLOCK / 64);
    for (uint64_t i = (uint64_t)blockIdx.x * (TKF_BLOCK / 64) + wv; i < n; i += n_waves) {
        const uint64_t c = (uint64_t)__builtin_amdgcn_readfirstlane((int)a.cut_list[i]);
        if (a.t.key_hash_mode == 0u) tk_flat_chunk<DBG, 0, 0, 1>(a, c, lane, lds);
        else tk_flat_chunk<DBG, 1, 0, 1>(a, c, lane, lds);
    }
    tk_flat_flush_memo_hits(a, lds, lane);
}
__global__ __launch_bounds__(TKF_BLOCK) void tk_flat_cut_kernel(TkFlatArgs a) {
    __shared__ uint32_t lds_all[(TKF_BLOCK / 64) * TKF_LDS_WORDS_CUT];
    tk_flat_cut_body<0>(a, lds_all);
}
__global__ __launch_bounds__(TKF_BLOCK) void tk_flat_cut_split_kernel(TkFlatArgs a) {
    __shared__ uint32_t lds_all[(TKF_BLOCK / 64) * TKF_LDS_WORDS_CUT];
    tk_flat_cut_body<1>(a, lds_all);
}

// which sub-queue holds the first item of every merge wave (tkf_wavefirst_body: thread e owns sub-queue e)
__global__ __launch_bounds__(TKF_BLOCK) void tk_merge_wavefirst_kernel(const uint64_t* __restrict__ prefix, uint64_t n_chunks,
                                                                        uint32_t* __restrict__ wave_first,
                                                                        uint32_t* __restrict__ wave_first_wide,
                                                                        uint32_t* __restrict__ narrow_left_out) {
    tkf_wavefirst_body((uint64_t)blockIdx.x * TKF_BLOCK + threadIdx.x, prefix, n_chunks, wave_first, wave_first_wide, narrow_left_out);
}

// persistent waves: groups of 64 queued pieces strided over the grid (the host does not know how many there are).
// Every block keeps the PAIR filter (tk_hash.h) in LDS: a probe whose filter bit is clear issues no gather.
template <int THREADS, uint32_t WORDS = TK_PAIRF_WORDS>
TK_DEV void tk_merge_load_filter(const TkFlatArgs& a, uint32_t* filt) {
    const tk_u32x4* src = reinterpret_cast<const tk_u32x4*>(a.t.pair_filter);
    for (uint32_t i = threadIdx.x; i < WORDS / 4; i += THREADS) reinterpret_cast<tk_u32x4*>(filt)[i] = src[i];
    __syncthreads();
}

// LDS per block: the narrow classes keep the PAIR filter (32 KB) in front of every wave's columns (tk_merge_lds: 8 KB); the wide
// classes spend all of the LDS on columns (10 KB per wave in the compact layout): 16 waves without the filter beat 12 with it
// (mixed shape, same box: 2.47 against 2.63 ms; 8 waves in the old layout: 3.08).  One block per CU.
#ifndef TKM_BLOCK
#define TKM_BLOCK 1024       /* 16 waves (the largest block there is): 32 KB + 16 x 8 KB = 160 KB */
#endif
#ifndef TKM_WIDE_BLOCK
#define TKM_WIDE_BLOCK 1024  /* 16 waves x 10 KB = 160 KB */
#endif
#ifndef TKM_FILTER
#define TKM_FILTER 1
#endif
#define TKM_FWORDS (TKM_FILTER ? TK_PAIRF_WORDS : 0u)
#define TKM_LDS_BYTES ((TKM_FWORDS + (TKM_BLOCK / 64) * TKM_LDS_WORDS(16)) * 4)
#ifndef TKM_WIDE_FILTER
#define TKM_WIDE_FILTER 0
#endif
#define TKM_WIDE_FWORDS (TKM_WIDE_FILTER ? TK_PAIRF_WORDS : 0u)
#define TKM_WIDE_LDS_BYTES ((TKM_WIDE_FWORDS + (TKM_WIDE_BLOCK / 64) * TKM_LDS_WORDS(32)) * 4)
// The narrow classes (2..16 bytes): groups of 64 of the first `total` queued pieces, strided over the grid's waves.  LOG: what they merge into goes to
// this wave's stretch of the memo log -- two loops, so that the log record stays in registers (a pointer that is its address or null: 24 bytes of scratch).
template <bool LOG>
__device__ __forceinline__ void tk_merge_narrow_loop(const TkFlatArgs& a, uint64_t wave, uint64_t n_waves, uint64_t total, uint32_t* mlds,
                                                     const uint32_t* filt) {
    if (LOG) {
        TkMemoLog ml;
        ml.base = a.memo_log + wave * a.memo_log_per_wave;
        ml.n = 0u;
        ml.cap = wave < a.memo_log_waves ? a.memo_log_per_wave : 0u;
        for (uint64_t w = wave; w * 64 < total; w += n_waves) tk_merge_wave<false>(a, w, wv_lane(), mlds, filt, &ml);
        if (wave < a.memo_log_waves && wv_lane() == 0) a.memo_log_counts[wave] = ml.n;
    } else {
        for (uint64_t w = wave; w * 64 < total; w += n_waves) tk_merge_wave<false>(a, w, wv_lane(), mlds, filt, nullptr);
    }
}
// The wide classes: w2 groups of 64 pieces of 17..32 bytes, then w3 of 33..64 bytes (wv: the wave's number in its block, scalar in every caller)
__device__ __forceinline__ void tk_merge_wide_loops(const TkFlatArgs& a, uint32_t wv, uint64_t wave, uint64_t n_waves, uint64_t w2, uint64_t w3,
                                                    uint32_t* mlds, const uint32_t* filt) {
    for (uint64_t w = wave; w < w2; w += n_waves) tk_merge_wave<true>(a, w, wv_lane(), mlds, filt);
    if (w3 == 0) return;                                     // (grid-uniform)
    // the class 33..64 bytes needs 64-entry columns: every second wave takes it, with its neighbour's LDS
    __syncthreads();
    if ((wv & 1u) == 0u) {
        const uint64_t ew = wave >> 1, n_ew = n_waves >> 1;
        for (uint64_t w = ew; w < w3; w += n_ew) tk_merge_wave_long3(a, w, wv_lane(), mlds, filt);
    }
}

__global__ __launch_bounds__(TKM_BLOCK) void tk_merge_kernel(TkFlatArgs a) {   // pieces of 2..16 bytes
    extern __shared__ __attribute__((aligned(16))) uint32_t wlds[];
    if (TKM_FILTER) tk_merge_load_filter<TKM_BLOCK, TK_PAIRF_WORDS>(a, wlds);
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (wave-uniform: say so, as in tk_merge_all_kernel)
    const uint64_t wave = (uint64_t)blockIdx.x * (TKM_BLOCK / 64) + wv;
    const uint64_t n_waves = (uint64_t)gridDim.x * (TKM_BLOCK / 64);
    const uint64_t total = a.miss_prefix[2 * a.n_chunks];
    uint32_t* mlds = wlds + TKM_FWORDS + wv * TKM_LDS_WORDS(16);
    if (a.memo_log) tk_merge_narrow_loop<true>(a, wave, n_waves, total, mlds, TKM_FILTER ? wlds : nullptr);   // (grid-uniform)
    else tk_merge_narrow_loop<false>(a, wave, n_waves, total, mlds, TKM_FILTER ? wlds : nullptr);
}

// the log of the merge kernel's new memo entries into the table (tk_memo_commit_one; the slots were claimed where the records were written)
__global__ __launch_bounds__(TKF_BLOCK) void tk_memo_commit_kernel(tk_memo_entry* __restrict__ tab, const tk_memo_entry* __restrict__ log,
                                                                    const uint32_t* __restrict__ counts, uint32_t per_wave, uint32_t n_waves,
                                                                    uint32_t key_hash_mode, uint32_t mask) {
    const uint32_t n = per_wave * n_waves;
    for (uint32_t i = blockIdx.x * TKF_BLOCK + threadIdx.x; i < n; i += gridDim.x * TKF_BLOCK)
        if (tk_memo_log_live(counts, per_wave, i)) tk_memo_commit_one(tab, log, i, key_hash_mode, mask);
}

__global__ __launch_bounds__(TKM_WIDE_BLOCK) void tk_merge_wide_kernel(TkFlatArgs a) {   // pieces of 17..64 bytes
    extern __shared__ __attribute__((aligned(16))) uint32_t wlds[];
    if (TKM_WIDE_FILTER) tk_merge_load_filter<TKM_WIDE_BLOCK, TKM_WIDE_FWORDS>(a, wlds);
    const uint32_t* wfilt = TKM_WIDE_FILTER ? wlds : nullptr;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (wave-uniform: say so, as in the other two)
    const uint64_t wave = (uint64_t)blockIdx.x * (TKM_WIDE_BLOCK / 64) + wv;
    const uint64_t n_waves = (uint64_t)gridDim.x * (TKM_WIDE_BLOCK / 64);
    const uint64_t n2 = a.miss_prefix[3 * a.n_chunks] - a.miss_prefix[2 * a.n_chunks];   // pieces of 17..32 bytes: 64 per wave
    const uint64_t n3 = a.miss_prefix[4 * a.n_chunks] - a.miss_prefix[3 * a.n_chunks];   // pieces of 33..64 bytes: 64 per wave
    const uint64_t w2 = (n2 + 63) / 64, w3 = (n3 + 63) / 64;
    tk_merge_wide_loops(a, wv, wave, n_waves, w2, w3, wlds + TKM_WIDE_FWORDS + wv * TKM_LDS_WORDS(32), wfilt);
}

// Both of the above in ONE launch (the folded tail): a block runs tk_merge_kernel's narrow loop, and then -- only if the wide
// classes hold anything, which on ordinary text they do not -- passes a barrier and runs tk_merge_wide_kernel's loops on the same
// 160 KB of LDS (the filter and the narrow columns are dead by then).  Same wave numbering, same memo log.  A block starts on its
// wide items as soon as ITS narrow ones are done.  (The two memo cases: tk_merge_narrow_loop.)
#define TKM_ALL_LDS_BYTES (TKM_LDS_BYTES > TKM_WIDE_LDS_BYTES ? TKM_LDS_BYTES : TKM_WIDE_LDS_BYTES)
__global__ __launch_bounds__(TKM_BLOCK) void tk_merge_all_kernel(TkFlatArgs a) {
    static_assert(TKM_BLOCK == TKM_WIDE_BLOCK && !TKM_WIDE_FILTER, "one block shape for both halves; the wide half reuses the filter's LDS");
    extern __shared__ __attribute__((aligned(16))) uint32_t wlds[];
    if (TKM_FILTER) tk_merge_load_filter<TKM_BLOCK, TK_PAIRF_WORDS>(a, wlds);
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t wave = (uint64_t)blockIdx.x * (TKM_BLOCK / 64) + wv;
    const uint64_t n_waves = (uint64_t)gridDim.x * (TKM_BLOCK / 64);
    const uint64_t p2 = a.miss_prefix[2 * a.n_chunks], p3 = a.miss_prefix[3 * a.n_chunks], p4 = a.miss_prefix[4 * a.n_chunks];
    {
        uint32_t* mlds = wlds + TKM_FWORDS + wv * TKM_LDS_WORDS(16);
        if (a.memo_log) tk_merge_narrow_loop<true>(a, wave, n_waves, p2, mlds, TKM_FILTER ? wlds : nullptr);   // (grid-uniform)
        else tk_merge_narrow_loop<false>(a, wave, n_waves, p2, mlds, TKM_FILTER ? wlds : nullptr);
    }
    if (p4 == p2) return;                                    // (grid-uniform: every thread of a block passes the barrier or none does)
    __syncthreads();
    const uint64_t w2 = (p3 - p2 + 63) / 64, w3 = (p4 - p3 + 63) / 64;   // pieces of 17..32 / 33..64 bytes: 64 per wave
    tk_merge_wide_loops(a, wv, wave, n_waves, w2, w3, wlds + wv * TKM_LDS_WORDS(32), nullptr);
}

// flagged documents -> list; the longest of them (it sizes the scratch of the piece-by-piece pass) -> *maxlen
__global__ __launch_bounds__(TKF_BLOCK) void tk_flat_todo_kernel(const uint32_t* __restrict__ flags, const uint64_t* __restrict__ doc_offs,
                                                                  uint64_t n_docs, uint32_t* __restrict__ todo,
                                                                  uint32_t* __restrict__ n_todo, uint32_t* __restrict__ maxlen) {
    tkf_todo_body((uint64_t)blockIdx.x * TKF_BLOCK + threadIdx.x, wv_lane(), flags, doc_offs, n_docs, todo, n_todo, maxlen);
}

// ids per document and the assembly's 16-byte record (TkFlatDocInfo): tkf_counts_body
__global__ __launch_bounds__(TKF_BLOCK) void tk_flat_counts_kernel(const uint64_t* __restrict__ doc_offs, uint64_t n_docs,
                                                                    uint64_t n_bytes, uint64_t n_chunks,
                                                                    const uint64_t* __restrict__ P,
                                                                    const uint32_t* __restrict__ lstart,
                                                                    const uint32_t* __restrict__ flags,
                                                                    const uint32_t* __restrict__ holes, uint32_t extra,
                                                                    uint32_t* __restrict__ counts,
                                                                    TkFlatDocInfo* __restrict__ info, int final_pass,
                                                                    uint32_t* __restrict__ n_flagged) {
    tkf_counts_body((uint64_t)blockIdx.x * TKF_BLOCK + threadIdx.x, wv_lane(), doc_offs, n_docs, n_bytes, n_chunks, P, lstart, flags, holes,
                    extra, counts, info, final_pass, n_flagged);
}

// one wave per 64 consecutive documents, strided over the grid (tkf_assemble_waves)
__global__ __launch_bounds__(TKF_BLOCK) void tk_flat_assemble_kernel(TkFlatAssembleArgs a) {
    tkf_assemble_waves(a, (uint64_t)blockIdx.x * (TKF_BLOCK / 64) + (threadIdx.x >> 6), (uint64_t)gridDim.x * (TKF_BLOCK / 64), wv_lane());
}

// ---- the folded tail (tk_flat_tail_impl.h: every consumer adds up the few partial sums below it itself) ----
// miss side: raw block sums -> miss_prefix, wave_first, wave_first_wide, TKC_NARROW_LEFT; one wave per 512 entries
__global__ __launch_bounds__(TKF_BLOCK) void tk_fold_apply_kernel(const uint32_t* __restrict__ counts, uint64_t n, uint64_t n_chunks,
                                                                   const uint64_t* __restrict__ block_sums, uint64_t* __restrict__ prefix,
                                                                   uint32_t* __restrict__ wave_first, uint32_t* __restrict__ wave_first_wide,
                                                                   uint32_t* __restrict__ narrow_left_out) {
    tkf_fold_apply_wave((uint64_t)blockIdx.x * (TKF_BLOCK / 64) + (threadIdx.x >> 6), wv_lane(), counts, n, n_chunks, block_sums, prefix,
                        wave_first, wave_first_wide, narrow_left_out);
}

// document side: tkf_counts_body, the sums of every group of 64 documents and of the block's 4096
#define TKF_FOLD_COUNTS_BLOCK (64u * (TKF_FOLD_DOC_BLOCK / (64u * TKF_FOLD_GROUPS)))   /* 16 waves */
__global__ __launch_bounds__(TKF_FOLD_COUNTS_BLOCK) void tk_flat_counts_sums_kernel(const uint64_t* __restrict__ doc_offs, uint64_t n_docs,
                                                                                     uint64_t n_bytes, uint64_t n_chunks,
                                                                                     const uint64_t* __restrict__ P,
                                                                                     const uint32_t* __restrict__ lstart,
                                                                                     const uint32_t* __restrict__ flags,
                                                                                     const uint32_t* __restrict__ holes, uint32_t extra,
                                                                                     uint32_t* __restrict__ counts,
                                                                                     TkFlatDocInfo* __restrict__ info, int final_pass,
                                                                                     uint32_t* __restrict__ n_flagged,
                                                                                     uint64_t* __restrict__ group_sums,
                                                                                     uint64_t* __restrict__ doc_block_sums) {
    __shared__ uint64_t wsum[TKF_FOLD_COUNTS_BLOCK / 64];
    const uint32_t wv = threadIdx.x >> 6;
    const uint64_t s = tkf_counts_sums_wave((uint64_t)blockIdx.x * (TKF_FOLD_COUNTS_BLOCK / 64) + wv, wv_lane(), doc_offs, n_docs, n_bytes,
                                            n_chunks, P, lstart, flags, holes, extra, counts, info, final_pass, n_flagged, group_sums);
    if (wv_lane() == 0) wsum[wv] = s;
    __syncthreads();                                         // (every thread of the block gets here)
    if (threadIdx.x == 0) {
        uint64_t t = 0;
        for (uint32_t w = 0; w < TKF_FOLD_COUNTS_BLOCK / 64; ++w) t += wsum[w];
        doc_block_sums[blockIdx.x] = t;
    }
}

// document side: one wave per 64 consecutive documents, output offsets made on the way (tkf_assemble_fold_waves)
__global__ __launch_bounds__(TKF_BLOCK) void tk_flat_assemble_fold_kernel(TkFlatAssembleArgs a, const uint32_t* __restrict__ counts,
                                                                           const uint64_t* __restrict__ group_sums,
                                                                           const uint64_t* __restrict__ doc_block_sums,
                                                                           uint64_t* __restrict__ out_offs) {
    tkf_assemble_fold_waves(a, counts, group_sums, doc_block_sums, out_offs, (uint64_t)blockIdx.x * (TKF_BLOCK / 64) + (threadIdx.x >> 6),
                            (uint64_t)gridDim.x * (TKF_BLOCK / 64), wv_lane());
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
static uint32_t tkf_blocks(uint64_t n_threads) { return (uint32_t)((n_threads + TKF_BLOCK - 1) / TKF_BLOCK); }

hipError_t tk_launch_flat_firstdoc(const uint64_t* doc_offs, uint64_t n_docs, uint64_t n_chunks, uint32_t* first_doc,
                                   uint32_t* flags, uint32_t* holes, uint32_t* counters16, hipStream_t s) {
    // (always launched: it also clears flags / holes [n_docs + 1] and the counters)
    hipLaunchKernelGGL(tk_flat_firstdoc_kernel, dim3(tkf_blocks(n_docs + 32)), dim3(TKF_BLOCK), 0, s, doc_offs, n_docs,
                       n_chunks, first_doc, flags, holes, counters16);
    return hipGetLastError();
}

hipError_t tk_launch_flat(const TkFlatArgs& a, hipStream_t s) {
    if (a.n_chunks == 0) return hipSuccess;
    uint64_t blocks = (a.n_chunks + (TKF_BLOCK / 64) - 1) / (TKF_BLOCK / 64);
    // persistent waves, chunks strided over them: exactly the blocks that are resident at once, so that no partially
    // filled last round of blocks trails behind
    // (per device, like the merge grids below: a process may hold contexts on several GPUs)
    static uint64_t cap_dev[64] = {0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    uint64_t& cap = cap_dev[dev & 63];
    if (cap == 0) {
        int cus = 256;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        int per_cu = 0;   // resident blocks per CU: 8 (16 bytes per lane, 8 waves per SIMD) or 7 (32 bytes per lane: LDS)
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, tk_flat_kernel, TKF_BLOCK, 0) != hipSuccess || per_cu <= 0) per_cu = 4;
        cap = (uint64_t)cus * (uint64_t)per_cu;
        if (const char* e = getenv("TK_FLAT_BLOCKS")) cap = (uint64_t)atoll(e);
        if (cap == 0) cap = 1280;
    }
    if (blocks > cap) blocks = cap;
    if (a.pattern == 1) hipLaunchKernelGGL(tk_flat_json_kernel, dim3((uint32_t)blocks), dim3(TKF_BLOCK), 0, s, a);
    else if (a.dbg_ablate || a.dbg_starts) hipLaunchKernelGGL(tk_flat_split_kernel, dim3((uint32_t)blocks), dim3(TKF_BLOCK), 0, s, a);
    else if (a.t.key_hash_mode == 0u && a.memo_tab && a.memo_probe) hipLaunchKernelGGL(tk_flat_memo_kernel, dim3((uint32_t)blocks), dim3(TKF_BLOCK), 0, s, a);
    else if (a.t.key_hash_mode == 0u) hipLaunchKernelGGL(tk_flat_kernel, dim3((uint32_t)blocks), dim3(TKF_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(tk_flat_mode1_kernel, dim3((uint32_t)blocks), dim3(TKF_BLOCK), 0, s, a);
    if (a.cut_list && a.pattern == 0) {
        // the chunks with a piece of more than 64 bytes (none on ordinary text: the blocks read a zero and leave -- two blocks
        // per CU, not the seven of the flat kernel: dispatching 1 792 blocks that do nothing took 10 us of every C2 step; the
        // 14 k listed regions of the 4 M-document Zipf shape are seven per wave instead of two)
        const uint64_t cblocks = blocks > cap / 7 * 2 && cap >= 7 ? cap / 7 * 2 : blocks;
        if (a.dbg_ablate || a.dbg_starts) hipLaunchKernelGGL(tk_flat_cut_split_kernel, dim3((uint32_t)cblocks), dim3(TKF_BLOCK), 0, s, a);
        else hipLaunchKernelGGL(tk_flat_cut_kernel, dim3((uint32_t)cblocks), dim3(TKF_BLOCK), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t tk_launch_merge_wavefirst(const uint64_t* prefix, uint64_t n_chunks, uint32_t* wave_first, uint32_t* wave_first_wide,
                                     uint32_t* narrow_left_out, hipStream_t s) {
    if (n_chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_merge_wavefirst_kernel, dim3(tkf_blocks(4 * n_chunks)), dim3(TKF_BLOCK), 0, s, prefix, n_chunks, wave_first,
                       wave_first_wide, narrow_left_out);
    return hipGetLastError();
}

// the two merge kernels: wave_first / wave_first_wide / TKC_NARROW_LEFT are there already (tk_launch_merge_wavefirst, or the folded apply)
hipError_t tk_launch_merge_kernels(const TkFlatArgs& a, hipStream_t s) {
    if (a.n_chunks == 0) return hipSuccess;
    // persistent grids (the number of queued pieces stays on the device): the blocks that are resident at once -- each
    // one copies the PAIR filter into its LDS first -- and never more than the sub-queues could fill
    // (per device: a process may hold contexts on several GPUs, and the LDS opt-in is a per-device function attribute;
    // two threads racing through the first call on a device compute the same values)
    static uint64_t res1_dev[64] = {0}, res2_dev[64] = {0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    uint64_t& res1 = res1_dev[dev & 63];
    uint64_t& res2 = res2_dev[dev & 63];
    if (res1 == 0) {
        int cus = 256, p1 = 0, p2 = 0;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(tk_merge_wide_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                TKM_WIDE_LDS_BYTES) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void*>(tk_merge_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                TKM_LDS_BYTES) != hipSuccess)
            return hipErrorInvalidValue;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&p1, tk_merge_kernel, TKM_BLOCK, TKM_LDS_BYTES) != hipSuccess || p1 <= 0) p1 = 1;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&p2, tk_merge_wide_kernel, TKM_WIDE_BLOCK, TKM_WIDE_LDS_BYTES) != hipSuccess || p2 <= 0) p2 = 1;
        res2 = (uint64_t)cus * (uint64_t)p2;
        res1 = (uint64_t)cus * (uint64_t)p1;
    }
    uint64_t b1 = (a.n_chunks * 4 + TKM_BLOCK / 64 - 1) / (TKM_BLOCK / 64), b2 = (a.n_chunks + TKM_WIDE_BLOCK / 64 - 1) / (TKM_WIDE_BLOCK / 64);
    if (b1 > res1) b1 = res1;
    if (b2 > res2) b2 = res2;
    // (the memo log is cut into one stretch per wave of THIS grid; a grid with more waves than the log was sized for logs nothing
    // from the surplus waves)
    hipLaunchKernelGGL(tk_merge_kernel, dim3((uint32_t)b1), dim3(TKM_BLOCK), TKM_LDS_BYTES, s, a);
    hipLaunchKernelGGL(tk_merge_wide_kernel, dim3((uint32_t)b2), dim3(TKM_WIDE_BLOCK), TKM_WIDE_LDS_BYTES, s, a);
    if (a.memo_tab && a.memo_log) {
        hipLaunchKernelGGL(tk_memo_commit_kernel, dim3(1024), dim3(TKF_BLOCK), 0, s, a.memo_tab, a.memo_log, a.memo_log_counts, a.memo_log_per_wave, a.memo_log_waves, a.t.key_hash_mode, a.memo_mask);
    }
    return hipGetLastError();
}

// tk_launch_merge_kernels with the two merge kernels in one launch (tk_merge_all_kernel); the memo's commit kernel behind it
hipError_t tk_launch_merge_all(const TkFlatArgs& a, hipStream_t s) {
    if (a.n_chunks == 0) return hipSuccess;
    static uint64_t res_dev[64] = {0};   // (per device, like tk_launch_merge_kernels)
    int dev = 0;
    (void)hipGetDevice(&dev);
    uint64_t& res = res_dev[dev & 63];
    if (res == 0) {
        int cus = 256, p = 0;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(tk_merge_all_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                TKM_ALL_LDS_BYTES) != hipSuccess)
            return hipErrorInvalidValue;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&p, tk_merge_all_kernel, TKM_BLOCK, TKM_ALL_LDS_BYTES) != hipSuccess || p <= 0) p = 1;
        res = (uint64_t)cus * (uint64_t)p;
    }
    uint64_t b = (a.n_chunks * 4 + TKM_BLOCK / 64 - 1) / (TKM_BLOCK / 64);
    if (b > res) b = res;
    hipLaunchKernelGGL(tk_merge_all_kernel, dim3((uint32_t)b), dim3(TKM_BLOCK), TKM_ALL_LDS_BYTES, s, a);
    if (a.memo_tab && a.memo_log) {
        hipLaunchKernelGGL(tk_memo_commit_kernel, dim3(1024), dim3(TKF_BLOCK), 0, s, a.memo_tab, a.memo_log, a.memo_log_counts, a.memo_log_per_wave, a.memo_log_waves, a.t.key_hash_mode, a.memo_mask);
    }
    return hipGetLastError();
}

// Pieces of 65..TKF_LONGCAP bytes (tk_flat_chunk_impl.h step 6): one wave per record -- the end of the piece where the chunk did
// not see it (sequential matcher), whole-piece lookup, the single-wave merge; ids + holes into the slots the chunk
// reserved, the document's hole count like the merge kernels.  Launched only when the flat kernel wrote records.
__global__ __launch_bounds__(256) void tk_flat_long_kernel(TkFlatArgs a, uint32_t* work_counter, uint32_t* scratch, uint32_t scratch_words) {
    const int lane = wv_lane();
    const TkPolyPow pw = tk_poly_pow(a.t, lane);
    const uint64_t wave_id = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    uint32_t* my = scratch + wave_id * scratch_words;
    const uint32_t n = *a.long_count < a.long_cap ? *a.long_count : a.long_cap;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4;
    (void)work_counter;                                      // (records strided over the waves: a ticket per record is an atomic per record)
    for (uint64_t q = wave_id; q < n; q += n_waves) tk_flat_long_wave(a, pw, (uint32_t)q, lane, my);
}

// stage two for the records of 65..128 bytes that are no vocabulary keys: one lane per piece (tk_merge_long_wave<128>), three
// waves per block (32 KB of PAIR filter + 3 x 40 KB of columns in the compact layout), one block per CU.  (The same with 256-entry columns for
// 129..256 bytes -- 128 KB per wave, ONE wave per CU -- was measured and dropped: 4.4 ms where the single-wave merge of stage
// one takes 4.7 ms for the same pieces; 64 chains per CU at ~3 us a round are no better than a dozen at 1.1 us a merge.)
#define TKM_L128_BLOCK 192
#define TKM_L128_LDS_BYTES ((TK_PAIRF_WORDS + (TKM_L128_BLOCK / 64) * TKM_LDS_WORDS(128)) * 4)
template <int N, int BLOCK>
__device__ __forceinline__ void tk_flat_longN_body(const TkFlatArgs& a, uint32_t* wlds) {
    const uint64_t n = *a.long_count < a.long_cap ? *a.long_count : a.long_cap;
    if (n == 0) return;                                      // (grid-uniform)
    tk_merge_load_filter<BLOCK>(a, wlds);
    const uint64_t wave = (uint64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (BLOCK / 64);
    uint32_t* mlds = wlds + TK_PAIRF_WORDS + (threadIdx.x >> 6) * TKM_LDS_WORDS(N);
    for (uint64_t w = wave; w * 64 < n; w += n_waves) tk_merge_long_wave<N>(a, w, wv_lane(), mlds, wlds);
}
__global__ __launch_bounds__(TKM_L128_BLOCK) void tk_flat_long128_kernel(TkFlatArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t wlds[];
    tk_flat_longN_body<128, TKM_L128_BLOCK>(a, wlds);
}

// stage two for the marked records of 129..TKF_LONGCAP bytes: the single-wave merge alone, records strided over the waves
__global__ __launch_bounds__(256) void tk_flat_long_coop_kernel(TkFlatArgs a, uint32_t* scratch, uint32_t scratch_words) {
    const int lane = wv_lane();
    const uint64_t wave_id = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    uint32_t* my = scratch + wave_id * scratch_words;
    const uint32_t n = *a.long_count < a.long_cap ? *a.long_count : a.long_cap;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4;
    for (uint64_t q = wave_id; q < n; q += n_waves) tk_flat_long_coop_wave(a, (uint32_t)q, lane, my);
}

hipError_t tk_launch_flat_long(const TkFlatArgs& a, uint32_t* work_counter, uint32_t* scratch, uint32_t scratch_words, uint32_t n_waves,
                               hipStream_t s) {
    hipLaunchKernelGGL(tk_flat_long_kernel, dim3((n_waves + 3) / 4), dim3(256), 0, s, a, work_counter, scratch, scratch_words);
    if (a.long_merge128) {
        static bool attr_set[64] = {false};        // (per device: the LDS opt-in is a per-device function attribute)
        int dev = 0, cus = 256;
        (void)hipGetDevice(&dev);
        if (!attr_set[dev & 63]) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(tk_flat_long128_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    TKM_L128_LDS_BYTES) != hipSuccess)
                return hipErrorInvalidValue;
            attr_set[dev & 63] = true;
        }
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        hipLaunchKernelGGL(tk_flat_long128_kernel, dim3((uint32_t)cus), dim3(TKM_L128_BLOCK), TKM_L128_LDS_BYTES, s, a);
        hipLaunchKernelGGL(tk_flat_long_coop_kernel, dim3((n_waves + 3) / 4), dim3(256), 0, s, a, scratch, scratch_words);
    }
    return hipGetLastError();
}

hipError_t tk_launch_flat_todo(const uint32_t* flags, const uint64_t* doc_offs, uint64_t n_docs, uint32_t* todo, uint32_t* n_todo,
                               uint32_t* maxlen, hipStream_t s) {
    if (n_docs == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_flat_todo_kernel, dim3(tkf_blocks(n_docs)), dim3(TKF_BLOCK), 0, s, flags, doc_offs, n_docs, todo, n_todo, maxlen);
    return hipGetLastError();
}

hipError_t tk_launch_flat_counts(const uint64_t* doc_offs, uint64_t n_docs, uint64_t n_bytes, uint64_t n_chunks,
                                 const uint64_t* P, const uint32_t* lstart, const uint32_t* flags, const uint32_t* holes,
                                 uint32_t extra, uint32_t* counts, void* doc_info, int final_pass, uint32_t* n_flagged, hipStream_t s) {
    if (n_docs == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_flat_counts_kernel, dim3(tkf_blocks(n_docs)), dim3(TKF_BLOCK), 0, s, doc_offs, n_docs, n_bytes,
                       n_chunks, P, lstart, flags, holes, extra, counts, (TkFlatDocInfo*)doc_info, final_pass, n_flagged);
    return hipGetLastError();
}

hipError_t tk_launch_flat_assemble(uint64_t n_docs, const void* doc_info, const uint32_t* kcount, const uint64_t* out_offs,
                                   const uint32_t* tmp, const uint32_t* staging, uint32_t* out_ids, uint32_t bos_id,
                                   uint32_t eos_id, int add_bos, int add_eos, uint64_t* total_out, const uint32_t* skip_if, hipStream_t s) {
    if (n_docs == 0) return hipSuccess;
    TkFlatAssembleArgs a;
    a.total_out = total_out;
    a.skip_if = skip_if;
    a.n_docs = n_docs; a.info = (const TkFlatDocInfo*)doc_info; a.kcount = kcount; a.out_offs = out_offs;
    a.tmp = tmp; a.staging = staging; a.out_ids = out_ids;
    a.bos_id = bos_id; a.eos_id = eos_id; a.add_bos = add_bos; a.add_eos = add_eos;
    uint64_t blocks = ((n_docs + 63) / 64 + (TKF_BLOCK / 64) - 1) / (TKF_BLOCK / 64);   // 64 documents per wave
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(tk_flat_assemble_kernel, dim3((uint32_t)blocks), dim3(TKF_BLOCK), 0, s, a);
    return hipGetLastError();
}

// ---- the folded tail: two launches for tk_launch_scan + tk_launch_merge_wavefirst, two for counts + scan + assembly ----
hipError_t tk_launch_fold_apply(const uint32_t* counts, uint64_t n, uint64_t n_chunks, uint64_t* prefix, uint64_t* block_sums,
                                uint32_t* wave_first, uint32_t* wave_first_wide, uint32_t* narrow_left_out, hipStream_t s) {
    if (n_chunks == 0 || n < 4 * n_chunks) return hipErrorInvalidValue;
    hipError_t e = tk_launch_scan_block_sums(counts, n, block_sums, s);
    if (e != hipSuccess) return e;
    const uint64_t waves = (n + TKF_FOLD_WAVE - 1) / TKF_FOLD_WAVE;
    hipLaunchKernelGGL(tk_fold_apply_kernel, dim3(tkf_blocks(waves * 64)), dim3(TKF_BLOCK), 0, s, counts, n, n_chunks, block_sums, prefix,
                       wave_first, wave_first_wide, narrow_left_out);
    return hipGetLastError();
}

hipError_t tk_launch_flat_counts_sums(const uint64_t* doc_offs, uint64_t n_docs, uint64_t n_bytes, uint64_t n_chunks, const uint64_t* P,
                                      const uint32_t* lstart, const uint32_t* flags, const uint32_t* holes, uint32_t extra,
                                      uint32_t* counts, void* doc_info, int final_pass, uint32_t* n_flagged, uint64_t* group_sums,
                                      uint64_t* doc_block_sums, hipStream_t s) {
    if (n_docs == 0) return hipErrorInvalidValue;
    const uint64_t blocks = (n_docs + TKF_FOLD_DOC_BLOCK - 1) / TKF_FOLD_DOC_BLOCK;
    hipLaunchKernelGGL(tk_flat_counts_sums_kernel, dim3((uint32_t)blocks), dim3(TKF_FOLD_COUNTS_BLOCK), 0, s, doc_offs, n_docs, n_bytes,
                       n_chunks, P, lstart, flags, holes, extra, counts, (TkFlatDocInfo*)doc_info, final_pass, n_flagged, group_sums,
                       doc_block_sums);
    return hipGetLastError();
}

hipError_t tk_launch_flat_assemble_fold(uint64_t n_docs, const void* doc_info, const uint32_t* kcount, const uint32_t* counts,
                                        const uint64_t* group_sums, const uint64_t* doc_block_sums, uint64_t* out_offs,
                                        const uint32_t* tmp, const uint32_t* staging, uint32_t* out_ids, uint32_t bos_id, uint32_t eos_id,
                                        int add_bos, int add_eos, uint64_t* total_out, const uint32_t* skip_if, hipStream_t s) {
    if (n_docs == 0) return hipErrorInvalidValue;
    TkFlatAssembleArgs a;
    a.total_out = total_out;
    a.skip_if = skip_if;
    a.n_docs = n_docs; a.info = (const TkFlatDocInfo*)doc_info; a.kcount = kcount; a.out_offs = out_offs;
    a.tmp = tmp; a.staging = staging; a.out_ids = out_ids;
    a.bos_id = bos_id; a.eos_id = eos_id; a.add_bos = add_bos; a.add_eos = add_eos;
    uint64_t blocks = ((n_docs + 63) / 64 + (TKF_BLOCK / 64) - 1) / (TKF_BLOCK / 64);   // 64 documents per wave
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(tk_flat_assemble_fold_kernel, dim3((uint32_t)blocks), dim3(TKF_BLOCK), 0, s, a, counts, group_sums, doc_block_sums,
                       out_offs);
    return hipGetLastError();
}
