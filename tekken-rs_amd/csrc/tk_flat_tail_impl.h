// tk_flat_tail_impl.h -- the bookkeeping tail of the flat path: everything between the chunk-dense id buffer and the ids a
// caller receives, except the exclusive scans (tk_kernels.hip).  Like tk_flat_impl.h it is written against the wv_* primitives
// alone, so the same source is compiled into the gfx950 kernels of tk_flat.hip (tk_wave_hip.h) and into the CPU wave emulator
// (tests/emu/tk_wave_emu.h), where it runs under the host's sanitizers.  A body takes what its kernel derives from the launch:
// the global thread index (d / e), or (wave, n_waves, lane).
//
//   tkf_firstdoc_body    per chunk: how many documents start below its loaded region; clears flags / holes / the counters
//   tkf_wavefirst_body   per sub-queue: the merge waves whose first item it holds
//   tkf_todo_body        flagged documents -> list for the per-document kernel, the longest of them
//   tkf_counts_body      ids per document from the chunk prefix sums and the document-start ranks; the assembly's record
//   tkf_assemble_waves   chunk-dense ids -> packed ids in document order with BOS / EOS (tkf_assemble_doc: the generic copy)
#ifndef TK_FLAT_TAIL_IMPL_H
#define TK_FLAT_TAIL_IMPL_H
#include <stdint.h>

#include "tk_flat_args.h"

// first_doc[c] = number of documents d with doc_offs[d] < lo(c), lo(c) = max(c * COMMIT - HL, 0);
// document d owns the chunks whose lo lies in (doc_offs[d], doc_offs[d + 1]]  (the last document: everything above)
TK_DEV void tkf_firstdoc_body(uint64_t d, const uint64_t* doc_offs, uint64_t n_docs, uint64_t n_chunks, uint32_t* first_doc,
                              uint32_t* flags, uint32_t* holes, uint32_t* counters16) {
    if (d == 0 && n_chunks) first_doc[0] = 0u;
    if (d < TKC_CLEARED || d == TKC_MEMO_HITS) counters16[d] = 0u;      // the batch's device counters (tk_counters.h)
    if (d <= n_docs) { flags[d] = 0u; holes[d] = 0u; }
    if (d >= n_docs) return;
    const uint64_t s = doc_offs[d], e = doc_offs[d + 1];
    const uint64_t c_lo = (s + TKF_HL) / TKF_COMMIT + 1;
    uint64_t c_hi = d + 1 == n_docs ? n_chunks - 1 : (e + TKF_HL) / TKF_COMMIT;
    if (n_chunks == 0) return;
    if (c_hi > n_chunks - 1) c_hi = n_chunks - 1;
    for (uint64_t c = c_lo; c <= c_hi; ++c) first_doc[c] = (uint32_t)(d + 1);
}

// wave w of tk_merge_kernel starts with item 64 w of the narrow classes, wave w of tk_merge_wide_kernel with item 64 w of
// the wide ones: note down which sub-queue holds it (thread e owns the waves whose first item falls into sub-queue e), so
// that the merge waves do not have to search the prefix sums
TK_DEV void tkf_wavefirst_body(uint64_t e, const uint64_t* prefix, uint64_t n_chunks, uint32_t* wave_first,
                               uint32_t* wave_first_wide, uint32_t* narrow_left_out) {
    if (e >= 4 * n_chunks) return;
    if (e == 0 && narrow_left_out) {   // pieces of 2..16 bytes left to the merge kernel: the memo's misses of this call (the host's hit-rate policy)
        const uint64_t nl = prefix[2 * n_chunks];
        *narrow_left_out = nl > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)nl;
    }
    const bool wide = e >= 2 * n_chunks;
    const uint64_t first = wide ? prefix[2 * n_chunks] : 0;
    const uint64_t lo = prefix[e] - first, hi = prefix[e + 1] - first;
    uint32_t* out = wide ? wave_first_wide : wave_first;
    for (uint64_t w = (lo + 63) / 64; w * 64 < hi; ++w) out[w] = (uint32_t)e;
}

// flagged documents -> list; the longest of them (it sizes the scratch of the piece-by-piece pass) -> *maxlen
// (every lane of the wave that holds document d calls it, lane = d & 63)
TK_DEV void tkf_todo_body(uint64_t d, int lane, const uint32_t* flags, const uint64_t* doc_offs, uint64_t n_docs, uint32_t* todo,
                          uint32_t* n_todo, uint32_t* maxlen) {
    const bool f = d < n_docs && flags[d] != 0u;
    const uint64_t m = wv_ballot(f);
    if (m == 0) return;
    uint32_t base = 0;
    if (lane == (int)__builtin_ctzll(m)) base = wv_atomic_add(n_todo, (uint32_t)__builtin_popcountll(m));
    base = wv_shfl(base, (int)__builtin_ctzll(m));
    if (f) {
        todo[base + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = (uint32_t)d;
        const uint64_t len = doc_offs[d + 1] - doc_offs[d];
        wv_atomic_max(maxlen, (uint32_t)(len > 0xFFFFFFFFull ? 0xFFFFFFFFull : len));
    }
}

// ids of the stream before byte doc_offs[i]
TK_DEV uint64_t tkf_G(const uint64_t* doc_offs, uint64_t i, uint64_t n_bytes, uint64_t n_chunks, const uint64_t* P,
                      const uint32_t* lstart) {
    const uint64_t p = doc_offs[i];
    if (p >= n_bytes) return P[n_chunks];
    return P[p / TKF_COMMIT] + lstart[i];
}

// per document: where its id slots start in the chunk-dense buffer, how many there are (holes included) and how many of
// them lie in the first chunk -- everything the assembly needs in one 16-byte load
struct alignas(16) TkFlatDocInfo {
    uint64_t src;      // (chunk << 32) | first slot inside the chunk's row of tmp -- no division by the row stride in the
                       // assembly; for a handed-back document the index into the per-document kernel's staging
    uint32_t n_slots;  // slots to walk (handed-back document: ids to copy)
    uint32_t n_first;  // slots in the first chunk; bit 31: not eligible for the two-segment fast copy; 0xFFFFFFFF marks a
                       // handed-back document
};

// (every lane of the wave that holds document d calls it, lane = d & 63)
TK_DEV void tkf_counts_body(uint64_t d, int lane, const uint64_t* doc_offs, uint64_t n_docs, uint64_t n_bytes, uint64_t n_chunks,
                            const uint64_t* P, const uint32_t* lstart, const uint32_t* flags, const uint32_t* holes,
                            uint32_t extra, uint32_t* counts, TkFlatDocInfo* info, int final_pass, uint32_t* n_flagged) {
    const bool flagged = d < n_docs && flags[d] != 0u;
    if (!final_pass) {
        // first (optimistic) pass: count the handed-back documents; the host redoes counts / scan / assembly after the
        // per-document kernels if there are any.  Until then they stand in as empty documents.
        const uint64_t m = wv_ballot(flagged);
        if (m && (unsigned)lane == (unsigned)__builtin_ctzll(m)) wv_atomic_add(n_flagged, (uint32_t)__builtin_popcountll(m));
    }
    if (d >= n_docs) return;
    TkFlatDocInfo di;
    if (flagged) {
        if (final_pass) {  // the document keeps the count of the per-document kernel, the assembly copies it from staging
            // (a document that a long-piece record flagged late has not been through those kernels yet and holds a stale count: no
            // document has more ids than bytes + 2, which keeps this pass inside the buffers; the host then redoes it)
            const uint64_t most = doc_offs[d + 1] - doc_offs[d] + 2;
            if ((uint64_t)counts[d] > most) counts[d] = (uint32_t)most;
            di.src = doc_offs[d] + 2 * d;
            di.n_slots = counts[d];
            di.n_first = 0xFFFFFFFFu;
        } else {
            // (counts[d] is left alone: the per-document kernels may be writing it right now, on the second stream -- whatever
            // this pass computes for a batch with flagged documents is thrown away)
            di.src = 0; di.n_slots = 0; di.n_first = 0;
        }
        info[d] = di;
        return;
    }
    const uint64_t g0 = tkf_G(doc_offs, d, n_bytes, n_chunks, P, lstart);
    const uint64_t g1 = tkf_G(doc_offs, d + 1, n_bytes, n_chunks, P, lstart);
    counts[d] = (uint32_t)(g1 - g0) - holes[d] + extra;
    const uint64_t p = doc_offs[d];
    di.src = 0;
    di.n_slots = (uint32_t)(g1 - g0);
    di.n_first = 0;
    if (p < n_bytes) {
        const uint64_t c = p / TKF_COMMIT;
        const uint64_t in_chunk = P[c + 1] - g0;  // slots of chunk c from the document start on
        di.src = (c << 32) | (uint64_t)lstart[d];
        di.n_first = (uint32_t)(in_chunk < (g1 - g0) ? in_chunk : (g1 - g0));
        // the assembly's prefetching copy takes documents of <= 128 slots that lie in at most two chunks
        const uint64_t rest = (g1 - g0) - di.n_first;
        if ((g1 - g0) > 128 || (rest && rest > P[c + 2] - P[c + 1])) di.n_first |= 0x80000000u;
    }
    info[d] = di;
}

struct TkFlatAssembleArgs {
    uint64_t n_docs;
    const TkFlatDocInfo* info;
    const uint32_t* kcount;
    const uint64_t* out_offs;
    const uint32_t* tmp;
    const uint32_t* staging;  // per-document kernel output (document d at doc_offs[d] + 2 d), flagged documents only
    uint32_t* out_ids;
    uint32_t bos_id, eos_id;
    int add_bos, add_eos;
    uint64_t* total_out;      // receives out_offs[n_docs] (the host reads it with the other counters)
    const uint32_t* skip_if;  // optimistic first pass (counters + TKC_HANDED_BACK): nothing is copied when documents were handed back
                              // or long-piece records wait for tk_flat_long_kernel (TKC_LONG_RECS, seen from there): the host
                              // runs the per-document kernels and assembles again); NULL for the final pass
};

// generic copy of one document (any number of chunks / slots, or a handed-back document)
TK_DEV void tkf_assemble_doc(const TkFlatAssembleArgs& a, const TkFlatDocInfo& di0, uint32_t* dst, int lane) {
    TkFlatDocInfo di = di0;
    if (di.n_first == 0xFFFFFFFFu) {
        const uint32_t* src = a.staging + di.src;
        for (uint32_t k = (uint32_t)lane; k < di.n_slots; k += 64u) dst[k] = src[k];
        return;
    }
    di.n_first &= 0x7FFFFFFFu;
    if (a.add_bos) {
        if (lane == 0) dst[0] = a.bos_id;
        dst += 1;
    }
    // the document's slots: n_first in its first chunk, then whole chunks (slot 0 on) until n_slots are walked;
    // holes (slots a missed piece reserved and did not need) are skipped
    uint32_t left = di.n_slots, nn = di.n_first;
    uint64_t c = di.src >> 32;
    const uint32_t* src = a.tmp + c * TKF_STRIDE + (uint32_t)di.src;
    // four groups of 64 slots are requested together (a long document is a chain of load -> ballot -> store steps: one
    // group at a time leaves the wave waiting a memory round trip per 64 ids), and the next row's slot count with them
    const uint64_t below = (1ull << lane) - 1ull;
    while (left) {
        uint32_t kc_next = 0;
        if (left > nn) kc_next = a.kcount[c + 1];
        for (uint32_t k0 = 0; k0 < nn; k0 += 256u) {
            uint32_t v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t k = k0 + 64u * (uint32_t)q + (uint32_t)lane;
                v[q] = k < nn ? src[k] : TKF_HOLE;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint64_t keep = wv_ballot(v[q] != TKF_HOLE);
                if (v[q] != TKF_HOLE) dst[__builtin_popcountll(keep & below)] = v[q];
                dst += __builtin_popcountll(keep);
            }
        }
        left -= nn;
        if (left == 0) break;
        ++c;
        nn = left < kc_next ? left : kc_next;
        src = a.tmp + c * TKF_STRIDE;
    }
    if (a.add_eos && lane == 0) dst[0] = a.eos_id;
}

// One wave takes 64 consecutive documents: their 16-byte records and output offsets are fetched with one coalesced
// load each (lane = document).  The documents are then copied EIGHT at a time: the 16 loads of a group (slots 0..63
// and 64..127 of each document, across its chunk boundary) are issued back to back, so eight documents' worth of
// HBM latency overlap; then each is squeezed (holes out) and stored with all 64 lanes.
#ifndef TKA_GROUP
#define TKA_GROUP 8
#endif
// the copy of the 64 documents from d0 on: lane j holds document d0 + j's record (`mine`; n_first = bit 31 beyond n_docs) and
// output offset (`oo`)
TK_DEV void tkf_assemble_group(const TkFlatAssembleArgs& a, uint64_t d0, const TkFlatDocInfo& mine, uint64_t oo, int lane) {
    const int nd = (int)(a.n_docs - d0 < 64 ? a.n_docs - d0 : 64);
    const uint32_t src_lo = (uint32_t)mine.src, src_hi = (uint32_t)(mine.src >> 32);
    const uint32_t oo_lo = (uint32_t)oo, oo_hi = (uint32_t)(oo >> 32);
    for (int j0 = 0; j0 < nd; j0 += TKA_GROUP) {
        uint32_t v0[TKA_GROUP], v1[TKA_GROUP];
#pragma unroll
        for (int g = 0; g < TKA_GROUP; ++g) {
            const int j = j0 + g;                     // lanes beyond nd hold n_first = bit 31: skipped
            v0[g] = TKF_HOLE; v1[g] = TKF_HOLE;
            const uint32_t nf = wv_readlane(mine.n_first, j & 63);
            if (!(nf & 0x80000000u)) {                // wave-uniform
                const uint32_t ns = wv_readlane(mine.n_slots, j & 63);
                // (chunk, slot) -> the chunk's row of tmp (a scalar base) + a 32-bit slot offset per lane; slots past
                // the document's n_first continue at slot 0 of the next row
                const uint32_t* rowp = a.tmp + (uint64_t)wv_readlane(src_hi, j & 63) * TKF_STRIDE;
                const uint32_t slot = wv_readlane(src_lo, j & 63);
                const uint32_t q0 = (uint32_t)lane, q1 = 64u + (uint32_t)lane;
                const uint32_t o0 = q0 < nf ? slot + q0 : (uint32_t)TKF_STRIDE + (q0 - nf);
                const uint32_t o1 = q1 < nf ? slot + q1 : (uint32_t)TKF_STRIDE + (q1 - nf);
                if (q0 < ns) v0[g] = rowp[o0];
                if (q1 < ns) v1[g] = rowp[o1];
            }
        }
#pragma unroll
        for (int g = 0; g < TKA_GROUP; ++g) {
            const int j = j0 + g;
            if (j >= nd) break;
            const uint32_t nf = wv_readlane(mine.n_first, j);
            uint32_t* dst = a.out_ids + (((uint64_t)wv_readlane(oo_hi, j) << 32) | wv_readlane(oo_lo, j));
            if (nf & 0x80000000u) {
                TkFlatDocInfo di;
                di.src = ((uint64_t)wv_readlane(src_hi, j) << 32) | wv_readlane(src_lo, j);
                di.n_slots = wv_readlane(mine.n_slots, j);
                di.n_first = nf;
                tkf_assemble_doc(a, di, dst, lane);
                continue;
            }
            if (a.add_bos) {
                if (lane == 0) dst[0] = a.bos_id;
                dst += 1;
            }
            const uint32_t c0 = v0[g], c1 = v1[g];
            const uint64_t k0 = wv_ballot(c0 != TKF_HOLE), k1 = wv_ballot(c1 != TKF_HOLE);
            const uint64_t below = (1ull << lane) - 1ull;
            const uint32_t n0 = (uint32_t)__builtin_popcountll(k0);
            if (c0 != TKF_HOLE) dst[(uint32_t)__builtin_popcountll(k0 & below)] = c0;
            if (c1 != TKF_HOLE) dst[n0 + (uint32_t)__builtin_popcountll(k1 & below)] = c1;
            if (a.add_eos && lane == 0) dst[n0 + (uint32_t)__builtin_popcountll(k1)] = a.eos_id;
        }
    }
}

TK_DEV void tkf_assemble_waves(const TkFlatAssembleArgs& a, uint64_t wave, uint64_t n_waves, int lane) {
    if (wave == 0 && lane == 0) *a.total_out = a.out_offs[a.n_docs];
    if (a.skip_if && (*a.skip_if != 0u || a.skip_if[TKC_LONG_RECS - TKC_HANDED_BACK] != 0u)) return;   // (grid-uniform)
    for (uint64_t d0 = wave * 64; d0 < a.n_docs; d0 += n_waves * 64) {
        const uint64_t dm = d0 + (uint64_t)lane;
        TkFlatDocInfo mine;
        mine.src = 0; mine.n_slots = 0; mine.n_first = 0x80000000u;
        uint64_t oo = 0;
        if (dm < a.n_docs) {
            mine = a.info[dm];
            oo = a.out_offs[dm];
        }
        tkf_assemble_group(a, d0, mine, oo, lane);
    }
}

// ------------------------------------------------------------------------------------------
// The FOLDED forms of the two exclusive scans around the bodies above.  A three-kernel scan (tk_kernels.hip: block sums, a
// one-block scan of them, apply) spends two of its launches on a few hundred partial sums.  Here every consumer adds up the
// partial sums below it itself: a few coalesced loads and one wave reduction, and no wave ever waits for another one.  The
// cost is (number of partial sums)^2 loads in all, so the host takes these forms only below a bound (tk_pipeline.cpp) and the
// three-kernel scan above it.  64-bit values cross the lanes as slices that the 32-bit wave scan adds up without overflow.
//
//   tkf_fold_apply_wave      miss side: raw block sums -> miss_prefix, wave_first, wave_first_wide, TKC_NARROW_LEFT
//   tkf_counts_sums_wave     document side: tkf_counts_body for 4 x 64 documents, and their sums per group of 64
//   tkf_assemble_fold_waves  document side: out_offs from block sums + group sums + counts, then tkf_assemble_group
// ------------------------------------------------------------------------------------------
// (the geometry -- TKF_FOLD_TILE, TKF_FOLD_WAVE, TKF_FOLD_GROUPS, TKF_FOLD_DOC_BLOCK -- is in tk_flat_args.h: the host sizes by it)

// sum of v over the 64 lanes mod 2^64, in every lane: slices of 26 / 26 / 12 bits (64 x (2^26 - 1) < 2^32)
TK_DEV uint64_t tkf_wave_sum_u64(uint64_t v) {
    const uint32_t s0 = wv_scan_incl_u32((uint32_t)v & 0x3FFFFFFu);
    const uint32_t s1 = wv_scan_incl_u32((uint32_t)(v >> 26) & 0x3FFFFFFu);
    const uint32_t s2 = wv_scan_incl_u32((uint32_t)(v >> 52));
    return (uint64_t)wv_readlane(s0, 63) + ((uint64_t)wv_readlane(s1, 63) << 26) + ((uint64_t)wv_readlane(s2, 63) << 52);
}

// exclusive prefix sum over the lanes of values below 2^36 (eight 32-bit counts at most): slices of 26 / 10 bits
TK_DEV uint64_t tkf_wave_scan_excl_u36(uint64_t v) {
    const uint32_t s0 = wv_scan_incl_u32((uint32_t)v & 0x3FFFFFFu);
    const uint32_t s1 = wv_scan_incl_u32((uint32_t)(v >> 26));
    return (uint64_t)s0 + ((uint64_t)s1 << 26) - v;
}

// this lane's share of the prefix sum of counts[0 .. x): raw block sums (one per TKF_FOLD_TILE counts) and the counts of the
// open tile, strided over the lanes; tkf_wave_sum_u64 of it is the prefix sum (x <= n, the same x in every lane)
TK_DEV uint64_t tkf_fold_share_at(const uint32_t* counts, const uint64_t* block_sums, uint64_t x, int lane) {
    const uint64_t nb = x / TKF_FOLD_TILE;
    uint64_t acc = 0;
    for (uint64_t i = (uint64_t)lane; i < nb; i += 64) acc += block_sums[i];
    for (uint64_t i = nb * TKF_FOLD_TILE + (uint64_t)lane; i < x; i += 64) acc += counts[i];
    return acc;
}

// Miss side.  counts[0 .. n) are the sub-queue counts (4 n_chunks, class-major) and whatever the caller scans behind them (the
// pipeline: the n_chunks slot counts), block_sums the raw sums of tk_scan_block_sums.  Wave `wave` owns the entries
// [512 wave, 512 wave + 512), lane l eight of them: prefix[e] as tk_scan_apply writes it, prefix[n] by the lane that owns
// entry n - 1, and, from prefix[e] and prefix[e + 1] in registers, exactly what tkf_wavefirst_body writes for sub-queue e.  The
// wide classes count from prefix[2 n_chunks], which the waves that hold one of their entries fold like their own start.
TK_DEV void tkf_fold_apply_wave(uint64_t wave, int lane, const uint32_t* counts, uint64_t n, uint64_t n_chunks,
                                const uint64_t* block_sums, uint64_t* prefix, uint32_t* wave_first, uint32_t* wave_first_wide,
                                uint32_t* narrow_left_out) {
    const uint64_t w0 = wave * TKF_FOLD_WAVE;
    if (w0 >= n) return;                                    // (wave-uniform)
    const uint64_t e0 = w0 + (uint64_t)lane * 8u;
    uint32_t c[8];
    uint64_t v = 0;
    for (int k = 0; k < 8; ++k) {
        c[k] = e0 + (uint64_t)k < n ? counts[e0 + (uint64_t)k] : 0u;
        v += c[k];
    }
    // (both folds' loads first, then the reductions)
    const bool holds_wide = w0 < 4 * n_chunks && w0 + TKF_FOLD_WAVE > 2 * n_chunks;   // (wave-uniform: a wide sub-queue is here)
    const uint64_t share = tkf_fold_share_at(counts, block_sums, w0, lane);
    const uint64_t share_wide = holds_wide ? tkf_fold_share_at(counts, block_sums, 2 * n_chunks, lane) : 0;
    uint64_t run = tkf_wave_sum_u64(share) + tkf_wave_scan_excl_u36(v);
    const uint64_t first_wide = holds_wide ? tkf_wave_sum_u64(share_wide) : 0;
    for (int k = 0; k < 8; ++k) {
        const uint64_t e = e0 + (uint64_t)k;
        if (e >= n) break;
        const uint64_t lo_abs = run;
        run += c[k];
        prefix[e] = lo_abs;
        if (e + 1 == n) prefix[n] = run;
        if (e == 2 * n_chunks && narrow_left_out) *narrow_left_out = lo_abs > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)lo_abs;
        if (e >= 4 * n_chunks) continue;
        const bool wide = e >= 2 * n_chunks;
        const uint64_t first = wide ? first_wide : 0;
        const uint64_t lo = lo_abs - first, hi = run - first;
        uint32_t* out = wide ? wave_first_wide : wave_first;
        for (uint64_t w = (lo + 63) / 64; w * 64 < hi; ++w) out[w] = (uint32_t)e;
    }
}

// Document side, counts.  Wave `wave` takes the groups 4 wave .. 4 wave + 3 of 64 documents through tkf_counts_body and leaves
// the sum of every group's counts in group_sums; returns the sum of the four (the kernel adds its 16 waves' up to the block sum).
TK_DEV uint64_t tkf_counts_sums_wave(uint64_t wave, int lane, const uint64_t* doc_offs, uint64_t n_docs, uint64_t n_bytes,
                                     uint64_t n_chunks, const uint64_t* P, const uint32_t* lstart, const uint32_t* flags,
                                     const uint32_t* holes, uint32_t extra, uint32_t* counts, TkFlatDocInfo* info, int final_pass,
                                     uint32_t* n_flagged, uint64_t* group_sums) {
    // (no early exit and unrolled: the four groups' chains of dependent loads -- flags, doc_offs, P -- are independent of each
    // other and overlap; a group beyond n_docs loads and stores nothing)
    uint32_t cnt[TKF_FOLD_GROUPS];
#pragma unroll
    for (uint32_t g = 0; g < TKF_FOLD_GROUPS; ++g) {
        const uint64_t d = (wave * TKF_FOLD_GROUPS + g) * 64 + (uint64_t)lane;
        tkf_counts_body(d, lane, doc_offs, n_docs, n_bytes, n_chunks, P, lstart, flags, holes, extra, counts, info, final_pass, n_flagged);
        // (a handed-back document of the optimistic pass keeps whatever count it has, as for the scan kernels: the pass is redone)
        cnt[g] = d < n_docs ? counts[d] : 0u;
    }
    uint64_t wave_sum = 0;
#pragma unroll
    for (uint32_t g = 0; g < TKF_FOLD_GROUPS; ++g) {
        const uint64_t grp = wave * TKF_FOLD_GROUPS + g;
        const uint64_t s = tkf_wave_sum_u64((uint64_t)cnt[g]);
        if (lane == 0 && grp * 64 < n_docs) group_sums[grp] = s;
        wave_sum += s;
    }
    return wave_sum;
}

// Document side, assembly.  A wave's 64 output offsets: the block sums below its block of 4096 documents, the group sums of
// its block below its group (one reduction for both), and an exclusive scan of its 64 counts.  It writes out_offs for its
// documents -- the wave with the last document also out_offs[n_docs] and *total_out -- and copies with tkf_assemble_group.
// (a.out_offs is not read.)
TK_DEV void tkf_assemble_fold_waves(const TkFlatAssembleArgs& a, const uint32_t* counts, const uint64_t* group_sums,
                                    const uint64_t* doc_block_sums, uint64_t* out_offs, uint64_t wave, uint64_t n_waves, int lane) {
    const bool skip = a.skip_if && (*a.skip_if != 0u || a.skip_if[TKC_LONG_RECS - TKC_HANDED_BACK] != 0u);   // (grid-uniform)
    for (uint64_t d0 = wave * 64; d0 < a.n_docs; d0 += n_waves * 64) {
        const uint64_t dm = d0 + (uint64_t)lane;
        const uint64_t grp = d0 / 64, blk = d0 / TKF_FOLD_DOC_BLOCK;
        uint64_t acc = 0;
        for (uint64_t i = (uint64_t)lane; i < blk; i += 64) acc += doc_block_sums[i];
        const uint64_t g = blk * (TKF_FOLD_DOC_BLOCK / 64) + (uint64_t)lane;
        if (g < grp) acc += group_sums[g];
        const uint32_t cnt = dm < a.n_docs ? counts[dm] : 0u;
        const uint64_t oo = tkf_wave_sum_u64(acc) + tkf_wave_scan_excl_u36(cnt);
        if (dm < a.n_docs) out_offs[dm] = oo;
        if (dm + 1 == a.n_docs) {
            out_offs[a.n_docs] = oo + cnt;
            *a.total_out = oo + cnt;
        }
        if (skip) continue;
        TkFlatDocInfo mine;
        mine.src = 0; mine.n_slots = 0; mine.n_first = 0x80000000u;
        if (dm < a.n_docs) mine = a.info[dm];
        tkf_assemble_group(a, d0, mine, oo, lane);
    }
}

#endif
