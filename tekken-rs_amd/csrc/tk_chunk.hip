// tk_chunk.hip -- gfx950 kernels of the boundary-aware token-budget chunks (include/tekken_hip.h tk_chunk_from_ids_device,
// tk_chunk_levels_device).
//
// No reference equivalent: the reference has pad_id() (src/tekkenizer.rs:304) and nothing that uses it.  Ragged ids + offsets and one
// LEVEL byte per id in (the strength of the break in front of the id: 0 NONE .. 5 PARAGRAPH); every document longer than
// max_length T cut into chunks of at most c = T - h - t body ids that end at the strongest break in [a + m, a + c], each with the
// document's head and tail; input_ids[W, L] (+ mask, spans, lengths, window_doc, window_start, doc_windows, cut_level,
// chunk_bytes, level_counts) out.  With every level equal the chunks are tk_window.hip's windows at stride = overlap.
//
// Three kernels:
//   1. tk_chunk_levels_kernel (tk_chunk_levels_device): the level bytes from text and spans.  A sibling of the words kernel's walk
//      (tk_words.hip): one wave per group of TK_DECODE_GROUP_DOCS consecutive documents, their ids as ONE stream, 64 ids a step,
//      the span starts requested one step ahead; a DPP prefix maximum over the marked document starts gives an id's document slot,
//      lanes j < 16 hold doc_offs[dA + j] and the document's length and a lane fetches its own by a cross-lane read.  Per id the
//      byte at the span start and a back-scan over at most 16 white-space bytes (typical text: one to three bytes), every read
//      inside text[0 : len] of the id's document; one byte stored per lane.
//   2. tk_chunk_walk_kernel<RUN>, run twice.  A wave takes `group` consecutive documents, one a lane: unsplit ones are settled
//      there.  Split ones are taken one after another by the WHOLE wave (a ballot loop): every step of the greedy chain scans the
//      candidate range [a + m, a + c] 64 positions at a time from the top with coalesced byte loads -- every lane keeps the best
//      (level, position) of its column, a position further up winning a tie, and two DPP prefix maxima give the cut; a block that
//      holds the top level ends the scan early -- and the at most o positions in front of the cut from the bottom for the next
//      start (a ballot per 64).  No LDS; a level byte is read about (c - m) / (m - o) + 1 times.  One lane per document would
//      serialise a long document into thousands of dependent loads.
//        RUN 0: w_d per document, the longest document, the split documents, the cuts made at every level (lane L counts level L:
//               one atomic a lane and wave).  tk_launch_scan over w_d gives doc_windows, one host read sizes the tensors.
//        RUN 1: the same chains again; lane 0 writes the record (body start, body length, cut level) of every window.
//   3. tk_chunk_kernel: tk_window_kernel's launch shape and body (the row-group launch shape of tk_rows.h over W rows, TkyRowOwners
//      over doc_windows with oo[d] and n_d beside them in LDS, the 4-wide gather, 16-byte stores where L % 4 == 0); bs and blen
//      come from the window's record instead of kw * step.  Every element of every selected output is written exactly once, pads
//      included.  The lane with a row's first unit writes lengths, window_doc, window_start, cut_level and chunk_bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tk_kernels.h"
#include "tk_layout.h"

#define TKC_LEVEL_TOKEN 1u
#define TKC_LEVEL_WORD 2u
#define TKC_LEVEL_TOP 5u
#define TKC_CUT_LAST 255u
#define TKC_BACK 16u           /* white-space bytes the back-scan of the levels walks at most */

__device__ __forceinline__ uint64_t tkc_readlane64(uint64_t v, uint32_t l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t tkc_shfl64(uint64_t v, uint32_t l) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)l);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)l);
    return ((uint64_t)hi << 32) | lo;
}

// ---- 1. the levels ----
__device__ __forceinline__ bool tkc_ws(uint32_t c) { return c == 0x20u || (c >= 0x09u && c <= 0x0Du); }

// the level of the break in front of byte p of text[0 : len], before the mask (the rules of include/tekken_hip.h, first match wins)
__device__ __forceinline__ uint32_t tkc_level(const uint8_t* __restrict__ text, uint64_t len, uint64_t p) {
    if (p >= len || p == 0u) return 1u;
    const uint32_t c0 = text[p];
    if ((c0 & 0xC0u) == 0x80u) return 0u;
    uint64_t q = p;
    uint32_t nl = 0, walked = 0;
    while (walked < TKC_BACK && q > 0u) {
        const uint32_t c = text[q - 1u];
        if (!tkc_ws(c)) break;
        nl += c == 0x0Au;
        --q; ++walked;
    }
    if (nl >= 2u) return 5u;
    if (nl == 1u) return 4u;
    const bool gap = q < p || tkc_ws(c0);
    if (walked < TKC_BACK && q > 0u) {
        const uint32_t e = text[q - 1u];
        if (gap && (e == '.' || e == '!' || e == '?')) return 3u;
        if (q >= 3u) {
            const uint32_t w = (uint32_t)text[q - 3u] << 16 | (uint32_t)text[q - 2u] << 8 | e;
            if (w == 0xE38082u || w == 0xEFBC81u || w == 0xEFBC9Fu) return 3u;
        }
    }
    return gap ? 2u : 1u;
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_chunk_levels_kernel(TkChunkArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * (TKY_BLOCK / 64) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (TKY_BLOCK / 64);
    const uint64_t n_groups = (a.n_docs + TK_DECODE_GROUP_DOCS - 1) / TK_DECODE_GROUP_DOCS;
    for (uint64_t g = wave; g < n_groups; g += n_waves) {
        const uint64_t dA = g * TK_DECODE_GROUP_DOCS, dB = dA + TK_DECODE_GROUP_DOCS < a.n_docs ? dA + TK_DECODE_GROUP_DOCS : a.n_docs;
        const uint32_t ndg = (uint32_t)(dB - dA);
        const uint64_t i0 = a.id_offs[dA], i1 = a.id_offs[dB];
        // lane j < ndg: document dA + j -- its first id, where its text begins, its length
        const uint64_t dfirst = lane < ndg ? a.id_offs[dA + lane] : ~0ull;
        const uint64_t dtext = lane < ndg ? a.doc_offs[dA + lane] : 0ull;
        const uint64_t dlen = lane < ndg ? a.doc_offs[dA + lane + 1u] - dtext : 0ull;
        uint32_t jn = 0;                                   // the next document whose first id has not been placed (wave-uniform)
        uint64_t nfirst = tkc_readlane64(dfirst, 0);
        uint32_t slot = 0;                                 // the slot of the document of the step before's last id
        uint32_t p0 = i0 + lane < i1 ? a.in_spans[2u * (i0 + lane)] : 0u;
        for (uint64_t c0 = i0; c0 < i1; c0 += 64) {
            const uint64_t i = c0 + lane;
            const bool have = i < i1;
            const uint32_t p1 = i + 64 < i1 ? a.in_spans[2u * (i + 64)] : 0u;    // one step ahead
            // documents whose first id is one of this step's 64: mark their lanes with the slot (scalar loop, the starts are in
            // order; of several documents that start at one id the last one owns it, the others are empty)
            uint32_t mark = 0;
            while (nfirst < c0 + 64) {
                if (lane == (uint32_t)(nfirst - c0)) mark = jn + 1u;
                ++jn;
                nfirst = jn < ndg ? tkc_readlane64(dfirst, jn) : ~0ull;
            }
            const uint32_t sm = tkd_scan_max(mark);
            const uint32_t j = sm ? sm - 1u : slot;
            const uint64_t text = tkc_shfl64(dtext, j), len = tkc_shfl64(dlen, j);
            if (have) a.lev_out[i] = (uint8_t)((a.demote >> (4u * tkc_level(a.bytes + text, len, p0))) & 15u);
            slot = (uint32_t)__builtin_amdgcn_readlane((int)j, 63);
            p0 = p1;
        }
    }
}

// ---- 2. the walk ----
template <int RUN>
__global__ __launch_bounds__(TKY_BLOCK) void tk_chunk_walk_kernel(TkChunkArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t T = a.max_len, h = a.keep_head, t = a.keep_tail, c = T - h - t, m = a.min_len, ov = a.overlap, G = a.group;
    const uint64_t wave = (uint64_t)blockIdx.x * (TKY_BLOCK / 64) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (TKY_BLOCK / 64);
    const uint64_t n_groups = (a.n_docs + G - 1u) / G;
    uint32_t longest = 0, n_split = 0;
    uint32_t cuts = 0;                                      // lane L < 6: the cuts this wave made at level L
    for (uint64_t g = wave; g < n_groups; g += n_waves) {
        const uint64_t d = g * G + lane;
        const bool have = lane < G && d < a.n_docs;
        uint64_t o0 = 0, row0 = 0;
        uint32_t n = 0;
        if (have) {
            o0 = a.id_offs[d];
            n = tky_len32(a.id_offs[d + 1u] - o0);
            if (RUN) row0 = a.doc_windows[d];
        }
        longest = longest > n ? longest : n;
        const bool split = have && n > T && n != 0xFFFFFFFFu;   // (a clamped n is refused by the host before w is used)
        if (have && !split) {
            if (RUN) a.rec[row0] = TkChunkRec{0u, n, TKC_CUT_LAST, 0u};
            else a.counts[d] = 1u;
        }
        n_split += split ? 1u : 0u;
        uint64_t todo = __ballot(split);
        while (todo) {                                      // one split document after another, by the whole wave
            const uint32_t l = (uint32_t)__builtin_amdgcn_readfirstlane((int)__builtin_ctzll(todo));
            todo &= todo - 1u;
            const uint64_t so = tkc_readlane64(o0, l), srow = RUN ? tkc_readlane64(row0, l) : 0ull;
            const uint32_t sn = (uint32_t)__builtin_amdgcn_readlane((int)n, (int)l);
            const uint8_t* __restrict__ L = a.lev + so + h;    // L[j]: the break in front of body id j, j < b
            const uint32_t b = sn - h - t;
            uint32_t s = 0, k = 0;                          // the chunk's start in the body; chunks so far
            for (;;) {
                if (b - s <= c) {                           // the last chunk
                    if (RUN && lane == 0u) a.rec[srow + k] = TkChunkRec{s, b - s, TKC_CUT_LAST, 0u};
                    ++k;
                    break;
                }
                // the cut: the largest j in [s + m, s + c] (all below b) of the highest level; from the top, lane i at top - i
                const uint32_t lo = s + m;
                uint32_t key = 0, pos = 0;                  // level + 1 and position of the lane's best (0: none yet)
                for (uint32_t top = s + c;; top -= 64u) {
                    const bool v = lane <= top - lo;
                    const uint32_t j = top - lane;
                    uint32_t lv = v ? (uint32_t)L[j] : 0u;
                    lv = lv > TKC_LEVEL_TOP ? TKC_LEVEL_TOP : lv;
                    const uint32_t kk = v ? lv + 1u : 0u;
                    if (kk > key) { key = kk; pos = j; }    // (a block further up keeps a tie)
                    if (top - lo < 64u || __ballot(key == TKC_LEVEL_TOP + 1u) != 0ull) break;
                }
                const uint32_t bk = (uint32_t)__builtin_amdgcn_readlane((int)tkd_scan_max(key), 63);
                const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)tkd_scan_max(key == bk ? pos : 0u), 63);   // (pos >= m >= 1)
                if (RUN) {
                    if (lane == 0u) a.rec[srow + k] = TkChunkRec{s, e - s, bk - 1u, 0u};
                } else {
                    cuts += lane == bk - 1u ? 1u : 0u;
                }
                ++k;
                // the next start: the first word break in [max(s + 1, e - o), e), else the first token break there, else e
                const uint32_t from = e - ov > s + 1u ? e - ov : s + 1u;    // (e >= s + m > o)
                uint32_t nxt = e;
                bool tok = false;
                for (uint32_t q = from; q < e; q += 64u) {
                    const uint32_t lv = lane < e - q ? (uint32_t)L[q + lane] : 0u;
                    const uint64_t bw = __ballot(lv >= TKC_LEVEL_WORD);
                    if (bw) { nxt = q + (uint32_t)__builtin_ctzll(bw); break; }
                    const uint64_t bt = __ballot(lv >= TKC_LEVEL_TOKEN);
                    if (!tok && bt) { nxt = q + (uint32_t)__builtin_ctzll(bt); tok = true; }
                    if (e - q <= 64u) break;                // (q + 64 stays below 2^32)
                }
                s = nxt;
            }
            if (!RUN && lane == l) a.counts[d] = k;
        }
    }
    if (!RUN) {
        tky_wave_max(a.stat, longest);
        tky_wave_add(a.stat + 1, n_split);
        if (lane < 6u && cuts) atomicAdd(a.stat + 2u + lane, (unsigned long long)cuts);
    }
}

// ---- 3. the fill ----
template <int I64, int MASK, int VEC>
__global__ __launch_bounds__(TKY_BLOCK) void tk_chunk_kernel(TkChunkArgs a) {
    constexpr uint32_t W = VEC ? 4u : 1u;
    __shared__ uint64_t s_oo[TKY_CAP + 1u];             // oo[d] of the block's documents, [0]: the one that holds its first row
    __shared__ uint32_t s_n[TKY_CAP + 1u];              // n_d of the same
    const uint32_t G = a.rows.units, L = a.row_len, T = a.max_len, h = a.keep_head, t = a.keep_tail;
    const uint64_t n_rb = tky_row_groups(a.rows, a.n_rows);
    for (uint64_t b = blockIdx.x; b < n_rb; b += gridDim.x) {
        const TkyRowGroup g(a.rows, a.n_rows, b);
        const TkyRowOwners docs(a.doc_windows, a.n_docs, g, [&](uint32_t j, uint64_t e) {
            const uint64_t o = a.id_offs[e];
            s_oo[j] = o;
            s_n[j] = (uint32_t)(a.id_offs[e + 1u] - o);
        });
        for (uint32_t li = g.first(); li < g.total; li += g.step()) {
            const uint32_t r = tky_row_of(a.rows, li), cg = li - r * G;
            const uint32_t kd = docs.count_le(r);       // the block's document that holds row r
            const uint64_t d = docs.n_lo - 1u + kd;
            uint64_t o0;
            uint32_t n;
            if (docs.lds) {
                o0 = s_oo[kd]; n = s_n[kd];
            } else {
                o0 = a.id_offs[d]; n = (uint32_t)(a.id_offs[d + 1u] - o0);
            }
            const uint64_t row = g.row0 + r;
            const tky_u32x4 rec = *reinterpret_cast<const tky_u32x4*>(a.rec + row);   // body start | body length | cut level
            // the three source runs of the window: [0, hh) head | [hh, hb) body, from body index bs | [hb, len) tail
            const uint32_t hh = n > T ? h : 0u, tt = n > T ? t : 0u, bs = rec.x, blen = rec.y;   // (unsplit: bs = 0, blen = n)
            const uint32_t hb = hh + blen, len = hb + tt;
            if (cg == 0u) {
                const uint64_t ws = (uint64_t)h + bs;
                a.lengths[row] = len;
                a.window_doc[row] = (uint32_t)d;
                a.window_start[row] = ws < n ? (uint32_t)ws : n;
                a.cut_level[row] = (uint8_t)rec.z;
                if (a.chunk_bytes) {                    // from the first body id's start to the last one's end
                    const uint64_t f = o0 + hh + bs;
                    a.chunk_bytes[2u * row] = blen ? a.in_spans[2u * f] : 0u;
                    a.chunk_bytes[2u * row + 1u] = blen ? a.in_spans[2u * (f + blen - 1u) + 1u] : 0u;
                }
            }
            if (L == 0u) continue;                      // (every document is empty: only the per-row outputs)
            const uint32_t j0 = cg * W;
            // where element j < len of the window lies in ids
            auto src = [&](uint32_t j) -> uint64_t {
                return o0 + (j < hh ? j : j < hb ? hh + bs + (j - hh) : (n - tt) + (j - hb));
            };
            uint32_t v[4], sp[8];
            uint32_t mbits = 0;
            bool run4 = false;
            uint64_t s0 = 0;
            if (VEC && j0 + 4u <= len) {
                s0 = src(j0);
                run4 = src(j0 + 3u) == s0 + 3u;
            }
            if (VEC && run4) {
                tky_gather4(a.ids + s0, v);
                mbits = 0x01010101u;
                if (a.out_spans) tky_gather4_spans(a.in_spans, s0, sp);
            } else {
#pragma unroll
                for (uint32_t q = 0; q < W; ++q) {
                    const uint32_t j = j0 + q;
                    const bool in = j < len;
                    const uint64_t sq = in ? src(j) : 0u;
                    v[q] = in ? a.ids[sq] : a.pad_id;
                    mbits |= (uint32_t)in << (8u * q);
                    if (a.out_spans) {
                        sp[2u * q] = in ? a.in_spans[2u * sq] : 0u;
                        sp[2u * q + 1u] = in ? a.in_spans[2u * sq + 1u] : 0u;
                    }
                }
            }
            const uint64_t at = row * L + j0;
            tky_store<I64, VEC>(a.out, at, v);
            if (MASK) tky_store_plane<VEC>(a.mask, at, mbits);
            if (a.out_spans) tky_store_spans<VEC>(a.out_spans, at, sp);
        }
    }
}

hipError_t tk_launch_chunk_levels(const TkChunkArgs& a, hipStream_t s) {
    if (a.n_docs == 0) return hipSuccess;
    const uint64_t n_groups = (a.n_docs + TK_DECODE_GROUP_DOCS - 1) / TK_DECODE_GROUP_DOCS;
    hipLaunchKernelGGL(tk_chunk_levels_kernel, dim3(tky_blocks(n_groups, 8192u, TKY_BLOCK / 64)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_chunk_walk(const TkChunkArgs& args, int records, hipStream_t s) {
    if (args.n_docs == 0) return hipSuccess;
    TkChunkArgs a = args;
    // 64 documents a wave where that still gives every SIMD of the part a wave (256 CUs x 4 SIMDs), fewer a wave for a smaller
    // batch: its split documents, which a wave takes one after another, then go to more waves
    a.group = 64u;
    while (a.group > 1u && (a.n_docs + a.group - 1u) / a.group < 1024u) a.group >>= 1;
    const uint64_t n_groups = (a.n_docs + a.group - 1u) / a.group;
    const dim3 grid(tky_blocks(n_groups, 8192u, TKY_BLOCK / 64));
    if (records) hipLaunchKernelGGL((tk_chunk_walk_kernel<1>), grid, dim3(TKY_BLOCK), 0, s, a);
    else hipLaunchKernelGGL((tk_chunk_walk_kernel<0>), grid, dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_chunk(const TkChunkArgs& args, int i64, hipStream_t s) {
    TkChunkArgs a = args;
    const TkyRowsGrid rg = tky_rows_shape(a.n_rows, a.row_len, true, a.rows);   // (L == 0: one unit a row, which writes the per-row outputs)
    if (rg.x == 0u) return hipSuccess;
    TKY_LAUNCH_I64_MASK_VEC(tk_chunk_kernel, i64, a.mask, a.row_len != 0u && a.row_len % 4u == 0u, dim3(rg.x, rg.y), s, a);
    return hipGetLastError();
}
