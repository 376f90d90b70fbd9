// tk_noise.hip -- gfx950 kernels of the noise pass (include/tekken_hip.h tk_noise_replace_device / tk_noise_spans_device).
//
// No reference equivalent.  The ragged ids of D documents in; a hash-drawn (or caller-given) choice of tokens, words or spans of
// each document; out either the ids with the chosen ones masked / replaced and the labels (replace mode: masked LM), or the
// documents with every chosen run replaced by a sentinel and the targets "sentinel, run, sentinel, run, ..." (spans mode: T5 / UL2).
//
// Every kernel over ids has the join / regroup / FIM shape (tk_layout.h): a block takes tiles of TKN_TILE input ids, two wave
// searches over offs find the tile's documents, their starts go to LDS; a thread takes 4 consecutive ids a round (one 16-byte
// load), 4 rounds a tile.
//   a. the selection (tk_noise_select_kernel<REPLACE>).  TOKEN unit: every thread makes the two hashes of its own positions; a
//      position that starts a span holds where the span ends (clamped to its document's end, so that a plain prefix maximum never
//      carries a span into the next document), and covered(x) is "the prefix maximum up to x lies behind x".  The maximum runs
//      over the thread's 4, the wave (tk_dpp_scan.h), the block's 4 waves through LDS and from round to round in a register; in
//      front of the tile one wave recomputes the span_max - 1 positions of the halo from their hashes, of which only the maximum
//      is needed.  Nothing is carried between tiles.  WORD unit: covered(x) is recomputed per id from the at most span_max
//      candidate starts q <= x -- word_ids are the caller's, so nothing about their order is assumed; an id with the word of the
//      id in front of it takes that id's answer.  REPLACE: the mode ends here -- ids, labels and the selected bytes in 16-byte
//      (4-byte) stores, the three counters one atomic a block (tkn_block_add).  Else only the selected bytes are written, for b.
//   b. spans mode works on the selected bytes.  tk_noise_count_kernel: the tile's (selected, run starts) -- a run start looks one
//      byte back, over the tile border too -- and, for every document that starts inside the tile, the two counts in front of
//      it.  Two scans over tiles; tk_noise_docs_kernel: the counts in front of every document (SB, RB).  Kept runs are the first
//      n_sentinels of a document, so the kept ids are a PREFIX of its selected ids: all the fill needs beside SB and RB is KS(d),
//      how many selected ids the document keeps -- where a run is dropped, the selected ids in front of run n_sentinels
//      (tk_noise_drop_kernel; it returns at once where no document drops a run).  tk_noise_lens_kernel, two scans over documents,
//      ONE host read that sizes the outputs, and tk_noise_fill_kernel: every id computes where it goes from its document's base and
//      the in-document prefix counts; a run start also writes its sentinel; the documents' final ids and joined_offsets by a
//      loop over documents at the kernel's end (an empty document has no id to own them).  Every output element is written once;
//      a position is used only where it lies inside the output.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tk_kernels.h"
#include "tk_layout.h"

#define TKN_FAR 0xFFFFFFFFu
#define TKN_GRID (1u << 20)    /* blocks of a launch at most: beyond it a block loops over its tiles (documents) */
typedef uint32_t __attribute__((aligned(1))) tkn_u32_a1;

// ---- the draws (step 2 of the definition) ----

__device__ __forceinline__ bool tkn_start(const TkNoiseArgs& a, uint32_t t0, uint32_t x) { return (uint64_t)tki_hash(t0, x) < a.start_q32; }
__device__ __forceinline__ uint32_t tkn_len(const TkNoiseArgs& a, uint32_t t1, uint32_t x) {
    return a.span_min + (uint32_t)(((uint64_t)tki_hash(t1, x) * (a.span_max - a.span_min + 1u)) >> 32);
}
// covered(x) from the candidate starts themselves: at most span_max of them
__device__ __forceinline__ bool tkn_covered(const TkNoiseArgs& a, uint32_t t0, uint32_t t1, uint32_t x) {
    const uint32_t back = x < a.span_max - 1u ? x : a.span_max - 1u;
    for (uint32_t j = 0; j <= back; ++j) {
        const uint32_t q = x - j;
        if (tkn_start(a, t0, q) && tkn_len(a, t1, q) > j) return true;
    }
    return false;
}

// ---- the block's scans: v of every thread -> what lies in front of the thread in the block, and the block's total.  Every thread
// of the block calls them; s_w: 4 words of LDS, free again on return ----
__device__ __forceinline__ uint32_t tkn_block_sum(uint32_t v, uint32_t* s_w, uint32_t* total) {
    const uint32_t incl = tkd_scan_incl(v), wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 63u) s_w[wave] = incl;
    __syncthreads();
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < TKY_BLOCK / 64u; ++w) {
        const uint32_t x = s_w[w];
        before += w < wave ? x : 0u;
        tot += x;
    }
    __syncthreads();
    *total = tot;
    return before + incl - v;
}
// the maximum over the threads in front of this one (0: none), and the block's
__device__ __forceinline__ uint32_t tkn_block_max(uint32_t v, uint32_t* s_w, uint32_t* total) {
    const uint32_t incl = tkd_scan_max(v), wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t up = (uint32_t)__shfl_up((int)incl, 1);
    if (lane == 63u) s_w[wave] = incl;
    __syncthreads();
    uint32_t before = lane ? up : 0u, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < TKY_BLOCK / 64u; ++w) {
        const uint32_t x = s_w[w];
        before = max(before, w < wave ? x : 0u);
        tot = max(tot, x);
    }
    __syncthreads();
    *total = tot;
    return before;
}

// A counter of the call: the block's sum of v in ONE atomic (none where it is 0), into one of TKN_SLOTS copies of the counter by the
// block's index -- tens of thousands of atomics on one address cost more than the kernel (the host adds the copies up).  Every
// thread of the block calls it.
__device__ __forceinline__ void tkn_block_add(unsigned long long* stat, uint32_t k, uint32_t v, uint32_t* s_w) {
    uint32_t total;
    (void)tkn_block_sum(v, s_w, &total);
    if (threadIdx.x == 0u && total) atomicAdd(stat + (blockIdx.x % TKN_SLOTS) * TKN_STATS + k, (unsigned long long)total);
}

// The tile's entry (kq) and the position inside its document (pq) of the thread's ids l .. l + 3; behind the tile's end: the last
// id's.  (The LAST document that starts at or before an id holds it: empty ones are stepped over.)
__device__ __forceinline__ void tkn_docs(const TkyTile<2>& tile, uint32_t l, uint32_t len, uint32_t* kq, uint32_t* pq) {
    uint32_t k = 0;
    int64_t start = 0;
    if (l < len) {
        k = tile.count_le(l);
        start = tile.start_of(k);
    }
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
        if (q && l + q < len)
            while (k < tile.count && tile.rel(k) <= l + q) { start = (int64_t)tile.rel(k); ++k; }
        kq[q] = k;
        pq[q] = (uint32_t)((int64_t)(l + q) - start);
    }
}

// x[0 .. 4) = src[g .. g + 4) where `full`, else the ones in front of n (the others 0); src 4-byte elements, g a multiple of 4
__device__ __forceinline__ void tkn_load4(const uint32_t* src, uint64_t g, uint64_t n, bool full, uint32_t* x) {
    if (full) {
        const tky_u32x4 v = *reinterpret_cast<const tky_u32x4_a4*>(src + g);   // (the caller's arrays: at any dword)
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) x[q] = g + q < n ? src[g + q] : 0u;
    }
}
// ... of a byte array: one dword
__device__ __forceinline__ void tkn_load4_u8(const uint8_t* src, uint64_t g, uint64_t n, bool full, uint32_t* x) {
    if (full) {
        const uint32_t v = *reinterpret_cast<const tkn_u32_a1*>(src + g);      // (... at any byte)
        x[0] = v & 255u; x[1] = (v >> 8) & 255u; x[2] = (v >> 16) & 255u; x[3] = v >> 24;
    } else {
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) x[q] = g + q < n ? src[g + q] : 0u;
    }
}

// ---- a. the selection; REPLACE: and the mode's outputs ----

template <int REPLACE>
__global__ __launch_bounds__(TKY_BLOCK) void tk_noise_select_kernel(TkNoiseArgs a) {
    __shared__ uint32_t s_w[TKY_BLOCK / 64u];
    __shared__ uint32_t s_halo;
    const uint64_t N = a.n_ids, D = a.n_docs;
    const uint64_t n_tiles = (N + TKN_TILE - 1) / TKN_TILE;
    const bool given = a.sel != nullptr, by_word = a.unit == TK_NOISE_UNIT_WORD, words = by_word && a.word_ids != nullptr;
    const bool scan = !given && !by_word;               // (block-uniform)
    uint32_t n_sel = 0, n_mask = 0, n_rand = 0;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t g0 = t * TKN_TILE;
        const uint64_t g1 = N - g0 < TKN_TILE ? N : g0 + TKN_TILE;
        TkyTile<2> tile(a.offs, g0);
        tile.search(D, g0, g1 - 1u);
        const uint64_t n_lo = tile.found(0);
        if (n_lo == 0 || tile.found(1) < n_lo) continue;
        tile.open(n_lo, tile.found(1) - n_lo);
        tile.stage();
        const uint32_t len = (uint32_t)(g1 - g0);
        uint32_t carry = 0;                             // how far the spans in front of the round reach into the tile
        if (scan) {
            // the halo: the span_max - 1 positions in front of the tile, as far as they are of the document that holds g0
            uint32_t r = 0;
            if (threadIdx.x < 64u) {
                const uint64_t j = threadIdx.x + 1u, in_doc = g0 - tile.start_lo;
                if (j < a.span_max && j <= in_doc) {
                    const uint32_t d = (uint32_t)(n_lo - 1u), p = (uint32_t)(in_doc - j);
                    if (tkn_start(a, tki_hash(a.s[0], d), p)) {
                        const uint32_t ln = tkn_len(a, tki_hash(a.s[1], d), p);
                        const uint32_t end = tile.count ? tile.rel(0) : TKN_FAR;
                        r = ln > j ? min(ln - (uint32_t)j, end) : 0u;
                    }
                }
                r = (uint32_t)__builtin_amdgcn_readlane((int)tkd_scan_max(r), 63);
                if (threadIdx.x == 0u) s_halo = r;
            }
            __syncthreads();
            carry = s_halo;
        }
        for (uint32_t base = 0; base < len; base += TKN_ROUND) {       // (every thread takes every round: the scans are the block's)
            const uint32_t l = base + threadIdx.x * 4u;
            const uint64_t g = g0 + l;
            const bool full = l + 4u <= len;
            uint32_t id[4], w[4] = {0u, 0u, 0u, 0u}, sl[4] = {0u, 0u, 0u, 0u}, kq[4], pq[4];
            tkn_load4(a.ids, g, g1, full, id);
            if (words) tkn_load4(a.word_ids, g, g1, full, w);
            if (given) tkn_load4_u8(a.sel, g, g1, full, sl);
            tkn_docs(tile, l, len, kq, pq);
            uint32_t tk[4] = {0u, 0u, 0u, 0u}, k_have = TKN_FAR, reach[4] = {0u, 0u, 0u, 0u}, t2[4] = {0u, 0u, 0u, 0u}, t3[4] = {0u, 0u, 0u, 0u};
            bool cov[4] = {false, false, false, false};
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q) {
                if (l + q >= len) break;
                if (kq[q] != k_have) {                  // the document's four t_k
                    k_have = kq[q];
                    const uint32_t d = (uint32_t)(n_lo - 1u + k_have);
#pragma unroll
                    for (uint32_t i = 0; i < 4u; ++i) tk[i] = tki_hash(a.s[i], d);
                }
                t2[q] = tk[2]; t3[q] = tk[3];
                if (given) cov[q] = sl[q] != 0u && !(words && w[q] == TK_WORD_NONE);   // (step 1's second condition)
                else if (by_word) {
                    if (q && w[q] == w[q - 1u] && kq[q] == kq[q - 1u]) cov[q] = cov[q - 1u];
                    else cov[q] = w[q] != TK_WORD_NONE && tkn_covered(a, tk[0], tk[1], w[q]);
                } else if (tkn_start(a, tk[0], pq[q])) {
                    const uint32_t end = kq[q] < tile.count ? tile.rel(kq[q]) : TKN_FAR;
                    reach[q] = min(l + q + tkn_len(a, tk[1], pq[q]), end);
                }
            }
            if (scan) {
                uint32_t own = max(max(reach[0], reach[1]), max(reach[2], reach[3])), total;
                uint32_t m = max(carry, tkn_block_max(own, s_w, &total));
#pragma unroll
                for (uint32_t q = 0; q < 4u; ++q) {
                    m = max(m, reach[q]);
                    cov[q] = m > l + q;
                }
                carry = max(carry, total);
            }
            // step 1 and, REPLACE, step 3
            uint32_t out[4], lab[4], bits = 0;
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q) {
                const bool s = l + q < len && cov[q] && id[q] >= a.num_special;
                out[q] = id[q];
                lab[q] = (uint32_t)a.ignore;
                bits |= (uint32_t)s << (8u * q);
                if (REPLACE && s) {
                    lab[q] = id[q];
                    const uint64_t r = tki_hash(t2[q], pq[q]);
                    if (r < a.mask_q32) { out[q] = a.mask_id; ++n_mask; }
                    else if (r < a.mask_random_q32) {
                        out[q] = a.num_special + (uint32_t)(((uint64_t)tki_hash(t3[q], pq[q]) * a.n_ordinary) >> 32);
                        ++n_rand;
                    }
                    ++n_sel;
                }
            }
            if (l >= len) continue;
            if (full) {
                if (REPLACE) {
                    const tky_u32x4 o = {out[0], out[1], out[2], out[3]}, b = {lab[0], lab[1], lab[2], lab[3]};
                    *reinterpret_cast<tky_u32x4*>(a.out_ids + g) = o;
                    *reinterpret_cast<tky_u32x4*>(a.labels + g) = b;
                }
                if (a.selected) *reinterpret_cast<uint32_t*>(a.selected + g) = bits;
            } else {
                for (uint32_t q = 0; l + q < len; ++q) {
                    if (REPLACE) { a.out_ids[g + q] = out[q]; a.labels[g + q] = (int32_t)lab[q]; }
                    if (a.selected) a.selected[g + q] = (uint8_t)(bits >> (8u * q));
                }
            }
        }
    }
    if (REPLACE) {
        tkn_block_add(a.stat, 0, n_sel, s_w);
        tkn_block_add(a.stat, 1, n_mask, s_w);
        tkn_block_add(a.stat, 2, n_rand, s_w);
    }
}

// ---- b. spans mode, over the selected bytes ----

// What a thread knows of its four ids in the kernels of b: the selected and run-start flags, the documents and positions, and how
// many selected ids (sb) and run starts (rb) of the TILE lie in front of each.  carry: the tile's counts in front of the round,
// packed (selected | run starts << 16: a tile has at most 4096 of each); it comes back with the round's added.
struct TknRound {
    uint32_t f[4], rs[4], kq[4], pq[4], sb[4], rb[4];
};
__device__ __forceinline__ uint32_t tkn_round(const TkNoiseArgs& a, const TkyTile<2>& tile, uint64_t g0, uint64_t g1, uint32_t l, uint32_t* s_w,
                                              uint32_t carry, TknRound* r) {
    const uint32_t len = (uint32_t)(g1 - g0);
    const uint64_t g = g0 + l;
    tkn_load4_u8(a.selected, g, g1, l + 4u <= len, r->f);
    tkn_docs(tile, l, len, r->kq, r->pq);
    uint32_t prev = l < len && g > 0u && r->pq[0] != 0u ? a.selected[g - 1u] : 0u, own = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
        const bool in = l + q < len;
        r->f[q] = in && r->f[q] ? 1u : 0u;
        r->rs[q] = r->f[q] && (r->pq[q] == 0u || !prev) ? 1u : 0u;
        prev = r->f[q];
        own += r->f[q] | r->rs[q] << 16;
    }
    uint32_t total;
    uint32_t front = carry + tkn_block_sum(own, s_w, &total);
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
        r->sb[q] = front & 0xFFFFu;
        r->rb[q] = front >> 16;
        front += r->f[q] | r->rs[q] << 16;
    }
    return carry + total;
}

// the tiles of the kernels of b: body(tile, g0, g1, n_lo) by every thread of the block, for every tile of the block
template <class F>
__device__ __forceinline__ void tkn_tiles(const TkNoiseArgs& a, F body) {
    const uint64_t N = a.n_ids, D = a.n_docs;
    for (uint64_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        const uint64_t g0 = t * TKN_TILE;
        const uint64_t g1 = N - g0 < TKN_TILE ? N : g0 + TKN_TILE;
        TkyTile<2> tile(a.offs, g0);
        tile.search(D, g0, g1 - 1u);
        const uint64_t n_lo = tile.found(0);
        if (n_lo == 0 || tile.found(1) < n_lo) continue;
        tile.open(n_lo, tile.found(1) - n_lo);
        tile.stage();
        body(tile, t, g0, g1, n_lo);
    }
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_noise_count_kernel(TkNoiseArgs a) {
    __shared__ uint32_t s_w[TKY_BLOCK / 64u];
    tkn_tiles(a, [&](const TkyTile<2>& tile, uint64_t t, uint64_t g0, uint64_t g1, uint64_t n_lo) {
        const uint32_t len = (uint32_t)(g1 - g0);
        uint32_t carry = 0;
        for (uint32_t base = 0; base < len; base += TKN_ROUND) {
            const uint32_t l = base + threadIdx.x * 4u;
            TknRound r;
            carry = tkn_round(a, tile, g0, g1, l, s_w, carry, &r);
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q) {
                if (l + q >= len || r.pq[q] != 0u) continue;
                // documents start here: the one that holds the id and the empty ones in front of it
                for (uint32_t j = r.kq[q]; j >= 1u && tile.rel(j - 1u) == l + q; --j) {
                    a.doc_sel0[n_lo - 1u + j] = r.sb[q];
                    a.doc_rs0[n_lo - 1u + j] = r.rb[q];
                }
            }
        }
        if (threadIdx.x == 0u) {
            a.tile_sel[t] = carry & 0xFFFFu;
            a.tile_rs[t] = carry >> 16;
        }
    });
}

// the selected ids | run starts in front of where document d starts (d <= D)
__device__ __forceinline__ void tkn_front(const TkNoiseArgs& a, uint64_t d, uint64_t* sb, uint64_t* rb) {
    const uint64_t o = d < a.n_docs ? a.offs[d] : a.n_ids;
    if (o >= a.n_ids) { *sb = a.tile_S[a.n_tiles]; *rb = a.tile_R[a.n_tiles]; return; }
    const uint64_t t = o / TKN_TILE;
    *sb = a.tile_S[t] + a.doc_sel0[d];
    *rb = a.tile_R[t] + a.doc_rs0[d];
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_noise_docs_kernel(TkNoiseArgs a) {
    const uint64_t D = a.n_docs;
    const uint64_t n_iter = (D + 1u + (uint64_t)gridDim.x * TKY_BLOCK - 1u) / ((uint64_t)gridDim.x * TKY_BLOCK);
    for (uint64_t it = 0; it < n_iter; ++it) {
        const uint64_t d = (it * gridDim.x + blockIdx.x) * TKY_BLOCK + threadIdx.x;
        if (d > D) continue;
        uint64_t sb, rb, sb1, rb1;
        tkn_front(a, d, &sb, &rb);
        a.SB[d] = sb;
        a.RB[d] = rb;
        if (d == D) continue;
        tkn_front(a, d + 1u, &sb1, &rb1);
        a.KS[d] = (uint32_t)(sb1 - sb);
        if (rb1 - rb > a.n_sentinels) a.stat[TKN_STAT_DROP] = 1ull;   // (every writer writes the same)
    }
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_noise_drop_kernel(TkNoiseArgs a) {
    __shared__ uint32_t s_w[TKY_BLOCK / 64u];
    if (a.stat[TKN_STAT_DROP] == 0ull) return;                      // (block-uniform: written by the kernel in front)
    tkn_tiles(a, [&](const TkyTile<2>& tile, uint64_t t, uint64_t g0, uint64_t g1, uint64_t n_lo) {
        const uint32_t len = (uint32_t)(g1 - g0);
        const uint64_t S0 = a.tile_S[t], R0 = a.tile_R[t];
        uint32_t carry = 0;
        for (uint32_t base = 0; base < len; base += TKN_ROUND) {
            const uint32_t l = base + threadIdx.x * 4u;
            TknRound r;
            carry = tkn_round(a, tile, g0, g1, l, s_w, carry, &r);
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q) {
                if (l + q >= len || !r.rs[q]) continue;
                const uint64_t d = n_lo - 1u + r.kq[q];
                if (R0 + r.rb[q] - a.RB[d] == a.n_sentinels) a.KS[d] = (uint32_t)(S0 + r.sb[q] - a.SB[d]);   // the first dropped run: one a document
            }
        }
    });
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_noise_lens_kernel(TkNoiseArgs a) {
    __shared__ uint32_t s_w[TKY_BLOCK / 64u];
    const uint64_t D = a.n_docs;
    const uint64_t n_iter = (D + (uint64_t)gridDim.x * TKY_BLOCK - 1u) / ((uint64_t)gridDim.x * TKY_BLOCK);
    const uint32_t fin = a.final_id != TK_JOIN_NONE;
    uint32_t n_sel = 0, n_runs = 0, n_drop = 0;
    for (uint64_t it = 0; it < n_iter; ++it) {          // (every thread stays to the block sums below)
        const uint64_t d = (it * gridDim.x + blockIdx.x) * TKY_BLOCK + threadIdx.x;
        if (d >= D) continue;
        const uint64_t n = a.offs[d + 1u] - a.offs[d], nr = a.RB[d + 1u] - a.RB[d];
        const uint32_t kr = (uint32_t)(nr < a.n_sentinels ? nr : a.n_sentinels), ks = a.KS[d];
        a.in_len[d] = (uint32_t)(n - ks + kr);
        a.tg_len[d] = ks + kr + fin;
        n_sel += ks; n_runs += kr; n_drop += (uint32_t)(nr - kr);
    }
    tkn_block_add(a.stat, 0, n_sel, s_w);
    tkn_block_add(a.stat, 1, n_runs, s_w);
    tkn_block_add(a.stat, 2, n_drop, s_w);
}

// element at of inputs_d (tg == 0) or targets_d: the split output and its place in joined_d
__device__ __forceinline__ void tkn_put(const TkNoiseArgs& a, uint64_t in_off, uint64_t tg_off, uint64_t in_n, bool tg, uint64_t at, uint32_t v) {
    if (a.split) {
        const uint64_t p = (tg ? tg_off : in_off) + at;
        if (p < (tg ? a.n_targets : a.n_inputs)) (tg ? a.targets : a.inputs)[p] = v;
    }
    if (a.joined) {
        const uint64_t p = in_off + tg_off + (tg ? in_n : 0u) + at;
        if (p < a.n_inputs + a.n_targets) {
            a.joined_ids[p] = v;
            a.joined_labels[p] = tg ? (int32_t)v : a.ignore;
        }
    }
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_noise_fill_kernel(TkNoiseArgs a) {
    __shared__ uint32_t s_w[TKY_BLOCK / 64u];
    tkn_tiles(a, [&](const TkyTile<2>& tile, uint64_t t, uint64_t g0, uint64_t g1, uint64_t n_lo) {
        const uint32_t len = (uint32_t)(g1 - g0);
        const uint64_t S0 = a.tile_S[t], R0 = a.tile_R[t];
        uint32_t carry = 0;
        for (uint32_t base = 0; base < len; base += TKN_ROUND) {
            const uint32_t l = base + threadIdx.x * 4u;
            TknRound r;
            uint32_t id[4];
            tkn_load4(a.ids, g0 + l, g1, l + 4u <= len, id);
            carry = tkn_round(a, tile, g0, g1, l, s_w, carry, &r);
            uint32_t k_have = TKN_FAR, ks = 0;
            uint64_t in_off = 0, tg_off = 0, in_n = 0, SBd = 0, RBd = 0;
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q) {
                if (l + q >= len) break;
                if (r.kq[q] != k_have) {
                    k_have = r.kq[q];
                    const uint64_t d = n_lo - 1u + k_have;
                    in_off = a.in_off[d]; tg_off = a.tg_off[d]; in_n = a.in_off[d + 1u] - in_off;
                    SBd = a.SB[d]; RBd = a.RB[d]; ks = a.KS[d];
                }
                const uint64_t sb = S0 + r.sb[q] - SBd, rb = R0 + r.rb[q] - RBd;   // selected ids | run starts of the document in front of the id
                const uint64_t run = rb + r.rs[q] - 1u;                            // (of a selected id: its run)
                if (r.f[q] && run < a.n_sentinels) {
                    if (r.rs[q]) {
                        const uint32_t sentinel = a.desc ? a.sentinel_first - (uint32_t)run : a.sentinel_first + (uint32_t)run;
                        tkn_put(a, in_off, tg_off, in_n, false, r.pq[q] - sb + rb, sentinel);
                        tkn_put(a, in_off, tg_off, in_n, true, sb + rb, sentinel);
                    }
                    tkn_put(a, in_off, tg_off, in_n, true, sb + run + 1u, id[q]);
                } else {
                    const uint64_t kept = sb < ks ? sb : ks, kr = rb < a.n_sentinels ? rb : a.n_sentinels;
                    tkn_put(a, in_off, tg_off, in_n, false, r.pq[q] - kept + kr, id[q]);
                }
            }
        }
    });
    // the documents' own elements: the final id, joined_offsets
    const uint64_t D = a.n_docs;
    for (uint64_t d = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; d <= D; d += (uint64_t)gridDim.x * TKY_BLOCK) {
        const uint64_t in_off = a.in_off[d], tg_off = a.tg_off[d];
        if (a.joined) a.joined_offs[d] = in_off + tg_off;
        if (d < D && a.final_id != TK_JOIN_NONE) {
            const uint64_t tg_n = a.tg_off[d + 1u] - tg_off;
            if (tg_n) tkn_put(a, in_off, tg_off, a.in_off[d + 1u] - in_off, true, tg_n - 1u, a.final_id);
        }
    }
}

hipError_t tk_launch_noise_replace(const TkNoiseArgs& a, hipStream_t s) {
    if (a.n_ids == 0 || a.n_docs == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_noise_select_kernel<1>, dim3(tky_blocks(a.n_ids, TKN_GRID, TKN_TILE)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}
hipError_t tk_launch_noise_select(const TkNoiseArgs& a, hipStream_t s) {
    if (a.n_ids == 0 || a.n_docs == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_noise_select_kernel<0>, dim3(tky_blocks(a.n_ids, TKN_GRID, TKN_TILE)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}
hipError_t tk_launch_noise_count(const TkNoiseArgs& a, hipStream_t s) {
    if (a.n_ids == 0 || a.n_docs == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_noise_count_kernel, dim3(tky_blocks(a.n_ids, TKN_GRID, TKN_TILE)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}
hipError_t tk_launch_noise_docs(const TkNoiseArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(tk_noise_docs_kernel, dim3(tky_blocks(a.n_docs + 1u, 1u << 16)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}
hipError_t tk_launch_noise_drop(const TkNoiseArgs& a, hipStream_t s) {
    if (a.n_ids == 0 || a.n_docs == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_noise_drop_kernel, dim3(tky_blocks(a.n_ids, TKN_GRID, TKN_TILE)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}
hipError_t tk_launch_noise_lens(const TkNoiseArgs& a, hipStream_t s) {
    if (a.n_docs == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_noise_lens_kernel, dim3(tky_blocks(a.n_docs, TKN_GRID)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}
hipError_t tk_launch_noise_fill(const TkNoiseArgs& a, hipStream_t s) {
    const uint64_t by_ids = (a.n_ids + TKN_TILE - 1) / TKN_TILE, by_docs = (a.n_docs + TKY_BLOCK) / TKY_BLOCK;
    const uint64_t blocks = by_ids > by_docs ? by_ids : by_docs;
    hipLaunchKernelGGL(tk_noise_fill_kernel, dim3((uint32_t)(blocks < TKN_GRID ? blocks : TKN_GRID)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}
