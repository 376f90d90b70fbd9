// tk_specials.hip -- gfx950 kernels of the specials pass (include/tekken_hip.h tk_specials_split_device).
//
// No reference equivalent: the reference passes an empty allowed_special set (src/tekkenizer.rs:384-386), so "[INST]" in text
// stays text.  The packed text of D documents in; the occurrences of the context's special-token strings found (leftmost-longest,
// non-overlapping, per document), and what tk_encode_parts_device_join takes out: the text without them, cut into parts, with
// the control id of every part.  The candidate kernel reads every text byte once and the compaction moves every kept byte
// once: the bar of both is HBM.  Everything else is per candidate, per match or per document.
//
//   a. tk_specials_cand_kernel<WRITE>: a block takes tiles of TKS_TILE text bytes, staged in LDS with the TKS_MAXLEN - 1 bytes
//      behind them (16-byte loads at any byte where 16 bytes lie inside the text, single bytes at its end: nothing outside
//      [bytes, bytes + n_bytes) is read).  A thread owns 16 consecutive positions, one 16-byte LDS read.  A byte outside the
//      256-bit first-byte mask of the match set costs one test.  At any other the byte trie is walked (an open-addressed table of
//      (node, byte) -> node, a probe or two a byte): the work is bounded by the longest string, not by the number of strings.
//      The longest terminal of the match set wins.  Which document holds it is asked only by a tile that has such a position
//      (__syncthreads_or): two 64-ary wave searches over doc_offs for the documents of the tile's first and last byte, then one
//      binary search among those few per candidate; where the string crosses the document's end the walk is repeated up to
//      that end.  What a walk found stays in LDS for the thread's later steps: one walk a position and launch.  WRITE = 0 counts the candidates of a tile; tk_launch_scan over the counts; the host reads NC; WRITE = 1
//      skips the tiles without a candidate, walks the others again and writes (pos, len, id, document) in position order: a
//      wave scan of the threads' counts, the waves ordered through LDS.
//   b. The choice among overlapping candidates.  nxt(c) = the first candidate at or behind pos_c + len_c (a galloping search
//      forward, then a binary one).  A candidate lies inside its document, so where no later candidate of the document is left
//      nxt(c) is the first candidate of a later document -- which is a match, because the walk of the definition cannot jump
//      over a document's first candidate.  The matches of the whole batch are therefore ONE chain 0, nxt(0), nxt(nxt(0)), ..., NC,
//      which tk_launch_chain_rounds marks and numbers (tk_rowfit.hip: the pointer doubling is shared, not copied).
//      tk_specials_mark_kernel: flen = the length of a match, 0 of another candidate, and the first RAISE match (atomicMin);
//      tk_launch_scan over flen: the bytes removed in front of every candidate.  The host reads M, n_removed and the RAISE word.
//   c. The part tables need no scan: match r of document d is part d * (1 + eos) + r + 1, document d's first part is
//      d * (1 + eos) + (matches in front of d), one binary search per document over the matches' positions.
//      tk_specials_matches_kernel: one thread a match; tk_specials_docs_kernel: one thread a document.
//   d. tk_specials_compact_kernel: the join / regroup kernel shape (tk_layout.h) over bytes.  The text behind match r - 1 is
//      segment r; seg_out is non-decreasing with ties where matches are adjacent, and the segment that holds an output byte is
//      the LAST one that starts at or before it.  A block takes tiles of TKS_CTILE output bytes; two wave searches; the starts
//      inside the tile go to LDS with every segment's source start beside them; a thread resolves 16 consecutive bytes: ONE
//      16-byte load at any byte where the 16 lie in one segment (the removed strings leave source and destination mutually
//      misaligned), a walk over ties otherwise; one 16-byte store.  Every byte is written exactly once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tk_kernels.h"
#include "tk_layout.h"

#define TKS_UNMARKED 0xFFFFFFFFu
#define TKS_STAGED (TKS_TILE + 256u)   /* a tile and its look-ahead, in whole 16-byte units */
#define TKS_CTILE (4u * TKY_TILE)      /* output bytes of a block's tile of the compaction: 64 a thread */

typedef uint32_t __attribute__((ext_vector_type(4), aligned(1))) tks_u32x4_a1;   /* a 16-byte load of text at any byte */

// the child of `node` under byte b, or TKS_NONE
__device__ __forceinline__ uint32_t tks_edge(const TkSpecialsArgs& a, uint32_t node, uint32_t b) {
    const uint32_t key = node << 8 | b;
    for (uint32_t slot = tks_edge_slot(key, a.edge_mask);; slot = (slot + 1u) & a.edge_mask) {
        const uint64_t e = a.edges[slot];
        if (e == 0) return TKS_NONE;                    // (the table is at most half full: an empty entry ends every probe)
        if ((uint32_t)(e >> 32) == key + 1u) return (uint32_t)e;
    }
}

// the longest string of the match set that is a prefix of p[0 .. limit): its length (0: none) and *id
__device__ __forceinline__ uint32_t tks_longest(const TkSpecialsArgs& a, const uint8_t* p, uint32_t limit, uint32_t* id) {
    uint32_t node = 0, best = 0;
    for (uint32_t k = 0; k < limit; ++k) {
        node = tks_edge(a, node, p[k]);
        if (node == TKS_NONE) break;
        const uint32_t t = a.term[node];
        if (t == TKS_NONE) continue;
        const uint32_t e = a.eff[t];
        if (e != TKS_NONE) { best = k + 1u; *id = e; }
    }
    return best;
}

// The document of the candidate of raw length `len` at text position gp, and the candidate inside it: its length (0: none).  n0 /
// n1: the documents that start at or before the tile's first / last byte -- the LAST document that starts at or before gp holds it
__device__ __forceinline__ uint32_t tks_in_document(const TkSpecialsArgs& a, const uint8_t* s, uint32_t len, uint64_t gp, uint64_t n0,
                                                    uint64_t n1, uint32_t* id, uint32_t* doc) {
    const uint64_t n = n0 + tky_count_le(a.doc_offs + n0, n1 - n0, gp);
    if (n == 0) return 0;                               // (offsets that do not start at 0: no document, no match)
    const uint64_t end = a.doc_offs[n];
    if (end <= gp) return 0;                            // (offsets that do not reach n_bytes)
    if (gp + len > end) len = tks_longest(a, s, (uint32_t)(end - gp), id);   // cut by the document's end: the longest that fits
    *doc = (uint32_t)(n - 1u);
    return len;
}

template <int WRITE>
__global__ __launch_bounds__(TKY_BLOCK) void tk_specials_cand_kernel(TkSpecialsArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_b[TKS_STAGED];
    __shared__ uint32_t s_first[8];
    __shared__ uint32_t s_wsum[TKY_BLOCK / 64];
    __shared__ uint32_t s_res[TKS_TILE];                // what begins at a position: len | id << 8 (TKS_RAISE stays bit 31); only its own thread reads it
    __shared__ uint64_t s_docs[2];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x < 8u) s_first[threadIdx.x] = a.first[threadIdx.x];
    if (WRITE && blockIdx.x == 0 && threadIdx.x == 0u) a.cpos[a.n_cand] = a.n_bytes;
    for (uint64_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        if (WRITE && a.tile_pos[t + 1u] == a.tile_pos[t]) continue;   // (block-uniform: a tile without a candidate is not read again)
        const uint64_t g0 = t * TKS_TILE;
        const uint32_t avail = a.n_bytes - g0 < TKS_STAGED ? (uint32_t)(a.n_bytes - g0) : TKS_STAGED;
        const uint32_t len = avail < TKS_TILE ? avail : TKS_TILE;
        __syncthreads();                                // (the previous tile's readers are done)
        for (uint32_t off = threadIdx.x * 16u; off < avail; off += TKY_BLOCK * 16u) {
            if (off + 16u <= avail) {
                *reinterpret_cast<tky_u32x4*>(s_b + off) = *reinterpret_cast<const tks_u32x4_a1*>(a.bytes + g0 + off);
            } else {
                for (uint32_t q = off; q < avail; ++q) s_b[q] = a.bytes[g0 + q];   // the last bytes of the text
            }
        }
        __syncthreads();
        // the thread's 16 positions: which of them begin with a first byte of the match set
        const uint32_t p0 = threadIdx.x * 16u;
        uint32_t hot = 0;
        if (p0 < len) {
            const tky_u32x4 w = *reinterpret_cast<const tky_u32x4*>(s_b + p0);
            const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (uint32_t q = 0; q < 16u; ++q) {
                const uint32_t b = (ws[q >> 2] >> (8u * (q & 3u))) & 255u;
                hot |= ((s_first[b >> 5] >> (b & 31u)) & 1u) << q;
            }
            if (p0 + 16u > len) hot &= (1u << (len - p0)) - 1u;   // (what lies behind the text was not staged)
        }
        uint32_t raw = 0;                               // ... and at which a string of the match set begins, documents aside
        for (uint32_t h = hot; h; h &= h - 1u) {
            const uint32_t q = (uint32_t)__builtin_ctz(h), p = p0 + q;
            uint32_t id = 0;
            const uint32_t l = tks_longest(a, s_b + p, avail - p < TKS_MAXLEN ? avail - p : TKS_MAXLEN, &id);
            if (l) { raw |= 1u << q; s_res[p] = l | (id & ~TKS_RAISE) << 8 | (id & TKS_RAISE); }
        }
        // only a tile that has one asks which documents it holds: two wave searches, and a search among those few per candidate
        const bool any = __syncthreads_or(raw != 0u) != 0;
        if (any) {
            if (wave < 2u) {
                const uint64_t c = tky_wave_count_le(a.doc_offs, a.n_docs, wave == 0u ? g0 : g0 + len - 1u);
                if (lane == 0u) s_docs[wave] = c;
            }
            __syncthreads();
        }
        const uint64_t n0 = any ? s_docs[0] : 0u, n1 = any ? s_docs[1] : 0u;
        uint32_t n = 0, keep = 0;                       // the thread's candidates, and at which of its positions
        uint64_t c = 0;
        for (int pass = 0; pass < (WRITE ? 2 : 1); ++pass) {   // counted; then -- WRITE -- written in position order
            for (uint32_t h = pass ? keep : raw; h; h &= h - 1u) {
                const uint32_t q = (uint32_t)__builtin_ctz(h), p = p0 + q;
                const uint32_t r = s_res[p], l0 = r & 255u;
                uint32_t id = ((r >> 8) & 0x7FFFFFu) | (r & TKS_RAISE), doc = 0;
                const uint32_t l = tks_in_document(a, s_b + p, l0, g0 + p, n0, n1, &id, &doc);
                if (l == 0u) continue;
                if (!pass) {                            // (cut by its document's end: what the second pass reads is what fits)
                    if (l != l0) s_res[p] = l | (id & ~TKS_RAISE) << 8 | (id & TKS_RAISE);
                    ++n; keep |= 1u << q;
                    continue;
                }
                if (c >= a.n_cand) continue;            // (c < n_cand always, where the counts are of the same text)
                a.cpos[c] = g0 + p;
                a.clen[c] = l;
                a.cid[c] = id;
                a.cdoc[c] = doc;
                ++c;
            }
            if (pass) break;
            const uint32_t incl = tkd_scan_incl(n);
            if (lane == 63u) s_wsum[wave] = incl;
            __syncthreads();
            uint32_t before = 0, total = 0;
#pragma unroll
            for (uint32_t w = 0; w < TKY_BLOCK / 64; ++w) {
                before += w < wave ? s_wsum[w] : 0u;
                total += s_wsum[w];
            }
            if (!WRITE && threadIdx.x == 0u) a.tile_cnt[t] = total;
            if (WRITE) c = a.tile_pos[t] + (before + incl - n);
        }
    }
}

__global__ void tk_specials_count_end_kernel(TkSpecialsArgs a) { a.stat[0] = a.tile_pos[a.n_tiles]; }

__global__ __launch_bounds__(TKY_BLOCK) void tk_specials_nxt_kernel(TkSpecialsArgs a) {
    const uint64_t NC = a.n_cand;
    for (uint64_t v = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; v <= NC; v += (uint64_t)gridDim.x * TKY_BLOCK) {
        a.row[v] = v ? TKS_UNMARKED : 0u;
        if (v == NC) { a.jump[v] = NC; continue; }      // (the sentinel: to itself, in 0 steps)
        const uint64_t key = a.cpos[v] + a.clen[v];
        uint64_t lo = v + 1u, w = 1;                    // every candidate in front of lo starts before key
        while (lo + w - 1u < NC && a.cpos[lo + w - 1u] < key) { lo += w; w <<= 1; }
        const uint64_t hi = lo + w - 1u < NC ? lo + w - 1u : NC;   // cpos[hi] >= key, or hi is the sentinel
        const uint64_t nxt = lo + tky_count_lt(a.cpos + lo, hi - lo, key);
        a.jump[v] = nxt | 1ull << 32;
    }
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_specials_mark_kernel(TkSpecialsArgs a) {
    const uint64_t NC = a.n_cand;
    for (uint64_t c = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; c < NC; c += (uint64_t)gridDim.x * TKY_BLOCK) {
        const bool m = a.row[c] != TKS_UNMARKED;
        a.flen[c] = m ? a.clen[c] : 0u;
        if (m && (a.cid[c] & TKS_RAISE)) atomicMin(a.stat + 1, (unsigned long long)c);
    }
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_specials_matches_kernel(TkSpecialsArgs a) {
    const uint64_t M = a.n_matches, per = 1u + a.eos_part;
    for (uint64_t r = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; r <= M; r += (uint64_t)gridDim.x * TKY_BLOCK) {
        if (r == 0) { a.seg_out[0] = 0; a.seg_src[0] = 0; continue; }
        const uint64_t c = a.open[r - 1u];              // match r - 1, and the text behind it: segment r
        const uint64_t pos = a.cpos[c], l = a.clen[c];
        const uint64_t src = pos + l, out = src - (a.remc[c] + l);
        a.mpos[r - 1u] = pos;
        a.seg_src[r] = src;
        a.seg_out[r] = out;
        const uint64_t p = (uint64_t)a.cdoc[c] * per + r;
        a.part_ctrl[p] = a.cid[c] & ~TKS_RAISE;
        a.part_offs[p] = out;
        if (a.part_src) a.part_src[p] = src;
    }
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_specials_docs_kernel(TkSpecialsArgs a) {
    const uint64_t D = a.n_docs, M = a.n_matches, per = 1u + a.eos_part;
    for (uint64_t d = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; d <= D; d += (uint64_t)gridDim.x * TKY_BLOCK) {
        const uint64_t o = a.doc_offs[d];
        const uint64_t mb = M ? tky_count_lt(a.mpos, M, o) : 0u;   // the matches of the documents in front of d
        const uint64_t rem = mb < M ? a.remc[a.open[mb]] : a.n_removed;
        const uint64_t p = d * per + mb;
        a.conv_offs[d] = p;
        if (d && a.eos_part) {                          // the closing part of document d - 1: empty, where d begins
            a.part_ctrl[p - 1u] = a.eos;
            a.part_offs[p - 1u] = o - rem;
            if (a.part_src) a.part_src[p - 1u] = o;
        }
        if (d == D) { a.part_offs[p] = a.n_bytes - a.n_removed; continue; }
        a.part_ctrl[p] = a.bos;
        a.part_offs[p] = o - rem;
        if (a.part_src) a.part_src[p] = o;
    }
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_specials_compact_kernel(TkSpecialsArgs a) {
    __shared__ uint64_t s_src[TKY_CAP + 1];             // source starts of the tile's segments: [0] is the one that holds g0
    const uint64_t K = a.n_matches + 1u, N = a.n_bytes - a.n_removed;
    const uint64_t n_tiles = (N + TKS_CTILE - 1) / TKS_CTILE;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t g0 = t * TKS_CTILE;
        const uint64_t g1 = N - g0 < TKS_CTILE ? N : g0 + TKS_CTILE;
        TkyTile<2> tile(a.seg_out, g0);
        tile.search(K, g0, g1 - 1u);                    // starts at or before the tile's first | last byte
        const uint64_t n_lo = tile.found(0);            // (block-uniform, as everything up to the unit loop; >= 1: seg_out[0] == 0)
        if (n_lo == 0 || tile.found(1) < n_lo) continue;
        tile.open(n_lo, tile.found(1) - n_lo);          // starts in (g0, g1): segments n_lo .. n_lo + count - 1, empty ones included
        tile.stage([&](uint32_t j, uint64_t k) { s_src[j] = a.seg_src[k]; });
        auto src_of = [&](uint32_t j) -> uint64_t { return tile.lds ? s_src[j] : a.seg_src[n_lo - 1u + j]; };
        const uint32_t len = (uint32_t)(g1 - g0);
        for (uint32_t l = threadIdx.x * 16u; l < len; l += TKY_BLOCK * 16u) {
            const uint64_t g = g0 + l;
            uint32_t k = tile.count_le(l);
            uint64_t sb = src_of(k);
            int64_t start = tile.start_of(k);
            // the common unit: 16 bytes of one segment -- one load of 16 bytes at any byte, one aligned store
            if (l + 16u <= len && (k == tile.count || tile.rel(k) >= l + 16u)) {
                const uint64_t s = sb + (uint64_t)((int64_t)l - start);
                *reinterpret_cast<tky_u32x4*>(a.out_bytes + g) = *reinterpret_cast<const tks_u32x4_a1*>(a.bytes + s);
                continue;
            }
            uint32_t v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (uint32_t q = 0; q < 16u; ++q) {
                if (l + q >= len) break;
                if (k < tile.count && tile.rel(k) <= l + q) {   // another segment (over ties too: the LAST that starts at or before the byte)
                    do ++k; while (k < tile.count && tile.rel(k) <= l + q);
                    sb = src_of(k);
                    start = (int64_t)tile.rel(k - 1u);
                }
                const uint64_t s = sb + (uint64_t)((int64_t)(l + q) - start);
                v[q >> 2] |= (uint32_t)a.bytes[s] << (8u * (q & 3u));
            }
            if (l + 16u <= len) {
                const tky_u32x4 x = {v[0], v[1], v[2], v[3]};
                *reinterpret_cast<tky_u32x4*>(a.out_bytes + g) = x;
            } else {
                for (uint32_t q = 0; l + q < len; ++q) a.out_bytes[g + q] = (uint8_t)(v[q >> 2] >> (8u * (q & 3u)));   // the last N % 16 bytes
            }
        }
    }
}

hipError_t tk_launch_specials_cand(const TkSpecialsArgs& a, int write, hipStream_t s) {
    if (a.n_tiles == 0) return hipSuccess;
    const dim3 grid(tky_blocks(a.n_tiles, 1u << 20, 1));
    if (write) hipLaunchKernelGGL(tk_specials_cand_kernel<1>, grid, dim3(TKY_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(tk_specials_cand_kernel<0>, grid, dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_specials_count_end(const TkSpecialsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(tk_specials_count_end_kernel, dim3(1), dim3(1), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_specials_nxt(const TkSpecialsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(tk_specials_nxt_kernel, dim3(tky_blocks(a.n_cand + 1u, 1u << 16)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_specials_mark(const TkSpecialsArgs& a, hipStream_t s) {
    if (a.n_cand == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_specials_mark_kernel, dim3(tky_blocks(a.n_cand, 1u << 16)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_specials_matches(const TkSpecialsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(tk_specials_matches_kernel, dim3(tky_blocks(a.n_matches + 1u, 1u << 16)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_specials_docs(const TkSpecialsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(tk_specials_docs_kernel, dim3(tky_blocks(a.n_docs + 1u, 1u << 16)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_specials_compact(const TkSpecialsArgs& a, hipStream_t s) {
    if (a.n_bytes == a.n_removed) return hipSuccess;
    hipLaunchKernelGGL(tk_specials_compact_kernel, dim3(tky_blocks(a.n_bytes - a.n_removed, 1u << 20, TKS_CTILE)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}
