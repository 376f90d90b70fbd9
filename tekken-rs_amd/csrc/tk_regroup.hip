// tk_regroup.hip -- gfx950 kernels of the regroup pass (include/tekken_hip.h tk_regroup_from_ids_device).
//
// No reference equivalent.  Ragged ids + offsets (and optionally a second int32 stream with the same offsets: labels, and a keep
// mask) in; the kept documents in another order, ragged again (ids, offsets, labels, perm), and the boundaries of the batches
// that a padded-token budget cuts that order into.  The gather moves every id once: the bar is HBM.  Everything else is per
// document.
//
//   a. tk_regroup_select_kernel: one thread a document: the kept flag, the drop counts under the first test that fails, the ids of
//      the kept documents and the longest of them (one atomic a wave each).  tk_launch_scan over the flags, and
//      tk_regroup_compact_kernel: kept[fpos[d]] = d.  The host reads K, the sum, the counts, the longest, where the offsets end.
//   b. The order.  KEEP: perm = kept.  Else a stable least-significant-digit radix sort of (key, document) pairs, 8 bits a pass:
//      tk_regroup_hist_kernel counts the digits of a block's TKG_CHUNK consecutive pairs into hist[digit * blocks + block]
//      (digit-major, so that its exclusive scan -- tk_launch_scan -- is where every block puts every digit), and
//      tk_regroup_scatter_kernel walks the same chunk in element order, 256 pairs a round: the rank of a pair among the equal
//      digits of its wave is a popcount over the lanes in front of it (eight ballots match the digit), the waves of a round are
//      ordered through a count per wave and digit in LDS, and the rounds through the running base of every digit.  A pass
//      therefore keeps the order of equal digits, which is all LSD needs.  Keys: LENGTH n_d (DESC: longest - n_d, which reverses
//      the lengths and not the ties); SHUFFLE h(seed, d); GROUPED the SHUFFLE sort, then the pairs (length key, shuffle rank)
//      sorted by the length key and then by rank / window -- the least significant part first.  The host knows the largest key
//      of every sort (the longest kept document, K) and runs only the passes below its highest set bit.
//      tk_regroup_perm_kernel: perm, m_k = n_perm[k], src[k] = id_offs[perm[k]]; tk_launch_scan over m: the new offsets.
//   c. tk_regroup_gather_kernel: the join / rowfit kernel shape (tk_layout.h).  A block takes tiles of TKY_TILE OUTPUT positions;
//      two wave searches over the new offsets (non-decreasing, with ties where documents are empty: the search returns the LAST
//      document that starts at or before a position, which is the one that holds it); the starts inside the tile go to LDS with
//      every document's source start beside them; a thread resolves 4 consecutive positions: one binary search, then ONE
//      16-byte load of ids (and one of labels), 4-byte aligned, where the 4 lie in one document, or a walk that steps over ties
//      as the search does.  One 16-byte store per output.  Every element is written exactly once.
//   d. Batches.  nxt(i): the smallest k > i at which a batch opened at i closes, else K.  The padded cost (k - i + 1) *
//      max(m_i .. m_k) does not decrease with k, so "closes at k" holds from nxt(i) on and nowhere before.  tk_regroup_pyr_kernel
//      builds a maximum pyramid over m (64 entries under one); tk_regroup_nxt_kernel walks it: up while the position is aligned
//      and the whole block under an entry still fits, down where it does not -- at most 63 steps a level each way, whatever the
//      lengths are (a run of empty documents without max_docs costs no more than any other).  The chain 0, nxt(0), nxt(nxt(0)),
//      ... is marked and numbered by tk_launch_chain_rounds (tk_rowfit.hip: the pointer doubling is shared, not copied), and
//      tk_regroup_batches_kernel writes batch_offsets / batch_rowlen and sums n_oversize and the padded size.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tk_kernels.h"
#include "tk_layout.h"

#define TKG_UNMARKED 0xFFFFFFFFu

// the wave's sum of a 64-bit v into *dst with one atomic (none where it is 0); every lane of the wave calls it
__device__ __forceinline__ void tkg_wave_add64(unsigned long long* dst, unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63u) == 0u && v) atomicAdd(dst, v);
}

// step 2 of the definition: a bijection of the 32-bit d
__device__ __forceinline__ uint32_t tkg_hash(uint32_t seed, uint32_t d) {
    uint32_t x = d * 0x9E3779B1u + seed;
    x ^= x >> 16; x *= 0x85EBCA6Bu;
    x ^= x >> 13; x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_regroup_select_kernel(TkRegroupArgs a) {
    const uint64_t D = a.n_docs;
    const uint64_t n_iter = (D + (uint64_t)gridDim.x * TKY_BLOCK - 1u) / ((uint64_t)gridDim.x * TKY_BLOCK);
    uint32_t masked = 0, too_short = 0, too_long = 0, huge = 0, longest = 0;
    unsigned long long sum = 0;
    for (uint64_t it = 0; it < n_iter; ++it) {          // (every lane stays to the wave sums below)
        const uint64_t d = (it * gridDim.x + blockIdx.x) * TKY_BLOCK + threadIdx.x;
        if (d >= D) continue;
        const uint64_t n = a.id_offs[d + 1] - a.id_offs[d];
        bool k = false;
        if (n >> 32) ++huge;                            // (the call is refused: no later kernel reads through these offsets)
        else if (a.keep && !a.keep[d]) ++masked;
        else if (n < a.min_len) ++too_short;
        else if (a.max_len && n > a.max_len) ++too_long;
        else { k = true; sum += n; longest = max(longest, (uint32_t)n); }
        a.flag[d] = k;
    }
    tky_wave_add(a.stat + 0, masked);
    tky_wave_add(a.stat + 1, too_short);
    tky_wave_add(a.stat + 2, too_long);
    tkg_wave_add64(a.stat + 3, sum);
    tky_wave_max(a.stat + 6, longest);
    tky_wave_add(a.stat + 7, huge);
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_regroup_compact_kernel(TkRegroupArgs a) {
    const uint64_t D = a.n_docs;
    for (uint64_t d = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; d <= D; d += (uint64_t)gridDim.x * TKY_BLOCK) {
        if (d == D) { a.stat[4] = a.fpos[D]; a.stat[5] = a.id_offs[D]; }
        else if (a.flag[d]) a.kept[a.fpos[d]] = (uint32_t)d;
    }
}

template <int WHAT>
__global__ __launch_bounds__(TKY_BLOCK) void tk_regroup_keys_kernel(TkRegroupArgs a) {
    for (uint64_t k = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; k < a.n_kept; k += (uint64_t)gridDim.x * TKY_BLOCK) {
        if (WHAT == 2) {                                // the group of shuffle rank val
            const uint32_t r = a.val_in[k];
            a.key_out[k] = r / a.window;
            a.val_out[k] = r;
            continue;
        }
        const uint32_t d = WHAT == 0 ? a.kept[k] : a.val_in[k];
        const uint32_t n = (uint32_t)(a.id_offs[d + 1u] - a.id_offs[d]);
        if (WHAT == 0 && a.order != TK_REGROUP_ORDER_LENGTH) a.key_out[k] = tkg_hash(a.seed, d);
        else a.key_out[k] = a.desc ? a.longest - n : n; // (descending lengths, ties still in the order they came in)
        a.val_out[k] = WHAT == 0 ? d : (uint32_t)k;
    }
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_regroup_hist_kernel(TkRegroupArgs a, uint32_t shift) {
    __shared__ uint32_t s_h[256];
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t c0 = (uint64_t)blockIdx.x * TKG_CHUNK;
    const uint64_t c1 = a.n_kept - c0 < TKG_CHUNK ? a.n_kept : c0 + TKG_CHUNK;
    for (uint64_t i = c0 + threadIdx.x; i < c1; i += TKY_BLOCK) atomicAdd(&s_h[(a.key_in[i] >> shift) & 255u], 1u);
    __syncthreads();
    a.hist[(uint64_t)threadIdx.x * gridDim.x + blockIdx.x] = s_h[threadIdx.x];
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_regroup_scatter_kernel(TkRegroupArgs a, uint32_t shift) {
    __shared__ uint32_t s_base[256];                    // where the block's next pair of every digit goes
    __shared__ uint32_t s_w[TKY_BLOCK / 64][256];       // pairs of every digit in every wave of the round
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    s_base[t] = (uint32_t)a.hpos[(uint64_t)t * gridDim.x + blockIdx.x];
#pragma unroll
    for (uint32_t w = 0; w < TKY_BLOCK / 64; ++w) s_w[w][t] = 0;
    __syncthreads();
    const uint64_t c0 = (uint64_t)blockIdx.x * TKG_CHUNK;
    const uint64_t c1 = a.n_kept - c0 < TKG_CHUNK ? a.n_kept : c0 + TKG_CHUNK;
    for (uint64_t r0 = c0; r0 < c1; r0 += TKY_BLOCK) {  // (block-uniform: every thread reaches the barriers)
        const uint64_t i = r0 + t;
        const bool active = i < c1;
        const uint32_t key = active ? a.key_in[i] : 0u, val = active ? a.val_in[i] : 0u;
        const uint32_t dg = (key >> shift) & 255u;
        unsigned long long same = __ballot(active);     // the wave's pairs with this lane's digit
#pragma unroll
        for (uint32_t bit = 0; bit < 8u; ++bit) {
            const bool one = (dg >> bit) & 1u;
            const unsigned long long b = __ballot(one);
            same &= one ? b : ~b;
        }
        const uint32_t rank = (uint32_t)__builtin_popcountll(same & ((1ull << lane) - 1ull));
        if (active && rank == 0u) s_w[wave][dg] = (uint32_t)__builtin_popcountll(same);
        __syncthreads();
        if (active) {
            uint32_t pos = s_base[dg] + rank;
            for (uint32_t w = 0; w < wave; ++w) pos += s_w[w][dg];
            if (pos < a.n_kept) {                       // (always, where hist is of the same keys)
                a.key_out[pos] = key;
                a.val_out[pos] = val;
            }
        }
        __syncthreads();
        uint32_t tot = 0;                               // thread t is digit t
#pragma unroll
        for (uint32_t w = 0; w < TKY_BLOCK / 64; ++w) { tot += s_w[w][t]; s_w[w][t] = 0; }
        s_base[t] += tot;
        __syncthreads();
    }
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_regroup_perm_kernel(TkRegroupArgs a) {
    for (uint64_t k = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; k < a.n_kept; k += (uint64_t)gridDim.x * TKY_BLOCK) {
        const uint32_t v = a.val_in[k];
        const uint32_t d = a.shuf ? a.shuf[v] : v;
        const uint64_t o = a.id_offs[d];
        a.perm[k] = d;
        a.len[k] = (uint32_t)(a.id_offs[d + 1u] - o);
        a.src[k] = o;
    }
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_regroup_gather_kernel(TkRegroupArgs a) {
    __shared__ uint64_t s_src[TKY_CAP + 1];             // source starts of the tile's documents: [0] is the one that holds g0
    const uint64_t K = a.n_kept, N = a.n_out;
    const uint64_t n_tiles = (N + TKY_TILE - 1) / TKY_TILE;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t g0 = t * TKY_TILE;
        const uint64_t g1 = N - g0 < TKY_TILE ? N : g0 + TKY_TILE;
        TkyTile<2> tile(a.out_offs, g0);
        tile.search(K, g0, g1 - 1u);                    // starts at or before the tile's first | last position
        const uint64_t n_lo = tile.found(0);            // (block-uniform, as everything up to the unit loop; >= 1: out_offs[0] == 0)
        if (n_lo == 0 || tile.found(1) < n_lo) continue;
        tile.open(n_lo, tile.found(1) - n_lo);          // starts in (g0, g1): documents n_lo .. n_lo + count - 1, empty ones included
        tile.stage([&](uint32_t j, uint64_t k) { s_src[j] = a.src[k]; });
        auto src_of = [&](uint32_t j) -> uint64_t { return tile.lds ? s_src[j] : a.src[n_lo - 1u + j]; };
        const uint32_t len = (uint32_t)(g1 - g0);
        for (uint32_t l = threadIdx.x * 4u; l < len; l += TKY_BLOCK * 4u) {
            const uint64_t g = g0 + l;
            uint32_t k = tile.count_le(l);
            uint64_t sb = src_of(k);
            int64_t start = tile.start_of(k);
            uint32_t v[4] = {0u, 0u, 0u, 0u}, lb[4] = {0u, 0u, 0u, 0u};
            // the common unit: 4 positions of one document -- one load of 16 bytes, 4-byte aligned
            if (l + 4u <= len && (k == tile.count || tile.rel(k) >= l + 4u)) {
                const uint64_t s = sb + (uint64_t)((int64_t)l - start);
                tky_gather4(a.ids + s, v);
                if (a.out_lab) tky_gather4(reinterpret_cast<const uint32_t*>(a.lab + s), lb);
            } else {
#pragma unroll
                for (uint32_t q = 0; q < 4u; ++q) {
                    if (l + q >= len) break;
                    if (k < tile.count && tile.rel(k) <= l + q) {   // another document (over ties too: the LAST that starts at or before the position)
                        do ++k; while (k < tile.count && tile.rel(k) <= l + q);
                        sb = src_of(k);
                        start = (int64_t)tile.rel(k - 1u);
                    }
                    const uint64_t s = sb + (uint64_t)((int64_t)(l + q) - start);
                    v[q] = a.ids[s];
                    if (a.out_lab) lb[q] = (uint32_t)a.lab[s];
                }
            }
            if (l + 4u <= len) {
                tky_store<0, 1>(a.out_ids, g, v);
                if (a.out_lab) tky_store<0, 1>(a.out_lab, g, lb);
            } else {
#pragma unroll
                for (uint32_t q = 0; q < 3u; ++q) {     // the last N % 4 elements
                    if (l + q >= len) break;
                    a.out_ids[g + q] = v[q];
                    if (a.out_lab) a.out_lab[g + q] = (int32_t)lb[q];
                }
            }
        }
    }
}

// level `lvl` (>= 1) of the pyramid from the one below it
__global__ __launch_bounds__(TKY_BLOCK) void tk_regroup_pyr_kernel(TkRegroupArgs a, uint32_t lvl) {
    const uint64_t n_in = (a.n_kept + (1ull << (6u * (lvl - 1u))) - 1u) >> (6u * (lvl - 1u));
    const uint64_t n_out = (n_in + TKG_FAN - 1u) / TKG_FAN;
    const uint32_t* in = lvl == 1u ? a.len : a.pyr + a.pyr_at[lvl - 1u];
    uint32_t* out = a.pyr + a.pyr_at[lvl];
    for (uint64_t j = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; j < n_out; j += (uint64_t)gridDim.x * TKY_BLOCK) {
        const uint64_t i0 = j * TKG_FAN, i1 = n_in - i0 < TKG_FAN ? n_in : i0 + TKG_FAN;
        uint32_t m = 0;
        for (uint64_t i = i0; i < i1; ++i) m = max(m, in[i]);
        out[j] = m;
    }
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_regroup_nxt_kernel(TkRegroupArgs a) {
    const uint64_t K = a.n_kept, T = a.max_tokens, cap_docs = a.max_docs;
    for (uint64_t v = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; v <= K; v += (uint64_t)gridDim.x * TKY_BLOCK) {
        a.row[v] = v ? TKG_UNMARKED : 0u;
        if (v == K) { a.jump[v] = K; continue; }        // (the sentinel: to itself, in 0 steps)
        uint32_t mx = a.len[v];
        uint64_t p = v + 1u;                            // documents v .. p - 1 fit one batch
        uint32_t lvl = 0, top = a.n_levels;             // top: the answer lies inside a block of level top + 1 that did not fit
        while (p < K) {
            while (lvl < top && (p & ((1ull << (6u * (lvl + 1u))) - 1u)) == 0u) ++lvl;
            const uint64_t end = K - p < (1ull << (6u * lvl)) ? K : p + (1ull << (6u * lvl));
            const uint32_t bm = lvl ? a.pyr[a.pyr_at[lvl] + (p >> (6u * lvl))] : a.len[p];
            const uint32_t m2 = max(mx, bm);
            const uint64_t cnt = end - v;               // (>= 2; cnt * m2 < 2^64)
            if (!(cnt * m2 > T || (cap_docs && cnt > cap_docs))) { mx = m2; p = end; continue; }
            if (lvl == 0u) break;                       // the batch closes at p
            top = --lvl;
        }
        a.jump[v] = p | 1ull << 32;
        a.bmax[v] = mx;
    }
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_regroup_batches_kernel(TkRegroupArgs a) {
    const uint64_t K = a.n_kept;
    const uint64_t n_iter = (K + 1u + (uint64_t)gridDim.x * TKY_BLOCK - 1u) / ((uint64_t)gridDim.x * TKY_BLOCK);
    uint32_t over = 0;
    unsigned long long padded = 0;
    for (uint64_t it = 0; it < n_iter; ++it) {          // (every lane stays to the wave sums below)
        const uint64_t v = (it * gridDim.x + blockIdx.x) * TKY_BLOCK + threadIdx.x;
        if (v > K) continue;
        const uint32_t b = a.row[v];
        if (b == TKG_UNMARKED) continue;
        if (a.batch_offs) a.batch_offs[b] = v;
        if (v == K) { a.stat[10] = b; continue; }
        const uint64_t cnt = a.open[b + 1u] - v, rl = a.bmax[v];
        if (a.batch_rowlen) a.batch_rowlen[b] = (uint32_t)rl;
        over += cnt * rl > a.max_tokens;
        padded += cnt * rl;
    }
    tky_wave_add(a.stat + 8, over);
    tkg_wave_add64(a.stat + 9, padded);
}

hipError_t tk_launch_regroup_select(const TkRegroupArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(tk_regroup_select_kernel, dim3(tky_blocks(a.n_docs, 2048u)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_regroup_compact(const TkRegroupArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(tk_regroup_compact_kernel, dim3(tky_blocks(a.n_docs + 1u, 1u << 16)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_regroup_keys(const TkRegroupArgs& a, int what, hipStream_t s) {
    if (a.n_kept == 0) return hipSuccess;
    const dim3 grid(tky_blocks(a.n_kept, 1u << 16));
    if (what == 0) hipLaunchKernelGGL(tk_regroup_keys_kernel<0>, grid, dim3(TKY_BLOCK), 0, s, a);
    else if (what == 1) hipLaunchKernelGGL(tk_regroup_keys_kernel<1>, grid, dim3(TKY_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(tk_regroup_keys_kernel<2>, grid, dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

uint32_t tk_regroup_sort_blocks(uint64_t n_kept) { return (uint32_t)((n_kept + TKG_CHUNK - 1u) / TKG_CHUNK); }

hipError_t tk_launch_regroup_hist(const TkRegroupArgs& a, uint32_t shift, hipStream_t s) {
    if (a.n_kept == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_regroup_hist_kernel, dim3(tk_regroup_sort_blocks(a.n_kept)), dim3(TKY_BLOCK), 0, s, a, shift);
    return hipGetLastError();
}

hipError_t tk_launch_regroup_scatter(const TkRegroupArgs& a, uint32_t shift, hipStream_t s) {
    if (a.n_kept == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_regroup_scatter_kernel, dim3(tk_regroup_sort_blocks(a.n_kept)), dim3(TKY_BLOCK), 0, s, a, shift);
    return hipGetLastError();
}

hipError_t tk_launch_regroup_perm(const TkRegroupArgs& a, hipStream_t s) {
    if (a.n_kept == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_regroup_perm_kernel, dim3(tky_blocks(a.n_kept, 1u << 16)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_regroup_gather(const TkRegroupArgs& a, hipStream_t s) {
    if (a.n_out == 0 || a.n_kept == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_regroup_gather_kernel, dim3(tky_blocks(a.n_out, 1u << 20, TKY_TILE)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_regroup_pyramid(const TkRegroupArgs& a, hipStream_t s) {
    for (uint32_t lvl = 1; lvl <= a.n_levels; ++lvl) {
        const uint64_t n_out = (a.n_kept + (1ull << (6u * lvl)) - 1u) >> (6u * lvl);
        hipLaunchKernelGGL(tk_regroup_pyr_kernel, dim3(tky_blocks(n_out, 1u << 16)), dim3(TKY_BLOCK), 0, s, a, lvl);
    }
    return hipGetLastError();
}

hipError_t tk_launch_regroup_nxt(const TkRegroupArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(tk_regroup_nxt_kernel, dim3(tky_blocks(a.n_kept + 1u, 1u << 16)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_regroup_batches(const TkRegroupArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(tk_regroup_batches_kernel, dim3(tky_blocks(a.n_kept + 1u, 2048u)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}
