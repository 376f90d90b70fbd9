// tk_rowfit.hip -- gfx950 kernels of the whole-document rows (include/tekken_hip.h tk_rowfit_from_ids_device).
//
// No reference equivalent: the reference has pad_id() (src/tekkenizer.rs:304) and nothing that uses it.  Ragged ids + offsets
// (and optionally a second int32 stream with the same offsets: labels) in; the documents placed next-fit, in the caller's order
// and never cut, into rows of L (input_ids[n_rows, L], pad elsewhere), labels, position_ids, segment_ids, cu_seqlens /
// max_seqlen over the flattened tensor and doc_start out.  Pure data movement behind a placement that looks sequential and is
// not: the bar is HBM.
//
// The placement (nothing read by the host before its end):
//   1. tk_rowfit_len_kernel: e[d] = min(n_d, L), "has ids", n_truncated; tk_launch_scan over each: E (D + 1 entries), nzp.
//   2. tk_rowfit_nxt_kernel: the row opened at document i holds i .. nxt(i) - 1, nxt(i) = the largest j with E[j] <= E[i] + L:
//      a galloping search forward from i + 1 (a row rarely holds many documents), then a binary one.  nxt(i) > i, nxt(D) = D.
//   3. tk_rowfit_round_kernel, K times: pointer doubling over the chain 0, nxt(0), nxt(nxt(0)), ..., D.  An entry of the jump
//      table is (target, steps): steps is the number of links the jump really takes, at most 2^k in round k and fewer where the
//      chain ends at D before (the sentinel jumps to itself in 0 steps), so row(target) = row(v) + steps is exact for every
//      marked v, in whatever order the lanes of a round run: a mark is the node's position in the chain, whoever writes it
//      writes the same value.  The table is squared from one buffer into the other.  After round k the first 2^(k+1)
//      positions of the chain are marked; the host knows an upper bound of n_rows (two neighbouring rows hold more than L ids)
//      and K from it.
//   4. tk_rowfit_open_kernel: open[row(v)] = v for every marked v: the documents that open a row, increasing, open[n_rows] = D.
//   The host reads n_truncated, row(D) = n_rows, E[D] and id_offs[D] (one copy of the statistics words), sizes the tensors, and then
//   5. tk_rowfit_place_kernel: doc_start[d] = row(v) * L + E[d] - E[v] for the last marked v <= d: a prefix maximum over the
//      wave (tkd_scan_max) and, for the lanes in front of the wave's first mark, one 64-ary wave search over open.  Beside it
//      the document's segment number inside its row and, per row, "has pads".  tk_launch_scan over the latter: padp.
//   6. tk_rowfit_kernel: a block takes a tile of TKY_TILE consecutive OUTPUT positions.  doc_start is non-decreasing with ties
//      (an empty document starts where the next id would go), and the document that holds position g is the LAST one with
//      doc_start <= g -- what the 64-ary wave search returns on ties (tk_layout.h has the argument); g is a pad where it lies
//      at or beyond that document's e.  Two waves search the tile's first and last position; the starts in between go to LDS
//      relative to the tile, beside them id_offs and the segment number of every document of the tile.  A tile with more than
//      TKY_CAP starts reads the same from global memory: decided per block.  A unit is 4 consecutive elements of one row where
//      L % 4 == 0 (one 16-byte store for each int32 output, two for int64), one element otherwise; 4 elements of one document's
//      head or kept tail are ONE 16-byte load of ids (and one of labels), 4-byte aligned.  Every element of every selected
//      output is written exactly once, pads included; an unselected output is not touched.
//   7. tk_rowfit_cu_kernel: one item per document, per row and one terminal.  The rank of a document's start in cu_seqlens is
//      (non-empty documents before it) + (pad runs of the rows before its row); of a row's pad run (non-empty documents up to
//      the row's end) + (pad runs before).  max_seqlen: a wave maximum and one atomicMax a wave.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tk_kernels.h"
#include "tk_layout.h"

#define TKR_UNMARKED 0xFFFFFFFFu

__global__ __launch_bounds__(TKY_BLOCK) void tk_rowfit_len_kernel(TkRowfitArgs a) {
    const uint64_t D = a.n_docs;
    const uint64_t n_iter = (D + (uint64_t)gridDim.x * TKY_BLOCK - 1u) / ((uint64_t)gridDim.x * TKY_BLOCK);
    uint32_t cut = 0;
    for (uint64_t it = 0; it < n_iter; ++it) {          // (every lane stays to the wave sum below)
        const uint64_t d = (it * gridDim.x + blockIdx.x) * TKY_BLOCK + threadIdx.x;
        if (d >= D) continue;
        const uint64_t n = a.id_offs[d + 1] - a.id_offs[d];
        a.e[d] = n < a.row_len ? (uint32_t)n : a.row_len;
        a.nz[d] = n != 0;
        cut += n > a.row_len;
    }
    tky_wave_add(a.stat, cut);
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_rowfit_nxt_kernel(TkRowfitArgs a) {
    const uint64_t D = a.n_docs;
    for (uint64_t v = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; v <= D; v += (uint64_t)gridDim.x * TKY_BLOCK) {
        a.row[v] = v ? TKR_UNMARKED : 0u;
        if (v == D) { a.jump_a[v] = D; continue; }      // (the sentinel: to itself, in 0 steps)
        const uint64_t key = a.E[v] + a.row_len;
        uint64_t lo = v + 1u, w = 1;                    // E[lo] <= key: a document takes at most L
        while (lo + w <= D && a.E[lo + w] <= key) { lo += w; w <<= 1; }
        const uint64_t hi = lo + w <= D ? lo + w : D + 1u;   // E[hi] > key, or hi is behind the array
        const uint64_t nxt = lo + tky_count_le(a.E + lo, hi - lo, key) - 1u;
        a.jump_a[v] = nxt | 1ull << 32;
    }
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_rowfit_round_kernel(TkRowfitArgs a, int flip) {
    const uint64_t* jin = flip ? a.jump_b : a.jump_a;
    uint64_t* jout = flip ? a.jump_a : a.jump_b;
    for (uint64_t v = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; v <= a.n_docs; v += (uint64_t)gridDim.x * TKY_BLOCK) {
        const uint64_t j = jin[v];
        const uint32_t t = (uint32_t)j, steps = (uint32_t)(j >> 32);
        const uint32_t r = a.row[v];
        if (r != TKR_UNMARKED && steps) a.row[t] = r + steps;
        const uint64_t j2 = jin[t];
        jout[v] = (j2 & 0xFFFFFFFFull) | (uint64_t)(steps + (uint32_t)(j2 >> 32)) << 32;
    }
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_rowfit_open_kernel(TkRowfitArgs a) {
    for (uint64_t v = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; v <= a.n_docs; v += (uint64_t)gridDim.x * TKY_BLOCK) {
        const uint32_t r = a.row[v];
        if (r != TKR_UNMARKED) a.open[r] = v;           // (r <= n_docs: the chain has at most n_docs links)
        if (v == a.n_docs) {                            // what the host reads to size the tensors, beside stat[0], in one copy
            a.stat[3] = r;
            a.stat[4] = a.E[v];
            a.stat[5] = a.id_offs[v];
        }
    }
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_rowfit_place_kernel(TkRowfitArgs a) {
    const uint64_t D = a.n_docs, L = a.row_len;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_iter = (D + 1u + (uint64_t)gridDim.x * TKY_BLOCK - 1u) / ((uint64_t)gridDim.x * TKY_BLOCK);
    for (uint64_t it = 0; it < n_iter; ++it) {
        const uint64_t base = (it * gridDim.x + blockIdx.x) * TKY_BLOCK + (threadIdx.x & ~63u);   // the wave's first document
        if (base > D) continue;                         // (wave-uniform: every lane of a wave that stays reaches the scan and the search)
        const uint64_t d = base + lane;
        const uint32_t r = d < D ? a.row[d] : TKR_UNMARKED;
        const uint32_t pm = tkd_scan_max(r != TKR_UNMARKED ? lane + 1u : 0u);
        // the lanes in front of the wave's first mark: the last document at or before base - 1 that opens a row (open[0] = 0)
        const uint64_t c = tky_wave_count_le(a.open, a.n_rows, base);
        if (d > D) continue;
        if (d == D) { a.dstart[D] = a.n_rows * L; continue; }
        const uint64_t v = pm ? base + pm - 1u : a.open[c - 1u];
        const uint64_t rv = pm ? a.row[v] : c - 1u;
        a.dstart[d] = rv * L + (a.E[d] - a.E[v]);
        a.segno[d] = (uint32_t)(a.nzp[d] - a.nzp[v]) + 1u;
        if (r != TKR_UNMARKED) a.padf[r] = a.E[a.open[r + 1u]] - a.E[d] < L;   // (d opens row r)
    }
}

// what a unit needs of the document that holds a position: where its ids lie and its number inside its row
struct TkrDoc { uint64_t o0, o1; uint32_t sg; };

template <int I64, int VEC>
__global__ __launch_bounds__(TKY_BLOCK) void tk_rowfit_kernel(TkRowfitArgs a) {
    constexpr uint32_t W = VEC ? 4u : 1u;
    __shared__ uint64_t s_oo[TKY_CAP + 2];              // id_offs of the tile's documents: [0] is the one that holds g0
    __shared__ uint32_t s_sg[TKY_CAP + 1];
    const uint32_t L = a.row_len, head = L - a.keep_tail, ign = (uint32_t)a.ignore;
    const uint64_t D = a.n_docs, total = a.n_rows * L;
    const uint64_t n_tiles = (total + TKY_TILE - 1) / TKY_TILE;
    const bool side = a.out_seg != nullptr;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t g0 = t * TKY_TILE;
        const uint64_t g1 = total - g0 < TKY_TILE ? total : g0 + TKY_TILE;
        TkyTile<2> tile(a.dstart, g0);
        tile.search(D, g0, g1 - 1u);                    // starts at or before the tile's first | last position
        const uint64_t n_lo = tile.found(0);            // (block-uniform, as everything up to the unit loop; >= 1: doc_start[0] == 0)
        if (n_lo == 0 || tile.found(1) < n_lo) continue;
        tile.open(n_lo, tile.found(1) - n_lo);          // starts in (g0, g1): documents n_lo .. n_lo + count - 1, empty ones included
        tile.stage([&](uint32_t j, uint64_t d) {
            s_oo[j] = a.id_offs[d];
            if (j == tile.count) s_oo[j + 1u] = a.id_offs[d + 1u];
            if (side) s_sg[j] = a.segno[d];
        });
        auto doc = [&](uint32_t k) -> TkrDoc {          // the tile's document k: n_lo - 1 + k
            if (tile.lds) return TkrDoc{s_oo[k], s_oo[k + 1u], side ? s_sg[k] : 0u};
            const uint64_t d = n_lo - 1u + k;
            return TkrDoc{a.id_offs[d], a.id_offs[d + 1u], side ? a.segno[d] : 0u};
        };
        const uint32_t units = (uint32_t)(g1 - g0) / W; // (VEC: total and g0 are multiples of 4)
        for (uint32_t u = threadIdx.x; u < units; u += TKY_BLOCK) {
            const uint32_t l = u * W;
            const uint64_t g = g0 + l;
            uint32_t k = tile.count_le(l);
            TkrDoc m = doc(k);
            int64_t start = tile.start_of(k);
            uint64_t n = m.o1 - m.o0;
            uint32_t e = n < L ? (uint32_t)n : L;
            uint32_t v[4] = {a.pad_id, a.pad_id, a.pad_id, a.pad_id}, lb[4] = {ign, ign, ign, ign};
            uint32_t p[4] = {0u, 0u, 0u, 0u}, sg[4] = {0u, 0u, 0u, 0u};
            const uint64_t k0 = (uint64_t)((int64_t)l - start);
            // the common unit: 4 elements of one document's head, or of its kept tail -- one load of 16 bytes, 4-byte aligned
            if (VEC && (k == tile.count || tile.rel(k) >= l + 4u) && k0 + 4u <= e && (n <= L || k0 + 4u <= head || k0 >= head)) {
                const uint64_t src = n > L && k0 >= head ? m.o1 - (L - k0) : m.o0 + k0;
                tky_gather4(a.ids + src, v);
                if (a.out_lab) tky_gather4(reinterpret_cast<const uint32_t*>(a.lab + src), lb);
#pragma unroll
                for (uint32_t q = 0; q < 4u; ++q) { p[q] = (uint32_t)k0 + q; sg[q] = m.sg; }
            } else {
#pragma unroll
                for (uint32_t q = 0; q < W; ++q) {
                    const uint32_t lq = l + q;
                    if (k < tile.count && tile.rel(k) <= lq) {   // another document (over ties too: the LAST that starts at or before the position)
                        do ++k; while (k < tile.count && tile.rel(k) <= lq);
                        m = doc(k);
                        start = (int64_t)tile.rel(k - 1u);
                        n = m.o1 - m.o0;
                        e = n < L ? (uint32_t)n : L;
                    }
                    const uint64_t kk = (uint64_t)((int64_t)lq - start);
                    if (kk >= e) continue;              // a pad
                    const uint64_t src = n > L && kk >= head ? m.o1 - (L - kk) : m.o0 + kk;
                    v[q] = a.ids[src];
                    if (a.out_lab) lb[q] = (uint32_t)a.lab[src];
                    p[q] = (uint32_t)kk;
                    sg[q] = m.sg;
                }
            }
            tky_store<I64, VEC>(a.out_ids, g, v);
            if (a.out_lab) tky_store<0, VEC>(a.out_lab, g, lb);
            if (a.out_pos) tky_store<I64, VEC>(a.out_pos, g, p);
            if (a.out_seg) tky_store<I64, VEC>(a.out_seg, g, sg);
        }
    }
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_rowfit_cu_kernel(TkRowfitArgs a) {
    const uint64_t D = a.n_docs, R = a.n_rows, L = a.row_len;
    const uint64_t n_items = D + R + 1u;                // documents | rows | the terminal
    const uint64_t n_iter = (n_items + (uint64_t)gridDim.x * TKY_BLOCK - 1u) / ((uint64_t)gridDim.x * TKY_BLOCK);
    uint32_t longest = 0;
    for (uint64_t it = 0; it < n_iter; ++it) {          // (every lane stays to the wave maximum below)
        const uint64_t t = (it * gridDim.x + blockIdx.x) * TKY_BLOCK + threadIdx.x;
        if (t < D) {
            const uint32_t e = a.e[t];
            if (e == 0) continue;
            const uint64_t s = a.dstart[t];
            longest = max(longest, e);
            if (a.cu) a.cu[a.nzp[t] + a.padp[s / L]] = (int32_t)s;
        } else if (t < D + R) {
            const uint64_t r = t - D, v2 = a.open[r + 1u];
            const uint64_t fill = a.E[v2] - a.E[a.open[r]];
            if (fill >= L) continue;
            longest = max(longest, (uint32_t)(L - fill));
            if (a.cu) a.cu[a.nzp[v2] + a.padp[r]] = (int32_t)(r * L + fill);
        } else if (t == D + R) {
            const uint64_t n_seg = a.nzp[D] + a.padp[R];
            if (a.cu) a.cu[n_seg] = (int32_t)(R * L);
            a.stat[1] = n_seg;
        }
    }
    tky_wave_max(a.stat + 2, longest);
}

hipError_t tk_launch_rowfit_len(const TkRowfitArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(tk_rowfit_len_kernel, dim3(tky_blocks(a.n_docs, 2048u)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_rowfit_chain(const TkRowfitArgs& a, uint32_t rounds, hipStream_t s) {
    const dim3 grid(tky_blocks(a.n_docs + 1u, 1u << 16));
    hipLaunchKernelGGL(tk_rowfit_nxt_kernel, grid, dim3(TKY_BLOCK), 0, s, a);
    return tk_launch_chain_rounds(a, rounds, s);
}

hipError_t tk_launch_chain_rounds(const TkRowfitArgs& a, uint32_t rounds, hipStream_t s) {
    const dim3 grid(tky_blocks(a.n_docs + 1u, 1u << 16));
    for (uint32_t k = 0; k < rounds; ++k) hipLaunchKernelGGL(tk_rowfit_round_kernel, grid, dim3(TKY_BLOCK), 0, s, a, (int)(k & 1u));
    hipLaunchKernelGGL(tk_rowfit_open_kernel, grid, dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_rowfit_place(const TkRowfitArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(tk_rowfit_place_kernel, dim3(tky_blocks(a.n_docs + 1u, 2048u)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_rowfit(const TkRowfitArgs& a, int i64, hipStream_t s) {
    if (a.n_rows == 0) return hipSuccess;
    const dim3 grid(tky_blocks(a.n_rows * a.row_len, 1u << 20, TKY_TILE));
    TKY_LAUNCH_I64_VEC(tk_rowfit_kernel, i64, a.row_len % 4u == 0u, grid, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_rowfit_cu(const TkRowfitArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(tk_rowfit_cu_kernel, dim3(tky_blocks(a.n_docs + a.n_rows + 1u, 2048u)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}
