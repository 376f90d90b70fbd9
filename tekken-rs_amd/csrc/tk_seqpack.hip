// tk_seqpack.hip -- gfx950 kernels of the packed fixed-length training rows (include/tekken_hip.h tk_seqpack_from_ids_device;
// DESIGN 4.5d).
//
// No reference equivalent: the reference has pad_id() (src/tekkenizer.rs:304) and nothing that uses it.  Ragged ids + offsets
// in; the stream of all ids cut into rows of L (input_ids[n_rows, L]), position_ids that restart at every document and row
// start, segment_ids that number those runs 1, 2, 3, ... within a row, and cu_seqlens / max_seqlen over the flattened tensor
// out.  Pure data movement plus a search for "which document holds stream position g": the bar is HBM.
//
// Four steps, all on the caller's stream, nothing read by the host in between:
//   1. tk_seqpack_flags_kernel: per document, "has ids" and "has ids and starts at a multiple of L" (a document start that is
//      also a row start is ONE segment start); tk_launch_scan over each.
//   2. tk_seqpack_starts_kernel: the starts of the non-empty documents, compacted into a strictly increasing array starts[M]
//      (+ the sentinel starts[M] = N), and beside each the number of aligned starts before it.  Runs of empty documents cost
//      nothing from here on.
//   3. tk_seqpack_kernel: a block takes a tile of TKY_TILE consecutive stream positions.  Three of its waves find, each with
//      one 64-ary search (every lane probes, a ballot narrows the range 64 times a step: 4 dependent loads for a million
//      documents), how many starts lie at or before the tile's first id, its last id and the start of its first row.  The
//      starts inside the tile go to LDS relative to the tile; a unit (4 consecutive elements of one row where L % 4 == 0 --
//      one 16-byte store for each int32 output, two for int64 --, one element otherwise) resolves its document there with a
//      binary search and walks forward over its elements.  A tile with more than TKY_CAP starts (many one-id documents) reads
//      the same values from global memory instead: decided per block.  Every output element is written exactly once, pads
//      included; an unselected output is not touched.
//   4. tk_seqpack_cu_kernel: one item per compacted start, per row and one terminal.  The rank of a segment start in
//      cu_seqlens is (document starts before it) + (row starts before it) - (aligned document starts before it), all known
//      from steps 1-2 and one binary search per ROW; its length is the distance to the next document start, row end or n_used.
//      max_seqlen: a wave maximum and one atomicMax a wave.  The terminal item writes cu_seqlens[n_segments] = n_used and
//      n_segments.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tk_kernels.h"
#include "tk_layout.h"

__global__ __launch_bounds__(TKY_BLOCK) void tk_seqpack_flags_kernel(TkSeqpackArgs a) {
    for (uint64_t d = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; d < a.n_docs; d += (uint64_t)gridDim.x * TKY_BLOCK) {
        const uint64_t o = a.id_offs[d];
        const bool has = a.id_offs[d + 1] > o;
        a.flags[d] = has;
        a.aflags[d] = has && o % a.row_len == 0;
    }
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_seqpack_starts_kernel(TkSeqpackArgs a) {
    for (uint64_t d = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; d <= a.n_docs; d += (uint64_t)gridDim.x * TKY_BLOCK) {
        if (d < a.n_docs && !a.flags[d]) continue;      // (d == n_docs: the sentinel behind the last start)
        const uint64_t i = a.fpos[d];
        a.starts[i] = a.id_offs[d];
        a.n_aligned[i] = a.apos[d];
    }
}

template <int I64, int VEC>
__global__ __launch_bounds__(TKY_BLOCK) void tk_seqpack_kernel(TkSeqpackArgs a) {
    constexpr uint32_t W = VEC ? 4u : 1u;
    const uint32_t L = a.row_len;
    const uint64_t total = a.n_rows * L, n_used = a.n_used;
    const uint64_t n_tiles = (total + TKY_TILE - 1) / TKY_TILE;
    const bool side = a.out_pos || a.out_seg;
    const uint64_t M = side ? a.fpos[a.n_docs] : 0;     // non-empty documents
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t g0 = t * TKY_TILE;
        const uint64_t g1 = total - g0 < TKY_TILE ? total : g0 + TKY_TILE;
        const uint64_t u1 = g1 < n_used ? g1 : n_used;  // behind the tile's last id (the rest is pad)
        const bool search = side && g0 < n_used;        // (block-uniform, as everything up to the unit loop)
        const uint64_t r0 = g0 / L;
        const uint32_t c0 = (uint32_t)(g0 - r0 * L);    // column of the tile's first position
        TkyTile<3> tile(a.starts, g0);
        uint64_t n_row = 0;                             // starts at or before the start of the tile's first row
        if (search) {
            tile.search(M, g0, u1 - 1u, r0 * L);         // starts at or before: the tile's first id (>= 1: starts[0] == 0) | its last id | n_row
            const uint64_t n_lo = tile.found(0);
            n_row = tile.found(2);
            tile.open(n_lo, (uint32_t)(tile.found(1) - n_lo));   // starts in (g0, u1): < TKY_TILE
            tile.stage();
        }
        const uint32_t units = (uint32_t)(g1 - g0) / W; // (VEC: total and g0 are multiples of 4)
        for (uint32_t u = threadIdx.x; u < units; u += TKY_BLOCK) {
            const uint32_t l = u * W;
            const uint64_t g = g0 + l;
            uint32_t v[4], p[4] = {0u, 0u, 0u, 0u}, sg[4] = {0u, 0u, 0u, 0u};
            if (VEC && a.ids_al16 && g + 4u <= n_used) {
                const tky_u32x4 x = *reinterpret_cast<const tky_u32x4*>(a.ids + g);
                v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
            } else {
#pragma unroll
                for (uint32_t q = 0; q < W; ++q) v[q] = g + q < n_used ? a.ids[g + q] : a.pad_id;
            }
            if (search && g < n_used) {
                const uint32_t cabs = c0 + l;           // column counted from the tile's first row (c0 < L < 2^31)
                const uint32_t rr = cabs / L, col = cabs - rr * L;
                const int64_t rowrel = (int64_t)l - (int64_t)col;     // the row's start relative to the tile (rr > 0: inside it)
                const uint64_t n_rowstart = rr == 0u ? n_row : tile.n_lo + tile.count_le((uint32_t)rowrel);
                uint32_t k = tile.count_le(l);
#pragma unroll
                for (uint32_t q = 0; q < W; ++q) {
                    if (g + q >= n_used) break;
                    const uint32_t lq = l + q;
                    while (k < tile.count && tile.rel(k) <= lq) ++k;
                    const int64_t docrel = tile.start_of(k);
                    p[q] = (uint32_t)((int64_t)lq - (docrel > rowrel ? docrel : rowrel));
                    sg[q] = (uint32_t)(tile.n_lo + k - n_rowstart) + 1u;
                }
            }
            tky_store<I64, VEC>(a.out_ids, g, v);
            if (a.out_pos) tky_store<I64, VEC>(a.out_pos, g, p);
            if (a.out_seg) tky_store<I64, VEC>(a.out_seg, g, sg);
        }
    }
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_seqpack_cu_kernel(TkSeqpackArgs a) {
    const uint32_t L = a.row_len;
    const uint64_t D = a.n_docs, n_used = a.n_used, M = a.fpos[D];
    const uint64_t n_items = D + a.n_rows + 1u;         // [0, D): compacted starts (the first M) | rows | the terminal
    const uint64_t n_iter = (n_items + (uint64_t)gridDim.x * TKY_BLOCK - 1u) / ((uint64_t)gridDim.x * TKY_BLOCK);
    uint32_t longest = 0;
    for (uint64_t it = 0; it < n_iter; ++it) {
        const uint64_t t = (it * gridDim.x + blockIdx.x) * TKY_BLOCK + threadIdx.x;
        if (t < D) {
            if (t >= M) continue;
            const uint64_t s = a.starts[t];
            const uint64_t r = s / L;
            if (s >= n_used || s == r * L) continue;    // (an aligned start is its row's item)
            uint64_t end = a.starts[t + 1u];
            if (end > (r + 1u) * L) end = (r + 1u) * L;
            if (end > n_used) end = n_used;
            longest = max(longest, (uint32_t)(end - s));
            if (a.cu) a.cu[t + r + 1u - a.n_aligned[t]] = (int32_t)s;
        } else if (t < D + a.n_rows) {
            const uint64_t r = t - D, s = r * L;
            const uint64_t j = tky_count_lt(a.starts, M, s);
            uint64_t end = a.starts[j] == s ? a.starts[j + 1u] : a.starts[j];   // (starts[M] = N: the sentinel)
            if (end > s + L) end = s + L;
            if (end > n_used) end = n_used;
            longest = max(longest, (uint32_t)(end - s));
            if (a.cu) a.cu[r + j - a.n_aligned[j]] = (int32_t)s;
        } else if (t == D + a.n_rows) {
            const uint64_t j = tky_count_lt(a.starts, M, n_used);
            const uint64_t n_seg = a.n_rows + j - a.n_aligned[j];
            if (a.cu) a.cu[n_seg] = (int32_t)n_used;
            a.stat[0] = n_seg;
        }
    }
    tky_wave_max(a.stat + 1, longest);
}

hipError_t tk_launch_seqpack_flags(const TkSeqpackArgs& a, hipStream_t s) {
    if (a.n_docs == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_seqpack_flags_kernel, dim3(tky_blocks(a.n_docs, 1u << 16)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_seqpack_starts(const TkSeqpackArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(tk_seqpack_starts_kernel, dim3(tky_blocks(a.n_docs + 1u, 1u << 16)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_seqpack(const TkSeqpackArgs& args, int i64, hipStream_t s) {
    if (args.n_rows == 0) return hipSuccess;
    TkSeqpackArgs a = args;
    a.ids_al16 = ((uintptr_t)a.ids & 15u) == 0u;
    const dim3 grid(tky_blocks(a.n_rows * a.row_len, 1u << 20, TKY_TILE));
    TKY_LAUNCH_I64_VEC(tk_seqpack_kernel, i64, a.row_len % 4u == 0u, grid, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_seqpack_cu(const TkSeqpackArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(tk_seqpack_cu_kernel, dim3(tky_blocks(a.n_docs + a.n_rows + 1u, 2048u)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}
