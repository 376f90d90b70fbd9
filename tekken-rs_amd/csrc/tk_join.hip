// tk_join.hip -- gfx950 kernels of the chat batches (include/tekken_hip.h tk_join_from_ids_device).
//
// No reference equivalent: the reference never makes a control token out of text, get_control_token (src/tekkenizer.rs:331-341)
// only hands out the id.  Ragged ids of P parts (encoded one by one, without BOS / EOS), a control id or none per part and the
// parts of every conversation in; the stream with every control id in front of its part's ids, its per-conversation offsets,
// labels and the part index of every element out.  Pure data movement plus a search for "which part holds output position g":
// the bar is HBM.
//
// Three steps behind tk_launch_scan, all on the caller's stream, nothing read by the host in between:
//   1. tk_join_has_kernel: per part, "has a control id"; tk_launch_scan over it gives cb[p], the control ids before part p.
//   2. tk_join_parts_kernel: start[p] = id_offs[p] + cb[p], where part p starts in the output (start[P] = N); the part's index
//      inside its conversation (one binary search over conv_offs a part, only when part_index is selected); offsets[c] =
//      start[conv_offs[c]]; n_labelled, summed over the wave, then the block, and added once a block.
//   3. tk_join_kernel: a block takes a tile of TKY_TILE consecutive output positions.  start is non-decreasing, NOT strictly
//      increasing (a part with neither a control id nor text starts where the next one does), and the part that holds g is the
//      LAST one with start <= g: exactly what the 64-ary wave search returns on an array with ties (tk_layout.h has the
//      argument), so nothing is compacted.  Two waves search the tile's first and last position; the starts in between go to LDS
//      relative to the tile, and beside them one record per part of the tile (control id, label bits, local index, the
//      control ids up to it), loaded coalesced once a tile.  A tile with more than TKY_CAP starts (one-element parts, runs of
//      empty ones) reads the same values from global memory: decided per block.  A thread resolves 4 consecutive positions:
//      one binary search, then ONE 16-byte load where the 4 lie in one part's text, or a walk forward that steps over ties as
//      the search does.  One 16-byte store per selected output; the last N % 4
//      elements go out one by one.  A control id sits at its part's start; a text id is read at g - cb[p + 1]: coalesced, 4-byte
//      aligned.  N is known on the device only (the grid is sized for n_ids + P, blocks without a tile leave), and is clamped
//      to what the buffers hold.  Every element is written exactly once; an unselected output is not touched.
//   tk_join_check_kernel (TK_CHECK_PARTS): the first conversation whose offset breaks "starts at 0, non-decreasing, ends at P"
//   and the first part whose control id is neither TK_JOIN_NONE nor special, by atomicMin.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tk_kernels.h"
#include "tk_layout.h"

__global__ __launch_bounds__(TKY_BLOCK) void tk_join_check_kernel(TkJoinArgs a) {
    const uint64_t P = a.n_parts, C = a.n_convs, n = (P > C + 1u ? P : C + 1u);
    for (uint64_t i = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TKY_BLOCK) {
        if (i <= C) {
            const uint64_t o = a.conv_offs[i];
            const bool bad = (i == 0 && o != 0) || (i < C && a.conv_offs[i + 1] < o) || (i == C && o != P);
            if (bad) atomicMin(a.stat + 1, (unsigned long long)i);
        }
        if (i < P) {
            const uint32_t c = a.ctrl[i];
            if (c != TK_JOIN_NONE && c >= a.num_special) atomicMin(a.stat + 2, (unsigned long long)i);
        }
    }
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_join_has_kernel(TkJoinArgs a) {
    for (uint64_t p = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; p < a.n_parts; p += (uint64_t)gridDim.x * TKY_BLOCK)
        a.has[p] = a.ctrl[p] != TK_JOIN_NONE;
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_join_parts_kernel(TkJoinArgs a) {
    const uint64_t P = a.n_parts, C = a.n_convs, n = (P > C ? P : C) + 1u;
    const uint64_t n_iter = (n + (uint64_t)gridDim.x * TKY_BLOCK - 1u) / ((uint64_t)gridDim.x * TKY_BLOCK);
    unsigned long long labelled = 0;
    for (uint64_t it = 0; it < n_iter; ++it) {          // (every lane stays to the wave sum below)
        const uint64_t i = (it * gridDim.x + blockIdx.x) * TKY_BLOCK + threadIdx.x;
        if (i <= P) {
            const uint64_t o = a.id_offs[i];
            a.start[i] = o + a.cb[i];
            if (i < P) {
                const uint32_t fl = a.pflags ? a.pflags[i] : 0u;
                if ((fl & TK_PART_LABEL_CTRL) && a.ctrl[i] != TK_JOIN_NONE) ++labelled;
                if (fl & TK_PART_LABEL_TEXT) labelled += a.id_offs[i + 1] - o;
                if (a.part_index) {                     // conversations that start at or before part i: the last of them holds it
                    const uint64_t lo = tky_count_le(a.conv_offs, C, i);
                    a.plocal[i] = (uint32_t)(lo ? i - a.conv_offs[lo - 1u] : i);
                }
            }
        }
        if (i <= C) {
            uint64_t q = a.conv_offs[i];
            if (q > P) q = P;                           // (malformed offsets: nothing is read beyond the arrays)
            a.out_offs[i] = a.id_offs[q] + a.cb[q];
        }
    }
    __shared__ unsigned long long s_sum[TKY_BLOCK / 64];
    for (int d = 32; d > 0; d >>= 1) labelled += __shfl_down(labelled, d, 64);
    if ((threadIdx.x & 63u) == 0u) s_sum[threadIdx.x >> 6] = labelled;
    __syncthreads();                                    // (same-address atomics serialise: one a block, not one a wave)
    if (threadIdx.x == 0) {
        labelled = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        if (labelled) atomicAdd(a.stat, labelled);
    }
}

// what a unit needs of the part that holds a position: its control id, the control ids up to and including its own (a text id
// of the part at output position g is ids[g - srcoff]), its label bits and its index inside its conversation
struct TkjPart { uint32_t ctrl, fl, pl; uint64_t srcoff; };

__global__ __launch_bounds__(TKY_BLOCK) void tk_join_kernel(TkJoinArgs a) {
    __shared__ uint32_t s_ctrl[TKY_CAP + 1], s_dfl[TKY_CAP + 1], s_pl[TKY_CAP + 1];   // of the tile's parts: [0] is the one that holds g0
    const uint64_t P = a.n_parts;
    uint64_t N = a.start[P];
    if (N > a.cap) N = a.cap;                           // (id_offs[P] > n_ids: the host reports it; nothing is written beyond the buffers)
    const uint64_t n_tiles = (N + TKY_TILE - 1) / TKY_TILE;
    const uint32_t ign = (uint32_t)a.ignore;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t g0 = t * TKY_TILE;
        const uint64_t g1 = N - g0 < TKY_TILE ? N : g0 + TKY_TILE;
        TkyTile<2> tile(a.start, g0);
        tile.search(P, g0, g1 - 1u);                    // starts at or before the tile's first | last position
        const uint64_t n_lo = tile.found(0);            // (block-uniform, as everything up to the unit loop)
        if (n_lo == 0 || tile.found(1) < n_lo) continue;   // (start[0] != 0 or a decreasing start: malformed id_offs, no part to read)
        tile.open(n_lo, tile.found(1) - n_lo);          // starts in (g0, g1): parts n_lo .. n_lo + count - 1, empty ones included (P < 2^32)
        const uint64_t cb_lo = a.cb[n_lo];              // srcoff of the part that holds g0
        tile.stage([&](uint32_t j, uint64_t p) {
            s_ctrl[j] = a.ctrl[p];
            s_dfl[j] = (uint32_t)(a.cb[p + 1u] - cb_lo) << 2 | ((a.pflags ? a.pflags[p] : 0u) & 3u);   // (at most TKY_TILE control ids a tile)
            if (a.part_index) s_pl[j] = a.plocal[p];
        });
        auto part = [&](uint32_t j) -> TkjPart {        // the tile's part j: n_lo - 1 + j
            if (tile.lds) return TkjPart{s_ctrl[j], s_dfl[j] & 3u, a.part_index ? s_pl[j] : 0u, cb_lo + (s_dfl[j] >> 2)};
            const uint64_t p = n_lo - 1u + j;
            return TkjPart{a.ctrl[p], a.pflags ? a.pflags[p] : 0u, a.part_index ? a.plocal[p] : 0u, a.cb[p + 1u]};
        };
        const uint32_t len = (uint32_t)(g1 - g0);
        for (uint32_t l = threadIdx.x * 4u; l < len; l += TKY_BLOCK * 4u) {
            const uint64_t g = g0 + l;
            uint32_t k = tile.count_le(l);
            TkjPart m = part(k);
            int64_t pstart = tile.start_of(k);
            uint32_t v[4] = {0u, 0u, 0u, 0u}, lab[4] = {0u, 0u, 0u, 0u}, pi[4] = {0u, 0u, 0u, 0u};
            // the common unit: 4 positions of one part's text -- one load of 16 bytes, 4-byte aligned
            if (l + 4u <= len && (k == tile.count || tile.rel(k) >= l + 4u) && !(m.ctrl != TK_JOIN_NONE && pstart == (int64_t)l)) {
                tky_gather4(a.ids + (g - m.srcoff), v);
                const bool lt = (m.fl & TK_PART_LABEL_TEXT) != 0u;
#pragma unroll
                for (uint32_t q = 0; q < 4u; ++q) { lab[q] = lt ? v[q] : ign; pi[q] = m.pl; }
            } else {
#pragma unroll
                for (uint32_t q = 0; q < 4u; ++q) {
                    if (l + q >= len) break;
                    if (k < tile.count && tile.rel(k) <= l + q) {   // another part (over ties too: the LAST that starts at or before the position)
                        do ++k; while (k < tile.count && tile.rel(k) <= l + q);
                        m = part(k);
                        pstart = (int64_t)tile.rel(k - 1u);
                    }
                    if (m.ctrl != TK_JOIN_NONE && pstart == (int64_t)(l + q)) {
                        v[q] = m.ctrl;
                        lab[q] = (m.fl & TK_PART_LABEL_CTRL) ? m.ctrl : ign;
                    } else {
                        v[q] = a.ids[g + q - m.srcoff];
                        lab[q] = (m.fl & TK_PART_LABEL_TEXT) ? v[q] : ign;
                    }
                    pi[q] = m.pl;
                }
            }
            if (l + 4u <= len) {
                const tky_u32x4 xv = {v[0], v[1], v[2], v[3]};
                *reinterpret_cast<tky_u32x4*>(a.out_ids + g) = xv;
                if (a.labels) {
                    const tky_u32x4 xl = {lab[0], lab[1], lab[2], lab[3]};
                    *reinterpret_cast<tky_u32x4*>(a.labels + g) = xl;
                }
                if (a.part_index) {
                    const tky_u32x4 xp = {pi[0], pi[1], pi[2], pi[3]};
                    *reinterpret_cast<tky_u32x4*>(a.part_index + g) = xp;
                }
            } else {
#pragma unroll
                for (uint32_t q = 0; q < 3u; ++q) {     // the last N % 4 elements
                    if (l + q >= len) break;
                    a.out_ids[g + q] = v[q];
                    if (a.labels) a.labels[g + q] = (int32_t)lab[q];
                    if (a.part_index) a.part_index[g + q] = pi[q];
                }
            }
        }
    }
}

hipError_t tk_launch_join_check(const TkJoinArgs& a, hipStream_t s) {
    const uint64_t n = a.n_parts > a.n_convs + 1u ? a.n_parts : a.n_convs + 1u;
    hipLaunchKernelGGL(tk_join_check_kernel, dim3(tky_blocks(n, 2048u)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_join_has(const TkJoinArgs& a, hipStream_t s) {
    if (a.n_parts == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_join_has_kernel, dim3(tky_blocks(a.n_parts, 1u << 16)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_join_parts(const TkJoinArgs& a, hipStream_t s) {
    const uint64_t n = (a.n_parts > a.n_convs ? a.n_parts : a.n_convs) + 1u;
    hipLaunchKernelGGL(tk_join_parts_kernel, dim3(tky_blocks(n, 1024u)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_join(const TkJoinArgs& a, hipStream_t s) {
    if (a.n_parts == 0 || a.cap == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_join_kernel, dim3(tky_blocks(a.cap, 1u << 20, TKY_TILE)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}
