// tk_pair.hip -- gfx950 kernels of the sentence-pair rows (include/tekken_hip.h tk_pair_from_ids_device).
//
// No reference equivalent: the reference encodes one text (src/tekkenizer.rs:378).  The ragged ids of 2P parts + offsets in (part
// 2p: the first text A, part 2p + 1: the second text B); rows head + A-part + sep + B-part + tail out, cut by one of three
// strategies, the windowed side of a pair that does not fit split into overlapping windows that repeat the fixed ids and the other
// side: input_ids[W, L] (+ mask, type_ids, sequence_ids, spans[W, L, 2], lengths, window_pair, window_start, second_start,
// pair_windows).  Pure data movement plus "which pair holds row r": the bar is HBM.
//
// Row k of pair p (a = |A|, b = |B|, c = T - n_head - n_sep - n_tail) keeps A[as : as + alen] and B[bs : bs + blen] (tkp_kept: the
// three strategies of the definition, from a, b and k alone, no division), and element j of it reads
//   head[j]                                      j < e0 = n_head
//   ids[oo[2p] + as + (j - e0)]                  j < e1 = e0 + alen        (A)
//   sep[j - e1]                                  j < e2 = e1 + n_sep
//   ids[oo[2p] + a + bs + (j - e2)]              j < e3 = e2 + blen        (B; part 2p + 1 begins a ids behind part 2p)
//   tail[j - e3]                                 j < e4 = e3 + n_tail      (the row's length)
// and pad_id behind.  The fixed ids come from the kernel arguments.  Four consecutive elements that lie in ONE of the two id runs
// take one unaligned 16-byte load (two more for their spans), every other unit loads element by element.
//
// Two steps on the caller's stream, one read by the host in between (W and the longest row size the tensors):
//   1. tk_pair_counts_kernel: w_p per pair, the longest row and the longest part (wave maxima, one atomic a wave) and the three
//      counters (tky_wave_add); tk_launch_scan over w_p gives pair_windows.
//   2. tk_pair_kernel, the row-group launch shape (tk_rows.h) over W rows; a unit of 4 elements stores one dword each of mask /
//      type_ids / sequence_ids and two 16-byte halves of spans.  The pairs of the block's rows come from TkyRowOwners
//      (tk_layout.h) over pair_windows, and beside their starts oo[2p], a and b go to LDS; where nothing is staged the same
//      values come from global memory.  Every element of every selected output is written exactly once, pads included; no
//      atomics.  The lane with a row's first unit writes lengths, window_pair, window_start and second_start.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tk_kernels.h"
#include "tk_layout.h"

struct TkpKept { uint32_t as, alen, bs, blen; };   // a row keeps A[as : as + alen] and B[bs : bs + blen]

__device__ __forceinline__ uint32_t tkp_min(uint32_t x, uint32_t y) { return x < y ? x : y; }

// what row k of a pair with a and b ids keeps (k < w_p; k == 0 is the pair's longest row)
__device__ __forceinline__ TkpKept tkp_kept(const TkPairArgs& p, uint32_t a, uint32_t b, uint32_t k) {
    TkpKept r = {0u, a, 0u, b};
    const uint32_t c = p.cap;
    if (p.strategy == TK_PAIR_LONGEST_FIRST) {
        if ((uint64_t)a + b > c) {
            if (a <= b) { r.alen = tkp_min(a, c / 2u); r.blen = tkp_min(b, c - r.alen); }
            else { r.blen = tkp_min(b, c / 2u); r.alen = tkp_min(a, c - r.blen); }
        }
        return r;
    }
    const bool second = p.strategy == TK_PAIR_ONLY_SECOND;
    const uint32_t v = second ? b : a;
    const uint32_t f = tkp_min(second ? a : b, p.max_fixed), cw = c - f;   // F <= c - 1: cw >= 1
    uint32_t vs = 0, vlen = v;
    if (v > cw) {
        if (p.overflow) {
            vs = k * (cw - p.stride);                   // < v for every window of the pair
            vlen = tkp_min(v - vs, cw);
        } else {
            vlen = cw;
        }
    }
    if (second) { r.alen = f; r.bs = vs; r.blen = vlen; }
    else { r.as = vs; r.alen = vlen; r.blen = f; }
    return r;
}

// entry q < 4 of a fixed id list of the kernel arguments (selects: no indexed access to the argument block)
__device__ __forceinline__ uint32_t tkp_pick(const uint32_t (&v)[4], uint32_t q) {
    return q == 0u ? v[0] : q == 1u ? v[1] : q == 2u ? v[2] : v[3];
}

__global__ __launch_bounds__(TKY_BLOCK) void tk_pair_counts_kernel(TkPairArgs p) {
    const uint32_t x = p.n_head + p.n_sep + p.n_tail;
    uint32_t longest = 0, part = 0, n_trunc = 0, n_split = 0, n_cut = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; i < p.n_pairs; i += (uint64_t)gridDim.x * TKY_BLOCK) {
        const uint64_t o0 = p.id_offs[2u * i], o1 = p.id_offs[2u * i + 1u], o2 = p.id_offs[2u * i + 2u];
        const uint32_t a = tky_len32(o1 - o0), b = tky_len32(o2 - o1);
        part = part > a ? part : a;
        part = part > b ? part : b;
        const TkpKept r = tkp_kept(p, a, b, 0u);
        const uint32_t len = x + r.alen + r.blen;       // <= T
        longest = longest > len ? longest : len;
        n_trunc += (r.alen < a || r.blen < b) ? 1u : 0u;
        uint32_t w = 1;
        if (p.strategy != TK_PAIR_LONGEST_FIRST) {
            const bool second = p.strategy == TK_PAIR_ONLY_SECOND;
            const uint32_t xl = second ? a : b, v = second ? b : a;
            const uint32_t cw = p.cap - tkp_min(xl, p.max_fixed);
            n_cut += xl > p.max_fixed ? 1u : 0u;
            if (p.overflow && v > cw) {
                const uint32_t step = cw - p.stride;    // >= 1
                w = (uint32_t)(1u + ((uint64_t)(v - cw) + step - 1u) / step);
                ++n_split;
            }
        }
        p.counts[i] = w;
    }
    tky_wave_max(p.stat, longest);
    tky_wave_add(p.stat + 1, n_trunc);
    tky_wave_add(p.stat + 2, n_split);
    tky_wave_add(p.stat + 3, n_cut);
    tky_wave_max(p.stat + 4, part);
}

template <int I64, int VEC>
__global__ __launch_bounds__(TKY_BLOCK) void tk_pair_kernel(TkPairArgs p) {
    constexpr uint32_t W = VEC ? 4u : 1u;
    __shared__ uint64_t s_oo[TKY_CAP + 1u];             // oo[2p] of the block's pairs, [0]: the one that holds its first row
    __shared__ uint32_t s_a[TKY_CAP + 1u];              // a and b of the same
    __shared__ uint32_t s_b[TKY_CAP + 1u];
    const uint32_t G = p.rows.units, L = p.row_len;
    const uint64_t n_rb = tky_row_groups(p.rows, p.n_rows);
    for (uint64_t blk = blockIdx.x; blk < n_rb; blk += gridDim.x) {
        const TkyRowGroup g(p.rows, p.n_rows, blk);
        const TkyRowOwners pairs(p.pair_windows, p.n_pairs, g, [&](uint32_t j, uint64_t e) {
            const uint64_t o = p.id_offs[2u * e], o1 = p.id_offs[2u * e + 1u];
            s_oo[j] = o;
            s_a[j] = (uint32_t)(o1 - o);
            s_b[j] = (uint32_t)(p.id_offs[2u * e + 2u] - o1);
        });
        for (uint32_t li = g.first(); li < g.total; li += g.step()) {
            const uint32_t r = tky_row_of(p.rows, li), cg = li - r * G;
            const uint32_t kd = pairs.count_le(r);      // the block's pair that holds row r
            const uint64_t pr = pairs.n_lo - 1u + kd;
            const uint32_t kw = (uint32_t)((int64_t)r - pairs.start_of(kd));  // the row's number inside its pair
            uint64_t o0;
            uint32_t a, b;
            if (pairs.lds) {
                o0 = s_oo[kd]; a = s_a[kd]; b = s_b[kd];
            } else {
                o0 = p.id_offs[2u * pr];
                const uint64_t o1 = p.id_offs[2u * pr + 1u];
                a = (uint32_t)(o1 - o0); b = (uint32_t)(p.id_offs[2u * pr + 2u] - o1);
            }
            // once a unit: what the row keeps, and the ends of its five source runs
            const TkpKept k = tkp_kept(p, a, b, kw);
            const uint32_t e0 = p.n_head, e1 = e0 + k.alen, e2 = e1 + p.n_sep, e3 = e2 + k.blen, e4 = e3 + p.n_tail;
            const uint64_t oa = o0 + k.as - e0;         // ids[oa + j]: element j of the A run (wraps where as < e0: only sums are used)
            const uint64_t ob = o0 + a + k.bs - e2;     // ids[ob + j]: element j of the B run
            const uint64_t row = g.row0 + r;
            if (cg == 0u) {
                p.lengths[row] = e4;
                p.window_pair[row] = (uint32_t)pr;
                p.window_start[row] = p.strategy == TK_PAIR_ONLY_SECOND ? k.bs : k.as;   // (LONGEST_FIRST: both are 0)
                p.second_start[row] = e2;
            }
            if (L == 0u) continue;                      // (no fixed id and every pair empty: only the per-row outputs)
            const uint32_t j0 = cg * W;
            uint32_t v[4], sp[8];
            uint32_t mbits = 0, tbits = 0, sbits = 0;
            // four elements inside one id run: j0 >= e0 && j0 + 4 <= e1 (A) or j0 >= e2 && j0 + 4 <= e3 (B)
            const bool in_a = VEC && j0 >= e0 && j0 + 4u <= e1, in_b = VEC && j0 >= e2 && j0 + 4u <= e3;
            if (VEC && (in_a || in_b)) {
                const uint64_t s0 = (in_a ? oa : ob) + j0;
                tky_gather4(p.ids + s0, v);
                mbits = 0x01010101u;
                tbits = in_b ? 0x01010101u : 0u;
                sbits = in_b ? 0x01010101u : 0u;
                if (p.out_spans) tky_gather4_spans(p.in_spans, s0, sp);
            } else {
#pragma unroll
                for (uint32_t q = 0; q < W; ++q) {
                    const uint32_t j = j0 + q;
                    const bool is_a = j >= e0 && j < e1, is_b = j >= e2 && j < e3, id = is_a || is_b;
                    const uint64_t sq = id ? (is_a ? oa : ob) + j : 0u;
                    const uint32_t fixed = j < e0 ? tkp_pick(p.head, j) : j < e2 ? tkp_pick(p.sep, j - e1)
                                           : j < e4 ? tkp_pick(p.tail, j - e3) : p.pad_id;
                    v[q] = id ? p.ids[sq] : fixed;
                    mbits |= (uint32_t)(j < e4) << (8u * q);
                    tbits |= (uint32_t)(j >= e2 && j < e4) << (8u * q);
                    sbits |= (is_a ? 0u : is_b ? 1u : (uint32_t)TK_PAIR_SEQ_NONE) << (8u * q);
                    if (p.out_spans) {
                        sp[2u * q] = id ? p.in_spans[2u * sq] : 0u;
                        sp[2u * q + 1u] = id ? p.in_spans[2u * sq + 1u] : 0u;
                    }
                }
            }
            const uint64_t at = row * L + j0;
            tky_store<I64, VEC>(p.out, at, v);
            if (p.mask) tky_store_plane<VEC>(p.mask, at, mbits);
            if (p.type_ids) tky_store_plane<VEC>(p.type_ids, at, tbits);
            if (p.seq_ids) tky_store_plane<VEC>(p.seq_ids, at, sbits);
            if (p.out_spans) tky_store_spans<VEC>(p.out_spans, at, sp);
        }
    }
}

hipError_t tk_launch_pair_counts(const TkPairArgs& a, hipStream_t s) {
    if (a.n_pairs == 0) return hipSuccess;
    // 8 pairs a thread: the kernel's time is its atomics on the five statistics words (measured: about 10 ns each, one after the
    // other), so fewer, longer waves
    hipLaunchKernelGGL(tk_pair_counts_kernel, dim3(tky_blocks(a.n_pairs, 2048u, TKY_BLOCK * 8u)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_pair(const TkPairArgs& args, int i64, hipStream_t s) {
    TkPairArgs a = args;
    const TkyRowsGrid rg = tky_rows_shape(a.n_rows, a.row_len, true, a.rows);   // (L == 0: one unit a row, which writes the per-row outputs)
    if (rg.x == 0u) return hipSuccess;
    TKY_LAUNCH_I64_VEC(tk_pair_kernel, i64, a.row_len != 0u && a.row_len % 4u == 0u, dim3(rg.x, rg.y), s, a);
    return hipGetLastError();
}
