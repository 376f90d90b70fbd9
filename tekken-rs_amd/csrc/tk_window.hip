// tk_window.hip -- gfx950 kernels of the overlapping windows for long documents (include/tekken_hip.h
// tk_window_from_ids_device).
//
// No reference equivalent: the reference has pad_id() (src/tekkenizer.rs:304) and nothing that uses it.  Ragged ids + offsets in;
// every document longer than max_length T split into windows that share `stride` body ids and repeat the document's head and
// tail, input_ids[W, L] (+ mask, spans[W, L, 2], lengths, window_doc, window_start, doc_windows) out.  Pure data movement plus
// "which document holds window row r": the bar is HBM.
//
// Window k of document d (n ids, head h, tail t, c = T - h - t, step = c - stride):
//   n <= T: the one window is R_d; it reads as h = t = 0, a body of n ids.
//   n >  T: b = n - h - t, the body run is B[k * step : min(k * step + c, b)], and element j of the window reads
//           ids[oo[d] + j]                        j < h                (head)
//           ids[oo[d] + h + k * step + (j - h)]   j < h + blen         (body)
//           ids[oo[d] + n - t + (j - h - blen)]   j < h + blen + t     (tail)
// The source index grows with j, so four consecutive elements lie at four consecutive ids exactly where the last one's index is
// the first one's + 3 (a run boundary without a gap -- head and body of window 0 -- included): then ONE unaligned 16-byte load
// fetches them (two for their spans), else element loads.
//
// Two steps on the caller's stream, one read by the host in between (W sizes the tensor):
//   1. tk_window_counts_kernel: w_d per document, the longest document (a wave maximum, one atomic a wave) and the number of
//      split documents (tky_wave_add); tk_launch_scan over w_d gives doc_windows.
//   2. tk_window_kernel, the launch shape of tk_dense_kernel over W rows: the unit is 4 consecutive elements of one row where
//      L % 4 == 0 (one 16-byte store for int32, two for int64, one dword of mask, two 16-byte stores of spans), one element
//      otherwise; a block takes `rb` consecutive rows (rb * G units <= TKW_TILE, G units a row; a longer row is one block row
//      split over blockIdx.y), the row of a unit comes from a per-launch reciprocal.  Two waves of the block find, one 64-ary
//      search over doc_windows each, the documents of its first and last row; the window starts of the documents in between go to
//      LDS relative to the block's first row (TkyTile), and beside them oo[d] and n_d; a unit finds its document there with a
//      binary search over at most rb entries.  More than TKY_CAP documents in the run (rows of 4 elements over one-window
//      documents): the same values come from global memory, decided per block.  Every element of every selected output is written
//      exactly once, pads included.  The lane with a row's first unit writes lengths, window_doc and window_start.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tk_kernels.h"
#include "tk_layout.h"

#define TKW_TILE 2048u     /* units of a block's row group (8 a thread); the reciprocal is exact for indices below it */

__global__ __launch_bounds__(TKY_BLOCK) void tk_window_counts_kernel(TkWindowArgs a) {
    const uint32_t T = a.max_len;
    uint32_t longest = 0, n_split = 0;
    for (uint64_t d = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; d < a.n_docs; d += (uint64_t)gridDim.x * TKY_BLOCK) {
        const uint64_t n = a.id_offs[d + 1] - a.id_offs[d];
        const uint32_t n32 = n < 0xFFFFFFFFull ? (uint32_t)n : 0xFFFFFFFFu;
        longest = longest > n32 ? longest : n32;
        uint32_t w = 1;
        if (n32 > T) {                                  // (a clamped n32 is refused by the host before w is used)
            w = 1u + (uint32_t)(((uint64_t)(n32 - T) + a.step - 1u) / a.step);   // b - c = n - T > 0
            ++n_split;
        }
        a.counts[d] = w;
    }
    tky_wave_max(a.stat, longest);
    tky_wave_add(a.stat + 1, n_split);
}

// row of unit li inside the block's row group (li < TKW_TILE when rb > 1)
__device__ __forceinline__ uint32_t tkw_row_of(const TkWindowArgs& a, uint32_t li) {
    if (a.rb == 1u) return 0u;
    return a.units == 1u ? li : __umulhi(li, a.magic);
}

template <int I64, int MASK, int VEC>
__global__ __launch_bounds__(TKY_BLOCK) void tk_window_kernel(TkWindowArgs a) {
    constexpr uint32_t W = VEC ? 4u : 1u;
    __shared__ uint64_t s_oo[TKY_CAP + 1u];             // oo[d] of the block's documents, [0]: the one that holds its first row
    __shared__ uint32_t s_n[TKY_CAP + 1u];              // n_d of the same
    const uint32_t G = a.units, L = a.row_len, T = a.max_len, h = a.keep_head, t = a.keep_tail;
    const uint32_t cap = T - h - t;
    const uint64_t n_rb = (a.n_rows + a.rb - 1) / a.rb;
    for (uint64_t b = blockIdx.x; b < n_rb; b += gridDim.x) {
        const uint64_t row0 = b * a.rb;
        const uint32_t nrows = a.n_rows - row0 < a.rb ? (uint32_t)(a.n_rows - row0) : a.rb;
        const uint32_t total = nrows * G;               // rb > 1: <= TKW_TILE; rb == 1: G < 2^31
        TkyTile<2> tile(a.doc_windows, row0);
        tile.search(a.n_docs, row0, row0 + nrows - 1u); // documents that start at or before: the first row (>= 1) | the last row
        const uint64_t n_lo = tile.found(0);
        tile.open(n_lo, (uint32_t)(tile.found(1) - n_lo));   // documents that start in (row0, row0 + nrows): < nrows
        tile.stage([&](uint32_t j, uint64_t e) {
            const uint64_t o = a.id_offs[e];
            s_oo[j] = o;
            s_n[j] = (uint32_t)(a.id_offs[e + 1u] - o);
        });
        for (uint32_t li = blockIdx.y * TKY_BLOCK + threadIdx.x; li < total; li += TKY_BLOCK * gridDim.y) {
            const uint32_t r = tkw_row_of(a, li), cg = li - r * G;
            const uint32_t kd = tile.count_le(r);       // the block's document that holds row r
            const uint64_t d = n_lo - 1u + kd;
            const uint32_t kw = (uint32_t)((int64_t)r - tile.start_of(kd));   // the window's number inside its document
            uint64_t o0;
            uint32_t n;
            if (tile.lds) {
                o0 = s_oo[kd]; n = s_n[kd];
            } else {
                o0 = a.id_offs[d]; n = (uint32_t)(a.id_offs[d + 1u] - o0);
            }
            // the three source runs of the window: [0, hh) head | [hh, hb) body, from body index bs | [hb, len) tail
            uint32_t hh = 0, tt = 0, bs = 0, blen = n;
            if (n > T) {
                const uint32_t body = n - h - t;
                hh = h; tt = t;
                bs = kw * a.step;                       // < body
                blen = body - bs < cap ? body - bs : cap;
            }
            const uint32_t hb = hh + blen, len = hb + tt;
            const uint64_t row = row0 + r;
            if (cg == 0u) {
                const uint64_t ws = (uint64_t)h + (uint64_t)kw * a.step;
                a.lengths[row] = len;
                a.window_doc[row] = (uint32_t)d;
                a.window_start[row] = ws < n ? (uint32_t)ws : n;
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
                const tky_u32x4 x = *reinterpret_cast<const tky_u32x4_a4*>(a.ids + s0);
                v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
                mbits = 0x01010101u;
                if (a.out_spans) {
                    const tky_u32x4 p0 = *reinterpret_cast<const tky_u32x4_a4*>(a.in_spans + 2u * s0);
                    const tky_u32x4 p1 = *reinterpret_cast<const tky_u32x4_a4*>(a.in_spans + 2u * s0 + 4u);
                    sp[0] = p0.x; sp[1] = p0.y; sp[2] = p0.z; sp[3] = p0.w;
                    sp[4] = p1.x; sp[5] = p1.y; sp[6] = p1.z; sp[7] = p1.w;
                }
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
            if (MASK) {
                if (VEC) *reinterpret_cast<uint32_t*>(a.mask + at) = mbits;
                else a.mask[at] = (uint8_t)mbits;
            }
            if (a.out_spans) {
                tky_store<0, VEC>(a.out_spans, 2u * at, sp);
                if (VEC) tky_store<0, 1>(a.out_spans, 2u * at + 4u, sp + 4);
                else a.out_spans[2u * at + 1u] = sp[1];
            }
        }
    }
}

hipError_t tk_launch_window_counts(const TkWindowArgs& a, hipStream_t s) {
    if (a.n_docs == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_window_counts_kernel, dim3(tky_blocks(a.n_docs, 2048u)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

template <int I64, int MASK>
static void tkw_launch2(const TkWindowArgs& a, bool vec, dim3 grid, hipStream_t s) {
    if (vec) hipLaunchKernelGGL((tk_window_kernel<I64, MASK, 1>), grid, dim3(TKY_BLOCK), 0, s, a);
    else hipLaunchKernelGGL((tk_window_kernel<I64, MASK, 0>), grid, dim3(TKY_BLOCK), 0, s, a);
}

hipError_t tk_launch_window(const TkWindowArgs& args, int i64, hipStream_t s) {
    if (args.n_rows == 0) return hipSuccess;
    TkWindowArgs a = args;
    const bool vec = a.row_len != 0u && a.row_len % 4u == 0u;
    a.units = vec ? a.row_len / 4u : a.row_len ? a.row_len : 1u;   // (L == 0: one unit a row, which writes the per-row outputs)
    a.rb = a.units <= TKW_TILE ? TKW_TILE / a.units : 1u;
    a.magic = a.units > 1u ? (uint32_t)((1ull << 32) / a.units) + 1u : 0u;
    uint32_t gy = 1;
    if (a.rb == 1u) {
        gy = (a.units + TKW_TILE - 1) / TKW_TILE;
        if (gy > 64u) gy = 64u;
    }
    const dim3 grid(tky_blocks(a.n_rows, 1u << 20, a.rb), gy);
    if (i64 && a.mask) tkw_launch2<1, 1>(a, vec, grid, s);
    else if (i64) tkw_launch2<1, 0>(a, vec, grid, s);
    else if (a.mask) tkw_launch2<0, 1>(a, vec, grid, s);
    else tkw_launch2<0, 0>(a, vec, grid, s);
    return hipGetLastError();
}
