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
//   2. tk_window_kernel, the row-group launch shape (tk_rows.h) over W rows; a unit of 4 elements also stores two 16-byte
//      halves of spans.  The documents of the block's rows come from TkyRowOwners (tk_layout.h) over doc_windows, and beside
//      their window starts oo[d] and n_d go to LDS; where nothing is staged the same values come from global memory.  Every
//      element of every selected output is written exactly once, pads included.  The lane with a row's first unit writes
//      lengths, window_doc and window_start.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tk_kernels.h"
#include "tk_layout.h"

__global__ __launch_bounds__(TKY_BLOCK) void tk_window_counts_kernel(TkWindowArgs a) {
    const uint32_t T = a.max_len;
    uint32_t longest = 0, n_split = 0;
    for (uint64_t d = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; d < a.n_docs; d += (uint64_t)gridDim.x * TKY_BLOCK) {
        const uint32_t n32 = tky_len32(a.id_offs[d + 1] - a.id_offs[d]);
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

template <int I64, int MASK, int VEC>
__global__ __launch_bounds__(TKY_BLOCK) void tk_window_kernel(TkWindowArgs a) {
    constexpr uint32_t W = VEC ? 4u : 1u;
    __shared__ uint64_t s_oo[TKY_CAP + 1u];             // oo[d] of the block's documents, [0]: the one that holds its first row
    __shared__ uint32_t s_n[TKY_CAP + 1u];              // n_d of the same
    const uint32_t G = a.rows.units, L = a.row_len, T = a.max_len, h = a.keep_head, t = a.keep_tail;
    const uint32_t cap = T - h - t;
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
            const uint32_t kw = (uint32_t)((int64_t)r - docs.start_of(kd));   // the window's number inside its document
            uint64_t o0;
            uint32_t n;
            if (docs.lds) {
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
            const uint64_t row = g.row0 + r;
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

hipError_t tk_launch_window_counts(const TkWindowArgs& a, hipStream_t s) {
    if (a.n_docs == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_window_counts_kernel, dim3(tky_blocks(a.n_docs, 2048u)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_window(const TkWindowArgs& args, int i64, hipStream_t s) {
    TkWindowArgs a = args;
    const TkyRowsGrid rg = tky_rows_shape(a.n_rows, a.row_len, true, a.rows);   // (L == 0: one unit a row, which writes the per-row outputs)
    if (rg.x == 0u) return hipSuccess;
    TKY_LAUNCH_I64_MASK_VEC(tk_window_kernel, i64, a.mask, a.row_len != 0u && a.row_len % 4u == 0u, dim3(rg.x, rg.y), s, a);
    return hipGetLastError();
}
