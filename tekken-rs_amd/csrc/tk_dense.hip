// tk_dense.hip -- gfx950 kernels of the model-ready dense layout (include/tekken_hip.h tk_dense_from_ids_device).
//
// No reference equivalent: the reference has pad_id() (src/tekkenizer.rs:304) and nothing that uses it.  Ragged ids + offsets in,
// dense[D, L] (+ mask[D, L], lengths[D], the truncated count) out, and the inverse.  Pure data movement: the bar is HBM.
//
// Kept ids of document d (n ids, limit lim, keep_head h, keep_tail t): k = min(n, lim) of them, and kept position j reads
//   ids[oo[d] + (j < split ? j : j + (n - k))],   split = TRUNC_LEFT ? h : lim - t
// (nothing is truncated: n - k == 0, every j reads itself).  Row d is those k ids and L - k pads, on the side PAD_LEFT says.
//
// Both directions have the row-group launch shape (tk_rows.h; the block's part: tk_layout.h TkyRowGroup).  oo[d], oo[d + 1] and
// the arithmetic above are per unit; the source ids are dword loads (a row's source run starts at an arbitrary id).  Every output
// element is written exactly once, pad included.  The lane that holds a row's first unit writes lengths[d]; the truncated
// documents are counted per lane across the grid stride and added with one atomic per wave (a scan over the wave's lanes).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tk_kernels.h"
#include "tk_layout.h"

template <int I64, int MASK, int VEC>
__global__ __launch_bounds__(TKY_BLOCK) void tk_dense_kernel(TkDenseArgs a) {
    constexpr uint32_t W = VEC ? 4u : 1u;
    const uint32_t G = a.rows.units, L = a.row_len;
    const uint64_t n_rb = tky_row_groups(a.rows, a.n_docs);
    uint32_t n_trunc = 0;
    for (uint64_t b = blockIdx.x; b < n_rb; b += gridDim.x) {
        const TkyRowGroup g(a.rows, a.n_docs, b);
        for (uint32_t li = g.first(); li < g.total; li += g.step()) {
            const uint32_t r = tky_row_of(a.rows, li), cg = li - r * G;
            const uint64_t d = g.row0 + r;
            const uint64_t o0 = a.id_offs[d], n = a.id_offs[d + 1] - o0;
            const uint32_t k = n < (uint64_t)a.lim ? (uint32_t)n : a.lim;
            const uint64_t skip = n - k;                      // ids cut out behind `split`
            const uint32_t split = a.trunc_left ? a.keep_head : a.lim - a.keep_tail;   // (only read when skip != 0: lim is finite then)
            const uint32_t lead = a.pad_left ? L - k : 0u;    // pads in front of the kept ids
            if (cg == 0u) {
                a.lengths[d] = k;
                n_trunc += skip != 0;
            }
            uint32_t v[4];
            uint32_t mbits = 0;
#pragma unroll
            for (uint32_t q = 0; q < W; ++q) {
                const uint32_t j = cg * W + q - lead;         // kept position (wraps above k under the left pads)
                const bool kept = j < k;
                v[q] = kept ? a.ids[o0 + (j < split ? (uint64_t)j : j + skip)] : a.pad_id;
                mbits |= (uint32_t)kept << (8u * q);
            }
            const uint64_t at = d * L + (uint64_t)cg * W;
            tky_store<I64, VEC>(a.out, at, v);
            if (MASK) tky_store_plane<VEC>(a.mask, at, mbits);
        }
    }
    if (blockIdx.y == 0) tky_wave_add(a.stat + 1, n_trunc);   // the truncated documents of this wave's row leaders
}

// stat[0] = max over d of min(n_d, 2^32 - 1) (zeroed by the caller): what the longest-row mode sizes the tensor by
__global__ __launch_bounds__(TKY_BLOCK) void tk_dense_maxlen_kernel(const uint64_t* id_offs, uint64_t n_docs, unsigned long long* stat) {
    uint32_t m = 0;
    for (uint64_t d = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; d < n_docs; d += (uint64_t)gridDim.x * TKY_BLOCK) {
        const uint32_t n32 = tky_len32(id_offs[d + 1] - id_offs[d]);
        m = m > n32 ? m : n32;
    }
    tky_wave_max(stat, m);
}

// ---- dense -> ragged ----

// lens[d]: the given length clamped to the row (one lane a row), or -- given == NULL -- the row without the maximal run of
// pad_id at its padded end (one wave a row, 64 elements a step from that end; the first step usually decides)
template <int I64>
__global__ __launch_bounds__(TKY_BLOCK) void tk_dense_rowlen_kernel(TkRaggedArgs a) {
    const uint32_t L = a.row_len;
    if (a.given) {
        for (uint64_t d = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; d < a.n_docs; d += (uint64_t)gridDim.x * TKY_BLOCK) {
            const uint32_t g = a.given[d];
            a.lens[d] = g < L ? g : L;
        }
        return;
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_waves = (uint64_t)gridDim.x * (TKY_BLOCK / 64);
    for (uint64_t d = (uint64_t)blockIdx.x * (TKY_BLOCK / 64) + (threadIdx.x >> 6); d < a.n_docs; d += n_waves) {
        uint32_t len = 0;
        for (uint32_t c0 = 0; c0 < L; c0 += 64u) {            // c0: elements already seen from the padded end (wave-uniform)
            const uint32_t back = c0 + lane;                  // distance from the padded end
            bool body = false;
            if (back < L) {
                const uint64_t at = d * L + (a.pad_left ? back : L - 1u - back);
                const uint32_t x = I64 ? (uint32_t)reinterpret_cast<const uint64_t*>(a.dense)[at] : reinterpret_cast<const uint32_t*>(a.dense)[at];
                body = x != a.pad_id;
            }
            const uint64_t m = __ballot(body);
            if (m) {
                len = L - (c0 + (uint32_t)__builtin_ctzll(m));
                break;
            }
        }
        if (lane == 0u) a.lens[d] = len;
    }
}

// out_ids[offs[d] + j] = the j-th element of row d's unpadded end, j < lens[d]; the row-group launch shape
template <int I64, int VEC>
__global__ __launch_bounds__(TKY_BLOCK) void tk_ragged_kernel(TkRaggedArgs a, TkyRows shape) {
    constexpr uint32_t W = VEC ? 4u : 1u;
    const uint32_t G = shape.units, L = a.row_len;
    const uint64_t n_rb = tky_row_groups(shape, a.n_docs);
    for (uint64_t b = blockIdx.x; b < n_rb; b += gridDim.x) {
        const TkyRowGroup g(shape, a.n_docs, b);
        for (uint32_t li = g.first(); li < g.total; li += g.step()) {
            const uint32_t r = tky_row_of(shape, li), cg = li - r * G;
            const uint64_t d = g.row0 + r;
            const uint32_t k = a.lens[d];
            const uint32_t lead = a.pad_left ? L - k : 0u;
            const uint32_t j0 = cg * W - lead;                // (wraps under the left pads)
            if (!a.pad_left && cg * W >= k) continue;         // a unit of pads only
            if (a.pad_left && cg * W + W <= lead) continue;
            const uint64_t o0 = a.offs[d];
            const uint64_t at = d * L + (uint64_t)cg * W;
            uint32_t v[4];
            tky_load<I64, VEC>(a.dense, at, v);
#pragma unroll
            for (uint32_t q = 0; q < W; ++q) {
                const uint32_t j = j0 + q;
                if (j < k) a.out_ids[o0 + j] = v[q];
            }
        }
    }
}

hipError_t tk_launch_dense(const TkDenseArgs& args, int i64, hipStream_t s) {
    TkDenseArgs a = args;
    const TkyRowsGrid rg = tky_rows_shape(a.n_docs, a.row_len, false, a.rows);
    if (rg.x == 0u) return hipSuccess;
    TKY_LAUNCH_I64_MASK_VEC(tk_dense_kernel, i64, a.mask, a.row_len % 4u == 0u, dim3(rg.x, rg.y), s, a);
    return hipGetLastError();
}

hipError_t tk_launch_dense_maxlen(const uint64_t* id_offs, uint64_t n_docs, unsigned long long* stat, hipStream_t s) {
    if (n_docs == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_dense_maxlen_kernel, dim3(tky_blocks(n_docs, 2048u)), dim3(TKY_BLOCK), 0, s, id_offs, n_docs, stat);
    return hipGetLastError();
}

hipError_t tk_launch_ragged_rowlen(const TkRaggedArgs& a, int i64, hipStream_t s) {
    if (a.n_docs == 0) return hipSuccess;
    const dim3 grid(tky_blocks(a.n_docs, 1u << 16, a.given ? TKY_BLOCK : TKY_BLOCK / 64));   // a lane | a wave a row
    if (i64) hipLaunchKernelGGL(tk_dense_rowlen_kernel<1>, grid, dim3(TKY_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(tk_dense_rowlen_kernel<0>, grid, dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_ragged_copy(const TkRaggedArgs& a, int i64, hipStream_t s) {
    TkyRows shape;
    const TkyRowsGrid rg = tky_rows_shape(a.n_docs, a.row_len, false, shape);
    if (rg.x == 0u) return hipSuccess;
    TKY_LAUNCH_I64_VEC(tk_ragged_kernel, i64, a.row_len % 4u == 0u, dim3(rg.x, rg.y), s, a, shape);
    return hipGetLastError();
}
