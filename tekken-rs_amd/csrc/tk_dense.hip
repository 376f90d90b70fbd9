// tk_dense.hip -- gfx950 kernels of the model-ready dense layout (include/tekken_hip.h tk_dense_from_ids_device).
//
// No reference equivalent: the reference has pad_id() (src/tekkenizer.rs:304) and nothing that uses it.  Ragged ids + offsets in,
// dense[D, L] (+ mask[D, L], lengths[D], the truncated count) out, and the inverse.  Pure data movement: the bar is HBM.
//
// Kept ids of document d (n ids, limit lim, keep_head h, keep_tail t): k = min(n, lim) of them, and kept position j reads
//   ids[oo[d] + (j < split ? j : j + (n - k))],   split = TRUNC_LEFT ? h : lim - t
// (nothing is truncated: n - k == 0, every j reads itself).  Row d is those k ids and L - k pads, on the side PAD_LEFT says.
//
// Launch shape, shared by both directions: the unit of work is a group of 4 consecutive elements of one row where L % 4 == 0
// (one 16-byte store for int32, two for int64, one dword of mask), a single element otherwise.  A block takes `rb` consecutive
// rows (rb * G units <= TKN_TILE, G units a row) and its threads walk the rb * G units in order, so a wave covers several
// short rows and every lane has work; the row of a unit comes from a per-launch reciprocal (exact below TKN_TILE), not from a
// division.  A row of more than TKN_TILE units is one block row (rb == 1) split over blockIdx.y.  oo[d], oo[d + 1] and the
// arithmetic above are per unit; the source ids are dword loads (a row's source run starts at an arbitrary id).  Every output
// element is written exactly once, pad included.  The lane that holds a row's first unit writes lengths[d]; the truncated
// documents are counted per lane across the grid stride and added with one atomic per wave (a scan over the wave's lanes).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tk_kernels.h"
#include "tk_layout.h"

#define TKN_TILE 2048u     /* units of a block's row group (8 a thread); the reciprocal is exact for indices below it */

// row of unit li inside the block's row group (li < TKN_TILE when rb > 1)
__device__ __forceinline__ uint32_t tkn_row_of(const TkDenseArgs& a, uint32_t li) {
    if (a.rb == 1u) return 0u;
    return a.units == 1u ? li : __umulhi(li, a.magic);
}

template <int I64, int MASK, int VEC>
__global__ __launch_bounds__(TKY_BLOCK) void tk_dense_kernel(TkDenseArgs a) {
    constexpr uint32_t W = VEC ? 4u : 1u;
    const uint32_t G = a.units, L = a.row_len;
    const uint64_t n_rb = (a.n_docs + a.rb - 1) / a.rb;
    uint32_t n_trunc = 0;
    for (uint64_t b = blockIdx.x; b < n_rb; b += gridDim.x) {
        const uint64_t row0 = b * a.rb;
        const uint32_t nrows = a.n_docs - row0 < a.rb ? (uint32_t)(a.n_docs - row0) : a.rb;
        const uint32_t total = nrows * G;      // rb > 1: <= TKN_TILE; rb == 1: G < 2^31
        for (uint32_t li = blockIdx.y * TKY_BLOCK + threadIdx.x; li < total; li += TKY_BLOCK * gridDim.y) {
            const uint32_t r = tkn_row_of(a, li), cg = li - r * G;
            const uint64_t d = row0 + r;
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
            if (MASK) {
                if (VEC) *reinterpret_cast<uint32_t*>(a.mask + at) = mbits;
                else a.mask[at] = (uint8_t)mbits;
            }
        }
    }
    if (blockIdx.y == 0) tky_wave_add(a.stat + 1, n_trunc);   // the truncated documents of this wave's row leaders
}

// stat[0] = max over d of min(n_d, 2^32 - 1) (zeroed by the caller): what the longest-row mode sizes the tensor by
__global__ __launch_bounds__(TKY_BLOCK) void tk_dense_maxlen_kernel(const uint64_t* id_offs, uint64_t n_docs, unsigned long long* stat) {
    uint32_t m = 0;
    for (uint64_t d = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; d < n_docs; d += (uint64_t)gridDim.x * TKY_BLOCK) {
        const uint64_t n = id_offs[d + 1] - id_offs[d];
        const uint32_t n32 = n < 0xFFFFFFFFull ? (uint32_t)n : 0xFFFFFFFFu;
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

// out_ids[offs[d] + j] = the j-th element of row d's unpadded end, j < lens[d]; the launch shape of tk_dense_kernel
template <int I64, int VEC>
__global__ __launch_bounds__(TKY_BLOCK) void tk_ragged_kernel(TkRaggedArgs a, TkDenseArgs shape) {
    constexpr uint32_t W = VEC ? 4u : 1u;
    const uint32_t G = shape.units, L = a.row_len;
    const uint64_t n_rb = (a.n_docs + shape.rb - 1) / shape.rb;
    for (uint64_t b = blockIdx.x; b < n_rb; b += gridDim.x) {
        const uint64_t row0 = b * shape.rb;
        const uint32_t nrows = a.n_docs - row0 < shape.rb ? (uint32_t)(a.n_docs - row0) : shape.rb;
        const uint32_t total = nrows * G;
        for (uint32_t li = blockIdx.y * TKY_BLOCK + threadIdx.x; li < total; li += TKY_BLOCK * gridDim.y) {
            const uint32_t r = tkn_row_of(shape, li), cg = li - r * G;
            const uint64_t d = row0 + r;
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

// the launch shape of a [n_docs, row_len] tensor (see the head of this file); false: nothing to launch
static bool tkn_shape(TkDenseArgs& a, dim3& grid) {
    if (a.n_docs == 0 || a.row_len == 0) return false;
    const bool vec = a.row_len % 4u == 0u;
    a.units = vec ? a.row_len / 4u : a.row_len;
    a.rb = a.units <= TKN_TILE ? TKN_TILE / a.units : 1u;
    a.magic = a.units > 1u ? (uint32_t)((1ull << 32) / a.units) + 1u : 0u;
    uint32_t gy = 1;
    if (a.rb == 1u) {
        gy = (a.units + TKN_TILE - 1) / TKN_TILE;
        if (gy > 64u) gy = 64u;
    }
    grid = dim3(tky_blocks(a.n_docs, 1u << 20, a.rb), gy);
    return true;
}

template <int I64, int MASK>
static void tkn_launch2(const TkDenseArgs& a, dim3 grid, hipStream_t s) {
    if (a.row_len % 4u == 0u) hipLaunchKernelGGL((tk_dense_kernel<I64, MASK, 1>), grid, dim3(TKY_BLOCK), 0, s, a);
    else hipLaunchKernelGGL((tk_dense_kernel<I64, MASK, 0>), grid, dim3(TKY_BLOCK), 0, s, a);
}

hipError_t tk_launch_dense(const TkDenseArgs& args, int i64, hipStream_t s) {
    TkDenseArgs a = args;
    dim3 grid;
    if (!tkn_shape(a, grid)) return hipSuccess;
    if (i64 && a.mask) tkn_launch2<1, 1>(a, grid, s);
    else if (i64) tkn_launch2<1, 0>(a, grid, s);
    else if (a.mask) tkn_launch2<0, 1>(a, grid, s);
    else tkn_launch2<0, 0>(a, grid, s);
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
    TkDenseArgs shape = {};
    shape.n_docs = a.n_docs;
    shape.row_len = a.row_len;
    dim3 grid;
    if (!tkn_shape(shape, grid)) return hipSuccess;
    const bool vec = a.row_len % 4u == 0u;
    if (i64 && vec) hipLaunchKernelGGL((tk_ragged_kernel<1, 1>), grid, dim3(TKY_BLOCK), 0, s, a, shape);
    else if (i64) hipLaunchKernelGGL((tk_ragged_kernel<1, 0>), grid, dim3(TKY_BLOCK), 0, s, a, shape);
    else if (vec) hipLaunchKernelGGL((tk_ragged_kernel<0, 1>), grid, dim3(TKY_BLOCK), 0, s, a, shape);
    else hipLaunchKernelGGL((tk_ragged_kernel<0, 0>), grid, dim3(TKY_BLOCK), 0, s, a, shape);
    return hipGetLastError();
}
