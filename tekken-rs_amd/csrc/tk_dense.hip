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

#include "tk_dpp_scan.h"
#include "tk_kernels.h"

#define TKN_BLOCK 256
#define TKN_TILE 2048u     /* units of a block's row group (8 a thread); the reciprocal is exact for indices below it */

typedef uint32_t __attribute__((ext_vector_type(4))) tkn_u32x4;

// row of unit li inside the block's row group (li < TKN_TILE when rb > 1)
__device__ __forceinline__ uint32_t tkn_row_of(const TkDenseArgs& a, uint32_t li) {
    if (a.rb == 1u) return 0u;
    return a.units == 1u ? li : __umulhi(li, a.magic);
}

template <int I64, int MASK, int VEC, int NT>
__global__ __launch_bounds__(TKN_BLOCK) void tk_dense_kernel(TkDenseArgs a) {
    constexpr uint32_t W = VEC ? 4u : 1u;
    const uint32_t G = a.units, L = a.row_len;
    const uint64_t n_rb = (a.n_docs + a.rb - 1) / a.rb;
    uint32_t n_trunc = 0;
    for (uint64_t b = blockIdx.x; b < n_rb; b += gridDim.x) {
        const uint64_t row0 = b * a.rb;
        const uint32_t nrows = a.n_docs - row0 < a.rb ? (uint32_t)(a.n_docs - row0) : a.rb;
        const uint32_t total = nrows * G;      // rb > 1: <= TKN_TILE; rb == 1: G < 2^31
        for (uint32_t li = blockIdx.y * TKN_BLOCK + threadIdx.x; li < total; li += TKN_BLOCK * gridDim.y) {
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
            if (VEC) {
                if (I64) {
                    tkn_u32x4* p = reinterpret_cast<tkn_u32x4*>(reinterpret_cast<uint64_t*>(a.out) + at);
                    const tkn_u32x4 lo = {v[0], 0u, v[1], 0u}, hi = {v[2], 0u, v[3], 0u};
                    if (NT) { __builtin_nontemporal_store(lo, p); __builtin_nontemporal_store(hi, p + 1); }
                    else { p[0] = lo; p[1] = hi; }
                } else {
                    tkn_u32x4* p = reinterpret_cast<tkn_u32x4*>(reinterpret_cast<uint32_t*>(a.out) + at);
                    const tkn_u32x4 x = {v[0], v[1], v[2], v[3]};
                    if (NT) __builtin_nontemporal_store(x, p); else *p = x;
                }
                if (MASK) {
                    uint32_t* pm = reinterpret_cast<uint32_t*>(a.mask + at);
                    if (NT) __builtin_nontemporal_store(mbits, pm); else *pm = mbits;
                }
            } else {
                if (I64) reinterpret_cast<uint64_t*>(a.out)[at] = v[0];
                else reinterpret_cast<uint32_t*>(a.out)[at] = v[0];
                if (MASK) a.mask[at] = (uint8_t)mbits;
            }
        }
    }
    if (blockIdx.y == 0) {
        // the truncated documents of this wave's row leaders: one atomic per wave
        uint32_t s = tkd_scan_incl(n_trunc);
        s = (uint32_t)__builtin_amdgcn_readlane((int)s, 63);
        if ((threadIdx.x & 63u) == 0u && s) atomicAdd(a.stat + 1, (unsigned long long)s);
    }
}

// stat[0] = max over d of min(n_d, 2^32 - 1) (zeroed by the caller): what the longest-row mode sizes the tensor by
__global__ __launch_bounds__(TKN_BLOCK) void tk_dense_maxlen_kernel(const uint64_t* id_offs, uint64_t n_docs, unsigned long long* stat) {
    uint32_t m = 0;
    for (uint64_t d = (uint64_t)blockIdx.x * TKN_BLOCK + threadIdx.x; d < n_docs; d += (uint64_t)gridDim.x * TKN_BLOCK) {
        const uint64_t n = id_offs[d + 1] - id_offs[d];
        const uint32_t n32 = n < 0xFFFFFFFFull ? (uint32_t)n : 0xFFFFFFFFu;
        m = m > n32 ? m : n32;
    }
    m = (uint32_t)__builtin_amdgcn_readlane((int)tkd_scan_max(m), 63);
    if ((threadIdx.x & 63u) == 0u && m) atomicMax(stat, (unsigned long long)m);
}

// ---- dense -> ragged ----

// lens[d]: the given length clamped to the row (one lane a row), or -- given == NULL -- the row without the maximal run of
// pad_id at its padded end (one wave a row, 64 elements a step from that end; the first step usually decides)
template <int I64>
__global__ __launch_bounds__(TKN_BLOCK) void tk_dense_rowlen_kernel(TkRaggedArgs a) {
    const uint32_t L = a.row_len;
    if (a.given) {
        for (uint64_t d = (uint64_t)blockIdx.x * TKN_BLOCK + threadIdx.x; d < a.n_docs; d += (uint64_t)gridDim.x * TKN_BLOCK) {
            const uint32_t g = a.given[d];
            a.lens[d] = g < L ? g : L;
        }
        return;
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_waves = (uint64_t)gridDim.x * (TKN_BLOCK / 64);
    for (uint64_t d = (uint64_t)blockIdx.x * (TKN_BLOCK / 64) + (threadIdx.x >> 6); d < a.n_docs; d += n_waves) {
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
__global__ __launch_bounds__(TKN_BLOCK) void tk_ragged_kernel(TkRaggedArgs a, TkDenseArgs shape) {
    constexpr uint32_t W = VEC ? 4u : 1u;
    const uint32_t G = shape.units, L = a.row_len;
    const uint64_t n_rb = (a.n_docs + shape.rb - 1) / shape.rb;
    for (uint64_t b = blockIdx.x; b < n_rb; b += gridDim.x) {
        const uint64_t row0 = b * shape.rb;
        const uint32_t nrows = a.n_docs - row0 < shape.rb ? (uint32_t)(a.n_docs - row0) : shape.rb;
        const uint32_t total = nrows * G;
        for (uint32_t li = blockIdx.y * TKN_BLOCK + threadIdx.x; li < total; li += TKN_BLOCK * gridDim.y) {
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
            if (VEC) {
                if (I64) {
                    const tkn_u32x4* p = reinterpret_cast<const tkn_u32x4*>(reinterpret_cast<const uint64_t*>(a.dense) + at);
                    const tkn_u32x4 lo = p[0], hi = p[1];
                    v[0] = lo.x; v[1] = lo.z; v[2] = hi.x; v[3] = hi.z;
                } else {
                    const tkn_u32x4 x = *reinterpret_cast<const tkn_u32x4*>(reinterpret_cast<const uint32_t*>(a.dense) + at);
                    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
                }
            } else {
                v[0] = I64 ? (uint32_t)reinterpret_cast<const uint64_t*>(a.dense)[at] : reinterpret_cast<const uint32_t*>(a.dense)[at];
            }
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
    const uint64_t n_rb = (a.n_docs + a.rb - 1) / a.rb;
    uint32_t gy = 1;
    if (a.rb == 1u) {
        gy = (a.units + TKN_TILE - 1) / TKN_TILE;
        if (gy > 64u) gy = 64u;
    }
    grid = dim3((uint32_t)(n_rb < (1ull << 20) ? n_rb : (1ull << 20)), gy);
    return true;
}

template <int I64, int MASK>
static void tkn_launch2(const TkDenseArgs& a, dim3 grid, bool vec, bool nt, hipStream_t s) {
    if (!vec) hipLaunchKernelGGL((tk_dense_kernel<I64, MASK, 0, 0>), grid, dim3(TKN_BLOCK), 0, s, a);
    else if (nt) hipLaunchKernelGGL((tk_dense_kernel<I64, MASK, 1, 1>), grid, dim3(TKN_BLOCK), 0, s, a);
    else hipLaunchKernelGGL((tk_dense_kernel<I64, MASK, 1, 0>), grid, dim3(TKN_BLOCK), 0, s, a);
}

hipError_t tk_launch_dense(const TkDenseArgs& args, int i64, int nontemporal, hipStream_t s) {
    TkDenseArgs a = args;
    dim3 grid;
    if (!tkn_shape(a, grid)) return hipSuccess;
    const bool vec = a.row_len % 4u == 0u, nt = nontemporal != 0;
    if (i64 && a.mask) tkn_launch2<1, 1>(a, grid, vec, nt, s);
    else if (i64) tkn_launch2<1, 0>(a, grid, vec, nt, s);
    else if (a.mask) tkn_launch2<0, 1>(a, grid, vec, nt, s);
    else tkn_launch2<0, 0>(a, grid, vec, nt, s);
    return hipGetLastError();
}

hipError_t tk_launch_dense_maxlen(const uint64_t* id_offs, uint64_t n_docs, unsigned long long* stat, hipStream_t s) {
    if (n_docs == 0) return hipSuccess;
    uint64_t blocks = (n_docs + TKN_BLOCK - 1) / TKN_BLOCK;
    if (blocks > 2048u) blocks = 2048u;
    hipLaunchKernelGGL(tk_dense_maxlen_kernel, dim3((uint32_t)blocks), dim3(TKN_BLOCK), 0, s, id_offs, n_docs, stat);
    return hipGetLastError();
}

hipError_t tk_launch_ragged_rowlen(const TkRaggedArgs& a, int i64, hipStream_t s) {
    if (a.n_docs == 0) return hipSuccess;
    const uint64_t per_block = a.given ? TKN_BLOCK : TKN_BLOCK / 64;
    uint64_t blocks = (a.n_docs + per_block - 1) / per_block;
    if (blocks > (1u << 16)) blocks = 1u << 16;
    if (i64) hipLaunchKernelGGL(tk_dense_rowlen_kernel<1>, dim3((uint32_t)blocks), dim3(TKN_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(tk_dense_rowlen_kernel<0>, dim3((uint32_t)blocks), dim3(TKN_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_ragged_copy(const TkRaggedArgs& a, int i64, hipStream_t s) {
    TkDenseArgs shape = {};
    shape.n_docs = a.n_docs;
    shape.row_len = a.row_len;
    dim3 grid;
    if (!tkn_shape(shape, grid)) return hipSuccess;
    const bool vec = a.row_len % 4u == 0u;
    if (i64 && vec) hipLaunchKernelGGL((tk_ragged_kernel<1, 1>), grid, dim3(TKN_BLOCK), 0, s, a, shape);
    else if (i64) hipLaunchKernelGGL((tk_ragged_kernel<1, 0>), grid, dim3(TKN_BLOCK), 0, s, a, shape);
    else if (vec) hipLaunchKernelGGL((tk_ragged_kernel<0, 1>), grid, dim3(TKN_BLOCK), 0, s, a, shape);
    else hipLaunchKernelGGL((tk_ragged_kernel<0, 0>), grid, dim3(TKN_BLOCK), 0, s, a, shape);
    return hipGetLastError();
}
