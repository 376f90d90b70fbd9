// tk_layout.h -- what the layout kernels share (tk_dense.hip, tk_seqpack.hip, tk_join.hip, tk_window.hip, tk_chunk.hip,
// tk_pair.hip, tk_rowfit.hip, tk_regroup.hip: ragged ids into what a model consumes; tk_fim.hip, tk_noise.hip and
// tk_specials.hip, which cut and reorder text or ids in front of them):
// the 4-wide element access of an int32 / int64 tensor and the 4-wide gather of ids and spans at any dword, the stores of a uint8
// plane and of span pairs, the clamped length, the searches for "which document / part holds stream position g", the staging of a
// tile's starts, the block's row group of the row-group launch shape (tk_rows.h) and the owner of a row, the grid size, the
// I64 x VEC and I64 x MASK x VEC launches and the one-atomic-a-wave tails.  (Names: tky_ -- tkl_ is tk_long_impl.h's.)
#ifndef TK_LAYOUT_H
#define TK_LAYOUT_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tk_dpp_scan.h"
#include "tk_rows.h"

#define TKY_BLOCK 256
#define TKY_TILE 4096u     /* stream positions of a block's tile (16 a thread) */
#define TKY_CAP 1024u      /* starts of a tile that LDS holds (4 KiB) */

typedef uint32_t __attribute__((ext_vector_type(4))) tky_u32x4;
typedef uint32_t __attribute__((ext_vector_type(4), aligned(4))) tky_u32x4_a4;   /* a 16-byte load of ids at any dword */

// blocks for n items, `per` of them a block, at most cap
static inline uint32_t tky_blocks(uint64_t n, uint64_t cap, uint64_t per = TKY_BLOCK) {
    const uint64_t b = (n + per - 1) / per;
    return (uint32_t)(b < cap ? b : cap);
}

// kernel<I64, VEC> by two run-time flags
#define TKY_LAUNCH_I64_VEC(kernel, i64, vec, grid, s, ...)                                               \
    do {                                                                                                 \
        if ((i64) && (vec)) hipLaunchKernelGGL((kernel<1, 1>), grid, dim3(TKY_BLOCK), 0, s, __VA_ARGS__); \
        else if (i64) hipLaunchKernelGGL((kernel<1, 0>), grid, dim3(TKY_BLOCK), 0, s, __VA_ARGS__);       \
        else if (vec) hipLaunchKernelGGL((kernel<0, 1>), grid, dim3(TKY_BLOCK), 0, s, __VA_ARGS__);       \
        else hipLaunchKernelGGL((kernel<0, 0>), grid, dim3(TKY_BLOCK), 0, s, __VA_ARGS__);                \
    } while (0)
// kernel<I64, MASK, VEC> by three
#define TKY_LAUNCH_I64_MASK_VEC(kernel, i64, mask, vec, grid, s, ...)                                       \
    do {                                                                                                    \
        switch (((i64) ? 4 : 0) | ((mask) ? 2 : 0) | ((vec) ? 1 : 0)) {                                     \
        case 7: hipLaunchKernelGGL((kernel<1, 1, 1>), grid, dim3(TKY_BLOCK), 0, s, __VA_ARGS__); break;     \
        case 6: hipLaunchKernelGGL((kernel<1, 1, 0>), grid, dim3(TKY_BLOCK), 0, s, __VA_ARGS__); break;     \
        case 5: hipLaunchKernelGGL((kernel<1, 0, 1>), grid, dim3(TKY_BLOCK), 0, s, __VA_ARGS__); break;     \
        case 4: hipLaunchKernelGGL((kernel<1, 0, 0>), grid, dim3(TKY_BLOCK), 0, s, __VA_ARGS__); break;     \
        case 3: hipLaunchKernelGGL((kernel<0, 1, 1>), grid, dim3(TKY_BLOCK), 0, s, __VA_ARGS__); break;     \
        case 2: hipLaunchKernelGGL((kernel<0, 1, 0>), grid, dim3(TKY_BLOCK), 0, s, __VA_ARGS__); break;     \
        case 1: hipLaunchKernelGGL((kernel<0, 0, 1>), grid, dim3(TKY_BLOCK), 0, s, __VA_ARGS__); break;     \
        default: hipLaunchKernelGGL((kernel<0, 0, 0>), grid, dim3(TKY_BLOCK), 0, s, __VA_ARGS__);           \
        }                                                                                                   \
    } while (0)

// a length as the kernels carry it: clamped to 2^32 - 1 (the host refuses a clamped one before anything derived from it is used)
__device__ __forceinline__ uint32_t tky_len32(uint64_t n) { return n < 0xFFFFFFFFull ? (uint32_t)n : 0xFFFFFFFFu; }

// v[0 .. W) <-> elements at .. at + W of an int32 (I64 = 0) or int64 tensor, W = VEC ? 4 : 1 (VEC: at is a multiple of 4 and the
// tensor 16-byte aligned -- one 16-byte access for int32, two for int64)
template <int I64, int VEC>
__device__ __forceinline__ void tky_store(void* base, uint64_t at, const uint32_t* v) {
    if (VEC) {
        if (I64) {
            tky_u32x4* p = reinterpret_cast<tky_u32x4*>(reinterpret_cast<uint64_t*>(base) + at);
            const tky_u32x4 lo = {v[0], 0u, v[1], 0u}, hi = {v[2], 0u, v[3], 0u};
            p[0] = lo; p[1] = hi;
        } else {
            const tky_u32x4 x = {v[0], v[1], v[2], v[3]};
            *reinterpret_cast<tky_u32x4*>(reinterpret_cast<uint32_t*>(base) + at) = x;
        }
    } else {
        if (I64) reinterpret_cast<uint64_t*>(base)[at] = v[0];
        else reinterpret_cast<uint32_t*>(base)[at] = v[0];
    }
}
template <int I64, int VEC>
__device__ __forceinline__ void tky_load(const void* base, uint64_t at, uint32_t* v) {
    if (VEC) {
        if (I64) {
            const tky_u32x4* p = reinterpret_cast<const tky_u32x4*>(reinterpret_cast<const uint64_t*>(base) + at);
            const tky_u32x4 lo = p[0], hi = p[1];
            v[0] = lo.x; v[1] = lo.z; v[2] = hi.x; v[3] = hi.z;
        } else {
            const tky_u32x4 x = *reinterpret_cast<const tky_u32x4*>(reinterpret_cast<const uint32_t*>(base) + at);
            v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
        }
    } else {
        v[0] = I64 ? (uint32_t)reinterpret_cast<const uint64_t*>(base)[at] : reinterpret_cast<const uint32_t*>(base)[at];
    }
}

// ---- the 4-wide gather: four consecutive ids that lie at four consecutive source ids ----
// v[0 .. 4) = src[0 .. 4), src at any dword: ONE unaligned 16-byte load
__device__ __forceinline__ void tky_gather4(const uint32_t* src, uint32_t* v) {
    const tky_u32x4 x = *reinterpret_cast<const tky_u32x4_a4*>(src);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
}
// sp[0 .. 8) = the (start, end) pairs of ids s0 .. s0 + 3: two such loads
__device__ __forceinline__ void tky_gather4_spans(const uint32_t* spans, uint64_t s0, uint32_t* sp) {
    tky_gather4(spans + 2u * s0, sp);
    tky_gather4(spans + 2u * s0 + 4u, sp + 4);
}
// elements at .. at + W of a uint8 plane (mask, type_ids, sequence_ids) from the bytes of `bits`: one dword, or one byte
template <int VEC>
__device__ __forceinline__ void tky_store_plane(uint8_t* plane, uint64_t at, uint32_t bits) {
    if (VEC) *reinterpret_cast<uint32_t*>(plane + at) = bits;
    else plane[at] = (uint8_t)bits;
}
// the span pairs sp[0 .. 2 W) of elements at .. at + W of a [.., 2] tensor
template <int VEC>
__device__ __forceinline__ void tky_store_spans(uint32_t* out, uint64_t at, const uint32_t* sp) {
    tky_store<0, VEC>(out, 2u * at, sp);
    if (VEC) tky_store<0, 1>(out, 2u * at + 4u, sp + 4);
    else out[2u * at + 1u] = sp[1];
}

// the wave's sum / maximum of v into *dst with one atomic (none where it is 0); every lane of the wave calls it
__device__ __forceinline__ void tky_wave_add(unsigned long long* dst, uint32_t v) {
    const uint32_t s = (uint32_t)__builtin_amdgcn_readlane((int)tkd_scan_incl(v), 63);
    if ((threadIdx.x & 63u) == 0u && s) atomicAdd(dst, (unsigned long long)s);
}
__device__ __forceinline__ void tky_wave_max(unsigned long long* dst, uint32_t v) {
    const uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)tkd_scan_max(v), 63);
    if ((threadIdx.x & 63u) == 0u && m) atomicMax(dst, (unsigned long long)m);
}

// entries of the non-decreasing a[0 .. n) that are <= key (OR_EQ) or < key, one lane on its own
template <bool OR_EQ>
__device__ __forceinline__ uint64_t tky_count(const uint64_t* a, uint64_t n, uint64_t key) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (OR_EQ ? a[mid] <= key : a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ uint64_t tky_count_le(const uint64_t* a, uint64_t n, uint64_t key) { return tky_count<true>(a, n, key); }
__device__ __forceinline__ uint64_t tky_count_lt(const uint64_t* a, uint64_t n, uint64_t key) { return tky_count<false>(a, n, key); }

// Entries of the non-decreasing a[0 .. n) that are <= key.  The whole wave calls it with the same arguments: every step the
// 64 lanes probe the last entries of 64 equal parts of the range and a ballot keeps the one part the answer lies in.
// Ties are fine (tk_seqpack.hip passes a strictly increasing array, tk_join.hip one with runs of equal entries): all the search
// needs is that "a[p] <= key" holds on a prefix of the array and nowhere else.  The probes go up with the lane, so the ballot is
// a prefix of the lanes, c of them.  c < 64: probe c - 1 was not clamped to hi - 1 (a clamped probe is repeated by every later
// lane, which would make c = 64), so the entries up to lo + c * step - 1 hold, and the first probe that fails, at pc, bounds the
// answer from above.  The answer is therefore also the index of the LAST entry <= key, plus one.
__device__ __forceinline__ uint64_t tky_wave_count_le(const uint64_t* a, uint64_t n, uint64_t key) {
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t lo = 0, hi = n;                            // the answer is in [lo, hi]
    while (hi > lo) {
        const uint64_t step = (hi - lo + 63u) / 64u;
        uint64_t p = lo + (lane + 1u) * step - 1u;
        if (p >= hi) p = hi - 1u;
        const uint32_t c = (uint32_t)__builtin_popcountll(__ballot(a[p] <= key));   // a prefix of the lanes
        if (c == 64u) { lo = hi; break; }
        uint64_t pc = lo + (c + 1u) * step - 1u;        // the first probe above key: the answer is at most its index
        if (pc >= hi) pc = hi - 1u;
        lo += c * step;
        hi = pc;
    }
    return lo;
}

// ---- the starts inside a block's tile ----
// A block takes tile after tile of TKY_TILE consecutive stream positions; starts[0 .. n] is non-decreasing with starts[0] == 0,
// and the entry that holds position g is the LAST one with starts <= g.  Per tile, in this order and by every thread of the
// block (the barriers are inside; what the calls give back is block-uniform):
//   TkyTile<NK> tile(starts, g0)   the tile that begins at position g0; never opened, it holds no entry
//   search(n, keys...), found(i)   NK waves find, one wave search each, how many starts lie at or before NK keys (the first: g0)
//   open(n_lo, count)              the tile's entries: n_lo - 1, which holds g0, and the `count` behind it, which start inside
//   stage() / stage(rec)           at most TKY_CAP of them: their starts go to LDS relative to g0, and rec(j, e) puts what else a
//                                  unit needs of entry e = n_lo - 1 + j beside them at [j], j <= count (coalesced, once a tile);
//                                  more (many one-element entries): nothing is staged and rel() reads global memory.  Decided per
//                                  block; `lds` says which
//   rel(j), count_le(x), start_of(k)   what a unit resolves its positions with
// ONE TkyTile<NK> a kernel: the LDS arrays belong to the type, a second object of it would share them.
template <int NK>
struct TkyTile {
    uint32_t* s_rel;                // LDS [TKY_CAP]: the starts inside the tile, relative to its first position
    uint64_t* s_cnt;                // LDS [NK]
    const uint64_t* starts;
    uint64_t g0, n_lo = 0;
    uint64_t start_lo = 0;          // where entry n_lo - 1 starts: at or before g0
    uint32_t count = 0;
    bool lds = true;
    __device__ __forceinline__ TkyTile(const uint64_t* starts_, uint64_t first) : starts(starts_), g0(first) {
        __shared__ uint32_t rel_[TKY_CAP];
        __shared__ uint64_t cnt_[NK];
        s_rel = rel_; s_cnt = cnt_;
    }

    __device__ __forceinline__ void search(uint64_t n, uint64_t k0, uint64_t k1, uint64_t k2 = 0) {
        const uint32_t wave = threadIdx.x >> 6;
        __syncthreads();                                // (the previous tile's readers of the shared arrays are done)
        if (wave < (uint32_t)NK) {
            const uint64_t c = tky_wave_count_le(starts, n, wave == 0u ? k0 : (NK == 2 || wave == 1u) ? k1 : k2);
            if ((threadIdx.x & 63u) == 0u) s_cnt[wave] = c;
        }
        __syncthreads();
    }
    // the starts at or before key i of the last search
    __device__ __forceinline__ uint64_t found(int i) const { return s_cnt[i]; }
    template <class N>              // (the count in the caller's width: 32 bits where it is known to be below TKY_TILE)
    __device__ __forceinline__ void open(uint64_t lo, N n_inside) {
        n_lo = lo; count = (uint32_t)n_inside;
        lds = n_inside <= TKY_CAP;
    }
    __device__ __forceinline__ void stage() {
        if (lds) {
            for (uint32_t j = threadIdx.x; j < count; j += TKY_BLOCK) s_rel[j] = (uint32_t)(starts[n_lo + j] - g0);
            __syncthreads();
        }
        start_lo = starts[n_lo - 1u];
    }
    template <class F>
    __device__ __forceinline__ void stage(F rec) {
        if (lds) {
            for (uint32_t j = threadIdx.x; j <= count; j += TKY_BLOCK) {
                const uint64_t e = n_lo - 1u + j;
                if (j) s_rel[j - 1u] = (uint32_t)(starts[e] - g0);
                rec(j, e);
            }
            __syncthreads();
        }
        start_lo = starts[n_lo - 1u];
    }
    // start of the tile's entry j + 1 relative to the tile, j < count
    __device__ __forceinline__ uint32_t rel(uint32_t j) const { return lds ? s_rel[j] : (uint32_t)(starts[n_lo + j] - g0); }
    // the tile's entries that start at or before relative position x: entry n_lo - 1 + the result holds it
    __device__ __forceinline__ uint32_t count_le(uint32_t x) const {
        uint32_t lo = 0, hi = count;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (rel(mid) <= x) lo = mid + 1u; else hi = mid;
        }
        return lo;
    }
    // where the tile's entry k starts, relative to the tile
    __device__ __forceinline__ int64_t start_of(uint32_t k) const { return k ? (int64_t)rel(k - 1u) : -(int64_t)(g0 - start_lo); }
};

// ---- the block's part of the row-group launch shape (tk_rows.h) ----
//   for (uint64_t b = blockIdx.x; b < tky_row_groups(shape, n_rows); b += gridDim.x) {
//       const TkyRowGroup g(shape, n_rows, b);
//       for (uint32_t li = g.first(); li < g.total; li += g.step()) {
//           const uint32_t r = tky_row_of(shape, li), cg = li - r * shape.units;     // unit cg of row g.row0 + r
struct TkyRowGroup {
    uint64_t row0;                  // the group's first row
    uint32_t nrows, total;          // its rows (rb, fewer in the last group) and units: rb > 1: <= TKY_ROWS_TILE; rb == 1: units < 2^31
    __device__ __forceinline__ TkyRowGroup(const TkyRows& s, uint64_t n_rows, uint64_t b) : row0(b * s.rb) {
        nrows = n_rows - row0 < s.rb ? (uint32_t)(n_rows - row0) : s.rb;
        total = nrows * s.units;
    }
    __device__ __forceinline__ static uint32_t first() { return blockIdx.y * TKY_BLOCK + threadIdx.x; }
    __device__ __forceinline__ static uint32_t step() { return TKY_BLOCK * gridDim.y; }
};

// Which owner (document, pair) holds each row of a row group: starts[0 .. n_owners] is the exclusive scan of the owners' row
// counts, strictly increasing.  Two waves find, one 64-ary search each, the owners of the group's first and last row; the starts
// of the owners in between go to LDS relative to the group's first row, and rec(j, e) puts what a unit needs of owner e beside
// them at [j] (TkyTile::stage).  More than TKY_CAP owners in the run (rows of 4 elements over one-row owners): nothing is staged
// and the caller reads the same values from global memory where !lds, decided per block.  Per unit, for row r of the group,
// with the tile's own members:
//   kd = count_le(r)              [kd] of what rec staged: a binary search over at most rb entries
//   n_lo - 1 + kd                 the owner's index
//   r - start_of(kd)              the row's number inside its owner
// (written out by the kernels: behind accessors of this struct the compiler orders tk_window_kernel's and tk_pair_kernel's
// instructions otherwise, and with one for the owner's index tk_window_kernel's per-block prologue grows by four instructions).
// ONE a kernel (it is the kernel's TkyTile<2>).
struct TkyRowOwners : TkyTile<2> {
    template <class F>
    __device__ __forceinline__ TkyRowOwners(const uint64_t* starts, uint64_t n_owners, const TkyRowGroup& g, F rec) : TkyTile<2>(starts, g.row0) {
        search(n_owners, g.row0, g.row0 + g.nrows - 1u);    // owners that start at or before: the first row (>= 1) | the last row
        const uint64_t lo = found(0);
        open(lo, (uint32_t)(found(1) - lo));                // owners that start in (row0, row0 + nrows): < nrows
        stage(rec);
    }
};

#endif
