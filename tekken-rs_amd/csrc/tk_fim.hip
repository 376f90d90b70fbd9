// tk_fim.hip -- gfx950 kernels of the fill-in-the-middle pass (include/tekken_hip.h tk_fim_split_device).
//
// No reference equivalent.  The packed units (text bytes: U = 1; ids: U = 4) of D documents in; every chosen document cut in two
// places into prefix, middle and suffix and written back in the order [SUFFIX] S [PREFIX] P M or [PREFIX] P [SUFFIX] S [MIDDLE] M
// inside its own range, with the five part records a document that tk_encode_parts_device_join / tk_join_from_ids_device take.
//
//   a. tk_fim_cut_kernel<U>: one thread a document.  The four draws are hashes of (seed, d), so nothing is carried between
//      documents; the snap of a cut steps back over at most 3 continuation bytes, one byte read each; the part records need no scan
//      (5 a document, and a document keeps its range).  The three counters: one atomic a wave (tky_wave_add).
//   b. tk_fim_permute_kernel<U>: the join / regroup / compaction kernel shape (tk_layout.h) over output units.  A block takes
//      tiles of TKI_TILE1 bytes or TKI_TILE4 ids; two wave searches over offs find the tile's documents; their (lo, hi, n, mode)
//      go to LDS beside their starts -- the cuts, not the part tables: in its own range a document is a head that stays, three
//      ranges of the body that each moved by one distance, and a tail that stays.  A thread resolves 16 bytes: where they lie
//      in one range (or in an untransformed document) ONE 16-byte load at any byte -- odd cuts leave source and destination
//      mutually misaligned -- and one aligned 16-byte store; over a seam or a document boundary it walks unit by unit.  Every
//      output unit is written exactly once; a source index is used only where it lies inside [0, n_units).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tk_kernels.h"
#include "tk_layout.h"

typedef uint32_t __attribute__((ext_vector_type(4), aligned(1))) tki_u32x4_a1;   /* a 16-byte load of text at any byte */

template <int U> struct TkiUnit;
template <> struct TkiUnit<1> { typedef uint8_t type; typedef tki_u32x4_a1 load16; enum : uint32_t { TILE = TKI_TILE1, PER = 16u }; };
template <> struct TkiUnit<4> { typedef uint32_t type; typedef tky_u32x4_a4 load16; enum : uint32_t { TILE = TKI_TILE4, PER = 4u }; };

// ---- a. the cuts and the part records ----

// step 3 of the definition: back over at most 3 continuation bytes (b: the body's first byte)
__device__ __forceinline__ uint64_t tki_snap(const uint8_t* b, uint64_t c, uint64_t n) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (c == 0 || c >= n || (b[c] & 0xC0u) != 0x80u) break;
        --c;
    }
    return c;
}

template <int U>
__global__ __launch_bounds__(TKY_BLOCK) void tk_fim_cut_kernel(TkFimArgs a) {
    const uint64_t D = a.n_docs;
    const uint64_t n_iter = (D + 1u + (uint64_t)gridDim.x * TKY_BLOCK - 1u) / ((uint64_t)gridDim.x * TKY_BLOCK);
    const uint32_t all = TK_PART_LABEL_CTRL | TK_PART_LABEL_TEXT;
    uint32_t n_tr = 0, n_spm = 0, n_skip = 0;
    for (uint64_t it = 0; it < n_iter; ++it) {          // (every lane stays to the wave sums below)
        const uint64_t d = (it * gridDim.x + blockIdx.x) * TKY_BLOCK + threadIdx.x;
        if (d > D) continue;
        a.conv_offs[d] = 5u * d;
        if (d == D) { a.part_offs[5u * D] = a.offs[D]; continue; }
        const uint64_t start = a.offs[d], end = a.offs[d + 1u];
        const uint64_t len = end >= start ? end - start : 0u;
        const uint64_t ht = (uint64_t)a.head + a.tail;
        const bool whole = len >= ht;                   // the head and the tail are there
        const uint64_t h = whole ? a.head : 0u, n = whole ? len - ht : len;
        const uint32_t dd = (uint32_t)d;
        uint64_t c0 = 0, c1 = 0;
        bool cand, ok;
        if (a.in_cuts) {
            c0 = a.in_cuts[2u * d];
            c1 = a.in_cuts[2u * d + 1u];
            cand = c0 != TK_FIM_NO_CUT;
            ok = whole && n < 0xFFFFFFFFull;
            c0 = c0 < n ? c0 : n;
            c1 = c1 < n ? c1 : n;
        } else {
            cand = (uint64_t)tki_hash(a.s[0], dd) < a.rate;
            ok = whole && n >= (a.min_units ? a.min_units : 1u) && n < 0xFFFFFFFFull;
            if (cand && ok) {
                c0 = ((uint64_t)tki_hash(a.s[2], dd) * (n + 1u)) >> 32;
                c1 = ((uint64_t)tki_hash(a.s[3], dd) * (n + 1u)) >> 32;
            }
        }
        const bool tr = cand && ok;
        const bool spm = tr && (uint64_t)tki_hash(a.s[1], dd) < a.spm;
        if (U == 1 && tr && (a.flags & TK_FIM_SNAP) && end <= a.n_units) {   // (offsets that point behind the text: nothing is read there)
            const uint8_t* body = (const uint8_t*)a.units + start + h;
            c0 = tki_snap(body, c0, n);
            c1 = tki_snap(body, c1, n);
        }
        const uint64_t lo = c0 < c1 ? c0 : c1, hi = c0 < c1 ? c1 : c0;
        n_tr += tr; n_spm += spm; n_skip += cand && !tr;
        a.mode[d] = tr ? (spm ? 2u : 1u) : 0u;
        a.cuts[2u * d] = tr ? lo : TK_FIM_NO_CUT;
        a.cuts[2u * d + 1u] = tr ? hi : TK_FIM_NO_CUT;
        // the five parts: where each starts in the output, and in the input
        const uint64_t b0 = start + h, b1 = b0 + n;     // the body
        uint64_t o[5] = {start, b0, b1, b1, b1}, src[5] = {start, b0, b1, b1, b1};
        uint32_t ctrl[5] = {a.bos, TK_JOIN_NONE, TK_JOIN_NONE, TK_JOIN_NONE, a.eos};
        uint32_t fl[5] = {all, all, all, all, all};
        if (tr) {
            if (spm) {                                  // S | P | M
                o[2] = b0 + (n - hi); o[3] = o[2] + lo;
                src[1] = b0 + hi; src[2] = b0; src[3] = b0 + lo;
                ctrl[1] = a.ctrl[1]; ctrl[2] = a.ctrl[0];
            } else {                                    // P | S | M
                o[2] = b0 + lo; o[3] = o[2] + (n - hi);
                src[1] = b0; src[2] = b0 + hi; src[3] = b0 + lo;
                ctrl[1] = a.ctrl[0]; ctrl[2] = a.ctrl[1];
            }
            ctrl[3] = a.ctrl[2];
            if (a.flags & TK_FIM_LABEL_MIDDLE) { fl[0] = fl[1] = fl[2] = 0u; fl[3] = TK_PART_LABEL_TEXT; }
        }
#pragma unroll
        for (uint32_t p = 0; p < 5u; ++p) {
            a.part_offs[5u * d + p] = o[p];
            a.part_ctrl[5u * d + p] = ctrl[p];
            a.part_flags[5u * d + p] = fl[p];
            if (a.part_src) a.part_src[5u * d + p] = src[p];
        }
    }
    tky_wave_add(a.stat, n_tr);
    tky_wave_add(a.stat + 1, n_spm);
    tky_wave_add(a.stat + 2, n_skip);
}

// ---- b. the units in the new order ----

// What the permute kernel knows of a document: the cuts and the body's length (32 bits each: a transformed body is shorter than
// 2^32 - 1), the mode, and TKI_HT where the document has its head and tail.  Of an untransformed one only mode == 0 is read.
struct TkiDoc { uint32_t lo, hi, n, mode; };

__device__ __forceinline__ TkiDoc tki_doc(const TkFimArgs& a, uint64_t e) {
    TkiDoc r;
    r.mode = a.mode[e];
    r.lo = r.hi = r.n = 0u;
    if (r.mode) {
        const uint64_t len = a.offs[e + 1u] - a.offs[e], ht = (uint64_t)a.head + a.tail;
        r.lo = (uint32_t)a.cuts[2u * e];
        r.hi = (uint32_t)a.cuts[2u * e + 1u];
        r.n = (uint32_t)(len - ht);                     // (transformed: len >= head + tail)
        r.mode |= TKI_HT;
    }
    return r;
}

// Unit r of a transformed document's output range: *shift = where it lies in the input relative to where it lies in the output,
// and the range it belongs to (0 head, 1 .. 3 the body's three, 4 tail) comes back.
__device__ __forceinline__ uint32_t tki_range(const TkiDoc& k, uint32_t head, uint64_t r, int64_t* shift) {
    const uint64_t h = (k.mode & TKI_HT) ? head : 0u;
    const int64_t lo = k.lo, hi = k.hi, n = k.n;
    const bool spm = (k.mode & 3u) == 2u;
    const uint64_t e1 = h + (uint64_t)(spm ? n - hi : lo), e2 = e1 + (uint64_t)(spm ? lo : n - hi), e3 = h + (uint64_t)n;
    const uint32_t seg = (uint32_t)(r >= h) + (uint32_t)(r >= e1) + (uint32_t)(r >= e2) + (uint32_t)(r >= e3);
    // PSM: P stays, S comes from hi, M from lo.  SPM: S comes from hi, P and M move together behind it
    const int64_t s1 = spm ? hi : 0, s2 = spm ? -(n - hi) : hi - lo, s3 = -(n - hi);
    *shift = seg == 1u ? s1 : seg == 2u ? s2 : seg == 3u ? s3 : 0;
    return seg;
}

template <int U>
__global__ __launch_bounds__(TKY_BLOCK) void tk_fim_permute_kernel(TkFimArgs a) {
    typedef typename TkiUnit<U>::type unit_t;
    typedef typename TkiUnit<U>::load16 load16_t;
    constexpr uint32_t TILE = TkiUnit<U>::TILE, PER = TkiUnit<U>::PER;
    __shared__ TkiDoc s_doc[TKY_CAP + 1];               // the tile's documents: [0] is the one that holds g0
    const unit_t* in = (const unit_t*)a.units;
    unit_t* out = (unit_t*)a.out_units;
    const uint64_t N = a.n_units, D = a.n_docs;
    const uint64_t n_tiles = (N + TILE - 1) / TILE;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t g0 = t * TILE;
        const uint64_t g1 = N - g0 < TILE ? N : g0 + TILE;
        TkyTile<2> tile(a.offs, g0);
        tile.search(D, g0, g1 - 1u);                    // documents that start at or before the tile's first | last unit
        const uint64_t n_lo = tile.found(0);            // (block-uniform, as everything up to the unit loop; >= 1: offs[0] == 0)
        if (n_lo == 0 || tile.found(1) < n_lo) continue;
        tile.open(n_lo, tile.found(1) - n_lo);          // starts in (g0, g1): documents n_lo .. n_lo + count - 1, empty ones included
        tile.stage([&](uint32_t j, uint64_t e) { s_doc[j] = tki_doc(a, e); });
        auto doc_of = [&](uint32_t j) -> TkiDoc { return tile.lds ? s_doc[j] : tki_doc(a, n_lo - 1u + j); };
        const uint32_t len = (uint32_t)(g1 - g0);
        for (uint32_t l = threadIdx.x * PER; l < len; l += TKY_BLOCK * PER) {
            const uint64_t g = g0 + l;
            uint32_t k = tile.count_le(l);
            TkiDoc doc = doc_of(k);
            int64_t start = tile.start_of(k);
            // the common unit: 16 bytes of one range of one document -- one load of 16 bytes at any byte, one aligned store
            if (l + PER <= len && (k == tile.count || tile.rel(k) >= l + PER)) {
                int64_t sh = 0;
                bool one = true;
                if (doc.mode) {
                    int64_t sh1;
                    const uint64_t r = (uint64_t)((int64_t)l - start);
                    const uint32_t first = tki_range(doc, a.head, r, &sh), last = tki_range(doc, a.head, r + PER - 1u, &sh1);
                    one = first == last || (last == first + 1u && sh == sh1);   // (neighbours that moved together: SPM's P and M, PSM's head and P)
                }
                const uint64_t s = g + (uint64_t)sh;
                if (one && s < N && N - s >= PER) {
                    *reinterpret_cast<tky_u32x4*>(out + g) = *reinterpret_cast<const load16_t*>(in + s);
                    continue;
                }
            }
            uint32_t v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (uint32_t q = 0; q < PER; ++q) {
                if (l + q >= len) break;
                if (k < tile.count && tile.rel(k) <= l + q) {   // another document (over empty ones too: the LAST that starts at or before the unit)
                    do ++k; while (k < tile.count && tile.rel(k) <= l + q);
                    doc = doc_of(k);
                    start = (int64_t)tile.rel(k - 1u);
                }
                int64_t sh = 0;
                if (doc.mode) (void)tki_range(doc, a.head, (uint64_t)((int64_t)(l + q) - start), &sh);
                const uint64_t s = g + q + (uint64_t)sh;
                const uint32_t x = s < N ? (uint32_t)in[s] : 0u;
                if (U == 1) v[q >> 2] |= x << (8u * (q & 3u));
                else v[q] = x;
            }
            if (l + PER <= len) {
                const tky_u32x4 x = {v[0], v[1], v[2], v[3]};
                *reinterpret_cast<tky_u32x4*>(out + g) = x;
            } else {                                    // the last units of the stream
                for (uint32_t q = 0; l + q < len; ++q) out[g + q] = U == 1 ? (unit_t)(v[q >> 2] >> (8u * (q & 3u))) : (unit_t)v[q];
            }
        }
    }
}

hipError_t tk_launch_fim_cut(const TkFimArgs& a, int unit_bytes, hipStream_t s) {
    const dim3 grid(tky_blocks(a.n_docs + 1u, 1u << 16));
    if (unit_bytes == 1) hipLaunchKernelGGL(tk_fim_cut_kernel<1>, grid, dim3(TKY_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(tk_fim_cut_kernel<4>, grid, dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_fim_permute(const TkFimArgs& a, int unit_bytes, hipStream_t s) {
    if (a.n_units == 0 || a.n_docs == 0) return hipSuccess;
    if (unit_bytes == 1) hipLaunchKernelGGL(tk_fim_permute_kernel<1>, dim3(tky_blocks(a.n_units, 1u << 20, TKI_TILE1)), dim3(TKY_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(tk_fim_permute_kernel<4>, dim3(tky_blocks(a.n_units, 1u << 20, TKI_TILE4)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}
