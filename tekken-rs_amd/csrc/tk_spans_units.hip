// tk_spans_units.hip -- gfx950 kernels of the per-token spans in code points / UTF-16 units and of the annotation -> token range
// look-up (include/tekken_hip.h tk_token_spans_units_device, tk_spans_locate_device).
//
// tk_spans_units_kernel is a sibling of tk_spans_kernel (tk_spans.hip) with its launch shape: one wave per group of
// TK_DECODE_GROUP_DOCS documents, their ids as ONE stream, 64 ids a step, the ids requested two steps ahead, one 8-byte store per
// lane.  It reads no text: what a token adds comes from the 16-bit per-rank entries of tk_units_table.h, the first TKU_LDS ranks
// of them from an LDS copy (64 KB: two blocks of 1024 fit the 160 KB of a CU).  Two scans a step:
//   - the DPP prefix SUM of the tokens' units places every id in the group's text, counted in units (U of the definition);
//   - a DPP prefix MAXIMUM of (position of the token's last character start) + 1 over the tokens that hold one, carried across
//     steps, gives every id the last character start in front of it: where a token that begins inside a character is widened to.
// Neither is segmented.  The document an id belongs to begins where the last document start at or before its lane was placed
// (the byte kernel's prefix maximum of the marked starts); a character start of an EARLIER document lies in front of that, so
// clamping to the document's beginning is the reset: nothing carries across a document boundary.
//
// Error words (atomicMin):  err[2] first id index outside the vocabulary   err[3] first id index whose span ends at or beyond 2^32
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tk_dpp_scan.h"
#include "tk_kernels.h"
#include "tk_units_table.h"

#define TKU_BLOCK 1024        /* as TKS_BLOCK: 16 waves share one LDS copy of the table */
#define TKU_DOCS TK_DECODE_GROUP_DOCS
#define TKU_LDS 32768u        /* the entries of the ranks below this live in LDS */

__device__ __forceinline__ uint64_t tku_readlane64(uint64_t v, uint32_t l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l);
    return ((uint64_t)hi << 32) | lo;
}

// lane i receives lane i - 1's value, lane 0 receives 0 (DPP wave_shr:1)
__device__ __forceinline__ uint32_t tku_dn1(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xF, 0xF, false); }

// UTF16: 0 code points, 1 UTF-16 units
template <int UTF16>
__global__ __launch_bounds__(TKU_BLOCK, 8) void tk_spans_units_kernel(TkSpansUnitsArgs a) {
    __shared__ uint32_t tabw[TKU_LDS / 2];
    const uint32_t n_lds = a.n_ranks < TKU_LDS ? a.n_ranks : TKU_LDS;
    for (uint32_t q = threadIdx.x; q < (n_lds + 1u) / 2u; q += TKU_BLOCK) tabw[q] = reinterpret_cast<const uint32_t*>(a.tok_units)[q];
    __syncthreads();
    const uint16_t* tab = reinterpret_cast<const uint16_t*>(tabw);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * (TKU_BLOCK / 64) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (TKU_BLOCK / 64);
    const uint64_t n_groups = (a.n_docs + TKU_DOCS - 1) / TKU_DOCS;
    // what id adds: its units; units in front of its last character start + 1 (0: it holds none); its first byte starts a character
    // (a special id or one outside the vocabulary: no bytes, and its zero-length span sits at the current position)
    auto id_units = [&](uint32_t id, uint64_t i, uint32_t& un, uint32_t& last1, bool& first) {
        un = 0u; last1 = 0u; first = true;
        if (id < a.num_special) return;
        const uint32_t r = id - a.num_special;
        if (r >= a.n_ranks) {
            atomicMin(a.err + 2, (unsigned long long)i);
            return;
        }
        const uint32_t e = r < TKU_LDS ? (uint32_t)tab[r] : (uint32_t)a.tok_units[r];
        uint32_t n_start = e & 0xFFu, n_four = (e >> 8) & TKU_FOUR_MAX, last4 = (e >> 15) & 1u;
        first = (e & TKU_FIRST) != 0u;
        if (n_start == TKU_LONG) {                         // too long for an entry: count its bytes
            const uint8_t* t = a.tok_blob + a.tok_offs[r];
            const uint32_t len = a.tok_offs[r + 1] - a.tok_offs[r];
            n_start = 0u; n_four = 0u; last4 = 0u;
            first = len != 0u && (t[0] & 0xC0u) != 0x80u;
            for (uint32_t k = 0; k < len; ++k) {
                const uint32_t b = t[k];
                if ((b & 0xC0u) != 0x80u) { ++n_start; last4 = b >= 0xF0u ? 1u : 0u; }
                n_four += b >= 0xF0u ? 1u : 0u;
            }
        }
        un = UTF16 ? n_start + n_four : n_start;
        last1 = n_start ? (UTF16 ? n_start + n_four - last4 : n_start) : 0u;
    };
    for (uint64_t g = wave; g < n_groups; g += n_waves) {
        const uint64_t dA = g * TKU_DOCS, dB = dA + TKU_DOCS < a.n_docs ? dA + TKU_DOCS : a.n_docs;
        const uint32_t ndg = (uint32_t)(dB - dA);
        const uint64_t i0 = a.id_offs[dA], i1 = a.id_offs[dB];
        const uint64_t dfirst = lane < ndg ? a.id_offs[dA + lane] : ~0ull;    // lane j < ndg: the first id of document dA + j
        uint32_t jn = 0;                                   // the next document whose first id has not been placed (wave-uniform)
        uint64_t nfirst = tku_readlane64(dfirst, 0);
        uint64_t cursor = 0;                               // where the step's first id begins in the group's text, in units
        uint64_t base = 0;                                 // where the document of the step before's last id begins
        uint64_t lead = 0;                                 // the last character start of the steps before, + 1 (0: none yet)
        uint32_t id0 = i0 + lane < i1 ? a.ids[i0 + lane] : 0u;
        uint32_t id1 = i0 + 64 + lane < i1 ? a.ids[i0 + 64 + lane] : 0u;
        for (uint64_t c0 = i0; c0 < i1; c0 += 64) {
            const uint64_t i = c0 + lane;
            const bool have = i < i1;
            const uint32_t id2 = i + 128 < i1 ? a.ids[i + 128] : 0u;    // two steps ahead
            uint32_t un = 0u, last1 = 0u;
            bool first = true;
            if (have) id_units(id0, i, un, last1, first);
            const uint32_t incl = tkd_scan_incl(un), excl = incl - un;
            // documents whose first id is one of this step's 64: mark their lanes (scalar loop, the starts are in order)
            uint64_t starts = 0;
            while (nfirst < c0 + 64) {
                starts |= 1ull << (uint32_t)(nfirst - c0);
                ++jn;
                nfirst = jn < ndg ? tku_readlane64(dfirst, jn) : ~0ull;
            }
            const uint32_t m = tkd_scan_max((starts >> lane) & 1ull ? excl + 1u : 0u);
            const uint64_t dbase = m ? cursor + (m - 1u) : base;
            // the last character start at or before the ids in FRONT of this lane, + 1: this step's (exclusive: one lane down), or the carry
            const uint32_t pm = tkd_scan_max(last1 ? excl + last1 : 0u);
            const uint32_t before = tku_dn1(pm);
            const uint64_t ld = before ? cursor + before : lead;
            const uint64_t at = cursor + excl;
            const uint64_t from = first ? at : (ld > dbase ? ld - 1u : dbase);
            const uint64_t st = from - dbase, en = at + un - dbase;
            if (have) {
                if (en > 0xFFFFFFFFull) atomicMin(a.err + 3, (unsigned long long)i);
                typedef uint32_t __attribute__((ext_vector_type(2))) u32x2;
                reinterpret_cast<u32x2*>(a.spans)[i] = u32x2{(uint32_t)st, (uint32_t)en};
            }
            base = tku_readlane64(dbase, 63);
            const uint32_t pm63 = (uint32_t)__builtin_amdgcn_readlane((int)pm, 63);
            if (pm63) lead = cursor + pm63;
            cursor += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            id0 = id1; id1 = id2;
        }
    }
}

hipError_t tk_launch_spans_units(const TkSpansUnitsArgs& a, int unit, hipStream_t s) {
    if (a.n_docs == 0) return hipSuccess;
    const uint64_t n_groups = (a.n_docs + TKU_DOCS - 1) / TKU_DOCS;
    uint64_t blocks = (n_groups + TKU_BLOCK / 64 - 1) / (TKU_BLOCK / 64);
    if (blocks > 256u * 2u) blocks = 256u * 2u;             // every block copies 64 KB into its LDS first: no more than are resident
    if (unit == 2) hipLaunchKernelGGL(tk_spans_units_kernel<1>, dim3((uint32_t)blocks), dim3(TKU_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(tk_spans_units_kernel<0>, dim3((uint32_t)blocks), dim3(TKU_BLOCK), 0, s, a);
    return hipGetLastError();
}

// ---- annotation -> token range: one lane per annotation, two binary searches over the spans of its document ----
// (S and E are non-decreasing along a document; whatever the spans hold, every probe stays inside the document's id range,
// which is clamped to the n_ids the spans buffer has)
__global__ __launch_bounds__(256) void tk_spans_locate_kernel(TkLocateArgs a) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= a.n_ann) return;
    const uint32_t d = a.ann_doc[k];
    const uint32_t as = a.ann[2 * k], ae = a.ann[2 * k + 1];
    if (d >= a.n_docs || as > ae) {
        atomicMin(a.err, (unsigned long long)k);
        return;
    }
    uint64_t e = a.id_offs[(uint64_t)d + 1], b = a.id_offs[d];
    if (e > a.n_ids) e = a.n_ids;
    if (b > e) b = e;
    // lo = #{i : E_i <= as}
    uint64_t l = b, h = e;
    while (l < h) {
        const uint64_t mid = l + (h - l) / 2;
        if (a.spans[2 * mid + 1] <= as) l = mid + 1; else h = mid;
    }
    const uint64_t lo = l - b;
    // hi = #{i : S_i < ae}
    l = b; h = e;
    while (l < h) {
        const uint64_t mid = l + (h - l) / 2;
        if (a.spans[2 * mid] < ae) l = mid + 1; else h = mid;
    }
    const uint64_t hi = l - b;
    a.out[2 * k] = (uint32_t)lo;
    a.out[2 * k + 1] = (uint32_t)(hi > lo ? hi : lo);
}

hipError_t tk_launch_spans_locate(const TkLocateArgs& a, hipStream_t s) {
    if (a.n_ann == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_spans_locate_kernel, dim3((uint32_t)((a.n_ann + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
