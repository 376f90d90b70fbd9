// tk_spans.hip -- gfx950 kernel of the per-token byte spans (include/tekken_hip.h tk_token_spans_device).
//
// No reference equivalent: its nearest relative, Tekkenizer::decode_all (src/tekkenizer.rs:463-560), gives per-segment
// strings, not positions in the input.  Encode is lossless (byte-level BPE tiles the text, and the only specials encode emits
// are BOS / EOS), so the span of output id i of document d is an exclusive prefix sum, per document, of the byte lengths of
// the ids (a special id: 0): spans[2i], spans[2i+1] = (start, end), uint32, relative to the start of document d.
//
// Launch shape of tk_decode_grouplen_kernel / tk_decode_emit_kernel: one wave per group of TK_DECODE_GROUP_DOCS
// consecutive documents, their ids as ONE stream, 64 ids a step, the ids requested two steps ahead.  A length comes from an LDS
// copy of the one-byte length table (its first 32 K ranks).  The step's DPP prefix sum places every id in the group's text;
// the document an id belongs to begins where the last document start at or before its lane was placed (a DPP prefix MAXIMUM
// of the marked starts, carried across steps), so the scan "resets" at document starts without a segmented scan.  One 8-byte
// store per lane, coalesced across the wave.
//
// Checks in the same pass (TK_SPANS_CHECK_*): COVER -- at the group's end, lane j compares where document j's text ends with
// doc_offs; BYTES -- every non-special id compares its token bytes with the text under its span.  Error words (atomicMin):
//   err[0] first document whose spans do not cover it      err[1] first id index whose bytes differ from the text
//   err[2] first id index outside the vocabulary           err[3] first id index whose span ends at or beyond 2^32
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tk_dpp_scan.h"
#include "tk_kernels.h"

#define TKS_BLOCK 1024        /* 16 waves share one LDS copy of the length table: two blocks fill a CU's wave slots (<= 64 VGPRs: the launch bounds ask for 8 waves per SIMD) */
#define TKS_DOCS TK_DECODE_GROUP_DOCS
#define TKS_L8_LDS 32768u     /* one-byte lengths of the ranks below this live in LDS */

__device__ __forceinline__ uint64_t tks_readlane64(uint64_t v, uint32_t l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l);
    return ((uint64_t)hi << 32) | lo;
}

typedef uint32_t __attribute__((ext_vector_type(4))) tks_u32x4;

// the inline entry of id (requested a step ahead of its use; zeros for a special id or one outside the vocabulary, which skip the check)
__device__ __forceinline__ tks_u32x4 tks_entry(const TkSpansArgs& a, uint32_t id, bool have) {
    tks_u32x4 v = {0u, 0u, 0u, 0u};
    const uint32_t r = id - a.num_special;
    if (have && id >= a.num_special && r < a.n_ranks) v = *reinterpret_cast<const tks_u32x4*>(a.tok_inline + 16ull * r);
    return v;
}

// does the text at bytes[gpos .. gpos + len) hold the token bytes of rank r (inline entry e)?  Inline entries (<= 15 bytes): the text is read as
// the aligned dwords that hold it (none starts past the span's last byte: no load leaves the pages of the caller's buffer) and
// aligned with v_alignbyte; longer tokens compare byte by byte against tok_blob.
__device__ __forceinline__ bool tks_bytes_equal(const TkSpansArgs& a, uint32_t r, const tks_u32x4& e, uint64_t gpos, uint32_t len) {
    if ((e.w >> 24) == 0xFFu) {
        const uint8_t* t = a.tok_blob + a.tok_offs[r];
        uint32_t diff = 0;
        for (uint32_t k = 0; k < len; ++k) diff |= (uint32_t)(t[k] ^ a.bytes[gpos + k]);
        return diff == 0;
    }
    const uintptr_t at = reinterpret_cast<uintptr_t>(a.bytes + gpos);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(at & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(at & 3u);
    uint32_t w[5];
#pragma unroll
    for (uint32_t k = 0; k < 5u; ++k) w[k] = 4u * k < sh + len ? q[k] : 0u;
    const uint32_t tok[4] = {e.x, e.y, e.z, e.w};
    uint32_t diff = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t t = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh);
        const uint32_t have = len > 4u * k ? len - 4u * k : 0u;
        diff |= (t ^ tok[k]) & (have >= 4u ? 0xFFFFFFFFu : (1u << (8u * have)) - 1u);
    }
    return diff == 0;
}

// CHK: 0 spans only, 1 + TK_SPANS_CHECK_COVER, 2 + TK_SPANS_CHECK_BYTES
template <int CHK>
__global__ __launch_bounds__(TKS_BLOCK, 8) void tk_spans_kernel(TkSpansArgs a) {
    __shared__ uint32_t l8w[TKS_L8_LDS / 4];
    const uint32_t n_lds = a.n_ranks < TKS_L8_LDS ? a.n_ranks : TKS_L8_LDS;
    for (uint32_t q = threadIdx.x; q < (n_lds + 3u) / 4u; q += TKS_BLOCK) l8w[q] = reinterpret_cast<const uint32_t*>(a.tok_len8)[q];
    __syncthreads();
    const uint8_t* l8 = reinterpret_cast<const uint8_t*>(l8w);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * (TKS_BLOCK / 64) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (TKS_BLOCK / 64);
    const uint64_t n_groups = (a.n_docs + TKS_DOCS - 1) / TKS_DOCS;
    auto id_len = [&](uint32_t id, uint64_t i) -> uint32_t {
        if (id < a.num_special) return 0u;
        const uint32_t r = id - a.num_special;
        if (r >= a.n_ranks) {
            atomicMin(a.err + 2, (unsigned long long)i);
            return 0u;
        }
        uint32_t len = r < TKS_L8_LDS ? (uint32_t)l8[r] : (uint32_t)a.tok_len8[r];
        if (len == 0xFFu) len = a.tok_offs[r + 1] - a.tok_offs[r];
        return len;
    };
    for (uint64_t g = wave; g < n_groups; g += n_waves) {
        const uint64_t dA = g * TKS_DOCS, dB = dA + TKS_DOCS < a.n_docs ? dA + TKS_DOCS : a.n_docs;
        const uint32_t ndg = (uint32_t)(dB - dA);
        const uint64_t i0 = a.id_offs[dA], i1 = a.id_offs[dB];
        // lane j < ndg: the first id of document dA + j, and -- once a step has placed it -- where its text begins in the group's
        // text (unset: an empty document at the group's very end, which begins where the group's text ends)
        const uint64_t dfirst = lane < ndg ? a.id_offs[dA + lane] : ~0ull;
        uint64_t dpos = ~0ull;
        uint32_t jn = 0;                                   // the next document whose first id has not been placed (wave-uniform)
        uint64_t nfirst = tks_readlane64(dfirst, 0);
        uint64_t cursor = 0;                               // where the step's first id begins in the group's text
        uint64_t base = 0;                                 // where the document of the step before's last id begins
        const uint64_t tbase = CHK == 2 ? a.doc_offs[dA] : 0, tend = CHK == 2 ? a.doc_offs[dB] : 0;
        uint32_t id0 = i0 + lane < i1 ? a.ids[i0 + lane] : 0u;
        uint32_t id1 = i0 + 64 + lane < i1 ? a.ids[i0 + 64 + lane] : 0u;
        tks_u32x4 e0 = {0u, 0u, 0u, 0u};
        if (CHK == 2) e0 = tks_entry(a, id0, i0 + lane < i1);
        for (uint64_t c0 = i0; c0 < i1; c0 += 64) {
            const uint64_t i = c0 + lane;
            const bool have = i < i1;
            const uint32_t id2 = i + 128 < i1 ? a.ids[i + 128] : 0u;    // two steps ahead
            tks_u32x4 e1 = {0u, 0u, 0u, 0u};
            if (CHK == 2) e1 = tks_entry(a, id1, i + 64 < i1);          // one step ahead
            const uint32_t id = id0;
            const uint32_t len = have ? id_len(id, i) : 0u;
            const uint32_t incl = tkd_scan_incl(len), excl = incl - len;
            // documents whose first id is one of this step's 64: mark their lanes (scalar loop, the starts are in order)
            uint64_t starts = 0;
            while (nfirst < c0 + 64) {
                const uint32_t l = (uint32_t)(nfirst - c0);
                starts |= 1ull << l;
                // (a lane past the group's last id has len 0 and the whole step in front of it)
                const uint64_t at = cursor + (uint32_t)__builtin_amdgcn_readlane((int)excl, (int)l);
                if (lane == jn) dpos = at;
                ++jn;
                nfirst = jn < ndg ? tks_readlane64(dfirst, jn) : ~0ull;
            }
            const uint32_t m = tkd_scan_max((starts >> lane) & 1ull ? excl + 1u : 0u);
            const uint64_t dbase = m ? cursor + (m - 1u) : base;
            const uint64_t st = cursor + excl - dbase, en = st + len;
            if (have) {
                if (en > 0xFFFFFFFFull) atomicMin(a.err + 3, (unsigned long long)i);
                typedef uint32_t __attribute__((ext_vector_type(2))) u32x2;
                reinterpret_cast<u32x2*>(a.spans)[i] = u32x2{(uint32_t)st, (uint32_t)en};
                if (CHK == 2 && len && id >= a.num_special) {
                    const uint64_t gpos = tbase + cursor + excl;
                    if (gpos + len > tend || !tks_bytes_equal(a, id - a.num_special, e0, gpos, len)) atomicMin(a.err + 1, (unsigned long long)i);
                }
            }
            base = tks_readlane64(dbase, 63);
            cursor += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            id0 = id1; id1 = id2;
            if (CHK == 2) e0 = e1;
        }
        if (CHK >= 1) {
            // document j covers [its position, the next document's position); the last one ends where the group's text ends
            if (dpos == ~0ull) dpos = cursor;
            const uint32_t nl = (uint32_t)__shfl((int)(uint32_t)dpos, (int)(lane + 1u) & 63);
            const uint32_t nh = (uint32_t)__shfl((int)(uint32_t)(dpos >> 32), (int)(lane + 1u) & 63);
            const uint64_t next = lane + 1u < ndg ? (((uint64_t)nh << 32) | nl) : cursor;
            if (lane < ndg && next - dpos != a.doc_offs[dA + lane + 1] - a.doc_offs[dA + lane]) atomicMin(a.err + 0, (unsigned long long)(dA + lane));
        }
    }
}

hipError_t tk_launch_spans(const TkSpansArgs& a, int checks, hipStream_t s) {
    if (a.n_docs == 0) return hipSuccess;
    const uint64_t n_groups = (a.n_docs + TKS_DOCS - 1) / TKS_DOCS;
    uint64_t blocks = (n_groups + TKS_BLOCK / 64 - 1) / (TKS_BLOCK / 64);
    if (blocks > 256u * 2u) blocks = 256u * 2u;             // every block copies 32 KB into its LDS first: no more than are resident
    if (checks & TK_SPANS_CHECK_BYTES) hipLaunchKernelGGL(tk_spans_kernel<2>, dim3((uint32_t)blocks), dim3(TKS_BLOCK), 0, s, a);
    else if (checks & TK_SPANS_CHECK_COVER) hipLaunchKernelGGL(tk_spans_kernel<1>, dim3((uint32_t)blocks), dim3(TKS_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(tk_spans_kernel<0>, dim3((uint32_t)blocks), dim3(TKS_BLOCK), 0, s, a);
    return hipGetLastError();
}
