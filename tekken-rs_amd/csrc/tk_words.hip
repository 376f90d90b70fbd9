// tk_words.hip -- gfx950 kernels of the word ids (include/tekken_hip.h tk_words_from_ids_device): which
// pre-tokenization piece every id came from (HF tokenizers' word_ids()).
//
// No reference equivalent: the reference splits inside CoreBPE::encode (src/tekkenizer.rs:384-386) and keeps no trace of it.
// Inputs: the ids with their offsets, the document offsets of the text, and one FLAG byte per text byte (1: a piece starts
// here), made on the device by the split-only launch of the encode kernel (hard-coded pattern) or by tk_words_split_json_kernel
// below (JSON pattern).  An id BEGINS a word when its span is not empty, starts inside its document and starts on a flag; the
// word of an id is the number of ids of its document that begin at or before it, less one.
//
// A sibling of tk_spans_kernel (tk_spans.hip) with its launch shape: one wave per group of TK_DECODE_GROUP_DOCS consecutive
// documents, their ids as ONE stream, 64 ids a step, the ids requested two steps ahead, the one-byte length table's first 32 K
// ranks in LDS.  Per step:
//   * the DPP prefix sum of the lengths places every id in the group's text (as the spans kernel);
//   * a DPP prefix MAXIMUM over the marked document starts gives where an id's document began, a second one the document's
//     slot j in the group (with the begins counted in front of it, below).  Lanes j < 16 hold doc_offs[dA + j] and the length of
//     document j: a lane fetches its own document's by a cross-lane read;
//   * the text position is doc_offs[d] + start (NOT the group-text position): for ids that are not the text's own the
//     definition stays exact and the one gathered flag byte is inside the document (start < doc_len is tested first);
//   * a second prefix sum, over begins, gives the word; the count in front of the document's first id comes out of the same
//     prefix maximum as the slot ((slot + 1) << 8 | (excl + 1) at the marked lanes is non-decreasing); the running total
//     and the last document's base are carried across steps;
//   * one 4-byte store per lane.  Lane j keeps the count in front of document j: n_words at the group's end.
// WHAT = 1 is the same walk for word_first: doc_words in lanes j < 16, one scattered 4-byte store per id that begins a word.
// Whether an id begins cannot be read back from word_ids alone (a special id in mid-document hides the id before it at any
// distance), and a begins array would cost a write and a read per id of EVERY call to save this walk's five bytes per id in
// the calls that ask for word_first.
//
// TK_WORDS_CHECK_ALIGNED (CHK = 1): at the group's end lane j compares the text its ids cover with the document's length;
// every non-special id looks for a flag STRICTLY inside its span (aligned dwords for spans of up to 16 bytes, byte by byte
// beyond).  Error words (atomicMin):
//   err[0] first document whose ids do not cover it exactly     err[1] first id index with a piece start inside its span
//   err[2] first id index outside the vocabulary                err[3] first id index whose span ends at or beyond 2^32
//   err[4] first document of 2^32 bytes or more
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tk_dpp_scan.h"
#include "tk_kernels.h"
#include "tk_wave_hip.h"
#include "tk_match.h"

#define TKW_BLOCK 1024        /* as TKS_BLOCK: 16 waves share one LDS copy of the length table */
#define TKW_DOCS TK_DECODE_GROUP_DOCS
#define TKW_L8_LDS 32768u

__device__ __forceinline__ uint64_t tkw_readlane64(uint64_t v, uint32_t l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t tkw_shfl64(uint64_t v, uint32_t l) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)l);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)l);
    return ((uint64_t)hi << 32) | lo;
}

// is a flag set in flags[lo .. hi)?  (hi - lo <= 15: the aligned dwords that hold the range -- the flag buffer is the pass's own,
// 256-byte aligned with 64 bytes behind the text --, shifted into place with v_alignbyte; longer ranges byte by byte)
__device__ __forceinline__ bool tkw_any_flag(const uint8_t* flags, uint64_t lo, uint64_t hi) {
    const uint32_t n = (uint32_t)(hi - lo);
    if (n > 15u) {
        uint32_t any = 0;
        for (uint64_t q = lo; q < hi; ++q) any |= flags[q];
        return any != 0;
    }
    const uintptr_t at = reinterpret_cast<uintptr_t>(flags + lo);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(at & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(at & 3u);
    uint32_t w[5];
#pragma unroll
    for (uint32_t k = 0; k < 5u; ++k) w[k] = 4u * k < sh + n ? q[k] : 0u;
    uint32_t any = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t t = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh);
        const uint32_t have = n > 4u * k ? n - 4u * k : 0u;
        any |= t & (have >= 4u ? 0xFFFFFFFFu : (1u << (8u * have)) - 1u);
    }
    return any != 0;
}

// WHAT: 0 word_ids and the per-document counts, 1 word_first (behind the scan of the counts).  CHK: 1 + TK_WORDS_CHECK_ALIGNED
template <int WHAT, int CHK>
__global__ __launch_bounds__(TKW_BLOCK, 8) void tk_words_kernel(TkWordsArgs a) {
    __shared__ uint32_t l8w[TKW_L8_LDS / 4];
    const uint32_t n_lds = a.n_ranks < TKW_L8_LDS ? a.n_ranks : TKW_L8_LDS;
    for (uint32_t q = threadIdx.x; q < (n_lds + 3u) / 4u; q += TKW_BLOCK) l8w[q] = reinterpret_cast<const uint32_t*>(a.tok_len8)[q];
    __syncthreads();
    const uint8_t* l8 = reinterpret_cast<const uint8_t*>(l8w);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * (TKW_BLOCK / 64) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (TKW_BLOCK / 64);
    const uint64_t n_groups = (a.n_docs + TKW_DOCS - 1) / TKW_DOCS;
    auto id_len = [&](uint32_t id, uint64_t i) -> uint32_t {
        if (id < a.num_special) return 0u;
        const uint32_t r = id - a.num_special;
        if (r >= a.n_ranks) {
            if (WHAT == 0) atomicMin(a.err + 2, (unsigned long long)i);
            return 0u;
        }
        uint32_t len = r < TKW_L8_LDS ? (uint32_t)l8[r] : (uint32_t)a.tok_len8[r];
        if (len == 0xFFu) len = a.tok_offs[r + 1] - a.tok_offs[r];
        return len;
    };
    for (uint64_t g = wave; g < n_groups; g += n_waves) {
        const uint64_t dA = g * TKW_DOCS, dB = dA + TKW_DOCS < a.n_docs ? dA + TKW_DOCS : a.n_docs;
        const uint32_t ndg = (uint32_t)(dB - dA);
        const uint64_t i0 = a.id_offs[dA], i1 = a.id_offs[dB];
        // lane j < ndg: document dA + j -- its first id, where its text begins, its length (clamped: a document of 2^32 bytes or
        // more fails the call), and WHAT = 1: where its words begin in word_first
        const uint64_t dfirst = lane < ndg ? a.id_offs[dA + lane] : ~0ull;
        const uint64_t dtext = lane < ndg ? a.doc_offs[dA + lane] : 0ull;
        uint32_t dlen = 0;
        if (lane < ndg) {
            const uint64_t l = a.doc_offs[dA + lane + 1] - dtext;
            if (l > 0xFFFFFFFFull && WHAT == 0) atomicMin(a.err + 4, (unsigned long long)(dA + lane));
            dlen = l > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)l;
        }
        const uint64_t dwords = WHAT == 1 && lane < ndg ? a.doc_words[dA + lane] : 0ull;
        uint32_t dcount = 0;                               // begins in front of document j's first id (set once it is placed)
        uint64_t dpos = 0;                                 // CHK: where document j's text begins in the group's text
        bool placed = false;
        uint32_t jn = 0;                                   // the next document whose first id has not been placed (wave-uniform)
        uint64_t nfirst = tkw_readlane64(dfirst, 0);
        uint64_t cursor = 0;                               // where the step's first id begins in the group's text
        uint64_t base = 0;                                 // where the document of the step before's last id begins
        uint32_t total = 0;                                // begins in front of the step's first id (mod 2^32: only differences are used)
        uint32_t wbase = 0;                                // ... in front of the first id of the document of the step before's last id
        uint32_t slot = 0;                                 // that document's slot
        uint32_t id0 = i0 + lane < i1 ? a.ids[i0 + lane] : 0u;
        uint32_t id1 = i0 + 64 + lane < i1 ? a.ids[i0 + 64 + lane] : 0u;
        for (uint64_t c0 = i0; c0 < i1; c0 += 64) {
            const uint64_t i = c0 + lane;
            const bool have = i < i1;
            const uint32_t id2 = i + 128 < i1 ? a.ids[i + 128] : 0u;    // two steps ahead
            const uint32_t id = id0;
            const uint32_t len = have ? id_len(id, i) : 0u;
            const uint32_t incl = tkd_scan_incl(len), excl = incl - len;
            // documents whose first id is one of this step's 64: mark their lanes with the slot (scalar loop, the starts are in
            // order; of several documents that start at one id the last one owns it, the others are empty)
            uint32_t mark = 0;
            while (nfirst < c0 + 64) {
                if (lane == (uint32_t)(nfirst - c0)) mark = jn + 1u;
                ++jn;
                nfirst = jn < ndg ? tkw_readlane64(dfirst, jn) : ~0ull;
            }
            const uint32_t m = tkd_scan_max(mark ? excl + 1u : 0u);
            const uint64_t dbase = m ? cursor + (m - 1u) : base;
            const uint64_t st = cursor + excl - dbase, en = st + len;
            // the slot of the id's document, and -- once begins is known -- the count in front of that document
            const uint32_t sm = tkd_scan_max(mark << 8);
            const uint32_t j = sm ? (sm >> 8) - 1u : slot;
            const uint64_t tpos = tkw_shfl64(dtext, j) + st;
            const uint32_t tlen = (uint32_t)__shfl((int)dlen, (int)j);
            const bool body = have && len != 0u && st < (uint64_t)tlen;   // (st < doc_len BEFORE the flag is read)
            const uint32_t b = body && a.flags[tpos] != 0 ? 1u : 0u;
            const uint32_t bincl = tkd_scan_incl(b), bexcl = bincl - b;
            const uint32_t wm = tkd_scan_max(mark ? (mark << 8) | (bexcl + 1u) : 0u);
            const uint32_t wb = wm ? total + ((wm & 0xFFu) - 1u) : wbase;
            const uint32_t word = total + bincl - wb - 1u;               // (no begins yet in the document: wraps to TK_WORD_NONE)
            // lane jj whose document was placed in this step: the count (and the text position) at its first id
            placed = placed || (lane < ndg && dfirst < c0 + 64);
            {
                const uint32_t l = (uint32_t)(dfirst - c0) & 63u;
                const uint32_t be = (uint32_t)__shfl((int)bexcl, (int)l);
                const uint32_t ex = CHK ? (uint32_t)__shfl((int)excl, (int)l) : 0u;
                if (lane < ndg && dfirst >= c0 && dfirst < c0 + 64) {
                    dcount = total + be;
                    if (CHK) dpos = cursor + ex;
                }
            }
            // (cross-lane reads stay outside the divergent stores)
            const uint64_t wdst = WHAT == 1 ? tkw_shfl64(dwords, j) : 0ull;
            const uint32_t ifirst = WHAT == 1 ? (uint32_t)__shfl((int)(uint32_t)dfirst, (int)j) : 0u;
            if (have) {
                if (WHAT == 0) {
                    if (en > 0xFFFFFFFFull) atomicMin(a.err + 3, (unsigned long long)i);
                    a.word_ids[i] = len ? word : 0xFFFFFFFFu;
                    if (CHK && len > 1u && st + 1u < (uint64_t)tlen) {
                        const uint64_t hi = en < (uint64_t)tlen ? en : (uint64_t)tlen;
                        if (tkw_any_flag(a.flags, tpos + 1u, tpos + (hi - st))) atomicMin(a.err + 1, (unsigned long long)i);
                    }
                } else if (b) {
                    a.word_first[wdst + word] = (uint32_t)i - ifirst;
                }
            }
            base = tkw_readlane64(dbase, 63);
            cursor += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            wbase = (uint32_t)__builtin_amdgcn_readlane((int)wb, 63);
            total += (uint32_t)__builtin_amdgcn_readlane((int)bincl, 63);
            slot = (uint32_t)__builtin_amdgcn_readlane((int)j, 63);
            id0 = id1; id1 = id2;
        }
        if (WHAT == 0) {
            // document j has the begins between its first id and the next document's (an empty document at the group's very end
            // was never placed: it begins where the group ends)
            if (!placed) { dcount = total; dpos = cursor; }
            const uint32_t nc = (uint32_t)__shfl((int)dcount, (int)(lane + 1u) & 63);
            const uint32_t next = lane + 1u < ndg ? nc : total;
            if (lane < ndg) a.n_words[dA + lane] = next - dcount;
            if (CHK) {
                const uint64_t np = tkw_shfl64(dpos, (lane + 1u) & 63u);
                const uint64_t nextp = lane + 1u < ndg ? np : cursor;
                if (lane < ndg && nextp - dpos != a.doc_offs[dA + lane + 1] - dtext) atomicMin(a.err + 0, (unsigned long long)(dA + lane));
            }
        }
    }
}

// The piece starts under the JSON pattern (the context after tk_ctx_set_pattern(ctx, 1)): one wave per document, piece by
// piece with the sequential matcher that pass 2 of the encode pipeline runs in that mode (tk_match_end2, tk_match.h) --
// the split-only instantiation of the encode kernel knows the hard-coded pattern alone.  flags is zeroed by the caller.
__global__ __launch_bounds__(256) void tk_words_split_json_kernel(TkTablesView t, const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ doc_offs,
                                                                  uint64_t n_docs, uint8_t* __restrict__ flags) {
    const int lane = wv_lane();
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4;
    for (uint64_t d = wave; d < n_docs; d += n_waves) {
        const uint64_t s0 = wv_first64(doc_offs[d]), s1 = wv_first64(doc_offs[d + 1]);
        uint64_t w0 = s0;
        while (w0 < s1) {
            if (lane == 0) flags[w0] = 1;
            w0 = wv_first64(tk_match_end2(t, bytes, w0, s1));
        }
    }
}

// The split-only launch of the encode kernel decides 64-byte windows at once and gives a continuation byte without a lead the
// class of the byte in front of it; the sequential matcher (and the oracle) take every byte that is not part of a well-formed
// sequence as a character of its own.  On well-formed text the two agree; a document with a malformed byte is split again
// here, piece by piece (every byte of it is written once).  One wave per document: 64 bytes a step, the neighbours of a byte
// are looked at only where the step holds a byte >= 0x80.
__global__ __launch_bounds__(256) void tk_words_resplit_kernel(TkTablesView t, const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ doc_offs,
                                                               uint64_t n_docs, uint8_t* __restrict__ flags) {
    const int lane = wv_lane();
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4;
    for (uint64_t d = wave; d < n_docs; d += n_waves) {
        const uint64_t s0 = wv_first64(doc_offs[d]), s1 = wv_first64(doc_offs[d + 1]);
        bool bad = false;
        for (uint64_t q = s0; q < s1 && !bad; q += 64) {
            const uint64_t p = q + (uint64_t)lane;
            const uint32_t c = p < s1 ? (uint32_t)bytes[p] : 0u;
            if (wv_ballot(c >= 0x80u) == 0) continue;
            bool mal = false;
            if (c >= 0xC0u) {           // a lead: its continuation bytes are there, inside the document
                const uint32_t n = c < 0xE0u ? 2u : c < 0xF0u ? 3u : c < 0xF8u ? 4u : 0u;
                mal = n == 0u || p + n > s1;
                for (uint32_t k = 1; !mal && k < n; ++k) mal = (bytes[p + k] & 0xC0u) != 0x80u;
            } else if (c >= 0x80u) {    // a continuation byte: the nearest byte in front that is none is a lead that reaches it
                mal = true;
                for (uint32_t k = 1; k <= 3u && p >= s0 + k; ++k) {
                    const uint32_t l = bytes[p - k];
                    if ((l & 0xC0u) == 0x80u) continue;
                    const uint32_t n = l < 0xC0u ? 1u : l < 0xE0u ? 2u : l < 0xF0u ? 3u : l < 0xF8u ? 4u : 0u;
                    mal = n <= k;
                    break;
                }
            }
            bad = wv_ballot(mal) != 0;
        }
        if (!bad) continue;
        uint64_t w0 = s0;
        while (w0 < s1) {
            const uint64_t e = wv_first64(tk_match_end(t, bytes, w0, s1));
            for (uint64_t q = w0 + (uint64_t)lane; q < e; q += 64) flags[q] = (q == w0);
            w0 = e;
        }
    }
}

hipError_t tk_launch_words_resplit(const TkTablesView& t, const uint8_t* bytes, const uint64_t* doc_offs, uint64_t n_docs, uint8_t* flags,
                                   hipStream_t s) {
    if (n_docs == 0) return hipSuccess;
    uint64_t blocks = (n_docs + 3) / 4;
    if (blocks > 8192u) blocks = 8192u;
    hipLaunchKernelGGL(tk_words_resplit_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, t, bytes, doc_offs, n_docs, flags);
    return hipGetLastError();
}

hipError_t tk_launch_words_split_json(const TkTablesView& t, const uint8_t* bytes, const uint64_t* doc_offs, uint64_t n_docs, uint8_t* flags,
                                      hipStream_t s) {
    if (n_docs == 0) return hipSuccess;
    uint64_t blocks = (n_docs + 3) / 4;
    if (blocks > 8192u) blocks = 8192u;
    hipLaunchKernelGGL(tk_words_split_json_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, t, bytes, doc_offs, n_docs, flags);
    return hipGetLastError();
}

static uint32_t tkw_blocks(uint64_t n_docs) {
    const uint64_t n_groups = (n_docs + TKW_DOCS - 1) / TKW_DOCS;
    const uint64_t blocks = (n_groups + TKW_BLOCK / 64 - 1) / (TKW_BLOCK / 64);
    return (uint32_t)(blocks > 256u * 2u ? 256u * 2u : blocks);   // every block copies 32 KB into its LDS first: no more than are resident
}

hipError_t tk_launch_words(const TkWordsArgs& a, int check_aligned, hipStream_t s) {
    if (a.n_docs == 0) return hipSuccess;
    if (check_aligned) hipLaunchKernelGGL((tk_words_kernel<0, 1>), dim3(tkw_blocks(a.n_docs)), dim3(TKW_BLOCK), 0, s, a);
    else hipLaunchKernelGGL((tk_words_kernel<0, 0>), dim3(tkw_blocks(a.n_docs)), dim3(TKW_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_words_first(const TkWordsArgs& a, hipStream_t s) {
    if (a.n_docs == 0) return hipSuccess;
    hipLaunchKernelGGL((tk_words_kernel<1, 0>), dim3(tkw_blocks(a.n_docs)), dim3(TKW_BLOCK), 0, s, a);
    return hipGetLastError();
}
