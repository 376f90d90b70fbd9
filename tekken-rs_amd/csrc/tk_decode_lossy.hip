// tk_decode_lossy.hip -- gfx950 kernels of LOSSY decode: invalid UTF-8 becomes U+FFFD instead of failing the call.
//
// One definition (tk_utf8_lossy.h: substitution of maximal subparts, what python's errors="replace" and Rust's from_utf8_lossy
// do), two ways of running it:
//
//   The bulk REPAIR pass behind the unchanged strict pipeline (tk_decode.hip).  The emit kernel left the raw text of the batch,
//   its document offsets and the run_bits bitmap in HBM; tk_decode_validate_kernel said that something is malformed.  The raw text
//   is ONE stream cut into tiles of TK_LOSSY_TILE bytes, a block a tile, 16 bytes a thread; document starts and run_bits
//   positions are hard boundaries (a character never spans a special id or a document), and so is the end of the text.  Every
//   input byte gives 1, 3 or 0 output bytes, decided from the three bytes on each side of it and the boundaries among them:
//     tk_decode_lossy_kernel<false>  the output length of every tile
//     (tk_launch_scan)               where every tile's output begins; the host reads the total
//     tk_decode_lossy_kernel<true>   the same classes again, a thread's place in the tile from a wave scan (tk_dpp_scan.h), the
//                                    tile's output assembled in LDS and streamed out with aligned dword stores; the new offset of
//                                    every document that begins in the tile (found with tky_wave_count_le over the old offsets,
//                                    as the seqpack and join kernels find theirs); U+FFFD and dirty documents counted
//   A thread whose 16 bytes are ASCII classifies nothing: the text of a document without a byte >= 0x80 (doc_hi == 0) is copied.
//   Nor does one whose bytes pass the validate kernel's check (tku8_err4 over six dwords): the classes are for the dirty spots.
//
//   The STREAM step for generation: one lane per sequence walks the few new ids of its sequence through tkul_feed, starting from
//   the sequence's state word (the open prefix of up to three bytes); count kernel, scan, write kernel.  Latency work: a step is
//   a handful of ids per sequence, and thousands of sequences.  A long step is correct and slow -- a lane copies byte by byte --:
//   prefill-sized input belongs in the bulk entry.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tk_kernels.h"
#include "tk_layout.h"
#include "tk_utf8_lossy.h"
#include "tk_utf8_swar.h"

#define TKDL_BLOCK 256
#define TKDL_PER 16u                                  /* bytes a thread */
#define TKDL_BIT0 32u                                 /* bit of the LDS bitmap that stands for the tile's first byte */
#define TKDL_BITS_WORDS ((TK_LOSSY_TILE + 64u) / 32u) /* positions g0 - 32 .. g0 + TILE + 31 */
static_assert(TK_LOSSY_TILE == TKDL_BLOCK * TKDL_PER, "a thread takes 16 bytes of the tile");

template <bool WRITE>
__global__ __launch_bounds__(TKDL_BLOCK) void tk_decode_lossy_kernel(TkLossyArgs a) {
    __shared__ uint32_t bits[TKDL_BITS_WORDS];        // hard boundaries around the tile: bit TKDL_BIT0 + r <-> position g0 + r
    __shared__ uint32_t wsum[TKDL_BLOCK / 64];
    __shared__ uint32_t base[WRITE ? TKDL_BLOCK + 1 : 1];          // output bytes of the tile in front of a thread's first byte
    __shared__ uint32_t packed[WRITE ? TKDL_BLOCK : 1];            // the thread's 16 output lengths, two bits each
    __shared__ uint32_t outw[WRITE ? 3u * TK_LOSSY_TILE / 4u : 1]; // the tile's output
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint64_t n_tiles = (a.n_bytes + TK_LOSSY_TILE - 1) / TK_LOSSY_TILE;
    const uint64_t n_offs = a.n_docs + 1;
    uint32_t nrep_all = 0;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t g0 = tile * TK_LOSSY_TILE;
        const uint32_t tile_len = a.n_bytes - g0 < TK_LOSSY_TILE ? (uint32_t)(a.n_bytes - g0) : TK_LOSSY_TILE;
        const bool last = tile + 1 == n_tiles;
        // 1. the run starts of the emit kernel ...
        for (uint32_t k = t; k < TKDL_BITS_WORDS; k += TKDL_BLOCK) {
            const uint64_t widx = (g0 >> 5) + k;                   // (the word of position g0 - 32 + 32 k is widx - 1)
            bits[k] = (widx >= 1u && widx - 1u <= (a.n_bytes >> 5) + 3u) ? a.run_bits[widx - 1u] : 0u;
        }
        // 2. ... and the documents that begin at g0 - 8 .. g0 + TILE + 3 (entry n_docs: the end of the text)
        const uint64_t klo = g0 >= 8u ? g0 - 8u : 0u;
        const uint64_t dA = klo ? tky_wave_count_le(a.offs, n_offs, klo - 1u) : 0u;
        const uint64_t dB = tky_wave_count_le(a.offs, n_offs, g0 + TK_LOSSY_TILE + 3u);
        __syncthreads();
        for (uint64_t d = dA + t; d < dB; d += TKDL_BLOCK) {
            const uint32_t rel = (uint32_t)(a.offs[d] + TKDL_BIT0 - g0);
            atomicOr(&bits[rel >> 5], 1u << (rel & 31u));
        }
        __syncthreads();
        // 3. the classes of the thread's 16 bytes
        const uint32_t r0 = TKDL_PER * t;
        const uint32_t nv = r0 < tile_len ? (tile_len - r0 < TKDL_PER ? tile_len - r0 : TKDL_PER) : 0u;
        uint32_t w[6] = {0u, 0u, 0u, 0u, 0u, 0u};
        uint32_t lens = 0u, sum = 0u, nrep = 0u;
        if (nv) {
            const uint8_t* p = a.bytes + g0 + r0;
            const tky_u32x4 own = *reinterpret_cast<const tky_u32x4*>(p);
            w[1] = own.x; w[2] = own.y; w[3] = own.z; w[4] = own.w;
            if (((own.x | own.y | own.z | own.w) & 0x80808080u) == 0u) {
                // ASCII (bytes behind the text may send a thread the long way, never the other way round): copied as it is
                sum = nv;
                lens = nv == TKDL_PER ? 0x55555555u : (0x55555555u & ((1u << (2u * nv)) - 1u));
            } else {
                w[0] = g0 + r0 >= 4u ? *reinterpret_cast<const uint32_t*>(p - 4) : 0u;
                w[5] = *reinterpret_cast<const uint32_t*>(p + 16);
                const uint32_t wm1 = g0 + r0 >= 8u ? *reinterpret_cast<const uint32_t*>(p - 8) : 0u;
                // bytes at and behind the end of the text read as NUL (tku8_err4 wants that; nothing else looks at them)
                const uint64_t left = a.n_bytes - (g0 + r0);
                if (left < 20u) {
#pragma unroll
                    for (uint32_t m = 0; m < 5u; ++m) {
                        const uint32_t have = left > 4u * m ? (uint32_t)left - 4u * m : 0u;
                        if (have < 4u) w[1u + m] &= (1u << (8u * have)) - 1u;
                    }
                }
                // boundary bits of the positions r0 - 8 .. r0 + 19 (bit i of F: position r0 - 8 + i; of f: r0 - 3 + i)
                const uint32_t bidx = r0 + TKDL_BIT0 - 8u;
                const uint32_t F = (uint32_t)((((uint64_t)bits[(bidx >> 5) + 1u] << 32) | bits[bidx >> 5]) >> (bidx & 31u));
                const uint32_t f = F >> 5;
                // Well-formed text -- nearly all of it -- needs no classes: the validate kernel's four-bytes-a-register check
                // (tk_utf8_swar.h, the same hard boundaries) over the dword in front, the thread's four and the one behind.  A unit
                // that is ill formed and touches the thread's bytes begins at r0 - 3 .. r0 + 15 and is flagged at its first byte or
                // one of the three behind it: at r0 - 3 .. r0 + 18, all of them judged here from the real bytes in front of them.
                uint32_t bad = tku8_err4(wm1, w[0], F) | tku8_err4(w[0], w[1], F >> 4) | tku8_err4(w[1], w[2], F >> 8);
                bad |= tku8_err4(w[2], w[3], F >> 12) | tku8_err4(w[3], w[4], F >> 16) | tku8_err4(w[4], w[5], F >> 20);
                if (bad == 0u) {
                    sum = nv;
                    lens = nv == TKDL_PER ? 0x55555555u : (0x55555555u & ((1u << (2u * nv)) - 1u));
                } else {
#pragma unroll
                for (uint32_t j = 0; j < TKDL_PER; ++j) {
                    if (j < nv) {
                        const uint32_t s = 1u + j;                     // the window: bytes s .. s + 6 of the 24 in w
                        const uint64_t two = ((uint64_t)w[(s >> 2) + 1u] << 32) | w[s >> 2];
                        uint64_t win = two >> (8u * (s & 3u));
                        if ((s & 3u) >= 2u) win |= (uint64_t)w[(s >> 2) + 2u] << (64u - 8u * (s & 3u));
                        const uint32_t b = (uint32_t)(win >> 24) & 0xFFu;
                        uint32_t len = 1u;
                        if (b >= 0x80u) {
                            const uint32_t mb = (f >> j) & 0xFu, ma = (f >> (j + 4u)) & 7u;
                            const uint32_t nb = (mb & 8u) ? 0u : (mb & 4u) ? 1u : (mb & 2u) ? 2u : 3u;
                            const uint32_t na = (ma & 1u) ? 0u : (ma & 2u) ? 1u : (ma & 4u) ? 2u : 3u;
                            len = tkul_class(win, nb, na) & TKUL_LEN_MASK;
                        }
                        lens |= len << (2u * j);
                        sum += len;
                        nrep += len == 3u ? 1u : 0u;
                    }
                }
                }
            }
        }
        // 4. the thread's place in the tile's output
        const uint32_t incl = tkd_scan_incl(sum);
        if (lane == 63u) wsum[wave] = incl;
        __syncthreads();
        uint32_t excl = incl - sum, total = 0u;
        for (uint32_t k = 0; k < TKDL_BLOCK / 64; ++k) {
            if (k < wave) excl += wsum[k];
            total += wsum[k];
        }
        if (!WRITE) {
            if (t == 0u) a.tile_cnt[tile] = total;
            __syncthreads();                                       // (wsum and bits are rewritten by the next tile)
            continue;
        }
        nrep_all += nrep;
        base[t] = excl;
        packed[t] = lens;
        if (t == 0u) base[TKDL_BLOCK] = total;
        uint8_t* out8 = reinterpret_cast<uint8_t*>(outw);
        {
            uint32_t at = excl;
            uint64_t doc_end = 0;                                  // the end of the document whose flag this thread set last
#pragma unroll
            for (uint32_t j = 0; j < TKDL_PER; ++j) {
                const uint32_t len = (lens >> (2u * j)) & 3u;
                if (len == 1u) {
                    out8[at++] = (uint8_t)(w[1u + (j >> 2)] >> (8u * (j & 3u)));
                } else if (len == 3u) {
                    out8[at] = 0xEFu; out8[at + 1u] = 0xBFu; out8[at + 2u] = 0xBDu;
                    at += 3u;
                    const uint64_t pos = g0 + r0 + j;
                    if (pos >= doc_end) {                          // the document of the position: the last one that begins at or before it
                        const uint64_t d = tky_count_le(a.offs, n_offs, pos) - 1u;
                        doc_end = a.offs[d + 1u];
                        if (atomicExch(a.bad_flags + d, 1u) == 0u) atomicAdd(a.stat + 1, 1ull);
                    }
                }
            }
        }
        __syncthreads();
        // 5. the tile's output, streamed out: bytes up to the first aligned dword, dwords (unaligned LDS reads: gfx950 takes them), the rest
        {
            typedef uint32_t __attribute__((aligned(1))) u32_u;
            const uint64_t ob = a.tile_offs[tile];
            uint32_t head = (4u - (uint32_t)(ob & 3u)) & 3u;
            if (head > total) head = total;
            const uint32_t nw = (total - head) / 4u, tail0 = head + 4u * nw;
            if (t < head) a.out_bytes[ob + t] = out8[t];
            for (uint32_t k = t; k < nw; k += TKDL_BLOCK)
                *reinterpret_cast<uint32_t*>(a.out_bytes + ob + head + 4u * k) = *reinterpret_cast<const u32_u*>(out8 + head + 4u * k);
            if (t < total - tail0) a.out_bytes[ob + tail0 + t] = out8[tail0 + t];
            // 6. the documents that begin in the tile (the last tile: at the end of the text too -- empty documents, entry n_docs)
            for (uint64_t d = dA + t; d < dB; d += TKDL_BLOCK) {
                const uint64_t o = a.offs[d];
                if (o < g0 || !(o < g0 + tile_len || (last && o == a.n_bytes))) continue;
                const uint32_t r = (uint32_t)(o - g0), tt = r >> 4, jj = r & 15u;
                uint32_t pre = base[tt];
                if (jj) {
                    const uint32_t x = packed[tt] & ((1u << (2u * jj)) - 1u);
                    pre += (uint32_t)__popc(x & 0x55555555u) + 2u * (uint32_t)__popc(x & 0xAAAAAAAAu);
                }
                a.out_offs[d] = ob + pre;
            }
        }
        __syncthreads();
    }
    if (WRITE) tky_wave_add(a.stat + 0, nrep_all);
}

static uint32_t tkdl_grid(uint64_t n_bytes) {
    const uint64_t n_tiles = (n_bytes + TK_LOSSY_TILE - 1) / TK_LOSSY_TILE;
    return (uint32_t)(n_tiles < TK_LOSSY_MAX_BLOCKS ? n_tiles : TK_LOSSY_MAX_BLOCKS);
}

hipError_t tk_launch_decode_lossy_counts(const TkLossyArgs& a, hipStream_t s) {
    if (a.n_bytes == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_decode_lossy_kernel<false>, dim3(tkdl_grid(a.n_bytes)), dim3(TKDL_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_decode_lossy_write(const TkLossyArgs& a, hipStream_t s) {
    if (a.n_bytes == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_decode_lossy_kernel<true>, dim3(tkdl_grid(a.n_bytes)), dim3(TKDL_BLOCK), 0, s, a);
    return hipGetLastError();
}

// ---- the stream step: one lane per sequence ----
// The sequence's text is `pending ++ bytes of its new ids` under the grouping of decode: a special id (a dropped one too) closes
// the run in front of it -- an open prefix becomes one U+FFFD, in front of the special's own string under KEEP --, and what is
// still open behind the last id stays in the state word, unless the step is final.
#define TKDS_BLOCK 64
template <bool WRITE>
__global__ __launch_bounds__(TKDS_BLOCK) void tk_decode_stream_kernel(TkStreamArgs a) {
    const uint64_t stride = (uint64_t)gridDim.x * TKDS_BLOCK;
    uint32_t nrep = 0u;
    for (uint64_t q = (uint64_t)blockIdx.x * TKDS_BLOCK + threadIdx.x; q < a.n_seqs; q += stride) {
        uint8_t* out = WRITE ? a.out_bytes + a.out_offs[q] : nullptr;
        uint32_t n = 0u, st = 0u;
        uint8_t tmp[8];
        auto emit = [&](uint32_t r) {
            const uint32_t k = r & 0xFFu;
            if (WRITE)
                for (uint32_t i = 0; i < k; ++i) out[n + i] = tmp[i];
            n += k;
            nrep += r >> 8;
        };
        // the pending bytes go through the same door as new ones: a well-formed state passes through, any other word is text
        const uint32_t old = a.state[q];
        const uint32_t cnt = (old >> 24) < 3u ? (old >> 24) : 3u;
        for (uint32_t k = 0; k < cnt; ++k) emit(tkul_feed(&st, (old >> (8u * k)) & 0xFFu, tmp));
        const uint64_t i0 = a.id_offs[q], i1 = a.id_offs[q + 1];
        for (uint64_t i = i0; i < i1; ++i) {
            const uint32_t id = a.ids[i];
            const uint8_t* src;
            uint32_t len;
            const bool special = id < a.num_special;
            if (special) {
                if (a.policy == TK_POLICY_RAISE) {
                    if (!WRITE) atomicMin(a.err + 0, (unsigned long long)i);
                    continue;
                }
                emit(tkul_flush(&st, tmp));
                if (a.policy != TK_POLICY_KEEP) continue;
                src = a.sp_blob + a.sp_offs[id];
                len = a.sp_offs[id + 1] - a.sp_offs[id];
                if (WRITE)
                    for (uint32_t k = 0; k < len; ++k) out[n + k] = src[k];
                n += len;
                continue;
            }
            const uint32_t r = id - a.num_special;
            if (r >= a.n_ranks) {
                if (!WRITE) atomicMin(a.err + 1, (unsigned long long)i);
                continue;
            }
            src = a.tok_blob + a.tok_offs[r];
            len = a.tok_offs[r + 1] - a.tok_offs[r];
            for (uint32_t k = 0; k < len; ++k) emit(tkul_feed(&st, src[k], tmp));
        }
        if (a.flags & TK_STREAM_FINAL) emit(tkul_flush(&st, tmp));
        if (WRITE) a.state[q] = st;
        else a.lens[q] = n;
    }
    if (WRITE) tky_wave_add(a.stat + 0, nrep);
}

static uint32_t tkds_grid(uint64_t n_seqs) {
    const uint64_t b = (n_seqs + TKDS_BLOCK - 1) / TKDS_BLOCK;
    return (uint32_t)(b < 4096u ? b : 4096u);
}

hipError_t tk_launch_decode_stream_count(const TkStreamArgs& a, hipStream_t s) {
    if (a.n_seqs == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_decode_stream_kernel<false>, dim3(tkds_grid(a.n_seqs)), dim3(TKDS_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t tk_launch_decode_stream_write(const TkStreamArgs& a, hipStream_t s) {
    if (a.n_seqs == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_decode_stream_kernel<true>, dim3(tkds_grid(a.n_seqs)), dim3(TKDS_BLOCK), 0, s, a);
    return hipGetLastError();
}
