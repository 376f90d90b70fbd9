// tk_utf8_lossy.h -- the scalar step of LOSSY UTF-8 decoding: what bytes.decode("utf-8", "replace"), Rust's
// String::from_utf8_lossy and the WHATWG decoder do ("substitution of maximal subparts", Unicode 3.9 / table 3-7).
//
// Plain C, usable from host and device like tk_utf8_swar.h: the repair kernels and the stream kernels of tk_decode_lossy.hip
// run it per byte, tests/utf8_lossy_check.c drives the very same functions against python's codec.
//
// The rule, scanning a run from the left: an ASCII byte is copied; a byte that cannot begin a sequence (80..BF, C0, C1, F5..FF)
// becomes U+FFFD (EF BF BD); a lead C2..F4 takes the longest prefix of its sequence that is still well formed -- the second byte
// bounded by the lead (E0: A0..BF, ED: 80..9F, F0: 90..BF, F4: 80..8F, otherwise 80..BF), later bytes 80..BF, never past the end of
// the run -- and the scan goes on behind that prefix.  A complete sequence is copied, a truncated prefix of 1..3 bytes becomes ONE
// U+FFFD.  Every input byte therefore contributes 1, 3 or 0 output bytes, and what a byte contributes is decided by the three
// bytes on each side of it: only continuation bytes are ever consumed behind a lead, so every other byte begins a unit, and a
// continuation byte belongs to the nearest non-continuation byte at most three positions in front of it, or to nothing.
#ifndef TK_UTF8_LOSSY_H
#define TK_UTF8_LOSSY_H
#include <stdint.h>

#if defined(__HIPCC__)
#define TK_UL_FN static __host__ __device__ inline
#else
#define TK_UL_FN static inline
#endif

#define TKUL_LEN_MASK 3u      /* tkul_class: bits 0..1, the output bytes of the position: 0, 1 or 3 */
#define TKUL_HOLD 4u          /* tkul_class: the position is part of a truncated prefix that reaches the end of the run */

// What byte b begins: 1 ASCII, 0 nothing (it cannot begin a sequence), 2..4 the length of the sequence of lead b; [*lo, *hi] is
// the range of the SECOND byte of that sequence.
TK_UL_FN uint32_t tkul_lead(uint32_t b, uint32_t* lo, uint32_t* hi) {
    *lo = 0x80u;
    *hi = 0xBFu;
    if (b < 0x80u) return 1u;
    if (b < 0xC2u || b > 0xF4u) return 0u;
    if (b < 0xE0u) return 2u;
    if (b < 0xF0u) {
        if (b == 0xE0u) *lo = 0xA0u;
        if (b == 0xEDu) *hi = 0x9Fu;
        return 3u;
    }
    if (b == 0xF0u) *lo = 0x90u;
    if (b == 0xF4u) *hi = 0x8Fu;
    return 4u;
}

TK_UL_FN int tkul_is_cont(uint32_t b) { return (b & 0xC0u) == 0x80u; }

// The longest well-formed prefix (1..need bytes) of the sequence of a lead with `need` and [lo, hi] from tkul_lead; b1 b2 b3 are
// the bytes behind the lead, `avail` (0..3) of them inside the run.
TK_UL_FN uint32_t tkul_prefix(uint32_t need, uint32_t lo, uint32_t hi, uint32_t b1, uint32_t b2, uint32_t b3, uint32_t avail) {
    if (avail < 1u || b1 < lo || b1 > hi) return 1u;
    if (need < 3u) return 2u;
    if (avail < 2u || !tkul_is_cont(b2)) return 2u;
    if (need < 4u) return 3u;
    if (avail < 3u || !tkul_is_cont(b3)) return 3u;
    return 4u;
}

// One position.  win: the bytes at p - 3 .. p + 3 in byte lanes 0 .. 6 (lane 3 is the position itself); nb / na (0..3 each): how
// many of the bytes in front / behind lie in the same run, 3 meaning "three or more" -- a hard boundary (run start, document
// boundary, end of the text) cuts them, and bytes beyond a boundary are never looked at.  Returns the position's output length
// (TKUL_LEN_MASK) and TKUL_HOLD where the position belongs to a truncated prefix that ends exactly at the run's end: a stream that
// may still receive the rest holds those positions back instead of writing their U+FFFD.
TK_UL_FN uint32_t tkul_class(uint64_t win, uint32_t nb, uint32_t na) {
#define TKUL_B(k) ((uint32_t)((win >> (8u * (k))) & 0xFFu))
    const uint32_t b = TKUL_B(3);
    uint32_t lo, hi;
    if (!tkul_is_cont(b)) {
        const uint32_t need = tkul_lead(b, &lo, &hi);
        if (need == 1u) return 1u;
        if (need == 0u) return 3u;
        const uint32_t m = tkul_prefix(need, lo, hi, TKUL_B(4), TKUL_B(5), TKUL_B(6), na);
        if (m == need) return 1u;
        return 3u | (m == na + 1u ? TKUL_HOLD : 0u);
    }
    for (uint32_t k = 1u; k <= 3u && k <= nb; ++k) {
        const uint32_t c = TKUL_B(3u - k);
        if (tkul_is_cont(c)) continue;
        const uint32_t need = tkul_lead(c, &lo, &hi);
        if (need < 2u) return 3u;
        uint32_t avail = k + na;
        if (avail > 3u) avail = 3u;
        const uint32_t m = tkul_prefix(need, lo, hi, TKUL_B(4u - k), TKUL_B(5u - k), TKUL_B(6u - k), avail);
        if (k >= m) return 3u;                         // the lead's prefix ended in front of this byte: a stray continuation byte
        if (m == need) return 1u;
        return m == k + na + 1u ? TKUL_HOLD : 0u;      // the lead wrote the prefix's one U+FFFD
    }
    return 3u;                                         // no lead within three bytes of the run: a stray continuation byte
#undef TKUL_B
}

// ---- the same rule fed one byte at a time (the stream kernels; long pieces of text belong to tkul_class) ----
// *st is the open prefix in the layout of the stream state: bytes 0..2 the pending bytes, byte 3 their count 0..3, 0 = fresh.
// Writes what byte b makes final to out[0..] (at most 6 bytes) and returns their number, plus 0x100 for every U+FFFD among them.
TK_UL_FN uint32_t tkul_feed(uint32_t* st, uint32_t b, uint8_t* out) {
    uint32_t n = 0u, lo, hi;
    const uint32_t cnt = *st >> 24;
    if (cnt) {
        const uint32_t need = tkul_lead(*st & 0xFFu, &lo, &hi);
        const int ok = need >= 2u && cnt < need && cnt <= 3u && (cnt == 1u ? (b >= lo && b <= hi) : tkul_is_cont(b));
        if (ok) {
            const uint32_t all = (*st & 0x00FFFFFFu) | (cnt < 3u ? b << (8u * cnt) : 0u);
            if (cnt + 1u < need) {
                *st = all | ((cnt + 1u) << 24);
                return 0u;
            }
            for (uint32_t k = 0u; k < cnt; ++k) out[k] = (uint8_t)(all >> (8u * k));
            out[cnt] = (uint8_t)b;
            *st = 0u;
            return need;
        }
        out[0] = 0xEFu; out[1] = 0xBFu; out[2] = 0xBDu;
        n = 0x103u;
        *st = 0u;
    }
    const uint32_t need = tkul_lead(b, &lo, &hi);
    if (need == 1u) {
        out[n & 0xFFu] = (uint8_t)b;
        return n + 1u;
    }
    if (need == 0u) {
        uint8_t* o = out + (n & 0xFFu);
        o[0] = 0xEFu; o[1] = 0xBFu; o[2] = 0xBDu;
        return n + 0x103u;
    }
    *st = b | (1u << 24);
    return n;
}

// A hard boundary or the end of a stream: an open prefix becomes one U+FFFD.  Same return as tkul_feed.
TK_UL_FN uint32_t tkul_flush(uint32_t* st, uint8_t* out) {
    if ((*st >> 24) == 0u) return 0u;
    out[0] = 0xEFu; out[1] = 0xBFu; out[2] = 0xBDu;
    *st = 0u;
    return 0x103u;
}

#endif
