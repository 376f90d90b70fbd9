// tk_units_table.h -- the per-rank table of the units pass (include/tekken_hip.h tk_token_spans_units_device; csrc/tk_spans_units.hip;
// DESIGN 4.5g).  Host only, plain C++ with no HIP in it: tests/units_table_check.cpp builds it stand-alone.
//
// By bytes (valid UTF-8 or not): a byte b STARTS a character when (b & 0xC0) != 0x80; it weighs 1 code point, and 1 more UTF-16
// unit when b >= 0xF0.  What the kernel needs of a token is how many units it holds, how many lie in front of its LAST character
// start (where a following token that begins inside a character is widened to), whether it holds a start at all, and whether
// its first byte is one (else its own span is widened backwards).  With n_start starts and n_four bytes >= 0xF0:
//   code points: units = n_start,           in front of the last start = n_start - 1
//   UTF-16:      units = n_start + n_four,  in front of the last start = n_start - 1 + n_four - (the last start is >= 0xF0)
// so one 16-bit entry per rank carries both units:
//   bits 0..7   n_start (TKU_LONG: the token does not fit an entry -- the kernel counts its bytes from tok_blob)
//   bits 8..13  n_four
//   bit 14      the first byte starts a character (set for a token of no bytes too: its span is (U(s), U(s)), like a special id's)
//   bit 15      the last character start is a byte >= 0xF0
#ifndef TK_UNITS_TABLE_H
#define TK_UNITS_TABLE_H
#include <stdint.h>

#define TKU_LONG 0xFFu          /* bits 0..7: count the bytes instead */
#define TKU_FOUR_MAX 63u        /* n_four of an entry */
#define TKU_FIRST (1u << 14)
#define TKU_LAST4 (1u << 15)

struct TkUnitsCount {
    uint32_t n_start, n_four;   // character starts; bytes >= 0xF0
    uint32_t first, last4;      // the first byte is a start (or there is no byte); the last start is >= 0xF0
};

// the counts of one token, byte by byte (what the kernel does for a TKU_LONG entry)
static inline TkUnitsCount tk_units_count(const uint8_t* t, uint32_t len) {
    TkUnitsCount c = {0u, 0u, len == 0u ? 1u : 0u, 0u};
    for (uint32_t k = 0; k < len; ++k) {
        const uint8_t b = t[k];
        if ((b & 0xC0u) != 0x80u) {
            ++c.n_start;
            c.last4 = b >= 0xF0u ? 1u : 0u;
            if (k == 0) c.first = 1u;
        }
        if (b >= 0xF0u) ++c.n_four;
    }
    return c;
}

static inline uint16_t tk_units_entry(const uint8_t* t, uint32_t len) {
    const TkUnitsCount c = tk_units_count(t, len);
    if (c.n_start >= TKU_LONG || c.n_four > TKU_FOUR_MAX) return (uint16_t)TKU_LONG;
    return (uint16_t)(c.n_start | (c.n_four << 8) | (c.first ? TKU_FIRST : 0u) | (c.last4 ? TKU_LAST4 : 0u));
}

// out[0 .. n_ranks): the entries of the tokens blob[offs[r] .. offs[r + 1])
static inline void tk_units_table_build(const uint8_t* blob, const uint32_t* offs, uint32_t n_ranks, uint16_t* out) {
    for (uint32_t r = 0; r < n_ranks; ++r) out[r] = tk_units_entry(blob + offs[r], offs[r + 1] - offs[r]);
}

#endif
