// tk_match.h -- the sequential matchers (overview: tk_encode_impl.h): tk_match_end, and tk_match_end2 for the JSON pattern
#ifndef TK_MATCH_H
#define TK_MATCH_H
#include "tk_lookup.h"

// ------------------------------------------------------------------------------------------
// sequential matcher used only by the long-piece path: end of the match that starts at `pos`
// (a piece start) in the document [.., s1).  Same alternatives, same order as
// src/tekkenizer.rs:123.  Every lane computes the same value.
// ------------------------------------------------------------------------------------------
TK_DEV uint32_t tk_decode_at(const uint8_t* b, uint64_t p, uint64_t n, uint32_t* len) {
    uint32_t b0 = b[p];
    if (b0 < 0x80u) { *len = 1; return b0; }
    if ((b0 & 0xE0u) == 0xC0u && p + 1 < n && (b[p + 1] & 0xC0u) == 0x80u) {
        *len = 2; return ((b0 & 0x1Fu) << 6) | (b[p + 1] & 0x3Fu);
    }
    if ((b0 & 0xF0u) == 0xE0u && p + 2 < n && (b[p + 1] & 0xC0u) == 0x80u && (b[p + 2] & 0xC0u) == 0x80u) {
        *len = 3; return ((b0 & 0x0Fu) << 12) | ((uint32_t)(b[p + 1] & 0x3Fu) << 6) | (b[p + 2] & 0x3Fu);
    }
    if ((b0 & 0xF8u) == 0xF0u && p + 3 < n && (b[p + 1] & 0xC0u) == 0x80u && (b[p + 2] & 0xC0u) == 0x80u &&
        (b[p + 3] & 0xC0u) == 0x80u) {
        *len = 4;
        return ((b0 & 0x07u) << 18) | ((uint32_t)(b[p + 1] & 0x3Fu) << 12) | ((uint32_t)(b[p + 2] & 0x3Fu) << 6) |
               (b[p + 3] & 0x3Fu);
    }
    *len = 1;
    return 0xFFFFFFFFu;
}

TK_DEV uint32_t tk_class_at(const TkTablesView& t, const uint8_t* b, uint64_t p, uint64_t n, uint32_t* len,
                            uint32_t* cp) {
    uint32_t c = tk_decode_at(b, p, n, len);
    *cp = c;
    if (c < 0x80u) return tk_ascii_class(c);
    return tk_uc_class(t, c);
}

TK_DEV uint32_t tk_fold(uint32_t cp) {
    if (cp >= 'A' && cp <= 'Z') return cp + 32u;
    if (cp == 0x17Fu) return 's';
    return cp;
}

// Wave-cooperative fast-forward over a run of ASCII bytes of class `cls`, 64 bytes per step (called by all 64 lanes in
// convergence; every lane gets the same answer): the first position at or after q whose byte is not ASCII of that class
// (or n).  The per-byte loops of the matcher below are sequential dependent loads -- 32 KiB of letters took a wave 6 ms.
TK_DEV uint64_t tk_skip_ascii_run(const uint8_t* b, uint64_t q, uint64_t n, uint32_t cls) {
    const int lane = wv_lane();
    for (;;) {
        const uint64_t p = q + (uint64_t)lane;
        const uint32_t c = p < n ? (uint32_t)b[p] : 0x80u;
        const uint64_t stop = wv_ballot(c >= 0x80u || tk_ascii_class(c) != cls);
        if (stop) return q + (uint64_t)tk_ctz64(stop);
        q += 64;
    }
}

TK_DEV uint64_t tk_match_end(const TkTablesView& t, const uint8_t* b, uint64_t pos, uint64_t n) {
    uint32_t l0, l1, l2, c0, c1, c2;
    uint32_t k0 = tk_class_at(t, b, pos, n, &l0, &c0);
    if (c0 == '\'' && pos + 1 < n) {  // alt 1
        (void)tk_class_at(t, b, pos + 1, n, &l1, &c1);
        uint32_t f1 = tk_fold(c1);
        if (f1 == 's' || f1 == 't' || f1 == 'm' || f1 == 'd') return pos + 1 + l1;
        if ((f1 == 'r' || f1 == 'v' || f1 == 'l') && pos + 1 + l1 < n) {
            (void)tk_class_at(t, b, pos + 1 + l1, n, &l2, &c2);
            uint32_t f2 = tk_fold(c2);
            if (((f1 == 'r' || f1 == 'v') && f2 == 'e') || (f1 == 'l' && f2 == 'l')) return pos + 1 + l1 + l2;
        }
    }
    {  // alt 2
        bool crlf = (c0 == '\r' || c0 == '\n');
        bool with_prefix = !(crlf || k0 == TK_CLS_L || k0 == TK_CLS_N);
        for (int attempt = with_prefix ? 0 : 1; attempt < 2; ++attempt) {
            uint64_t p = attempt == 0 ? pos + l0 : pos;
            uint64_t q = p;
            while (q < n) {
                q = tk_skip_ascii_run(b, q, n, TK_CLS_L);           // ASCII letters 64 at a time, then char by char
                if (q >= n) break;
                uint32_t l, c;
                if (tk_class_at(t, b, q, n, &l, &c) != TK_CLS_L) break;
                q += l;
            }
            if (q > p) return q;
        }
    }
    if (k0 == TK_CLS_N) {  // alt 3
        uint64_t q = pos + l0;
        for (int cnt = 1; cnt < 3 && q < n; ++cnt) {
            uint32_t l, c;
            if (tk_class_at(t, b, q, n, &l, &c) != TK_CLS_N) break;
            q += l;
        }
        return q;
    }
    for (int attempt = (c0 == ' ') ? 0 : 1; attempt < 2; ++attempt) {  // alt 4
        uint64_t p = attempt == 0 ? pos + 1 : pos;
        uint64_t q = p;
        while (q < n) {
            q = tk_skip_ascii_run(b, q, n, TK_CLS_O);
            if (q >= n) break;
            uint32_t l, c;
            if (tk_class_at(t, b, q, n, &l, &c) != TK_CLS_O) break;
            q += l;
        }
        if (q > p) {
            while (q < n && (b[q] == '\r' || b[q] == '\n')) ++q;
            return q;
        }
    }
    // alts 5-7 over the maximal white-space run
    uint64_t e = pos, after_last_nl = 0, last_char = pos;
    bool has_nl = false;
    {
        // whole blocks of 64 ASCII white-space bytes at a time (the last CR / LF of a block from a ballot)
        const int lane = wv_lane();
        while (e + 64 <= n) {
            const uint32_t c = b[e + (uint64_t)lane];
            if (wv_ballot(c >= 0x80u || tk_ascii_class(c) != TK_CLS_S)) break;
            const uint64_t NL = wv_ballot(c == '\r' || c == '\n');
            if (NL) { has_nl = true; after_last_nl = e + (uint64_t)tk_msb64(NL) + 1; }
            last_char = e + 63;
            e += 64;
        }
    }
    while (e < n) {
        uint32_t l, c;
        if (tk_class_at(t, b, e, n, &l, &c) != TK_CLS_S) break;
        last_char = e;
        e += l;
        if (c == '\r' || c == '\n') { has_nl = true; after_last_nl = e; }
    }
    if (has_nl) return after_last_nl;
    if (e == n) return e;
    if (last_char > pos) return last_char;
    return e > pos ? e : pos + l0;
}

// ------------------------------------------------------------------------------------------
// SURVEY section 8 row f-3, opt-in: the `pattern` string that Mistral's tekken.json carries and the reference ignores
// (src/tekkenizer.rs:74; literal in tests/test_small_vocab.rs:62):
//   [^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]*[\p{Ll}\p{Lm}\p{Lo}\p{M}]+ | [^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]+[\p{Ll}\p{Lm}\p{Lo}\p{M}]*
//   | \p{N} | ' '?[^\s\p{L}\p{N}]+[\r\n/]* | \s*[\r\n]+ | \s+(?!\S) | \s+
// as a sequential matcher (leftmost-first alternation, greedy with backtracking), used by the piece-by-piece path of
// pass 2 only: first version of the opt-in, every document takes that path.  Classes from unicode_tables2.h:
// 1 U = Lu|Lt, 2 W = Ll, 3 X = Lm|Lo, 4 M, 5 N, 6 S, 0 anything else.  "Upper side" = U X M, "lower side" = W X M.
// ------------------------------------------------------------------------------------------
TK_DEV uint32_t tk_class2_at(const TkTablesView& t, const uint8_t* b, uint64_t p, uint64_t n, uint32_t* len, uint32_t* cp) {
    const uint32_t c = tk_decode_at(b, p, n, len);
    *cp = c;
    return tk_uc_class2(t, c);
}
TK_DEV bool tk_c2_upper_side(uint32_t k) { return k == 1u || k == 3u || k == 4u; }
TK_DEV bool tk_c2_lower_side(uint32_t k) { return k == 2u || k == 3u || k == 4u; }

// word of the first / second alternative that starts at p (behind the optional prefix); p itself = no match
TK_DEV uint64_t tk_word2_at(const TkTablesView& t, const uint8_t* b, uint64_t p, uint64_t n, bool second_alt) {
    uint64_t q = p, last_both = ~0ull;           // last char of the upper-side run that is also lower-side (X or M)
    while (q < n) {
        uint32_t l, c;
        const uint32_t k = tk_class2_at(t, b, q, n, &l, &c);
        if (!tk_c2_upper_side(k)) break;
        if (tk_c2_lower_side(k)) last_both = q;
        q += l;
    }
    uint64_t from;
    if (second_alt) {                            // [upper side]+ [lower side]*
        if (q == p) return p;
        from = q;
    } else {                                     // [upper side]* [lower side]+ : give chars back until the lower side can start
        from = ~0ull;
        if (q < n) {
            uint32_t l, c;
            if (tk_c2_lower_side(tk_class2_at(t, b, q, n, &l, &c))) from = q;
        }
        if (from == ~0ull) from = last_both;
        if (from == ~0ull) return p;
    }
    uint64_t e = from;
    while (e < n) {
        uint32_t l, c;
        if (!tk_c2_lower_side(tk_class2_at(t, b, e, n, &l, &c))) break;
        e += l;
    }
    return e;
}

TK_DEV uint64_t tk_match_end2(const TkTablesView& t, const uint8_t* b, uint64_t pos, uint64_t n) {
    uint32_t l0, c0;
    const uint32_t k0 = tk_class2_at(t, b, pos, n, &l0, &c0);
    const bool letter = k0 == 1u || k0 == 2u || k0 == 3u;
    const bool prefix_ok = !(c0 == '\r' || c0 == '\n' || letter || k0 == 5u) && pos + l0 < n;
    for (int alt = 0; alt < 2; ++alt) {          // alternatives 1 and 2: with the prefix char first, then without
        if (prefix_ok) {
            const uint64_t e = tk_word2_at(t, b, pos + l0, n, alt == 1);
            if (e > pos + l0) return e;
        }
        const uint64_t e = tk_word2_at(t, b, pos, n, alt == 1);
        if (e > pos) return e;
    }
    if (k0 == 5u) return pos + l0;               // \p{N}: one digit
    for (int attempt = (c0 == ' ') ? 0 : 1; attempt < 2; ++attempt) {   // ' '?[^\s\p{L}\p{N}]+[\r\n/]*  (classes O and M)
        const uint64_t p = attempt == 0 ? pos + 1 : pos;
        uint64_t q = p;
        while (q < n) {
            uint32_t l, c;
            const uint32_t k = tk_class2_at(t, b, q, n, &l, &c);
            if (!(k == 0u || k == 4u)) break;
            q += l;
        }
        if (q > p) {
            while (q < n && (b[q] == '\r' || b[q] == '\n' || b[q] == '/')) ++q;
            return q;
        }
    }
    // the three white-space alternatives, over the maximal white-space run
    uint64_t e = pos, after_last_nl = 0, last_char = pos;
    bool has_nl = false;
    while (e < n) {
        uint32_t l, c;
        if (tk_class2_at(t, b, e, n, &l, &c) != 6u) break;
        last_char = e;
        e += l;
        if (c == '\r' || c == '\n') { has_nl = true; after_last_nl = e; }
    }
    if (e == pos) return pos + l0;               // (not reached for valid UTF-8)
    if (has_nl) return after_last_nl;
    if (e == n) return e;
    if (last_char > pos) return last_char;
    return e;
}

#endif
