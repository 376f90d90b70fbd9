// tk_lookup.h -- what every kernel of the encode path shares: class constants, bit helpers, code-point classes, the table probes (KEY8 /
// KEY16, LONG, KEY64, PAIR), wave reductions.  All the flat and merge kernels need of the per-document source (overview: tk_encode_impl.h).
#ifndef TK_LOOKUP_H
#define TK_LOOKUP_H
#include <stdint.h>

#include "tk_hash.h"
#include "tk_tables.h"

#define TK_CLS_O 0u
#define TK_CLS_L 1u
#define TK_CLS_N 2u
#define TK_CLS_S 3u
#define TK_DEAD 0xFFFFFFFFu
#define TK_NONE 0xFFFFFFFFu

struct TkPolyPow {  // per-lane powers of the two polynomial bases
    uint32_t pw1, ipw1, pw2, ipw2;
};

// ------------------------------------------------------------------------------------------
// small helpers
// ------------------------------------------------------------------------------------------
TK_DEV uint64_t tk_lowmask(int n) { return n >= 64 ? ~0ull : ((1ull << n) - 1ull); }
TK_DEV int tk_ctz64(uint64_t x) { return x ? __builtin_ctzll(x) : 64; }
TK_DEV int tk_msb64(uint64_t x) { return x ? 63 - __builtin_clzll(x) : 0; }
TK_DEV bool tk_bit(uint64_t m, int i) { return (m >> i) & 1ull; }
TK_DEV int tk_popc64(uint64_t x) { return __builtin_popcountll(x); }

TK_DEV uint32_t tk_ascii_class(uint32_t b) {
    if (((b | 0x20u) - 0x61u) < 26u) return TK_CLS_L;
    if ((b - 0x30u) < 10u) return TK_CLS_N;
    if ((b - 9u) < 5u || b == 0x20u) return TK_CLS_S;
    return TK_CLS_O;
}

TK_DEV uint32_t tk_uc_class(const TkTablesView& t, uint32_t cp) {
    if (cp >= 0x110000u) return TK_CLS_O;
    uint32_t blk = t.uc_stage1[cp >> 7];
    uint32_t w = t.uc_stage2[blk * 8u + ((cp & 127u) >> 4)];
    return (w >> (2u * (cp & 15u))) & 3u;
}
// the classes of the JSON pattern (tk_match.h: tk_match_end2; the flat walk asks too): 1 U, 2 W, 3 X, 4 M, 5 N, 6 S, 0 other
TK_DEV uint32_t tk_uc_class2(const TkTablesView& t, uint32_t cp) {
    if (cp >= 0x110000u) return 0u;
    const uint32_t blk = t.uc2_stage1[cp >> 7];
    const uint32_t w = t.uc2_stage2[blk * 16u + ((cp & 127u) >> 3)];
    return (w >> (4u * (cp & 7u))) & 15u;
}

// One probe = ONE round trip: both candidate entries (cuckoo, tk_hash.h) are fetched together with 16-byte loads
// and compared with bitwise ops; there is no probe loop.
struct alignas(16) tk_u32x4 { uint32_t x, y, z, w; };
struct alignas(8) tk_u32x2 { uint32_t x, y; };

// Whole-piece lookup.  Pieces of up to 8 bytes -- most of the text -- take ONE 16-byte load (key, rank and length in one
// entry of KEY8); pieces of 9..16 bytes a 16-byte + an 8-byte load from KEY16, whose first 16 bytes have the KEY8 layout:
// a short piece has k2 = k3 = 0 and loads nothing for them, so ONE compare sequence without selects serves both.  The
// second cuckoo location is fetched only by the lanes whose first one did not match AND is flagged (first choices are
// filled first by the builder; an unflagged slot that does not match is a definite miss).
// One location: rank or TK_RANK_MAX; *lw = the slot's length word (TK_KEY_SPILL = something spilled from here).
TK_DEV uint32_t tk_key_slot(const uint8_t* p, bool s8, uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3, uint32_t len, uint32_t* lw) {
    tk_u32x4 a = *reinterpret_cast<const tk_u32x4*>(p);           // {k0, k1, rank, len | flag}
    tk_u32x2 b;
    b.x = 0u; b.y = 0u;
    if (!s8) b = *reinterpret_cast<const tk_u32x2*>(p + 16);      // KEY16: {k2, k3}
    WV_PIN(a.x); WV_PIN(a.y); WV_PIN(a.z); WV_PIN(a.w); WV_PIN(b.x); WV_PIN(b.y);   // both loads before the first compare
    const uint32_t d = (a.x ^ k0) | (a.y ^ k1) | ((a.w & ~TK_KEY_SPILL) ^ len) | (b.x ^ k2) | (b.y ^ k3);
    *lw = a.w;
    return d == 0u ? a.z : TK_RANK_MAX;                           // an empty entry has len 0
}
// h = tk_key_hash of the key; KEY8 / KEY16 lanes issue their loads TOGETHER and wait once
TK_DEV uint32_t tk_probe_key_h(const uint8_t* key8_tab, uint32_t key8_mask, const uint8_t* key16_tab, uint32_t key16_mask, uint32_t h,
                               uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3, uint32_t len) {
    const bool s8 = len <= 8u;
    const uint8_t* base = s8 ? key8_tab : key16_tab;
    const uint32_t o1 = s8 ? (h & key8_mask) << 4 : (h & key16_mask) << 5;
    uint32_t lw;
    uint32_t r = tk_key_slot(base + o1, s8, k0, k1, k2, k3, len, &lw);
    if (r == TK_RANK_MAX && (lw & TK_KEY_SPILL)) {
        const uint32_t h2 = tk_hash_alt(h);
        const uint32_t o2 = s8 ? (h2 & key8_mask) << 4 : (h2 & key16_mask) << 5;
        r = tk_key_slot(base + o2, s8, k0, k1, k2, k3, len, &lw);
    }
    return r;
}
TK_DEV uint32_t tk_probe_key(const TkTablesView& t, uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3, uint32_t len) {
    return tk_probe_key_h(reinterpret_cast<const uint8_t*>(t.key8_tab), t.key8_mask, reinterpret_cast<const uint8_t*>(t.key_tab), t.key_mask,
                          tk_key_hash(t.key_hash_mode, k0, k1, k2, k3, len), k0, k1, k2, k3, len);
}

// text points at the piece bytes in the packed buffer; a tag match is verified byte by byte so
// that the result is exact, not probabilistic.
TK_DEV uint32_t tk_probe_long(const TkTablesView& t, uint32_t h1, uint32_t h2, uint32_t len, const uint8_t* text) {
    uint32_t s = tk_long_hash(h1, len) & t.long_mask;
    for (uint32_t tries = 0; tries <= t.long_mask; ++tries) {
        const tk_u32x4 e = *reinterpret_cast<const tk_u32x4*>(t.long_tab + s);  // {tag, rank, len, blob_off}
        if (e.z == 0u) return TK_RANK_MAX;
        if (((e.z ^ len) | (e.x ^ h2)) == 0u) {
            const uint8_t* q = t.blob + e.w;
            uint32_t diff = 0;
            for (uint32_t k = 0; k < len; ++k) diff |= (uint32_t)(q[k] ^ text[k]);  // no early exit: loads pipeline
            if (diff == 0u) return e.y;
        }
        s = (s + 1u) & t.long_mask;
    }
    return TK_RANK_MAX;
}

// KEY64 (tk_hash.h): the whole-piece look-up of a piece of 17..64 bytes by ONE LANE, the piece's bytes as dwords -- tw = the
// aligned word of the text copy that holds its first byte, sh = that byte's offset in it (the words behind the piece are
// readable).  One multiply per dword, the verification against the blob by dwords too.
TK_DEV uint32_t tk_load_u32_unaligned(const uint8_t* p) {
    typedef uint32_t __attribute__((aligned(1))) u32_u;
    return *reinterpret_cast<const u32_u*>(p);
}
TK_DEV uint32_t tk_probe_key64(const TkTablesView& t, const uint32_t* tw, uint32_t sh, uint32_t len, uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3) {
    // k0..k3: the piece's first 16 bytes (the caller has them in registers: the exact-key probe of the shorter pieces takes them too)
    const uint32_t nd = (len + 3u) >> 2;                    // 5..16
    const uint32_t tail = (len & 3u) ? ((1u << (8u * (len & 3u))) - 1u) : 0xFFFFFFFFu;
    uint32_t ha = tk_k64_start(k0, k1, k2, k3);
    {
        uint32_t lo = tw[4];
        for (uint32_t j = 4; j < nd; ++j) {
            const uint32_t hi = tw[j + 1];
            uint32_t w = wv_alignbyte(hi, lo, sh);
            if (j + 1u == nd) w &= tail;
            tk_k64_step(ha, w);
            lo = hi;
        }
    }
    const uint32_t hb = tk_k64_tag(ha);
    uint32_t s = tk_k64_slot(ha, len) & t.key64_mask;
    // Two slots per round trip: a piece that is no token (most long pieces of running text) ends at the first EMPTY slot, and with
    // one slot per trip the wave waited for the longest probe chain among its lanes.
    for (uint32_t tries = 0; tries <= t.key64_mask; tries += 2) {
        const uint32_t s1 = (s + 1u) & t.key64_mask;
        tk_u32x4 e0 = *reinterpret_cast<const tk_u32x4*>(t.key64_tab + s);   // {tag, rank, len, blob_off}
        tk_u32x4 e1 = *reinterpret_cast<const tk_u32x4*>(t.key64_tab + s1);
        WV_PIN(e0.x); WV_PIN(e1.x);                         // both loads before the first compare
        for (int q = 0; q < 2; ++q) {
            const tk_u32x4 e = q ? e1 : e0;
            if (e.z == 0u) return TK_RANK_MAX;
            if (((e.z ^ len) | (e.x ^ hb)) == 0u) {
                const uint8_t* qb = t.blob + e.w;                                 // (the blob has 16 bytes of slack behind its last token)
                uint32_t diff = 0, lo = tw[0];
                for (uint32_t j = 0; j < nd; ++j) {
                    const uint32_t hi = tw[j + 1];
                    uint32_t w = wv_alignbyte(hi, lo, sh) ^ tk_load_u32_unaligned(qb + 4u * j);
                    if (j + 1u == nd) w &= tail;
                    diff |= w;
                    lo = hi;
                }
                if (diff == 0u) return e.y;
            }
        }
        s = (s + 2u) & t.key64_mask;
    }
    return TK_RANK_MAX;
}

struct alignas(16) tk_u64x2 { uint64_t x, y; };

// PAIR: buckets of two entries (one 16-byte load).  Most probes of the merge loop are for pairs that are NOT tokens;
// the first-choice bucket alone settles them unless it is flagged (something spilled from it): one scattered load per
// probe instead of two -- the merge kernel is bound by exactly those loads.  An empty entry is all ones and matches
// no key.
TK_DEV uint32_t tk_pair_in(const tk_u64x2& p, uint64_t key) {
    uint32_t r = TK_RANK_MAX;
    if (tk_pair_key(p.x) == key) r = tk_pair_rank(p.x);
    if (tk_pair_key(p.y) == key) r = tk_pair_rank(p.y);
    return r;
}
TK_DEV bool tk_pair_spilled(const tk_u64x2& p) { return p.x != TK_PAIR_EMPTY && (p.x & TK_PAIR_SPILL) != 0ull; }

// the merge kernels' form: either probe may be unwanted, and `filt` (the PAIR filter, tk_hash.h, in LDS there) lets a
// probe whose bit is clear skip its gather -- the pair is in no bucket
TK_DEV void tk_probe_pair_x2f(const TkTablesView& t, const uint32_t* filt, bool want0, uint32_t a0, uint32_t b0, bool want1,
                              uint32_t a1, uint32_t b1, uint32_t& r0, uint32_t& r1) {
    const uint64_t key0 = ((uint64_t)a0 << TK_ID_BITS) | (uint64_t)b0, key1 = ((uint64_t)a1 << TK_ID_BITS) | (uint64_t)b1;
    const uint32_t h0 = tk_pair_hash(a0, b0), h1 = tk_pair_hash(a1, b1);
    const uint32_t f0 = tk_pair_fbit(h0), f1 = tk_pair_fbit(h1);
    bool m0 = want0, m1 = want1;
    if (filt) {
        const uint32_t w0 = filt[f0 >> 5], w1 = filt[f1 >> 5];
        m0 = m0 && ((w0 >> (f0 & 31u)) & 1u);
        m1 = m1 && ((w1 >> (f1 & 31u)) & 1u);
    }
    tk_u64x2 p0, p1;
    p0.x = p0.y = p1.x = p1.y = TK_PAIR_EMPTY;
    if (m0) p0 = *reinterpret_cast<const tk_u64x2*>(t.pair_tab + 2u * (h0 & t.pair_mask));
    if (m1) p1 = *reinterpret_cast<const tk_u64x2*>(t.pair_tab + 2u * (h1 & t.pair_mask));
    WV_PIN(p0.x); WV_PIN(p0.y); WV_PIN(p1.x); WV_PIN(p1.y);
    r0 = tk_pair_in(p0, key0);
    r1 = tk_pair_in(p1, key1);
    const bool n0 = r0 == TK_RANK_MAX && tk_pair_spilled(p0), n1 = r1 == TK_RANK_MAX && tk_pair_spilled(p1);
    if (n0 || n1) {
        tk_u64x2 q0, q1;
        q0.x = q0.y = q1.x = q1.y = TK_PAIR_EMPTY;
        if (n0) q0 = *reinterpret_cast<const tk_u64x2*>(t.pair_tab + 2u * (tk_hash_alt(h0) & t.pair_mask));
        if (n1) q1 = *reinterpret_cast<const tk_u64x2*>(t.pair_tab + 2u * (tk_hash_alt(h1) & t.pair_mask));
        WV_PIN(q0.x); WV_PIN(q0.y); WV_PIN(q1.x); WV_PIN(q1.y);
        if (n0) r0 = tk_pair_in(q0, key0);
        if (n1) r1 = tk_pair_in(q1, key1);
    }
}

// two independent PAIR probes: both first-choice buckets are in flight together, and so are the second-choice ones of
// the (few) lanes that need them
TK_DEV void tk_probe_pair_x2(const TkTablesView& t, uint32_t a0, uint32_t b0, uint32_t a1, uint32_t b1, uint32_t& r0,
                             uint32_t& r1) {
    tk_probe_pair_x2f(t, nullptr, true, a0, b0, true, a1, b1, r0, r1);
}

TK_DEV uint32_t tk_probe_pair(const TkTablesView& t, uint32_t a, uint32_t b) {
    const uint64_t key = ((uint64_t)a << TK_ID_BITS) | (uint64_t)b;
    const uint32_t h = tk_pair_hash(a, b);
    tk_u64x2 p = *reinterpret_cast<const tk_u64x2*>(t.pair_tab + 2u * (h & t.pair_mask));
    WV_PIN(p.x); WV_PIN(p.y);
    uint32_t r = tk_pair_in(p, key);
    if (r == TK_RANK_MAX && tk_pair_spilled(p)) {
        tk_u64x2 q = *reinterpret_cast<const tk_u64x2*>(t.pair_tab + 2u * (tk_hash_alt(h) & t.pair_mask));
        WV_PIN(q.x); WV_PIN(q.y);
        r = tk_pair_in(q, key);
    }
    return r;
}
TK_DEV uint32_t tk_probe_pair_f(const TkTablesView& t, const uint32_t* filt, uint32_t a, uint32_t b) {
    if (!filt) return tk_probe_pair(t, a, b);
    const uint32_t f = tk_pair_fbit(tk_pair_hash(a, b));
    return ((filt[f >> 5] >> (f & 31u)) & 1u) ? tk_probe_pair(t, a, b) : TK_RANK_MAX;
}

TK_DEV uint32_t tk_wave_sum(uint32_t v, int lane) {
    for (int d = 1; d < 64; d <<= 1) v += wv_shfl(v, lane ^ d);
    return v;
}

TK_DEV uint64_t tk_wave_min64(uint64_t v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t lo = wv_shfl((uint32_t)v, lane ^ d);
        uint32_t hi = wv_shfl((uint32_t)(v >> 32), lane ^ d);
        uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

// minimum of (rank << 32 | pos) over the wave with the DPP reduction (two 32-bit minima: the rank, then the position
// among the lanes that hold it) -- about 150 clocks instead of the 1 500 of the bpermute butterfly on 64-bit values
TK_DEV uint64_t tk_wave_min_key(uint32_t rank, uint32_t pos) {
    const uint32_t r = wv_min_u32(rank);
    const uint32_t p = wv_min_u32(rank == r ? pos : 0xFFFFFFFFu);
    return r == TK_RANK_MAX ? ~0ull : (((uint64_t)r << 32) | (uint64_t)p);
}

TK_DEV TkPolyPow tk_poly_pow(const TkTablesView& t, int lane) {
    TkPolyPow p;
    p.pw1 = 1u; p.ipw1 = 1u; p.pw2 = 1u; p.ipw2 = 1u;
    for (int i = 0; i < lane; ++i) {
        p.pw1 *= TK_POLY_P1; p.ipw1 *= t.p1inv;
        p.pw2 *= TK_POLY_P2; p.ipw2 *= t.p2inv;
    }
    return p;
}

#endif
