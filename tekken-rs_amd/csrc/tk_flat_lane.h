// tk_flat_lane.h -- the flat path's lane layout (overview: tk_flat_impl.h): LDS words of a wave, mask algebra, classification, split rules
#ifndef TK_FLAT_LANE_H
#define TK_FLAT_LANE_H
#include "tk_lookup.h"
#include "tk_flat_args.h"

#define TKF_WM 0xFFFFFFFFu
#define TKF_LOGW 5
#define TKF_TOPBIT 0x80000000u
#define TKF_NHL (TKF_HL / TKF_W)                     /* lanes of the left halo: 2 / 1 */
/* entries of the LDS piece list.  16 bytes per lane: every byte could start a piece.  32 bytes per lane: a chunk with
   more pieces than this (an average of under two bytes per piece over 2 KB) is handed back as a whole */
#ifndef TKF_LISTCAP
#define TKF_LISTCAP 1056
#endif
#define TKF_MAXPIECES (TKF_LISTCAP - 2)              /* + the sentinel */

// LDS words of one wave
#define TKF_L_LIST 0                                /* u16 [REGION + 4] piece positions, then the id slot of every piece */
#define TKF_L_DS (TKF_L_LIST + TKF_LISTCAP / 2)      /* [64] document-start mask words */
#define TKF_L_PS (TKF_L_DS + 64)                    /* [64] owned piece-start mask words */
#define TKF_L_PFX (TKF_L_PS + 64)                   /* [64] pieces before the lane */
#define TKF_L_BAD (TKF_L_PFX + 64)                  /* [64] positions that make their document fall back */
#define TKF_L_BPFX (TKF_L_BAD + 64)                 /* [64] bad positions before the lane */
/* the dealt walk's list of lead-byte positions (step 1, default pattern): u16 entries in the list words behind the class words */
#define TKF_WALKOFF 192                              /* words */
#define TKF_WALKCAP (2 * (TKF_LISTCAP / 2 - TKF_WALKOFF))   /* 672 positions; a region with more lead bytes is walked lane by lane */
#define TKF_L_CL TKF_L_LIST                          /* [3 * 64] classes L, N, S of the multi-byte code points (step 1 only: shares the
                                                        words of the piece list, which is built in step 5) */
#define TKF_L_KM (TKF_L_BPFX + 64)                  /* [17 * 4] byte masks of a zero-padded key of length 0..16 (filled once per wave) */
#define TKF_L_MEMO TKF_L_KM                          /* [4] row 0 of the key masks (length 0: never read): memo table base lo / hi, mask, the wave's hit count */
#define TKF_L_TXT (TKF_L_KM + 17 * 4)                /* [REGION / 4 + 4] the region's bytes: a piece's 16 bytes are read from here */
#define TKF_L_CONST (TKF_L_TXT + TKF_REGION / 4 + 4)              /* [8] wave-uniform constants of the probe: KEY8 mask, KEY16 mask, KEY8 base, KEY16 base.
                                                        The kernel is out of scalar registers (spilled SGPRs come back through
                                                        v_readlane, a VALU slot each, and VALU issue is what bounds it); an LDS
                                                        broadcast read costs an LDS slot, of which it has plenty */
#define TKF_LDS_WORDS (TKF_L_CONST + 8)
#define TKF_L_FS TKF_LDS_WORDS                       /* [64] CUT instantiation only: cut-only piece starts (fragments begin / end there) */
#define TKF_LDS_WORDS_CUT (TKF_LDS_WORDS + 64)

// ------------------------------------------------------------------------------------------
// lane-layout mask primitives (TKF_W bits per lane, bit i of lane l = region byte W l + i)
// ------------------------------------------------------------------------------------------
// (own word above / below the neighbour's in one register, then ONE bit-field extract: 3 VALU per shift, and the
// combined word is shared by shifts of the same mask)
// (one funnel shift over {own word : neighbour's word}: DPP move + v_alignbit)
TK_DEV uint32_t tkf_shl(uint32_t x, int k) { return (uint32_t)((((uint64_t)x << 32) | (uint64_t)wv_dn1(x)) >> (32 - k)); }  // 1 <= k <= 31
TK_DEV uint32_t tkf_shr(uint32_t x, int k) { return (uint32_t)((((uint64_t)wv_up1(x) << 32) | (uint64_t)x) >> k); }
TK_DEV uint32_t tkf_shl_any(uint32_t x, int k, int lane) {
    const int q = k >> TKF_LOGW, r = k & (TKF_W - 1);
    const int s1 = lane - q, s2 = lane - q - 1;
    uint32_t v1 = wv_shfl(x, s1 & 63), v2 = wv_shfl(x, s2 & 63);
    if (s1 < 0) v1 = 0;
    if (s2 < 0) v2 = 0;
    return (uint32_t)((((uint64_t)v1 << TKF_W) | (uint64_t)v2) >> (TKF_W - r)) & TKF_WM;
}
TK_DEV uint32_t tkf_shr_any(uint32_t x, int k, int lane) {
    const int q = k >> TKF_LOGW, r = k & (TKF_W - 1);
    const int s1 = lane + q, s2 = lane + q + 1;
    uint32_t v1 = wv_shfl(x, s1 & 63), v2 = wv_shfl(x, s2 & 63);
    if (s1 > 63) v1 = 0;
    if (s2 > 63) v2 = 0;
    return (uint32_t)((((uint64_t)v2 << TKF_W) | (uint64_t)v1) >> r) & TKF_WM;
}
TK_DEV bool tkf_any(uint32_t x) { return wv_ballot(x != 0u) != 0ull; }

// a + b over the whole region (64 x W bits): per-lane add, then a 64-bit carry look-ahead over the lane carries
// (G = lanes that generate a carry, P = lanes that would pass one on) hands every lane its carry-in
TK_DEV uint32_t tkf_add(uint32_t a, uint32_t b) {
    const uint32_t t = a + b;
    const uint64_t G = wv_ballot(t < a);                  // the word itself overflowed
    const uint64_t P = wv_ballot((t & TKF_WM) == TKF_WM);
    const uint64_t x = G | P;
    const uint64_t cin = (x + G) ^ x ^ G;  // carry into lane l = bit l
    return (t + (wv_inverse_ballot(cin) ? 1u : 0u)) & TKF_WM;
}
// bits of `run` covered by a carry that starts at `seeds` (subset of run) and ripples upwards through
// consecutive run bits, across lanes
TK_DEV uint32_t tkf_ripple(uint32_t run, uint32_t seeds) { return (tkf_add(run, seeds) ^ run) & run; }
// where a carry started at `seeds` comes to rest: the first position at or above each seed that is not in `run`
TK_DEV uint32_t tkf_land(uint32_t run, uint32_t seeds) { return tkf_add(run, seeds) & ~run & TKF_WM; }

TK_DEV uint32_t tkf_scan_excl(uint32_t v, int lane, uint32_t* total) {
    (void)lane;
    const uint32_t x = wv_scan_incl_u32(v);
    *total = wv_readlane(x, 63);
    return x - v;
}

// ------------------------------------------------------------------------------------------
// bit-plane classification of the lane's TKF_W bytes -> W-bit masks
// ------------------------------------------------------------------------------------------
struct TkfClass {
    uint32_t L, N, S, NL, SP, AP, HI, STMD, RV, E, LL;
    uint32_t U8C, LEAD, C5, BF;  // UTF-8: continuation bytes, lead bytes; C5 BF = U+017F (folds to 's')
    uint32_t UP, SL, X, M;    // upper-case letters, '/', neutral letters (Lm | Lo), marks (the JSON pattern of row f-3 only)
    uint32_t F2, F3;          // lead bytes of 2- / 3-byte chars that the RANGE RULES know to be letters (tkf_classify; 0 in an ASCII region)
    bool nmb;                 // wave-uniform: the region holds a multi-byte \p{N} char
};

// 8x8 bit-matrix transpose of 8 bytes (lo = bytes 0..3, hi = bytes 4..7): afterwards byte b holds bit b of every
// input byte (bit i of the result byte = bit b of input byte i).  Three delta swaps (1x1 blocks inside 2x2,
// 2x2 inside 4x4, 4x4 inside 8x8); the first two never cross the 32-bit halves.
TK_DEV void tkf_transpose8(uint32_t& lo, uint32_t& hi) {
    uint32_t t;
    t = ((lo >> 7) ^ lo) & 0x00AA00AAu; lo ^= t ^ (t << 7);
    t = ((hi >> 7) ^ hi) & 0x00AA00AAu; hi ^= t ^ (t << 7);
    t = ((lo >> 14) ^ lo) & 0x0000CCCCu; lo ^= t ^ (t << 14);
    t = ((hi >> 14) ^ hi) & 0x0000CCCCu; hi ^= t ^ (t << 14);
    t = (((lo >> 28) | (hi << 4)) ^ lo) & 0xF0F0F0F0u;   // delta 28 across the halves
    lo ^= t ^ (t << 28);
    hi ^= t >> 4;
}

// the lane's bytes -> the 8 bit planes (already in lane layout: bit i of plane b = bit b of byte i) -> the class
// masks as boolean functions of the planes.  ASCII classes of the pattern of src/tekkenizer.rs:123: L = [A-Za-z],
// N = [0-9], S = \s (9..13, 0x20); bytes >= 0x80 only set HI.
TK_DEV TkfClass tkf_classify(const uint32_t* x) {
    uint32_t a_lo = x[0], a_hi = x[1], b_lo = x[2], b_hi = x[3];
    tkf_transpose8(a_lo, a_hi);
    tkf_transpose8(b_lo, b_hi);
    // four groups of 8 bytes: plane p = byte p of the four transposed groups -- a 4 x 4 byte transpose (v_perm), twice
    uint32_t c_lo = x[4], c_hi = x[5], d_lo = x[6], d_hi = x[7];
    tkf_transpose8(c_lo, c_hi);
    tkf_transpose8(d_lo, d_hi);
    const uint32_t u0 = wv_perm(b_lo, a_lo, 0x05010400u), u1 = wv_perm(b_lo, a_lo, 0x07030602u);   // {a0 b0 a1 b1}, {a2 b2 a3 b3}
    const uint32_t v0 = wv_perm(d_lo, c_lo, 0x05010400u), v1 = wv_perm(d_lo, c_lo, 0x07030602u);
    const uint32_t p0 = wv_perm(v0, u0, 0x05040100u), p1 = wv_perm(v0, u0, 0x07060302u);
    const uint32_t p2 = wv_perm(v1, u1, 0x05040100u), p3 = wv_perm(v1, u1, 0x07060302u);
    const uint32_t u2 = wv_perm(b_hi, a_hi, 0x05010400u), u3 = wv_perm(b_hi, a_hi, 0x07030602u);
    const uint32_t v2 = wv_perm(d_hi, c_hi, 0x05010400u), v3 = wv_perm(d_hi, c_hi, 0x07030602u);
    const uint32_t p4 = wv_perm(v2, u2, 0x05040100u), p5 = wv_perm(v2, u2, 0x07060302u);
    const uint32_t p6 = wv_perm(v3, u3, 0x05040100u), p7 = wv_perm(v3, u3, 0x07060302u);
    TkfClass c;
    const uint32_t hz = TKF_WM & ~(p7 | p6 | p5 | p4);            // high nibble 0
    const uint32_t pre = p6 & ~p7;                                // 0x40..0x7F: letters differ in bit 5 only
    c.HI = p7;
    c.L = pre & (p4 | p3 | p2 | p1 | p0) & ~(p4 & p3 & (p2 | (p1 & p0)));       // low five bits in 1..26
    c.N = p5 & p4 & ~(p7 | p6) & ~(p3 & (p2 | p1));                             // 0x30..0x39
    c.SP = p5 & ~(p7 | p6 | p4) & ~(p3 | p2 | p1 | p0);                         // 0x20
    c.S = (hz & p3 & ((~p2 & (p1 | p0)) | (p2 & ~p1))) | c.SP;                  // 9..13, 0x20
    c.NL = hz & p3 & ((~p2 & p1 & ~p0) | (p2 & ~p1 & p0));                      // 10, 13
    c.AP = p5 & ~(p7 | p6 | p4) & ~p3 & p2 & p1 & p0;                           // 0x27
    const uint32_t q = pre & ~p3 & p4;                                          // low five bits 10xxx
    c.STMD = (q & ((~p2 & p1 & p0) | (p2 & ~p1 & ~p0))) |                       // s 10011, t 10100
             (pre & ~p4 & p2 & ~p1 & ((p3 & p0) | (~p3 & ~p0)));                // m 01101, d 00100
    c.RV = q & p1 & ~p0;                                                        // r 10010, v 10110
    c.E = pre & ~p4 & ~p3 & p2 & ~p1 & p0;                                      // e 00101
    c.LL = pre & ~p4 & p3 & p2 & ~p1 & ~p0;                                     // l 01100
    c.U8C = p7 & ~p6;
    c.LEAD = p7 & p6;
    c.C5 = p7 & p6 & ~(p5 | p4 | p3) & p2 & ~p1 & p0;                           // 1100 0101
    c.BF = p7 & ~p6 & p5 & p4 & p3 & p2 & p1 & p0;                              // 1011 1111
    c.UP = c.L & ~p5;                                                           // A..Z (letters differ in bit 5 only)
    c.SL = p5 & ~(p7 | p6 | p4) & p3 & p2 & p1 & p0;                             // 0x2F
    c.X = 0u;
    c.M = 0u;
    c.nmb = false;
    c.F2 = 0u;
    c.F3 = 0u;
    if (tkf_any(p7)) {
        // Range rules for the big letter blocks, as mask algebra on the planes (one instruction = 2048 bytes): a char they cover needs
        // no decode and no table look-up -- the per-char walk of tk_flat_chunk (two chars per round and lane: a third of this
        // kernel on mixed UTF-8 text) is left with what the rules do not cover.  Every rule names (lead byte, range of the
        // second byte) whose WHOLE block of code points is class L in the trie (tests/test_flat_path.py checks every code point
        // of the BMP through this path against the oracle, which reads the trie):
        //   3 bytes: E4 B8..BF, E5..E8, E9 80..BD (CJK unified U+4E00..9F7F); EA B0..BF, EB, EC, ED 80..9D (Hangul U+AC00..D77F)
        //   2 bytes: C3 except 97 / B7 (U+00C0..00FF without the two operators); D0, D1 80..8F (Cyrillic U+0400..044F);
        //            CE B1..BF, CF 80..8F (Greek U+03B1..03CF); D8 A0..BF (Arabic U+0620..063F)
        // The bytes behind the lead must be continuation bytes (anything else is for the walk to judge).
#define NX(m) tkf_shr((m), 1)
        const uint32_t cont = p7 & ~p6;
        const uint32_t nc1 = NX(cont), nc2 = tkf_shr(cont, 2);
        const uint32_t x54 = p5 & p4, x321 = p3 & p2 & p1;
        const uint32_t n_geB0 = NX(x54), n_geB8 = NX(x54 & p3), n_BEBF = NX(x54 & x321), n_ge90 = NX(p5 | p4), n_geA0 = NX(p5);
        const uint32_t n_ge9E = NX(p5 | (p4 & x321)), n_B1BF = NX(x54 & (p3 | p2 | p1 | p0)), n_x7 = NX(p4 & ~p3 & p2 & p1 & p0);
        const uint32_t hE = p7 & p6 & p5 & ~p4, hC = p7 & p6 & ~p5 & ~p4, hD = p7 & p6 & ~p5 & p4;
        const uint32_t l0 = ~p3 & ~p2 & ~p1 & ~p0, l1 = ~p3 & ~p2 & ~p1 & p0, l3 = ~p3 & ~p2 & p1 & p0, l4 = ~p3 & p2 & ~p1 & ~p0;
        const uint32_t l5678 = (~p3 & p2 & (p1 | p0)) | (p3 & ~p2 & ~p1 & ~p0);
        const uint32_t l8 = p3 & ~p2 & ~p1 & ~p0, l9 = p3 & ~p2 & ~p1 & p0, lA = p3 & ~p2 & p1 & ~p0, lB = p3 & ~p2 & p1 & p0;
        const uint32_t lC = p3 & p2 & ~p1 & ~p0, lD = p3 & p2 & ~p1 & p0, lE = p3 & p2 & p1 & ~p0, lF = p3 & p2 & p1 & p0;
        c.F3 = hE & nc1 & nc2 & (l5678 | (l4 & n_geB8) | (l9 & ~n_BEBF) | lB | lC | (lA & n_geB0) | (lD & ~n_ge9E));
        c.F2 = nc1 & ((hC & l3 & ~n_x7) | (hD & l0) | (hD & l1 & ~n_ge90) | (hC & lE & n_B1BF) | (hC & lF & ~n_ge90) | (hD & l8 & n_geA0));
#undef NX
    }
    return c;
}

// a mask set at the first bytes of chars (up to four bytes, inside a document) -> on all their bytes
TK_DEV uint32_t tkf_whole_chars(uint32_t X, uint32_t U8C, uint32_t nDS) {
    for (int k = 0; k < 3; ++k) X |= tkf_shl(X, 1) & nDS & U8C;
    return X;
}
// white space: piece starts of the runs SPR (the white space that no punctuation piece absorbs); *cont_out: run bytes behind the first
TK_DEV uint32_t tkf_space_starts(uint32_t SPR, uint32_t NL, uint32_t U8C, bool u8, uint32_t nDS, uint32_t nDE, int lane, uint32_t* cont_out) {
    const uint32_t CS = TKF_WM & ~U8C;
    const uint32_t cont = SPR & tkf_shl(SPR, 1) & nDS;
    uint32_t Z = NL & SPR;
    {
        uint32_t C = tkf_shr(cont, 1);
        int k = 1;
        while (tkf_any(C) && tkf_any(Z)) {
            Z |= tkf_shr_any(Z, k, lane) & C;
            C &= tkf_shr_any(C, k, lane);
            k *= 2;
        }
    }
    uint32_t last = SPR & ~tkf_shr(cont, 1) & ~Z & nDE;   // last byte of a run that a non-space char follows
    if (u8) {                                              // -> the first byte of its char
        last = (last & CS) | (tkf_shr(last & U8C, 1) & nDE);
        last = (last & CS) | (tkf_shr(last & U8C, 1) & nDE);
        last = (last & CS) | (tkf_shr(last & U8C, 1) & nDE);
        last &= CS;
    }
    const uint32_t psS = (SPR & ~cont) | (tkf_shl(Z, 1) & cont & ~Z) | last;
    *cont_out = cont;
    return psS;
}

// ------------------------------------------------------------------------------------------
// piece starts of the region (tools/flat_split_model.py flat_rules); also returns SPR / cont for the
// deferral test of the white-space run that reaches the region end
// ------------------------------------------------------------------------------------------
TK_DEV uint32_t tkf_rules(const TkfClass& m, uint32_t DS, int lane, uint32_t* SPR_out, uint32_t* cont_out) {
    const uint32_t nDS = ~DS & TKF_WM;
    const uint32_t DE = tkf_shr(DS, 1) | (lane == 63 ? TKF_TOPBIT : 0u);
    const uint32_t nDE = ~DE & TKF_WM;
#define P1(x) (tkf_shl((x), 1) & nDS)
#define N1(x) (tkf_shr((x), 1) & nDE)
    const uint32_t mL = m.L, mN = m.N, mS = m.S, NL = m.NL, SP = m.SP;
    const uint32_t U8C = m.U8C, CS = TKF_WM & ~U8C;  // first byte of every code point
    const bool u8 = tkf_any(m.HI);                   // wave-uniform: the region holds multi-byte code points
    const uint32_t mO = TKF_WM & ~(mL | mN | mS);
    const uint32_t pOS = P1(mO | SP);            // previous byte is class O or U+0020
    uint32_t CEND = 0;
    if (tkf_any(m.AP)) {                         // alt 1: fires only where a match starts at the apostrophe
        const uint32_t ok = m.AP & ~pOS;
        const uint32_t c2 = ok & N1(m.STMD);
        uint32_t three = (m.RV & N1(m.E)) | (m.LL & N1(m.LL));
        if (u8) three |= m.C5 & N1(m.BF);        // U+017F folds to 's' ((?i) of the pattern)
        const uint32_t c3 = ok & ~c2 & N1(three);
        CEND = tkf_shl(c2, 2) | tkf_shl(c3, 3);
    }
    const uint32_t L1 = P1(mL), O1 = P1(mO);
    const uint32_t Lst = mL & ~L1;
    // "the O char before me is not available as alt 2's prefix": it is itself preceded by O or U+0020.
    // X = such O chars, on all their bytes
    uint32_t X = CS & mO & pOS;
    if (u8) X = tkf_whole_chars(X, U8C, nDS);
    const uint32_t psL = (mL & L1 & CEND) | (Lst & P1(mN | NL)) | (Lst & P1(X));
    const uint32_t psO = mO & ~O1 & ~P1(SP);
    // numbers: every 3rd char of a run (\p{N}{1,3})
    const uint32_t N1m = P1(mN);
    uint32_t psN = mN & ~N1m;
    if (!m.nmb) {
        // one byte per char: prefix doubling on byte positions
        const uint32_t N2m = P1(N1m);
        uint32_t M = mN & N1m & N2m & P1(N2m);
        int k = 3;
        while (tkf_any(M)) {
            psN |= tkf_shl_any(psN, k, lane) & M;
            M &= tkf_shl_any(M, k, lane);
            k *= 2;
        }
    } else {
        // multi-byte digits: walk the runs three CHARS at a time (next char start = where a carry through the
        // continuation bytes comes to rest)
        uint32_t cur = psN;
        while (tkf_any(cur)) {
            for (int q = 0; q < 3; ++q) cur = tkf_land(U8C, tkf_shl(cur, 1)) & mN & nDS;
            cur &= ~psN;
            psN |= cur;
        }
    }
    // white space
    const uint32_t seeds = NL & O1;
    uint32_t ABS = 0;
    if (tkf_any(seeds)) ABS = tkf_ripple(NL & nDS, seeds);
    const uint32_t SPR = mS & ~ABS;
    uint32_t cont;
    const uint32_t psS = tkf_space_starts(SPR, NL, U8C, u8, nDS, nDE, lane, &cont);
#undef P1
#undef N1
    *SPR_out = SPR;
    *cont_out = cont;
    return psL | psN | psO | psS | DS;
}

// ------------------------------------------------------------------------------------------
// Row f-3: the JSON pattern of Mistral's tekken.json in lane layout (tools/flat_split_model.py flat_rules_tekken).  Scope:
// chars of the classes upper (Lu | Lt), lower (Ll), N, \s, other; a region with a neutral letter (Lm / Lo) or a mark
// is handed back.  Against tkf_rules: no contraction alternative; inside a letter run a piece starts at an upper-case
// char that follows a lower-case one; every digit is a piece; the tail absorbed after a punctuation run is made of
// CR / LF / '/' and whatever follows it starts a piece.
// ------------------------------------------------------------------------------------------
TK_DEV uint32_t tkf_rules_json(const TkfClass& m, uint32_t DS, int lane, uint32_t* SPR_out, uint32_t* cont_out) {
    const uint32_t nDS = ~DS & TKF_WM;
    const uint32_t DE = tkf_shr(DS, 1) | (lane == 63 ? TKF_TOPBIT : 0u);
    const uint32_t nDE = ~DE & TKF_WM;
#define P1(x) (tkf_shl((x), 1) & nDS)
#define N1(x) (tkf_shr((x), 1) & nDE)
    const uint32_t mL = m.L, mN = m.N, mS = m.S, NL = m.NL, SP = m.SP, mX = m.X, mM = m.M;
    const uint32_t U8C = m.U8C, CS = TKF_WM & ~U8C;
    const bool u8 = tkf_any(m.HI);
    const bool marks = u8 && tkf_any(mM), neutral = u8 && tkf_any(mX | mM);
    const uint32_t mO0 = TKF_WM & ~(mL | mX | mM | mN | mS);          // punctuation / symbols / everything else
    // Two sets that feed each other, both decided by the char to the LEFT: T = the tail [\r\n/]* of a punctuation piece (a
    // CR / LF behind any punctuation char, behind a mark that the 4th alternative swallowed, or behind a tail char; a '/'
    // behind a tail char) and A = where the 4th alternative is running (a punctuation char -- not one of a tail -- behind
    // U+0020, behind a punctuation char that is not in a tail, or behind A; a mark behind A: that alternative's class
    // holds \p{M}).  Position i needs position i - 1 only: iterating both definitions from nothing settles chains of
    // length k after k rounds (the chains are runs of punctuation / marks / line ends: short).
    uint32_t T = 0u, A = 0u;
    {
        const uint32_t O01 = P1(mO0);
        if (tkf_any(NL & O01) || marks) {
            const uint32_t SP1 = P1(SP);
            for (;;) {
                const uint32_t T1 = P1(T);
                const uint32_t T2 = (NL & (O01 | T1 | P1(mM & A))) | (m.SL & T1);
                uint32_t A2 = 0u;
                if (marks) {
                    A2 = CS & ((mO0 & ~T2 & (SP1 | P1(mO0 & ~T2) | P1(A))) | (mM & P1(A)));   // decided at the char's first byte ...
                    A2 = tkf_whole_chars(A2, U8C, nDS);                                      // ... and valid for all its bytes
                }
                const bool changed = tkf_any((T2 ^ T) | (A2 ^ A));
                T = T2;
                A = A2;
                if (!changed) break;
            }
        }
    }
    const uint32_t ABS = T;
    const uint32_t Mabs = mM & A;                                      // marks that count as punctuation
    const uint32_t mO = mO0 | Mabs;
    const uint32_t neut = mX | (mM & ~Mabs);                           // upper-side AND lower-side word chars
    const uint32_t mWd = mL | neut;                                    // word chars
    const uint32_t after_abs = P1(ABS) & ~ABS & CS;                    // whatever follows the tail starts a piece
    const uint32_t Oe = mO & ~ABS;
    const uint32_t pOS = P1(Oe | SP);
    const uint32_t Wst = mWd & ~P1(mWd);                               // first byte of a word run
    uint32_t X = CS & Oe & pOS;                                        // an O char that is not available as a word's one-char prefix
    if (u8) X = tkf_whole_chars(X, U8C, nDS);
    // inside a word run: an upper-case char starts a piece when the lower side has begun (a lower-case char, then any
    // neutral chars), and the all-upper tail of a run starts one behind a neutral char (the first alternative gives the
    // upper-side run back down to its last neutral char when nothing lower-side follows)
    uint32_t LW = mL & ~m.UP;
    uint32_t psC;
    if (neutral) {
        for (;;) {
            const uint32_t nxt = LW | (P1(LW) & neut);
            const bool grew = tkf_any(nxt & ~LW);
            LW = nxt;
            if (!grew) break;
        }
        uint32_t UE = m.UP & ~N1(mWd);                                 // upper-case chars with only upper-case chars up to the run end
        for (;;) {
            const uint32_t nxt = UE | (N1(UE) & m.UP);
            const bool grew = tkf_any(nxt & ~UE);
            UE = nxt;
            if (!grew) break;
        }
        psC = CS & ((m.UP & P1(LW)) | (UE & P1(neut)));
    } else {
        psC = CS & m.UP & P1(LW);
    }
    const uint32_t psL = (Wst & P1(mN | NL | X)) | psC;
    const uint32_t psO = Oe & ~P1(Oe) & ~P1(SP);
    const uint32_t psN = mN & CS;
    const uint32_t SPR = mS & ~ABS;
    uint32_t cont;
    const uint32_t psS = tkf_space_starts(SPR, NL, U8C, u8, nDS, nDE, lane, &cont);
#undef P1
#undef N1
    *SPR_out = SPR;
    *cont_out = cont;
    return psL | psN | psO | psS | after_abs | DS;
}

TK_DEV uint32_t tkf_lowmask32(int n) { return n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1u); }

#endif
