// tk_encode_impl.h -- the wave-level tokenization algorithm (split + lookup + merge + emit).
//
// This is the device code of the hot path named by BASELINE.json: what the reference does in
//   CoreBPE::encode(text, {})              reference src/tekkenizer.rs:384-386
//   token += num_special_tokens            reference src/tekkenizer.rs:390-392
//   BOS / EOS insertion                    reference src/tekkenizer.rs:394-402
// re-designed for 64-wide CDNA4 wavefronts: one wave walks one document with a sliding
// 64-byte window, ONE LANE PER BYTE.
//
//   1. load 64 bytes, classify every code point (ASCII by ALU, others via the class trie)
//   2. wave ballots turn the classes into 64-bit masks; every lane decides locally whether a
//      piece starts at its byte (the 7 alternatives of src/tekkenizer.rs:123 restated as
//      local rules -- DESIGN.md "Split rules", modelled in tools/split_rules_model.py)
//   3. the window commits up to its last start that no unseen byte can change
//   4. each piece-start lane probes SHORT/LONG for the whole-piece shortcut
//   5. pieces that miss are merged in place: lanes are parts, an `alive` ballot mask is the
//      part list, the leftmost minimum-rank pair of every piece is found with a segmented
//      min-scan over lanes and merged, one merge per piece per round (exactly the order of
//      tiktoken's _byte_pair_merge); pair ranks come from PAIR2/PAIR
//   6. surviving part heads are compacted with popcounts and written as final ids
//
// A document with a piece that does not fit a window (>~60 bytes) is handed to a second pass
// (tk_encode_doc_seq): sequential end search per piece, wave-wide polynomial hash, LONG probe
// and, on a miss, a wave-cooperative merge over scratch memory with per-64-part block minima.
//
// The file is included with a set of wave primitives already defined (wv_lane, wv_ballot,
// wv_shfl, wv_first, wv_first64, wv_up1, wv_dn1, wv_sync, wv_atomic_add, wv_atomic_add_all, wv_brev64, wv_min_u32, wv_readlane, TK_DEV): tk_wave_hip.h for gfx950, and a
// fiber emulator in tests/emu/ that lets the CPU test-suite run this very source.
//
// Beside this file: tk_lookup.h (classes, probes, reductions: all the flat path takes), tk_match.h (matchers), tk_piece_impl.h (one piece).
#ifndef TK_ENCODE_IMPL_H
#define TK_ENCODE_IMPL_H
#include <stdint.h>

#include "tk_encode_impl_args.h"
#include "tk_lookup.h"
#include "tk_match.h"
#include "tk_piece_impl.h"

#define TK_DOC_CHUNK 8u /* documents taken per work-queue fetch */

// ---- one document: its staging slots, BOS in front (the ids written so far: 0 / 1) -- EOS behind, and the id count
TK_DEV uint32_t tk_doc_begin(const TkEncodeArgs& a, uint64_t d, int lane, uint64_t& s0, uint64_t& s1, uint32_t*& out) {
    s0 = wv_first64(a.doc_offs[d]);
    s1 = wv_first64(a.doc_offs[d + 1]);
    out = a.staging + s0 + 2 * d;
    if (!a.add_bos) return 0u;
    if (lane == 0) out[0] = a.t.bos_id;
    return 1u;
}
TK_DEV void tk_doc_end(const TkEncodeArgs& a, uint64_t d, int lane, uint32_t* out, uint32_t cursor) {
    if (a.add_eos) {
        if (lane == 0) out[cursor] = a.t.eos_id;
        cursor += 1;
    }
    if (lane == 0) a.counts[d] = cursor;
}

// ---- the window of tk_encode_doc (TkWin: what lives from one window to the next), and what one step of a window hands the
// next (TkStep: made anew for every window -- a step's result kept across the loop costs the split-only kernel registers)
struct TkWin {
    uint64_t w0, s1;           // the window starts at byte w0; the document ends at s1
    uint32_t cur, nxt;         // my byte of [w0, w0+64) and of [w0+64, w0+128) (0 past the document end)
};
struct TkStep {
    int nv; bool at_end;       // 1: bytes of the window that are decided here; the window holds the document's last byte
    uint32_t b0, b1, b2, b3;   //    my byte (0 from nv on) and the three behind it
    uint64_t PS; int fu;       // 2: piece starts decided by this window; first position whose decision unseen bytes could change
};
TK_DEV uint32_t tk_win_bytes(const TkEncodeArgs& a, uint64_t pos, uint64_t s1, int lane) {
    return (pos + (uint64_t)lane < s1) ? (uint32_t)a.bytes[pos + lane] : 0u;
}
// software prefetch: `cur` = bytes [w0, w0+64), `nxt` = bytes [w0+64, w0+128) (0 past the document end).
// The next window starts at w0 + region_end <= w0 + 64, so its bytes are a lane rotation of
// (cur, nxt); the global load issued for the new `nxt` is only consumed one window later.
TK_DEV void tk_win_load(const TkEncodeArgs& a, TkWin& W, int lane) {
    W.cur = tk_win_bytes(a, W.w0, W.s1, lane);
    W.nxt = tk_win_bytes(a, W.w0 + 64, W.s1, lane);
}

// ---- 1. load + classify: nv, at_end, b0..b3; true = no byte >= 0x80 (wave-uniform: the common case takes the scalar rules)
TK_DEV bool tk_win_trim(const TkWin& W, TkStep& S, int lane) {
    const uint64_t rem = W.s1 - W.w0;
    int nv = rem < 64 ? (int)rem : 64;
    S.at_end = rem <= 64;
    uint32_t b0 = lane < nv ? W.cur : 0u;
    const bool ascii = wv_ballot(b0 >= 0x80u) == 0;
    if (!S.at_end && !ascii) {
        // a char cut by the window end has an unknown class: leave it to the next window
        uint32_t nominal = b0 < 0xC0u ? 1u : b0 < 0xE0u ? 2u : b0 < 0xF0u ? 3u : b0 < 0xF8u ? 4u : 1u;
        uint64_t csraw = wv_ballot(lane < nv && ((b0 & 0xC0u) != 0x80u || lane == 0));
        int last = tk_msb64(csraw);
        uint32_t nl = wv_first(wv_shfl(nominal, last));
        if (last + (int)nl > nv && last > 0) nv = last;
        if (lane >= nv) b0 = 0u;
    }
    S.nv = nv;
    S.b0 = b0;
    S.b1 = wv_up1(b0); S.b2 = wv_up1(S.b1); S.b3 = wv_up1(S.b2);
    return ascii;
}

// carry ripple: the bits of the runs of `run` from a seed (a bit of `run`) up to the run's top
TK_DEV uint64_t tk_ripple(uint64_t run, uint64_t seeds) { return ((run + seeds) ^ run) & run; }

// ---- 2a. ASCII window: one byte = one char, the rules are pure 64-bit mask algebra on
//          SGPR pairs (no per-lane work, no divergent branch).  Same rules as 2b below.
TK_DEV void tk_rules_ascii(TkStep& S) {
    const uint32_t b0 = S.b0;
    const int nv = S.nv;
    const uint32_t cls = tk_ascii_class(b0);
    const uint64_t VAL = tk_lowmask(nv);
    // bytes past nv are 0 (class O), so single compares are already masked by validity
    const uint64_t mL = wv_ballot(cls == TK_CLS_L);
    const uint64_t mN = wv_ballot(cls == TK_CLS_N);
    const uint64_t mS = wv_ballot(cls == TK_CLS_S);
    const uint64_t mO = VAL & ~(mL | mN | mS);
    const uint64_t NLm = wv_ballot(b0 == 10u) | wv_ballot(b0 == 13u);
    const uint64_t SPm = wv_ballot(b0 == 0x20u);
    const uint64_t APm = wv_ballot(b0 == 0x27u);
    uint64_t CEND = 0;
    if (APm) {  // alt 1 fires only where a match starts at the apostrophe
        const uint32_t f1 = S.b1 | 0x20u, f2 = S.b2 | 0x20u;
        const bool c2 = f1 == 's' || f1 == 't' || f1 == 'm' || f1 == 'd';
        const bool c3 = ((f1 == 'r' || f1 == 'v') && f2 == 'e') || (f1 == 'l' && f2 == 'l');
        const uint64_t ok = APm & ~((mO | SPm) << 1);
        CEND = ((wv_ballot(c2) & ok) << 2) | ((wv_ballot(c3 && !c2) & ok) << 3);
    }
    const uint64_t L1 = mL << 1, O1 = mO << 1;
    const uint64_t Lst = mL & ~L1;
    const uint64_t psL = (mL & L1 & CEND) | (Lst & ((mN | NLm) << 1)) | (Lst & O1 & ((mO | SPm) << 2));
    const uint64_t psO = mO & ~O1 & ~(SPm << 1);
    uint64_t psN = mN & ~(mN << 1);
    {
        const uint64_t M3 = mN & (mN << 1) & (mN << 2) & (mN << 3);  // q-3..q all numbers
        if (M3) {  // a run of >= 4 numbers: starts every 3 chars (\p{N}{1,3}), by prefix doubling
            const uint64_t M6 = M3 & (M3 << 3), M12 = M6 & (M6 << 6), M24 = M12 & (M12 << 12);
            const uint64_t M48 = M24 & (M24 << 24);
            psN |= (psN << 3) & M3;
            psN |= (psN << 6) & M6;
            psN |= (psN << 12) & M12;
            psN |= (psN << 24) & M24;
            psN |= (psN << 48) & M48;
        }
    }
    // white space: CR/LF absorbed by alt 4 directly after an O run (carry ripple)
    const uint64_t seeds = NLm & O1;
    const uint64_t ABS = seeds ? tk_ripple(NLm, seeds) : 0ull;
    const uint64_t SPR = mS & ~ABS;
    const uint64_t NLp = NLm & SPR;
    uint64_t Z = 0;  // positions up to and including the last CR/LF of their run (\s*[\r\n]+)
    if (NLp) {
        // T = the part of each run above its last CR/LF, found in bit-reversed space by a
        // ripple from the run tops through the non-CR/LF bits
        const uint64_t r = wv_brev64(SPR), s = wv_brev64(NLp);
        const uint64_t u = r & ~s;
        const uint64_t tops = r & ~(r << 1) & u;
        const uint64_t T = wv_brev64(tk_ripple(u, tops));
        Z = SPR & ~T;
    }
    const uint64_t psS = (SPR & ~(SPR << 1)) | ((Z << 1) & SPR & ~Z) | (SPR & ~(SPR >> 1) & ~Z & (VAL >> 1));
    S.PS = (psL | psN | psO | psS | 1ull) & VAL;
    S.fu = nv;
    if (!S.at_end && tk_bit(SPR, nv - 1)) {  // the run that touches the window end is undecided past its first char
        const uint64_t below = ~SPR & VAL;
        const int rs = below ? tk_msb64(below) + 1 : 0;
        S.fu = rs + 1 < nv ? rs + 1 : nv;
    }
}

// ---- 2b. general window (multi-byte code points): per-lane rules
TK_DEV void tk_rules_general(const TkTablesView& t, TkStep& S, int lane) {
    const uint32_t b0 = S.b0, b1 = S.b1, b2 = S.b2;
    const int nv = S.nv;
    const bool at_end = S.at_end, valid = lane < nv;
    const bool lead = (b0 & 0xC0u) != 0x80u || lane == 0;
    uint32_t cls = TK_CLS_O, clen = 1;
    if (b0 < 0x80u) {
        cls = tk_ascii_class(b0);
    } else if (lead && b0 >= 0xC0u) {
        const uint32_t b3 = S.b3;
        uint32_t cp = 0xFFFFFFFFu;
        if (b0 < 0xE0u) {
            if ((b1 & 0xC0u) == 0x80u) { cp = ((b0 & 0x1Fu) << 6) | (b1 & 0x3Fu); clen = 2; }
        } else if (b0 < 0xF0u) {
            if ((b1 & 0xC0u) == 0x80u && (b2 & 0xC0u) == 0x80u) {
                cp = ((b0 & 0x0Fu) << 12) | ((b1 & 0x3Fu) << 6) | (b2 & 0x3Fu); clen = 3;
            }
        } else if (b0 < 0xF8u) {
            if ((b1 & 0xC0u) == 0x80u && (b2 & 0xC0u) == 0x80u && (b3 & 0xC0u) == 0x80u) {
                cp = ((b0 & 0x07u) << 18) | ((b1 & 0x3Fu) << 12) | ((b2 & 0x3Fu) << 6) | (b3 & 0x3Fu); clen = 4;
            }
        }
        if (cp != 0xFFFFFFFFu) cls = tk_uc_class(t, cp);
    }
    const uint64_t CS = wv_ballot(valid && lead);
    {
        // continuation bytes take the class of their lead byte so that runs are contiguous
        const uint32_t c1 = wv_dn1(cls), c2 = wv_dn1(c1), c3 = wv_dn1(c2);
        if (!lead) {
            int dist = lane - tk_msb64(CS & tk_lowmask(lane));
            cls = dist == 1 ? c1 : dist == 2 ? c2 : dist == 3 ? c3 : TK_CLS_O;
        }
    }
    const uint64_t mL = wv_ballot(valid && cls == TK_CLS_L);
    const uint64_t mN = wv_ballot(valid && cls == TK_CLS_N);
    const uint64_t mS = wv_ballot(valid && cls == TK_CLS_S);
    const uint64_t mO = wv_ballot(valid && cls == TK_CLS_O);
    const uint64_t NLm = wv_ballot(valid && (b0 == 10u || b0 == 13u));
    const uint64_t SPm = wv_ballot(valid && b0 == 0x20u);

    // (local piece-start rules, per lane) ---------------------------------------------------
    // alt 1 (?i:'s|'t|'re|'ve|'m|'ll|'d): fires only where a match starts at the apostrophe
    uint32_t ce = 0;
    if (b0 == 0x27u) {
        const uint32_t f1 = b1 | 0x20u, f2 = b2 | 0x20u;
        if (f1 == 's' || f1 == 't' || f1 == 'm' || f1 == 'd') ce = 2;
        else if (b1 == 0xC5u && b2 == 0xBFu) ce = 3;  // U+017F folds to 's'
        else if (((f1 == 'r' || f1 == 'v') && f2 == 'e') || (f1 == 'l' && f2 == 'l')) ce = 3;
    }
    const bool fire = ce && (lane == 0 || (!tk_bit(mO, lane - 1) && !tk_bit(SPm, lane - 1)));
    const uint64_t F2 = wv_ballot(valid && fire && ce == 2);
    const uint64_t F3 = wv_ballot(valid && fire && ce == 3);
    const uint64_t CEND = (F2 << 2) | (F3 << 3);
    // CR/LF absorbed by alt 4's trailing [\r\n]*: leading CR/LF of a white-space run that
    // directly follows a class-O byte (carry ripple through the CR/LF run)
    const uint64_t ABS = tk_ripple(NLm, NLm & (mO << 1));
    const uint64_t SPR = mS & ~ABS;  // effective white space
    const uint64_t Nst = mN & ~(mN << 1);

    bool st = false, unc = false;
    if (valid && lead) {
        if (lane == 0) {
            st = true;
        } else {
            const int pm = lane - 1;
            const bool pL = tk_bit(mL, pm), pN = tk_bit(mN, pm), pS = tk_bit(mS, pm), pO = tk_bit(mO, pm);
            if (cls == TK_CLS_L) {
                if (pL) st = tk_bit(CEND, lane);             // only right after a contraction
                else if (pN) st = true;
                else if (pS) st = tk_bit(NLm, pm);           // other white space is alt 2's prefix
                else {
                    const int qs = tk_msb64(CS & tk_lowmask(lane));
                    const bool runstart = qs == 0 || !tk_bit(mO, qs - 1);
                    st = !runstart || (qs > 0 && tk_bit(SPm, qs - 1));
                }
            } else if (cls == TK_CLS_N) {
                if (!pN) st = true;
                else {
                    const int rs = tk_msb64(Nst & tk_lowmask(lane + 1));
                    const int k = tk_popc64(CS & tk_lowmask(lane) & ~tk_lowmask(rs));
                    st = (k % 3) == 0;                       // \p{N}{1,3}
                }
            } else if (cls == TK_CLS_O) {
                st = !pO && !tk_bit(SPm, pm);                // ' ?' of alt 4 takes one U+0020
            } else {
                (void)pS;
                if (tk_bit(ABS, lane)) st = false;
                else if (!tk_bit(SPR, pm)) st = true;        // start of the effective run
                else {
                    const uint64_t x = SPR >> lane;
                    const int rl = tk_ctz64(~x);
                    const int e = lane + rl;
                    if (!at_end && e >= nv) unc = true;      // run reaches unseen bytes
                    else {
                        const bool later_nl = ((NLm >> lane) & tk_lowmask(rl)) != 0;
                        if (later_nl) st = false;            // inside \s*[\r\n]+
                        else if (tk_bit(NLm, pm)) st = true; // first char after the last CR/LF
                        else st = (lane + (int)clen == e) && (e < nv);  // \s+(?!\S) leaves the last char
                    }
                }
            }
        }
    }
    S.PS = wv_ballot(st);
    const uint64_t UNC = wv_ballot(unc);
    S.fu = UNC ? tk_ctz64(UNC) : nv;
}

// MODE 0: pass 1 (a document whose first unfinished piece does not end inside a window is handed
//         to pass 2: return false);  MODE 2: split only (tk_split_batch), long pieces are skipped
//         over with the sequential matcher.
template <int MODE>
TK_DEV bool tk_encode_doc(const TkEncodeArgs& a, uint64_t d, int lane, const TkPolyPow& pw) {
    const TkTablesView& t = a.t;
    TkWin W;
    uint64_t s0;
    uint32_t* out;
    uint32_t cursor = tk_doc_begin(a, d, lane, s0, W.s1, out);
    W.w0 = s0;
    tk_win_load(a, W, lane);
    while (W.w0 < W.s1) {
        TkStep S;
        if (tk_win_trim(W, S, lane)) tk_rules_ascii(S);
        else tk_rules_general(t, S, lane);
        // ---- 3. how far may this window commit? -------------------------------------------
        int region_end;
        uint64_t PSp;
        if (S.at_end) {
            region_end = S.nv;
            PSp = S.PS;
        } else {
            const uint64_t cert = S.PS & tk_lowmask(S.fu);
            const int estar = tk_msb64(cert);
            if (estar == 0) {
                // the first piece does not end inside the window
                if (MODE != 2) return false;
                const uint64_t e = wv_first64(tk_match_end(t, a.bytes, W.w0, W.s1));
                for (uint64_t q = W.w0 + (uint64_t)lane; q < e; q += 64) a.dbg_starts[q] = (q == W.w0);
                W.w0 = e;
                tk_win_load(a, W, lane);
                continue;
            }
            region_end = estar;
            PSp = cert & ~(1ull << estar);
        }
        const bool inreg = lane < region_end;
        // slide: rotate (cur, nxt) by region_end lanes and start the load of the following 64 bytes
        {
            const int idx = region_end + lane;
            const uint32_t ra = wv_shfl(W.cur, idx & 63), rb = wv_shfl(W.nxt, idx & 63);
            const uint64_t nw = W.w0 + (uint64_t)region_end;
            W.cur = idx < 64 ? ra : rb;
            W.nxt = tk_win_bytes(a, nw + 64, W.s1, lane);
        }
        if (MODE == 2) {
            if (inreg) a.dbg_starts[W.w0 + lane] = tk_bit(PSp, lane);
            W.w0 += (uint64_t)region_end;
            continue;
        }
        const uint32_t b0 = S.b0, b1 = S.b1, b2 = S.b2, b3 = S.b3;

        // ---- 4. whole-piece lookup ----------------------------------------------------------
        const uint64_t E = PSp | (region_end < 64 ? (1ull << region_end) : 0ull);
        const int ps = tk_msb64(PSp & tk_lowmask(lane + 1));
        int pe;
        {
            const uint64_t y = lane < 63 ? (E >> (lane + 1)) : 0ull;
            pe = y ? lane + 1 + tk_ctz64(y) : 64;
        }
        const bool isstart = inreg && tk_bit(PSp, lane);
        const int len = pe - lane;
        // exact-key material: every lane masks its own 4 bytes to its piece (bytes of the NEXT piece are
        // zeroed at the source), the start lane then gathers the dwords at +4, +8, +12
        const uint32_t d4 = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
        const uint32_t d4m = len >= 4 ? d4 : (d4 & ((1u << (8 * len)) - 1u));  // len = bytes left in my piece (>= 1)
        const uint32_t g1 = wv_shfl(d4m, (lane + 4) & 63), g2 = wv_shfl(d4m, (lane + 8) & 63);
        const uint32_t g3 = wv_shfl(d4m, (lane + 12) & 63);

        uint32_t h1 = 0, h2 = 0;
        const uint64_t LONGM = wv_ballot(isstart && len >= 17);
        if (LONGM) {
            const uint32_t t1 = b0 * pw.ipw1, t2 = b0 * pw.ipw2;
            uint32_t f1 = t1, f2 = t2;
            for (int dd = 1; dd < 64; dd <<= 1) {
                const uint32_t o1 = wv_shfl(f1, lane >= dd ? lane - dd : lane);
                const uint32_t o2 = wv_shfl(f2, lane >= dd ? lane - dd : lane);
                if (lane >= dd) { f1 += o1; f2 += o2; }
            }
            const int el = pe - 1;
            const uint32_t fe1 = wv_shfl(f1, el), fe2 = wv_shfl(f2, el);
            const uint32_t pe1 = wv_shfl(pw.pw1, el), pe2 = wv_shfl(pw.pw2, el);
            h1 = (fe1 - (f1 - t1)) * pe1;
            h2 = (fe2 - (f2 - t2)) * pe2;
        }

        uint32_t tokv = TK_RANK_MAX;
        if (a.dbg_ablate & 1) tokv = 7u;
        else if (isstart) {
            if (len == 1) {
                tokv = b0;  // rank of a single byte is the byte (src/tekkenizer.rs:793-798)
            } else if (len <= 16) {
                // exact key: the piece bytes themselves, zero padded to 16 (lane + 4j is in my piece iff len > 4j)
                const uint32_t k0 = d4m, k1 = len > 4 ? g1 : 0u, k2 = len > 8 ? g2 : 0u, k3 = len > 12 ? g3 : 0u;
                tokv = tk_probe_key(t, k0, k1, k2, k3, (uint32_t)len);
            } else {
                tokv = tk_probe_long(t, h1, h2, (uint32_t)len, a.bytes + W.w0 + lane);
            }
        }
        const uint64_t Hm = wv_ballot(isstart && tokv != TK_RANK_MAX);
        const uint64_t Mi = PSp & ~Hm;

        // ---- 5. in-window byte-pair merge for the pieces that missed ------------------------
        uint64_t A = 0;
        uint32_t tok = b0;
        const bool inmiss = inreg && tk_bit(Mi, ps);
        if (Mi && !(a.dbg_ablate & 2)) {
            A = wv_ballot(inmiss);
            uint32_t prank = TK_RANK_MAX;
            if (inmiss && lane + 1 < pe) prank = t.pair2[b0 | (b1 << 8)];
            const int sl = pe - 1 < 63 ? pe - 1 : 63;
            for (int round = 0; round < 64; ++round) {  // a window holds at most 63 merges per piece
                const uint32_t key = prank == TK_RANK_MAX ? 0xFFFFFFFFu : ((prank << 6) | (uint32_t)lane);
                uint32_t m = key;
                for (int dd = 1; dd < 64; dd <<= 1) {
                    const uint32_t o = wv_shfl(m, lane >= dd ? lane - dd : lane);
                    if (lane >= dd && lane - dd >= ps) m = o < m ? o : m;
                }
                const uint32_t segmin = wv_shfl(m, sl);
                const bool winner = inmiss && key != 0xFFFFFFFFu && key == segmin;
                const uint64_t W = wv_ballot(winner);
                if (!W) break;
                const bool alive = tk_bit(A, lane);
                const uint64_t below = A & tk_lowmask(lane);
                const bool dead = alive && below && tk_bit(W, tk_msb64(below));
                const uint64_t Dm = wv_ballot(dead);
                A &= ~Dm;
                if (winner) tok = prank;          // merged token id == rank of the pair
                if (dead) prank = TK_RANK_MAX;
                const uint64_t z = lane < 63 ? (A >> (lane + 1)) : 0ull;
                const int na = z ? lane + 1 + tk_ctz64(z) : 64;
                const bool has_next = na < pe;
                const uint32_t tn = wv_shfl(tok, na < 64 ? na : lane);
                const bool need = tk_bit(A, lane) && (winner || (has_next && tk_bit(W, na)));
                if (need) prank = has_next ? tk_probe_pair(t, tok, tn) : TK_RANK_MAX;
            }
        }

        // ---- 6. emit --------------------------------------------------------------------------
        const bool hitstart = isstart && tokv != TK_RANK_MAX;
        const bool istok = hitstart || (inmiss && tk_bit(A, lane));
        const uint64_t Tm = wv_ballot(istok);
        if (istok && !(a.dbg_ablate & 4)) {
            out[cursor + (uint32_t)tk_popc64(Tm & tk_lowmask(lane))] = (hitstart ? tokv : tok) + t.num_special;
        }
        cursor += (uint32_t)tk_popc64(Tm);
        W.w0 += (uint64_t)region_end;
    }
    if (MODE != 2) tk_doc_end(a, d, lane, out, cursor);
    return true;
}

// ------------------------------------------------------------------------------------------
// pass 2: one deferred document, piece by piece (sequential matcher, tk_piece_lookup, tk_piece_merge_coop)
// ------------------------------------------------------------------------------------------
TK_DEV void tk_encode_doc_seq(const TkEncodeArgs& a, uint64_t d, int lane, const TkPolyPow& pw, uint32_t* scratch) {
    const TkTablesView& t = a.t;
    uint64_t s0, s1;
    uint32_t* out;
    uint32_t cursor = tk_doc_begin(a, d, lane, s0, s1, out);
    uint64_t w0 = s0;
    while (w0 < s1) {
        const uint64_t e = wv_first64(a.pattern ? tk_match_end2(t, a.bytes, w0, s1) : tk_match_end(t, a.bytes, w0, s1));
        const uint32_t r = tk_piece_lookup(a, pw, lane, w0, e);
        if (r != TK_RANK_MAX) {
            if (lane == 0) out[cursor] = r + t.num_special;
            cursor += 1;
        } else if (a.long_list && tk_piece_is_long(a, lane, w0, e) != 0u) {
            // a LONG piece that is not a vocabulary key: thousands of dependent merges for one wave.  The document goes to
            // tk_long.hip, which merges such a piece in rounds by a workgroup (all occurrences of a rank at once)
            if (lane == 0) {
                a.counts[d] = 0;
                a.long_list[wv_atomic_add(a.long_count, 1u)] = (uint32_t)d;
            }
            return;
        } else {
            tk_piece_merge_coop(a, lane, w0, e, out, cursor, scratch);
        }
        w0 = e;
    }
    tk_doc_end(a, d, lane, out, cursor);
}

// ------------------------------------------------------------------------------------------
// one wave: pull documents from the work queue until it is empty
// ------------------------------------------------------------------------------------------
// MODE 0: pass 1 over all documents; MODE 1: pass 2 over todo_list; MODE 2: split only;
// MODE 3: pass 1 over todo_list (the documents the flat path, tk_flat_impl.h, handed back)
template <int MODE>
TK_DEV void tk_encode_wave(const TkEncodeArgs& a, int lane, uint64_t wave_id) {
    const TkPolyPow pw = tk_poly_pow(a.t, lane);
    uint32_t* scratch = MODE == 1 ? a.scratch + wave_id * a.scratch_words_per_wave : nullptr;
    const uint64_t total = (MODE == 1 || MODE == 3) ? (uint64_t)(a.n_todo_dev ? wv_first(*a.n_todo_dev) : a.n_todo) : a.n_docs;
    const uint32_t chunk = MODE == 1 ? 1u : TK_DOC_CHUNK;
    for (;;) {
        // Every lane takes part in the fetch (the compiler folds it into ONE atomic of 64*chunk and
        // hands lane i the value old + i*chunk), so no lane-dependent branch feeds the loop condition:
        // with `if (lane == 0) base = atomicAdd(..)` the optimizer threaded lanes 1..63 around the
        // atomic and they re-ran the loop without lane 0 (observed on gfx950, ROCm 7.2).
        const uint32_t ticket = wv_first(wv_atomic_add_all(a.work_counter, chunk));
        const uint32_t base = ticket / 64u;  // scalar: document index, offsets and the window loop are wave-uniform
        if ((uint64_t)base >= total) break;
        const uint64_t hi = (uint64_t)base + chunk < total ? (uint64_t)base + chunk : total;
        for (uint64_t q = base; q < hi; ++q) {
            if (MODE == 1) {
                tk_encode_doc_seq(a, (uint64_t)wv_first(a.todo_list[q]), lane, pw, scratch);
            } else {
                const uint64_t doc = MODE == 3 ? (uint64_t)wv_first(a.todo_list[q]) : q;
                const bool ok = tk_encode_doc<(MODE == 3 ? 0 : MODE)>(a, doc, lane, pw);
                if (!ok && lane == 0) {
                    // pass 1 only: the document has a piece that does not fit a window
                    a.counts[doc] = 0;
                    const uint32_t slot = wv_atomic_add(a.defer_count, 1u);
                    a.defer_list[slot] = (uint32_t)doc;
                }
            }
        }
    }
}

#endif
