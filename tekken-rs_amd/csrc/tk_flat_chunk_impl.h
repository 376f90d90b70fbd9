// tk_flat_chunk_impl.h -- one chunk of the flat path by one wave (overview: tk_flat_impl.h).  A WV_KARGS field is read where it is used.
#ifndef TK_FLAT_CHUNK_IMPL_H
#define TK_FLAT_CHUNK_IMPL_H
#include "tk_flat_lane.h"

// once per wave, before its first chunk: the key byte masks
TK_DEV void tk_flat_init_lds(const TkFlatArgs& a, uint32_t* lds, int lane) {
    if (lane == 63) {
        const uint64_t b8 = (uint64_t)reinterpret_cast<uintptr_t>(a.t.key8_tab), b16 = (uint64_t)reinterpret_cast<uintptr_t>(a.t.key_tab);
        lds[TKF_L_CONST + 0] = a.t.key8_mask;
        lds[TKF_L_CONST + 1] = a.t.key_mask;
        lds[TKF_L_CONST + 2] = (uint32_t)b8; lds[TKF_L_CONST + 3] = (uint32_t)(b8 >> 32);
        lds[TKF_L_CONST + 4] = (uint32_t)b16; lds[TKF_L_CONST + 5] = (uint32_t)(b16 >> 32);
        const uint64_t lc = (uint64_t)reinterpret_cast<uintptr_t>(a.long_ctl);
        lds[TKF_L_CONST + 6] = (uint32_t)lc; lds[TKF_L_CONST + 7] = (uint32_t)(lc >> 32);
    }
    if (lane >= 1 && lane <= 16) {
        for (int q = 0; q < 4; ++q) {
            const int keep = lane - 4 * q;
            lds[TKF_L_KM + 4 * lane + q] = keep >= 4 ? 0xFFFFFFFFu : keep <= 0 ? 0u : ((1u << (8 * keep)) - 1u);
        }
    }
    if (lane == 0) {
        // row 0 of the key masks is never read (no piece has length 0): it holds the memo's constants -- table base, mask -- and the
        // wave's count of memo hits (tk_flat_flush_memo_hits); the kernel has no LDS granule and no scalar register to spare
        const uint64_t mb = a.memo_probe ? (uint64_t)reinterpret_cast<uintptr_t>(a.memo_tab) : 0ull;
        lds[TKF_L_MEMO + 0] = (uint32_t)mb; lds[TKF_L_MEMO + 1] = (uint32_t)(mb >> 32);
        lds[TKF_L_MEMO + 2] = a.memo_mask;
        lds[TKF_L_MEMO + 3] = 0u;
    }
    wv_lds_sync();
}

// once per wave, behind its last chunk: the wave's memo hits into the call's device counter
TK_DEV void tk_flat_flush_memo_hits(const TkFlatArgs& a, uint32_t* lds, int lane) {
    if (a.memo_tab && a.memo_hits) {
        wv_lds_sync();
        const uint32_t v = lds[TKF_L_MEMO + 3];
        if (lane == 0 && v != 0u) wv_atomic_add(a.memo_hits, v);
    }
}

// timing-only ablations of the flat kernel (TK_DEBUG_ABLATE): compiled in by `make ablate` (-DTK_ABLATE) only -- the shipped
// library's DBG instantiation carries nothing but the per-byte piece-start flags of tk_split_batch
#ifdef TK_ABLATE
#define TKF_ABL(a, bit) (DBG && ((a).dbg_ablate & (bit)))
#else
#define TKF_ABL(a, bit) false
#endif

// chunk c commits the bytes [c0, c1) of the stream's n and loads the region [r0, r1); [ca, cb) = the commit range in region coordinates
struct TkfGeom {
    uint64_t c;
    int64_t n, c0, c1, r0, r1;
    int ca, cb, lane;
    uint32_t* lds;
    uint16_t* list;                                         // the LDS piece list
};
// steps 5 to 7, one pass over all lanes or two over half of them: pieces listed / owned, owned ones of the earlier pass, slots beyond one per piece,
// queued misses by class, lanes of the pass, end of its last piece
struct TkfPass {
    int npass;
    uint32_t np_all, np_own, base_own, E, nm0, nm1, nm2, nm3, lane_lo, lane_hi, sentinel;
};
// set bits of a mask kept in 64 LDS words below position p, given the counts before every word
TK_DEV uint32_t tkf_lds_rank(const uint32_t* pfx, const uint32_t* words, uint32_t p) {
    return pfx[p >> TKF_LOGW] + (uint32_t)__builtin_popcount(words[p >> TKF_LOGW] & ((1u << (p & (TKF_W - 1))) - 1u));
}
// the first piece start in the lanes from `from` on (dflt: there is none)
TK_DEV uint32_t tkf_first_start(uint32_t PS, int lane, int from, uint32_t dflt) {
    const uint64_t Bm = wv_ballot(lane >= from && PS != 0u);
    if (Bm) {
        const int fl = tk_ctz64(Bm);
        return (uint32_t)TKF_W * (uint32_t)fl + (uint32_t)__builtin_ctz(wv_readlane(PS, fl));
    }
    return dflt;
}
// (timing ablations 8 / 16: v keeps the work alive without producing slot counts -- the downstream kernels must see an empty chunk)
TK_DEV bool tkf_ablated_chunk(const TkFlatArgs& a, uint64_t c, int lane, uint32_t v) {
    if (lane == 0) {
        a.kcount[c] = v == 0xFFFFFFFFu ? 1u : 0u;
        for (int k = 0; k < 4; ++k) a.miss_count[k * a.n_chunks + c] = 0u;
    }
    return false;
}
// ---- 1. multi-byte code points ------------------------------------------------------------------
// the char at region byte p: code point (0xFFFFFFFF: malformed) and byte length, from the LDS copy of the region (zero outside [0, n))
TK_DEV uint32_t tkf_decode_at(const uint32_t* lds, uint32_t p, uint32_t* clen_out) {
    const uint32_t* tw = lds + TKF_L_TXT + (p >> 2);
    const uint32_t v4 = wv_alignbyte(tw[1], tw[0], p & 3u);
    const uint32_t b0 = v4 & 0xFFu, b1 = (v4 >> 8) & 0xFFu, b2 = (v4 >> 16) & 0xFFu, b3 = v4 >> 24;
    uint32_t cp = 0xFFFFFFFFu, clen = 1;
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
    *clen_out = clen;
    return cp;
}
// class L / N / S / O, default pattern: ONE load from the trie flattened for the BMP (callers request several words first); beyond it the trie
TK_DEV uint32_t tkf_bmp_word(const TkTablesView& t, uint32_t cp) { return t.uc_bmp[(cp < 0x10000u ? cp : 0u) >> 4]; }
TK_DEV uint32_t tkf_bmp_class(const TkTablesView& t, uint32_t cp, uint32_t cw) {
    const uint32_t q = cp < 0x10000u ? cp : 0u;
    uint32_t cls = (cw >> (2u * (q & 15u))) & 3u;
    if (cp >= 0x10000u) cls = cp == 0xFFFFFFFFu ? (uint32_t)TK_CLS_O : tk_uc_class(t, cp);
    return cls;
}
// ALL bytes of the char (clen bytes at bit sh of word wi; it may reach into the next word) into its class words; JSON: extra = 1 upper, 2 Lm | Lo, 3 mark
template <int PAT>
TK_DEV void tkf_mark_char(uint32_t* cl, uint32_t wi, uint32_t sh, uint32_t clen, uint32_t cls, uint32_t extra, bool& nmb) {
    const uint64_t bits = (uint64_t)((1u << clen) - 1u) << sh;
    if (PAT && extra) {
        wv_lds_or(cl + (2u + extra) * 64u + wi, (uint32_t)(bits & TKF_WM));
        if ((bits >> TKF_W) && wi < 63u) wv_lds_or(cl + (2u + extra) * 64u + wi + 1u, (uint32_t)(bits >> TKF_W));
    }
    if (cls != TK_CLS_O) {
        wv_lds_or(cl + (cls - 1u) * 64u + wi, (uint32_t)(bits & TKF_WM));
        if ((bits >> TKF_W) && wi < 63u) wv_lds_or(cl + (cls - 1u) * 64u + wi + 1u, (uint32_t)(bits >> TKF_W));
        if (cls == TK_CLS_N) nmb = true;
    }
}

// multi-byte code points: the lead bytes in `walk` decoded, classed by the trie, ALL bytes of the char marked in the class masks of m
template <int PAT>
TK_DEV void tkf_walk_chars(const TkFlatArgs& a, const TkfGeom& g, TkfClass& m, uint32_t walk) {
    const TkTablesView& t = a.t;
    const int lane = g.lane;
    uint32_t* lds = g.lds;
    uint32_t* cl = lds + TKF_L_CL;
    cl[lane] = 0u; cl[64 + lane] = 0u; cl[128 + lane] = 0u;
    if (PAT) { cl[192 + lane] = 0u; cl[256 + lane] = 0u; cl[320 + lane] = 0u; }   // upper case, Lm | Lo, marks
    if (lane == 0) {
        // the code point of a lead byte in the region's last three bytes ends beyond it: the pad word takes the real bytes
        uint32_t pad = 0u;
        for (int k = 0; k < 4; ++k)
            if (g.r1 + k < g.n) pad |= (uint32_t)a.bytes[g.r1 + k] << (8 * k);
        lds[TKF_L_TXT + TKF_REGION / 4] = pad;
    }
    wv_lds_sync();
    bool nmb = false;
    uint32_t w = walk;
    // Default pattern: the lead bytes are dealt out over ALL lanes -- their positions go into an LDS list (the words of the
    // piece list behind the class words; step 5 builds its list later), one lane per char, 64 chars per round.  The chars
    // the range rules leave over sit in a few lanes (a Thai word, a run of symbols): with every lane walking its own
    // bytes the wave ran as many rounds -- each one a table load and its latency -- as its fullest lane had chars.
    bool dealt = false;
    if (!PAT) {
        uint32_t tot;
        const uint32_t before = tkf_scan_excl((uint32_t)__builtin_popcount(w), lane, &tot);
        if (tot <= TKF_WALKCAP) {
            dealt = true;
            uint16_t* wl = g.list + 2 * TKF_WALKOFF;
            uint32_t ww = w, idx = before;
            while (wv_ballot(ww != 0u)) {
                if (ww) {
                    wl[idx++] = (uint16_t)(TKF_W * lane + __builtin_ctz(ww));
                    ww &= ww - 1u;
                }
            }
            wv_lds_sync();
            for (uint32_t b0 = 0; b0 < tot; b0 += 64u) {
                const uint32_t i = b0 + (uint32_t)lane;
                if (i < tot) {
                    const uint32_t p = wl[i];
                    uint32_t clen;
                    const uint32_t cp = tkf_decode_at(lds, p, &clen);
                    const uint32_t cls = tkf_bmp_class(t, cp, tkf_bmp_word(t, cp));
                    tkf_mark_char<PAT>(cl, p >> TKF_LOGW, p & (TKF_W - 1), clen, cls, 0u, nmb);
                }
            }
        }
    }
    // otherwise (a region with more lead bytes than the list holds; the JSON pattern): every lane walks the lead bytes among its own bytes
    const uint32_t p0 = (uint32_t)TKF_W * (uint32_t)lane;
    while (!dealt && wv_ballot(w != 0u)) {
        if (w) {
            if (PAT) {
                const int i = __builtin_ctz(w);
                w &= w - 1u;
                uint32_t clen;
                const uint32_t cp = tkf_decode_at(lds, p0 + (uint32_t)i, &clen);
                uint32_t cls = TK_CLS_O, extra = 0;
                if (cp != 0xFFFFFFFFu) {
                    // classes of unicode_tables2.h: 1 upper (Lu | Lt), 2 lower, 3 Lm | Lo, 4 mark, 5 N, 6 \s
                    const uint32_t c2 = tk_uc_class2(t, cp);
                    cls = c2 == 1u || c2 == 2u ? TK_CLS_L : c2 == 5u ? TK_CLS_N : c2 == 6u ? TK_CLS_S : TK_CLS_O;
                    extra = c2 == 1u ? 1u : c2 == 3u ? 2u : c2 == 4u ? 3u : 0u;
                }
                tkf_mark_char<PAT>(cl, (uint32_t)lane, (uint32_t)i, clen, cls, extra, nmb);
            } else {
                // two chars per round, their class words requested together (two dependent loads through the two-stage trie, one
                // char at a time, were half of this kernel's time on mixed UTF-8 text)
                const int i0 = __builtin_ctz(w);
                w &= w - 1u;
                const bool two = w != 0u;
                const int i1 = two ? __builtin_ctz(w) : i0;
                w &= w - 1u;                          // (w == 0 stays 0)
                uint32_t l0, l1;
                const uint32_t cp0 = tkf_decode_at(lds, p0 + (uint32_t)i0, &l0), cp1 = tkf_decode_at(lds, p0 + (uint32_t)i1, &l1);
                uint32_t w0 = tkf_bmp_word(t, cp0), w1 = tkf_bmp_word(t, cp1);
                WV_PIN(w0); WV_PIN(w1);
                const uint32_t c0 = tkf_bmp_class(t, cp0, w0), c1 = tkf_bmp_class(t, cp1, w1);
                tkf_mark_char<PAT>(cl, (uint32_t)lane, (uint32_t)i0, l0, c0, 0u, nmb);
                if (two) tkf_mark_char<PAT>(cl, (uint32_t)lane, (uint32_t)i1, l1, c1, 0u, nmb);
            }
        }
    }
    wv_lds_sync();
    m.L |= cl[lane];
    m.N |= cl[64 + lane];
    m.S |= cl[128 + lane];
    m.nmb = wv_ballot(nmb) != 0ull;
    if (PAT) {
        m.UP |= cl[192 + lane];
        m.X = cl[256 + lane];
        m.M = cl[320 + lane];
    }
}

TK_DEV uint32_t tkf_range_mask(int lo, int hi, int lane) {
    return (tkf_lowmask32(hi - TKF_W * lane < 0 ? 0 : hi - TKF_W * lane) & ~tkf_lowmask32(lo - TKF_W * lane < 0 ? 0 : lo - TKF_W * lane)) & TKF_WM;
}
// ---- 5. / 6. helpers: the pieces of a pass before every lane and in all, one scan for both counts (each < 2^16) ----
TK_DEV void tkf_count_pieces(uint32_t PSlist, uint32_t PSown, int lane, TkfPass& ps, uint32_t* pfx_all, uint32_t* pfx_own) {
    uint32_t tot;
    const uint32_t pf = tkf_scan_excl((uint32_t)__builtin_popcount(PSlist) | ((uint32_t)__builtin_popcount(PSown) << 16), lane, &tot);
    *pfx_all = pf & 0xFFFFu; *pfx_own = pf >> 16;
    ps.np_all = tot & 0xFFFFu; ps.np_own = tot >> 16;
}
// the misses of a batch (q: this lane has one) into the chunk's sub-queues by length class, in piece order: ONE scan over four packed 8-bit counters
TK_DEV void tkf_queue_by_class(uint32_t* mq, TkfPass& ps, bool q, uint32_t pos, uint32_t len, uint32_t slot, int lane) {
    const uint32_t cls = (len > 8u ? 1u : 0u) + (len > 16u ? 1u : 0u) + (len > 32u ? 1u : 0u);
    const uint32_t sh = cls * 8u;
    uint32_t ctot;
    const uint32_t before = (tkf_scan_excl(q ? 1u << sh : 0u, lane, &ctot) >> sh) & 0xFFu;
    if (q) {
        const uint32_t qb = cls == 0u ? TKF_MISSOFF0 + ps.nm0 : cls == 1u ? TKF_MISSOFF1 + ps.nm1 : cls == 2u ? TKF_MISSOFF2 + ps.nm2 : TKF_MISSOFF3 + ps.nm3;
        mq[qb + before] = TKF_REC(pos, len, slot);
    }
    ps.nm0 += ctot & 0xFFu;
    ps.nm1 += (ctot >> 8) & 0xFFu;
    ps.nm2 += (ctot >> 16) & 0xFFu;
    ps.nm3 += ctot >> 24;
}
// a batch with a piece of more than 16 bytes (rare): KEY64 up to 64 bytes; beyond, a record or the fall-back mark.  true: the batch held a
// long piece and is finished HERE, in the general forms of the bookkeeping of tk_flat_chunk's batch loop, so that the common path carries
// nothing of it (two more spilled scalars there were 1.5 % of the kernel on C2)
template <int DBG, int PAT, int CUT>
TK_DEV bool tkf_long_pieces(const TkFlatArgs& a, const TkfGeom& g, TkfPass& ps, uint32_t idx, bool act, uint32_t pos, uint32_t len, uint32_t h,
                            const uint32_t* kk, bool frag, uint32_t& r, bool& toolong, uint32_t* tmp, uint32_t* mq) {
    const TkTablesView& t = a.t;
    const int lane = g.lane;
    uint32_t* lds = g.lds;
    uint32_t lres = 0;                              // a long piece that stays on the flat path: id slots reserved for it
    bool lopen = false;
    if (len > 64u) {
        // More than 64 bytes.  Up to TKF_LONGCAP the piece is left to tk_flat_long_kernel (whole-piece lookup, merge)
        // and the document stays here: `len` slots are reserved like for any missed piece.  The chunk's LAST piece
        // may end beyond the region (its length here is only "up to the region end"): it reserves LONGCAP slots and
        // the long kernel finds the end with the sequential matcher -- beyond LONGCAP it flags the document itself.
        lopen = idx + 1u == ps.np_all && ps.sentinel == TKF_REGION && g.r0 + (int64_t)TKF_REGION < (int64_t)a.n_bytes;
        const bool have_ctl = (lds[TKF_L_CONST + 6] | lds[TKF_L_CONST + 7]) != 0u;
        if (!PAT && have_ctl && (lopen || len <= TKF_LONGCAP) && !(CUT && frag && lopen)) lres = lopen ? TKF_LONGCAP : len;
        else toolong = true;                        // (a fragment whose end the region does not show: no cut in 64 bytes)
    } else if (len > 16u && !TKF_ABL(a, 1) && !(CUT && frag)) {
        // 17..64 bytes: KEY64, the piece's dwords from the LDS copy of the region (the polynomial byte hash of LONG,
        // two multiplies and a global load per byte, was 44 % of this kernel on mixed UTF-8 text, whose words are long).
        // First the pre-filter: the hash of (first 16 bytes, length) is at hand, and a clear bit says "no token"
        // without the fold over the piece's dwords and without a probe -- the answer for most long pieces of running text
        r = TK_RANK_MAX;
        const uint32_t pb = tk_k64_prebit(h);
        const uint32_t* pre = reinterpret_cast<const uint32_t*>(t.key64_tab + t.key64_mask + 1u);
        const bool maybe = TKF_ABL(a, 64) || TKF_ABL(a, 128) || ((pre[pb >> 5] >> (pb & 31u)) & 1u) != 0u;
        if (maybe) r = tk_probe_key64(t, lds + TKF_L_TXT + (pos >> 2), pos & 3u, len, kk[0], kk[1], kk[2], kk[3]);
    }
    if (toolong) wv_lds_or(lds + TKF_L_BAD + (pos >> TKF_LOGW), 1u << (pos & (TKF_W - 1)));
    if (wv_ballot(lres != 0u) == 0ull) return false;
    const bool longp = lres != 0u;
    const bool lmiss = r == TK_RANK_MAX && !toolong && !longp && !TKF_ABL(a, 2);
    uint32_t lslot = ps.base_own + idx + ps.E;
    {
        uint32_t tot;
        lslot += tkf_scan_excl(lmiss ? len - 1u : longp ? lres - 1u : 0u, lane, &tot);
        ps.E += tot;
    }
    {
        // (records, capacity and counter through the control words: see TkFlatArgs::long_ctl; ONE atomic for the
        // batch's long pieces -- a counter every long piece of the batch bumps on its own serialises in the L2)
        const uint64_t LB = wv_ballot(longp);
        const int lfirst = tk_ctz64(LB);
        const uint32_t* ctl = reinterpret_cast<const uint32_t*>(wv_global_ptr((uint64_t)lds[TKF_L_CONST + 6] | ((uint64_t)lds[TKF_L_CONST + 7] << 32)));
        uint32_t qbase = 0;
        if (lane == lfirst) qbase = wv_atomic_add(const_cast<uint32_t*>(ctl) + TKC_CTL(TKC_LONG_RECS), (uint32_t)tk_popc64(LB));
        qbase = wv_shfl(qbase, lfirst);
        const uint32_t q = qbase + (uint32_t)tk_popc64(LB & tk_lowmask(lane));
        TkFlatLongRec* recs = reinterpret_cast<TkFlatLongRec*>(const_cast<uint8_t*>(wv_global_ptr((uint64_t)ctl[TKC_CTL(TKC_LONG_CTL)] | ((uint64_t)ctl[TKC_CTL(TKC_LONG_CTL_HI)] << 32))));
        if (!longp) {
        } else if (q < ctl[TKC_CTL(TKC_LONG_CTL_CAP)]) {
            TkFlatLongRec lr;
            lr.pos = (uint64_t)(g.r0 + (int64_t)pos); lr.chunk = (uint32_t)g.c; lr.slot = lslot; lr.len = lopen ? 0u : (CUT && frag ? len | TKF_LREC_FRAG : len); lr.reserved = lres;
            recs[q] = lr;
        } else {                                // no room for the record: the document is handed back after all
            wv_lds_or(lds + TKF_L_BAD + (pos >> TKF_LOGW), 1u << (pos & (TKF_W - 1)));
        }
    }
    if (wv_ballot(lmiss)) tkf_queue_by_class(mq, ps, lmiss, pos, len, lslot, lane);
    wv_lds_sync();                              // positions read before they are overwritten
    if (act) {
        g.list[idx] = (uint16_t)lslot;
        if (!lmiss && !longp && !TKF_ABL(a, 4)) tmp[lslot] = r + a.t.num_special;
    }
    return true;
}
// ---- 7. per-document outputs: slot of every document start, fall-back flags ---------------------
// slot of every document that starts inside the lanes of the pass (and, with want_flags, the hand-back flags)
TK_DEV void tkf_doc_outputs(const TkFlatArgs& a, const TkfGeom& g, const TkfPass& ps, uint64_t fd, bool want_flags, bool anybad) {
    const uint32_t* lds = g.lds;
    // documents that touch the commit range: fd - 1 (the one that contains the region start) onwards
    const uint64_t dfirst = fd > 0 ? fd - 1 : 0;
    const auto& ka = WV_KARGS(TkFlatArgs, a);           // (n_docs, doc_offs, lstart, flags: read here, not kept in scalar registers)
    for (uint64_t base = dfirst;; base += 64) {
        const uint64_t d = base + (uint64_t)g.lane;
        int64_t s = INT64_MAX, e = INT64_MAX;
        if (d < ka.n_docs) {
            s = (int64_t)ka.doc_offs[d];
            e = (int64_t)ka.doc_offs[d + 1];
        }
        const bool in = s < g.c1;
        if (in && s >= g.c0) {
            // id slots of this chunk before the document's first byte (a document start is a piece start)
            const uint32_t p = (uint32_t)(s - g.r0);
            const uint32_t pl = p >> TKF_LOGW;
            if (ps.npass == 1 || (pl >= ps.lane_lo && pl < ps.lane_hi)) {
                const uint32_t pi = tkf_lds_rank(lds + TKF_L_PFX, lds + TKF_L_PS, p);
                ka.lstart[d] = pi < ps.np_own ? g.list[pi] : ps.base_own + ps.np_own + ps.E;
            }
        }
        if (want_flags && anybad && in && e > g.c0) {
            // any bad position inside [s, e) clipped to the region?
            const int64_t lo = s > g.r0 ? s - g.r0 : 0, hi = e < g.r1 ? e - g.r0 : TKF_REGION;
            if (hi > lo) {
                const uint32_t pl = (uint32_t)lo, ph = (uint32_t)hi;
                const uint32_t cl = tkf_lds_rank(lds + TKF_L_BPFX, lds + TKF_L_BAD, pl);
                uint32_t ch;
                if (ph >= TKF_REGION) ch = lds[TKF_L_BPFX + 63] + (uint32_t)__builtin_popcount(lds[TKF_L_BAD + 63]);
                else ch = tkf_lds_rank(lds + TKF_L_BPFX, lds + TKF_L_BAD, ph);
                if (ch > cl) ka.flags[d] = 1u;
            }
        }
        if (wv_ballot(in) != ~0ull) break;
    }
}
// ---- one chunk.  DBG = 1 adds the per-byte piece-start flags of tk_split_batch (and, in a `make ablate` build, the timing ablations):
// every one of those tests costs scalar registers and VALU slots the production kernel (DBG = 0) does not have.  MODE = the key hash the
// tables were built with (TkTablesView::key_hash_mode).  PAT = 1: the JSON pattern of tekken.json (row f-3, opt-in).  CUT = 0: a chunk that
// holds a piece of more than 64 bytes (two neighbouring lanes without a piece start) is appended to a.cut_list and left untouched -- the
// function returns true; CUT = 1 (tk_flat_cut_kernel, over that list): such pieces are cut into FRAGMENTS wherever the vocabulary rules
// out a part that spans the boundary (step 4b); fragments merge on their own, without the whole-piece look-up.  MEMO = 1: the look-up in
// the memo of merged pieces compiled in (step 6); a call that does not use the table runs the MEMO = 0 instantiation, the kernel without
// a single instruction of it (13 M of 326 M VALU wave-instructions per C2 launch, two VGPRs and a spill).
template <int DBG, int MODE, int PAT = 0, int CUT = 0, int MEMO = 1>
TK_DEV bool tk_flat_chunk(const TkFlatArgs& a, uint64_t c, int lane, uint32_t* lds) {
    const TkTablesView& t = a.t;
    const int64_t n = (int64_t)a.n_bytes;
    const int64_t c0 = (int64_t)c * TKF_COMMIT, r0 = c0 - TKF_HL, r1 = r0 + TKF_REGION;
    const int64_t c1 = c0 + TKF_COMMIT < n ? c0 + TKF_COMMIT : n;
    const int ca = TKF_HL, cb = (int)(c1 - r0);  // commit range in region coordinates
    uint16_t* list = reinterpret_cast<uint16_t*>(lds + TKF_L_LIST);
    const TkfGeom g = {c, n, c0, c1, r0, r1, ca, cb, lane, lds, list};

    // ---- 1. load TKF_W bytes per lane, classify ---------------------------------------------------
    uint32_t x[TKF_W / 4];
    for (int k = 0; k < TKF_W / 4; ++k) x[k] = 0u;
    {
        const uint8_t* bytes = WV_KARGS(TkFlatArgs, a).bytes;
        const int64_t g = r0 + TKF_W * lane;
        if (g >= 0 && g + TKF_W <= n) {
            for (int k = 0; k < TKF_W / 16; ++k) wv_load16(bytes + g + 16 * k, x + 4 * k);
        } else if (g + TKF_W > 0 && g < n) {
            for (int k = 0; k < TKF_W; ++k) {
                const int64_t q = g + k;
                if (q >= 0 && q < n) x[k >> 2] |= (uint32_t)bytes[q] << (8 * (k & 3));
            }
        }
    }
    {
        uint32_t* txt = lds + TKF_L_TXT + (TKF_W / 4) * lane;   // bytes outside [0, n) are zero
        for (int k = 0; k < TKF_W / 4; ++k) txt[k] = x[k];
        if (lane == 0) for (int k = 0; k < 4; ++k) lds[TKF_L_TXT + TKF_REGION / 4 + k] = 0u;
    }
    uint32_t nextb = 0;                                     // CUT: the byte behind the region (the last lane's trigram reaches it)
    if (CUT && r1 < n) nextb = (uint32_t)a.bytes[r1];
    TkfClass m = tkf_classify(x);
    uint32_t walk = m.LEAD;                                 // lead bytes the per-char walk has to look up
    if (!PAT && tkf_any(m.F2 | m.F3)) {
        // the chars the range rules cover: letters, all their bytes (a char may reach into the next lane)
        m.L |= m.F2 | m.F3 | tkf_shl(m.F2 | m.F3, 1) | tkf_shl(m.F3, 2);
        walk &= ~(m.F2 | m.F3);
    }
    if (tkf_any(walk)) tkf_walk_chars<PAT>(a, g, m, walk);
    if (TKF_ABL(a, 16)) return tkf_ablated_chunk(a, c, lane, m.L + m.N + m.S + m.NL + m.SP + m.AP + m.HI + m.STMD + m.RV + m.E + m.LL);

    // ---- 2. document starts inside the region -> DS (lane layout, through LDS) ------------------
    lds[TKF_L_DS + lane] = 0u;
    lds[TKF_L_BAD + lane] = 0u;
    wv_lds_sync();
    const uint64_t fd = WV_KARGS(TkFlatArgs, a).first_doc[c];          // documents that start below max(r0, 0)
    bool starts_at_r1 = false;
    {
        // documents d >= fd start at or above the region start; d == n_docs stands for the end of the stream
        const auto& ka = WV_KARGS(TkFlatArgs, a);
        for (uint64_t base = fd;; base += 64) {
            const uint64_t d = base + (uint64_t)lane;
            int64_t s = INT64_MAX;
            if (d <= ka.n_docs) s = (int64_t)ka.doc_offs[d];
            const bool in = s < r1;
            if (in) wv_lds_or(lds + TKF_L_DS + ((s - r0) >> TKF_LOGW), 1u << ((s - r0) & (TKF_W - 1)));
            if (s == r1) starts_at_r1 = true;
            if (wv_ballot(in) != ~0ull) break;
        }
        starts_at_r1 = wv_ballot(starts_at_r1) != 0ull;
    }
    wv_lds_sync();
    const uint32_t DS = lds[TKF_L_DS + lane];

    // ---- 3. piece starts ---------------------------------------------------------------------------
    uint32_t SPR, cont;
    uint32_t PS = PAT ? tkf_rules_json(m, DS, lane, &SPR, &cont) : tkf_rules(m, DS, lane, &SPR, &cont);
    if (TKF_ABL(a, 8)) return tkf_ablated_chunk(a, c, lane, PS + SPR + cont);
    if (!CUT && !PAT) {
        // A piece of more than 64 bytes (surely one of 96 and more, and any piece that begins or goes on beyond this region)
        // leaves two neighbouring lanes of the commit range / right halo without a piece start: the chunk is left to the CUT
        // instantiation.  Both chunks of a piece that crosses a commit boundary decide alike: the one it starts in sees no
        // start in its right halo (lanes 62, 63), the next one none in its first 64 commit bytes (lanes 2, 3).
        const uint64_t Zm = wv_ballot(PS == 0u) & ~(((uint64_t)1 << TKF_NHL) - 1ull);
        if (Zm & (Zm >> 1)) {
            const uint64_t lc = (uint64_t)wv_first(lds[TKF_L_CONST + 6]) | ((uint64_t)wv_first(lds[TKF_L_CONST + 7]) << 32);
            if (lc != 0ull) {
                const uint32_t* ctl = reinterpret_cast<const uint32_t*>(wv_global_ptr(lc));
                const uint64_t lp = (uint64_t)wv_first(ctl[TKC_CTL(TKC_CUT_CTL)]) | ((uint64_t)wv_first(ctl[TKC_CTL(TKC_CUT_CTL_HI)]) << 32);
                if (lp != 0ull) {
                    if (lane == 0) {
                        const uint32_t q = wv_atomic_add(const_cast<uint32_t*>(ctl) + TKC_CTL(TKC_CUT_CHUNKS), 1u);
                        reinterpret_cast<uint32_t*>(const_cast<uint8_t*>(wv_global_ptr(lp)))[q] = (uint32_t)c;
                    }
                    return true;
                }
            }
        }
    }
    // bits of the commit range [ca, cb): whole lanes 2..59 for every chunk but the last one of the stream
    uint32_t commit_mask = (uint32_t)(lane - TKF_NHL) < (uint32_t)(TKF_COMMIT / TKF_W) ? TKF_WM : 0u;
    if (cb != TKF_HL + TKF_COMMIT) commit_mask = tkf_range_mask(ca, cb, lane);
    if (DBG && a.dbg_starts) {
        for (int k = 0; k < TKF_W; ++k)
            if ((commit_mask >> k) & 1u) a.dbg_starts[r0 + TKF_W * lane + k] = (PS >> k) & 1u;
    }

    // ---- 4. positions that make their document fall back ---------------------------------------
    uint32_t BAD = 0;
    {
        // (A) a digit / CR-LF run that comes from below the region and covers the whole left halo
        // (the region may begin inside a code point: its leading continuation bytes have no class and count as part of the run)
        const uint32_t d0 = wv_readlane(DS, 0);
        const uint32_t n0 = wv_readlane(m.N | (m.U8C & ~(m.U8C + 1u)), 0);
        // (the CR / LF run counts the orphan continuation bytes too: whether the char they belong to was punctuation -- the run is
        // then the tail its piece absorbs -- or white space is not known here.  Found by the GPU fuzz in round 4: U+3000, forty CRs,
        // eleven TABs, a region that began inside the U+3000 -> the CRs looked absorbed and a piece began at the first TAB)
        const uint32_t l0 = wv_readlane((PAT ? (m.NL | m.SL) : m.NL) | (m.U8C & ~(m.U8C + 1u)), 0);   // (JSON pattern: the absorbed tail runs through CR / LF / '/')
        const bool covered = n0 == TKF_WM || l0 == TKF_WM;
        if (r0 > 0 && d0 == 0u && covered && lane == TKF_NHL) BAD |= 1u;
        if (PAT) {
            // JSON pattern: two more runs whose state comes from below the region -- a word run (upper or lower side?) and a
            // punctuation / mark run (is the 4th alternative running?) must not cover the whole left halo either
            const uint32_t lead_cont = m.U8C & ~(m.U8C + 1u);
            const uint32_t wd = m.L | m.X | m.M, om = (TKF_WM & ~(m.L | m.X | m.N | m.S));
            // (the tail and the punctuation / mark state feed each other -- a mark behind a tail char is a word char, behind running
            // punctuation it is punctuation, a '/' behind a tail char is tail --, so a CHAIN of tail chars, punctuation and marks that
            // comes from below and covers the halo is as undecidable as a run of one kind.  Found by the model campaign of round 4:
            // "-----" + forty CRs + eleven '/' + thirty-one U+0301 + "'''''", the region beginning inside the CRs)
            bool cov2 = wv_readlane(wd | lead_cont, 0) == TKF_WM || wv_readlane(om | m.NL | m.SL | lead_cont, 0) == TKF_WM;
            if (r0 > 0 && d0 == 0u && cov2 && lane == TKF_NHL) BAD |= 1u;
        }
        // (B) a white-space run that reaches the region end, goes on in the same document and started inside
        //     the commit range
        const uint32_t top = wv_readlane(SPR, 63);
        if (r1 < n && (top & TKF_TOPBIT) && !starts_at_r1) {
            const uint32_t nz = ~cont & TKF_WM;
            const uint64_t NZ = wv_ballot(nz != 0u);
            int f = 0;
            if (NZ) {
                const int tl = tk_msb64(NZ);
                const uint32_t w = wv_readlane(nz, tl);
                f = TKF_W * tl + (31 - __builtin_clz(w));
            }
            if (f < cb) {
                const int at = f > ca ? f : ca;
                if (lane == (at >> TKF_LOGW)) BAD |= 1u << (at & (TKF_W - 1));
            }
        }
    }

    // ---- 4b. CUT instantiation: pieces of more than 64 bytes are cut into fragments -------------------------------
    // (tools/cut_model.py.)  The merge loop joins two parts only if their bytes are a vocabulary key, so a part that spans
    // the boundary between bytes i-1 and i is a key that contains b[i-1] b[i] there: the bigram itself, or a longer key
    // that holds the trigram b[i-2..i] or b[i-1..i+1].  Where the vocabulary has neither (cut_k2: two-byte keys; cut_g3:
    // trigrams inside tokens) no part ever spans the boundary and both sides merge on their own, in their own order:
    // position i becomes a piece start.  A piece with a cut is no key (its n-grams would occur in a token: itself), so its
    // FRAGMENTS skip the whole-piece look-up -- and must: what merging a fragment gives need not be the key it may happen
    // to be.  Which pieces: those of more than 64 bytes that start in the commit range (S64: 64 bytes without a start behind
    // them; that includes a piece whose end this region does not see) and the piece that comes in from the last chunk when
    // it covers the first 64 commit bytes -- exactly when that chunk saw no end of it.  A cut is a pure function of four
    // bytes, so the chunks of a piece agree on every fragment; a chunk owns the fragments that start in its commit range
    // and, when the piece ends in its right halo, those up to that end (the next chunk sees fewer than 64 foreign bytes
    // and leaves them alone).
    uint32_t own_mask = commit_mask;
    uint32_t FS = 0;                                        // cut-only piece starts
    if (CUT) {
        const uint32_t R1 = lane >= TKF_NHL ? (~PS & TKF_WM) : 0u;
        uint32_t F = R1 & tkf_shr(R1, 1);                   // F(i): no start at i .. i + 2^k - 1
        F &= tkf_shr(F, 2);
        F &= tkf_shr(F, 4);
        F &= tkf_shr(F, 8);
        F &= tkf_shr(F, 16);
        F &= wv_up1(F);                                     // ... i + 63 (the bit 32 positions on is the next lane's)
        const uint32_t S64 = PS & commit_mask & tkf_shr(F, 1);
        uint32_t LM = 0;                                    // bytes of the pieces that are cut (behind their first byte)
        if (tkf_any(S64)) LM = tkf_ripple(R1, tkf_shl(S64, 1) & R1);
        // the piece that comes in from the chunk before: up to the first start at or behind the commit start
        const uint32_t f_lo = tkf_first_start(PS, lane, TKF_NHL, TKF_REGION);
        uint32_t LMc = 0;
        if (f_lo >= (uint32_t)ca + 64u) {
            LMc = tkf_range_mask(ca, (int)f_lo, lane);
            LM |= LMc;
        }
        const uint32_t ge_cb = ~tkf_lowmask32(cb - TKF_W * lane < 0 ? 0 : cb - TKF_W * lane);
        const bool closed = tkf_any(PS & ge_cb);            // the piece that crosses the commit end ends inside the region
        // where a cut is wanted: T(j) = the trigram around byte j occurs inside a token, K(j) = bytes j-1, j are a key
        const uint32_t need = LM | tkf_shr(LM, 1);
        uint32_t TG = 0, K2 = 0;
        {
            const uint32_t prevb = wv_dn1(x[TKF_W / 4 - 1]) >> 24;
            uint32_t nb = wv_up1(x[0]) & 0xFFu;
            if (lane == 63) nb = nextb;
            if (need) {
                uint32_t b0 = prevb, b1 = x[0] & 0xFFu;
                for (int k = 0; k < TKF_W; ++k) {
                    const uint32_t b2 = k + 1 < TKF_W ? (x[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 0xFFu : nb;
                    if ((need >> k) & 1u) {
                        const uint32_t i3 = b0 | (b1 << 8) | (b2 << 16), i2 = b0 | (b1 << 8);
                        TG |= ((a.t.cut_g3[i3 >> 5] >> (i3 & 31u)) & 1u) << k;
                        K2 |= ((a.t.cut_k2[i2 >> 5] >> (i2 & 31u)) & 1u) << k;
                    }
                    b0 = b1; b1 = b2;
                }
            }
        }
        FS = LM & ~PS & ~K2 & ~TG & ~tkf_shl(TG, 1);
        // The piece that comes in is taken over only at a cut among the first 64 commit bytes -- the stretch the chunk before
        // sees as well (its right halo).  Without one that chunk saw no end of its last fragment: either it knows of no cut
        // at all and has left the WHOLE piece to a long-piece record (then every byte of it here is foreign, later cuts
        // included), or it has flagged the document.
        if (tkf_any(LMc)) {
            const uint32_t win = ((uint32_t)lane == (uint32_t)TKF_NHL || (uint32_t)lane == (uint32_t)TKF_NHL + 1u) ? TKF_WM : 0u;
            if (!tkf_any(FS & LMc & win)) { FS &= ~LMc; LM &= ~LMc; }
        }
        PS |= FS;
        if (closed) own_mask |= LM & ge_cb;
        lds[TKF_L_FS + lane] = FS;
    }

    // ---- 5. enumerate the pieces: positions of the set bits of PS from the commit start on -------
    // One pass over all lanes when the pieces fit the LDS list (always with 16 bytes per lane; with 32 bytes per lane
    // unless the region averages under two bytes per piece); otherwise two passes, lanes below 32 and lanes from 32 on.
    uint32_t PSown = PS & own_mask;
    uint32_t PSlist = lane >= TKF_NHL ? PS : 0u;            // commit range and right halo (ends of the last pieces)
    TkfPass ps;
    uint32_t pfx_all, pfx_own;
    tkf_count_pieces(PSlist, PSown, lane, ps, &pfx_all, &pfx_own);
    ps.npass = ps.np_all > TKF_MAXPIECES ? 2 : 1;
    uint32_t* tmp = WV_KARGS(TkFlatArgs, a).tmp + c * TKF_STRIDE;
    uint32_t* mq = WV_KARGS(TkFlatArgs, a).miss_list + c * TKF_MISSCAP;
    ps.E = 0; ps.base_own = 0;                              // slots beyond one per piece so far; pieces of the earlier pass
    ps.nm0 = 0; ps.nm1 = 0; ps.nm2 = 0; ps.nm3 = 0;
    ps.lane_lo = TKF_NHL; ps.lane_hi = 64;                  // lanes of the pass
  for (int pass = 0; pass < ps.npass; ++pass) {
    ps.sentinel = TKF_REGION;                               // end of the pass's last piece: the region end ...
    if (ps.npass == 2) {
        ps.lane_lo = pass ? 32 : TKF_NHL;
        ps.lane_hi = pass ? 64 : 32;
        const bool mine = (uint32_t)lane >= ps.lane_lo && (uint32_t)lane < ps.lane_hi;
        PSlist = mine ? PS : 0u;
        PSown = PSlist & own_mask;
        tkf_count_pieces(PSlist, PSown, lane, ps, &pfx_all, &pfx_own);
        if (pass == 0) ps.sentinel = tkf_first_start(PS, lane, 32, TKF_REGION);   // ... or the first piece start of the second pass
    }
    {
        uint32_t w = PSlist, idx = pfx_all;
        while (wv_ballot(w != 0u)) {
            if (w) {
                list[idx++] = (uint16_t)(TKF_W * lane + __builtin_ctz(w));
                w &= w - 1u;
            }
        }
        if (lane == 0) list[ps.np_all] = (uint16_t)ps.sentinel;
    }
    lds[TKF_L_PS + lane] = PSown;
    lds[TKF_L_PFX + lane] = pfx_own;
    wv_lds_sync();

    // ---- 6. whole-piece lookup, one lane per piece; ids stored at once ---------------------------------
    // A piece that misses the vocabulary reserves `len` id slots (it cannot produce more ids than bytes) and is
    // queued for tk_merge_wave; the slots it does not fill stay TKF_HOLE and are squeezed out by the assembly.
    const uint32_t nbatch = (ps.np_own + 63u) / 64u;
    for (uint32_t j = 0; j < nbatch; ++j) {
        // Straight-line for the common case (a piece of up to 16 bytes): every lane fetches bytes and hashes -- a lane
        // without a piece takes position 0, length 1 -- and only the table loads are predicated.
        const uint32_t idx = j * 64u + (uint32_t)lane;
        const bool act = idx < ps.np_own;
        uint32_t pos, len;
        if (j + 1u < nbatch) {
            // every batch but the last one: all 64 lanes own a piece and idx + 1 is inside the list -- no clamping, no selects
            // (a scalar branch; six instructions less per batch)
            const uint32_t p0 = list[idx], p1 = list[idx + 1u];
            pos = p0;
            len = p1 - p0;
        } else {
            const uint32_t p0 = list[idx < ps.np_all ? idx : ps.np_all], p1 = list[idx < ps.np_all ? idx + 1 : ps.np_all];   // (never past the sentinel)
            pos = act ? p0 : 0u;
            len = act ? p1 - p0 : 1u;
        }
        // the piece's first 16 bytes from the LDS copy of the region (five aligned dwords, funnel-shifted), zeroed past the
        // piece (masks by length from LDS)
        uint32_t kk[4];
        {
            const uint32_t* tw = lds + TKF_L_TXT + (pos >> 2);
            const uint32_t t0 = tw[0], t1 = tw[1], t2 = tw[2], t3 = tw[3], t4 = tw[4];
            const uint32_t sh = pos & 3u;
            const uint32_t* km = lds + TKF_L_KM + 4u * (len < 16u ? len : 16u);
            kk[0] = wv_alignbyte(t1, t0, sh) & km[0]; kk[1] = wv_alignbyte(t2, t1, sh) & km[1];
            kk[2] = wv_alignbyte(t3, t2, sh) & km[2]; kk[3] = wv_alignbyte(t4, t3, sh) & km[3];
        }
        uint32_t r = kk[0];                                 // rank of a single byte is the byte (src/tekkenizer.rs:793-798)
        uint32_t h = 0;
        if (TKF_ABL(a, 1)) {
            r = 7u;
        } else if (TKF_ABL(a, 64)) {
            r = (kk[0] ^ kk[1] ^ kk[2] ^ kk[3]) & 0xFFFFu;                                            // timing: no hash, no table
        } else {
            h = tk_key_hash((uint32_t)MODE, kk[0], kk[1], kk[2], kk[3], len);
            if (TKF_ABL(a, 128)) {
                r = h & 0xFFFFu;                                                                      // timing: no table
            } else if (len - 2u <= 14u) {                   // 2..16 bytes: exact-key probe
                const uint32_t* kc = lds + TKF_L_CONST;
                const uint64_t b8 = (uint64_t)kc[2] | ((uint64_t)kc[3] << 32), b16 = (uint64_t)kc[4] | ((uint64_t)kc[5] << 32);
                // (timing only, 512: the probes stay inside the first 1 / 16 of either table -- what the look-up would cost if the tables fitted the L2)
                r = tk_probe_key_h(wv_global_ptr(b8), TKF_ABL(a, 512) ? kc[0] >> 4 : kc[0], wv_global_ptr(b16), TKF_ABL(a, 512) ? kc[1] >> 4 : kc[1],
                                   h, kk[0], kk[1], kk[2], kk[3], len);
            }
        }
        // CUT: a fragment (it begins or ends at a cut) takes no whole-piece look-up: a single byte is its own rank, anything
        // longer goes to the merge queues as it is
        bool frag = false;
        if (CUT) {
            const uint32_t pe = pos + len;
            frag = act && ((((lds[TKF_L_FS + (pos >> TKF_LOGW)] >> (pos & (TKF_W - 1))) & 1u) != 0u) ||
                           (pe < (uint32_t)TKF_REGION && ((lds[TKF_L_FS + (pe >> TKF_LOGW)] >> (pe & (TKF_W - 1))) & 1u) != 0u));
            if (frag && len >= 2u) r = TK_RANK_MAX;
        }
        bool toolong = false;
        if (wv_ballot(len > 16u)) {                         // rare: KEY64; > 64: a record or the fall-back mark (true: the batch is finished)
            if (tkf_long_pieces<DBG, PAT, CUT>(a, g, ps, idx, act, pos, len, h, kk, frag, r, toolong, tmp, mq)) continue;
        }
        // (a lane without a piece holds a byte value in r: never TK_RANK_MAX)
        const bool miss = r == TK_RANK_MAX && !toolong && !TKF_ABL(a, 2);
        uint32_t slot = ps.base_own + idx + ps.E;
        const uint64_t MB = wv_ballot(miss);
        uint32_t res = len;                                 // id slots of a missed piece
        bool mhit = false;
        uint32_t mv0 = 0, mv1 = 0, mv2 = 0, mv4 = 0;        // the entry's rank words; mv4 = its fifth rank (kept across the slot scan: loading
                                                            // the entry again where the ids are stored was a second dependent load, +0.08 ms)
        if (MB) {
            // MEMO (tk_hash.h): a piece of 2..16 bytes that is no vocabulary key may have been merged in an earlier call -- its exact
            // key and the ids the merge gave it sit in a 32-byte entry (two loads, one round trip).  A hit reserves exactly its ids'
            // slots and stores them right here: no queue entry, no holes, nothing for the merge kernel to do.  The entry is a pure
            // function of the bytes (of a fragment's too: fragments take the pure merge), so a hit can never change an id.
            const uint64_t mbase = MEMO ? (uint64_t)wv_first(lds[TKF_L_MEMO + 0]) | ((uint64_t)wv_first(lds[TKF_L_MEMO + 1]) << 32) : 0ull;
            if (MEMO && mbase != 0ull) {
                if (miss && len <= 16u) {
                    const uint32_t ms = tk_memo_slot(h) & lds[TKF_L_MEMO + 2];
                    const tk_u32x4* me = reinterpret_cast<const tk_u32x4*>(wv_global_ptr(mbase) + ((uint64_t)ms << 5));
                    tk_u32x4 ek = me[0], ev = me[1];
                    WV_PIN(ek.x); WV_PIN(ev.x);                 // both loads before the compare
                    if ((((ek.x ^ kk[0]) | (ek.y ^ kk[1]) | (ek.z ^ kk[2]) | (ek.w ^ kk[3])) == 0u) && tk_memo_len(ev.w) == len) {
                        mhit = true;
                        res = tk_memo_n(ev.w);
                        mv0 = ev.y; mv1 = ev.z; mv2 = ev.w; mv4 = ev.x;
                    }
                }
                const uint64_t HB = wv_ballot(mhit);
                if (HB && lane == 0) lds[TKF_L_MEMO + 3] += (uint32_t)tk_popc64(HB);
            }
            // A miss reserves `len` id slots (it cannot produce more ids than bytes): one per piece + (len - 1) more for
            // every miss before it.  The misses are queued in the chunk's own region (no global atomics), records in
            // piece order, one sub-queue per length class (2..8, 9..16, 17..32, 33..64 bytes): the merge kernels run one
            // class per wave.  The two common cases are cheap: ONE miss in the batch (its extra slots shift the lanes
            // behind it: one readlane) and misses of the first class only (rank inside the class = misses before the
            // lane: mbcnt); otherwise a DPP scan of the extra slots and ONE scan over four packed 8-bit counters.
            if ((MB & (MB - 1ull)) == 0ull) {
                const int src = tk_ctz64(MB);
                const uint32_t extra = wv_readlane(res, src) - 1u;
                if (lane > src) slot += extra;
                ps.E += extra;
            } else {
                uint32_t tot;
                slot += tkf_scan_excl(miss ? res - 1u : 0u, lane, &tot);
                ps.E += tot;
            }
            const bool qmiss = MEMO ? miss && !mhit : miss; // what is left for the merge kernels
            const uint64_t QB = wv_ballot(qmiss);
            if (QB == 0ull) {
            } else if (wv_ballot(qmiss && len > 8u) == 0ull) {
                if (qmiss) mq[TKF_MISSOFF0 + ps.nm0 + (uint32_t)tk_popc64(QB & tk_lowmask(lane))] = TKF_REC(pos, len, slot);
                ps.nm0 += (uint32_t)tk_popc64(QB);
            } else {
                tkf_queue_by_class(mq, ps, qmiss, pos, len, slot, lane);
            }
        }
        wv_lds_sync();                                      // positions read before they are overwritten
        if (act) {
            list[idx] = (uint16_t)slot;                     // step 7 looks the slot of a document start up here
            if (!miss && !TKF_ABL(a, 4)) tmp[slot] = r + t.num_special;
        }
        if (MEMO && mhit) {                                 // the ids of the memo entry
            tmp[slot] = tk_memo_id(mv4, mv0, mv1, mv2, 0u) + t.num_special;
            if (res > 1u) tmp[slot + 1u] = tk_memo_id(mv4, mv0, mv1, mv2, 1u) + t.num_special;
            if (res > 2u) tmp[slot + 2u] = tk_memo_id(mv4, mv0, mv1, mv2, 2u) + t.num_special;
            if (res > 3u) tmp[slot + 3u] = tk_memo_id(mv4, mv0, mv1, mv2, 3u) + t.num_special;
            if (res > 4u) tmp[slot + 4u] = tk_memo_id(mv4, mv0, mv1, mv2, 4u) + t.num_special;
        }
    }
    if (pass + 1 < ps.npass) {
        wv_lds_sync();                                      // the slots written by the last batch
        tkf_doc_outputs(a, g, ps, fd, false, false);        // the slots of this pass's documents, while its list is there
        ps.base_own += ps.np_own;
        wv_lds_sync();                                      // the list is rebuilt by the next pass
    }
  }
    if (lane == 0) {
        const auto& ka = WV_KARGS(TkFlatArgs, a);
        ka.kcount[c] = ps.base_own + ps.np_own + ps.E;
        ka.miss_count[c] = ps.nm0;                      // class-major: class k of chunk c at [k * n_chunks + c]
        ka.miss_count[ka.n_chunks + c] = ps.nm1;
        ka.miss_count[2 * ka.n_chunks + c] = ps.nm2;
        ka.miss_count[3 * ka.n_chunks + c] = ps.nm3;
    }

    // ---- 7. per-document outputs: slot of every document start, fall-back flags ---------------------
    BAD |= lds[TKF_L_BAD + lane];                           // piece-level marks of step 6
    const bool anybad = tkf_any(BAD);
    if (anybad) {
        uint32_t nb;
        const uint32_t bp = tkf_scan_excl((uint32_t)__builtin_popcount(BAD), lane, &nb);
        lds[TKF_L_BAD + lane] = BAD;
        lds[TKF_L_BPFX + lane] = bp;
    }
    wv_lds_sync();
    tkf_doc_outputs(a, g, ps, fd, true, anybad);
    wv_lds_sync();  // the next chunk reuses the LDS slice
    return false;
}

#endif
