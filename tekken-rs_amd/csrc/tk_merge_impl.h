// tk_merge_impl.h -- behind the flat kernel (overview: tk_flat_impl.h): the long-piece records, the merge of the queued misses, the memo log
#ifndef TK_MERGE_IMPL_H
#define TK_MERGE_IMPL_H
#include "tk_match.h"
#include "tk_piece_impl.h"
#include "tk_flat_args.h"

// ------------------------------------------------------------------------------------------
// One long-piece record (tk_flat_chunk_impl.h step 6), by one wave: what the per-document kernels would do with this piece, but
// only with this piece -- the rest of its document stays on the flat path.
// ------------------------------------------------------------------------------------------
TK_DEV void tk_flat_long_wave(const TkFlatArgs& a, const TkPolyPow& pw, uint32_t q, int lane, uint32_t* scratch) {
    const TkFlatLongRec lr = a.long_recs[q];
    const uint64_t g = lr.pos;
    // the piece's document: largest d with doc_offs[d] <= g
    uint64_t d = a.first_doc[lr.chunk];
    d = d > 0 ? d - 1 : 0;
    while (d + 1 < a.n_docs && a.doc_offs[d + 1] <= g) ++d;
    d = wv_first64(d);
    if (wv_first(a.flags[d]) != 0u) return;                 // handed back anyway: its slots are never read
    TkEncodeArgs ea;
    ea.bytes = a.bytes; ea.doc_offs = a.doc_offs; ea.n_docs = a.n_docs; ea.staging = nullptr; ea.counts = nullptr;
    ea.work_counter = nullptr; ea.defer_count = nullptr; ea.defer_list = nullptr; ea.todo_list = nullptr; ea.n_todo = 0; ea.n_todo_dev = nullptr;
    ea.scratch = scratch; ea.scratch_words_per_wave = 0; ea.add_bos = 0; ea.add_eos = 0; ea.split_only = 0; ea.pattern = 0; ea.dbg_ablate = 0;
    ea.dbg_starts = nullptr; ea.dbg_mark = nullptr; ea.long_list = nullptr; ea.long_count = nullptr; ea.long_min = 0; ea.long_lazy_mul = 0; ea.long_force = 0;
    ea.long_jobs = nullptr; ea.long_job_count = nullptr; ea.long_job_cap = 0; ea.t = a.t;
    const uint64_t s1 = wv_first64(a.doc_offs[d + 1]);
    const bool frag = (lr.len & TKF_LREC_FRAG) != 0u;       // a fragment of a cut piece: merged as it is, no whole-piece look-up
    const uint32_t rlen = lr.len & ~TKF_LREC_FRAG;
    const uint64_t e = rlen ? g + rlen : wv_first64(tk_match_end(a.t, a.bytes, g, s1));
    const uint32_t len = (uint32_t)(e - g);
    uint32_t* out = a.tmp + (uint64_t)lr.chunk * TKF_STRIDE + lr.slot;
    if (e - g > (uint64_t)lr.reserved) {                    // an open piece of more than LONGCAP bytes: the per-document kernels take the document
        if (lane == 0) {
            // (flagged AFTER the list of the handed-back documents was made -- it is made right behind the flat kernel, beside
            // the merge kernels --: the first record to flag a document puts it on the late list)
            if (a.late_list) {
                if (wv_atomic_exch(a.flags + d, 1u) == 0u) a.late_list[wv_atomic_add(a.late_count, 1u)] = (uint32_t)d;
            } else {
                a.flags[d] = 1u;
            }
        }
        return;
    }
    uint32_t cur = 0;
    const uint32_t r = frag ? TK_RANK_MAX : tk_piece_lookup(ea, pw, lane, g, e);
    if (r != TK_RANK_MAX) {
        if (lane == 0) out[0] = r + a.t.num_special;
        cur = 1;
    } else if (a.long_merge128) {
        // not a vocabulary key: the merge is left to the kernels that do nothing else -- up to 128 bytes one lane per piece
        // (tk_flat_long128_kernel: 64 chains per wave instead of one), beyond that the single-wave merge in a kernel of
        // its own (tk_flat_long_coop_kernel: this one's matcher and lookup cost it half its waves).  The record keeps
        // its length and a mark (no list, no counter: those kernels walk all records).
        if (lane == 0) {
            a.long_recs[q].len = len;
            a.long_recs[q].reserved = lr.reserved | (len <= 128u ? 0x80000000u : 0x40000000u);
        }
        return;
    } else {
        tk_piece_merge_coop(ea, lane, g, e, out, cur, scratch);
    }
    for (uint32_t k = cur + (uint32_t)lane; k < lr.reserved; k += 64u) out[k] = TKF_HOLE;
    if (lane == 0) wv_atomic_add(a.holes + d, lr.reserved - cur);
}

// a record of 129..TKF_LONGCAP bytes that tk_flat_long_wave marked: one wave merges it with the parts in registers
TK_DEV void tk_flat_long_coop_wave(const TkFlatArgs& a, uint32_t q, int lane, uint32_t* scratch) {
    TkFlatLongRec lr = a.long_recs[q];
    if (wv_first(lr.reserved & 0x40000000u) == 0u) return;
    lr.reserved &= 0x3FFFFFFFu;
    const uint64_t g = lr.pos;
    uint64_t d = a.first_doc[lr.chunk];
    d = d > 0 ? d - 1 : 0;
    while (d + 1 < a.n_docs && a.doc_offs[d + 1] <= g) ++d;
    d = wv_first64(d);
    uint32_t* out = a.tmp + (uint64_t)lr.chunk * TKF_STRIDE + lr.slot;
    uint32_t cur = 0;
    (void)scratch;
    tk_piece_merge_small(a.t, a.bytes, lane, g, lr.len, out, cur);   // (<= TKF_LONGCAP = 256 bytes: the parts in registers)
    for (uint32_t k = cur + (uint32_t)lane; k < lr.reserved; k += 64u) out[k] = TKF_HOLE;
    if (lane == 0) wv_atomic_add(a.holes + d, lr.reserved - cur);
}

// ------------------------------------------------------------------------------------------
// tk_merge_wave: byte-pair merge of 64 queued pieces, ONE LANE PER PIECE (tiktoken's _byte_pair_merge,
// repeatedly merge the leftmost minimum-rank adjacent pair).  Every lane runs its own
// chain of dependent PAIR probes, 64 chains per wave and several waves per SIMD hide their latency.
// Pieces of up to 32 bytes keep their parts in LDS columns of the lane's own (tk_merge_lds); the rare longer
// ones (<= 64 bytes) are merged one at a time, one lane per byte, with the segmented-min rounds.
// The ids go to the `len` slots the flat kernel reserved; unused slots become TKF_HOLE and the
// document's hole count is raised so that tk_flat_counts / assemble can squeeze them out.
// ------------------------------------------------------------------------------------------
#define TKM_SHORT 16

// the calling wave's own stretch of the memo log (tk_merge_lds): no counter is shared between waves -- one counter for all of them
// was up to 2 ms of the merge kernel (hundreds of thousands of atomics, and as many look-sees, on one address)
struct TkMemoLog {
    tk_memo_entry* base;   // this wave's records
    uint32_t n, cap;       // records written so far (wave-uniform), room
};
template <bool WIDE>
TK_DEV void tk_merge_items(const TkFlatArgs& a, bool have, uint32_t rec, uint32_t chunk, int lane, uint32_t* mlds, const uint32_t* filt, TkMemoLog* ml = nullptr);

// 64 queued pieces per wave.  The queue counts are laid out class-major ([k * n_chunks + c]); their exclusive prefix
// sums (total at [4 n_chunks]) order all queued pieces by class first, chunk second: item i lives in the sub-queue e
// with prefix[e] <= i < prefix[e + 1].  WIDE = false takes the items of the classes 2..8 / 9..16 bytes, WIDE = true
// those of 17..32 / 33..64 bytes (own kernel: its 32-entry LDS columns would cost the common case occupancy).
// mlds: TKM_LDS_WORDS(32 if WIDE, else 16) words of LDS of the wave's own; filt: the block's LDS copy of the PAIR
// filter (TK_PAIRF_WORDS words, tk_hash.h)
template <bool WIDE>
TK_DEV bool tk_merge_find(const TkFlatArgs& a, uint64_t wave_id, int lane, bool& have_out, uint32_t& rec_out, uint32_t& chunk_out) {
    const uint64_t* prefix = a.miss_prefix;
    const uint64_t n_e = 4 * a.n_chunks;
    // (WIDE takes the class 17..32 bytes; the class 33..64 bytes is merged one piece at a time, one lane per byte: eight
    // pieces per wave, tk_merge_wave_long3 below)
    const uint64_t first = WIDE ? prefix[2 * a.n_chunks] : 0, total = WIDE ? prefix[3 * a.n_chunks] : prefix[2 * a.n_chunks];
    const uint64_t item0 = first + wave_id * 64;
    have_out = false; rec_out = 0u; chunk_out = 0u;
    if (item0 >= total) return false;                 // wave-uniform
    const uint64_t item = item0 + (uint64_t)lane;
    const bool have = item < total;
    uint64_t cl = 0, pcl = 0;                         // the lane's sub-queue and its first item
    {
        // the wave's first sub-queue was written down by tk_merge_wavefirst_kernel (one table for the narrow classes, one
        // for the wide ones); the sub-queues of the 64 items follow from ONE coalesced load of the next 64 prefix sums and
        // a binary search across the lanes (bpermute)
        uint64_t base = (WIDE ? a.wave_first_wide : a.wave_first)[wave_id];        // prefix[base] <= item0
        uint64_t pbase = prefix[base];
        bool done = !have;
        int windows = 0;
        for (;;) {
            const uint64_t idx = base + 1 + (uint64_t)lane;
            const uint64_t pf = idx <= n_e ? prefix[idx] : ~0ull;
            // d = first item of sub-queue idx relative to item0, clamped to 0..65 (non-decreasing over the lanes)
            const uint32_t d = pf <= item0 ? 0u : (pf - item0 > 64 ? 65u : (uint32_t)(pf - item0));
            // cnt = number of lanes j with d_j <= lane: binary lifting over the lanes (bpermute), then the 64th
            uint32_t cnt = 0;
            for (uint32_t step = 32; step >= 1; step >>= 1) {
                const uint32_t dm = wv_shfl(d, (int)(cnt + step - 1u));
                if (dm <= (uint32_t)lane) cnt += step;
            }
            const uint32_t d63 = wv_shfl(d, 63);
            if (cnt == 63u && d63 <= (uint32_t)lane) cnt = 64u;
            const uint32_t dprev = wv_shfl(d, cnt ? (int)cnt - 1 : 0);
            if (!done && cnt < 64u) {
                cl = base + cnt;
                pcl = cnt ? item0 + dprev : pbase;       // (d is exact for every entry <= item0 + 63)
                done = true;
            }
            if (wv_ballot(!done) == 0ull) break;
            // all 64 sub-queues start at or below some lane's item (sparse queues: on the Zipf shape 64 wide items span
            // ~10^5 sub-queues, and walking them 64 at a time was 1.9 ms of one wave): two more windows, then every
            // lane left over searches the rest of its class by bisection (~20 dependent loads)
            pbase = ((uint64_t)wv_shfl((uint32_t)(pf >> 32), 63) << 32) | wv_shfl((uint32_t)pf, 63);
            base += 64;
            if (++windows < 3) continue;
            if (!done) {
                uint64_t lo = base, hi = WIDE ? 3 * a.n_chunks : 2 * a.n_chunks;      // prefix[lo] <= item < prefix[hi]
                while (hi - lo > 1) {
                    const uint64_t mid = (lo + hi) / 2;
                    if (prefix[mid] <= item) lo = mid; else hi = mid;
                }
                cl = lo;
                pcl = prefix[lo];
                done = true;
            }
            break;
        }
    }
    uint32_t rec = 0;
    uint64_t chunk = 0;
    if (have) {
        const uint64_t k = cl / a.n_chunks;
        chunk = cl - k * a.n_chunks;
        const uint32_t off = k == 0 ? TKF_MISSOFF0 : k == 1 ? TKF_MISSOFF1 : k == 2 ? TKF_MISSOFF2 : TKF_MISSOFF3;
        rec = a.miss_list[chunk * TKF_MISSCAP + off + (item - pcl)];
    }
    have_out = have; rec_out = rec; chunk_out = (uint32_t)chunk;
    return true;
}
template <bool WIDE>
TK_DEV void tk_merge_wave(const TkFlatArgs& a, uint64_t wave_id, int lane, uint32_t* mlds, const uint32_t* filt, TkMemoLog* ml = nullptr) {
    bool have; uint32_t rec, chunk;
    if (!tk_merge_find<WIDE>(a, wave_id, lane, have, rec, chunk)) return;
    tk_merge_items<WIDE>(a, have, rec, chunk, lane, mlds, filt, ml);
}

// The class 33..64 bytes: 64 pieces per wave, one lane each, in 64-entry LDS columns (tk_merge_lds<64>: 32 KB per wave, so
// every second wave of the wide kernel takes these, with its neighbour's columns).  The first form merged such a piece
// with the whole wave, one lane per byte, eight pieces per wave one after the other: fine while the class is rare, but
// text whose pieces are long by nature (CJK: a run of ideographs between two punctuation marks is ONE \p{L}+ piece of
// 3 bytes per character) puts most of its bytes here.  The lane's sub-queue by bisection over the class's prefix sums.
TK_DEV void tk_merge_items64(const TkFlatArgs& a, bool have, uint32_t rec, uint32_t chunk, int lane, uint32_t* mlds, const uint32_t* filt);
TK_DEV void tk_merge_wave_long3(const TkFlatArgs& a, uint64_t wave_id, int lane, uint32_t* mlds, const uint32_t* filt) {
    const uint64_t* prefix = a.miss_prefix;
    const uint64_t e0 = 3 * a.n_chunks, e1 = 4 * a.n_chunks;
    const uint64_t first = prefix[e0], total = prefix[e1];
    const uint64_t item0 = first + wave_id * 64;
    if (item0 >= total) return;                       // wave-uniform
    const uint64_t item = item0 + (uint64_t)lane;
    const bool have = item < total;
    uint32_t rec = 0;
    uint64_t chunk = 0;
    if (have) {
        uint64_t lo = e0, hi = e1;                    // prefix[lo] <= item < prefix[hi]
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) / 2;
            if (prefix[mid] <= item) lo = mid; else hi = mid;
        }
        chunk = lo - e0;
        rec = a.miss_list[chunk * TKF_MISSCAP + TKF_MISSOFF3 + (item - prefix[lo])];
    }
    tk_merge_items64(a, have, rec, (uint32_t)chunk, lane, mlds, filt);
}

// sequential merge of one piece of up to N bytes per lane (N = 8, 16, 32), parts in LDS: lane l owns column l of an
// N x 64 word array of KEYS and an N / 4 x 64 word array holding the piece's BYTES (word i * 64 + l, so whatever positions
// the lanes index, a wave's access is free of bank conflicts, and no lane ever touches another one's words: no barrier).
// Parts never move: bit i of `alive` says that a part starts at byte i and key[i] = (rank of the pair (part i, its
// successor) << PB) | i, or all ones -- so the leftmost smallest rank is one unsigned minimum over the column (v_min3: half
// an instruction per entry), and a merge is a handful of bit operations and a few LDS accesses.  The ID of a part needs no
// column of its own: a part of one byte is that byte, and a part of several bytes has a dead position right behind its first
// one -- key[i + 1], which no minimum may pick any more, holds 0x80000000 | id (anything from 0x80000000 up loses against
// every key; ids are below 2^21).  5 N bytes of LDS per lane instead of 8 N: the columns of a wave are what bounds the
// waves per CU of the merge kernels, and the waves are what hides their chains of dependent PAIR probes.  This COMPACT
// layout costs ~10 % more instructions per merge: it is used from 32-entry columns on (TKM_COMPACT), where it buys waves --
// tk_merge_wide_kernel runs 16 waves per CU (no PAIR filter in its LDS either) where it ran 8; the narrow classes keep a
// column of ids of their own (their block of 16 waves is the largest there is, and with twice the waves and no filter the
// kernel is slower: 2.76 against 2.49 ms on the mixed shape -- it is bound by its gathers, not by their latency).  (Parts in N-wide
// register arrays, shifted by predication -- the first form of this -- cost ~3x (N = 16) to ~4x (N = 32) the VALU issues
// per merge and 95 / 153 VGPRs.)
#ifndef TKM_COMPACT_MIN
#define TKM_COMPACT_MIN 32
#endif
#define TKM_COMPACT(N) ((N) >= TKM_COMPACT_MIN)           /* the classes whose waves per CU are bounded by their columns */
#define TKM_LDS_WORDS(N) (TKM_COMPACT(N) ? ((N) + (N) / 4) * 64 : 2 * (N) * 64)
#ifdef TKM_ABLATE   /* timing-only experiments on the merge kernels (never defined in the shipped build) */
#define TKM_AB(a, bit) (((a).dbg_ablate & (bit)) != 0)
#else
#define TKM_AB(a, bit) false
#endif
template <int N> struct TkmAlive { typedef uint32_t type; };
template <> struct TkmAlive<64> { typedef uint64_t type; };
template <> struct TkmAlive<128> { typedef unsigned __int128 type; };
// mask helpers: the low n bits (n up to the width), one bit, any bit set, lowest set bit cleared (the type is chosen by
// a null pointer argument)
template <typename T> TK_DEV T tkm_low(uint32_t n, const T*) { return n >= 8u * (uint32_t)sizeof(T) ? (T)~(T)0 : (T)(((T)1 << n) - (T)1); }
template <typename T> TK_DEV T tkm_bit(uint32_t n, const T*) { return (T)((T)1 << n); }
template <typename T> TK_DEV bool tkm_any(T v) { return v != (T)0; }
template <typename T> TK_DEV T tkm_clear_lowest(T v) { return (T)(v & (v - (T)1)); }
TK_DEV uint32_t tkm_ctz(uint32_t v) { return (uint32_t)__builtin_ctz(v); }
TK_DEV uint32_t tkm_ctz(uint64_t v) { return (uint32_t)__builtin_ctzll(v); }
TK_DEV uint32_t tkm_msb(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }
TK_DEV uint32_t tkm_msb(uint64_t v) { return 63u - (uint32_t)__builtin_clzll(v); }
TK_DEV uint32_t tkm_popc(uint32_t v) { return (uint32_t)__builtin_popcount(v); }
TK_DEV uint32_t tkm_popc(uint64_t v) { return (uint32_t)__builtin_popcountll(v); }
TK_DEV uint32_t tkm_ctz(unsigned __int128 v) { const uint64_t lo = (uint64_t)v; return lo ? (uint32_t)__builtin_ctzll(lo) : 64u + (uint32_t)__builtin_ctzll((uint64_t)(v >> 64)); }
TK_DEV uint32_t tkm_msb(unsigned __int128 v) { const uint64_t hi = (uint64_t)(v >> 64); return hi ? 127u - (uint32_t)__builtin_clzll(hi) : 63u - (uint32_t)__builtin_clzll((uint64_t)v); }
TK_DEV uint32_t tkm_popc(unsigned __int128 v) { return (uint32_t)__builtin_popcountll((uint64_t)v) + (uint32_t)__builtin_popcountll((uint64_t)(v >> 64)); }

// N = 8, 16, 32, 64, 128 (64: the class 33..64 bytes, keys carry six position bits and the live mask is 64 bits wide;
// 128: the long-piece records of 65..128 bytes, seven position bits, a 128-bit mask)
template <int N>
TK_DEV uint32_t tk_merge_lds(const TkFlatArgs& a, const uint32_t* filt, bool mine, const uint32_t* kk, uint32_t len,
                             uint32_t* out, uint32_t* mlds, int lane, TkMemoLog* ml = nullptr) {
    typedef typename TkmAlive<N>::type alive_t;
    constexpr uint32_t PB = N > 64 ? 7u : N > 32 ? 6u : 5u, PM = (1u << PB) - 1u;
    constexpr uint32_t DEAD = 0x80000000u;                  // key[i] >= DEAD: no pair starts at i (all ones), or the id of the part that begins at i - 1
    const TkTablesView& t = a.t;
    constexpr bool C = TKM_COMPACT(N);
    // compact: keys, then the piece's bytes; otherwise ids, then keys (a column of ids of its own: fewer instructions per merge,
    // kept where the block cannot hold more waves anyway)
    uint32_t* keyc = C ? mlds + lane : mlds + N * 64 + lane;
    uint32_t* bytc = mlds + N * 64 + lane;
    uint32_t* tokc = mlds + lane;
    const uint32_t n = mine ? len : 0u;
    if (C) {
#pragma unroll
        for (int q = 0; q < N / 4; ++q) bytc[q * 64] = kk[q];
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const uint32_t b = (kk[i >> 2] >> (8 * (i & 3))) & 0xFFu;
        const uint32_t b1 = i + 1 < N ? (kk[(i + 1) >> 2] >> (8 * ((i + 1) & 3))) & 0xFFu : 0u;
        uint32_t key = 0xFFFFFFFFu;
        if ((uint32_t)(i + 1) < n && !TKM_AB(a, 2048)) {
            const uint32_t r = t.pair2[b | (b1 << 8)];
            if (r != TK_RANK_MAX) key = (r << PB) | (uint32_t)i;
        }
        if (!C) tokc[i * 64] = b;
        keyc[i * 64] = key;
    }
    alive_t alive = tkm_low(n, (const alive_t*)nullptr);
    // id of the live part at position x (see above)
    auto tok_at = [&](uint32_t x, alive_t al) -> uint32_t {
        if (!C) return tokc[x * 64u];
        const bool multi = x + 1u < n && !tkm_any((alive_t)(al & tkm_bit(x + 1u < (uint32_t)N ? x + 1u : 0u, (const alive_t*)nullptr)));
        const uint32_t v = multi ? keyc[(x + 1u) * 64u] : bytc[(x >> 2) * 64u];
        return multi ? v & ~DEAD : (v >> (8u * (x & 3u))) & 0xFFu;
    };
    bool active = mine && !TKM_AB(a, 1024);
    while (wv_ballot(active)) {
        if (active) {
            uint32_t best = 0xFFFFFFFFu;
#pragma unroll
            for (int i = 0; i < N - 1; ++i) {
                const uint32_t k = keyc[i * 64];
                best = k < best ? k : best;
            }
            if (best >= DEAD) {
                active = false;
            } else {
                // the parts at bi and at the next live position j become one part (at bi) whose id is the rank
                const uint32_t bi = best & PM, rank = best >> PB;
                const alive_t above = alive & ~tkm_low(bi + 1u, (const alive_t*)nullptr);       // bi <= N - 2
                const uint32_t j = tkm_ctz(above);                            // exists: key[bi] was a pair
                const alive_t above2 = tkm_clear_lowest(above);
                const alive_t below = alive & tkm_low(bi, (const alive_t*)nullptr);
                const bool has_next = tkm_any(above2), has_prev = tkm_any(below);
                const uint32_t k = has_next ? tkm_ctz(above2) : 0u;
                const uint32_t p = has_prev ? tkm_msb(below) : 0u;
                const uint32_t tn = tok_at(k, alive), tp = tok_at(p, alive);   // (neither lives in a word written below: p + 1 <= bi, k + 1 > j)
                alive = alive & ~tkm_bit(j, (const alive_t*)nullptr);
                keyc[j * 64] = 0xFFFFFFFFu;                                   // j's own pair is gone ...
                if (C) keyc[(bi + 1u) * 64] = DEAD | rank;                    // ... and the word behind bi (dead: j or an older one) takes the new id
                else tokc[bi * 64] = rank;
                uint32_t r_next = TK_RANK_MAX, r_prev = TK_RANK_MAX;
                tk_probe_pair_x2f(t, filt, has_next, rank, tn, has_prev, tp, rank, r_next, r_prev);
                keyc[bi * 64] = r_next == TK_RANK_MAX ? 0xFFFFFFFFu : ((r_next << PB) | bi);
                if (has_prev) keyc[p * 64] = r_prev == TK_RANK_MAX ? 0xFFFFFFFFu : ((r_prev << PB) | p);
            }
        }
    }
    const uint32_t np = tkm_popc(alive);
    if (!C && ml != nullptr) {
        // MEMO (tk_hash.h): what this piece merged into, for the look-ups of the NEXT call -- exact key (the bytes, zero padded,
        // and the length), at most TK_MEMO_MAXIDS ranks.  The entry goes into this wave's stretch of a LOG (a full stretch drops
        // it, which only delays the entry by a call); tk_memo_commit_kernel puts the log into the table behind the merge kernels
        // -- a hot new word arrives in hundreds of lanes at once, and taking table slots with atomics from here would serialise
        // them.
        bool ins = mine && np <= TK_MEMO_MAXIDS;
        uint32_t k[4] = {0u, 0u, 0u, 0u};
        tk_memo_entry* slot = nullptr;
        if (wv_ballot(ins) && ml->n < ml->cap) {
            if (ins) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int keep = (int)len - 4 * q;
                    k[q] = (q < N / 4 && keep > 0) ? (kk[q < N / 4 ? q : 0] & (keep >= 4 ? 0xFFFFFFFFu : ((1u << (8 * keep)) - 1u))) : 0u;
                }
                slot = a.memo_tab + (tk_memo_slot(tk_key_hash(t.key_hash_mode, k[0], k[1], k[2], k[3], len)) & a.memo_mask);
                // a slot that already carries a claim of THIS call (a record index: no tag bit; the commit kernel leaves every claimed
                // slot tagged) is most often the same word merged somewhere else a moment ago -- a new word comes in hundreds of lanes:
                // no second record for it (a colliding word waits a call).  The load may be stale: then there is a duplicate, as before.
                // Only on the call that fills an empty table (no look-ups yet: EVERY merged piece comes here, and the hot words would fill
                // the log with copies of themselves -- with the check the second batch already runs warm, 2.32 -> 1.54 ms); later calls
                // log only what the table missed, and the extra gather would cost them 2 %.
                if (a.memo_probe == 0u) {
                    const uint32_t cw = slot->w4;
                    if (cw != 0u && (cw & TK_MEMO_TAG) == 0u) ins = false;
                }
            }
        }
        const uint64_t IB = wv_ballot(ins);
        if (IB && ml->n < ml->cap) {
            const uint32_t at = ml->n + (uint32_t)tk_popc64(IB & tk_lowmask(lane));
            if (ins && at < ml->cap) {
                uint32_t r5[5] = {0u, 0u, 0u, 0u, 0u};
                alive_t rem = alive;
#pragma unroll
                for (int q = 0; q < 5; ++q) {
                    if ((uint32_t)q < np) r5[q] = tokc[tkm_ctz(rem) * 64u];
                    rem = tkm_clear_lowest(rem);
                }
                uint32_t v[3], w4;
                tk_memo_pack(r5, np, len, &w4, v);
                tk_memo_entry* w = ml->base + at;           // (a log record is the entry it will become)
                wv_store16(w->k, k[0], k[1], k[2], k[3]);
                wv_store16(&w->w4, w4, v[0], v[1], v[2]);
                // ... and CLAIMS its slot: the record's index into the slot's claim word, a plain store -- of all the records that want
                // a slot in this call one index stays, and tk_memo_commit_kernel lets that record write (nothing reads the table
                // while the merge and commit kernels run)
                slot->w4 = (uint32_t)(w - a.memo_log);
            }
            const uint32_t nn = ml->n + (uint32_t)tk_popc64(IB);
            ml->n = nn < ml->cap ? nn : ml->cap;
        }
    }
    if (mine && !TKM_AB(a, 256)) {
        // the piece's `len` slots: its np ids, then holes -- gathered into registers and stored four at a time (the cost
        // of a scattered store is per lane and instruction, not per byte), single words only for the last len % 4
        alive_t rem = alive;
#pragma unroll
        for (int q0 = 0; q0 < N; q0 += 4) {
            uint32_t v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t pos = tkm_any(rem) ? tkm_ctz(rem) : 0u;
                const uint32_t id = tok_at(pos, alive) + t.num_special;
                v[q] = (uint32_t)(q0 + q) < np ? id : TKF_HOLE;
                rem = tkm_clear_lowest(rem);
            }
            if ((uint32_t)q0 + 4u <= len) {
                wv_store16(out + q0, v[0], v[1], v[2], v[3]);
            } else {
                if ((uint32_t)q0 < len) out[q0] = v[0];
                if ((uint32_t)q0 + 1u < len) out[q0 + 1] = v[1];
                if ((uint32_t)q0 + 2u < len) out[q0 + 2] = v[2];
            }
        }
    }
    return mine ? len - np : 0u;
}

// the document of a merged piece loses `holes` ids.  Queued pieces are in text order inside a sub-queue, so neighbouring
// lanes mostly share their document: the counts of a run of lanes with the same document are summed in the wave (one
// scan) and its last lane does the one atomic -- 64 atomics on two or three addresses serialise in the L2.
TK_DEV void tk_merge_holes(const TkFlatArgs& a, bool have, uint32_t holes, uint32_t chunk, int64_t g, int lane) {
    if (wv_ballot(have && holes != 0u) && !TKM_AB(a, 512)) {
        // largest d with doc_offs[d] <= g: the documents from first_doc[chunk] - 1 on start at or above the region
        uint64_t d = 0;
        if (have) {
            d = a.first_doc[chunk];
            d = d > 0 ? d - 1 : 0;
            // four offsets per round trip (one at a time this was a chain of up to four dependent loads per lane on 512-byte
            // documents -- a tenth of the merge kernel there); doc_offs[n_docs] = n_bytes > g ends the search by itself
            for (;;) {
                const uint64_t i1 = d + 1 < a.n_docs ? d + 1 : a.n_docs, i2 = d + 2 < a.n_docs ? d + 2 : a.n_docs;
                const uint64_t i3 = d + 3 < a.n_docs ? d + 3 : a.n_docs, i4 = d + 4 < a.n_docs ? d + 4 : a.n_docs;
                uint64_t o1 = a.doc_offs[i1], o2 = a.doc_offs[i2], o3 = a.doc_offs[i3], o4 = a.doc_offs[i4];
                const uint32_t cnt = ((int64_t)o1 <= g ? 1u : 0u) + ((int64_t)o2 <= g ? 1u : 0u) + ((int64_t)o3 <= g ? 1u : 0u) + ((int64_t)o4 <= g ? 1u : 0u);
                d += cnt;                                   // (the offsets do not decrease: the count is the number of steps)
                if (cnt < 4u) break;
            }
        }
        const uint32_t key = have ? (uint32_t)d : 0xFFFFFFFFu;             // (documents are numbered below 2^32 - 1)
        const uint32_t kprev = wv_shfl(key, lane > 0 ? lane - 1 : 0), knext = wv_shfl(key, lane < 63 ? lane + 1 : 63);
        const bool head = lane == 0 || kprev != key, tail = lane == 63 || knext != key;
        const uint64_t HEADS = wv_ballot(head);
        const uint32_t P = wv_scan_incl_u32(have ? holes : 0u);
        const int start = tk_msb64(HEADS & (tk_lowmask(lane) | (1ull << lane)));      // the head of this lane's run
        const uint32_t before = wv_shfl(P, start > 0 ? start - 1 : 0);
        const uint32_t sum = P - (start > 0 ? before : 0u);
        if (have && tail && sum) wv_atomic_add(a.holes + d, sum);
    }
}

// the piece's bytes, zero padded to N: N / 16 wide loads, byte by byte at the end of the stream
template <int N>
TK_DEV void tkm_load_piece(const TkFlatArgs& a, bool have, int64_t g, uint32_t len, uint32_t* kk) {
    for (int q = 0; q < N / 4; ++q) kk[q] = 0u;
    if (have && g + N <= (int64_t)a.n_bytes) {
#pragma unroll
        for (int q = 0; q < N / 16; ++q) wv_load16(a.bytes + g + 16 * q, kk + 4 * q);
    } else if (have) {
        for (uint32_t q = 0; q < len; ++q) kk[q >> 2] |= (uint32_t)a.bytes[g + q] << (8 * (q & 3));
    }
}
// the class 33..64 bytes, one lane per piece like the shorter classes: 64-entry columns (32 KB of LDS per wave)
TK_DEV void tk_merge_items64(const TkFlatArgs& a, bool have, uint32_t rec, uint32_t chunk, int lane, uint32_t* mlds, const uint32_t* filt) {
    const uint32_t pos = TKF_REC_POS(rec), len = TKF_REC_LEN(rec), slot = TKF_REC_SLOT(rec);
    const int64_t g = (int64_t)chunk * TKF_COMMIT - TKF_HL + (int64_t)pos;   // first byte of the piece
    uint32_t* out = a.tmp + (uint64_t)chunk * TKF_STRIDE + slot;
    uint32_t kk[16];
    tkm_load_piece<64>(a, have, g, len, kk);
    uint32_t holes = 0;
    if (wv_ballot(have)) holes = tk_merge_lds<64>(a, filt, have, kk, len, out, mlds, lane);
    tk_merge_holes(a, have, holes, chunk, g, lane);
}

// the long-piece records that are no vocabulary keys (marked by tk_flat_long_wave): 64 consecutive records per wave, one
// lane each, in N-entry LDS columns -- N = 128 for 65..128 bytes (64 KB per wave: two waves and the PAIR filter fill a CU's
// LDS) -- still 128 chains per CU where the single-wave merge runs a dozen
template <int N>
TK_DEV void tk_merge_long_wave(const TkFlatArgs& a, uint64_t wave_id, int lane, uint32_t* mlds, const uint32_t* filt) {
    const uint64_t n = *a.long_count < a.long_cap ? *a.long_count : a.long_cap;
    const uint64_t item = wave_id * 64 + (uint64_t)lane;
    if (wave_id * 64 >= n) return;                    // wave-uniform
    TkFlatLongRec lr;
    lr.pos = 0; lr.chunk = 0; lr.slot = 0; lr.len = 0; lr.reserved = 0;
    if (item < n) lr = a.long_recs[item];
    // marked by tk_flat_long_wave, and of this kernel's length class
    const bool have = (lr.reserved & 0x80000000u) != 0u && lr.len <= (uint32_t)N && lr.len > (uint32_t)N / 2u;
    lr.reserved &= 0x3FFFFFFFu;
    if (wv_ballot(have) == 0ull) return;
    const int64_t g = (int64_t)lr.pos;
    uint32_t* out = a.tmp + (uint64_t)lr.chunk * TKF_STRIDE + lr.slot;
    uint32_t kk[N / 4];
    tkm_load_piece<N>(a, have, g, lr.len, kk);
    uint32_t holes = tk_merge_lds<N>(a, filt, have, kk, lr.len, out, mlds, lane);
    if (have) {
        // (a piece whose end the chunk did not see reserved TKF_LONGCAP slots: the rest are holes too)
        for (uint32_t k = lr.len; k < lr.reserved; ++k) out[k] = TKF_HOLE;
        holes += lr.reserved - lr.len;
    }
    tk_merge_holes(a, have, holes, lr.chunk, g, lane);
}

template <bool WIDE>
TK_DEV void tk_merge_items(const TkFlatArgs& a, bool have, uint32_t rec, uint32_t chunk, int lane, uint32_t* mlds, const uint32_t* filt, TkMemoLog* ml) {
    const TkTablesView& t = a.t;
    const uint32_t pos = TKF_REC_POS(rec), len = TKF_REC_LEN(rec), slot = TKF_REC_SLOT(rec);
    const int64_t g = (int64_t)chunk * TKF_COMMIT - TKF_HL + (int64_t)pos;   // first byte of the piece
    uint32_t* out = a.tmp + (uint64_t)chunk * TKF_STRIDE + slot;
    uint32_t holes = 0;

    // ---- pieces of up to 32 bytes: one lane each, parts in LDS columns (8 / 16 / 32 entries by class) ------
    {
        const uint32_t cap = WIDE ? 32u : TKM_SHORT;
        const bool inregs = have && len <= cap;
        uint32_t kk[WIDE ? 8 : 4];
        for (int q = 0; q < (WIDE ? 8 : 4); ++q) kk[q] = 0u;
        if (inregs) {
            if (g + (int64_t)cap <= (int64_t)a.n_bytes) {
                wv_load16(a.bytes + g, kk);
                if (WIDE) wv_load16(a.bytes + g + 16, kk + 4);
            } else {
                for (uint32_t q = 0; q < len; ++q) kk[q >> 2] |= (uint32_t)a.bytes[g + q] << (8 * (q & 3));
            }
        }
        if (!WIDE) {
            const bool s8 = inregs && len <= 8u, s16 = inregs && len > 8u;
            if (wv_ballot(s8)) holes += tk_merge_lds<8>(a, filt, s8, kk, len, out, mlds, lane, ml);
            if (wv_ballot(s16)) holes += tk_merge_lds<16>(a, filt, s16, kk, len, out, mlds, lane, ml);
        } else {
            if (wv_ballot(inregs)) holes += tk_merge_lds<32>(a, filt, inregs, kk, len, out, mlds, lane);
        }
    }

    // ---- longer pieces (33..64 bytes; 17..64 if they ever reach the narrow kernel): one at a time, one lane per byte
    uint64_t LONGM = wv_ballot(have && len > (WIDE ? 32u : TKM_SHORT));
    while (LONGM) {
        const int src = tk_ctz64(LONGM);
        LONGM &= LONGM - 1ull;
        const uint32_t plen = wv_shfl(len, src);
        const uint32_t glo = wv_shfl((uint32_t)g, src), ghi = wv_shfl((uint32_t)((uint64_t)g >> 32), src);
        const int64_t pg = (int64_t)(((uint64_t)ghi << 32) | glo);
        const uint32_t pchunk = wv_shfl(chunk, src), pslot = wv_shfl(slot, src);
        uint32_t* pout = a.tmp + (uint64_t)pchunk * TKF_STRIDE + pslot;
        const int pe = (int)plen;
        const bool inmiss = lane < pe;
        const uint32_t b0 = inmiss ? (uint32_t)a.bytes[pg + lane] : 0u;
        const uint32_t b1 = wv_up1(b0);
        uint64_t A = wv_ballot(inmiss);
        uint32_t tok = b0;
        uint32_t prank = TK_RANK_MAX;
        if (inmiss && lane + 1 < pe) prank = t.pair2[b0 | (b1 << 8)];
        for (int round = 0; round < 64; ++round) {
            const uint32_t key = prank == TK_RANK_MAX ? 0xFFFFFFFFu : ((prank << 6) | (uint32_t)lane);
            const uint32_t segmin = wv_min_u32(key);
            if (segmin == 0xFFFFFFFFu) break;
            const bool winner = key == segmin;
            const uint64_t Wm = wv_ballot(winner);
            const bool alive = tk_bit(A, lane);
            const uint64_t below = A & tk_lowmask(lane);
            const bool dead = alive && below && tk_bit(Wm, tk_msb64(below));
            const uint64_t Dm = wv_ballot(dead);
            A &= ~Dm;
            if (winner) tok = prank;
            if (dead) prank = TK_RANK_MAX;
            const uint64_t z = lane < 63 ? (A >> (lane + 1)) : 0ull;
            const int na = z ? lane + 1 + tk_ctz64(z) : 64;
            const bool has_next = na < pe;
            const uint32_t tn = wv_shfl(tok, na < 64 ? na : lane);
            const bool need = tk_bit(A, lane) && (winner || (has_next && tk_bit(Wm, na)));
            if (need) prank = has_next ? tk_probe_pair_f(t, filt, tok, tn) : TK_RANK_MAX;
        }
        const uint32_t k = (uint32_t)tk_popc64(A);
        if (inmiss && tk_bit(A, lane)) pout[tk_popc64(A & tk_lowmask(lane))] = tok + t.num_special;
        if (inmiss && (uint32_t)lane >= k) pout[lane] = TKF_HOLE;
        if (lane == src) holes = plen - k;
    }

    tk_merge_holes(a, have, holes, chunk, g, lane);
}

// The log of a call's new entries (tk_merge_lds) into the table, without a single atomic -- a word that is new in this call is new in
// hundreds of records, and that many read-modify-writes on one address serialise (measured: up to 1.4 ms for a million records).
// Record i = j-th record of merge wave w, i = w * per_wave + j, j < counts[w].  Step 1, in the merge kernel where the record is
// written: its INDEX goes into the claim word (w4) of its slot (plain stores: one of them stays).  Step 2, tk_memo_commit_kernel behind
// the merge kernels: the record whose index is the one that stayed owns the slot and writes key and ids.  One writer per slot and call
// by construction; nothing reads the table while the merge and commit kernels run.
TK_DEV bool tk_memo_log_live(const uint32_t* counts, uint32_t per_wave, uint32_t i) { return i % per_wave < counts[i / per_wave]; }
TK_DEV uint32_t tk_memo_slot_of(const tk_memo_entry& r, uint32_t key_hash_mode, uint32_t mask) {
    return tk_memo_slot(tk_key_hash(key_hash_mode, r.k[0], r.k[1], r.k[2], r.k[3], tk_memo_len(r.v[2]))) & mask;
}
TK_DEV void tk_memo_commit_one(tk_memo_entry* tab, const tk_memo_entry* log, uint32_t i, uint32_t key_hash_mode, uint32_t mask) {
    const tk_memo_entry r = log[i];
    tk_memo_entry* w = tab + tk_memo_slot_of(r, key_hash_mode, mask);
    if (w->w4 == i) {
        wv_store16(w->k, r.k[0], r.k[1], r.k[2], r.k[3]);
        wv_store16(&w->w4, r.w4, r.v[0], r.v[1], r.v[2]);
    }
}

#endif
