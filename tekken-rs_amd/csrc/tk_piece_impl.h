// tk_piece_impl.h -- one piece [w0, e) of any length by one wave (overview: tk_encode_impl.h): its lookup and its merges
#ifndef TK_PIECE_IMPL_H
#define TK_PIECE_IMPL_H
#include "tk_encode_impl_args.h"
#include "tk_lookup.h"

#define TK_LONG_MAX 32768u /* longest piece the round-based merge takes (16 waves x 32 steps x 64 parts) */

// ------------------------------------------------------------------------------------------
// pass 2, one piece [w0, e) of any length: whole-piece lookup (wave-wide polynomial hash for
// pieces of >= 9 bytes), and on a miss the wave-cooperative merge over scratch memory.
// ------------------------------------------------------------------------------------------
// Which merge a piece [w0, e) that is not a vocabulary key takes (wave-uniform; a pure function of the bytes and the
// thresholds, so every kernel that asks gets the same answer): 0 = one merge per step by this wave; 1 = the compacting
// rounds of tk_long.hip (repetitive pieces of >= long_min bytes: thousands of occurrences per rank -- 15x); 2 = the lazy
// rounds (pieces with many distinct pairs of >= 4 long_min bytes: 2.3x at 32 KiB, break-even near 4 KiB; below that the
// rounds' fixed cost of ~5 us loses against a dozen steps of 1.1 us -- but a job of the rounds has a CU of its own while the
// single-wave merge holds up the kernel that walks ALL handed-back documents, so the threshold is 2 long_min: Zipf shape,
// 500 k documents 10.0 -> 9.15 ms, 4 M documents 32.2 -> 32.6 ms).  long_force (tests): 1 / 2 = every long piece there.
TK_DEV bool tk_piece_repetitive(const TkEncodeArgs& a, int lane, uint64_t w0, uint64_t e);
TK_DEV uint32_t tk_piece_is_long(const TkEncodeArgs& a, int lane, uint64_t w0, uint64_t e) {
    const uint64_t len = e - w0;
    if (len < (uint64_t)a.long_min || len > TK_LONG_MAX) return 0u;
    if (a.long_force) return a.long_force == 1u ? 1u : 2u;
    if (tk_piece_repetitive(a, lane, w0, e)) return 1u;
    return len >= (uint64_t)(a.long_lazy_mul ? a.long_lazy_mul : 2u) * a.long_min ? 2u : 0u;
}

// whole-piece lookup of the piece [w0, e): its rank or TK_RANK_MAX (wave-uniform)
TK_DEV uint32_t tk_piece_lookup(const TkEncodeArgs& a, const TkPolyPow& pw, int lane, uint64_t w0, uint64_t e) {
    const TkTablesView& t = a.t;
    const uint64_t n = e - w0;
    uint32_t r = TK_RANK_MAX;
    if (n == 1) {
        r = a.bytes[w0];
    } else if (n <= 16) {
        uint32_t kk[4] = {0u, 0u, 0u, 0u};
        for (uint64_t j = 0; j < n; ++j) kk[j >> 2] |= (uint32_t)a.bytes[w0 + j] << (8 * (j & 3));
        r = tk_probe_key(t, kk[0], kk[1], kk[2], kk[3], (uint32_t)n);
    } else {
        // H = sum b_j P^(n-1-j), folded 64 bytes at a time: H = H * P^m + (sum b_i P^-i) * P^(m-1)
        uint32_t h1 = 0, h2 = 0;
        for (uint64_t c = w0; c < e; c += 64) {
            int m = (e - c) < 64 ? (int)(e - c) : 64;
            uint32_t bb = lane < m ? (uint32_t)a.bytes[c + lane] : 0u;
            uint32_t s1 = tk_wave_sum(bb * pw.ipw1, lane);
            uint32_t s2 = tk_wave_sum(bb * pw.ipw2, lane);
            uint32_t pm1 = wv_shfl(pw.pw1, m - 1), pm2 = wv_shfl(pw.pw2, m - 1);
            h1 = h1 * (pm1 * TK_POLY_P1) + s1 * pm1;
            h2 = h2 * (pm2 * TK_POLY_P2) + s2 * pm2;
        }
        r = tk_probe_long(t, h1, h2, (uint32_t)n, a.bytes + w0);
    }
    return wv_first(r);
}

// Is the long piece [w0, e) REPETITIVE -- few distinct adjacent byte pairs among its first 512 bytes (runs of white space,
// of one symbol, of a short period)?  Such a piece merges many pairs per rank: the round-based workgroup merge
// (tk_long.hip) is up to 15x faster on it than one merge per step; on a piece with many distinct pairs (random letters: a
// dozen merges per rank) a round costs more than the dozen steps, and the piece stays with the single-wave merge
// (measured).  A pure function of the bytes: every kernel that asks gets the same answer.  Wave-uniform.
TK_DEV bool tk_piece_repetitive(const TkEncodeArgs& a, int lane, uint64_t w0, uint64_t e) {
    uint64_t seen = 0ull;                                        // pairs hashed into 64 buckets
    for (uint32_t k0 = 0; k0 < 512u; k0 += 64u) {
        const uint64_t p = w0 + k0 + (uint64_t)lane;
        if (p + 1 < e) {
            const uint32_t h = ((uint32_t)a.bytes[p] * 31u + (uint32_t)a.bytes[p + 1] * 7u) & 63u;
            seen |= 1ull << h;
        }
    }
    // OR over the lanes: one ballot per bucket would be 64 ballots; fold with shuffles instead (6 steps, two words)
    uint32_t lo = (uint32_t)seen, hi = (uint32_t)(seen >> 32);
    for (int d = 1; d < 64; d <<= 1) {
        lo |= wv_shfl(lo, lane ^ d);
        hi |= wv_shfl(hi, lane ^ d);
    }
    return (uint32_t)__builtin_popcount(wv_first(lo)) + (uint32_t)__builtin_popcount(wv_first(hi)) <= 20u;
}

// One merge of tk_piece_merge_coop: the pair at node i = (uint32_t)best, of rank rr = best >> 32, becomes one part.  What is
// read of i, its successor j, its predecessor p and j's successor k, the two re-probes with their TK_RANK_MAX patches, and
// the lane-0 rewrite of the four nodes.  REG (the block minima in registers): the token behind j comes from tokn, and the
// rank rows of the blocks of i, j and p are requested in the same round trip (row[3]); otherwise it is node k's.
struct TkpMerge {
    uint32_t i, j, p, new_i, new_p;            // the three nodes whose pair rank changed, and the ranks of i and p (j: TK_RANK_MAX)
    uint32_t bi, bj, bp;                       // their blocks (bp = bi where there is no p)
};
TK_DEV uint32_t tkp_merge_blk(const TkpMerge& m, int q) { return q == 0 ? m.bi : q == 1 ? m.bj : m.bp; }
// the rank of row element x as the merge left it: the three just-written ranks patched in registers (no wait on the stores)
TK_DEV uint32_t tkp_patched_rank(const TkpMerge& m, uint32_t x, uint32_t rk) {
    if (x == m.i) rk = m.new_i;
    if (x == m.j) rk = TK_RANK_MAX;
    if (m.p != TK_NONE && x == m.p) rk = m.new_p;
    return rk;
}
template <bool REG>
TK_DEV TkpMerge tkp_merge_step(const TkTablesView& t, tk_u32x4* node, uint32_t* tokn, uint32_t nn, int lane, uint64_t best, uint32_t* row) {
    TkpMerge m;
    const uint32_t i = (uint32_t)best, rr = (uint32_t)(best >> 32);
    const tk_u32x4 Ni = node[i];
    const uint32_t j = Ni.z, p = Ni.w;
    m.i = i; m.j = j; m.p = p;
    m.bi = i / 64u; m.bj = j / 64u; m.bp = (p != TK_NONE) ? p / 64u : m.bi;
    // one round trip: the two neighbours (REG: the token behind j, the rank rows of the blocks to refresh)
    const tk_u32x4 Nj = node[j];
    const tk_u32x4 Np = node[p != TK_NONE ? p : i];
    uint32_t tok_k = 0;
    if constexpr (REG) {
        tok_k = tokn[j];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const uint32_t x = tkp_merge_blk(m, q) * 64u + (uint32_t)lane;
            row[q] = x < nn ? node[x].y : TK_RANK_MAX;
        }
    }
    const uint32_t k = Nj.z;
    if constexpr (!REG) tok_k = node[k < nn ? k : i].x;
    tk_probe_pair_x2(t, rr, tok_k, Np.x, rr, m.new_i, m.new_p);
    if (k >= nn) m.new_i = TK_RANK_MAX;
    if (p == TK_NONE) m.new_p = TK_RANK_MAX;
    wv_sync();  // every lane has read the nodes before lane 0 rewrites them
    if (lane == 0) {
        tk_u32x4 v;
        v.x = rr; v.y = m.new_i; v.z = k; v.w = p;
        node[i] = v;
        if constexpr (REG) tokn[i] = tok_k;                        // i's successor is now k
        v.x = TK_DEAD; v.y = TK_RANK_MAX; v.z = Nj.z; v.w = Nj.w;
        node[j] = v;
        if (k < nn) node[k].w = i;
        if (p != TK_NONE) { node[p].y = m.new_p; if constexpr (REG) tokn[p] = rr; }
    }
    return m;
}

// the wave-cooperative merge of a piece that is not a vocabulary key (one merge per step, tiktoken's order)
TK_DEV void tk_piece_merge_small(const TkTablesView& t, const uint8_t* bytes, int lane, uint64_t w0, uint32_t n, uint32_t* out,
                                 uint32_t& cursor);
TK_DEV void tk_piece_merge_coop(const TkEncodeArgs& a, int lane, uint64_t w0, uint64_t e, uint32_t* out, uint32_t& cursor, uint32_t* scratch) {
    const TkTablesView& t = a.t;
    const uint64_t n = e - w0;
    if (n <= 256u && !a.dbg_mark) {            // short enough for the parts to live in registers: no scratch traffic at all
        tk_piece_merge_small(t, a.bytes, lane, w0, (uint32_t)n, out, cursor);
        return;
    }

    // ---- wave-cooperative merge over scratch: node[nn] = {tok, prk, nxt, prv} (16 B) | bmin[nb] (u64) ----
    // prk = rank of the pair (this part, next part); bmin[b] = min over the 64 nodes of block b of
    // (prk << 32 | position), so the global leftmost minimum is the min over bmin.  Per merge: one read
    // of bmin, node i, nodes j and p together, node k, both re-probes together, one store batch, and a
    // refresh of at most 3 block minima that patches the just-written ranks in registers (no wait on
    // the stores): about 5 dependent round trips.
    const uint32_t nn = (uint32_t)n;
    const uint32_t nb = (nn + 63u) / 64u;
    tk_u32x4* node = reinterpret_cast<tk_u32x4*>(scratch);
    uint32_t* bmin = scratch + 4u * nn;  // 2 words per block: lo = position, hi = rank
    if (a.dbg_mark && lane == 0) { a.dbg_mark[0] = 1u; a.dbg_mark[1] = nn; }
    for (uint32_t i = (uint32_t)lane; i < nn; i += 64u) {
        const uint32_t b0 = a.bytes[w0 + i];
        const uint32_t b1 = (i + 1u < nn) ? (uint32_t)a.bytes[w0 + i + 1u] : 0u;
        tk_u32x4 v;
        v.x = b0;
        v.y = (i + 1u < nn) ? t.pair2[b0 | (b1 << 8)] : TK_RANK_MAX;
        v.z = i + 1u;
        v.w = i ? i - 1u : TK_NONE;
        node[i] = v;
    }
    wv_sync();
    if (nb <= 512u) {
        // ---- up to 32 KiB: the block minima live in REGISTERS (lane l holds blocks l, l + 64, ...: 8 slots), every node
        // carries the token of its successor (tokn), and the rows of the (at most three) blocks whose minimum changes are
        // requested together with nodes j and p.  Dependent round trips per merge: node i | nodes j, p, tokn[j], rows |
        // the two re-probes | the stores' acknowledgement -- four instead of seven.
        uint32_t* tokn = bmin + 2u * nb;
        for (uint32_t i = (uint32_t)lane; i < nn; i += 64u) tokn[i] = (i + 1u < nn) ? (uint32_t)a.bytes[w0 + i + 1u] : 0u;
        uint64_t bm[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) bm[q] = ~0ull;
        for (uint32_t blk = 0; blk < nb; ++blk) {
            const uint32_t x = blk * 64u + (uint32_t)lane;
            const uint32_t rk = x < nn ? node[x].y : TK_RANK_MAX;
            const uint64_t m = tk_wave_min_key(rk, x);
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if ((uint32_t)q == (blk >> 6) && (uint32_t)lane == (blk & 63u)) bm[q] = m;
        }
        wv_sync();
        for (uint32_t merges = 0; merges < nn; ++merges) {  // at most nn - 1 merges can happen
            uint64_t best = bm[0];
#pragma unroll
            for (int q = 1; q < 8; ++q) best = bm[q] < best ? bm[q] : best;
            best = tk_wave_min_key((uint32_t)(best >> 32), (uint32_t)best);   // (~0: rank MAX)
            if (best == ~0ull) break;                        // wave-uniform
            uint32_t row[3];
            const TkpMerge m = tkp_merge_step<true>(t, node, tokn, nn, lane, best, row);
            // refresh the block minima of i, j and p from the rows, with the three just-written ranks patched in
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint32_t blk = tkp_merge_blk(m, q);
                if ((q == 1 && m.bj == m.bi) || (q == 2 && (m.bp == m.bi || m.bp == m.bj))) continue;   // (wave-uniform)
                const uint32_t x = blk * 64u + (uint32_t)lane;
                const uint64_t mk = tk_wave_min_key(tkp_patched_rank(m, x, row[q]), x);
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if ((uint32_t)u == (blk >> 6) && (uint32_t)lane == (blk & 63u)) bm[u] = mk;
            }
            wv_sync();  // this merge's stores are visible before the next merge's loads
        }
    } else {
        for (uint32_t blk = 0; blk < nb; ++blk) {
            const uint32_t x = blk * 64u + (uint32_t)lane;
            const uint32_t rk = x < nn ? node[x].y : TK_RANK_MAX;
            const uint64_t key = rk == TK_RANK_MAX ? ~0ull : (((uint64_t)rk << 32) | x);
            const uint64_t m = tk_wave_min64(key, lane);
            if (lane == 0) { bmin[2 * blk] = (uint32_t)m; bmin[2 * blk + 1] = (uint32_t)(m >> 32); }
        }
        wv_sync();
        for (uint32_t merges = 0; merges < nn; ++merges) {  // at most nn - 1 merges can happen
            if (a.dbg_mark && lane == 0) a.dbg_mark[2] = merges;
            uint64_t best = ~0ull;
            for (uint32_t bq = (uint32_t)lane; bq < nb; bq += 64u) {
                const uint64_t v = ((uint64_t)bmin[2 * bq + 1] << 32) | bmin[2 * bq];
                best = v < best ? v : best;
            }
            best = tk_wave_min64(best, lane);
            if (wv_ballot(best != ~0ull) == 0) break;  // decided on a ballot => a scalar branch
            const TkpMerge m = tkp_merge_step<false>(t, node, nullptr, nn, lane, best, nullptr);
            // refresh the block minima of i, j and p; the three just-written ranks are patched in registers
            const bool skip1 = wv_ballot(m.bj != m.bi) == 0;
            const bool skip2 = wv_ballot(m.bp != m.bi && m.bp != m.bj) == 0;
            for (int q = 0; q < 3; ++q) {
                if ((q == 1 && skip1) || (q == 2 && skip2)) continue;
                const uint32_t blk = tkp_merge_blk(m, q);
                const uint32_t x = blk * 64u + (uint32_t)lane;
                const uint32_t rk = tkp_patched_rank(m, x, x < nn ? node[x].y : TK_RANK_MAX);
                const uint64_t key = rk == TK_RANK_MAX ? ~0ull : (((uint64_t)rk << 32) | x);
                const uint64_t mk = tk_wave_min64(key, lane);
                if (lane == 0) { bmin[2 * blk] = (uint32_t)mk; bmin[2 * blk + 1] = (uint32_t)(mk >> 32); }
            }
            wv_sync();  // this merge's stores are visible before the next merge's loads
        }
    }
    if (a.dbg_mark && lane == 0) a.dbg_mark[0] = 5u;
    for (uint32_t blk = 0; blk < nb; ++blk) {
        const uint32_t x = blk * 64u + (uint32_t)lane;
        const uint32_t tv = x < nn ? node[x].x : TK_DEAD;
        const uint64_t am = wv_ballot(tv != TK_DEAD);
        if (tv != TK_DEAD) out[cursor + (uint32_t)tk_popc64(am & tk_lowmask(lane))] = tv + t.num_special;
        cursor += (uint32_t)tk_popc64(am);
    }
    if (a.dbg_mark && lane == 0) a.dbg_mark[0] = 6u;
}

// ------------------------------------------------------------------------------------------
// The byte-pair merge of ONE piece of up to 256 bytes by one wave with the parts in REGISTERS: position p = 64 j + lane
// (j = 0..3) holds the id of the part that starts there and the rank of its pair with the next part; four wave-uniform
// 64-bit masks say which positions are live.  A merge (tiktoken's order: the leftmost smallest rank) is one wave
// minimum, a few bit scans over the masks for the neighbours, two readlanes for their ids, ONE round trip for the two
// pairs the merge creates, and a handful of predicated moves -- no memory but the probes.  (tk_piece_merge_coop keeps
// the parts of a piece of ANY length in scratch and refreshes block minima from 64-lane rows: three wave-wide gathers
// per merge, which is what bounded it on pieces this short -- ~3 merges per microsecond and CU whatever the occupancy.)
// ------------------------------------------------------------------------------------------
TK_DEV uint32_t tkp_sel4(const uint32_t* v, uint32_t j) { return j == 0u ? v[0] : j == 1u ? v[1] : j == 2u ? v[2] : v[3]; }
TK_DEV uint64_t tkp_sel4(const uint64_t* v, uint32_t j) { return j == 0u ? v[0] : j == 1u ? v[1] : j == 2u ? v[2] : v[3]; }
// first live position above pos (256: none) / last live position below pos (TK_NONE: none); A, pos wave-uniform
TK_DEV uint32_t tkp_next(const uint64_t* A, uint32_t pos) {
    const uint32_t j = pos >> 6, l = pos & 63u;
    const uint64_t m = l < 63u ? (tkp_sel4(A, j) >> (l + 1u)) << (l + 1u) : 0ull;
    if (m) return 64u * j + (uint32_t)__builtin_ctzll(m);
    for (uint32_t jj = j + 1u; jj < 4u; ++jj) {
        const uint64_t a = tkp_sel4(A, jj);
        if (a) return 64u * jj + (uint32_t)__builtin_ctzll(a);
    }
    return 256u;
}
TK_DEV uint32_t tkp_prev(const uint64_t* A, uint32_t pos) {
    const uint32_t j = pos >> 6, l = pos & 63u;
    const uint64_t m = tkp_sel4(A, j) & ((1ull << l) - 1ull);
    if (m) return 64u * j + 63u - (uint32_t)__builtin_clzll(m);
    for (uint32_t jj = j; jj-- > 0u;) {
        const uint64_t a = tkp_sel4(A, jj);
        if (a) return 64u * jj + 63u - (uint32_t)__builtin_clzll(a);
    }
    return TK_NONE;
}
TK_DEV void tk_piece_merge_small(const TkTablesView& t, const uint8_t* bytes, int lane, uint64_t w0, uint32_t n, uint32_t* out,
                                 uint32_t& cursor) {
    uint32_t tok[4], rk[4];
    uint64_t A[4];
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t p = 64u * j + (uint32_t)lane;
        const uint32_t b0 = p < n ? (uint32_t)bytes[w0 + p] : 0u;
        const uint32_t b1 = p + 1u < n ? (uint32_t)bytes[w0 + p + 1u] : 0u;
        tok[j] = b0;
        rk[j] = p + 1u < n ? t.pair2[b0 | (b1 << 8)] : TK_RANK_MAX;
        A[j] = wv_first64(n >= 64u * (j + 1u) ? ~0ull : n <= 64u * j ? 0ull : ((1ull << (n - 64u * j)) - 1ull));
    }
    for (uint32_t merges = 0; merges < n; ++merges) {          // at most n - 1 merges can happen
        uint32_t key = 0xFFFFFFFFu;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t k = rk[j] == TK_RANK_MAX ? 0xFFFFFFFFu : ((rk[j] << 8) | (64u * j + (uint32_t)lane));
            key = k < key ? k : key;
        }
        key = wv_first(wv_min_u32(key));
        if (key == 0xFFFFFFFFu) break;                         // wave-uniform
        const uint32_t i = key & 255u, rr = key >> 8;
        // (readfirstlane on everything that is the same in all lanes: the mask arithmetic then runs on the scalar unit)
        const uint32_t jn = wv_first(tkp_next(A, i));           // exists: the pair at i was live
        const uint32_t nn = wv_first(tkp_next(A, jn)), p = wv_first(tkp_prev(A, i));
        const uint32_t tok_nn = nn < 256u ? wv_shfl(tkp_sel4(tok, nn >> 6), (int)(nn & 63u)) : 0u;
        const uint32_t tok_p = p != TK_NONE ? wv_shfl(tkp_sel4(tok, p >> 6), (int)(p & 63u)) : 0u;
        uint32_t new_i, new_p;
        tk_probe_pair_x2(t, rr, tok_nn, tok_p, rr, new_i, new_p);   // (every lane asks for the same two buckets: one request each)
        if (nn >= 256u) new_i = TK_RANK_MAX;
        if (p == TK_NONE) new_p = TK_RANK_MAX;
        // the part at i takes the merged id and its new pair rank, the part at jn dies, the part at p gets its new pair rank
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t pos = 64u * j + (uint32_t)lane;
            if (pos == i) { tok[j] = rr; rk[j] = new_i; }
            if (pos == jn) rk[j] = TK_RANK_MAX;
            if (p != TK_NONE && pos == p) rk[j] = new_p;
            if ((jn >> 6) == j) A[j] = wv_first64(A[j] & ~(1ull << (jn & 63u)));
        }
    }
    uint32_t base = cursor;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        if ((A[j] >> lane) & 1ull) out[base + (uint32_t)tk_popc64(A[j] & tk_lowmask(lane))] = tok[j] + t.num_special;
        base += (uint32_t)tk_popc64(A[j]);
    }
    cursor = base;
}

#endif
