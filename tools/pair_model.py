"""The pair pass (tekken-rs_amd/csrc/tk_pair.hip) restated index by index in Python: the counts, pair_windows, a block's run of rows,
its two searches, the staged starts (LDS or, beyond `cap` pairs, global memory), a unit's pair / row number / kept ranges (tkp_kept),
the five source runs, the 4-wide load where four elements lie in one id run.  Every read of the ids and every write is asserted to
stay inside its array, and every element to be written exactly once.  tests/test_pair_cpu.py runs it against the definition at
small tiles, where every block boundary case shows up in small inputs, and at the kernel's own sizes."""
import bisect

import numpy as np

LONGEST_FIRST, ONLY_FIRST, ONLY_SECOND = 0, 1, 2
SEQ_NONE = 255
M32 = 2 ** 32


def kept(strategy, overflow, c, s, F, a, b, k):
    """tkp_kept: (as, alen, bs, blen) of row k of a pair with a and b ids; F is resolved (never 0 with an ONLY_ strategy)."""
    if strategy == LONGEST_FIRST:
        alen, blen = a, b
        if a + b > c:
            if a <= b:
                alen = min(a, c // 2)
                blen = min(b, c - alen)
            else:
                blen = min(b, c // 2)
                alen = min(a, c - blen)
        return 0, alen, 0, blen
    second = strategy == ONLY_SECOND
    v = b if second else a
    f = min(a if second else b, F)
    cw = c - f
    assert cw >= 1 and cw - s >= 1
    vs, vlen = 0, v
    if v > cw:
        if overflow:
            vs = k * (cw - s)
            assert vs < v and vs < M32
            vlen = min(v - vs, cw)
        else:
            vlen = cw
    return (0, f, vs, vlen) if second else (vs, vlen, 0, f)


def pair_model(ids, oo, T, strategy, s, F, overflow, head, sep, tail, L, pad_id, tile=2048, cap=1024):
    """-> (input_ids [W, L] int64, mask, type_ids, sequence_ids [W, L], lengths, window_pair, window_start, second_start,
    pair_windows, (longest row, n_truncated, n_split, n_fixed_cut)) as arrays / lists."""
    P, N = (len(oo) - 1) // 2, len(ids)
    x = len(head) + len(sep) + len(tail)
    c = T - x
    if strategy != LONGEST_FIRST and F == 0:
        F = c - 1
    counts, longest, n_trunc, n_split, n_cut = [], 0, 0, 0, 0       # tk_pair_counts_kernel
    for p in range(P):
        a, b = oo[2 * p + 1] - oo[2 * p], oo[2 * p + 2] - oo[2 * p + 1]
        _, alen, _, blen = kept(strategy, overflow, c, s, F, a, b, 0)
        assert x + alen + blen <= T
        longest = max(longest, x + alen + blen)
        n_trunc += alen < a or blen < b
        w = 1
        if strategy != LONGEST_FIRST:
            xl, v = (a, b) if strategy == ONLY_SECOND else (b, a)
            cw = c - min(xl, F)
            n_cut += xl > F
            if overflow and v > cw:
                step = cw - s
                w = 1 + (v - cw + step - 1) // step
                n_split += 1
        counts.append(w)
    pw = [0]
    for w in counts:                                   # tk_launch_scan
        pw.append(pw[-1] + w)
    W = pw[-1]
    vec = L != 0 and L % 4 == 0                        # tk_launch_pair
    G = L // 4 if vec else (L if L else 1)
    width = 4 if vec else 1
    rb = tile // G if G <= tile else 1
    shape = (W, max(L, 1))
    out, written = np.full(shape, -1, np.int64), np.zeros(shape, np.int64)
    mask, typ, seq = np.full(shape, -1, np.int64), np.full(shape, -1, np.int64), np.full(shape, -1, np.int64)
    lengths, wpair, wstart, second = [-1] * W, [-1] * W, [-1] * W, [-1] * W
    starts = pw[:P]
    for row0 in range(0, W, rb):                       # tk_pair_kernel: one block
        nrows = min(rb, W - row0)
        n_lo = bisect.bisect_right(starts, row0)       # the two wave searches
        assert n_lo >= 1
        count = bisect.bisect_right(starts, row0 + nrows - 1) - n_lo
        assert 0 <= count < nrows or (nrows == 1 and count == 0)
        lds = count <= cap
        rel = [starts[n_lo + j] - row0 for j in range(count)]
        assert all(0 < r < nrows for r in rel)
        staged = [(oo[2 * e], oo[2 * e + 1] - oo[2 * e], oo[2 * e + 2] - oo[2 * e + 1]) for e in range(n_lo - 1, n_lo + count)] if lds else None
        start_lo = starts[n_lo - 1]
        for li in range(nrows * G):                    # a unit
            r = li // G if rb > 1 else 0
            cg = li - r * G
            kd = bisect.bisect_right(rel, r)
            p = n_lo - 1 + kd
            assert 0 <= p < P
            kw = r - (rel[kd - 1] if kd else -(row0 - start_lo))
            assert 0 <= kw < counts[p]
            o0, a, b = staged[kd] if lds else (oo[2 * p], oo[2 * p + 1] - oo[2 * p], oo[2 * p + 2] - oo[2 * p + 1])
            assert (o0, a, b) == (oo[2 * p], oo[2 * p + 1] - oo[2 * p], oo[2 * p + 2] - oo[2 * p + 1])
            as_, alen, bs, blen = kept(strategy, overflow, c, s, F, a, b, kw)
            assert as_ + alen <= a and bs + blen <= b
            e0 = len(head)
            e1 = e0 + alen
            e2 = e1 + len(sep)
            e3 = e2 + blen
            e4 = e3 + len(tail)
            assert e4 <= T and (L == 0 or e4 <= L)
            oa = (o0 + as_ - e0) % 2 ** 64             # (the kernel's sums wrap and wrap back)
            ob = (o0 + a + bs - e2) % 2 ** 64
            row = row0 + r
            if cg == 0:
                assert lengths[row] == -1
                lengths[row], wpair[row], wstart[row], second[row] = e4, p, bs if strategy == ONLY_SECOND else as_, e2
            if L == 0:
                continue
            j0 = cg * width

            def load(at, lo, n):                       # ids[at], which must lie in ids[lo : lo + n]
                at %= 2 ** 64
                assert lo <= at < lo + n and at < N
                return ids[at]
            in_a = vec and j0 >= e0 and j0 + 4 <= e1
            in_b = vec and j0 >= e2 and j0 + 4 <= e3
            for q in range(width):
                j = j0 + q
                assert j < L
                if in_a or in_b:                       # one 16-byte load: all four inside the run
                    out[row, j] = load((oa if in_a else ob) + j, o0 + as_ if in_a else o0 + a + bs, alen if in_a else blen)
                    mask[row, j], typ[row, j], seq[row, j] = 1, int(in_b), int(in_b)
                else:
                    is_a, is_b = e0 <= j < e1, e2 <= j < e3
                    if is_a:
                        out[row, j] = load(oa + j, o0 + as_, alen)
                    elif is_b:
                        out[row, j] = load(ob + j, o0 + a + bs, blen)
                    else:
                        out[row, j] = head[j] if j < e0 else sep[j - e1] if j < e2 else tail[j - e3] if j < e4 else pad_id
                    mask[row, j], typ[row, j] = int(j < e4), int(e2 <= j < e4)
                    seq[row, j] = 0 if is_a else 1 if is_b else SEQ_NONE
                written[row, j] += 1
    assert L == 0 or np.all(written == 1)
    assert -1 not in lengths
    return (out[:, :L], mask[:, :L], typ[:, :L], seq[:, :L], lengths, wpair, wstart, second, pw, (longest, int(n_trunc), n_split, int(n_cut)))
