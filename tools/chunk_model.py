"""The chunk pass (tekken-rs_amd/csrc/tk_chunk.hip) restated index by index in Python, in the manner of tools/window_model.py: the
wave walk -- a wave of `width` lanes takes `group` documents, settles the unsplit ones a lane each and walks the split ones one after
another, scanning the candidates `width` positions at a time from the top and the overlap from the bottom --, run twice (counts,
then records), the scan between the two, and the fill kernel (a block's run of rows, its two searches, the staged starts, a unit's
document / record / source runs, the 4-wide load).  levels_model is the levels kernel's walk: the document slot of every id of a
group of documents from the marked starts, and the byte reads of the rules.  Every read of the ids, levels, spans and text and
every write is asserted to stay inside its array, and every output element to be written exactly once.  tests/test_chunk_cpu.py
runs both against the definition at wave widths 4 and 64."""
import bisect

import numpy as np

U32 = 2 ** 32
TOP, CUT_LAST = 5, 255


def walk_model(oo, lev, T, m, o, h, t, width, group, dw=None):
    """tk_chunk_walk_kernel<RUN>: dw None: RUN 0 -> (counts, longest, n_split, level_counts); else RUN 1 -> rec [(start, len, level)]."""
    D, N = len(oo) - 1, len(lev)
    c = T - h - t
    assert 1 <= group <= width and c >= 1 and 0 <= o < m <= c
    run = dw is not None
    counts, cuts = [None] * D, [0] * 6
    rec = [None] * dw[-1] if run else None
    longest = n_split = 0

    def put(row, value):
        assert 0 <= row < len(rec) and rec[row] is None
        rec[row] = value

    for g in range((D + group - 1) // group):
        lanes = []                                     # (lane, d, o0, n) of the lanes that hold a document
        for lane in range(width):
            d = g * group + lane
            if lane < group and d < D:
                lanes.append((lane, d, oo[d], oo[d + 1] - oo[d]))
        todo = []
        for lane, d, o0, n in lanes:
            assert n < U32 - 1
            longest = max(longest, n)
            if n > T:
                todo.append((lane, d, o0, n))
                n_split += 1
            elif run:
                put(dw[d], (0, n, CUT_LAST))
            else:
                assert counts[d] is None
                counts[d] = 1
        for lane, d, so, sn in todo:                   # the ballot loop: one split document after another, by the whole wave
            b = sn - h - t
            base = so + h                              # L[j] = lev[base + j], j < b

            def L(j):
                assert 0 <= j < b and so <= base + j < so + sn and base + j < N
                return lev[base + j]
            s = k = 0
            while True:
                assert 0 <= s < b
                if b - s <= c:
                    if run:
                        put(dw[d] + k, (s, b - s, CUT_LAST))
                    k += 1
                    break
                lo, top = s + m, s + c
                assert top < b < U32
                key, pos = [0] * width, [0] * width
                while True:
                    assert top >= lo
                    for i in range(width):
                        if i <= top - lo:
                            kk = min(L(top - i), TOP) + 1
                            if kk > key[i]:
                                key[i], pos[i] = kk, top - i
                    if top - lo < width or TOP + 1 in key:
                        break
                    top -= width
                bk = max(key)                          # the two prefix maxima
                assert bk >= 1
                e = max(pos[i] if key[i] == bk else 0 for i in range(width))
                assert lo <= e <= s + c
                if run:
                    put(dw[d] + k, (s, e - s, bk - 1))
                else:
                    cuts[bk - 1] += 1
                k += 1
                assert e >= o
                frm = max(e - o, s + 1)
                nxt, tok, q = e, False, frm
                while q < e:
                    lv = [L(q + i) if i < e - q else 0 for i in range(width)]
                    words = [i for i in range(width) if lv[i] >= 2]
                    if words:
                        nxt = q + words[0]
                        break
                    tokens = [i for i in range(width) if lv[i] >= 1]
                    if not tok and tokens:
                        nxt, tok = q + tokens[0], True
                    q += width
                assert s < nxt <= e
                s = nxt
            if not run:
                assert counts[d] is None and k < U32
                counts[d] = k
    if run:
        assert None not in rec
        return rec
    assert None not in counts
    return counts, longest, n_split, cuts


def fill_model(ids, oo, spans, dw, rec, T, h, t, L, pad_id, tile, cap):
    """tk_chunk_kernel -> (input_ids [W, L], lengths, window_doc, window_start, cut_level, chunk_bytes)."""
    D, N, W = len(oo) - 1, len(ids), dw[-1]
    vec = L != 0 and L % 4 == 0
    G = L // 4 if vec else (L if L else 1)
    width = 4 if vec else 1
    rb = tile // G if G <= tile else 1
    out = np.full((W, max(L, 1)), -1, np.int64)
    written = np.zeros((W, max(L, 1)), np.int64)
    lengths, wdoc, wstart, cut, cbytes = [-1] * W, [-1] * W, [-1] * W, [-1] * W, [None] * W
    starts = dw[:D]
    for row0 in range(0, W, rb):                       # one block
        nrows = min(rb, W - row0)
        n_lo = bisect.bisect_right(starts, row0)       # the two wave searches
        assert n_lo >= 1
        count = bisect.bisect_right(starts, row0 + nrows - 1) - n_lo
        assert 0 <= count < nrows or (nrows == 1 and count == 0)
        lds = count <= cap
        rel = [starts[n_lo + j] - row0 for j in range(count)]
        s_oo = [oo[n_lo - 1 + j] for j in range(count + 1)] if lds else None
        for li in range(nrows * G):                    # a unit
            r = li // G if rb > 1 else 0
            cg = li - r * G
            kd = bisect.bisect_right(rel, r)
            d = n_lo - 1 + kd
            assert 0 <= d < D
            o0 = s_oo[kd] if lds else oo[d]
            assert o0 == oo[d]
            n = oo[d + 1] - o0
            row = row0 + r
            assert dw[d] <= row < dw[d + 1]
            bs, blen, level = rec[row]
            hh, tt = (h, t) if n > T else (0, 0)
            assert hh + bs + blen <= n - tt and (n > T or (bs, blen) == (0, n))
            hb = hh + blen
            ln = hb + tt
            assert ln <= max(L, 0) or L == 0

            def src(j):
                assert j < ln
                x = o0 + (j if j < hh else hh + bs + (j - hh) if j < hb else (n - tt) + (j - hb))
                assert o0 <= x < o0 + n and x < N
                return x
            if cg == 0:
                assert lengths[row] == -1
                lengths[row], wdoc[row], wstart[row], cut[row] = ln, d, min(h + bs, n), level
                if blen:
                    f = o0 + hh + bs
                    assert o0 <= f and f + blen - 1 < o0 + n
                    cbytes[row] = [spans[f][0], spans[f + blen - 1][1]]
                else:
                    cbytes[row] = [0, 0]
            if L == 0:
                continue
            j0 = cg * width
            run4 = False
            if vec and j0 + 4 <= ln:
                s0 = src(j0)
                run4 = src(j0 + 3) == s0 + 3
            for q in range(width):
                j = j0 + q
                assert j < L
                out[row, j] = ids[s0 + q] if run4 else ids[src(j)] if j < ln else pad_id
                written[row, j] += 1
    assert L == 0 or np.all(written == 1)
    assert -1 not in lengths and None not in cbytes
    return out[:, :L], lengths, wdoc, wstart, cut, cbytes


def chunk_model(ids, oo, lev, spans, T, m, o, h, t, L, pad_id, width=64, group=64, tile=2048, cap=1024):
    """The pass as tk_capi_chunk.cpp runs it: walk (counts), scan, walk (records), fill."""
    counts, longest, n_split, cuts = walk_model(oo, lev, T, m, o, h, t, width, group)
    dw = [0]
    for x in counts:                                   # tk_launch_scan
        dw.append(dw[-1] + x)
    rec = walk_model(oo, lev, T, m, o, h, t, width, group, dw)
    out, lengths, wdoc, wstart, cut, cbytes = fill_model(ids, oo, spans, dw, rec, T, h, t, L, pad_id, tile, cap)
    return {"input_ids": out, "lengths": lengths, "window_doc": wdoc, "window_start": wstart, "doc_windows": dw, "cut_level": cut,
            "chunk_bytes": cbytes, "level_counts": cuts, "n_split": n_split, "longest": longest}


WS = (0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20)


def level_model(data, text, ln, p):
    """tkc_level: the level in front of byte p of the document data[text : text + ln], before the mask."""
    def at(x):
        assert 0 <= x < ln and text + x < len(data)
        return data[text + x]
    if p >= ln or p == 0:
        return 1
    c0 = at(p)
    if c0 & 0xC0 == 0x80:
        return 0
    q, nl, walked = p, 0, 0
    while walked < 16 and q > 0:
        ch = at(q - 1)
        if ch not in WS:
            break
        nl += ch == 0x0A
        q -= 1
        walked += 1
    if nl >= 2:
        return 5
    if nl == 1:
        return 4
    gap = q < p or c0 in WS
    if walked < 16 and q > 0:
        e = at(q - 1)
        if gap and e in b".!?":
            return 3
        if q >= 3 and (at(q - 3) << 16 | at(q - 2) << 8 | e) in (0xE38082, 0xEFBC81, 0xEFBC9F):
            return 3
    return 2 if gap else 1


def levels_model(data, offs, spans, oo, mask, width=64):
    """tk_chunk_levels_kernel -> the level byte of every id.  A wave of `width` lanes takes min(16, width) documents."""
    D, N = len(oo) - 1, len(spans)
    docs = min(16, width)
    demote, to = 1 << 4, 1                             # tk_capi_chunk.cpp run_levels
    for lv in range(2, 6):
        if mask & (1 << lv):
            to = lv
        demote |= to << (4 * lv)
    out = [None] * N
    for dA in range(0, D, docs):
        dB = min(dA + docs, D)
        ndg = dB - dA
        i0, i1 = oo[dA], oo[dB]
        dfirst = [oo[dA + j] for j in range(ndg)]
        dtext = [offs[dA + j] for j in range(ndg)]
        dlen = [offs[dA + j + 1] - offs[dA + j] for j in range(ndg)]
        jn, slot = 0, 0
        nfirst = dfirst[0]
        for c0 in range(i0, i1, width):
            mark = [0] * width
            while nfirst is not None and nfirst < c0 + width:
                assert nfirst >= c0
                mark[nfirst - c0] = jn + 1
                jn += 1
                nfirst = dfirst[jn] if jn < ndg else None
            sm = 0
            for lane in range(width):                  # the prefix maximum
                sm = max(sm, mark[lane])
                j = sm - 1 if sm else slot
                i = c0 + lane
                if lane == width - 1:
                    last = j
                if i < i1:
                    assert 0 <= j < ndg and oo[dA + j] <= i < oo[dA + j + 1] and out[i] is None
                    out[i] = (demote >> (4 * level_model(data, dtext[j], dlen[j], spans[i][0]))) & 15
            slot = last
    assert None not in out
    return out
