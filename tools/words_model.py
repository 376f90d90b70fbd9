"""Lane-level model of tk_words_kernel (csrc/tk_words.hip): the step of one wave restated with numpy over 64 lanes
-- the two prefix sums, the three prefix maxima over the marked document starts, the values carried across steps, the counts
lane j keeps for document j -- so that the carries and the marks can be held against the definition without a GPU
(tests/test_words_cpu.py runs it against restatement A on random batches: foreign ids, specials anywhere, empty documents,
several document starts in one step, documents of hundreds of ids).

    kernel(ids, id_offs, doc_offs, flags, tok_len, ns, what, doc_words=None) -> (word_ids, n_words, word_first)
what = 0: word_ids and n_words (tk_words_kernel<0, *>); what = 1: word_first, given doc_words (tk_words_kernel<1, 0>).
"""
import numpy as np

M32 = 0xFFFFFFFF
NONE = 0xFFFFFFFF
GROUP = 16      # TK_DECODE_GROUP_DOCS
UNSET = 0xDEAD  # what an output element holds that the kernel never wrote


def scan_incl(v):
    return np.cumsum(v) & M32


def scan_max(v):
    return np.maximum.accumulate(v)


def kernel(ids, id_offs, doc_offs, flags, tok_len, ns, what, doc_words=None):
    n_docs = len(id_offs) - 1
    word_ids = np.full(len(ids), UNSET, np.int64)
    n_words = np.full(n_docs, UNSET, np.int64)
    word_first = np.full(int(doc_words[-1]) if doc_words is not None else 0, UNSET, np.int64)
    lane = np.arange(64)
    never = 1 << 62
    for g in range((n_docs + GROUP - 1) // GROUP):
        dA, dB = g * GROUP, min(g * GROUP + GROUP, n_docs)
        ndg = dB - dA
        i0, i1 = int(id_offs[dA]), int(id_offs[dB])
        dfirst = np.array([int(id_offs[dA + l]) if l < ndg else never for l in lane])
        dtext = np.array([int(doc_offs[dA + l]) if l < ndg else 0 for l in lane])
        dlen = np.array([int(doc_offs[dA + l + 1] - doc_offs[dA + l]) if l < ndg else 0 for l in lane])
        dwords = np.array([int(doc_words[dA + l]) if (what == 1 and l < ndg) else 0 for l in lane])
        dcount = np.zeros(64, np.int64)
        placed = np.zeros(64, bool)
        jn, nfirst = 0, dfirst[0]
        cursor = base = total = wbase = slot = 0
        c0 = i0
        while c0 < i1:
            i = c0 + lane
            have = i < i1
            idv = np.array([int(ids[x]) if x < i1 else 0 for x in i])
            ln = np.array([(tok_len[v - ns] if v >= ns else 0) if h else 0 for v, h in zip(idv, have)])
            incl = scan_incl(ln)
            excl = incl - ln
            mark = np.zeros(64, np.int64)
            while nfirst < c0 + 64:
                mark[nfirst - c0] = jn + 1
                jn += 1
                nfirst = dfirst[jn] if jn < ndg else never
            m = scan_max(np.where(mark > 0, excl + 1, 0))
            dbase = np.where(m > 0, cursor + m - 1, base)
            st = cursor + excl - dbase
            sm = scan_max(mark << 8)
            j = np.where(sm > 0, (sm >> 8) - 1, slot)
            tpos = dtext[j] + st
            tlen = dlen[j]
            body = have & (ln != 0) & (st < tlen)
            b = np.array([1 if (bd and flags[tp]) else 0 for bd, tp in zip(body, tpos)])
            bincl = scan_incl(b)
            bexcl = bincl - b
            wm = scan_max(np.where(mark > 0, (mark << 8) | (bexcl + 1), 0))
            wb = np.where(wm > 0, (total + ((wm & 0xFF) - 1)) & M32, wbase)
            word = (total + bincl - wb - 1) & M32
            placed |= (lane < ndg) & (dfirst < c0 + 64)
            be = bexcl[(dfirst - c0) & 63]
            sel = (lane < ndg) & (dfirst >= c0) & (dfirst < c0 + 64)
            dcount = np.where(sel, (total + be) & M32, dcount)
            for k in lane[have]:
                if what == 0:
                    word_ids[i[k]] = word[k] if ln[k] else NONE
                elif b[k]:
                    word_first[dwords[j[k]] + word[k]] = (i[k] - dfirst[j[k]]) & M32
            base, wbase, slot = dbase[63], wb[63], j[63]
            cursor += incl[63]
            total = (total + bincl[63]) & M32
            c0 += 64
        if what == 0:
            dcount = np.where(placed, dcount, total)
            nxt = np.where(lane + 1 < ndg, dcount[(lane + 1) & 63], total)
            for l in range(ndg):
                n_words[dA + l] = (nxt[l] - dcount[l]) & M32
    return word_ids, n_words, word_first
