"""The window pass (tekken-rs_amd/csrc/tk_window.hip) restated index by index in Python: the counts, doc_windows, a block's run of
rows, its two searches, the staged starts (LDS or, beyond `cap` documents, global memory), a unit's document / window number /
source runs, the 4-wide load where four elements lie at four consecutive ids.  Every read of the ids and every write is asserted to
stay inside its array, and every element to be written exactly once.  tests/test_window_cpu.py runs it against the definition at
small tiles, where every block boundary case shows up in small inputs, and at the kernel's own sizes."""
import bisect

import numpy as np


def window_model(ids, oo, T, s, h, t, L, pad_id, tile=2048, cap=1024):
    """-> (input_ids [W, L] int64, lengths, window_doc, window_start, doc_windows) as lists / an array."""
    D, N = len(oo) - 1, len(ids)
    c = T - h - t
    step = c - s
    counts = []                                        # tk_window_counts_kernel
    for d in range(D):
        n = oo[d + 1] - oo[d]
        counts.append(1 if n <= T else 1 + (n - T + step - 1) // step)
    dw = [0]
    for x in counts:                                   # tk_launch_scan
        dw.append(dw[-1] + x)
    W = dw[-1]
    vec = L != 0 and L % 4 == 0                        # tk_launch_window
    G = L // 4 if vec else (L if L else 1)
    width = 4 if vec else 1
    rb = tile // G if G <= tile else 1
    out = np.full((W, max(L, 1)), -1, np.int64)
    written = np.zeros((W, max(L, 1)), np.int64)
    lengths, wdoc, wstart = [-1] * W, [-1] * W, [-1] * W
    starts = dw[:D]
    for row0 in range(0, W, rb):                       # tk_window_kernel: one block
        nrows = min(rb, W - row0)
        n_lo = bisect.bisect_right(starts, row0)       # the two wave searches
        assert n_lo >= 1
        count = bisect.bisect_right(starts, row0 + nrows - 1) - n_lo
        assert 0 <= count < nrows or (nrows == 1 and count == 0)
        lds = count <= cap
        rel = [starts[n_lo + j] - row0 for j in range(count)]
        assert all(0 < x < nrows for x in rel)
        s_oo = [oo[n_lo - 1 + j] for j in range(count + 1)] if lds else None
        start_lo = starts[n_lo - 1]
        for li in range(nrows * G):                    # a unit
            r = li // G if rb > 1 else 0
            cg = li - r * G
            kd = bisect.bisect_right(rel, r)
            d = n_lo - 1 + kd
            assert 0 <= d < D
            kw = r - (rel[kd - 1] if kd else -(row0 - start_lo))
            assert 0 <= kw < counts[d]
            o0 = s_oo[kd] if lds else oo[d]
            assert o0 == oo[d]
            n = oo[d + 1] - o0
            hh, tt, bs, blen = 0, 0, 0, n
            if n > T:
                body = n - h - t
                hh, tt, bs = h, t, kw * step
                assert bs < body < 2 ** 32
                blen = min(body - bs, c)
            hb = hh + blen
            ln = hb + tt
            row = row0 + r

            def src(j):
                assert j < ln
                x = o0 + (j if j < hh else hh + bs + (j - hh) if j < hb else (n - tt) + (j - hb))
                assert o0 <= x < o0 + n and x < N
                return x
            if cg == 0:
                assert lengths[row] == -1
                lengths[row], wdoc[row], wstart[row] = ln, d, min(h + kw * step, n)
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
    assert -1 not in lengths
    return out[:, :L], lengths, wdoc, wstart, dw
