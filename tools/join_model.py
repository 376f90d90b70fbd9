"""The join kernels (csrc/tk_join.hip) step for step in Python: the parts pass and, tile by tile and unit by unit,
the main kernel -- the 64-ary wave search on an array with ties (seqpack_model.wave_count_le), the staged starts and part
records, the binary search of a unit, its one-load form and its walk forward over 4 positions.  Every index the kernel would read or write is asserted to lie inside
its array, and every output element to be written exactly once.  tests/test_join_cpu.py checks the model against the plain-loop
definition at small tile sizes; the kernels themselves are checked on the GPU (tests/test_gpu_join.py)."""
from seqpack_model import wave_count_le

NONE = 0xFFFFFFFF


def join_model(ids, id_offs, ctrl, pflags, conv_offs, ignore, want_labels=True, want_part_index=True, tile=4096, cap=1024):
    ids, oo, ctrl, conv = [int(x) for x in ids], [int(x) for x in id_offs], [int(x) for x in ctrl], [int(x) for x in conv_offs]
    P, C = len(oo) - 1, len(conv) - 1
    pf = [0] * P if pflags is None else [int(x) for x in pflags]
    size = len(ids) + P                                   # elements the outputs hold
    # tk_join_has_kernel + tk_launch_scan
    has = [int(c != NONE) for c in ctrl]
    cb = [0]
    for h in has:
        cb.append(cb[-1] + h)
    # tk_join_parts_kernel
    start = [oo[p] + cb[p] for p in range(P + 1)]
    plocal, n_labelled = [0] * P, 0
    for p in range(P):
        if pf[p] & 1 and has[p]:
            n_labelled += 1
        if pf[p] & 2:
            n_labelled += oo[p + 1] - oo[p]
        lo, hi = 0, C
        while lo < hi:
            mid = lo + (hi - lo) // 2
            if conv[mid] <= p:
                lo = mid + 1
            else:
                hi = mid
        plocal[p] = p - conv[lo - 1] if lo else p
    offsets = [oo[min(q, P)] + cb[min(q, P)] for q in conv]
    # tk_join_kernel
    N = min(start[P], size)
    out, lab, pidx, written = [None] * size, [None] * size, [None] * size, [0] * size
    forms = set()
    for t in range((N + tile - 1) // tile):
        g0 = t * tile
        g1 = N if N - g0 < tile else g0 + tile
        n_lo, n_hi = wave_count_le(start, P, g0), wave_count_le(start, P, g1 - 1)
        if n_lo == 0 or n_hi < n_lo:
            continue
        cnt = n_hi - n_lo
        forms.add("lds" if cnt <= cap else "global")
        rel = [start[n_lo + j] - g0 for j in range(cnt)]  # (s_rel, or the same values from global memory)
        assert all(0 < r < g1 - g0 for r in rel)
        # the tile's parts n_lo - 1 + j, j <= cnt: (ctrl, label bits, local index, srcoff) -- staged in LDS, or read in place
        cb_lo = cb[n_lo]
        for j in range(cnt + 1):
            assert 0 <= n_lo - 1 + j < P and 0 <= cb[n_lo + j] - cb_lo <= tile
        part = lambda j: (ctrl[n_lo - 1 + j], pf[n_lo - 1 + j] & 3, plocal[n_lo - 1 + j], cb_lo + (cb[n_lo + j] - cb_lo))
        rel_lo = start[n_lo - 1] - g0
        assert rel_lo <= 0
        length = g1 - g0
        for l in range(0, length, 4):
            g = g0 + l
            k, hi = 0, cnt
            while k < hi:
                mid = (k + hi) >> 1
                if rel[mid] <= l:
                    k = mid + 1
                else:
                    hi = mid
            c, fl, pl, srcoff = part(k)
            pstart = rel[k - 1] if k else rel_lo
            vals = []
            if l + 4 <= length and (k == cnt or rel[k] >= l + 4) and not (c != NONE and pstart == l):
                forms.add("one load")
                assert 0 <= g - srcoff and g - srcoff + 4 <= len(ids), (g, srcoff)
                vals = [(ids[g - srcoff + q], ids[g - srcoff + q] if fl & 2 else ignore, pl) for q in range(4)]
            else:
                forms.add("walk")
                for q in range(4):
                    if l + q >= length:
                        break
                    if k < cnt and rel[k] <= l + q:
                        while k < cnt and rel[k] <= l + q:
                            k += 1
                        c, fl, pl, srcoff = part(k)
                        pstart = rel[k - 1]
                    if c != NONE and pstart == l + q:
                        vals.append((c, c if fl & 1 else ignore, pl))
                    else:
                        assert 0 <= g + q - srcoff < len(ids), (g + q, srcoff)
                        v = ids[g + q - srcoff]
                        vals.append((v, v if fl & 2 else ignore, pl))
            assert len(vals) == min(4, length - l) and (len(vals) == 4 or g1 == N)
            for q, (v, lb, pl) in enumerate(vals):
                assert g + q < size
                out[g + q], lab[g + q], pidx[g + q] = v, lb, pl
                written[g + q] += 1
    assert written[:N] == [1] * N and not any(written[N:])
    return {"ids": out[:N], "offsets": offsets, "labels": lab[:N] if want_labels else None,
            "part_index": pidx[:N] if want_part_index else None, "n_ids": N, "n_ctrl": cb[P], "n_labelled": n_labelled, "forms": forms}
