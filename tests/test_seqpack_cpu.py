"""Packed fixed-length training rows (include/tekken_hip.h tk_seqpack_from_ids_device), the parts that need no GPU: the plain-loop
restatement of the definition that tests/test_gpu_seqpack.py checks the kernels against, the hand-made cases of the definition,
the Rust shim's declarations, and the host-only tokenizer."""
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["tk_seqpack_from_ids_device", "tk_encode_batch_device_seqpack", "tk_encode_batch_seqpack", "tk_free_seqpack"]
I64, POSITIONS, SEGMENTS, CU_SEQLENS, DROP_LAST = 1, 2, 4, 8, 16
ALL = POSITIONS | SEGMENTS | CU_SEQLENS
FLAG_VALUES = {"TK_SEQPACK_I64": 1, "TK_SEQPACK_POSITIONS": 2, "TK_SEQPACK_SEGMENTS": 4, "TK_SEQPACK_CU_SEQLENS": 8,
               "TK_SEQPACK_DROP_LAST": 16}


def expected_packed(ids, oo, seq_len, pad_id, flags=ALL):
    """The definition, restated document by document with plain loops (no cumulative sum, no search).  -> dict(input_ids,
    position_ids, segment_ids [n_rows, L] int32 / int64 (an unselected one: None), cu_seqlens int32 [n_segments + 1] or None,
    n_rows, n_used, n_left, n_segments, max_seqlen).  Invalid options raise ValueError (the entries: TK_ERR_INVALID_ARG)."""
    ids = np.asarray(ids, np.int64)
    oo = [int(x) for x in oo]
    L, D, N = int(seq_len), len(oo) - 1, int(oo[-1])
    if L <= 0 or L >= 2 ** 31 or flags & ~(I64 | ALL | DROP_LAST):
        raise ValueError("seq_len / flags")
    n_rows = N // L if flags & DROP_LAST else (N + L - 1) // L
    if n_rows * L > 2 ** 36:
        raise ValueError("tensor too large")
    n_used = min(N, n_rows * L)
    if flags & CU_SEQLENS and n_used >= 2 ** 31:
        raise ValueError("cu_seqlens is int32")
    inp, pos, seg = [pad_id] * (n_rows * L), [0] * (n_rows * L), [0] * (n_rows * L)   # (lists: the loops below touch every element)
    src = ids.tolist()
    cu = []
    for d in range(D):
        p, s = 0, 0                                   # position inside the current segment, its number inside the row
        for g in range(oo[d], min(oo[d + 1], n_used)):
            c = g % L
            if g == oo[d] or c == 0:                  # a document start or a row start: a new segment
                cu.append(g)
                p = 0
                # (its number: one more than the last segment of this row, which the element to the left carries)
                s = 1 if c == 0 else seg[g - 1] + 1
            inp[g], pos[g], seg[g] = src[g], p, s
            p += 1
    dt = np.int64 if flags & I64 else np.int32
    inp, pos, seg = np.array(inp, dt), np.array(pos, dt), np.array(seg, dt)
    n_segments = len(cu)
    cu.append(n_used)
    max_seqlen = 0
    for i in range(n_segments):
        max_seqlen = max(max_seqlen, cu[i + 1] - cu[i])
    shape = (n_rows, L)
    return {"input_ids": inp.reshape(shape), "position_ids": pos.reshape(shape) if flags & POSITIONS else None,
            "segment_ids": seg.reshape(shape) if flags & SEGMENTS else None,
            "cu_seqlens": np.array(cu, np.int32) if flags & CU_SEQLENS else None, "n_rows": n_rows, "n_used": n_used,
            "n_left": N - n_used, "n_segments": n_segments, "max_seqlen": max_seqlen}


def ragged(rows):
    oo = [0]
    for r in rows:
        oo.append(oo[-1] + len(r))
    return np.array([i for r in rows for i in r], np.int64), np.array(oo, np.int64)


P = 9   # the pad id of the hand-made cases
DOCS = [[1, 20, 21, 22, 23, 24, 2], [1, 30, 2], [], [1, 40, 41, 42, 2]]


def check(e, input_ids, position_ids, segment_ids, cu_seqlens, max_seqlen, n_left):
    assert e["input_ids"].tolist() == input_ids
    assert e["position_ids"].tolist() == position_ids
    assert e["segment_ids"].tolist() == segment_ids
    assert e["cu_seqlens"].tolist() == cu_seqlens and e["cu_seqlens"].dtype == np.int32
    assert e["max_seqlen"] == max_seqlen and e["n_left"] == n_left
    assert e["n_segments"] == len(cu_seqlens) - 1 and e["n_rows"] == len(input_ids)


def test_hand_made_table():
    ids, oo = ragged(DOCS)
    inp4 = [[1, 20, 21, 22], [23, 24, 2, 1], [30, 2, 1, 40], [41, 42, 2, 9]]
    pos4 = [[0, 1, 2, 3], [0, 1, 2, 0], [0, 1, 0, 1], [0, 1, 2, 0]]
    seg4 = [[1, 1, 1, 1], [1, 1, 1, 2], [1, 1, 2, 2], [1, 1, 1, 0]]
    check(expected_packed(ids, oo, 4, P), inp4, pos4, seg4, [0, 4, 7, 8, 10, 12, 15], 4, 0)
    check(expected_packed(ids, oo, 4, P, ALL | DROP_LAST), inp4[:3], pos4[:3], seg4[:3], [0, 4, 7, 8, 10, 12], 4, 3)
    # L = 5: the document start at 10 coincides with a row start and appears once
    check(expected_packed(ids, oo, 5, P), [[1, 20, 21, 22, 23], [24, 2, 1, 30, 2], [1, 40, 41, 42, 2]],
          [[0, 1, 2, 3, 4], [0, 1, 0, 1, 2], [0, 1, 2, 3, 4]], [[1, 1, 1, 1, 1], [1, 1, 2, 2, 2], [1, 1, 1, 1, 1]], [0, 5, 7, 10, 15], 5, 0)
    check(expected_packed(ids, oo, 7, P), [[1, 20, 21, 22, 23, 24, 2], [1, 30, 2, 1, 40, 41, 42], [2, 9, 9, 9, 9, 9, 9]],
          [[0, 1, 2, 3, 4, 5, 6], [0, 1, 2, 0, 1, 2, 3], [0, 0, 0, 0, 0, 0, 0]],
          [[1] * 7, [1, 1, 1, 2, 2, 2, 2], [1, 0, 0, 0, 0, 0, 0]], [0, 7, 10, 14, 15], 7, 0)
    check(expected_packed(ids, oo, 16, P), [[1, 20, 21, 22, 23, 24, 2, 1, 30, 2, 1, 40, 41, 42, 2, 9]],
          [[0, 1, 2, 3, 4, 5, 6, 0, 1, 2, 0, 1, 2, 3, 4, 0]], [[1] * 7 + [2] * 3 + [3] * 5 + [0]], [0, 7, 10, 15], 7, 0)
    check(expected_packed(ids, oo, 1, P), [[i] for i in ids.tolist()], [[0]] * 15, [[1]] * 15, list(range(16)), 1, 0)


def test_hand_made_types_selection_and_invalid_options():
    ids, oo = ragged(DOCS)
    e = expected_packed(ids, oo, 4, P, ALL | I64)
    assert e["input_ids"].dtype == e["position_ids"].dtype == e["segment_ids"].dtype == np.int64 and e["cu_seqlens"].dtype == np.int32
    assert expected_packed(ids, oo, 4, P)["input_ids"].dtype == np.int32
    e = expected_packed(ids, oo, 4, P, 0)
    assert e["position_ids"] is None and e["segment_ids"] is None and e["cu_seqlens"] is None
    assert e["n_segments"] == 6 and e["max_seqlen"] == 4 and e["input_ids"].shape == (4, 4)
    for L, flags in ((0, ALL), (2 ** 31, ALL), (4, ALL | 32), (4, 1 << 31)):
        with pytest.raises(ValueError):
            expected_packed(ids, oo, L, P, flags)
    with pytest.raises(ValueError):                      # n_rows * L > 2^36 (nothing of that size is made before the check)
        expected_packed([], [0, 2 ** 36 + 1], 1, P, 0)
    with pytest.raises(ValueError):                      # cu_seqlens is int32
        expected_packed([], [0, 2 ** 32], 2 ** 30, P, CU_SEQLENS)


def test_hand_made_empty_shapes():
    for ids, oo in (([], [0]), ([], [0, 0, 0, 0])):      # D = 0; all-empty documents
        e = expected_packed(ids, oo, 4, P)
        assert e["input_ids"].shape == (0, 4) and e["cu_seqlens"].tolist() == [0]
        assert (e["n_rows"], e["n_used"], e["n_left"], e["n_segments"], e["max_seqlen"]) == (0, 0, 0, 0, 0)
    ids, oo = ragged(DOCS)
    e = expected_packed(ids, oo, 16, P, ALL | DROP_LAST)   # N < L with DROP_LAST
    assert e["n_rows"] == 0 and e["n_left"] == 15 and e["cu_seqlens"].tolist() == [0] and e["max_seqlen"] == 0


def random_ragged(rng, D, longest):
    n = rng.integers(0, longest, D)
    n[rng.integers(0, D, max(D // 8, 1))] = 0
    oo = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    return rng.integers(0, 1000, int(oo[-1])), oo


def test_invariants_on_random_input():
    rng = np.random.default_rng(12)
    for case in range(40):
        ids, oo = random_ragged(rng, int(rng.integers(1, 31)), int(rng.integers(1, 60)))
        L = int(rng.integers(1, 41))
        flags = ALL | (I64 if case & 1 else 0) | (DROP_LAST if case & 2 else 0)
        e = expected_packed(ids, oo, L, P, flags)
        N, n_used, cu = int(oo[-1]), e["n_used"], e["cu_seqlens"]
        assert n_used + e["n_left"] == N and e["input_ids"].shape == (e["n_rows"], L)
        assert e["n_rows"] == (N // L if flags & DROP_LAST else -(-N // L))
        flat = e["input_ids"].reshape(-1)
        assert np.array_equal(flat[:n_used], ids[:n_used]) and np.all(flat[n_used:] == P)
        assert cu[0] == 0 and cu[-1] == n_used and np.all(np.diff(cu) > 0) and len(cu) == e["n_segments"] + 1
        assert e["max_seqlen"] == (int(np.diff(cu).max()) if n_used else 0) and e["max_seqlen"] <= L
        pos, seg = e["position_ids"].reshape(-1), e["segment_ids"].reshape(-1)
        for i in range(e["n_segments"]):
            a, b = int(cu[i]), int(cu[i + 1])
            assert np.array_equal(pos[a:b], np.arange(b - a))
            assert np.all(seg[a:b] == seg[a]) and a // L == (b - 1) // L       # one number, one row
            assert seg[a] == (1 if a % L == 0 else seg[a - 1] + 1)
        assert np.array_equal(seg == 0, np.arange(len(seg)) >= n_used) and np.all(pos[n_used:] == 0)
        starts = set(cu[:-1].tolist())
        n = np.diff(oo)
        for d in range(len(n)):
            assert (int(oo[d]) in starts) or n[d] == 0 or oo[d] >= n_used or oo[d] % L == 0
            if n[d] > 0 and oo[d] < n_used:
                assert int(oo[d]) in starts
        assert all(r * L in starts for r in range(e["n_rows"]) if r * L < n_used)
        assert starts == {int(oo[d]) for d in range(len(n)) if n[d] > 0 and oo[d] < n_used} | {r * L for r in range(e["n_rows"]) if r * L < n_used}


def test_wave_search_model_against_bisect():
    """tools/seqpack_model.py restates the kernels' 64-ary search (64 probes a step, a ballot keeps one part): the count it
    returns, that the ballot is a prefix of the lanes at every step, and that it ends, at sizes on both sides of 64 and 64^2."""
    import bisect
    import seqpack_model
    rng = np.random.default_rng(13)
    for n in (0, 1, 2, 63, 64, 65, 127, 4095, 4096, 4097, 300_000):
        a = sorted(set(rng.integers(0, 10**7, n).tolist()))
        keys = rng.integers(0, 10**7, 100).tolist() + a[:3] + a[-3:] + [x + 1 for x in a[:3]] + [0, 10**8]
        for key in keys:
            assert seqpack_model.wave_count_le(a, len(a), key) == bisect.bisect_right(a, key), (n, key)


def test_new_symbols_declared_in_header_and_shim():
    hdr = open(os.path.join(ROOT, "include", "tekken_hip.h")).read()
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bfn\s+%s\s*\(" % name, ffi), name
    for name, value in FLAG_VALUES.items():
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name
        assert re.search(r"\bconst %s\s*:\s*\w+\s*=\s*%d\s*;" % (name, value), ffi), name
    assert re.search(r"typedef struct tk_seqpack_opts\b", hdr) and re.search(r"typedef struct tk_seqpack\b", hdr)
    assert re.search(r"\bstruct TkSeqpackOpts\b", ffi) and re.search(r"\bstruct TkSeqpack\b", ffi)


def test_python_constants_match_the_header(tk):
    assert (tk.SEQPACK_I64, tk.SEQPACK_POSITIONS, tk.SEQPACK_SEGMENTS, tk.SEQPACK_CU_SEQLENS, tk.SEQPACK_DROP_LAST) \
        == (I64, POSITIONS, SEGMENTS, CU_SEQLENS, DROP_LAST)
    for name in NEW_SYMBOLS:
        assert hasattr(tk.lib(), name), name
    for name in ("seqpack_from_ids_device", "encode_batch_device_seqpack", "encode_batch_seqpack"):
        assert hasattr(tk.Engine, name), name
    assert hasattr(tk, "SeqpackResult") and hasattr(tk.Tekkenizer, "encode_batch_packed")


def test_host_only_tokenizer_has_no_packed_batches(tk, small_vocab):
    from test_host_tokenizer import model
    t = tk.Tekkenizer.from_json(json.dumps(model(small_vocab["tokens"])), device=-1)
    for kw in ({}, {"return_tensors": "np"}, {"drop_last": True, "dtype": "int32"}):
        with pytest.raises(tk.TokenizerError) as e:
            t.encode_batch_packed(["hello world"], 4, **kw)
        assert e.value.code == tk.TK_ERR_NO_DEVICE
    t.close()
