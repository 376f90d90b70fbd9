"""Whole documents packed into rows without cutting them (include/tekken_hip.h tk_rowfit_from_ids_device), the parts that need no
GPU: the plain-loop restatement of the definition that tests/test_gpu_rowfit.py checks the kernels against, the hand-made cases
of the definition, the model of the doubling placement (tools/rowfit_model.py) against the plain loop, the Rust shim's
declarations, and the host-only tokenizer."""
import json
import os
import re

import numpy as np
import pytest

from test_seqpack_cpu import DOCS, P, ragged

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["tk_rowfit_from_ids_device", "tk_encode_batch_device_rowfit", "tk_encode_parts_device_rowfit", "tk_encode_batch_rowfit",
               "tk_free_rowfit", "tk_last_rowfit_ms"]
I64, POSITIONS, SEGMENTS, CU_SEQLENS, LABELS, DOC_START = 1, 2, 4, 8, 16, 32
ALL = POSITIONS | SEGMENTS | CU_SEQLENS | LABELS | DOC_START
FLAG_VALUES = {"TK_ROWFIT_I64": 1, "TK_ROWFIT_POSITIONS": 2, "TK_ROWFIT_SEGMENTS": 4, "TK_ROWFIT_CU_SEQLENS": 8, "TK_ROWFIT_LABELS": 16,
               "TK_ROWFIT_DOC_START": 32}
IGN = -100


def next_fit(lengths, L):
    """Step 2 of the definition, as written there.  -> (doc_start, n_rows)"""
    r, fill, doc_start = -1, L, []
    for n in lengths:
        e = min(n, L)
        if e > 0 and fill + e > L:
            r, fill = r + 1, 0
        doc_start.append(r * L + fill)
        fill += e
    return doc_start, r + 1


def expected_rowfit(ids, oo, lab, seq_len, pad_id, ignore_index=IGN, keep_tail=0, flags=ALL):
    """The definition, restated document by document with plain loops (no prefix sum, no search).  -> dict(input_ids,
    position_ids, segment_ids [n_rows, L] int32 / int64, labels [n_rows, L] int32, cu_seqlens int32 [n_segments + 1], doc_start
    uint64 [D] (an unselected one: None), n_rows, n_segments, max_seqlen, n_truncated, n_pad).  Invalid options raise ValueError
    (the entries: TK_ERR_INVALID_ARG)."""
    oo = [int(x) for x in oo]
    L, D, N = int(seq_len), len(oo) - 1, int(oo[-1])
    if L <= 0 or L >= 2 ** 31 or flags & ~(I64 | ALL) or keep_tail > L:
        raise ValueError("seq_len / flags / keep_tail")
    if flags & LABELS and lab is None and N > 0:
        raise ValueError("labels without a labels stream")
    lengths = [oo[d + 1] - oo[d] for d in range(D)]
    doc_start, n_rows = next_fit(lengths, L)
    if n_rows * L > 2 ** 36:
        raise ValueError("tensor too large")
    if flags & CU_SEQLENS and n_rows * L >= 2 ** 31:
        raise ValueError("cu_seqlens is int32")
    total = n_rows * L
    inp, labels, pos, seg = [pad_id] * total, [ignore_index] * total, [0] * total, [0] * total
    src = np.asarray(ids, np.int64).tolist()
    lsrc = np.asarray(lab, np.int64).tolist() if lab is not None else None
    n_truncated, used = 0, 0
    in_row = {}                                           # non-empty documents placed in each row so far
    starts = []
    for d in range(D):
        n, e = lengths[d], min(lengths[d], L)
        n_truncated += n > L
        if e == 0:
            continue
        r = doc_start[d] // L
        in_row[r] = in_row.get(r, 0) + 1
        starts.append(doc_start[d])
        for k in range(e):
            s = oo[d] + k if k < L - keep_tail or n <= L else oo[d] + n - (L - k)
            g = doc_start[d] + k
            inp[g], pos[g], seg[g] = src[s], k, in_row[r]
            if lsrc is not None:
                labels[g] = lsrc[s]
        used += e
    is_pad = [True] * total
    for d in range(D):
        for k in range(min(lengths[d], L)):
            is_pad[doc_start[d] + k] = False
    for r in range(n_rows):                               # the row's pad run: from its first pad to its end
        for c in range(L):
            if is_pad[r * L + c]:
                starts.append(r * L + c)
                break
    cu = sorted(starts) + [total]
    n_segments = len(cu) - 1
    max_seqlen = 0
    for i in range(n_segments):
        max_seqlen = max(max_seqlen, cu[i + 1] - cu[i])
    dt = np.int64 if flags & I64 else np.int32
    shape = (n_rows, L)
    return {"input_ids": np.array(inp, dt).reshape(shape),
            "labels": np.array(labels, np.int32).reshape(shape) if flags & LABELS else None,
            "position_ids": np.array(pos, dt).reshape(shape) if flags & POSITIONS else None,
            "segment_ids": np.array(seg, dt).reshape(shape) if flags & SEGMENTS else None,
            "cu_seqlens": np.array(cu, np.int32) if flags & CU_SEQLENS else None,
            "doc_start": np.array(doc_start, np.uint64) if flags & DOC_START else None,
            "n_rows": n_rows, "n_segments": n_segments, "max_seqlen": max_seqlen, "n_truncated": n_truncated, "n_pad": total - used}


def fit(rows, L, keep_tail=0, flags=ALL, lab=True):
    ids, oo = ragged(rows)
    return expected_rowfit(ids, oo, -ids - 1 if lab else None, L, P, IGN, keep_tail, flags)


def check(e, input_ids, position_ids, segment_ids, cu_seqlens, doc_start, max_seqlen, n_truncated=0):
    assert e["input_ids"].tolist() == input_ids
    assert e["position_ids"].tolist() == position_ids
    assert e["segment_ids"].tolist() == segment_ids
    assert e["labels"].tolist() == [[IGN if x == P else -x - 1 for x in row] for row in input_ids] and e["labels"].dtype == np.int32
    assert e["cu_seqlens"].tolist() == cu_seqlens and e["cu_seqlens"].dtype == np.int32
    assert e["doc_start"].tolist() == doc_start and e["doc_start"].dtype == np.uint64
    assert e["max_seqlen"] == max_seqlen and e["n_truncated"] == n_truncated
    assert e["n_segments"] == len(cu_seqlens) - 1 and e["n_rows"] == len(input_ids)
    assert e["n_pad"] == sum(row.count(P) for row in input_ids)


def test_hand_made_table():
    # DOCS = [7 ids], [3 ids], [], [5 ids] (tests/test_seqpack_cpu.py); no id of theirs is the pad id
    a, b, c = DOCS[0], DOCS[1], DOCS[3]
    check(fit(DOCS, 7), [a, b + [P] * 4, c + [P] * 2], [[0, 1, 2, 3, 4, 5, 6], [0, 1, 2, 0, 0, 0, 0], [0, 1, 2, 3, 4, 0, 0]],
          [[1] * 7, [1, 1, 1, 0, 0, 0, 0], [1, 1, 1, 1, 1, 0, 0]], [0, 7, 10, 14, 19, 21], [0, 7, 10, 14], 7)
    check(fit(DOCS, 8), [a + [P], b + c], [[0, 1, 2, 3, 4, 5, 6, 0], [0, 1, 2, 0, 1, 2, 3, 4]],
          [[1] * 7 + [0], [1, 1, 1, 2, 2, 2, 2, 2]], [0, 7, 8, 11, 16], [0, 8, 11, 11], 7)
    check(fit(DOCS, 16), [a + b + c + [P]], [[0, 1, 2, 3, 4, 5, 6, 0, 1, 2, 0, 1, 2, 3, 4, 0]], [[1] * 7 + [2] * 3 + [3] * 5 + [0]],
          [0, 7, 10, 15, 16], [0, 7, 10, 10], 7)


def test_hand_made_exact_fit_and_miss_by_one():
    check(fit([[1, 2, 3], [4, 5]], 5), [[1, 2, 3, 4, 5]], [[0, 1, 2, 0, 1]], [[1, 1, 1, 2, 2]], [0, 3, 5], [0, 3], 3)
    check(fit([[1, 2, 3], [4, 5, 6]], 5), [[1, 2, 3, P, P], [4, 5, 6, P, P]], [[0, 1, 2, 0, 0]] * 2, [[1, 1, 1, 0, 0]] * 2,
          [0, 3, 5, 8, 10], [0, 5], 3)
    check(fit([[1], [2], [3]], 1), [[1], [2], [3]], [[0]] * 3, [[1]] * 3, [0, 1, 2, 3], [0, 1, 2], 1)   # L = 1


def test_hand_made_empty_documents():
    # leading, middle and trailing empty documents; empties behind an exactly full row start where the next id would go
    check(fit([[], [], [1, 2], [], [3, 4], [], [], [5], []], 4), [[1, 2, 3, 4], [5, P, P, P]], [[0, 1, 0, 1], [0, 0, 0, 0]],
          [[1, 1, 2, 2], [1, 0, 0, 0]], [0, 2, 4, 5, 8], [0, 0, 0, 2, 2, 4, 4, 4, 5], 3)
    check(fit([[1, 2, 3, 4], [], []], 4), [[1, 2, 3, 4]], [[0, 1, 2, 3]], [[1] * 4], [0, 4], [0, 4, 4], 4)
    for rows in ([], [[], [], []]):                       # D = 0; all documents empty
        e = fit(rows, 4)
        assert e["input_ids"].shape == e["labels"].shape == (0, 4) and e["cu_seqlens"].tolist() == [0]
        assert e["doc_start"].tolist() == [0] * len(rows)
        assert (e["n_rows"], e["n_segments"], e["max_seqlen"], e["n_truncated"], e["n_pad"]) == (0, 0, 0, 0, 0)


def test_hand_made_over_long_documents():
    long = [1, 2, 3, 4, 5, 6, 7]
    for keep_tail, kept in ((0, [1, 2, 3, 4]), (1, [1, 2, 3, 7]), (4, [4, 5, 6, 7])):
        check(fit([[8], long, [10, 11]], 4, keep_tail), [[8, P, P, P], kept, [10, 11, P, P]], [[0, 0, 0, 0], [0, 1, 2, 3], [0, 1, 0, 0]],
              [[1, 0, 0, 0], [1] * 4, [1, 1, 0, 0]], [0, 1, 4, 8, 10, 12], [0, 4, 8], 4, 1)
    # a document of exactly L ids is not truncated, whatever keep_tail says
    check(fit([[1, 2, 3, 4]], 4, 4), [[1, 2, 3, 4]], [[0, 1, 2, 3]], [[1] * 4], [0, 4], [0], 4, 0)


def test_hand_made_types_selection_and_invalid_options():
    ids, oo = ragged(DOCS)
    e = expected_rowfit(ids, oo, ids, 8, P, IGN, 0, ALL | I64)
    assert e["input_ids"].dtype == e["position_ids"].dtype == e["segment_ids"].dtype == np.int64
    assert e["labels"].dtype == e["cu_seqlens"].dtype == np.int32
    e = expected_rowfit(ids, oo, None, 8, P, IGN, 0, 0)
    assert all(e[k] is None for k in ("labels", "position_ids", "segment_ids", "cu_seqlens", "doc_start"))
    assert e["n_segments"] == 4 and e["max_seqlen"] == 7 and e["input_ids"].shape == (2, 8) and e["input_ids"].dtype == np.int32
    for L, keep_tail, flags, lab in ((0, 0, ALL, ids), (2 ** 31, 0, ALL, ids), (8, 0, ALL | 64, ids), (8, 0, 1 << 31, ids), (8, 9, ALL, ids),
                                     (8, 0, LABELS, None)):
        with pytest.raises(ValueError):
            expected_rowfit(ids, oo, lab, L, P, IGN, keep_tail, flags)
    assert expected_rowfit([], [0, 0], None, 8, P, IGN, 0, LABELS)["n_rows"] == 0      # N == 0: no labels stream is needed
    half = 2 ** 29 + 1                                    # three documents of L // 2 + 1 ids: 3 rows of 2^30 (nothing of that size is made before the check)
    with pytest.raises(ValueError):
        expected_rowfit([], [0, half, 2 * half, 3 * half], None, 2 ** 30, P, IGN, 0, CU_SEQLENS)
    with pytest.raises(ValueError):                       # n_rows * L > 2^36
        expected_rowfit([], [0] + [half * (i + 1) for i in range(65)], None, 2 ** 30, P, IGN, 0, 0)


def random_lengths(rng, D, L):
    """Empty, exact-fit, over-long and L // 2 + 1 documents among random ones."""
    n = rng.integers(0, max(2 * L // 3, 2), D)
    for special in (0, L, L + 1, 3 * L, L // 2 + 1, 1):
        n[rng.integers(0, D, max(D // 10, 1))] = special
    if rng.integers(0, 3) == 0:
        a = int(rng.integers(0, D))
        n[a:a + int(rng.integers(1, 80))] = 0
    return n


def test_invariants_on_random_input():
    rng = np.random.default_rng(21)
    for case in range(40):
        D, L = int(rng.integers(1, 40)), int(rng.integers(1, 41))
        n = random_lengths(rng, D, L)
        oo = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        ids = rng.integers(10, 1000, int(oo[-1]))
        lab = rng.integers(-50, 1000, int(oo[-1]))
        lab[lab == IGN] = 0
        keep_tail = int(rng.integers(0, L + 1))
        e = expected_rowfit(ids, oo, lab, L, P, IGN, keep_tail, ALL | (I64 if case & 1 else 0))
        R, ds, cu = e["n_rows"], e["doc_start"].astype(np.int64), e["cu_seqlens"]
        flat, labels = e["input_ids"].reshape(-1), e["labels"].reshape(-1)
        covered = np.zeros(R * L, bool)
        assert np.all(np.diff(ds) >= 0)
        for d in range(D):
            k = min(int(n[d]), L)
            if k == 0:
                continue
            a = int(ds[d])
            assert a // L == (a + k - 1) // L and not covered[a:a + k].any()      # contiguous in one row, on nobody's ground
            covered[a:a + k] = True
            doc, dl = ids[oo[d]:oo[d + 1]], lab[oo[d]:oo[d + 1]]
            if n[d] > L:
                doc, dl = np.concatenate([doc[:L - keep_tail], doc[n[d] - keep_tail:]]), np.concatenate([dl[:L - keep_tail], dl[n[d] - keep_tail:]])
            assert np.array_equal(flat[a:a + k], doc) and np.array_equal(labels[a:a + k], dl)
            assert np.array_equal(e["position_ids"].reshape(-1)[a:a + k], np.arange(k))
        assert np.all(flat[~covered] == P) and np.array_equal(labels == IGN, ~covered)
        assert np.array_equal(e["segment_ids"].reshape(-1) == 0, ~covered)
        assert e["n_pad"] == int((~covered).sum()) and e["n_truncated"] == int((n > L).sum())
        assert cu[0] == 0 and cu[-1] == R * L and np.all(np.diff(cu) > 0) and len(cu) == e["n_segments"] + 1
        assert e["max_seqlen"] == (int(np.diff(cu).max()) if R else 0)
        for i in range(e["n_segments"]):                  # a segment is one document or one pad run
            a, b = int(cu[i]), int(cu[i + 1])
            assert covered[a:b].all() or not covered[a:b].any()
        # no row could have taken the next row's first document
        first = {}
        for d in range(D):
            if n[d] > 0:
                first.setdefault(int(ds[d]) // L, min(int(n[d]), L))
        for r in range(R - 1):
            assert int(covered[r * L:(r + 1) * L].sum()) + first[r + 1] > L


def test_doubling_model_against_the_plain_loop():
    """tools/rowfit_model.py restates the kernels' placement (prefix sum, one search per document, pointer doubling with exact
    step counts, the wave's prefix maximum): it equals the plain loop on random inputs, in any order of the nodes of a round."""
    import rowfit_model
    rng = np.random.default_rng(22)
    for case in range(300):
        D, L = int(rng.integers(1, 200)), int(rng.integers(1, 50))
        n = random_lengths(rng, D, L).tolist()
        order = None
        if case % 3 == 1:
            order = lambda k, m: range(m - 1, -1, -1)
        elif case % 3 == 2:
            order = lambda k, m: rng.permutation(m).tolist()
        ds, n_rows, _ = rowfit_model.place(n, L, order)
        assert (ds, n_rows) == next_fit(n, L), (case, n, L)
    for case in range(20_000):                            # many small ones: every mix of empty, exact-fit, over-long and half-row documents
        D, L = int(rng.integers(1, 24)), int(rng.integers(1, 12))
        n = random_lengths(rng, D, L).tolist()
        ds, n_rows, _ = rowfit_model.place(n, L, (lambda k, m: range(m - 1, -1, -1)) if case & 1 else None)
        assert (ds, n_rows) == next_fit(n, L), (case, n, L)


@pytest.mark.parametrize("n_rows", [1, 2, 3, 4, 5, 1023, 1024, 1025])
def test_doubling_model_rounds_across_powers_of_two(n_rows):
    """Documents of L // 2 + 1 ids: each gets a row of its own and the chain has n_rows links."""
    import rowfit_model
    for L in (8, 9):
        n = [L // 2 + 1] * n_rows
        ds, got, rounds = rowfit_model.place(n, L)
        assert got == n_rows and ds == [r * L for r in range(n_rows)] and (ds, got) == next_fit(n, L)
        assert rounds == n_rows.bit_length()              # the smallest K with 2^K > n_rows: ceil(log2(n_rows)) + 1 at most


def test_new_symbols_declared_in_header_and_shim():
    hdr = open(os.path.join(ROOT, "include", "tekken_hip.h")).read()
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bfn\s+%s\s*\(" % name, ffi), name
    for name, value in FLAG_VALUES.items():
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name
        assert re.search(r"\bconst %s\s*:\s*\w+\s*=\s*%d\s*;" % (name, value), ffi), name
    assert re.search(r"typedef struct tk_rowfit_opts\b", hdr) and re.search(r"typedef struct tk_rowfit\b", hdr)
    assert re.search(r"\bstruct TkRowfitOpts\b", ffi) and re.search(r"\bstruct TkRowfit\b", ffi)


def test_python_constants_match_the_header(tk):
    assert (tk.ROWFIT_I64, tk.ROWFIT_POSITIONS, tk.ROWFIT_SEGMENTS, tk.ROWFIT_CU_SEQLENS, tk.ROWFIT_LABELS, tk.ROWFIT_DOC_START) \
        == (I64, POSITIONS, SEGMENTS, CU_SEQLENS, LABELS, DOC_START)
    for name in NEW_SYMBOLS:
        assert hasattr(tk.lib(), name), name
    for name in ("rowfit_from_ids_device", "encode_batch_device_rowfit", "encode_batch_rowfit"):
        assert hasattr(tk.Engine, name), name
    assert hasattr(tk, "RowfitResult") and hasattr(tk.RowfitResult, "views")
    assert hasattr(tk.Tekkenizer, "encode_batch_packed_whole") and hasattr(tk.Tekkenizer, "encode_chat_packed")


def test_host_only_tokenizer_has_no_whole_document_rows(tk, small_vocab):
    from test_host_tokenizer import model
    t = tk.Tekkenizer.from_json(json.dumps(model(small_vocab["tokens"])), device=-1)
    for kw in ({}, {"return_tensors": "np"}, {"dtype": "int32", "add_eos": False}):
        with pytest.raises(tk.TokenizerError) as e:
            t.encode_batch_packed_whole(["hello world"], 4, **kw)
        assert e.value.code == tk.TK_ERR_NO_DEVICE
    with pytest.raises(tk.TokenizerError) as e:
        t.encode_chat_packed([[{"role": "user", "content": "hi"}, {"role": "assistant", "content": "yo"}]], 8)
    assert e.value.code == tk.TK_ERR_NO_DEVICE
    t.close()
