"""Model-ready dense batches (include/tekken_hip.h tk_dense_from_ids_device), the parts that need no GPU: the numpy restatement of
the definition that tests/test_gpu_dense.py checks the kernels against, the Rust shim's declarations, and the host-only tokenizer."""
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["tk_dense_from_ids_device", "tk_encode_batch_device_dense", "tk_encode_batch_dense", "tk_free_dense",
               "tk_ragged_from_dense_device"]
PAD_LEFT, TRUNC_LEFT, FIXED, I64, MASK = 1, 2, 4, 8, 16
FLAG_VALUES = {"TK_DENSE_PAD_LEFT": 1, "TK_DENSE_TRUNC_LEFT": 2, "TK_DENSE_FIXED": 4, "TK_DENSE_I64": 8, "TK_DENSE_MASK": 16}


def kept_ids(R, T, h, t, trunc_left):
    """Step 2 of the definition for one document (R: its ids as a list / array)."""
    n = len(R)
    if T == 0 or n <= T:
        return list(R)
    if trunc_left:
        return list(R[:h]) + list(R[n - (T - h):])
    return list(R[:T - t]) + list(R[n - t:] if t else [])


def expected_dense(ids, oo, max_length=0, multiple_of=0, pad_id=0, keep_head=0, keep_tail=0, flags=0):
    """The definition, restated document by document.  -> dict(dense [D, L] int32 / int64, mask uint8 [D, L] or None,
    lengths uint32 [D], row_len, n_truncated).  Invalid options raise ValueError (the entries: TK_ERR_INVALID_ARG)."""
    ids = np.asarray(ids, np.int64)
    oo = np.asarray(oo, np.int64)
    D, T = len(oo) - 1, int(max_length)
    left = bool(flags & TRUNC_LEFT)
    if (flags & FIXED) and T == 0:
        raise ValueError("FIXED needs max_length")
    if T > 0 and (keep_head > T if left else keep_tail > T):
        raise ValueError("keep_head / keep_tail exceed max_length")
    K = [kept_ids(ids[oo[d]:oo[d + 1]], T, keep_head, keep_tail, left) for d in range(D)]
    n = np.diff(oo)
    if flags & FIXED:
        L = T
    else:
        L = int(n.max()) if D else 0
        if T > 0:
            L = min(L, T)
    if multiple_of:
        L = (L + multiple_of - 1) // multiple_of * multiple_of
    dense = np.full((D, L), pad_id, np.int64 if flags & I64 else np.int32)
    mask = np.zeros((D, L), np.uint8)
    for d, k in enumerate(K):
        if flags & PAD_LEFT:
            dense[d, L - len(k):] = k
            mask[d, L - len(k):] = 1
        else:
            dense[d, :len(k)] = k
            mask[d, :len(k)] = 1
    return {"dense": dense, "mask": mask if flags & MASK else None, "lengths": np.array([len(k) for k in K], np.uint32),
            "row_len": L, "n_truncated": int((n > T).sum()) if T > 0 else 0}


def expected_ragged(dense, lengths, pad_id, pad_left):
    """The inverse: (ids uint32[T], offsets uint64[D + 1]).  lengths None: the maximal run of pad_id at the padded end goes."""
    dense = np.asarray(dense)
    D, L = dense.shape
    rows = []
    for d in range(D):
        row = dense[d]
        if lengths is None:
            k = L
            if pad_left:
                while k > 0 and row[L - k] == pad_id:
                    k -= 1
            else:
                while k > 0 and row[k - 1] == pad_id:
                    k -= 1
        else:
            k = int(lengths[d])
        rows.append(row[L - k:] if pad_left else row[:k])
    oo = np.zeros(D + 1, np.uint64)
    if D:
        oo[1:] = np.cumsum([len(r) for r in rows])
    flat = np.concatenate(rows).astype(np.uint32) if D and int(oo[-1]) else np.zeros(0, np.uint32)
    return flat, oo


def ragged(rows):
    oo = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return np.array([i for r in rows for i in r], np.int64), oo


P = 9   # the pad id of the hand-made cases
ROWS = [[1, 20, 21, 22, 23, 24, 2], [1, 30, 2], [], [1, 40, 41, 42, 2]]   # 7, 3, 0 and 5 ids


def test_hand_made_right_truncation_with_head_and_tail():
    ids, oo = ragged(ROWS)
    # t = 0, 1, 2 at lim = 5: the first lim - t ids and the last t
    for t, row0 in ((0, [1, 20, 21, 22, 23]), (1, [1, 20, 21, 22, 2]), (2, [1, 20, 21, 24, 2])):
        e = expected_dense(ids, oo, max_length=5, pad_id=P, keep_head=2, keep_tail=t, flags=MASK)   # (keep_head: unused on the right)
        assert e["dense"].tolist() == [row0, [1, 30, 2, P, P], [P] * 5, [1, 40, 41, 42, 2]]
        assert e["mask"].tolist() == [[1] * 5, [1, 1, 1, 0, 0], [0] * 5, [1] * 5]
        assert e["lengths"].tolist() == [5, 3, 0, 5] and e["row_len"] == 5 and e["n_truncated"] == 1   # n_d == lim exactly: not truncated
        assert e["dense"].dtype == np.int32


def test_hand_made_left_truncation_with_head_and_tail():
    ids, oo = ragged(ROWS)
    for h, row0 in ((0, [22, 23, 24, 2]), (1, [1, 23, 24, 2]), (2, [1, 20, 24, 2])):
        e = expected_dense(ids, oo, max_length=4, pad_id=P, keep_head=h, keep_tail=2, flags=TRUNC_LEFT | I64)
        row3 = {0: [40, 41, 42, 2], 1: [1, 41, 42, 2], 2: [1, 40, 42, 2]}[h]
        assert e["dense"].tolist() == [row0, [1, 30, 2, P], [P] * 4, row3]
        assert e["mask"] is None and e["n_truncated"] == 2 and e["dense"].dtype == np.int64
        assert e["lengths"].tolist() == [4, 3, 0, 4]


def test_hand_made_lim_equals_head_plus_tail():
    ids, oo = ragged(ROWS)
    e = expected_dense(ids, oo, max_length=2, pad_id=P, keep_tail=1)                 # h + t == lim in the fused form: BOS, EOS
    assert e["dense"].tolist() == [[1, 2], [1, 2], [P, P], [1, 2]]
    e = expected_dense(ids, oo, max_length=2, pad_id=P, keep_head=1, flags=TRUNC_LEFT)
    assert e["dense"].tolist() == [[1, 2], [1, 2], [P, P], [1, 2]]
    e = expected_dense(ids, oo, max_length=2, pad_id=P, keep_tail=2)                 # t == lim: nothing of the head
    assert e["dense"].tolist() == [[24, 2], [30, 2], [P, P], [42, 2]]
    e = expected_dense(ids, oo, max_length=2, pad_id=P, keep_head=2, flags=TRUNC_LEFT)
    assert e["dense"].tolist() == [[1, 20], [1, 30], [P, P], [1, 40]]
    for kw in (dict(keep_tail=3), dict(keep_head=3, flags=TRUNC_LEFT), dict(max_length=0, flags=FIXED)):
        with pytest.raises(ValueError):
            expected_dense(ids, oo, **{"max_length": 2, **kw})
    expected_dense(ids, oo, max_length=2, keep_head=3)            # (the head is not used on the right)


def test_hand_made_padding_sides_multiple_of_and_fixed():
    ids, oo = ragged(ROWS)
    e = expected_dense(ids, oo, max_length=5, pad_id=P, keep_tail=1, flags=PAD_LEFT | MASK)
    assert e["dense"].tolist() == [[1, 20, 21, 22, 2], [P, P, 1, 30, 2], [P] * 5, [1, 40, 41, 42, 2]]
    assert e["mask"].tolist() == [[1] * 5, [0, 0, 1, 1, 1], [0] * 5, [1] * 5]
    # multiple_of: the row grows, the truncation stays at lim
    e = expected_dense(ids, oo, max_length=5, multiple_of=4, pad_id=P, keep_tail=1, flags=MASK)
    assert e["row_len"] == 8 and e["dense"][0].tolist() == [1, 20, 21, 22, 2, P, P, P] and e["lengths"].tolist() == [5, 3, 0, 5]
    e = expected_dense(ids, oo, max_length=0, multiple_of=4, pad_id=P, flags=PAD_LEFT)
    assert e["row_len"] == 8 and e["dense"][0].tolist() == [P, 1, 20, 21, 22, 23, 24, 2] and e["n_truncated"] == 0
    # longest mode: L = min(longest, lim)
    assert expected_dense(ids, oo, max_length=100, pad_id=P)["row_len"] == 7
    assert expected_dense(ids, oo, max_length=0, pad_id=P)["row_len"] == 7
    # FIXED with every document shorter
    e = expected_dense(ids, oo, max_length=9, pad_id=P, flags=FIXED | MASK)
    assert e["dense"].shape == (4, 9) and e["n_truncated"] == 0 and e["dense"][1].tolist() == [1, 30, 2] + [P] * 6
    assert e["mask"].sum(1).tolist() == [7, 3, 0, 5]
    e = expected_dense(ids, oo, max_length=9, multiple_of=8, pad_id=P, flags=FIXED)
    assert e["row_len"] == 16


def test_hand_made_empty_shapes():
    e = expected_dense([], [0], max_length=0, pad_id=P, flags=MASK)                 # D = 0
    assert e["dense"].shape == (0, 0) and e["mask"].shape == (0, 0) and e["lengths"].shape == (0,) and e["n_truncated"] == 0
    e = expected_dense([], [0], max_length=6, pad_id=P, flags=FIXED)
    assert e["dense"].shape == (0, 6)
    e = expected_dense([], [0, 0, 0, 0], max_length=0, multiple_of=8, pad_id=P, flags=MASK)   # all-empty documents: L = 0
    assert e["dense"].shape == (3, 0) and e["lengths"].tolist() == [0, 0, 0]
    e = expected_dense([], [0, 0, 0], max_length=4, pad_id=P, flags=FIXED | MASK)
    assert e["dense"].tolist() == [[P] * 4] * 2 and e["mask"].sum() == 0
    flat, oo = expected_ragged(np.zeros((0, 5), np.int32), None, P, False)
    assert len(flat) == 0 and oo.tolist() == [0]
    flat, oo = expected_ragged(np.zeros((2, 0), np.int32), None, P, False)
    assert len(flat) == 0 and oo.tolist() == [0, 0, 0]


def test_hand_made_inverse():
    dense = np.array([[1, 5, P, 2, P, P], [P, P, P, P, P, P], [P, 3, 4, 5, 6, 7]], np.int64)
    flat, oo = expected_ragged(dense, None, P, False)
    assert flat.tolist() == [1, 5, P, 2, P, 3, 4, 5, 6, 7] and oo.tolist() == [0, 4, 4, 10]     # (a pad inside a row stays)
    flat, oo = expected_ragged(dense, None, P, True)
    assert flat.tolist() == [1, 5, P, 2, P, P, 3, 4, 5, 6, 7] and oo.tolist() == [0, 6, 6, 11]
    flat, oo = expected_ragged(dense, [2, 0, 3], P, False)
    assert flat.tolist() == [1, 5, P, 3, 4] and oo.tolist() == [0, 2, 2, 5]
    flat, oo = expected_ragged(dense, [2, 0, 3], P, True)
    assert flat.tolist() == [P, P, 5, 6, 7] and oo.tolist() == [0, 2, 2, 5]
    assert flat.dtype == np.uint32 and oo.dtype == np.uint64


def random_ragged(rng, D, longest, pad_id):
    n = rng.integers(0, longest, D)
    n[rng.integers(0, D, max(D // 8, 1))] = 0
    oo = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    ids = rng.integers(0, 1000, int(oo[-1]))
    ids[ids == pad_id] += 1                          # (a document that ends in pad_id does not survive the pad trim)
    return ids, oo


def test_invariants_on_random_input():
    rng = np.random.default_rng(11)
    for case in range(40):
        ids, oo = random_ragged(rng, int(rng.integers(1, 30)), int(rng.integers(1, 60)), P)
        n = np.diff(oo)
        T = int(rng.integers(0, 40))
        h, t = (int(x) for x in rng.integers(0, 4, 2))
        flags = int(rng.integers(0, 4)) | MASK | (I64 if case & 1 else 0)      # the two sides, both ways
        if T and (h if flags & TRUNC_LEFT else t) > T:
            continue
        e = expected_dense(ids, oo, T, int(rng.integers(0, 9)), P, h, t, flags)
        k = np.minimum(n, T) if T else n
        assert np.array_equal(e["lengths"], k)
        assert np.array_equal(e["mask"].sum(1), e["lengths"])
        assert np.all(e["dense"][e["mask"] == 0] == P)
        assert e["n_truncated"] == (int((n > T).sum()) if T else 0)
        for d in range(len(n)):
            R = ids[oo[d]:oo[d + 1]]
            row = e["dense"][d][e["mask"][d] == 1]
            if n[d] > k[d]:
                if flags & TRUNC_LEFT:
                    assert np.array_equal(row[:h], R[:h]) and np.array_equal(row[h:], R[n[d] - (T - h):])
                else:
                    assert np.array_equal(row[:T - t], R[:T - t]) and np.array_equal(row[T - t:], R[n[d] - t:][:t])
            else:
                assert np.array_equal(row, R)
        # the round trip at T = 0, with the lengths and with the pad trim
        e0 = expected_dense(ids, oo, 0, int(rng.integers(0, 9)), P, h, t, flags)
        for lengths in (e0["lengths"], None):
            flat, roo = expected_ragged(e0["dense"], lengths, P, bool(flags & PAD_LEFT))
            assert np.array_equal(flat, ids) and np.array_equal(roo, oo)


def test_new_symbols_declared_in_header_and_shim():
    hdr = open(os.path.join(ROOT, "include", "tekken_hip.h")).read()
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bfn\s+%s\s*\(" % name, ffi), name
    for name, value in FLAG_VALUES.items():
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name
        assert re.search(r"\bconst %s\s*:\s*\w+\s*=\s*%d\s*;" % (name, value), ffi), name
    assert re.search(r"typedef struct tk_dense_opts\b", hdr) and re.search(r"typedef struct tk_dense\b", hdr)
    assert re.search(r"\bstruct TkDenseOpts\b", ffi) and re.search(r"\bstruct TkDense\b", ffi)


def test_python_constants_match_the_header(tk):
    assert (tk.DENSE_PAD_LEFT, tk.DENSE_TRUNC_LEFT, tk.DENSE_FIXED, tk.DENSE_I64, tk.DENSE_MASK) == (PAD_LEFT, TRUNC_LEFT, FIXED, I64, MASK)
    for name in NEW_SYMBOLS:
        assert hasattr(tk.lib(), name), name
    v = tk.DeviceView(4096, (3, 5), "<i4").__cuda_array_interface__          # the 2-D form, and the old one unchanged
    assert v["shape"] == (3, 5) and tk.DeviceView(4096, 7, "<i4").__cuda_array_interface__["shape"] == (7,)


def test_host_only_tokenizer_has_no_padded_batches(tk, small_vocab):
    from test_host_tokenizer import model
    t = tk.Tekkenizer.from_json(json.dumps(model(small_vocab["tokens"])), device=-1)
    for kw in ({}, {"return_tensors": "np"}, {"max_length": 4, "padding": "max_length"}):
        with pytest.raises(tk.TokenizerError) as e:
            t.encode_batch_padded(["hello world"], True, True, **kw)
        assert e.value.code == tk.TK_ERR_NO_DEVICE
    with pytest.raises(tk.TokenizerError) as e:
        t.decode_batch_padded(np.zeros((1, 4), np.int64))
    assert e.value.code == tk.TK_ERR_NO_DEVICE
    t.close()
