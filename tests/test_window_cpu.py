"""Overlapping windows for long documents (include/tekken_hip.h tk_window_from_ids_device), the parts that need no GPU: the
plain-loop restatement of the definition that tests/test_gpu_window.py checks the kernels against, the hand-made cases of the
definition, the Rust shim's declarations, and the host-only tokenizer."""
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["tk_window_from_ids_device", "tk_encode_batch_device_window", "tk_encode_batch_window", "tk_free_window"]
FIXED, I64, MASK, SPANS = 1, 2, 4, 8
FLAG_VALUES = {"TK_WINDOW_FIXED": 1, "TK_WINDOW_I64": 2, "TK_WINDOW_MASK": 4, "TK_WINDOW_SPANS": 8}
MAX_ROW, MAX_ELEMS = 2 ** 31 - 1, 2 ** 36


def expected_windows(ids, oo, T, s, h, t, m, pad_id, flags, spans=None):
    """The definition, restated document by document with plain loops: the windows of a split document are walked until one
    reaches the end of its body (no cumulative sum, no closed form for their number).  spans: [N, 2] or None.  -> dict(input_ids
    [W, L] int32 / int64, mask uint8 [W, L] or None, lengths, window_doc, window_start uint32 [W], doc_windows uint64 [D + 1],
    spans uint32 [W, L, 2] or None, n_windows, n_split, row_len).  Invalid options raise ValueError (the entries:
    TK_ERR_INVALID_ARG)."""
    oo = [int(x) for x in oo]
    T, s, h, t, m, D = int(T), int(s), int(h), int(t), int(m or 0), len(oo) - 1
    if T <= 0 or T > MAX_ROW or h < 0 or t < 0 or h + t >= T or flags & ~(FIXED | I64 | MASK | SPANS):
        raise ValueError("max_length / keep_head / keep_tail / flags")
    c = T - h - t
    if not 0 <= s < c:
        raise ValueError("stride")
    step = c - s
    if flags & SPANS and spans is None:
        raise ValueError("no spans buffer")
    if D == 0 and len(ids):
        raise ValueError("ids without a document")
    longest = 0
    for d in range(D):
        longest = max(longest, oo[d + 1] - oo[d])
    if longest >= 2 ** 32 - 1:
        raise ValueError("window_start is uint32")
    L = T if flags & FIXED else min(longest, T)
    if m:
        L = (L + m - 1) // m * m
    if L > MAX_ROW:
        raise ValueError("row too long")
    # a window holds at most c body ids, so a split document has at least ceil(b / c) of them: where that bound alone is beyond
    # what a tensor holds, refuse before walking (the walk below decides every other case exactly)
    at_least = 0
    for d in range(D):
        n = oo[d + 1] - oo[d]
        at_least += 1 if n <= T else -(-(n - h - t) // c)
    if at_least >= 2 ** 32 or at_least * L > MAX_ELEMS:
        raise ValueError("tensor too large")
    src = np.asarray(ids, np.int64)
    span_src = np.asarray(spans, np.uint32).reshape(-1, 2) if flags & SPANS else None
    rows, doc, start, dw, n_split = [], [], [], [0], 0
    for d in range(D):
        o, n = oo[d], oo[d + 1] - oo[d]
        if n <= T:
            rows.append(list(range(o, o + n)))
            doc.append(d)
            start.append(min(h, n))
        else:
            b, k = n - h - t, 0
            n_split += 1
            while True:
                lo, hi = k * step, min(k * step + c, b)
                rows.append(list(range(o, o + h)) + list(range(o + h + lo, o + h + hi)) + list(range(o + n - t, o + n)))
                doc.append(d)
                start.append(min(h + lo, n))
                if hi >= b:
                    break
                k += 1
        dw.append(len(rows))
    W = len(rows)
    if W >= 2 ** 32 or W * L > MAX_ELEMS:
        raise ValueError("tensor too large")
    dt = np.int64 if flags & I64 else np.int32
    inp = np.full((W, L), pad_id, dt)
    mask = np.zeros((W, L), np.uint8)
    sp = np.zeros((W, L, 2), np.uint32) if flags & SPANS else None
    lengths = []
    for r, idx in enumerate(rows):
        lengths.append(len(idx))
        if idx:                                       # (the row's elements at once: idx lists where each comes from)
            inp[r, :len(idx)] = src[idx]
            mask[r, :len(idx)] = 1
            if sp is not None:
                sp[r, :len(idx)] = span_src[idx]
    return {"input_ids": inp, "mask": mask if flags & MASK else None, "lengths": np.array(lengths, np.uint32),
            "window_doc": np.array(doc, np.uint32), "window_start": np.array(start, np.uint32), "doc_windows": np.array(dw, np.uint64),
            "spans": sp, "n_windows": W, "n_split": n_split, "row_len": L}


def ragged(rows):
    oo = [0]
    for r in rows:
        oo.append(oo[-1] + len(r))
    return np.array([i for r in rows for i in r], np.int64), np.array(oo, np.int64)


P = 9   # the pad id of the hand-made cases
DOCS = [[1] + list(range(20, 30)) + [2], [1, 30, 2], [], [1] + list(range(40, 45)) + [2]]


def check(e, rows, window_doc, window_start, lengths, doc_windows, n_split):
    assert e["input_ids"].tolist() == rows
    assert e["window_doc"].tolist() == window_doc and e["window_start"].tolist() == window_start and e["lengths"].tolist() == lengths
    assert e["doc_windows"].tolist() == doc_windows and e["n_split"] == n_split and e["n_windows"] == len(rows)
    if e["mask"] is not None:
        assert e["mask"].tolist() == [[1] * n + [0] * (len(rows[0]) - n) for n in lengths]


def test_worked_example():
    ids, oo = ragged(DOCS)
    e = expected_windows(ids, oo, 6, 1, 1, 1, 0, P, FIXED | MASK)
    check(e, [[1, 20, 21, 22, 23, 2], [1, 23, 24, 25, 26, 2], [1, 26, 27, 28, 29, 2], [1, 30, 2, 9, 9, 9], [9, 9, 9, 9, 9, 9],
              [1, 40, 41, 42, 43, 2], [1, 43, 44, 2, 9, 9]], [0, 0, 0, 1, 2, 3, 3], [1, 4, 7, 1, 0, 1, 4], [6, 6, 6, 3, 0, 6, 4],
          [0, 3, 4, 5, 7], 2)
    assert e["input_ids"].dtype == np.int32 and e["row_len"] == 6
    # longest mode gives the same rows here (the longest document has more than T ids); multiple_of pads further
    assert expected_windows(ids, oo, 6, 1, 1, 1, 0, P, MASK)["input_ids"].tolist() == e["input_ids"].tolist()
    e8 = expected_windows(ids, oo, 6, 1, 1, 1, 8, P, I64)
    assert e8["input_ids"].shape == (7, 8) and e8["input_ids"].dtype == np.int64 and e8["mask"] is None
    assert e8["input_ids"][:, :6].tolist() == e["input_ids"].tolist() and np.all(e8["input_ids"][:, 6:] == P)


def test_hand_made_cases():
    body = list(range(100, 110))
    ids, oo = ragged([body])
    # T = 4, no overlap, no head / tail: 10 ids in 4 + 4 + 2
    check(expected_windows(ids, oo, 4, 0, 0, 0, 0, P, FIXED), [[100, 101, 102, 103], [104, 105, 106, 107], [108, 109, 9, 9]],
          [0, 0, 0], [0, 4, 8], [4, 4, 2], [0, 3], 1)
    # T = 4, stride 2: step 2; the window that starts at 6 reaches the end
    check(expected_windows(ids, oo, 4, 2, 0, 0, 0, P, FIXED),
          [[100, 101, 102, 103], [102, 103, 104, 105], [104, 105, 106, 107], [106, 107, 108, 109]], [0] * 4, [0, 2, 4, 6], [4] * 4, [0, 4], 1)
    # T = 5, stride 2, head and tail of one id: c = 3, step 1, body 101..108
    check(expected_windows(ids, oo, 5, 2, 1, 1, 0, P, FIXED),
          [[100, 101 + k, 102 + k, 103 + k, 109] for k in range(6)], [0] * 6, [1, 2, 3, 4, 5, 6], [5] * 6, [0, 6], 1)
    # h = 2, t = 3 at T = 8: c = 3; 12 ids, body 102..108 (7 ids) in 3 + 3 + 1
    ids, oo = ragged([list(range(100, 112))])
    check(expected_windows(ids, oo, 8, 0, 2, 3, 0, P, FIXED | MASK),
          [[100, 101, 102, 103, 104, 109, 110, 111], [100, 101, 105, 106, 107, 109, 110, 111], [100, 101, 108, 109, 110, 111, 9, 9]],
          [0, 0, 0], [2, 5, 8], [8, 8, 6], [0, 3], 1)
    # exactly T ids: one window, as it lies; T + 1: split, and the second window holds the one id that did not fit
    ids, oo = ragged([list(range(100, 106)), list(range(200, 207))])
    check(expected_windows(ids, oo, 6, 1, 1, 1, 0, P, FIXED),
          [[100, 101, 102, 103, 104, 105], [200, 201, 202, 203, 204, 206], [200, 204, 205, 206, 9, 9]], [0, 1, 1], [1, 1, 4], [6, 6, 4],
          [0, 1, 3], 1)
    # a document shorter than the head: window_start = min(h, n)
    ids, oo = ragged([[7], []])
    e = expected_windows(ids, oo, 8, 0, 2, 3, 0, P, 0)
    assert e["window_start"].tolist() == [1, 0] and e["input_ids"].tolist() == [[7], [9]] and e["row_len"] == 1


def test_hand_made_spans_and_empty_shapes():
    ids, oo = ragged(DOCS)
    sp = np.array([[3 * g, 3 * g + 2] for g in range(len(ids))], np.uint32)
    e = expected_windows(ids, oo, 6, 1, 1, 1, 0, P, FIXED | SPANS, sp)
    assert e["spans"].shape == (7, 6, 2) and e["spans"].dtype == np.uint32
    assert e["spans"][1].tolist() == [[0, 2], [12, 14], [15, 17], [18, 20], [21, 23], [33, 35]]       # ids 0, 4, 5, 6, 7, 11
    assert e["spans"][3].tolist() == [[36, 38], [39, 41], [42, 44], [0, 0], [0, 0], [0, 0]] and np.all(e["spans"][4] == 0)
    for oo0 in ([0], [0, 0, 0, 0]):                   # D = 0; all-empty documents
        D = len(oo0) - 1
        e = expected_windows([], oo0, 4, 1, 1, 1, 0, P, MASK)
        assert e["input_ids"].shape == (D, 0) and e["mask"].shape == (D, 0) and e["n_windows"] == D and e["n_split"] == 0
        assert e["doc_windows"].tolist() == list(range(D + 1)) and e["window_doc"].tolist() == list(range(D)) and e["lengths"].tolist() == [0] * D
        e = expected_windows([], oo0, 4, 1, 1, 1, 8, P, FIXED)
        assert e["input_ids"].shape == (D, 8) and np.all(e["input_ids"] == P)


# every refused case of step 8 (ids, oo, T, s, h, t, m, flags, spans): what the GPU test passes to the entries as well
def refused_cases():
    ids, oo = ragged(DOCS)
    big = [0] + [(i + 1) * 2 ** 31 for i in range(9)]
    return [("T == 0", ids, oo, 0, 0, 0, 0, 0, 0, None), ("h + t == T", ids, oo, 6, 0, 3, 3, 0, 0, None),
            ("h + t > T", ids, oo, 6, 0, 4, 3, 0, 0, None), ("s == c", ids, oo, 6, 4, 1, 1, 0, 0, None),
            ("s > c", ids, oo, 6, 7, 0, 0, 0, 0, None),
            ("unknown flag", ids, oo, 6, 1, 1, 1, 0, 16, None), ("unknown high flag", ids, oo, 6, 1, 1, 1, 0, 1 << 31, None),
            ("T beyond a row", ids, oo, 2 ** 31, 1, 1, 1, 0, 0, None),
            ("rounded L beyond a row", ids, oo, 2 ** 31 - 1, 1, 1, 1, 64, FIXED, None),
            ("W >= 2^32", [], big, 4, 0, 0, 0, 0, FIXED, None),                        # 9 documents of 2^29 windows each
            ("W * L > 2^36", [], [0] * 70, 2 ** 30, 0, 0, 0, 0, FIXED, None),          # 69 rows of 2^30 elements
            ("spans without a buffer", ids, oo, 6, 1, 1, 1, 0, SPANS, None),
            ("ids without a document", ids, [0], 6, 1, 1, 1, 0, 0, None),
            ("a document of 2^32 - 1 ids", [], [0, 2 ** 32 - 1], 2 ** 20, 0, 0, 0, 0, FIXED, None)]


def test_refused_options_raise():
    for what, ids, oo, T, s, h, t, m, flags, sp in refused_cases():
        with pytest.raises(ValueError):
            expected_windows(ids, oo, T, s, h, t, m, P, flags, sp)
    ids, oo = ragged(DOCS)                              # (and the neighbours that are valid)
    expected_windows(ids, oo, 6, 3, 1, 1, 0, P, 0)      # s = c - 1
    expected_windows(ids, oo, 3, 0, 1, 1, 0, P, 0)      # c = 1
    expected_windows([], [0] * 65, 2 ** 30, 0, 0, 0, 0, P, 0)   # 64 empty rows of length 0


def random_ragged(rng, D, longest):
    n = rng.integers(0, longest, D)
    n[rng.integers(0, D, max(D // 8, 1))] = 0
    oo = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    return rng.integers(10, 1000, int(oo[-1])), oo


def test_invariants_on_random_input():
    rng = np.random.default_rng(14)
    for case in range(60):
        ids, oo = random_ragged(rng, int(rng.integers(1, 25)), int(rng.integers(1, 90)))
        T = int(rng.integers(1, 33))
        h = int(rng.integers(0, min(T, 3)))
        t = int(rng.integers(0, min(T - h, 4)))
        c = T - h - t
        s = int(rng.integers(0, c))
        m = (0, 4, 7)[case % 3]
        flags = (FIXED if case & 1 else 0) | (I64 if case & 2 else 0) | MASK
        e = expected_windows(ids, oo, T, s, h, t, m, P, flags)
        n, dw, step = np.diff(oo), e["doc_windows"], c - s
        L = e["row_len"]
        base = T if flags & FIXED else min(int(n.max()), T)
        assert L == (-(-base // m) * m if m else base)
        assert dw[0] == 0 and dw[-1] == e["n_windows"] and np.all(np.diff(dw.astype(np.int64)) > 0)       # strictly increasing
        assert e["n_split"] == int(np.sum(n > T))
        for d in range(len(n)):
            w = int(dw[d + 1] - dw[d])
            nd, doc = int(n[d]), ids[int(oo[d]):int(oo[d + 1])].tolist()
            b = nd - h - t
            assert w == (1 if nd <= T else 1 + -(-(b - c) // step)), (T, s, h, t, nd)                     # the closed form
            rows = e["input_ids"][int(dw[d]):int(dw[d + 1])]
            lens = e["lengths"][int(dw[d]):int(dw[d + 1])].tolist()
            assert np.all(e["window_doc"][int(dw[d]):int(dw[d + 1])] == d)
            if nd <= T:
                assert rows[0][:nd].tolist() == doc and lens == [nd] and e["window_start"][int(dw[d])] == min(h, nd)
                continue
            body = []
            for k in range(w):
                row = rows[k][:lens[k]].tolist()
                assert row[:h] == doc[:h] and row[lens[k] - t:] == doc[nd - t:] and lens[k] <= T
                part = row[h:lens[k] - t]
                assert e["window_start"][int(dw[d]) + k] == h + k * step
                assert len(part) == c or (k == w - 1 and 0 < len(part) <= c)
                if k:
                    assert part[:min(s, len(part))] == body[len(body) - s:][:len(part)]                   # the overlap with the window before
                    part = part[s:]
                    assert part                                                                           # every window brings new ids
                body += part
            assert body == doc[h:nd - t]
        for r in range(e["n_windows"]):
            k = int(e["lengths"][r])
            assert np.all(e["input_ids"][r, k:] == P) and e["mask"][r].tolist() == [1] * k + [0] * (L - k)


def test_kernel_index_model_against_the_definition():
    """tools/window_model.py restates the kernels index by index and asserts that every read and write stays inside its array and
    that every element is written once; its outputs equal the definition's, at tiles of 16 and 64 units (LDS room for 4 and 8
    documents, so both forms of the staging run on small inputs) and at the kernel's own 2048 / 1024."""
    import window_model
    rng = np.random.default_rng(15)
    for case in range(150):
        ids, oo = random_ragged(rng, int(rng.integers(1, 40)), int(rng.integers(1, 70)))
        T = int(rng.integers(1, 24))
        h = int(rng.integers(0, min(T, 3)))
        t = int(rng.integers(0, min(T - h, 4)))
        s = int(rng.integers(0, T - h - t))
        e = expected_windows(ids, oo, T, s, h, t, (0, 4, 8)[case % 3], P, FIXED if case & 1 else 0)
        tile, cap = ((16, 4), (64, 8), (2048, 1024))[case % 3 if case < 100 else (case // 3) % 3]
        out, lengths, wdoc, wstart, dw = window_model.window_model(ids.tolist(), [int(x) for x in oo], T, s, h, t, e["row_len"], P, tile, cap)
        assert np.array_equal(out, e["input_ids"]), case
        assert lengths == e["lengths"].tolist() and wdoc == e["window_doc"].tolist() and wstart == e["window_start"].tolist()
        assert dw == e["doc_windows"].tolist()


def test_new_symbols_declared_in_header_and_shim():
    hdr = open(os.path.join(ROOT, "include", "tekken_hip.h")).read()
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bfn\s+%s\s*\(" % name, ffi), name
    for name, value in FLAG_VALUES.items():
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name
        assert re.search(r"\bconst %s\s*:\s*\w+\s*=\s*%d\s*;" % (name, value), ffi), name
    assert re.search(r"typedef struct tk_window_opts\b", hdr) and re.search(r"typedef struct tk_window\b", hdr)
    assert re.search(r"\bstruct TkWindowOpts\b", ffi) and re.search(r"\bstruct TkWindow\b", ffi)


def test_python_constants_match_the_header(tk):
    assert (tk.WINDOW_FIXED, tk.WINDOW_I64, tk.WINDOW_MASK, tk.WINDOW_SPANS) == (FIXED, I64, MASK, SPANS)
    for name in NEW_SYMBOLS:
        assert hasattr(tk.lib(), name), name
    for name in ("window_from_ids_device", "encode_batch_device_window", "encode_batch_window"):
        assert hasattr(tk.Engine, name), name
    assert hasattr(tk, "WindowResult") and hasattr(tk.Tekkenizer, "encode_batch_windows")
    import ctypes
    assert ctypes.sizeof(tk._WindowOpts) == 28 and ctypes.sizeof(tk._Window) == 7 * ctypes.sizeof(ctypes.c_void_p) + 32


def test_host_only_tokenizer_has_no_windows(tk, small_vocab):
    from test_host_tokenizer import model
    t = tk.Tekkenizer.from_json(json.dumps(model(small_vocab["tokens"])), device=-1)
    for kw in ({}, {"return_tensors": "np"}, {"stride": 1, "dtype": "int32", "padding": "longest"}):
        with pytest.raises(tk.TokenizerError) as e:
            t.encode_batch_windows(["hello world"], 4, **kw)
        assert e.value.code == tk.TK_ERR_NO_DEVICE
    t.close()
