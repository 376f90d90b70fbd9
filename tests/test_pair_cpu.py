"""Sentence-pair rows (include/tekken_hip.h tk_pair_from_ids_device), the parts that need no GPU: the plain-loop restatement of
the definition that tests/test_gpu_pair.py checks the kernels against, the hand-made cases of the definition, every refusal, the
flag values, the Rust shim's declarations, the binding's declaration of the result struct, and the host-only tokenizer."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from test_layout_binding_cpu import header_members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["tk_pair_from_ids_device", "tk_encode_pairs_device", "tk_encode_pairs", "tk_free_pair"]
LONGEST_FIRST, ONLY_FIRST, ONLY_SECOND = 0, 1, 2
FIXED, I64, MASK, SPANS, TYPE_IDS, SEQUENCE_IDS, OVERFLOW = 1, 2, 4, 8, 16, 32, 64
ALL_FLAGS = 127
SEQ_NONE = 255
VALUES = {"TK_PAIR_LONGEST_FIRST": 0, "TK_PAIR_ONLY_FIRST": 1, "TK_PAIR_ONLY_SECOND": 2, "TK_PAIR_FIXED": 1, "TK_PAIR_I64": 2, "TK_PAIR_MASK": 4,
          "TK_PAIR_SPANS": 8, "TK_PAIR_TYPE_IDS": 16, "TK_PAIR_SEQUENCE_IDS": 32, "TK_PAIR_OVERFLOW": 64, "TK_PAIR_SEQ_NONE": 255}
MAX_ROW, MAX_ELEMS = 2 ** 31 - 1, 2 ** 36
ARRAYS = ("input_ids", "mask", "type_ids", "sequence_ids", "lengths", "window_pair", "window_start", "second_start", "spans", "pair_windows")
COUNTS = ("n_pairs", "n_windows", "row_len", "n_truncated", "n_split", "n_fixed_cut")


def expected_pairs(ids, oo, T, strategy, s, F, m, pad_id, head, sep, tail, flags, spans=None):
    """The definition, restated pair by pair with plain loops: the windows of a pair are walked until one reaches the end of the
    windowed side (no cumulative sum, no closed form for their number), the cuts are the stated formulas.  ids / oo: the ragged ids
    of the 2P parts; spans: [N, 2] or None.  -> dict of ARRAYS (an unselected one None) and COUNTS.  Invalid options raise
    ValueError (the entries: TK_ERR_INVALID_ARG)."""
    oo = [int(x) for x in oo]
    T, s, F, m, n_parts = int(T), int(s), int(F), int(m or 0), len(oo) - 1
    head, sep, tail = list(head), list(sep), list(tail)
    if flags & ~ALL_FLAGS or strategy not in (LONGEST_FIRST, ONLY_FIRST, ONLY_SECOND):
        raise ValueError("flags / strategy")
    if len(head) > 4 or len(sep) > 4 or len(tail) > 4:
        raise ValueError("a list of more than 4 ids")
    if T <= 0 or T > MAX_ROW:
        raise ValueError("max_length")
    x = len(head) + len(sep) + len(tail)
    c = T - x
    if c < 2:
        raise ValueError("no room for the texts")
    if strategy == LONGEST_FIRST:
        if flags & OVERFLOW or s > 0:
            raise ValueError("overflow / stride with longest_first")
    else:
        if F > c - 1:
            raise ValueError("max_fixed")
        if F == 0:
            F = c - 1
        if s >= c - F:
            raise ValueError("stride")
    if n_parts % 2:
        raise ValueError("an odd number of parts")
    if flags & SPANS and spans is None:
        raise ValueError("no spans buffer")
    if n_parts == 0 and len(ids):
        raise ValueError("ids without a part")
    for i in range(n_parts):
        if oo[i + 1] - oo[i] >= 2 ** 32 - 1:
            raise ValueError("window_start is uint32")
    if flags & FIXED and m and (T + m - 1) // m * m > MAX_ROW:
        raise ValueError("row too long")
    P = n_parts // 2
    # a window holds at most c ids of the windowed side: where that bound alone is beyond what a tensor holds, refuse before
    # walking (the walk below decides every other case exactly)
    at_least = 0
    for p in range(P):
        a, b = oo[2 * p + 1] - oo[2 * p], oo[2 * p + 2] - oo[2 * p + 1]
        v = 0 if strategy == LONGEST_FIRST or not flags & OVERFLOW else b if strategy == ONLY_SECOND else a
        at_least += max(1, -(-v // c))
    if at_least >= 2 ** 32 or (flags & FIXED and at_least * T > MAX_ELEMS):
        raise ValueError("tensor too large")
    # per row: (pair, indices into ids of its A-part, of its B-part, window_start)
    rows, pw, n_truncated, n_split, n_fixed_cut = [], [0], 0, 0, 0
    for p in range(P):
        oa, ob, oe = oo[2 * p], oo[2 * p + 1], oo[2 * p + 2]
        a, b = ob - oa, oe - ob
        if strategy == LONGEST_FIRST:
            a2, b2 = a, b
            if a + b > c:
                if a <= b:
                    a2 = min(a, c // 2)
                    b2 = min(b, c - a2)
                else:
                    b2 = min(b, c // 2)
                    a2 = min(a, c - b2)
                n_truncated += 1
            rows.append((p, range(oa, oa + a2), range(ob, ob + b2), 0))
        else:
            xo, xl, vo, v = (oa, a, ob, b) if strategy == ONLY_SECOND else (ob, b, oa, a)
            f = min(xl, F)
            cw = c - f
            xs = range(xo, xo + f)
            wins = []
            if v <= cw:
                wins.append((0, v))
            elif not flags & OVERFLOW:
                wins.append((0, cw))
            else:
                step, k = cw - s, 0
                while True:
                    lo, hi = k * step, min(k * step + cw, v)
                    wins.append((lo, hi))
                    if hi >= v:
                        break
                    k += 1
            for lo, hi in wins:
                vs = range(vo + lo, vo + hi)
                rows.append((p, xs, vs, lo) if strategy == ONLY_SECOND else (p, vs, xs, lo))
            n_fixed_cut += xl > F
            n_truncated += xl > F or v > cw
            n_split += len(wins) > 1
        pw.append(len(rows))
    W = len(rows)
    longest = 0
    for _, ra, rb, _ in rows:
        longest = max(longest, x + len(ra) + len(rb))
    L = T if flags & FIXED else min(longest, T)
    if m:
        L = (L + m - 1) // m * m
    if L > MAX_ROW or W >= 2 ** 32 or W * L > MAX_ELEMS:
        raise ValueError("tensor too large")
    src = np.asarray(ids, np.int64)
    span_src = np.asarray(spans, np.uint32).reshape(-1, 2) if flags & SPANS else None
    inp = np.full((W, L), pad_id, np.int64 if flags & I64 else np.int32)
    mask, typ = np.zeros((W, L), np.uint8), np.zeros((W, L), np.uint8)
    seq = np.full((W, L), SEQ_NONE, np.uint8)
    sp = np.zeros((W, L, 2), np.uint32) if flags & SPANS else None
    lengths, wpair, wstart, second = [], [], [], []
    for r, (p, ra, rb, ws) in enumerate(rows):
        j = 0
        for i in head:
            inp[r, j] = i
            j += 1
        if len(ra):                                     # (a part's elements at once: ra is where they come from)
            inp[r, j:j + len(ra)] = src[ra.start:ra.stop]
            seq[r, j:j + len(ra)] = 0
            if sp is not None:
                sp[r, j:j + len(ra)] = span_src[ra.start:ra.stop]
            j += len(ra)
        for i in sep:
            inp[r, j] = i
            j += 1
        second.append(j)
        if len(rb):
            inp[r, j:j + len(rb)] = src[rb.start:rb.stop]
            seq[r, j:j + len(rb)] = 1
            typ[r, j:j + len(rb)] = 1
            if sp is not None:
                sp[r, j:j + len(rb)] = span_src[rb.start:rb.stop]
            j += len(rb)
        for i in tail:
            inp[r, j] = i
            typ[r, j] = 1
            j += 1
        mask[r, :j] = 1
        lengths.append(j)
        wpair.append(p)
        wstart.append(ws)
    u32 = lambda a: np.array(a, np.uint32)      # noqa: E731
    return {"input_ids": inp, "mask": mask if flags & MASK else None, "type_ids": typ if flags & TYPE_IDS else None,
            "sequence_ids": seq if flags & SEQUENCE_IDS else None, "lengths": u32(lengths), "window_pair": u32(wpair),
            "window_start": u32(wstart), "second_start": u32(second), "spans": sp, "pair_windows": np.array(pw, np.uint64),
            "n_pairs": P, "n_windows": W, "row_len": L, "n_truncated": int(n_truncated), "n_split": int(n_split),
            "n_fixed_cut": int(n_fixed_cut)}


def ragged(rows):
    oo = [0]
    for r in rows:
        oo.append(oo[-1] + len(r))
    return np.array([i for r in rows for i in r], np.int64), np.array(oo, np.int64)


PAD = 9      # the pad id of the hand-made cases
HW = [266, 42, 129, 121, 124, 118, 110]      # "hello world" with the small vocabulary (tests/test_gpu_spans.py); "hello" is [266]
EVERY = MASK | TYPE_IDS | SEQUENCE_IDS


def one(A, B, T, strategy, s=0, F=0, flags=FIXED | EVERY, head=(1,), sep=(), tail=(2,), m=0):
    ids, oo = ragged([A, B])
    return expected_pairs(ids, oo, T, strategy, s, F, m, PAD, head, sep, tail, flags)


def test_worked_example_only_second_overflow():
    """The first case of the issue, worked by hand there; the restatement agrees with it."""
    e = one([266], HW, 8, ONLY_SECOND, s=1, F=2, flags=FIXED | EVERY | OVERFLOW, sep=(2,))
    assert e["input_ids"].tolist() == [[1, 266, 2, 266, 42, 129, 121, 2], [1, 266, 2, 121, 124, 118, 110, 2]]
    assert e["window_start"].tolist() == [0, 3] and e["second_start"].tolist() == [3, 3] and e["window_pair"].tolist() == [0, 0]
    assert e["type_ids"].tolist() == [[0, 0, 0, 1, 1, 1, 1, 1]] * 2
    assert e["sequence_ids"].tolist() == [[255, 0, 255, 1, 1, 1, 1, 255]] * 2
    assert e["mask"].tolist() == [[1] * 8] * 2 and e["lengths"].tolist() == [8, 8] and e["pair_windows"].tolist() == [0, 2]
    assert (e["n_windows"], e["n_split"], e["n_truncated"], e["n_fixed_cut"], e["row_len"]) == (2, 1, 1, 0, 8)
    assert e["input_ids"].dtype == np.int32
    # the same without OVERFLOW: the first window alone; ONLY_FIRST swaps the sides
    e = one([266], HW, 8, ONLY_SECOND, s=1, F=2, sep=(2,))
    assert e["input_ids"].tolist() == [[1, 266, 2, 266, 42, 129, 121, 2]] and (e["n_split"], e["n_truncated"]) == (0, 1)
    e = one(HW, [266], 8, ONLY_FIRST, s=1, F=2, flags=EVERY | OVERFLOW | I64, sep=(2,))
    assert e["input_ids"].tolist() == [[1, 266, 42, 129, 121, 2, 266, 2], [1, 121, 124, 118, 110, 2, 266, 2]]
    assert e["window_start"].tolist() == [0, 3] and e["second_start"].tolist() == [6, 6] and e["input_ids"].dtype == np.int64
    assert e["sequence_ids"].tolist() == [[255, 0, 0, 0, 0, 255, 1, 255]] * 2 and e["type_ids"].tolist() == [[0] * 6 + [1, 1]] * 2


def test_worked_example_longest_first():
    """The second case of the issue."""
    e = one(HW, HW, 10, LONGEST_FIRST)
    assert e["input_ids"].tolist() == [[1, 266, 42, 129, 121, 266, 42, 129, 121, 2]]
    assert (e["n_truncated"], e["n_split"], e["n_fixed_cut"], e["n_windows"]) == (1, 0, 0, 1)
    assert e["second_start"].tolist() == [5] and e["window_start"].tolist() == [0]
    assert e["type_ids"].tolist() == [[0] * 5 + [1] * 5] and e["sequence_ids"].tolist() == [[255, 0, 0, 0, 0, 1, 1, 1, 1, 255]]


def kept(e):
    """(A ids, B ids) of the first row, from sequence_ids."""
    row, seq = e["input_ids"][0], e["sequence_ids"][0]
    return row[seq == 0].tolist(), row[seq == 1].tolist()


def test_longest_first_around_half_of_c():
    A, B = list(range(100, 120)), list(range(200, 220))
    for c in (8, 9):                                     # even and odd c; head and tail of one id
        T, h = c + 2, c // 2
        for a, b, ea, eb in ((h, 20, h, c - h), (h + 1, 20, h, c - h), (20, h, c - h, h), (20, h + 1, c - h, h),
                             (h - 1, 20, h - 1, c - h + 1), (20, h - 1, c - h + 1, h - 1),
                             (h, h, h, h), (h + 1, h + 1, h, c - h), (20, 20, h, c - h),        # ties: a <= b, A keeps c / 2
                             (h, c - h, h, c - h), (3, 2, 3, 2), (0, 20, 0, c), (20, 0, c, 0), (0, 0, 0, 0)):
            e = one(A[:a], B[:b], T, LONGEST_FIRST)
            assert kept(e) == (A[:ea], B[:eb]), (c, a, b)
            assert e["n_truncated"] == int(a + b > c) and e["lengths"].tolist() == [2 + ea + eb]
            assert e["second_start"].tolist() == [1 + ea]


def test_windows_at_cw_and_cw_plus_one():
    A, V = [50, 51, 52], list(range(100, 140))
    # T = 10, head and tail of one id, sep of one: c = 7; F = 3 -> f = 3, cw = 4
    for v, rows in ((4, [(0, 4)]), (5, [(0, 4), (2, 5)]), (6, [(0, 4), (2, 6)]), (7, [(0, 4), (2, 6), (4, 7)])):
        e = one(A, V[:v], 10, ONLY_SECOND, s=2, F=3, flags=FIXED | EVERY | OVERFLOW, sep=(7,))
        assert e["n_windows"] == len(rows) and e["n_split"] == int(len(rows) > 1) and e["n_truncated"] == int(len(rows) > 1)
        for r, (lo, hi) in enumerate(rows):
            assert e["input_ids"][r].tolist() == ([1] + A + [7] + V[lo:hi] + [2] + [PAD] * 10)[:10], (v, r)
            assert e["window_start"][r] == lo and e["second_start"][r] == 5 and e["lengths"][r] == 6 + hi - lo
    # |X| > F: the fixed side is cut to F in every window, and counted once
    e = one([50, 51, 52, 53, 54], V[:9], 10, ONLY_SECOND, s=0, F=3, flags=FIXED | EVERY | OVERFLOW, sep=(7,))
    assert e["input_ids"].tolist() == [[1, 50, 51, 52, 7] + V[0:4] + [2], [1, 50, 51, 52, 7] + V[4:8] + [2], [1, 50, 51, 52, 7, V[8], 2, 9, 9, 9]]
    assert (e["n_fixed_cut"], e["n_truncated"], e["n_split"]) == (1, 1, 1)
    # F = 0 reads as c - 1: a long fixed side leaves one id a window
    e = one(list(range(50, 70)), V[:3], 10, ONLY_SECOND, flags=EVERY | OVERFLOW, sep=(7,))
    assert e["n_windows"] == 3 and e["window_start"].tolist() == [0, 1, 2] and e["n_fixed_cut"] == 1 and e["row_len"] == 10
    assert e["input_ids"][2].tolist() == [1] + list(range(50, 56)) + [7, V[2], 2]
    # a short fixed side leaves its room to the windowed side
    e = one([50], V[:6], 10, ONLY_SECOND, s=0, F=3, flags=EVERY | OVERFLOW, sep=(7,))
    assert e["n_windows"] == 1 and e["lengths"].tolist() == [10] and e["n_truncated"] == 0


def test_empty_sides_and_fixed_lists():
    for strategy in (LONGEST_FIRST, ONLY_FIRST, ONLY_SECOND):
        e = one([], [7, 8], 8, strategy, flags=EVERY)
        assert e["input_ids"].tolist() == [[1, 7, 8, 2]] and e["second_start"].tolist() == [1] and e["sequence_ids"].tolist() == [[255, 1, 1, 255]]
        e = one([7, 8], [], 8, strategy, flags=EVERY)
        assert e["input_ids"].tolist() == [[1, 7, 8, 2]] and e["second_start"].tolist() == [3] and e["type_ids"].tolist() == [[0, 0, 0, 1]]
        e = one([], [], 8, strategy, flags=EVERY)
        assert e["input_ids"].tolist() == [[1, 2]] and e["row_len"] == 2 and e["lengths"].tolist() == [2] and e["type_ids"].tolist() == [[0, 1]]
        # all three lists empty; all pairs empty as well: rows of no element
        e = one([7], [8, 9], 8, strategy, flags=EVERY, head=(), tail=())
        assert e["input_ids"].tolist() == [[7, 8, 9]] and e["sequence_ids"].tolist() == [[0, 1, 1]] and e["second_start"].tolist() == [1]
        e = one([], [], 8, strategy, flags=EVERY, head=(), tail=())
        assert e["input_ids"].shape == (1, 0) and e["lengths"].tolist() == [0] and e["n_windows"] == 1
        # all three with 4 ids: x = 12
        e = one([7], [8], 16, strategy, flags=FIXED | EVERY, head=(1, 2, 3, 4), sep=(5, 6, 5, 6), tail=(4, 3, 2, 1))
        assert e["input_ids"].tolist() == [[1, 2, 3, 4, 7, 5, 6, 5, 6, 8, 4, 3, 2, 1, 9, 9]]
        assert e["type_ids"].tolist() == [[0] * 9 + [1] * 5 + [0, 0]] and e["second_start"].tolist() == [9]
        assert e["sequence_ids"].tolist() == [[255] * 4 + [0] + [255] * 4 + [1] + [255] * 6]
    # P = 0: no row; L = 0, or T with FIXED
    e = expected_pairs([], [0], 8, LONGEST_FIRST, 0, 0, 0, PAD, (1,), (), (2,), EVERY)
    assert e["input_ids"].shape == (0, 0) and e["pair_windows"].tolist() == [0] and e["n_windows"] == 0
    assert expected_pairs([], [0], 8, LONGEST_FIRST, 0, 0, 4, PAD, (1,), (), (2,), FIXED)["input_ids"].shape == (0, 8)
    # multiple_of and the longest row
    e = one([7], [8, 9], 64, LONGEST_FIRST, flags=EVERY, m=4)
    assert e["input_ids"].tolist() == [[1, 7, 8, 9, 2, 9, 9, 9]] and e["mask"].tolist() == [[1] * 5 + [0] * 3]
    assert e["sequence_ids"].tolist() == [[255, 0, 1, 1, 255, 255, 255, 255]]


def test_spans_follow_their_ids():
    ids, oo = ragged([[266], HW])
    sp = np.array([[0, 5]] + [[0, 5], [5, 6], [6, 7], [7, 8], [8, 9], [9, 10], [10, 11]], np.uint32)
    e = expected_pairs(ids, oo, 8, ONLY_SECOND, 1, 2, 0, PAD, (1,), (2,), (2,), FIXED | SPANS | OVERFLOW, sp)
    assert e["spans"].tolist() == [[[0, 0], [0, 5], [0, 0], [0, 5], [5, 6], [6, 7], [7, 8], [0, 0]],
                                   [[0, 0], [0, 5], [0, 0], [7, 8], [8, 9], [9, 10], [10, 11], [0, 0]]]
    assert e["mask"] is None and e["type_ids"] is None and e["sequence_ids"] is None


# every refused case of step 8 (what, ids, oo, T, strategy, s, F, m, head, sep, tail, flags): what the GPU test passes to the
# entries as well (the offsets of the cases are read there, never their ids)
def refused_cases():
    ids, oo = ragged([[266], HW, HW, [266]])
    h, t = (1,), (2,)
    big = [0]
    for _ in range(9):
        big += [big[-1], big[-1] + 2 ** 31]
    return [("c == 1", ids, oo, 3, LONGEST_FIRST, 0, 0, 0, h, (), t, 0), ("c == 0", ids, oo, 2, ONLY_SECOND, 0, 0, 0, h, (), t, 0),
            ("T == 0", ids, oo, 0, LONGEST_FIRST, 0, 0, 0, (), (), (), 0), ("T == 0 with FIXED", ids, oo, 0, ONLY_FIRST, 0, 0, 0, (), (), (), FIXED),
            ("T below x", ids, oo, 5, LONGEST_FIRST, 0, 0, 0, (1, 1, 1), (2, 2), t, 0),
            ("unknown strategy", ids, oo, 8, 3, 0, 0, 0, h, (), t, 0), ("unknown flag", ids, oo, 8, LONGEST_FIRST, 0, 0, 0, h, (), t, 128),
            ("unknown high flag", ids, oo, 8, ONLY_SECOND, 0, 0, 0, h, (), t, 1 << 31),
            ("5 head ids", ids, oo, 16, LONGEST_FIRST, 0, 0, 0, (1,) * 5, (), t, 0), ("5 sep ids", ids, oo, 16, ONLY_FIRST, 0, 0, 0, h, (2,) * 5, t, 0),
            ("5 tail ids", ids, oo, 16, ONLY_SECOND, 0, 0, 0, h, (), (2,) * 5, 0),
            ("OVERFLOW with LONGEST_FIRST", ids, oo, 8, LONGEST_FIRST, 0, 0, 0, h, (), t, OVERFLOW),
            ("stride with LONGEST_FIRST", ids, oo, 8, LONGEST_FIRST, 1, 0, 0, h, (), t, 0),
            ("F == c", ids, oo, 8, ONLY_SECOND, 0, 6, 0, h, (), t, 0), ("F > c", ids, oo, 8, ONLY_FIRST, 0, 7, 0, h, (), t, 0),
            ("s == c - F", ids, oo, 8, ONLY_SECOND, 4, 2, 0, h, (), t, OVERFLOW), ("s > c - F", ids, oo, 8, ONLY_FIRST, 5, 2, 0, h, (), t, 0),
            ("s == 1 with F == 0", ids, oo, 8, ONLY_SECOND, 1, 0, 0, h, (), t, OVERFLOW),
            ("an odd part count", ids, oo[:4], 8, LONGEST_FIRST, 0, 0, 0, h, (), t, 0),
            ("spans without a buffer", ids, oo, 8, LONGEST_FIRST, 0, 0, 0, h, (), t, SPANS),
            ("T beyond a row", ids, oo, 2 ** 31, LONGEST_FIRST, 0, 0, 0, h, (), t, 0),
            ("rounded L beyond a row", ids, oo, 2 ** 31 - 1, LONGEST_FIRST, 0, 0, 64, h, (), t, FIXED),
            ("W >= 2^32", [], big, 4, ONLY_SECOND, 0, 1, 0, (), (), (), FIXED | OVERFLOW),        # 9 pairs of 2^29 windows each
            ("W * L > 2^36", [], [0] * 139, 2 ** 30, LONGEST_FIRST, 0, 0, 0, (), (), (), FIXED),   # 69 rows of 2^30 elements
            ("a part of 2^32 - 1 ids", [], [0, 0, 2 ** 32 - 1], 2 ** 20, LONGEST_FIRST, 0, 0, 0, (), (), (), FIXED),
            ("ids without a part", ids, [0], 8, LONGEST_FIRST, 0, 0, 0, h, (), t, 0)]


def test_refused_options_raise():
    for what, ids, oo, T, strategy, s, F, m, head, sep, tail, flags in refused_cases():
        with pytest.raises(ValueError):
            expected_pairs(ids, oo, T, strategy, s, F, m, PAD, head, sep, tail, flags)
            pytest.fail(what)
    ids, oo = ragged([[266], HW, HW, [266]])            # (and the neighbours that are valid)
    h, t = (1,), (2,)
    expected_pairs(ids, oo, 4, LONGEST_FIRST, 0, 0, 0, PAD, h, (), t, 0)                 # c = 2
    expected_pairs(ids, oo, 4, ONLY_SECOND, 0, 1, 0, PAD, h, (), t, OVERFLOW)           # c = 2, F = c - 1
    expected_pairs(ids, oo, 8, ONLY_FIRST, 3, 2, 0, PAD, h, (), t, OVERFLOW)            # s = c - F - 1
    expected_pairs(ids, oo, 8, ONLY_SECOND, 0, 5, 0, PAD, h, (), t, 0)                  # F = c - 1
    expected_pairs(ids, oo, 16, LONGEST_FIRST, 0, 0, 0, PAD, (1,) * 4, (2,) * 4, (2,) * 4, 0)
    expected_pairs([], [0] * 129, 2 ** 30, LONGEST_FIRST, 0, 0, 0, PAD, (), (), (), 0)  # 64 empty rows of length 0
    expected_pairs([], [0], 8, LONGEST_FIRST, 0, 0, 0, PAD, h, (), t, 0)                # P = 0 on its own


def random_parts(rng, P, longest):
    n = rng.integers(0, longest, 2 * P)
    n[rng.integers(0, 2 * P, max(P // 4, 1))] = 0
    oo = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    return rng.integers(10, 1000, int(oo[-1])), oo


def test_invariants_on_random_input():
    rng = np.random.default_rng(41)
    for case in range(90):
        ids, oo = random_parts(rng, int(rng.integers(1, 20)), int(rng.integers(1, 60)))
        strategy = case % 3
        lists = [list(rng.integers(1, 9, int(rng.integers(0, 5)))) for _ in range(3)]
        x = sum(len(l) for l in lists)
        T = x + int(rng.integers(2, 30))
        c = T - x
        F = int(rng.integers(1, c)) if strategy else 0
        s = int(rng.integers(0, c - F)) if strategy else 0
        m = (0, 4, 7)[(case // 3) % 3]
        flags = EVERY | (FIXED if case & 1 else 0) | (OVERFLOW if strategy and case & 2 else 0)
        e = expected_pairs(ids, oo, T, strategy, s, F, m, PAD, *lists, flags)
        pw, L = e["pair_windows"].astype(np.int64), e["row_len"]
        assert pw[0] == 0 and pw[-1] == e["n_windows"] and np.all(np.diff(pw) > 0)
        assert np.array_equal(e["window_pair"], np.repeat(np.arange(len(pw) - 1), np.diff(pw)))
        base = T if flags & FIXED else int(e["lengths"].max())
        assert L == (-(-base // m) * m if m else base) and e["lengths"].max() <= T
        for p in range(len(pw) - 1):
            A, B = (ids[int(oo[2 * p + i]):int(oo[2 * p + i + 1])].tolist() for i in (0, 1))
            a, b, w = len(A), len(B), int(pw[p + 1] - pw[p])
            got_v = []
            for k, r in enumerate(range(int(pw[p]), int(pw[p + 1]))):
                row, seq, n = e["input_ids"][r], e["sequence_ids"][r], int(e["lengths"][r])
                ra, rb = row[seq == 0].tolist(), row[seq == 1].tolist()
                assert row[:n].tolist() == lists[0] + ra + lists[1] + rb + lists[2] and np.all(row[n:] == PAD)
                assert e["mask"][r].tolist() == [1] * n + [0] * (L - n)
                s2 = int(e["second_start"][r])
                assert s2 == len(lists[0]) + len(ra) + len(lists[1])
                assert e["type_ids"][r].tolist() == [0] * s2 + [1] * (n - s2) + [0] * (L - n)
                ws = int(e["window_start"][r])
                if strategy == LONGEST_FIRST:
                    assert w == 1 and ra == A[:len(ra)] and rb == B[:len(rb)] and ws == 0
                    assert (len(ra), len(rb)) == (a, b) if a + b <= c else len(ra) + len(rb) == c
                    continue
                X, V, rx, rv = (A, B, ra, rb) if strategy == ONLY_SECOND else (B, A, rb, ra)
                f = min(len(X), F)
                cw = c - f
                assert rx == X[:f] and rv == V[ws:ws + len(rv)] and len(rv) <= cw
                if w == 1:
                    assert ws == 0 and len(rv) == min(len(V), cw)
                else:
                    assert flags & OVERFLOW and ws == k * (cw - s) and (len(rv) == cw or k == w - 1) and rv
                    if k:
                        assert len(rv) > s                                  # every window brings new ids
                    got_v += rv if not k else rv[s:]
            if w > 1:
                assert got_v == V and w == 1 + -(-(len(V) - cw) // (cw - s))     # the closed form


def test_kernel_index_model_against_the_definition():
    """tools/pair_model.py restates the kernels index by index and asserts that every read and write stays inside its array and
    that every element is written once; its outputs equal the definition's, at tiles of 16 and 64 units (LDS room for 4 and 8
    pairs, so both forms of the staging run on small inputs) and at the kernel's own 2048 / 1024."""
    import pair_model
    rng = np.random.default_rng(42)
    for case in range(180):
        ids, oo = random_parts(rng, int(rng.integers(1, 40)), int(rng.integers(1, 50)))
        strategy = case % 3
        lists = [[int(i) for i in rng.integers(1, 9, int(rng.integers(0, 5)))] for _ in range(3)]
        x = sum(len(l) for l in lists)
        c = int(rng.integers(2, 22))
        F = int(rng.integers(0, c)) if strategy else 0
        s = int(rng.integers(0, c - (F or c - 1))) if strategy else 0
        flags = EVERY | (FIXED if case & 1 else 0) | (OVERFLOW if strategy and case & 2 else 0)
        e = expected_pairs(ids, oo, x + c, strategy, s, F, (0, 4, 8)[(case // 3) % 3], PAD, *lists, flags)
        tile, cap = ((16, 4), (64, 8), (2048, 1024))[case % 3 if case < 120 else (case // 3) % 3]
        out, mask, typ, seq, lengths, wpair, wstart, second, pw, counts = pair_model.pair_model(
            ids.tolist(), [int(i) for i in oo], x + c, strategy, s, F, bool(flags & OVERFLOW), *lists, e["row_len"], PAD, tile, cap)
        assert np.array_equal(out, e["input_ids"]), case
        assert np.array_equal(mask, e["mask"]) and np.array_equal(typ, e["type_ids"]) and np.array_equal(seq, e["sequence_ids"]), case
        assert lengths == e["lengths"].tolist() and wpair == e["window_pair"].tolist() and wstart == e["window_start"].tolist()
        assert second == e["second_start"].tolist() and pw == e["pair_windows"].tolist()
        longest = max(lengths)
        assert counts == (longest, e["n_truncated"], e["n_split"], e["n_fixed_cut"]), case


def test_new_symbols_declared_in_header_and_shim():
    hdr = open(os.path.join(ROOT, "include", "tekken_hip.h")).read()
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bfn\s+%s\s*\(" % name, ffi), name
    for name, value in VALUES.items():
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name
        assert re.search(r"\bconst %s\s*:\s*\w+\s*=\s*%d\s*;" % (name, value), ffi), name
    assert re.search(r"typedef struct tk_pair_opts\b", hdr) and re.search(r"typedef struct tk_pair\b", hdr)
    assert re.search(r"\bstruct TkPairOpts\b", ffi) and re.search(r"\bstruct TkPair\b", ffi)
    # the shim's structs have the header's members, in its order
    m = re.search(r"typedef struct tk_pair_opts\s*\{(.*?)\}", hdr, re.S)
    names = re.findall(r"(\w+)(?:\[4\])?\s*[,;]", m.group(1))
    assert re.findall(r"pub (\w+):", re.search(r"struct TkPairOpts \{(.*?)\}", ffi, re.S).group(1)) == names
    assert re.findall(r"pub (\w+):", re.search(r"struct TkPair \{(.*?)\}", ffi, re.S).group(1)) == [n for n, _ in header_members("pair")]


def test_python_constants_match_the_header(tk):
    assert (tk.PAIR_LONGEST_FIRST, tk.PAIR_ONLY_FIRST, tk.PAIR_ONLY_SECOND) == (LONGEST_FIRST, ONLY_FIRST, ONLY_SECOND)
    assert (tk.PAIR_FIXED, tk.PAIR_I64, tk.PAIR_MASK, tk.PAIR_SPANS, tk.PAIR_TYPE_IDS, tk.PAIR_SEQUENCE_IDS, tk.PAIR_OVERFLOW,
            tk.PAIR_SEQ_NONE) == (FIXED, I64, MASK, SPANS, TYPE_IDS, SEQUENCE_IDS, OVERFLOW, SEQ_NONE)
    for name in NEW_SYMBOLS:
        assert hasattr(tk.lib(), name), name
    for name in ("pair_from_ids_device", "encode_pairs_device", "encode_pairs"):
        assert hasattr(tk.Engine, name), name
    assert hasattr(tk.Tekkenizer, "encode_pairs")
    assert ctypes.sizeof(tk._PairOpts) == 88 and [f[0] for f in tk._PairOpts._fields_] == [
        "max_length", "strategy", "stride", "max_fixed", "multiple_of", "pad_id", "n_head", "n_sep", "n_tail", "head", "sep", "tail", "flags"]
    o = tk._pair_opts(8, ONLY_SECOND, 1, 2, 4, 9, (1,), (), (2, 3, 4, 5, 6), FIXED)
    assert (o.max_length, o.strategy, o.stride, o.max_fixed, o.multiple_of, o.pad_id, o.flags) == (8, 2, 1, 2, 4, 9, 1)
    assert (o.n_head, o.n_sep, o.n_tail, list(o.head), list(o.tail)) == (1, 0, 5, [1, 0, 0, 0], [2, 3, 4, 5])


def test_pair_result_declares_the_header_struct(tk):
    """What tests/test_layout_binding_cpu.py holds for the five earlier passes, for tk_pair."""
    R, members = tk.PairResult, header_members("pair")
    assert issubclass(R, tk._LayoutResult) and R.PASS == "pair" and R.I64 == I64
    assert [o[0] for o in R.OUTPUTS] == [m for m, ptr in members if ptr] == list(ARRAYS)
    assert list(R.COUNTS) == [m for m, ptr in members if not ptr] == list(COUNTS)
    assert [ptr for _, ptr in members] == sorted((ptr for _, ptr in members), reverse=True)
    assert ctypes.sizeof(R.STRUCT) == sum(ctypes.sizeof(ctypes.c_void_p) if ptr else 8 for _, ptr in members)
    assert [f[0] for f in R.STRUCT._fields_] == [m for m, _ in members]
    for (_, ptr), (_, ctype) in zip(members, R.STRUCT._fields_):
        assert ctype is (ctypes.c_void_p if ptr else ctypes.c_uint64)
    st = R.STRUCT()
    for i, (field, _) in enumerate(R.STRUCT._fields_):
        setattr(st, field, 0x1000 * (i + 1) if field in ARRAYS else i + 2)
    st.type_ids = None
    r = R(st, I64)
    assert r.typestr == "<i8" and r.type_ids_ptr is None and r.n_pairs == st.n_pairs
    for (out, typestr, shape, _, optional), v in zip(R.OUTPUTS, r.views()):
        assert optional == (out in ("mask", "type_ids", "sequence_ids", "spans"))
        if out == "type_ids":
            assert v is None
            continue
        cai = v.__cuda_array_interface__
        assert cai["data"][0] == getattr(st, out) and cai["shape"] == tuple(shape(r)) and cai["typestr"] == (typestr or "<i8")
    assert r.views()[0].__cuda_array_interface__["shape"] == (st.n_windows, st.row_len)
    assert r.views()[8].__cuda_array_interface__["shape"] == (st.n_windows, st.row_len, 2)
    assert r.views()[9].__cuda_array_interface__["shape"] == (st.n_pairs + 1,)
    assert set(r._counts()) == set(R.DICT_COUNTS) == {"n_windows", "n_truncated", "n_split", "n_fixed_cut"}


def test_host_only_tokenizer_has_no_pairs(tk, small_vocab):
    from test_host_tokenizer import model
    t = tk.Tekkenizer.from_json(json.dumps(model(small_vocab["tokens"])), device=-1)
    for kw in ({}, {"return_tensors": "np"}, {"truncation": "only_second", "stride": 1, "max_fixed": 2, "return_overflowing_tokens": True}):
        with pytest.raises(tk.TokenizerError) as e:
            t.encode_pairs(["hello"], ["hello world"], 8, **kw)
        assert e.value.code == tk.TK_ERR_NO_DEVICE
    t.close()
