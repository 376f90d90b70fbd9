"""Boundary-aware token-budget chunks (include/tekken_hip.h tk_chunk_from_ids_device, tk_chunk_levels_device), the parts that need
no GPU: the plain-loop restatement of the definition that tests/test_gpu_chunk.py checks the kernels against, the known answer and
the hand-made cases of the definition, its invariants, its reduction to the window pass, the kernels' index model, the Rust shim's
declarations, the binding's description of the result, and the host-only tokenizer."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from test_layout_binding_cpu import header_members
from test_window_cpu import expected_windows, ragged, random_ragged

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["tk_chunk_levels_device", "tk_chunk_from_ids_device", "tk_encode_batch_device_chunk", "tk_encode_batch_chunk", "tk_free_chunk",
               "tk_last_chunk_ms"]
FIXED, I64, MASK, SPANS, BYTES = 1, 2, 4, 8, 16
NONE, TOKEN, WORD, SENTENCE, LINE, PARAGRAPH = 0, 1, 2, 3, 4, 5
ALL_LEVELS, CUT_LAST = 60, 255
CONSTANTS = {"TK_CHUNK_FIXED": 1, "TK_CHUNK_I64": 2, "TK_CHUNK_MASK": 4, "TK_CHUNK_SPANS": 8, "TK_CHUNK_BYTES": 16, "TK_CHUNK_LEVEL_NONE": 0,
             "TK_CHUNK_LEVEL_TOKEN": 1, "TK_CHUNK_LEVEL_WORD": 2, "TK_CHUNK_LEVEL_SENTENCE": 3, "TK_CHUNK_LEVEL_LINE": 4,
             "TK_CHUNK_LEVEL_PARAGRAPH": 5, "TK_CHUNK_LEVELS_ALL": 60, "TK_CHUNK_CUT_LAST": 255}
MAX_ROW, MAX_ELEMS = 2 ** 31 - 1, 2 ** 36
WS = (0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20)
CJK_ENDERS = (b"\xe3\x80\x82", b"\xef\xbc\x81", b"\xef\xbc\x9f")


def level_at(text, p, mask=ALL_LEVELS):
    """The level of the break in front of byte p of the document `text` (bytes), rule by rule."""
    n = len(text)
    if p >= n or p == 0:
        return TOKEN
    if text[p] & 0xC0 == 0x80:
        return NONE
    q, walked, nl = p, 0, 0
    while walked < 16 and q > 0 and text[q - 1] in WS:
        q -= 1
        walked += 1
        nl += text[q] == 0x0A
    if nl >= 2:
        lv = PARAGRAPH
    elif nl == 1:
        lv = LINE
    else:
        gap = q < p or text[p] in WS
        lv = WORD if gap else TOKEN
        if walked < 16 and q > 0:                     # (16 bytes walked: stopped by the bound, whatever lies in front)
            if gap and text[q - 1] in b".!?":
                lv = SENTENCE
            if q >= 3 and bytes(text[q - 3:q]) in CJK_ENDERS:
                lv = SENTENCE
    while lv >= WORD and not mask & (1 << lv):        # demoted to the highest enabled level below, or to TOKEN
        lv -= 1
    return lv


def expected_levels(text, spans, mask=ALL_LEVELS):
    """The level byte of every id of ONE document: text its bytes, spans [n, 2] the doc-relative spans of its ids."""
    if mask & ~ALL_LEVELS:
        raise ValueError("levels")
    return [level_at(text, int(s), mask) for s, _ in np.asarray(spans, np.int64).reshape(-1, 2)]


def expected_levels_batch(docs, oo, spans, mask=ALL_LEVELS):
    """... of a batch: docs a list of bytes, oo the id offsets, spans [N, 2].  -> uint8 [N]"""
    spans = np.asarray(spans, np.int64).reshape(-1, 2)
    out = []
    for d, text in enumerate(docs):
        out += expected_levels(text, spans[int(oo[d]):int(oo[d + 1])], mask)
    return np.array(out, np.uint8)


def walk(L, b, c, m, o):
    """The greedy chain over a body of b ids with L[j] the level in front of body id j -> [(a, e, cut_level)]."""
    out, a = [], 0
    while True:
        if b - a <= c:
            out.append((a, b, CUT_LAST))
            return out
        cand = np.minimum(np.asarray(L[a + m:a + c + 1]), PARAGRAPH)       # (a byte above 5 reads as 5)
        best = int(cand.max())
        e = a + m + int(np.nonzero(cand == best)[0][-1])                       # the LARGEST candidate of that level
        out.append((a, e, best))
        lo = max(a + 1, e - o)
        front = np.asarray(L[lo:e])
        words, tokens = np.nonzero(front >= WORD)[0], np.nonzero(front >= TOKEN)[0]
        a = lo + int(words[0]) if len(words) else lo + int(tokens[0]) if len(tokens) else e


def expected_chunks(ids, oo, lev, T, m, o, h, t, multiple_of, pad_id, flags, spans=None):
    """The definition, restated document by document.  lev: one level per id (None: no level buffer); spans: [N, 2] or None.
    -> dict(expected_windows's entries, cut_level uint8 [W], chunk_bytes uint32 [W, 2] or None, level_counts uint64 [6]).  Invalid
    options raise ValueError (the entries: TK_ERR_INVALID_ARG)."""
    oo = [int(x) for x in oo]
    T, m, o, h, t, mo, D = int(T), int(m), int(o), int(h), int(t), int(multiple_of or 0), len(oo) - 1
    if T <= 0 or T > MAX_ROW or h < 0 or t < 0 or h + t >= T or flags & ~(FIXED | I64 | MASK | SPANS | BYTES):
        raise ValueError("max_length / keep_head / keep_tail / flags")
    c = T - h - t
    if not 0 <= o < m <= c:
        raise ValueError("min_length / overlap")
    if flags & (SPANS | BYTES) and spans is None:
        raise ValueError("no spans buffer")
    if D == 0 and len(ids):
        raise ValueError("ids without a document")
    if lev is None and len(ids):
        raise ValueError("no level buffer")
    longest = 0
    for d in range(D):
        longest = max(longest, oo[d + 1] - oo[d])
    if longest >= 2 ** 32 - 1:
        raise ValueError("window_start is uint32")
    L = T if flags & FIXED else min(longest, T)
    if mo:
        L = (L + mo - 1) // mo * mo
    if L > MAX_ROW:
        raise ValueError("row too long")
    # a chunk holds at most c body ids, so a split document has at least ceil(b / c) of them: where that bound alone is beyond what a
    # tensor holds, refuse before walking (the walk below decides every other case exactly; it gives a document no more than
    # 1 + ceil((b - c) / (m - o)) chunks)
    at_least = 0
    for d in range(D):
        n = oo[d + 1] - oo[d]
        at_least += 1 if n <= T else -(-(n - h - t) // c)
    if at_least >= 2 ** 32 or at_least * L > MAX_ELEMS:
        raise ValueError("tensor too large")
    src = np.asarray(ids, np.int64)
    lev = np.asarray(lev if lev is not None else [], np.uint8)
    span_src = np.asarray(spans, np.uint32).reshape(-1, 2) if flags & (SPANS | BYTES) else None
    rows, doc, start, dw, cut, cb, n_split, counts = [], [], [], [0], [], [], 0, [0] * 6
    for d in range(D):
        p, n = oo[d], oo[d + 1] - oo[d]
        if n <= T:
            rows.append(list(range(p, p + n)))
            doc.append(d)
            start.append(min(h, n))
            cut.append(CUT_LAST)
            cb.append((p, p + n - 1) if n else None)
        else:
            b = n - h - t
            n_split += 1
            chain = walk(lev[p + h:p + h + b], b, c, m, o)
            assert len(chain) <= 1 + -(-(b - c) // (m - o))
            for a, e, level in chain:
                rows.append(list(range(p, p + h)) + list(range(p + h + a, p + h + e)) + list(range(p + n - t, p + n)))
                doc.append(d)
                start.append(min(h + a, n))
                cut.append(level)
                cb.append((p + h + a, p + h + e - 1))
                if level != CUT_LAST:
                    counts[level] += 1
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
        if idx:
            inp[r, :len(idx)] = src[idx]
            mask[r, :len(idx)] = 1
            if sp is not None:
                sp[r, :len(idx)] = span_src[idx]
    chunk_bytes = None
    if flags & BYTES:
        chunk_bytes = np.array([(0, 0) if x is None else (span_src[x[0], 0], span_src[x[1], 1]) for x in cb], np.uint32).reshape(W, 2)
    return {"input_ids": inp, "mask": mask if flags & MASK else None, "lengths": np.array(lengths, np.uint32),
            "window_doc": np.array(doc, np.uint32), "window_start": np.array(start, np.uint32), "doc_windows": np.array(dw, np.uint64),
            "spans": sp, "cut_level": np.array(cut, np.uint8), "chunk_bytes": chunk_bytes, "level_counts": np.array(counts, np.uint64),
            "n_windows": W, "n_split": n_split, "row_len": L}


# ---- the levels ----

KNOWN_TEXT = "Hello world. Next one!\n\nPara two\n  indented 3.14 eé".encode("utf-8")
KNOWN_LEVELS = [1, 1, 1, 1, 1, 2, 2, 1, 1, 1, 1, 1, 3, 3, 1, 1, 1, 2, 2, 1, 1, 1, 3, 4, 5, 1, 1, 1, 2, 2, 1, 1, 2, 4, 4, 4, 1, 1, 1, 1, 1, 1, 1,
                2, 2, 1, 1, 1, 2, 2, 1, 0]


def test_known_answer_levels():
    assert len(KNOWN_TEXT) == 52 == len(KNOWN_LEVELS)
    assert [level_at(KNOWN_TEXT, p) for p in range(52)] == KNOWN_LEVELS
    spans = [(p, p + 1) for p in range(52)]
    assert expected_levels(KNOWN_TEXT, spans) == KNOWN_LEVELS


def test_hand_made_levels():
    for k, bounded in ((15, False), (16, True), (17, True)):
        # a run of k blanks behind a full stop: within the bound the sentence is seen, at 16 walked bytes it is a word break
        text = b"end." + b" " * k + b"Next"
        assert level_at(text, 4 + k) == (WORD if bounded else SENTENCE), k
        # ... with a newline at the run's far end: counted only where the walk reaches it
        text = b"end.\n" + b" " * (k - 1) + b"Next"
        assert level_at(text, 4 + k) == (LINE if k <= 16 else WORD), k
        text = b"end.\n\n" + b" " * (k - 2) + b"Next"
        assert level_at(text, 4 + k) == (PARAGRAPH if k <= 16 else LINE if k == 17 else WORD), k
        # a run that begins the document: q == 0, no sentence to look for
        assert level_at(b" " * k + b"x", k) == WORD
    assert level_at(b". a", 0) == TOKEN and level_at(b". a", 1) == SENTENCE and level_at(b". a", 2) == SENTENCE       # '.' at byte 0
    assert level_at(b".a", 1) == TOKEN                                                                              # no gap
    text = b"pi 3.14 is"
    assert [level_at(text, p) for p in range(len(text))] == [1, 1, 2, 2, 1, 1, 1, 2, 2, 1]                          # 3.14 is not cut
    for ender in CJK_ENDERS:
        text = "你好".encode() + ender + "再见".encode()
        assert level_at(text, 9) == SENTENCE and level_at(text, 6) == TOKEN and level_at(text, 7) == NONE and level_at(text, 10) == NONE
        assert level_at(ender + b"a", 3) == SENTENCE and level_at(ender[1:] + b"a", 2) == TOKEN                     # q >= 3 is needed
    assert level_at(b"a\xa9b", 1) == NONE and level_at(b"\xa9\xa9", 1) == NONE and level_at(b"\xa9\xa9", 0) == TOKEN  # a continuation byte
    assert level_at(b"abc", 3) == TOKEN and level_at(b"abc", 7) == TOKEN and level_at(b"", 0) == TOKEN              # p == len, beyond
    no_sentence, no_paragraph = ALL_LEVELS & ~(1 << SENTENCE), ALL_LEVELS & ~(1 << PARAGRAPH)
    assert level_at(b"a. b", 3) == SENTENCE and level_at(b"a. b", 3, no_sentence) == WORD
    assert level_at(b"a\n\nb", 3) == PARAGRAPH and level_at(b"a\n\nb", 3, no_paragraph) == LINE
    assert level_at(b"a\n\nb", 3, 1 << WORD) == WORD and level_at(b"a\n\nb", 3, 0) == TOKEN and level_at(b"a\xa9", 1, 0) == NONE
    assert level_at(b"a\n\nb", 3, 1 << SENTENCE) == SENTENCE and level_at(b"a b", 2, 1 << SENTENCE) == TOKEN
    with pytest.raises(ValueError):
        expected_levels(b"a b", [(0, 1)], 2)
    with pytest.raises(ValueError):
        expected_levels(b"a b", [(0, 1)], 64)


# ---- the walk ----

P = 9


def chunks_of(lev, T, m, o, h=0, t=0, flags=FIXED, ids=None):
    ids = list(range(100, 100 + len(lev))) if ids is None else ids
    return expected_chunks(ids, [0, len(ids)], lev, T, m, o, h, t, 0, P, flags)


def test_hand_made_walk():
    # 12 ids, T = 6, m = 3: candidates 3 .. 6; a paragraph break at 4 is preferred over the later word break at 6
    lev = [1, 1, 1, 1, 5, 1, 2, 1, 1, 1, 1, 1]
    e = chunks_of(lev, 6, 3, 0)
    assert e["input_ids"].tolist() == [[100, 101, 102, 103, 9, 9], [104, 105, 106, 107, 108, 109], [110, 111, 9, 9, 9, 9]]
    assert e["cut_level"].tolist() == [PARAGRAPH, TOKEN, CUT_LAST] and e["window_start"].tolist() == [0, 4, 10]
    assert e["level_counts"].tolist() == [0, 1, 0, 0, 0, 1] and e["n_split"] == 1 and e["doc_windows"].tolist() == [0, 3]
    # of two paragraph breaks among the candidates the LARGEST wins
    assert chunks_of([1, 1, 1, 5, 1, 5, 1, 1, 1, 1, 1, 1], 6, 3, 0)["window_start"].tolist() == [0, 5, 11]
    # a forced cut inside a character: every candidate is NONE
    lev = [1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1]
    e = chunks_of(lev, 4, 2, 0)
    assert e["cut_level"].tolist() == [NONE, NONE, CUT_LAST] and e["window_start"].tolist() == [0, 4, 8] and e["level_counts"].tolist() == [2, 0, 0, 0, 0, 0]
    # an overlap start snapped to a word: the cut at 6, overlap 3 looks at 3 .. 5 and takes the word break at 4, not the token at 3
    lev = [1, 1, 1, 1, 2, 1, 3, 1, 1, 1, 1]
    e = chunks_of(lev, 6, 4, 3)
    # (the second cut, at 10, is a token break; in front of it 7 .. 9 hold no word break, so the third chunk starts at 7)
    assert e["window_start"].tolist() == [0, 4, 7] and e["lengths"].tolist() == [6, 6, 4] and e["cut_level"].tolist() == [SENTENCE, TOKEN, CUT_LAST]
    # ... no word there: the first token break; none at all: the cut itself
    assert chunks_of([1, 1, 1, 0, 1, 1, 3, 1, 1, 1, 1], 6, 4, 3)["window_start"].tolist()[:2] == [0, 4]
    assert chunks_of([1, 1, 1, 0, 0, 0, 3, 1, 1, 1, 1], 6, 4, 3)["window_start"].tolist()[:2] == [0, 6]
    # head and tail repeated, chunk_bytes from the body's first id to its last, an unsplit and an empty document beside it
    ids, oo = ragged([[1] + list(range(20, 30)) + [2], [1, 30, 2], []])
    lev = [1] + [1, 1, 2, 1, 1, 2, 1, 1, 1, 1] + [1] + [1, 1, 1]
    sp = np.array([[3 * g, 3 * g + 2] for g in range(len(ids))], np.uint32)
    e = expected_chunks(ids, oo, lev, 6, 2, 1, 1, 1, 0, P, FIXED | MASK | BYTES | SPANS, sp)
    # (overlap 1 and no word break in front of a cut: every chunk starts on the token in front of the cut before)
    assert e["input_ids"].tolist() == [[1, 20, 21, 2, 9, 9], [1, 21, 22, 23, 24, 2], [1, 24, 25, 26, 27, 2], [1, 27, 28, 29, 2, 9], [1, 30, 2, 9, 9, 9], [9] * 6]
    assert e["window_doc"].tolist() == [0, 0, 0, 0, 1, 2] and e["window_start"].tolist() == [1, 2, 5, 8, 1, 0]
    assert e["cut_level"].tolist() == [WORD, WORD, TOKEN, CUT_LAST, CUT_LAST, CUT_LAST]
    assert e["chunk_bytes"].tolist() == [[3, 8], [6, 17], [15, 26], [24, 32], [36, 44], [0, 0]]
    assert e["spans"][0].tolist() == [[0, 2], [3, 5], [6, 8], [33, 35], [0, 0], [0, 0]] and e["mask"][3].tolist() == [1, 1, 1, 1, 1, 0]
    # a level byte above 5 reads as 5
    assert chunks_of([1, 1, 1, 9, 1, 5, 1, 1, 1], 6, 3, 0)["cut_level"].tolist() == [PARAGRAPH, CUT_LAST]
    assert chunks_of([1, 1, 1, 9, 1, 5, 1, 1, 1], 6, 3, 0)["window_start"].tolist() == [0, 5]


def random_case(rng, levels=None):
    T = int(rng.integers(1, 33))
    h = int(rng.integers(0, min(T, 3)))
    t = int(rng.integers(0, min(T - h, 4)))
    c = T - h - t
    m = int(rng.integers(1, c + 1))
    o = int(rng.integers(0, m))
    ids, oo = random_ragged(rng, int(rng.integers(1, 25)), int(rng.integers(1, 120)))
    lev = rng.integers(0, 6, len(ids)).astype(np.uint8) if levels is None else np.full(len(ids), levels, np.uint8)
    return ids, oo, lev, T, m, o, h, t


def test_invariants_on_random_input():
    rng = np.random.default_rng(41)
    for case in range(200):
        ids, oo, lev, T, m, o, h, t = random_case(rng)
        c = T - h - t
        e = expected_chunks(ids, oo, lev, T, m, o, h, t, (0, 4, 7)[case % 3], P, MASK | (FIXED if case & 1 else 0))
        n, dw = np.diff(oo), e["doc_windows"].astype(np.int64)
        assert dw[0] == 0 and dw[-1] == e["n_windows"] and np.all(np.diff(dw) > 0) and e["n_split"] == int(np.sum(n > T))
        made = [0] * 6
        for d in range(len(n)):
            nd, w, r0 = int(n[d]), int(dw[d + 1] - dw[d]), int(dw[d])
            doc = ids[int(oo[d]):int(oo[d + 1])].tolist()
            assert np.all(e["window_doc"][r0:r0 + w] == d)
            if nd <= T:
                assert w == 1 and e["input_ids"][r0][:nd].tolist() == doc and e["cut_level"][r0] == CUT_LAST and e["window_start"][r0] == min(h, nd)
                continue
            b = nd - h - t
            a = [int(x) - h for x in e["window_start"][r0:r0 + w]]
            en = [a[k] + int(e["lengths"][r0 + k]) - h - t for k in range(w)]
            assert a[0] == 0 and en[-1] == b and w <= 1 + -(-(b - c) // (m - o))
            for k in range(w):
                row = e["input_ids"][r0 + k][:int(e["lengths"][r0 + k])].tolist()
                assert row == doc[:h] + doc[h + a[k]:h + en[k]] + doc[nd - t:]
                if k + 1 < w:
                    assert a[k] < a[k + 1] <= en[k] < en[k + 1] and en[k] - a[k + 1] <= o and m <= en[k] - a[k] <= c
                    L = lev[int(oo[d]) + h:int(oo[d]) + h + b]
                    level = int(e["cut_level"][r0 + k])
                    assert level == L[en[k]] == max(L[a[k] + m:a[k] + c + 1]) and not np.any(L[en[k] + 1:a[k] + c + 1] == level)
                    made[level] += 1
                else:
                    assert e["cut_level"][r0 + k] == CUT_LAST and en[k] - a[k] <= c
        assert e["level_counts"].tolist() == made
        for r in range(e["n_windows"]):
            k = int(e["lengths"][r])
            assert np.all(e["input_ids"][r, k:] == P) and e["mask"][r].tolist() == [1] * k + [0] * (e["row_len"] - k)


def test_all_token_levels_are_the_windows():
    rng = np.random.default_rng(42)
    for case in range(150):
        ids, oo, lev, T, m, o, h, t = random_case(rng, levels=(TOKEN, WORD, PARAGRAPH)[case % 3] if case % 5 else TOKEN)
        flags = MASK | (FIXED if case & 1 else 0) | (I64 if case & 2 else 0)
        e = expected_chunks(ids, oo, lev, T, m, o, h, t, (0, 4)[case % 2], P, flags)
        w = expected_windows(ids, oo, T, o, h, t, (0, 4)[case % 2], P, flags)
        for k in ("input_ids", "mask", "lengths", "window_doc", "window_start", "doc_windows"):
            assert np.array_equal(e[k], w[k]), (case, k)
        assert (e["n_windows"], e["n_split"], e["row_len"]) == (w["n_windows"], w["n_split"], w["row_len"])


# every refused case (what, ids, oo, lev, T, m, o, h, t, multiple_of, flags, on_device): what the GPU test passes to the entries as
# well, but for the one whose offsets describe ids that do not exist -- the walk reads a level byte per candidate, so it is the
# restatement's alone (the entry refuses it by the same comparison, behind the walk)
def refused_cases():
    docs = [[1] + list(range(20, 30)) + [2], [1, 30, 2], [], [1] + list(range(40, 45)) + [2]]
    ids, oo = ragged(docs)
    lev = [1] * len(ids)
    big = [0] + [(i + 1) * 2 ** 31 for i in range(9)]
    return [("T == 0", ids, oo, lev, 0, 1, 0, 0, 0, 0, 0, True), ("h + t == T", ids, oo, lev, 6, 1, 0, 3, 3, 0, 0, True),
            ("h + t > T", ids, oo, lev, 6, 1, 0, 4, 3, 0, 0, True), ("m == 0", ids, oo, lev, 6, 0, 0, 1, 1, 0, 0, True),
            ("m > c", ids, oo, lev, 6, 5, 0, 1, 1, 0, 0, True), ("o == m", ids, oo, lev, 6, 2, 2, 1, 1, 0, 0, True),
            ("o > m", ids, oo, lev, 6, 2, 3, 1, 1, 0, 0, True), ("o >= c", ids, oo, lev, 6, 4, 4, 1, 1, 0, 0, True),
            ("unknown flag", ids, oo, lev, 6, 2, 1, 1, 1, 0, 32, True), ("unknown high flag", ids, oo, lev, 6, 2, 1, 1, 1, 0, 1 << 31, True),
            ("T beyond a row", ids, oo, lev, 2 ** 31, 2, 1, 1, 1, 0, 0, True),
            ("rounded L beyond a row", ids, oo, lev, 2 ** 31 - 1, 2, 1, 1, 1, 64, FIXED, True),
            ("W >= 2^32", [], big, [], 4, 4, 0, 0, 0, 0, FIXED, False),                   # 9 documents of 2^29 chunks each
            ("W * L > 2^36", [], [0] * 70, [], 2 ** 30, 1, 0, 0, 0, 0, FIXED, True),       # 69 rows of 2^30 elements
            ("spans without a buffer", ids, oo, lev, 6, 2, 1, 1, 1, 0, SPANS, True),
            ("chunk_bytes without a buffer", ids, oo, lev, 6, 2, 1, 1, 1, 0, BYTES, True),
            ("no level buffer", ids, oo, None, 6, 2, 1, 1, 1, 0, 0, True),
            ("ids without a document", ids, [0], lev, 6, 2, 1, 1, 1, 0, 0, True),
            ("a document of 2^32 - 1 ids", [], [0, 2 ** 32 - 1], [], 2 ** 20, 2, 1, 0, 0, 0, FIXED, True)]


def test_refused_options_raise():
    for what, ids, oo, lev, T, m, o, h, t, mo, flags, _ in refused_cases():
        with pytest.raises(ValueError):
            expected_chunks(ids, oo, lev, T, m, o, h, t, mo, P, flags, None)
    _, ids, oo, lev = refused_cases()[0][:4]            # (and the neighbours that are valid)
    expected_chunks(ids, oo, lev, 6, 4, 3, 1, 1, 0, P, 0)       # m = c, o = m - 1
    expected_chunks(ids, oo, lev, 3, 1, 0, 1, 1, 0, P, 0)       # c = 1
    expected_chunks([], [0] * 65, [], 2 ** 30, 1, 0, 0, 0, 0, P, 0)


def test_kernel_index_model_against_the_definition():
    """tools/chunk_model.py restates the wave walk and the fill kernel index by index and asserts that every read stays inside its
    array and that every output element is written once; its outputs equal the definition's at wave widths 4 and 64, with groups
    of a whole wave and of fewer documents, at fill tiles of 16 and 64 units and at the kernel's own."""
    import chunk_model
    rng = np.random.default_rng(43)
    for case in range(160):
        ids, oo, lev, T, m, o, h, t = random_case(rng, levels=None if case % 4 else TOKEN)
        if case % 7 == 0:
            lev[rng.integers(0, max(len(lev), 1), len(lev) // 3)] = PARAGRAPH     # (the early end of a scan)
        sp = np.stack([np.arange(len(ids)) * 2 + 1, np.arange(len(ids)) * 3 + 7], axis=1).astype(np.uint32)
        e = expected_chunks(ids, oo, lev, T, m, o, h, t, (0, 4, 8)[case % 3], P, (FIXED if case & 1 else 0) | BYTES, sp)
        width = (4, 64)[case & 1]
        group = (width, width, 1, 2)[(case >> 1) % 4]
        tile, cap = ((16, 4), (64, 8), (2048, 1024))[case % 3]
        got = chunk_model.chunk_model(ids.tolist(), [int(x) for x in oo], lev.tolist(), sp.tolist(), T, m, o, h, t, e["row_len"], P, width, group,
                                      tile, cap)
        assert np.array_equal(got["input_ids"], e["input_ids"]), case
        for k in ("lengths", "window_doc", "window_start", "doc_windows", "cut_level", "level_counts"):
            assert got[k] == e[k].tolist(), (case, k)
        assert got["chunk_bytes"] == e["chunk_bytes"].tolist() and got["n_split"] == e["n_split"]
    for case in range(12):                              # candidate ranges of several blocks of 64, strong breaks rare
        T = int(rng.integers(130, 300))
        m, o = int(rng.integers(1, T - 128)), 0
        o = int(rng.integers(0, min(m, 140)))
        ids, oo = random_ragged(rng, 6, 4 * T)
        lev = rng.choice(6, len(ids), p=[0.3, 0.55, 0.1, 0.03, 0.015, 0.005]).astype(np.uint8)
        sp = np.stack([np.arange(len(ids)) * 2 + 1, np.arange(len(ids)) * 3 + 7], axis=1).astype(np.uint32)
        e = expected_chunks(ids, oo, lev, T, m, o, 0, 0, 0, P, FIXED | BYTES, sp)
        got = chunk_model.chunk_model(ids.tolist(), [int(x) for x in oo], lev.tolist(), sp.tolist(), T, m, o, 0, 0, T, P, 64, (64, 2)[case & 1])
        assert np.array_equal(got["input_ids"], e["input_ids"]) and got["cut_level"] == e["cut_level"].tolist(), case
        assert got["window_start"] == e["window_start"].tolist() and got["level_counts"] == e["level_counts"].tolist()


def test_levels_model_against_the_definition():
    """... and the levels kernel's walk: the document slot of every id of a group of 16 documents, step by step."""
    import chunk_model
    rng = np.random.default_rng(44)
    alphabet = [b"a", b"b", b" ", b" ", b"\n", b".", b"!", b"\t", b"\xc3\xa9", b"\xe3\x80\x82", b"\xa9", b"\xef\xbc\x9f"]
    for case in range(40):
        docs = [b"".join(alphabet[i] for i in rng.integers(0, len(alphabet), int(rng.integers(0, 60)))) for _ in range(int(rng.integers(1, 40)))]
        for d in rng.integers(0, len(docs), len(docs) // 4):
            docs[d] = b""
        spans, oo = [], [0]
        for text in docs:                               # ids that begin anywhere, in order; a head at 0 and a tail at len
            starts = sorted(rng.integers(0, len(text) + 1, int(rng.integers(0, len(text) + 2))).tolist())
            starts = ([0] if case & 1 else []) + starts + ([len(text)] if case & 2 else [])
            spans += [(s, min(s + 2, len(text))) for s in starts]
            oo.append(len(spans))
        mask = (ALL_LEVELS, ALL_LEVELS & ~(1 << SENTENCE), 1 << LINE, 0)[case % 4]
        offs = np.concatenate([[0], np.cumsum([len(x) for x in docs])]).tolist()
        got = chunk_model.levels_model(b"".join(docs), offs, spans, oo, mask, (4, 64)[case & 1])
        assert got == expected_levels_batch(docs, oo, np.array(spans, np.int64).reshape(-1, 2), mask).tolist(), case


# ---- the declarations ----

def test_new_symbols_declared_in_header_and_shim():
    hdr = open(os.path.join(ROOT, "include", "tekken_hip.h")).read()
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bfn\s+%s\s*\(" % name, ffi), name
    for name, value in CONSTANTS.items():
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name
        assert re.search(r"\bconst %s\s*:\s*\w+\s*=\s*%d\s*;" % (name, value), ffi), name
    assert re.search(r"typedef struct tk_chunk_opts\b", hdr) and re.search(r"typedef struct tk_chunk\b", hdr)
    assert re.search(r"\bstruct TkChunkOpts\b", ffi) and re.search(r"\bstruct TkChunk\b", ffi)
    opts = re.search(r"typedef struct tk_chunk_opts\s*\{\s*uint32_t([^}]*);\s*\}", hdr).group(1)
    fields = re.search(r"pub struct TkChunkOpts \{(.*?)\}", ffi, re.S).group(1)
    assert [x.strip() for x in opts.split(",")] == re.findall(r"pub (\w+): u32,", fields)
    fields = re.search(r"pub struct TkChunk \{(.*?)\}", ffi, re.S).group(1)
    assert [m for m, _ in header_members("chunk")] == re.findall(r"pub (\w+):", fields)


def test_python_constants_match_the_header(tk):
    for name, value in CONSTANTS.items():
        assert getattr(tk, name[3:]) == value, name
    for name in NEW_SYMBOLS:
        assert hasattr(tk.lib(), name), name
    for name in ("chunk_levels_device", "chunk_from_ids_device", "encode_batch_device_chunk", "encode_batch_chunk", "last_chunk_ms"):
        assert hasattr(tk.Engine, name), name
    assert hasattr(tk, "ChunkResult") and hasattr(tk.Tekkenizer, "encode_batch_chunks")
    assert ctypes.sizeof(tk._ChunkOpts) == 36 and ctypes.sizeof(tk._Chunk) == 10 * ctypes.sizeof(ctypes.c_void_p) + 32
    hdr = open(os.path.join(ROOT, "include", "tekken_hip.h")).read()
    opts = re.search(r"typedef struct tk_chunk_opts\s*\{\s*uint32_t([^}]*);\s*\}", hdr).group(1)
    assert [x.strip() for x in opts.split(",")] == [f[0] for f in tk._ChunkOpts._fields_]
    assert all(f[1] is ctypes.c_uint32 for f in tk._ChunkOpts._fields_)


def test_result_class_declares_the_header_struct(tk):
    R = tk.ChunkResult
    members = header_members("chunk")
    assert R.PASS == "chunk" and R.I64 == tk.CHUNK_I64
    assert [o[0] for o in R.OUTPUTS] == [m for m, ptr in members if ptr]
    assert list(R.COUNTS) == [m for m, ptr in members if not ptr]
    assert [ptr for _, ptr in members] == sorted((ptr for _, ptr in members), reverse=True)        # pointers first: no padding
    assert ctypes.sizeof(R.STRUCT) == sum(ctypes.sizeof(ctypes.c_void_p) if ptr else 8 for _, ptr in members)
    assert [f[0] for f in R.STRUCT._fields_] == [m for m, _ in members]
    for (_, ptr), (_, ctype) in zip(members, R.STRUCT._fields_):
        assert ctype is (ctypes.c_void_p if ptr else ctypes.c_uint64)
    st = R.STRUCT()
    for i, (field, _) in enumerate(R.STRUCT._fields_):
        setattr(st, field, 0x1000 * (i + 1) if field in [o[0] for o in R.OUTPUTS] else i + 2)
    st.mask = None
    r = R(st, R.I64, 5)
    views = r.views()
    assert r.mask_ptr is None and views[1] is None and len(views) == 10 and r.typestr == "<i8"
    for (out, typestr, shape, _, _), v in zip(R.OUTPUTS, views):
        if out == "mask":
            continue
        cai = v.__cuda_array_interface__
        assert cai["data"][0] == getattr(st, out) == getattr(r, out + "_ptr") and cai["shape"] == tuple(shape(r)) and cai["typestr"] == (typestr or "<i8")
    assert views[7].__cuda_array_interface__["shape"] == (r.n_windows,) and views[8].__cuda_array_interface__["shape"] == (r.n_windows, 2)
    assert views[9].__cuda_array_interface__["shape"] == (6,) and set(r._counts()) == {"n_windows", "n_split"}


def test_host_only_tokenizer_has_no_chunks(tk, small_vocab):
    from test_host_tokenizer import model
    t = tk.Tekkenizer.from_json(json.dumps(model(small_vocab["tokens"])), device=-1)
    for kw in ({}, {"return_tensors": "np"}, {"overlap": 1, "min_length": 2, "dtype": "int32", "padding": "longest", "return_text": True}):
        with pytest.raises(tk.TokenizerError) as e:
            t.encode_batch_chunks(["hello world"], 4, **kw)
        assert e.value.code == tk.TK_ERR_NO_DEVICE
    t.close()
