"""Spans in code points / UTF-16 units and the annotation -> token range look-up (include/tekken_hip.h
tk_token_spans_units_device, tk_spans_locate_device), the parts that need no GPU: two restatements of the definition that
tests/test_gpu_spans_units.py checks the kernels against, Python's own str semantics on their output, the brute-force restatement
of the look-up, the per-rank table builder as a stand-alone sanitized program, the declarations, and the host-only tokenizer."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTE, CHAR, UTF16 = 0, 1, 2
NEW_SYMBOLS = ["tk_token_spans_units_device", "tk_encode_batch_device_spans_units", "tk_encode_batch_spans_units", "tk_spans_locate_device"]


def doc_text(ids, tokens, ns):
    """T of the definition and the byte span of every id: the concatenation of the non-special ids' token bytes."""
    T, spans = bytearray(), []
    for i in ids:
        s = len(T)
        if i >= ns:
            T += tokens[i - ns]
        spans.append((s, len(T)))
    return bytes(T), spans


def is_start(b):
    return (b & 0xC0) != 0x80


def weight(b, unit):
    if unit == BYTE:
        return 1
    return (1 if is_start(b) else 0) + (1 if unit == UTF16 and b >= 0xF0 else 0)


def unit_spans_bytewise(ids, id_offs, tokens, ns, unit):
    """The definition, restated byte by byte with plain loops: U(p) = the weights of the bytes in front of p, lead(p) = the
    last character start at or before p (0 without one).  -> int64[n_ids, 2], relative to the start of the id's document."""
    out = []
    for d in range(len(id_offs) - 1):
        T, spans = doc_text([int(i) for i in ids[int(id_offs[d]):int(id_offs[d + 1])]], tokens, ns)
        U = [0] * (len(T) + 1)
        for p in range(len(T)):
            U[p + 1] = U[p] + weight(T[p], unit)
        for s, e in spans:
            if s == e:
                out.append((U[s], U[s]))
                continue
            q = s
            if unit != BYTE:
                while q > 0 and not is_start(T[q]):
                    q -= 1
                if not is_start(T[q]):
                    q = 0
            out.append((U[q], U[e]))
    return np.array(out, np.int64).reshape(len(out), 2)


def unit_spans_str(ids, id_offs, tokens, ns, unit):
    """The same on VALID UTF-8, by walking the decoded str character by character: a token covers the characters it shares a
    byte with, from the first one's index to behind the last one's."""
    out = []
    for d in range(len(id_offs) - 1):
        T, spans = doc_text([int(i) for i in ids[int(id_offs[d]):int(id_offs[d + 1])]], tokens, ns)
        text = T.decode("utf-8")
        char_of, first, last, u = [], [], [], 0        # per byte: its character; per character: its first unit, behind its last
        for k, ch in enumerate(text):
            w = 1 if unit == CHAR else (2 if ord(ch) >= 0x10000 else 1)
            if unit == BYTE:
                w = len(ch.encode("utf-8"))
            first.append(u)
            u += w
            last.append(u)
            char_of += [k] * len(ch.encode("utf-8"))
        assert len(char_of) == len(T)
        for s, e in spans:
            if s == e:                                  # (in valid text a special sits between two characters)
                at = first[char_of[s]] if s < len(T) else u
                out.append((at, at))
            elif unit == BYTE:
                out.append((s, e))
            else:
                out.append((first[char_of[s]], last[char_of[e - 1]]))
    return np.array(out, np.int64).reshape(len(out), 2)


def widened_bytes(T, s, e):
    """The byte range of the characters a token with byte span (s, e), s < e, is widened to."""
    q = s
    while q > 0 and not is_start(T[q]):
        q -= 1
    r = e
    while r < len(T) and not is_start(T[r]):
        r += 1
    return q, r


def locate_brute(spans, id_offs, ann_doc, ann):
    """Part 3, restated: lo = #{i : E_i <= as}, hi = #{i : S_i < ae} over the spans of the annotation's document -> (lo, max(lo, hi))."""
    out = []
    for d, (a0, a1) in zip(ann_doc, ann):
        sp = spans[int(id_offs[d]):int(id_offs[d + 1])]
        lo = sum(1 for s, e in sp if e <= a0)
        hi = sum(1 for s, e in sp if s < a1)
        out.append((lo, max(lo, hi)))
    return np.array(out, np.int64).reshape(len(out), 2)


# ---- a byte vocabulary + a few longer tokens: ids of a text by greedy longest match (any tiling of the text will do here) ----
NS = 3                                                   # 0 <unk>, 1 BOS, 2 EOS
TOKENS = [bytes([b]) for b in range(256)] + [b"hello", " wor".encode(), "é".encode(), "中".encode(), "\U0001f680".encode(),
                                             b"\xf0\x9f", b"\x9a\x80", "a中".encode() + b"\xf0", b"\x80a", b"\x80\x80"]


def tid(tok):
    return NS + TOKENS.index(tok)


def greedy_ids(raw):
    ids, p = [], 0
    by_len = sorted(range(len(TOKENS)), key=lambda r: -len(TOKENS[r]))
    while p < len(raw):
        r = next(r for r in by_len if raw.startswith(TOKENS[r], p))
        ids.append(NS + r)
        p += len(TOKENS[r])
    return ids


def byte_ids(raw):
    return [NS + b for b in raw]


def spans_of(ids, unit):
    return unit_spans_bytewise(ids, [0, len(ids)], TOKENS, NS, unit).tolist()


def test_hand_made_cases():
    # ASCII: characters are bytes
    ids = [1] + greedy_ids(b"hello world") + [2]
    assert spans_of(ids, BYTE) == spans_of(ids, CHAR) == spans_of(ids, UTF16)
    assert spans_of(ids, CHAR)[:3] == [[0, 0], [0, 5], [5, 9]] and spans_of(ids, CHAR)[-1] == [11, 11]
    # "é🚀中" as whole-character tokens: 2 + 4 + 3 bytes, 1 + 1 + 1 code points, 1 + 2 + 1 UTF-16 units
    ids = [tid("é".encode()), tid("\U0001f680".encode()), tid("中".encode())]
    assert spans_of(ids, BYTE) == [[0, 2], [2, 6], [6, 9]]
    assert spans_of(ids, CHAR) == [[0, 1], [1, 2], [2, 3]]
    assert spans_of(ids, UTF16) == [[0, 1], [1, 3], [3, 4]]
    # an emoji as four byte tokens behind "ab": all four are the whole character; BOS / EOS sit at 0 and at the end
    ids = [1] + byte_ids(b"ab" + "\U0001f680".encode()) + [2]
    assert spans_of(ids, CHAR) == [[0, 0], [0, 1], [1, 2], [2, 3], [2, 3], [2, 3], [2, 3], [3, 3]]
    assert spans_of(ids, UTF16) == [[0, 0], [0, 1], [1, 2], [2, 4], [2, 4], [2, 4], [2, 4], [4, 4]]
    # ... and as two halves, with a special between them: the carry goes through it
    ids = [tid(b"\xf0\x9f"), 0, tid(b"\x9a\x80")]
    assert spans_of(ids, CHAR) == [[0, 1], [1, 1], [0, 1]]
    assert spans_of(ids, UTF16) == [[0, 2], [2, 2], [0, 2]]
    # a document that starts with continuation bytes: lead = 0 there, and they weigh nothing
    ids = byte_ids(b"\x98\x80") + [tid(b"\x80a"), tid(b"hello")]
    assert spans_of(ids, CHAR) == [[0, 0], [0, 0], [0, 1], [1, 6]]
    # one that ends in a truncated lead byte; a token that ends inside a character it began ("a中" + a lead) and the rest of it
    ids = [tid(b"hello"), tid("a中".encode() + b"\xf0"), tid(b"\x80\x80"), NS + 0x80, NS + 0xe4]
    assert spans_of(ids, CHAR) == [[0, 5], [5, 8], [7, 8], [7, 8], [8, 9]]
    assert spans_of(ids, UTF16) == [[0, 5], [5, 9], [7, 9], [7, 9], [9, 10]]
    # nothing carries across a document boundary
    ids = byte_ids(b"a\xf0\x9f") + byte_ids(b"\x98\x80b")
    got = unit_spans_bytewise(ids, [0, 3, 3, 6], TOKENS, NS, CHAR).tolist()
    assert got == [[0, 1], [1, 2], [1, 2], [0, 0], [0, 0], [0, 1]]
    assert unit_spans_bytewise([], [0, 0, 0], TOKENS, NS, CHAR).shape == (0, 2)


VALID_TEXTS = ["", "a", "hello world", "é\U0001f680中", "ab\U0001f680\U0001f680 wor中é", "中中hello\U0001f680", "\U0001f680", "ééé wor"]


def tilings(text):
    raw = text.encode("utf-8")
    yield greedy_ids(raw)
    yield byte_ids(raw)
    yield [1] + greedy_ids(raw) + [2]
    yield [1] + byte_ids(raw) + [2]


def test_the_two_restatements_agree_and_match_python_str():
    for text in VALID_TEXTS:
        raw = text.encode("utf-8")
        u16 = text.encode("utf-16-le")
        for ids in tilings(text):
            offs = [0, len(ids)]
            T, bspans = doc_text(ids, TOKENS, NS)
            assert T == raw
            for unit in (BYTE, CHAR, UTF16):
                a = unit_spans_bytewise(ids, offs, TOKENS, NS, unit)
                assert np.array_equal(a, unit_spans_str(ids, offs, TOKENS, NS, unit)), (text, unit)
                assert np.all(a[1:, 0] >= a[:-1, 0]) and np.all(a[1:, 1] >= a[:-1, 1])        # what the look-up relies on
            ch = unit_spans_bytewise(ids, offs, TOKENS, NS, CHAR).tolist()
            w = unit_spans_bytewise(ids, offs, TOKENS, NS, UTF16).tolist()
            for (s, e), (cs, ce), (ws, we) in zip(bspans, ch, w):
                if s == e:
                    assert cs == ce and ws == we and text[:cs].encode("utf-8") == raw[:s]
                    continue
                q, r = widened_bytes(raw, s, e)
                assert text[cs:ce].encode("utf-8") == raw[q:r]
                assert u16[2 * ws:2 * we] == raw[q:r].decode("utf-8").encode("utf-16-le")


def test_restatement_on_random_bytes_keeps_its_invariants():
    """Invalid UTF-8 included: spans stay ordered, a unit never exceeds the bytes, the last end is U(len)."""
    rng = np.random.default_rng(11)
    alphabet = np.array([0x61, 0x20, 0x80, 0xBF, 0xC3, 0xE4, 0xF0, 0x9F, 0xFF], np.uint8)
    for _ in range(40):
        raw = bytes(alphabet[rng.integers(0, len(alphabet), int(rng.integers(0, 24)))])
        ids = greedy_ids(raw)
        for unit in (CHAR, UTF16):
            a = unit_spans_bytewise(ids, [0, len(ids)], TOKENS, NS, unit)
            b = unit_spans_bytewise(ids, [0, len(ids)], TOKENS, NS, BYTE)
            assert np.all(a[:, 0] <= a[:, 1]) and np.all(a[1:, 0] >= a[:-1, 0]) and np.all(a[1:, 1] >= a[:-1, 1])
            if len(a):
                assert a[-1, 1] == sum(weight(x, unit) for x in raw) and np.all(a[:, 1] <= b[:, 1] * (2 if unit == UTF16 else 1))


def test_locate_is_the_overlap_set_exhaustively():
    """The contiguity claim: for every (as, ae) of a short document the ids whose span overlaps [as, ae) are exactly lo .. hi - 1."""
    texts = ["hello wor中é", "ab\U0001f680\U0001f680cd", "é\U0001f680中", "", "中"]
    assert all(len(t) <= 12 for t in texts)
    for text in texts:
        for ids in tilings(text):
            for unit in (BYTE, CHAR, UTF16):
                sp = unit_spans_bytewise(ids, [0, len(ids)], TOKENS, NS, unit).tolist()
                n = max([e for _, e in sp], default=0)
                for a0 in range(n + 1):
                    for a1 in range(a0, n + 1):
                        lo, hi = locate_brute(sp, [0, len(ids)], [0], [(a0, a1)])[0]
                        overlap = [i for i, (s, e) in enumerate(sp) if s < a1 and e > a0]
                        assert overlap == list(range(lo, hi)), (text, unit, a0, a1)
                        if a1 > a0:                     # BOS / EOS are never inside a non-empty range
                            assert all(ids[i] >= NS for i in overlap)
    # char_to_token(c) is the annotation (c, c + 1)
    ids = [1] + byte_ids("a\U0001f680".encode()) + [2]
    sp = spans_of(ids, CHAR)
    assert locate_brute(sp, [0, len(ids)], [0, 0], [(0, 1), (1, 2)]).tolist() == [[1, 2], [2, 6]]
    # documents without ids, an annotation beyond the text
    assert locate_brute([], [0, 0], [0], [(0, 3)]).tolist() == [[0, 0]]
    assert locate_brute(sp, [0, len(ids)], [0], [(5, 9)]).tolist() == [[len(ids), len(ids)]]


def test_new_symbols_declared_in_header_and_shim():
    hdr = open(os.path.join(ROOT, "include", "tekken_hip.h")).read()
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bfn\s+%s\s*\(" % name, ffi), name
    for name, val in (("TK_UNIT_BYTE", 0), ("TK_UNIT_CHAR", 1), ("TK_UNIT_UTF16", 2)):
        assert re.search(r"#define %s %d\b" % (name, val), hdr), name
        assert re.search(r"pub const %s: c_int = %d;" % (name, val), ffi), name
    assert "Character offsets are not provided" not in hdr


def test_python_constants_and_library_symbols(tk):
    assert (tk.UNIT_BYTE, tk.UNIT_CHAR, tk.UNIT_UTF16) == (BYTE, CHAR, UTF16)
    for name in NEW_SYMBOLS:
        assert hasattr(tk.lib(), name), name


def test_host_only_tokenizer_has_no_unit_offsets(tk, small_vocab):
    from test_host_tokenizer import model
    t = tk.Tekkenizer.from_json(json.dumps(model(small_vocab["tokens"])), device=-1)
    try:
        calls = [lambda: t.encode_with_offsets("hello world", True, True, offsets_unit="char"),
                 lambda: t.encode_with_offsets("hello world", offsets_unit="utf16"),
                 lambda: t.encode_batch_with_offsets(["hello world"], offsets_unit="char"),
                 lambda: t.encode_batch_windows(["hello world"], 8, return_offsets_mapping=True, offsets_unit="char"),
                 lambda: t.encode_batch_with_alignment(["hello world"], [[(0, 5)]])]
        for call in calls:
            with pytest.raises(tk.TokenizerError) as e:
                call()
            assert e.value.code == tk.TK_ERR_NO_DEVICE
    finally:
        t.close()


# ---- the table builder, stand-alone and sanitized ----
def entry_of(tok):
    """The 16-bit entry of csrc/tk_units_table.h, restated; and the counts."""
    starts = [k for k, b in enumerate(tok) if is_start(b)]
    n_start, n_four = len(starts), sum(1 for b in tok if b >= 0xF0)
    first = 1 if not tok or is_start(tok[0]) else 0           # (a token of no bytes: its span is (U(s), U(s)), like a special's)
    last4 = 1 if starts and tok[starts[-1]] >= 0xF0 else 0
    if n_start >= 0xFF or n_four > 63:
        return 0xFF, (n_start, n_four, first, last4)
    return n_start | (n_four << 8) | (first << 14) | (last4 << 15), (n_start, n_four, first, last4)


def test_table_builder_standalone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "units_table_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "units_table_check.cpp")])
    toks = [b"hello",                                   # ASCII
            b"\x80a",                                   # starts with a continuation byte
            "a中".encode() + b"\xf0",                    # ends in a truncated lead
            "\U0001f680".encode(),                      # a 4-byte character
            ("中" * 100),                                # 300 bytes
            b"\x80\xbf\x9f",                            # no character start at all
            b"", b"\xf0", "\U0001f680".encode() * 63, "\U0001f680".encode() * 64, b"a" * 254, b"a" * 255, b"a" * 300,
            ("中" * 85).encode() + b"\xe4", b"\xff\xfe"]
    toks = [t.encode() if isinstance(t, str) else t for t in toks]
    assert len(toks[4]) == 300
    r = subprocess.run([exe], input="".join(t.hex() + "\n" for t in toks).encode(), capture_output=True, timeout=60)
    assert r.returncode == 0, r.stderr.decode()
    rows = [[int(x) for x in line.split()] for line in r.stdout.decode().splitlines()]
    assert len(rows) == len(toks)
    for tok, row in zip(toks, rows):
        entry, counts = entry_of(tok)
        assert row[0] == entry and tuple(row[1:]) == counts, (tok, row, entry, counts)
    # what the kernel reads out of an entry, against the definition's own terms, for both units
    for tok, row in zip(toks, rows):
        e = row[0]
        if (e & 0xFF) == 0xFF:
            assert len(tok) >= 64                        # only a long token takes the byte-counting path
            continue
        n_start, n_four, last4 = e & 0xFF, (e >> 8) & 63, e >> 15
        assert n_start == sum(weight(b, CHAR) for b in tok) and n_start + n_four == sum(weight(b, UTF16) for b in tok)
        if n_start:
            at = max(k for k, b in enumerate(tok) if is_start(b))
            assert n_start - 1 == sum(weight(b, CHAR) for b in tok[:at])
            assert n_start - 1 + n_four - last4 == sum(weight(b, UTF16) for b in tok[:at])
        assert bool(e & (1 << 14)) == bool(not tok or is_start(tok[0]))
