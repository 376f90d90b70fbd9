"""Word ids (include/tekken_hip.h tk_words_from_ids_device, csrc/tk_words.hip), the parts that need no GPU: two restatements of
the definition that tests/test_gpu_words.py checks the kernels against -- A, the definition in plain loops, total; B, for
encode's own output, every piece encoded on its own --, their agreement on the spans sweep under both patterns, the numpy
restatement of encode_batch_padded_words, the declarations, and the host-only tokenizer."""
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
NEW_SYMBOLS = ["tk_words_from_ids_device", "tk_encode_batch_device_words", "tk_encode_batch_words", "tk_free_words", "tk_last_words_ms"]


def starts_of(doc, split):
    return list(split(doc)) if len(doc) else []


def expected_words(ids, id_offs, tokens, ns, data, offs, split):
    """Restatement A: the definition of the header, id by id.  Total: any ids, specials anywhere, text longer or shorter than the
    document.  -> dict(word_ids uint32[n_ids], doc_words uint64[D + 1], word_first uint32[n_words], n_words, per_doc)."""
    word_ids, word_first, per_doc = [], [], []
    raw = bytes(np.asarray(data, np.uint8))
    for d in range(len(id_offs) - 1):
        doc = raw[int(offs[d]):int(offs[d + 1])]
        F = set(starts_of(doc, split))
        pos = count = 0
        for k, i in enumerate(ids[int(id_offs[d]):int(id_offs[d + 1])]):
            i = int(i)
            s, e = pos, pos + (len(tokens[i - ns]) if i >= ns else 0)
            pos = e
            if s < e and s < len(doc) and s in F:
                count += 1
                word_first.append(k)
            word_ids.append(NONE if s == e else (count - 1) & 0xFFFFFFFF)
        per_doc.append(count)
    dw = np.zeros(len(per_doc) + 1, np.uint64)
    if per_doc:
        dw[1:] = np.cumsum(per_doc)
    return {"word_ids": np.array(word_ids, np.uint32), "doc_words": dw, "word_first": np.array(word_first, np.uint32),
            "n_words": int(dw[-1]), "per_doc": per_doc}


def first_unaligned(ids, id_offs, tokens, ns, data, offs, split):
    """TK_WORDS_CHECK_ALIGNED restated: the first document whose ids' text is not exactly as long as the document, or that has a
    piece start strictly inside a token's span -- (document, document-relative index of its first such id or None), or None."""
    raw = bytes(np.asarray(data, np.uint8))
    for d in range(len(id_offs) - 1):
        doc = raw[int(offs[d]):int(offs[d + 1])]
        F = set(starts_of(doc, split))
        pos, inside = 0, None
        for k, i in enumerate(ids[int(id_offs[d]):int(id_offs[d + 1])]):
            s, e = pos, pos + (len(tokens[int(i) - ns]) if int(i) >= ns else 0)
            pos = e
            if inside is None and any(p in F for p in range(s + 1, min(e, len(doc)))):
                inside = k
        if pos != len(doc) or inside is not None:
            return d, inside
    return None


def words_by_piece(orc, docs, split, add_bos, add_eos):
    """Restatement B, encode's own output only: every piece encoded on its own, its index once per id.  -> (word_ids uint32,
    pieces per document)."""
    out, per_doc = [], []
    for doc in docs:
        st = starts_of(doc, split) + [len(doc)]
        if add_bos:
            out.append(NONE)
        for w in range(len(st) - 1):
            out += [w] * len(orc.encode(doc[st[w]:st[w + 1]]))
        if add_eos:
            out.append(NONE)
        per_doc.append(len(st) - 1)
    return np.array(out, np.uint32), per_doc


def expected_padded_words(ids, oo, word_ids, add_bos, add_eos, max_length, padding, truncation_side, padding_side, multiple_of, pad_id, dtype):
    """encode_batch_padded_words restated: the kept POSITIONS of every row are chosen once (BOS / EOS survive), and input_ids and
    word_ids are read at them; word_ids under a special id and under the padding is -1."""
    oo = np.asarray(oo, np.int64)
    T, h, t = int(max_length or 0), int(bool(add_bos)), int(bool(add_eos))
    keep = []
    for d in range(len(oo) - 1):
        idx = list(range(int(oo[d]), int(oo[d + 1])))
        n = len(idx)
        if T and n > T:
            idx = idx[:h] + idx[n - (T - h):] if truncation_side == "left" else idx[:T - t] + (idx[n - t:] if t else [])
        keep.append(idx)
    L = T if padding == "max_length" else min(max([len(k) for k in keep], default=0), T or (1 << 62))
    if multiple_of:
        L = (L + multiple_of - 1) // multiple_of * multiple_of
    dt = np.int64 if dtype == "int64" else np.int32
    inp, wid, mask = np.full((len(keep), L), pad_id, dt), np.full((len(keep), L), -1, dt), np.zeros((len(keep), L), np.uint8)
    w = np.asarray(word_ids, np.uint32).view(np.int32)
    for d, k in enumerate(keep):
        sl = slice(L - len(k), L) if padding_side == "left" else slice(0, len(k))
        inp[d, sl], wid[d, sl], mask[d, sl] = np.asarray(ids, np.int64)[k], w[k], 1
    return {"input_ids": inp, "word_ids": wid, "attention_mask": mask, "lengths": np.array([len(k) for k in keep], np.int32),
            "n_truncated": sum(1 for d in range(len(keep)) if len(keep[d]) < oo[d + 1] - oo[d])}


# ---- hand-made: the 256 bytes + two longer tokens; the split stands in for a pattern ----
NS = 3
TOKENS = [bytes([b]) for b in range(256)] + [b"hello", b" wor", b"b c"]


def tid(tok):
    return NS + TOKENS.index(tok)


def by_spaces(doc):
    """A stand-in split: a piece starts at 0 and at every space."""
    return [p for p in range(len(doc)) if p == 0 or doc[p] == 0x20]


def test_restatement_a_hand_made():
    doc = b"hello world"
    ids = [1, tid(b"hello"), tid(b" wor"), tid(b"l"), tid(b"d"), 2]
    data = np.frombuffer(doc, np.uint8)
    got = expected_words(ids, [0, len(ids)], TOKENS, NS, data, [0, len(doc)], by_spaces)
    assert got["word_ids"].tolist() == [NONE, 0, 1, 1, 1, NONE]
    assert got["doc_words"].tolist() == [0, 2] and got["word_first"].tolist() == [1, 2] and got["per_doc"] == [2]
    # a special in mid-document is None and does not end the word; a token that crosses a piece start begins no word
    ids = [tid(b"a"), 0, tid(b"b c"), tid(b"d")]
    doc = b"ab cd"
    got = expected_words(ids, [0, len(ids)], TOKENS, NS, np.frombuffer(doc, np.uint8), [0, len(doc)], by_spaces)
    assert got["word_ids"].tolist() == [0, NONE, 0, 0] and got["per_doc"] == [1] and got["word_first"].tolist() == [0]
    # ids in front of the first begins wrap to None; text beyond the document begins nothing; two documents, one without ids
    ids = [tid(b"x"), tid(b" "), tid(b"y"), tid(b" "), tid(b"z")]
    data = np.frombuffer(b"Q Yab", np.uint8)
    got = expected_words(ids, [0, 5, 5], TOKENS, NS, data, [0, 3, 5], lambda doc: [1] if doc == b"Q Y" else by_spaces(doc))
    assert got["word_ids"].tolist() == [NONE, 0, 0, 0, 0] and got["per_doc"] == [1, 0] and got["doc_words"].tolist() == [0, 1, 1]
    assert got["word_first"].tolist() == [1]
    got = expected_words([], [0, 0], TOKENS, NS, np.zeros(0, np.uint8), [0, 0], by_spaces)
    assert got["n_words"] == 0 and got["doc_words"].tolist() == [0, 0] and len(got["word_ids"]) == 0


@pytest.mark.parametrize("pattern", [0, 1])
def test_restatements_agree_on_the_sweep(test_vocab, pattern):
    """A (the definition over the oracle's ids) and B (piece by piece) on the documents the spans sweep runs, empty documents, a
    70 000-byte word and invalid UTF-8 among them; every piece of encode's output is a run of whole tokens: n_words = |F_d|."""
    import helpers
    import tk_oracle
    from test_gpu_spans import pack, sweep_docs
    from test_gpu_spans_units import INVALID
    docs = sweep_docs() + list(INVALID)
    data, offs = pack(docs)
    v = test_vocab
    orc = helpers.oracle_for(v)
    orc.set_pattern(pattern)
    split = tk_oracle.split_tekken if pattern else tk_oracle.split
    for bos, eos in ((False, False), (True, True)):
        ids, oo = orc.encode_batch(data, offs, bos, eos, threads=4)
        a = expected_words(ids, oo, v["tokens"], v["num_special"], data, offs, split)
        b, pieces = words_by_piece(orc, docs, split, bos, eos)
        bad = np.nonzero(a["word_ids"] != b)[0]
        assert len(a["word_ids"]) == len(b) and len(bad) == 0, ("first differing id", int(bad[0]) if len(bad) else None)
        assert a["per_doc"] == pieces
        # word_first: strictly increasing inside a document, and the word of the id it names is the word's index
        dw = a["doc_words"].astype(np.int64)
        for d in range(len(docs)):
            wf = a["word_first"][dw[d]:dw[d + 1]].astype(np.int64)
            assert np.all(np.diff(wf) > 0)
            assert np.array_equal(a["word_ids"][int(oo[d]) + wf], np.arange(len(wf), dtype=np.uint32))


def test_kernel_model_agrees_with_restatement_a():
    """tools/words_model.py, the words kernel's step over 64 lanes, on random batches: ids that are not the text's own, specials
    and empty tokens anywhere, empty documents, several document starts in one step, documents of several steps."""
    import words_model
    rng = np.random.default_rng(1)
    tokens = [bytes([b]) for b in range(256)] + [b"ab", b" cd", b"x" * 5, b"", b"hello world", b"q" * 40]
    tok_len = [len(t) for t in tokens]
    pool = [0, 1, 2, NS + 0x61, NS + 0x20] + [NS + 256 + k for k in range(6)]

    def split(doc):
        return [p for p in range(len(doc)) if p == 0 or doc[p] == 0x20 or (doc[p - 1] == 0x20 and p % 3 == 0)]

    for trial in range(60):
        n_docs = int(rng.integers(0, 40))
        docs = [bytes(rng.choice(np.frombuffer(b"ab cdx \nq", np.uint8), int(rng.choice([0, 0, 1, 3, 10, 70, 200])))) for _ in range(n_docs)]
        rows = [[int(x) for x in rng.choice(pool, int(rng.choice([0, 1, 5, 63, 64, 65, 130, 200])))] for _ in range(n_docs)]
        data = np.frombuffer(b"".join(docs), np.uint8)
        offs = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
        ids = np.array(sum(rows, []), np.int64)
        oo = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        flags = np.zeros(len(data) + 64, np.uint8)
        for d, doc in enumerate(docs):
            flags[offs[d] + np.array(split(doc), np.int64)] = 1
        exp = expected_words(ids, oo, tokens, NS, data, offs, split)
        w, nw, _ = words_model.kernel(ids, oo, offs, flags, tok_len, NS, 0)
        assert np.array_equal(w, exp["word_ids"].astype(np.int64)) and nw.tolist() == exp["per_doc"], trial
        wf = words_model.kernel(ids, oo, offs, flags, tok_len, NS, 1, exp["doc_words"].astype(np.int64))[2]
        assert np.array_equal(wf, exp["word_first"].astype(np.int64)), trial


def test_padded_words_restatement_hand_made():
    # two rows with BOS and EOS: 6 and 3 ids; words 0 0 1 1 and 0
    ids = [1, 50, 51, 52, 53, 2, 1, 60, 2]
    words = [NONE, 0, 0, 1, 1, NONE, NONE, 0, NONE]
    kw = dict(add_bos=True, add_eos=True, multiple_of=0, pad_id=9, dtype="int64")
    r = expected_padded_words(ids, [0, 6, 9], words, max_length=4, padding="longest", truncation_side="right", padding_side="right", **kw)
    assert r["input_ids"].tolist() == [[1, 50, 51, 2], [1, 60, 2, 9]] and r["word_ids"].tolist() == [[-1, 0, 0, -1], [-1, 0, -1, -1]]
    assert r["lengths"].tolist() == [4, 3] and r["n_truncated"] == 1 and r["word_ids"].dtype == np.int64
    r = expected_padded_words(ids, [0, 6, 9], words, max_length=4, padding="longest", truncation_side="left", padding_side="left", **kw)
    assert r["input_ids"].tolist() == [[1, 52, 53, 2], [9, 1, 60, 2]] and r["word_ids"].tolist() == [[-1, 1, 1, -1], [-1, -1, 0, -1]]
    assert r["attention_mask"].tolist() == [[1, 1, 1, 1], [0, 1, 1, 1]]
    kw.update(multiple_of=4, dtype="int32")
    r = expected_padded_words(ids, [0, 6, 9], words, max_length=None, padding="longest", truncation_side="right", padding_side="right", **kw)
    assert r["input_ids"].shape == (2, 8) and r["word_ids"][0].tolist() == [-1, 0, 0, 1, 1, -1, -1, -1] and r["word_ids"].dtype == np.int32
    r = expected_padded_words(ids, [0, 6, 9], words, max_length=5, padding="max_length", truncation_side="right", padding_side="right", **kw)
    assert r["input_ids"].shape == (2, 8) and r["input_ids"][0].tolist() == [1, 50, 51, 52, 2, 9, 9, 9]


def test_new_symbols_declared_in_header_and_binding(tk):
    hdr = open(os.path.join(ROOT, "include", "tekken_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        fn = getattr(tk.lib(), name, None)
        assert fn is not None and fn.argtypes, name
    for name, val in (("TK_WORD_NONE", "0xFFFFFFFFu"), ("TK_WORDS_FIRST", "1u"), ("TK_WORDS_CHECK_ALIGNED", "32")):
        assert re.search(r"#define %s %s\b" % (name, val), hdr), name
    assert (tk.WORD_NONE, tk.WORDS_FIRST, tk.WORDS_CHECK_ALIGNED) == (NONE, 1, 32)
    # the check bit sits above every other check bit, so one word can carry them all
    assert tk.WORDS_CHECK_ALIGNED > max(tk.CHECK_OFFSETS, tk.CHECK_UTF8, tk.SPANS_CHECK_COVER, tk.SPANS_CHECK_BYTES, tk.CHECK_PARTS)


def test_words_result_declares_the_header_struct_once(tk):
    import ctypes
    from test_layout_binding_cpu import header_members
    R = tk.WordsResult
    members = header_members("words")
    assert R.PASS == "words" and issubclass(R, tk._LayoutResult)
    assert [o[0] for o in R.OUTPUTS] == [m for m, ptr in members if ptr] == ["word_ids", "doc_words", "word_first"]
    assert list(R.COUNTS) == [m for m, ptr in members if not ptr]
    assert [f[0] for f in R.STRUCT._fields_] == [m for m, _ in members]
    assert ctypes.sizeof(R.STRUCT) == 8 * len(members) and ctypes.sizeof(tk._WordsOpts) == 4
    st = R.STRUCT(0x1000, 0x2000, None, 3, 7, 5)
    r = R(st)
    assert (r.word_ids_ptr, r.doc_words_ptr, r.word_first_ptr, r.n_docs, r.n_ids, r.n_words) == (0x1000, 0x2000, None, 3, 7, 5)
    v = r.views()
    assert v[2] is None and v[0].__cuda_array_interface__["shape"] == (7,) and v[1].__cuda_array_interface__["shape"] == (4,)
    assert v[0].__cuda_array_interface__["typestr"] == "<i4" and v[1].__cuda_array_interface__["typestr"] == "<i8"
    # the C side describes the struct once as well: in layout_outputs, from which tk_free_words and the copy-out are made
    lay = open(os.path.join(ROOT, "tekken-rs_amd", "csrc", "tk_capi_layout.h")).read()
    m = re.search(r"layout_outputs\(tk_words& r.*?\n\}", lay, re.S)
    assert m and re.findall(r"f\(r\.(\w+),", m.group(0)) == ["word_ids", "doc_words", "word_first"]
    src = open(os.path.join(ROOT, "tekken-rs_amd", "csrc", "tk_capi_words.cpp")).read()
    assert "layout_free(r)" in src and "layout_copy_out(c, r" in src and "tk_pinned_put" not in src


def test_host_only_tokenizer_has_no_words(tk, small_vocab):
    from test_host_tokenizer import model
    t = tk.Tekkenizer.from_json(json.dumps(model(small_vocab["tokens"])), device=-1)
    try:
        for call in (lambda: t.encode_with_words("hello world", True, True), lambda: t.encode_batch_with_words(["hello world"]),
                     lambda: t.encode_batch_padded_words(["hello world"])):
            with pytest.raises(tk.TokenizerError) as e:
                call()
            assert e.value.code == tk.TK_ERR_NO_DEVICE
    finally:
        t.close()
