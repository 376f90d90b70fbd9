"""Word ids on the GPU (include/tekken_hip.h tk_words_from_ids_device and the entries around it, csrc/tk_words.hip) against the
restatements of the definition in tests/test_words_cpu.py: A, id by id, for any ids; B, piece by piece, for encode's own output.
Everything is an integer: every comparison is exact."""
import ctypes
import json

import numpy as np
import pytest

import helpers
import tk_oracle
from helpers import dev, on_device, to_host
from test_gpu_spans import pack, sweep_docs
from test_gpu_spans_units import INVALID
from test_words_cpu import NONE, expected_padded_words, expected_words, first_unaligned, words_by_piece

pytestmark = pytest.mark.gpu

ARRAYS = ("word_ids", "doc_words", "word_first")
SPLITS = {0: tk_oracle.split, 1: tk_oracle.split_tekken}


def fetch(res):
    """WordsResult -> dict like expected_words'."""
    v = res.views()
    return {"word_ids": to_host(v[0], (res.n_ids,), np.uint32), "doc_words": to_host(v[1], (res.n_docs + 1,), np.uint64),
            "word_first": to_host(v[2], (res.n_words,), np.uint32), "n_words": res.n_words}


def assert_words(got, exp, what="", first=True):
    assert got["n_words"] == exp["n_words"], (what, got["n_words"], exp["n_words"])
    for k in ARRAYS if first else ARRAYS[:2]:
        helpers.assert_array_same(got[k], exp[k], (what, k))
    if not first:
        assert got["word_first"] is None, what


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def from_ids(tk, eng, ids, oo, data, offs, flags=1, checks=0):
    """tk_words_from_ids_device over host arrays (uploaded here)."""
    d_ids, d_oo = on_device(ids, oo)
    d_data, d_offs = dev(data, np.uint8), dev(offs, np.uint64)
    res = eng.words_from_ids_device(d_ids.data_ptr() if len(ids) else 0, d_oo.data_ptr(), len(oo) - 1, len(ids),
                                    d_data.data_ptr() if len(data) else 0, d_offs.data_ptr(), len(data), flags, checks, stream())
    return fetch(res)


def three_entries(tk, eng, data, offs, bos, eos, flags=1, checks=0):
    """The same batch through the three entries -> [(what, ids, id offsets, result dict)]."""
    out = []
    d_data, d_offs = dev(data, np.uint8), dev(offs, np.uint64)
    D = len(offs) - 1
    d_ids, d_oo, n, res = eng.encode_batch_device_words(d_data.data_ptr() if len(data) else 0, d_offs.data_ptr(), D, len(data), bos, eos, flags,
                                                        tk.CHECK_OFFSETS | checks, stream())
    ids = to_host(tk.DeviceView(d_ids, n, "<i4"), (n,), np.uint32).copy()
    oo = to_host(tk.DeviceView(d_oo, D + 1, "<i8"), (D + 1,), np.uint64).copy()
    out.append(("text on the device", ids, oo, fetch(res)))
    out.append(("ids on the device", ids, oo, from_ids(tk, eng, ids, oo, data, offs, flags, checks)))
    hids, hoo, w = eng.encode_batch_words(data, offs, bos, eos, False, flags, checks)
    out.append(("host", hids, hoo, w))
    return out


def with_specials(word_ids, per_doc_ids, bos, eos):
    """Restatement B is made without BOS / EOS: a None goes in front of / behind every document's ids."""
    parts, at = [], 0
    for n in per_doc_ids:
        parts += [[NONE]] * bool(bos) + [word_ids[at:at + n]] + [[NONE]] * bool(eos)
        at += n
    return np.concatenate([np.asarray(p, np.uint32) for p in parts]) if parts else np.zeros(0, np.uint32)


@pytest.fixture(scope="module")
def vocabs(test_vocab, bench_vocab):
    return {"test": test_vocab, "bench": bench_vocab}


@pytest.fixture(scope="module")
def eng(tk, test_vocab):
    e = tk.Engine(test_vocab["tokens"], test_vocab["num_special"], test_vocab["bos"], test_vocab["eos"], device=0)
    yield e
    e.close()


def expected_for(v, ids, oo, data, offs, pattern=0):
    return expected_words(ids, oo, v["tokens"], v["num_special"], data, offs, SPLITS[pattern])


# ---- 1. known answers through the Tekkenizer ----
def test_known_answers_small_vocab(tk, small_vocab):
    from test_host_tokenizer import model
    t = tk.Tekkenizer.from_json(json.dumps(model(small_vocab["tokens"])), device=0)
    orc = helpers.oracle_for(small_vocab)

    def a(text, bos, eos):
        raw = text.encode()
        ids = orc.encode(raw, bos, eos)
        w = expected_for(small_vocab, ids, [0, len(ids)], np.frombuffer(raw, np.uint8), [0, len(raw)])["word_ids"].tolist()
        return ids, [None if x == NONE else x for x in w]

    try:
        for bos, eos in ((False, False), (True, False), (False, True), (True, True)):
            assert t.encode_with_words("hello world", bos, eos) == a("hello world", bos, eos)
        # "hello" is a vocabulary key; " world" is one piece of six byte tokens
        assert a("hello world", True, True)[1] == [None, 0, 1, 1, 1, 1, 1, 1, None]
        # two words: "hé" (three byte tokens), and the emoji, whose four byte tokens share one word
        assert t.encode_with_words("hé\U0001f680") == a("hé\U0001f680", False, False)
        assert a("hé\U0001f680", False, False)[1] == [0, 0, 0, 1, 1, 1, 1]
        assert t.encode_with_words("", True, True) == ([1, 2], [None, None])
        # a batch of three documents (the one-launch small path), with word_first
        docs = ["hello world", "hé\U0001f680", ""]
        got = t.encode_batch_with_words(docs, True, True)
        data, offs = pack([d.encode() for d in docs])
        exp = expected_for(small_vocab, got["ids"], got["id_offsets"], data, offs)
        assert got["ids"].tolist() == sum((orc.encode(d.encode(), True, True) for d in docs), [])
        assert got["word_ids"].dtype == np.int32 and np.array_equal(got["word_ids"].view(np.uint32), exp["word_ids"])
        assert got["word_ids"].tolist() == [-1, 0, 1, 1, 1, 1, 1, 1, -1, -1, 0, 0, 0, 1, 1, 1, 1, -1, -1, -1]
        assert got["doc_words"].dtype == np.int64 and got["doc_words"].tolist() == [0, 2, 4, 4] and got["n_words"] == 4
        assert got["word_first"].tolist() == exp["word_first"].tolist() == [1, 2, 1, 4]
        pt = t.encode_batch_with_words(docs, True, True, return_tensors="pt")
        for k in ("ids", "id_offsets", "word_ids", "doc_words", "word_first"):
            assert np.array_equal(pt[k].cpu().numpy().astype(np.int64), np.asarray(got[k]).astype(np.int64)), k
        assert t.encode_batch_with_words(docs, return_word_first=False)["word_first"] is None
    finally:
        t.close()


# ---- 2. sweep parity ----
@pytest.mark.parametrize("vname", ["test", "bench"])
@pytest.mark.parametrize("pattern", [0, 1])
def test_sweep_parity(tk, vocabs, vname, pattern):
    """The three entries against restatement A (and B) on the spans sweep, and on the malformed documents behind it.

    On malformed UTF-8 the encode kernels and the oracle split differently (a continuation byte without a lead goes with its
    neighbours in the kernels' windows and is a character of its own in the oracle): with the bench vocabulary, which holds the
    token b"\x80z", encode gives that token for the end of b"\x80" * 130 + b"z", across the oracle's piece start at byte 130.
    The words pass follows the oracle there.  So: on the sweep itself the ids are the oracle's, A over them equals B, and
    TK_WORDS_CHECK_ALIGNED passes with n_words = the oracle's piece count; on the malformed documents the outputs equal A over
    the ids the entry returned (the definition is total), and the check says what its restatement says about those ids."""
    v = vocabs[vname]
    sweep = sweep_docs()
    docs = sweep + list(INVALID)
    S = len(sweep)
    data, offs = pack(docs)
    orc = helpers.oracle_for(v)
    orc.set_pattern(pattern)
    e = tk.Engine(v["tokens"], v["num_special"], v["bos"], v["eos"], device=0)
    try:
        e.set_pattern(pattern)
        b, pieces = words_by_piece(orc, docs, SPLITS[pattern], False, False)
        plain_oo = None
        for bos, eos in ((False, False), (True, False), (False, True), (True, True)):
            eids, eoo = orc.encode_batch(data, offs, bos, eos, threads=8)
            if plain_oo is None:
                plain_oo = eoo
            exp_o = expected_for(v, eids, eoo, data, offs, pattern)
            assert exp_o["per_doc"] == pieces
            assert np.array_equal(exp_o["word_ids"], with_specials(b, np.diff(plain_oo.astype(np.int64)).tolist(), bos, eos))
            n_sweep = int(eoo[S])
            for what, ids, oo, got in three_entries(tk, e, data, offs, bos, eos, 1, 0):
                assert np.array_equal(ids[:n_sweep], eids[:n_sweep]) and np.array_equal(oo[:S + 1], eoo[:S + 1]), what
                own = np.array_equal(ids, eids) and np.array_equal(oo, eoo)
                exp = exp_o if own else expected_for(v, ids, oo, data, offs, pattern)
                assert exp["per_doc"][:S] == pieces[:S]
                assert_words(got, exp, (what, bos, eos))
        # without TK_WORDS_FIRST the output is not there
        for what, ids, oo, got in three_entries(tk, e, data, offs, True, True, 0):
            assert_words(got, exp, what, first=False)
        full_ids, full_oo = ids, oo
        # TK_WORDS_CHECK_ALIGNED passes on encode's own output over the whole sweep
        sdata, soffs = pack(sweep)
        for what, ids, oo, got in three_entries(tk, e, sdata, soffs, True, True, 1, tk.WORDS_CHECK_ALIGNED):
            assert np.diff(got["doc_words"].astype(np.int64)).tolist() == pieces[:S], what
        # ... and on the malformed documents it says what its restatement says about the ids encode gave
        ids, oo = full_ids, full_oo
        bad = first_unaligned(ids, oo, v["tokens"], v["num_special"], data, offs, SPLITS[pattern])
        if bad is None:
            from_ids(tk, e, ids, oo, data, offs, 1, tk.WORDS_CHECK_ALIGNED)
        else:
            assert bad[0] >= S
            with pytest.raises(tk.TokenizerError) as err:
                from_ids(tk, e, ids, oo, data, offs, 1, tk.WORDS_CHECK_ALIGNED)
            assert err.value.code == tk.TK_ERR_RUNTIME and err.value.bad_doc == bad[0], (str(err.value), bad)
            if bad[1] is not None:
                assert "document %d " % bad[0] in str(err.value) and str(err.value).endswith("id index %d" % bad[1])
    finally:
        e.close()


# ---- 3. group and grid edges ----
TINY = [b"", b"a", b"hello world", b" x  y\n", "\U0001f680 é".encode(), b"the quick brown fox jumps", b"1234 5"]


def tiled_expectation(v, orc, which, bos, eos):
    """Restatement A, document by document: a document's words depend on nothing but its own ids and text, so the seven
    distinct documents are restated once and laid out in the order drawn."""
    per = []
    for doc in TINY:
        ids = orc.encode(doc, bos, eos)
        per.append((ids, expected_for(v, ids, [0, len(ids)], np.frombuffer(doc, np.uint8), [0, len(doc)])))
    n_ids = np.array([len(p[0]) for p in per], np.int64)[which]
    n_w = np.array([p[1]["n_words"] for p in per], np.int64)[which]

    def cat(key, dt):
        arrs = [np.asarray(p[1][key] if key else p[0], dt) for p in per]
        return np.concatenate([arrs[k] for k in which.tolist()] + [np.zeros(0, dt)])

    oo = np.concatenate([[0], np.cumsum(n_ids)]).astype(np.uint64)
    return cat(None, np.uint32), oo, {"word_ids": cat("word_ids", np.uint32), "doc_words": np.concatenate([[0], np.cumsum(n_w)]).astype(np.uint64),
                                      "word_first": cat("word_first", np.uint32), "n_words": int(n_w.sum())}


def test_more_groups_than_waves(tk, eng, test_vocab):
    """150 001 tiny documents: 9 376 groups for at most 8 192 waves (the grid-stride loop runs), a last group of one document,
    several document starts -- empty documents among them -- inside one 64-id step."""
    orc = helpers.oracle_for(test_vocab)
    which = np.random.default_rng(5).integers(0, len(TINY), 150001)
    data, offs = pack([TINY[k] for k in which.tolist()])
    eids, eoo, exp = tiled_expectation(test_vocab, orc, which, True, False)
    d_data, d_offs = dev(data, np.uint8), dev(offs, np.uint64)
    d_ids, d_oo, n, res = eng.encode_batch_device_words(d_data.data_ptr(), d_offs.data_ptr(), len(which), len(data), True, False, tk.WORDS_FIRST,
                                                        tk.WORDS_CHECK_ALIGNED, stream())
    assert n == len(eids) and np.array_equal(to_host(tk.DeviceView(d_ids, n, "<i4"), (n,), np.uint32), eids)
    assert_words(fetch(res), exp, "150 001 documents")


@pytest.mark.parametrize("n_docs", [1, 15, 16, 17])
def test_batches_around_one_group(tk, eng, test_vocab, n_docs):
    orc = helpers.oracle_for(test_vocab)
    which = np.random.default_rng(n_docs).integers(0, len(TINY), n_docs)
    which[-1] = 0                                         # (the batch ends with an empty document)
    data, offs = pack([TINY[k] for k in which.tolist()])
    for bos, eos in ((False, False), (True, True)):
        eids, eoo, exp = tiled_expectation(test_vocab, orc, which, bos, eos)
        for what, ids, oo, got in three_entries(tk, eng, data, offs, bos, eos):
            assert np.array_equal(ids, eids) and np.array_equal(oo, eoo), what
            assert_words(got, exp, (what, n_docs, bos, eos))


# ---- 4. ids that are not the text's own ----
def test_foreign_ids(tk, eng, test_vocab):
    v = test_vocab
    ns = v["num_special"]
    orc = helpers.oracle_for(v)
    docs = [b"the first document stays as it is", b"a second one, somewhat longer than the third", b"short third", b"", b"x y z " * 40,
            "café \U0001f680 naïve".encode(), b"tail"]
    enc = [orc.encode(d) for d in docs]
    rows = [enc[0],
            enc[2],                                       # another document's ids: shorter text than the document
            enc[1],                                       # ... and longer
            enc[4][:7],                                   # ids for an empty document
            enc[4][:50] + [1, 0, 2] + enc[4][50:],        # specials in mid-document (the text still fits)
            enc[6] + enc[5],                              # starts off the flags, ends beyond the document
            [2, 1]]                                       # specials only over a document with text
    data, offs = pack(docs)
    ids = np.array(sum(rows, []), np.uint32)
    oo = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    exp = expected_for(v, ids, oo, data, offs)
    assert exp["per_doc"][3] == 0 and exp["per_doc"][4] == len(tk_oracle.split(docs[4])) and exp["per_doc"][6] == 0
    assert_words(from_ids(tk, eng, ids, oo, data, offs), exp, "foreign ids")
    bad = first_unaligned(ids, oo, v["tokens"], ns, data, offs, tk_oracle.split)
    assert bad is not None and bad[0] == 1
    with pytest.raises(tk.TokenizerError) as e:
        from_ids(tk, eng, ids, oo, data, offs, checks=tk.WORDS_CHECK_ALIGNED)
    assert e.value.code == tk.TK_ERR_RUNTIME and e.value.bad_doc == 1 and "document 1 " in str(e.value)
    # the specials in mid-document alone leave the document aligned
    one = np.array(rows[4], np.uint32)
    d4, o4 = pack([docs[4]])
    exp4 = expected_for(v, one, [0, len(one)], d4, o4)
    assert_words(from_ids(tk, eng, one, np.array([0, len(one)], np.uint64), d4, o4, checks=tk.WORDS_CHECK_ALIGNED), exp4, "specials in mid-document")
    # an id outside the vocabulary, as in the spans pass
    wild = ids.copy()
    wild[len(rows[0]) + 2] = ns + len(v["tokens"])
    with pytest.raises(tk.TokenizerError) as e:
        from_ids(tk, eng, wild, oo, data, offs)
    assert e.value.code == tk.TK_ERR_RUNTIME and e.value.bad_doc == 1 and "outside the vocabulary" in str(e.value)


def test_foreign_ids_over_table_edges(tk):
    """The caller's ids over helpers.table_edge_vocab(33001): tokens of 255 bytes and more (a length byte of 0xFF: the length comes
    from the offsets) and ranks on both sides of the LDS part of the length table, the text their concatenation (so a token of
    " quick brown fox ..." holds many piece starts) and, for one document, another document's text."""
    v = helpers.table_edge_vocab(33001)
    ns, toks = v["num_special"], v["tokens"]
    a, z = ns + 0x61, ns + 0x20
    longs = [ns + v["edge"][(n, f)] for n in (16, 17, 254, 255, 256, 300) for f in ("ascii", "mb")]
    longs += [ns + v["long"]] + [ns + r for r in sorted(v["hand"])] + [ns + r for r in sorted(v["high"])]
    rows = [[t] for t in longs] + [[a, z, t, 1, z, t, a] for t in longs] + [longs, longs[::-1], [], [3, 7]]
    rows += [[ns + r for r in range(32760, 32776)], [ns + 32767, z, ns + 32768, z, ns + 32769] * 3]
    docs = [b"".join(toks[i - ns] for i in r if i >= ns) for r in rows]
    docs[len(longs)], docs[len(longs) + 1] = docs[len(longs) + 1], docs[len(longs)]          # two documents under each other's ids
    data, offs = pack(docs)
    ids = np.array(sum(rows, []), np.uint32)
    oo = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    exp = expected_for(v, ids, oo, data, offs)
    assert exp["n_words"] > 100 and max(exp["per_doc"]) >= 10    # (a word counts where a TOKEN begins on a piece start)
    e = tk.Engine(toks, ns, v["bos"], v["eos"], device=0)
    try:
        assert_words(from_ids(tk, e, ids, oo, data, offs), exp, "table edges")
        bad = first_unaligned(ids, oo, toks, ns, data, offs, tk_oracle.split)
        assert bad is not None and bad[0] == 0                     # (a piece starts inside the first long token)
        with pytest.raises(tk.TokenizerError) as err:
            from_ids(tk, e, ids, oo, data, offs, checks=tk.WORDS_CHECK_ALIGNED)
        assert err.value.code == tk.TK_ERR_RUNTIME and err.value.bad_doc == 0
    finally:
        e.close()


# ---- 5. TK_WORDS_CHECK_ALIGNED ----
def test_check_aligned_names_the_crossing_token(tk):
    """(That the check passes on encode's own output, with n_words = the oracle's piece count, is part of test_sweep_parity.)"""
    tokens = [bytes([b]) for b in range(256)] + [b"b c"]
    ns = 3
    e = tk.Engine(tokens, ns, 1, 2, device=0)
    try:
        doc = b"ab cd"
        assert tk_oracle.split(doc) == [0, 2]
        ids = np.array([ns + 0x61, ns + 256, ns + 0x64], np.uint32)
        oo = np.array([0, 3], np.uint64)
        data, offs = pack([doc])
        exp = expected_words(ids, oo, tokens, ns, data, offs, tk_oracle.split)
        assert exp["word_ids"].tolist() == [0, 0, 0] and exp["n_words"] == 1
        assert_words(from_ids(tk, e, ids, oo, data, offs), exp, "crossing token, unchecked")
        assert first_unaligned(ids, oo, tokens, ns, data, offs, tk_oracle.split) == (0, 1)
        with pytest.raises(tk.TokenizerError) as err:
            from_ids(tk, e, ids, oo, data, offs, checks=tk.WORDS_CHECK_ALIGNED)
        assert err.value.code == tk.TK_ERR_RUNTIME and err.value.bad_doc == 0 and "id index 1" in str(err.value)
        # behind two aligned documents the index stays relative to the document; a token of more than 16 bytes takes the byte loop
        long_tok = b"q" * 9 + b" " + b"q" * 9
        tokens2 = tokens + [long_tok]
        e2 = tk.Engine(tokens2, ns, 1, 2, device=0)
        try:
            docs = [b"a", b"", b"z" + long_tok]
            data, offs = pack(docs)
            ids = np.array([ns + 0x61, ns + 0x7a, ns + 257], np.uint32)
            oo = np.array([0, 1, 1, 3], np.uint64)
            assert first_unaligned(ids, oo, tokens2, ns, data, offs, tk_oracle.split) == (2, 1)
            with pytest.raises(tk.TokenizerError) as err:
                from_ids(tk, e2, ids, oo, data, offs, checks=tk.WORDS_CHECK_ALIGNED)
            assert err.value.bad_doc == 2 and "document 2 " in str(err.value) and "id index 1" in str(err.value)
        finally:
            e2.close()
    finally:
        e.close()


# ---- 6. buffers of its own ----
def test_buffers_of_its_own(tk, eng, test_vocab):
    docs = sweep_docs()[:80]
    data, offs = pack(docs)
    d_data, d_offs = dev(data, np.uint8), dev(offs, np.uint64)
    D = len(docs)
    d_ids, d_oo, d_sp, n = eng.encode_batch_device_spans(d_data.data_ptr(), d_offs.data_ptr(), D, len(data), True, True, 0, stream())
    snap = lambda: (to_host(tk.DeviceView(d_ids, n, "<i4"), (n,), np.uint32).copy(), to_host(tk.DeviceView(d_oo, D + 1, "<i8"), (D + 1,), np.uint64).copy(),
                    to_host(tk.DeviceView(d_sp, 2 * n, "<i4"), (2 * n,), np.uint32).copy())
    before = snap()
    res = eng.words_from_ids_device(d_ids, d_oo, D, n, d_data.data_ptr(), d_offs.data_ptr(), len(data), tk.WORDS_FIRST, 0, stream())
    after = snap()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    exp = expected_for(test_vocab, before[0], before[1], data, offs)
    first = fetch(res)
    assert_words(first, exp, "behind encode + spans")
    # a later encode and spans call (other documents) leaves the words result where it is
    other, ooffs = pack(sweep_docs()[100:160])
    d_other, d_ooffs = dev(other, np.uint8), dev(ooffs, np.uint64)
    eng.encode_batch_device_spans(d_other.data_ptr(), d_ooffs.data_ptr(), len(ooffs) - 1, len(other), False, False, tk.SPANS_CHECK_BYTES, stream())
    assert_words(fetch(res), first, "after a later encode + spans")


# ---- 7. arguments ----
def test_arguments_and_their_order(tk, eng, test_vocab):
    L = tk.lib()
    docs = [b"hello world", b"second"]
    data, offs = pack(docs)
    d_data, d_offs = dev(data, np.uint8), dev(offs, np.uint64)
    d_ids, d_oo, n = eng.encode_batch_device(d_data.data_ptr(), d_offs.data_ptr(), 2, len(data), False, False, stream())
    vp, st, bad = ctypes.c_void_p, tk._Words(), ctypes.c_uint64(0)
    good, wild = tk._WordsOpts(tk.WORDS_FIRST), tk._WordsOpts(2)

    def from_ids_rc(ids=d_ids, oo=d_oo, text=d_data.data_ptr(), toffs=d_offs.data_ptr(), checks=0, o=good, out=st):
        return L.tk_words_from_ids_device(eng._h, vp(ids), vp(oo), 2, n, vp(text), vp(toffs), len(data), checks, ctypes.byref(o) if o else None,
                                          vp(stream()), ctypes.byref(out) if out is not None else None, ctypes.byref(bad))

    def err():
        return L.tk_last_error(eng._h).decode()

    assert from_ids_rc() == tk.TK_OK and st.n_words == 3
    # an unknown flag or check bit first -- also beside a null argument --, then the null arguments
    for kw in (dict(o=wild), dict(checks=tk.SPANS_CHECK_BYTES), dict(checks=tk.CHECK_OFFSETS), dict(o=wild, ids=None), dict(checks=64, out=None)):
        assert from_ids_rc(**kw) == tk.TK_ERR_INVALID_ARG and err() == "unknown flag", kw
    for kw in (dict(ids=None), dict(oo=None), dict(text=None), dict(toffs=None), dict(o=None), dict(out=None)):
        assert from_ids_rc(**kw) == tk.TK_ERR_INVALID_ARG and err() == "null argument", kw

    # text on the device: unknown bits, null arguments, then encode (its offsets check), then the pass (an unaligned id is not
    # possible here: the pass is reached, and succeeds)
    ids_p, oo_p, n_p = vp(), vp(), ctypes.c_uint64(0)

    def device_rc(checks=0, o=good, out=st, toffs=d_offs.data_ptr(), n_bytes=len(data)):
        return L.tk_encode_batch_device_words(eng._h, vp(d_data.data_ptr()), vp(toffs), 2, n_bytes, 0, 0, checks, ctypes.byref(o) if o else None,
                                              vp(stream()), ctypes.byref(ids_p), ctypes.byref(oo_p), ctypes.byref(n_p),
                                              ctypes.byref(out) if out is not None else None, ctypes.byref(bad))

    assert device_rc(checks=tk.SPANS_CHECK_COVER, o=None) == tk.TK_ERR_INVALID_ARG and err() == "unknown flag"
    assert device_rc(o=wild, out=None) == tk.TK_ERR_INVALID_ARG and err() == "unknown flag"
    assert device_rc(o=None) == tk.TK_ERR_INVALID_ARG and err() == "null argument"
    assert device_rc(out=None, checks=tk.CHECK_OFFSETS, n_bytes=len(data) + 1) == tk.TK_ERR_INVALID_ARG and err() == "null argument"
    assert device_rc(checks=tk.CHECK_OFFSETS | tk.WORDS_CHECK_ALIGNED, n_bytes=len(data) + 1) == tk.TK_ERR_INVALID_ARG and "doc_offsets" in err()
    assert device_rc(toffs=None) == tk.TK_ERR_INVALID_ARG and err() == "null argument"
    assert device_rc(checks=tk.CHECK_OFFSETS | tk.CHECK_UTF8 | tk.WORDS_CHECK_ALIGNED) == tk.TK_OK and st.n_words == 3 and n_p.value == n

    # host: the same order
    res = tk._Result()
    u8, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)

    def host_rc(checks=0, o=good, out=st, text=data, result=res):
        return L.tk_encode_batch_words(eng._h, text.ctypes.data_as(u8) if text is not None else None, offs.ctypes.data_as(u64), 2, 0, 0, 1, checks,
                                       ctypes.byref(o) if o else None, ctypes.byref(result) if result is not None else None,
                                       ctypes.byref(out) if out is not None else None, ctypes.byref(bad))

    assert host_rc(checks=tk.CHECK_UTF8, text=None) == tk.TK_ERR_INVALID_ARG and err() == "unknown flag"
    assert host_rc(o=wild, out=None) == tk.TK_ERR_INVALID_ARG and err() == "unknown flag"
    for kw in (dict(o=None), dict(out=None), dict(text=None), dict(result=None)):
        assert host_rc(**kw) == tk.TK_ERR_INVALID_ARG and err() == "null argument", kw
    broken = data.copy()
    broken[3] = 0xFF
    assert host_rc(text=broken) == tk.TK_ERR_INVALID_UTF8 and not st.word_ids and not res.ids
    assert host_rc(checks=tk.WORDS_CHECK_ALIGNED) == tk.TK_OK and st.n_words == 3 and st.n_ids == n and st.word_first
    L.tk_free_words(ctypes.byref(st))
    L.tk_free_result(ctypes.byref(res))
    assert not st.word_ids and st.n_words == 0
    L.tk_free_words(ctypes.byref(st))                    # (a freed struct, and NULL, are fine)
    L.tk_free_words(None)


def test_empty_batches(tk, eng, test_vocab):
    z8, z32, o1 = np.zeros(0, np.uint8), np.zeros(0, np.uint32), np.zeros(1, np.uint64)
    # no document
    got = from_ids(tk, eng, z32, o1, z8, o1)
    assert got["n_words"] == 0 and got["doc_words"].tolist() == [0] and len(got["word_ids"]) == 0 and len(got["word_first"]) == 0
    ids, oo, w = eng.encode_batch_words(z8, o1, True, True, False, tk.WORDS_FIRST, tk.WORDS_CHECK_ALIGNED)
    assert len(ids) == 0 and w["n_words"] == 0 and w["doc_words"].tolist() == [0] and len(w["word_first"]) == 0
    # documents without ids: empty text without BOS / EOS, and text whose ids the caller left out
    for docs in ([b"", b"", b""], [b"some text", b"", b"more"]):
        data, offs = pack(docs)
        got = from_ids(tk, eng, z32, np.zeros(4, np.uint64), data, offs)
        assert got["n_words"] == 0 and got["doc_words"].tolist() == [0, 0, 0, 0] and len(got["word_ids"]) == 0
    for what, ids, oo, got in three_entries(tk, eng, *pack([b"", b"", b""]), False, False, 1, tk.WORDS_CHECK_ALIGNED):
        assert len(ids) == 0 and got["n_words"] == 0 and got["doc_words"].tolist() == [0, 0, 0, 0], what
    for what, ids, oo, got in three_entries(tk, eng, *pack([b"", b""]), True, True):
        assert ids.tolist() == [1, 2, 1, 2] and got["word_ids"].tolist() == [NONE] * 4 and got["doc_words"].tolist() == [0, 0, 0], what
    assert len(eng.last_words_ms()) == 4


# ---- 8. encode_batch_padded_words ----
def test_padded_words(tk, small_vocab):
    import torch
    from test_host_tokenizer import model
    t = tk.Tekkenizer.from_json(json.dumps(model(small_vocab["tokens"])), device=0)
    docs = ["hello world", "", "hé\U0001f680 and a longer row of words, to be cut", "a", "hello hello hello", "x " * 30]
    try:
        for bos, eos in ((True, True), (False, False)):
            base = t.encode_batch_with_words(docs, bos, eos)
            for max_length, padding, mult in ((None, "longest", None), (8, "longest", None), (8, "max_length", None), (100, "max_length", None),
                                              (None, "longest", 16), (7, "longest", 4), (6, "max_length", 4)):
                for tside, pside, dtype in (("right", "right", "int64"), ("left", "left", "int32"), ("left", "right", "int64"), ("right", "left", "int32")):
                    kw = dict(add_bos=bos, add_eos=eos, max_length=max_length, padding=padding, truncation_side=tside, padding_side=pside,
                              pad_id=7, dtype=dtype)
                    exp = expected_padded_words(base["ids"], base["id_offsets"], base["word_ids"].view(np.uint32), multiple_of=mult or 0, **kw)
                    got = t.encode_batch_padded_words(docs, pad_to_multiple_of=mult, **kw)
                    ref = t.encode_batch_padded(docs, pad_to_multiple_of=mult, **kw)
                    what = (bos, eos, max_length, padding, mult, tside, pside, dtype)
                    want_dt = torch.int64 if dtype == "int64" else torch.int32
                    assert got["word_ids"].dtype == got["input_ids"].dtype == want_dt and got["word_ids"].is_cuda, what
                    for k in ("input_ids", "word_ids", "attention_mask", "lengths"):
                        helpers.assert_array_same(got[k].cpu().numpy(), exp[k], (what, k))
                        if k != "word_ids":
                            assert torch.equal(got[k], ref[k]), (what, k)
                    assert got["n_truncated"] == exp["n_truncated"] == ref["n_truncated"], what
        got = t.encode_batch_padded_words(docs, True, True, max_length=8, pad_id=7, return_tensors="np")
        base = t.encode_batch_with_words(docs, True, True)
        exp = expected_padded_words(base["ids"], base["id_offsets"], base["word_ids"].view(np.uint32), True, True, 8, "longest", "right", "right", 0, 7,
                                    "int64")
        assert isinstance(got["word_ids"], np.ndarray) and np.array_equal(got["word_ids"], exp["word_ids"]) and np.array_equal(got["input_ids"], exp["input_ids"])
        with pytest.raises(tk.TokenizerError):
            t.encode_batch_padded_words(docs, padding="shortest")
    finally:
        t.close()


# ---- 9. the JSON pattern through the tokenizer ----
def test_honour_pattern_through_the_tokenizer(tk, test_vocab):
    import synth_vocab as sv
    from test_host_tokenizer import model
    v = test_vocab
    m = model(v["tokens"], num_special=v["num_special"], specials=("<unk>", "<s>", "</s>"))
    m["config"]["pattern"] = sv.MISTRAL_PATTERN
    docs = [b"HelloWorld XMLHttpRequest iPhone 1234 a/b/c\n", b"", b"it's 2024-01-02: DON'T   panic\r\n\r\n  ok", "CaféLatte \U0001f680\U0001f680 x".encode()] \
        + helpers.random_unicode_docs(60, seed=3)
    data, offs = pack(docs)
    t = tk.Tekkenizer.from_json(json.dumps(m), device=0)
    try:
        plain = t.encode_batch_with_words(docs, True, True, checks=tk.WORDS_CHECK_ALIGNED)
        assert_words({"word_ids": plain["word_ids"].view(np.uint32), "doc_words": plain["doc_words"].astype(np.uint64),
                      "word_first": plain["word_first"], "n_words": plain["n_words"]},
                     expected_for(v, plain["ids"], plain["id_offsets"], data, offs, 0), "pattern ignored")
        t.set_honour_pattern(True)
        got = t.encode_batch_with_words(docs, True, True, checks=tk.WORDS_CHECK_ALIGNED)
        orc = helpers.oracle_for(v)
        orc.set_pattern(1)
        eids, eoo = orc.encode_batch(data, offs, True, True)
        assert np.array_equal(got["ids"], eids) and np.array_equal(got["id_offsets"], eoo.astype(np.int64))
        exp = expected_for(v, eids, eoo, data, offs, 1)
        assert np.array_equal(got["word_ids"].view(np.uint32), exp["word_ids"]) and np.array_equal(got["doc_words"], exp["doc_words"].astype(np.int64))
        assert np.array_equal(got["word_first"], exp["word_first"]) and got["n_words"] == exp["n_words"]
        assert exp["per_doc"] == [len(tk_oracle.split_tekken(d)) if d else 0 for d in docs]
        assert exp["per_doc"][0] != len(tk_oracle.split(docs[0]))      # (the two patterns do differ on these documents)
    finally:
        t.close()
