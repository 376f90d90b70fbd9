"""Spans in code points / UTF-16 units and the annotation -> token range look-up on the GPU (include/tekken_hip.h
tk_token_spans_units_device, tk_spans_locate_device and the entries around them, csrc/tk_spans_units.hip) against the
restatements of tests/test_spans_units_cpu.py.  Everything is integer: every comparison is exact."""
import json

import numpy as np
import pytest

import helpers
from helpers import dev, on_device, to_host
from test_gpu_spans import pack, sweep_docs
from test_spans_units_cpu import BYTE, CHAR, UTF16, locate_brute, unit_spans_bytewise, unit_spans_str
from test_window_cpu import FIXED, I64, MASK, SPANS, expected_windows

pytestmark = pytest.mark.gpu

UNITS = (BYTE, CHAR, UTF16)
INVALID = [b"\x80", b"\xf0", b"a\xc3", b"\xe4\xb8", b"\x98\x80 tail", b"\xff\xfe\xfd", b"ab\x80cd", b"\xf0\x9f" * 40, b"\x80" * 130 + b"z",
           "中".encode()[:2] * 3 + b" x " + "\U0001f680".encode()[1:], b"\xc3" * 70, b"q\xf0\x9f\x9a"]


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def fetch_spans(tk, ptr, n):
    if n == 0:
        return np.zeros((0, 2), np.uint32)
    return to_host(tk.DeviceView(ptr, 2 * n, "<i4"), (n, 2), np.uint32)


def units_from_ids(tk, eng, ids, oo, unit):
    d_ids, d_oo = on_device(ids, oo)
    p = eng.token_spans_units_device(d_ids.data_ptr(), d_oo.data_ptr(), len(oo) - 1, len(ids), unit, stream())
    return fetch_spans(tk, p, len(ids))


def assert_spans(got, exp, what=""):
    got, exp = np.asarray(got, np.int64), np.asarray(exp, np.int64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.nonzero(np.any(got != exp, axis=1))[0]
    assert len(bad) == 0, (what, "first differing id", int(bad[0]), got[bad[0]].tolist(), exp[bad[0]].tolist())


def engine_of(tk, v):
    return tk.Engine(v["tokens"], v["num_special"], v["bos"], v["eos"], device=0)


@pytest.fixture(scope="module")
def vocabs(test_vocab, bench_vocab):
    return {"test": test_vocab, "bench": bench_vocab}


@pytest.fixture(scope="module")
def eng_bench(tk, bench_vocab):
    e = engine_of(tk, bench_vocab)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_small(tk, small_vocab):
    e = engine_of(tk, small_vocab)
    yield e
    e.close()


@pytest.fixture(scope="module")
def sweep(tk, vocabs):
    """Per vocabulary, computed once and left unchanged: the sweep's documents (the valid ones first), their ids with BOS / EOS,
    and the byte-wise restatement in the three units."""
    valid = sweep_docs()
    docs = valid + INVALID
    data, offs = pack(docs)
    out = {}
    for name, v in vocabs.items():
        eng = engine_of(tk, v)
        try:
            ids, oo = eng.encode_batch(data, offs, True, True)
        finally:
            eng.close()
        ids, oo = ids.astype(np.uint32), oo.astype(np.int64)
        exp = {u: unit_spans_bytewise(ids, oo, v["tokens"], v["num_special"], u) for u in UNITS}
        out[name] = {"docs": docs, "n_valid": len(valid), "data": data, "offs": offs, "ids": ids, "oo": oo, "exp": exp}
    return out


def test_known_answers_small_vocab(tk, small_vocab):
    from test_host_tokenizer import model
    t = tk.Tekkenizer.from_json(json.dumps(model(small_vocab["tokens"])), device=0)
    try:
        # every character of "hé🚀" is byte tokens: 1 + 2 + 4 ids
        text = "hé\U0001f680"
        ids, spans = t.encode_with_offsets(text, offsets_unit="char")
        assert ids == [10 + b for b in text.encode()]
        assert spans == [(0, 1), (1, 2), (1, 2), (2, 3), (2, 3), (2, 3), (2, 3)]
        assert t.encode_with_offsets(text, offsets_unit="utf16")[1] == [(0, 1), (1, 2), (1, 2), (2, 4), (2, 4), (2, 4), (2, 4)]
        assert t.encode_with_offsets(text, offsets_unit="byte") == t.encode_with_offsets(text)
        assert t.encode_with_offsets(text)[1] == [(k, k + 1) for k in range(7)]
        ids, spans = t.encode_with_offsets(text, True, True, offsets_unit="char")
        assert ids[0] == 1 and ids[-1] == 2 and spans[0] == (0, 0) and spans[-1] == (3, 3) and spans[1:-1] == [(0, 1), (1, 2), (1, 2)] + [(2, 3)] * 4
        assert t.encode_with_offsets(text, True, True, offsets_unit="utf16")[1][-1] == (4, 4)
        # ASCII: characters are bytes; "hello" is a vocabulary key
        for unit in ("byte", "char", "utf16"):
            assert t.encode_with_offsets("hello world", True, True, offsets_unit=unit) == t.encode_with_offsets("hello world", True, True)
        got = t.encode_batch_with_offsets(["hello world", text, ""], True, True, offsets_unit="char")
        assert got[0] == t.encode_with_offsets("hello world", True, True)
        assert got[1] == (ids, spans) and got[2] == ([1, 2], [(0, 0), (0, 0)])
        assert t.encode_batch_with_offsets([text], offsets_unit="byte") == t.encode_batch_with_offsets([text])
        for call in (lambda: t.encode_with_offsets(text, offsets_unit="chars"),
                     lambda: t.encode_batch_with_offsets([text], checks=tk.SPANS_CHECK_BYTES, offsets_unit="char")):
            with pytest.raises(tk.TokenizerError) as e:
                call()
            assert e.value.code == tk.TK_ERR_INVALID_ARG
        # the alignment entry: "hé🚀" as a str -- char_to_token(2) is the four ids of the emoji
        r = t.encode_batch_with_alignment([text, "", "hello world"], [[(2, 3), (0, 2), (1, 1)], [], [(0, 5), (6, 11), (20, 30)]], add_bos=True)
        assert r["ids"].dtype == np.int32 and r["id_offsets"].tolist() == [0, 8, 9, 17] and r["ann_offsets"].tolist() == [0, 3, 3, 6]
        assert r["token_ranges"].tolist() == [[4, 8], [1, 4], [2, 2], [1, 2], [3, 8], [8, 8]]
        assert r["offset_mapping"][:8].tolist() == [[0, 0], [0, 1], [1, 2], [1, 2]] + [[2, 3]] * 4
        r16 = t.encode_batch_with_alignment([text], [[(2, 4)]], offsets_unit="utf16", return_tensors="pt")
        assert r16["token_ranges"].is_cuda and r16["token_ranges"].tolist() == [[3, 7]]
        with pytest.raises(tk.TokenizerError) as e:
            t.encode_batch_with_alignment([text], [[(3, 2)]])
        assert e.value.code == tk.TK_ERR_INVALID_ARG and e.value.bad_ann == 0
    finally:
        t.close()


@pytest.mark.parametrize("vname", ["test", "bench"])
def test_sweep(tk, vocabs, sweep, vname):
    v, s = vocabs[vname], sweep[vname]
    ids, oo, n_docs = s["ids"], s["oo"], len(s["docs"])
    ns = v["num_special"]
    # the str restatement on the valid documents
    nv = int(oo[s["n_valid"]])
    for u in UNITS:
        assert_spans(s["exp"][u][:nv], unit_spans_str(ids[:nv], oo[:s["n_valid"] + 1], v["tokens"], ns, u), ("restatements", u))
        e = s["exp"][u]
        same = np.repeat(np.arange(n_docs), np.diff(oo))
        same = same[1:] == same[:-1]
        assert np.all(e[1:][same] >= e[:-1][same])               # starts and ends are non-decreasing along a document
    eng = engine_of(tk, v)
    try:
        for u in UNITS:
            gids, goo, sp = eng.encode_batch_spans_units(s["data"], s["offs"], True, True, unit=u)     # host in, host out
            assert np.array_equal(gids, ids) and np.array_equal(goo.astype(np.int64), oo)
            assert sp.dtype == np.uint32
            assert_spans(sp, s["exp"][u], (vname, "host entry", u))
        # device in, device out; TK_UNIT_BYTE equals tk_token_spans_device on the same ids
        d_bytes, d_offs = dev(s["data"], np.uint8), dev(s["offs"], np.uint64)
        for u in UNITS:
            p_ids, p_oo, p_sp, n = eng.encode_batch_device_spans_units(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, len(s["data"]), True, True,
                                                                       u, tk.CHECK_OFFSETS, stream())
            assert n == len(ids)
            assert_spans(fetch_spans(tk, p_sp, n), s["exp"][u], (vname, "device entry", u))
        p_b = eng.token_spans_device(p_ids, p_oo, n_docs, n, 0, 0, 0, stream())
        p_u = eng.token_spans_units_device(p_ids, p_oo, n_docs, n, tk.UNIT_BYTE, stream())
        assert p_b != p_u
        assert np.array_equal(fetch_spans(tk, p_b, n), fetch_spans(tk, p_u, n))
        # without BOS / EOS, and a batch small enough for the one-launch path
        for bos, eos in ((False, False), (True, False)):
            ids2, oo2 = eng.encode_batch(s["data"], s["offs"], bos, eos)
            for u in (CHAR, UTF16):
                _, _, sp = eng.encode_batch_spans_units(s["data"], s["offs"], bos, eos, unit=u)
                assert_spans(sp, unit_spans_bytewise(ids2, oo2.astype(np.int64), v["tokens"], ns, u), (vname, bos, eos, u))
        small = ["hé\U0001f680 中文".encode(), b"", b"plain words", "\U0001f680\U0001f680".encode()]
        sd, so = pack(small)
        calls0 = eng.small_path_calls()
        sids, soo, sp = eng.encode_batch_spans_units(sd, so, True, True, unit=CHAR)
        assert eng.small_path_calls() > calls0
        assert_spans(sp, unit_spans_str(sids, soo.astype(np.int64), v["tokens"], ns, CHAR), (vname, "small path"))
        # refusals: an unknown unit, a spans check bit, an id outside the vocabulary; the context works afterwards
        d_ids, d_oo = on_device(ids, oo)
        with pytest.raises(tk.TokenizerError) as e:
            eng.token_spans_units_device(d_ids.data_ptr(), d_oo.data_ptr(), n_docs, len(ids), 3, stream())
        assert e.value.code == tk.TK_ERR_INVALID_ARG
        with pytest.raises(tk.TokenizerError) as e:
            eng.encode_batch_device_spans_units(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, len(s["data"]), True, True, CHAR,
                                                tk.SPANS_CHECK_COVER, stream())
        assert e.value.code == tk.TK_ERR_INVALID_ARG
        bad = ids.copy()
        bad[len(bad) // 2] = ns + len(v["tokens"]) + 5
        with pytest.raises(tk.TokenizerError) as e:
            units_from_ids(tk, eng, bad, oo, CHAR)
        assert e.value.code == tk.TK_ERR_RUNTIME and "outside the vocabulary" in str(e.value)
        assert_spans(units_from_ids(tk, eng, ids, oo, UTF16), s["exp"][UTF16], "after the refusals")
    finally:
        eng.close()


def ragged(lists):
    ids = np.array([i for x in lists for i in x], np.uint32)
    oo = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return ids, oo


def test_step_and_group_edges(tk, eng_small, small_vocab):
    """The small vocabulary, where an emoji is four ids: a character straddles the 64-id step; the carry stops at a document, at
    the 16-document group, and goes through empty documents' absence of ids."""
    v = small_vocab
    rocket = "\U0001f680".encode()
    docs = [b"a" * k + rocket * 3 for k in range(58, 67)]
    docs += [b"", b""]
    for k in range(33):                                        # ... \xf0\x9f | \x98\x80 ...: the second kind starts at 0
        docs.append((b"x" * (k % 5) + b"\xf0\x9f") if k % 2 == 0 else (b"\x98\x80" + b"y" * (k % 3)))
        if k % 4 == 1:
            docs.append(b"")
    docs += [b"a" * 63 + b"\xf0", b"\x9f\x9a\x80" + b"b" * 70, b"\x80" * 200, b"", rocket * 40]
    assert any(d.startswith(b"\x98\x80") and k % 16 == 0 and docs[k - 1].endswith(b"\xf0\x9f") for k, d in enumerate(docs))
    by_bytes = [[10 + b for b in d] for d in docs]
    for lists in (by_bytes, [[1] + x + [2] for x in by_bytes]):
        ids, oo = ragged(lists)
        for u in UNITS:
            assert_spans(units_from_ids(tk, eng_small, ids, oo, u), unit_spans_bytewise(ids, oo, v["tokens"], v["num_special"], u), u)
    # what the encode entry itself gives for the same documents is the same definition over ITS ids
    data, offs = pack(docs)
    gids, goo, sp = eng_small.encode_batch_spans_units(data, offs, True, True, unit=CHAR)
    assert_spans(sp, unit_spans_bytewise(gids, goo.astype(np.int64), v["tokens"], v["num_special"], CHAR), "encode")
    # second kind of document: every span starts at 0 until its first character start
    ids, oo = ragged(by_bytes)
    got = units_from_ids(tk, eng_small, ids, oo, CHAR)
    for d, doc in enumerate(docs):
        if doc.startswith(b"\x98\x80"):
            assert got[int(oo[d])].tolist() == [0, 0] and got[int(oo[d]) + 1].tolist() == [0, 0]


def test_callers_ids(tk, eng_bench, bench_vocab):
    v = bench_vocab
    ns, toks = v["num_special"], v["tokens"]
    # ranks at or above 32768 (beyond the LDS part of the table) that hold non-ASCII bytes, tokens that begin or end inside a character
    high = [r for r in range(32768, len(toks)) if any(b >= 0x80 for b in toks[r])]
    assert len(high) >= 50
    cut = [r for r in range(len(toks)) if (toks[r][0] & 0xC0) == 0x80 or toks[r][-1] >= 0xC0][:200]
    rng = np.random.default_rng(3)
    lists = []
    pool = np.array(high[:2000] + cut + list(range(256)) + list(range(300, 800)))
    for d in range(40):
        n = int(rng.integers(0, 150))
        x = (pool[rng.integers(0, len(pool), n)] + ns).tolist()
        for _ in range(int(rng.integers(0, 4))):                # specials in mid-document
            if x:
                x.insert(int(rng.integers(0, len(x) + 1)), int(rng.integers(0, ns)))
        lists.append(x)
    lists += [[], [0], [5, 6, 7], [ns + high[0]] * 130]
    ids, oo = ragged(lists)
    for u in UNITS:
        assert_spans(units_from_ids(tk, eng_bench, ids, oo, u), unit_spans_bytewise(ids, oo, toks, ns, u), u)
    # a made-up vocabulary: tokens the one-byte fields of an entry cannot hold count their bytes from the token blob
    zh = "中".encode()
    extra = [(zh * 6)[:16], (zh * 85)[:254], zh * 85, zh * 100, b"a" * 254, b"a" * 255, b"a" * 300, "\U0001f680".encode() * 63,
             "\U0001f680".encode() * 64, (zh * 100)[1:], b"\x80" * 300]
    assert [len(x) for x in extra[:4]] == [16, 254, 255, 300]
    made = {"tokens": [bytes([b]) for b in range(256)] + extra, "num_special": 4, "bos": 1, "eos": 2}
    eng = engine_of(tk, made)
    try:
        rng = np.random.default_rng(4)
        lists = [(4 + 256 + rng.integers(0, len(extra), 30)).tolist(), [4 + 256 + k for k in range(len(extra))] * 3,
                 [4 + 0xe4, 4 + 256 + 9, 3, 4 + 256 + 10, 4 + 256 + 6], []]
        lists += [[4 + int(b) for b in rng.integers(0, 256, 90)] + [4 + 256 + int(rng.integers(0, len(extra)))] for _ in range(20)]
        ids, oo = ragged(lists)
        for u in (CHAR, UTF16, BYTE):                           # a units call is the FIRST call on this fresh engine
            assert_spans(units_from_ids(tk, eng, ids, oo, u), unit_spans_bytewise(ids, oo, made["tokens"], 4, u), ("made-up", u))
    finally:
        eng.close()


def test_windows_in_characters(tk, bench_vocab):
    t = tk.Tekkenizer.from_file(bench_vocab["path"], device=0)
    try:
        docs = [x.decode("utf-8") for x in sweep_docs()[40:75] if len(x) < 3000] + ["", "hé\U0001f680 中文" * 9]
        ns, toks = bench_vocab["num_special"], bench_vocab["tokens"]
        for bos, eos in ((True, True), (False, False)):
            lists = t.encode_batch(docs, bos, eos)
            ids, oo = ragged(lists)
            for unit, u in (("char", CHAR), ("utf16", UTF16)):
                spans = unit_spans_str(ids, oo, toks, ns, u)
                exp = expected_windows(ids, oo, 8, 3, int(bos), int(eos), 0, t.pad_id(), FIXED | I64 | MASK | SPANS, spans)
                assert exp["n_split"] > 0
                for rt in ("pt", "np"):
                    r = t.encode_batch_windows(docs, 8, 3, bos, eos, return_offsets_mapping=True, return_tensors=rt, offsets_unit=unit)
                    got = {k: (x.cpu().numpy() if rt == "pt" else x) for k, x in r.items() if k not in ("n_windows", "n_split")}
                    assert (r["n_windows"], r["n_split"]) == (exp["n_windows"], exp["n_split"])
                    assert np.array_equal(got["input_ids"], exp["input_ids"]) and np.array_equal(got["attention_mask"], exp["mask"])
                    assert got["offset_mapping"].dtype == np.int32
                    assert np.array_equal(got["offset_mapping"], exp["spans"].astype(np.int32)), (bos, eos, unit, rt)
                    assert np.array_equal(got["window_start"], exp["window_start"].astype(np.int32))
        # the default stays bytes, and without the mapping the unit changes nothing
        a = t.encode_batch_windows(docs, 8, 3, True, True, return_offsets_mapping=True, return_tensors="np")
        b = t.encode_batch_windows(docs, 8, 3, True, True, return_offsets_mapping=True, return_tensors="np", offsets_unit="byte")
        assert np.array_equal(a["offset_mapping"], b["offset_mapping"])
        c = t.encode_batch_windows(docs, 8, 3, True, True, return_tensors="np", offsets_unit="char")
        assert c["offset_mapping"] is None and np.array_equal(c["input_ids"], a["input_ids"])
        # "np" in characters goes through the device tensors: the same keys and dtypes as the byte branch's
        d = t.encode_batch_windows(docs, 8, 3, True, True, return_offsets_mapping=True, return_tensors="np", offsets_unit="char")
        assert set(d) == set(a)
        for k in a:
            assert type(d[k]) is type(a[k]) and (not isinstance(a[k], np.ndarray) or (d[k].dtype == a[k].dtype and d[k].shape[:1] == a[k].shape[:1])), k
    finally:
        t.close()


def locate(tk, eng, d_spans_ptr, d_oo, n_docs, n_ids, ann_doc, ann):
    A = len(ann_doc)
    d_doc, d_ann = dev(np.asarray(ann_doc, np.uint32), np.uint32), dev(np.asarray(ann, np.uint32).reshape(-1), np.uint32)
    p = eng.spans_locate_device(d_spans_ptr, d_oo.data_ptr(), n_docs, n_ids, d_doc.data_ptr(), d_ann.data_ptr(), A, stream())
    return p, (to_host(tk.DeviceView(p, 2 * A, "<i4"), (A, 2), np.uint32) if A else np.zeros((0, 2), np.uint32))


def test_locate(tk, vocabs, sweep, eng_small, small_vocab):
    # exhaustively: every (as, ae) of a few short documents, in the three units, byte tokens with BOS / EOS
    texts = ["hello w中é", "ab\U0001f680\U0001f680cd", "é\U0001f680中", "", "中"]
    lists = [[1] + [10 + b for b in x.encode()] + [2] for x in texts] + [[]]
    ids, oo = ragged(lists)
    d_ids, d_oo = on_device(ids, oo)
    for u in UNITS:
        p_sp = eng_small.token_spans_units_device(d_ids.data_ptr(), d_oo.data_ptr(), len(lists), len(ids), u, stream())
        sp = fetch_spans(tk, p_sp, len(ids)).astype(np.int64)
        assert_spans(sp, unit_spans_bytewise(ids, oo, small_vocab["tokens"], small_vocab["num_special"], u), u)
        ann_doc, ann = [], []
        for d in range(len(lists)):
            n = int(sp[int(oo[d]):int(oo[d + 1]), 1].max(initial=0)) + 1        # one beyond the text as well
            for a0 in range(n + 1):
                for a1 in range(a0, n + 1):
                    ann_doc.append(d)
                    ann.append((a0, a1))
        _, got = locate(tk, eng_small, p_sp, d_oo, len(lists), len(ids), ann_doc, ann)
        assert_spans(got, locate_brute(sp.tolist(), oo, ann_doc, ann), ("exhaustive", u))
    # random annotations over the sweep (bench vocabulary, characters), inside and beyond the documents
    v, s = vocabs["bench"], sweep["bench"]
    ids, oo, n_docs = s["ids"], s["oo"], len(s["docs"])
    eng = engine_of(tk, v)
    try:
        d_ids, d_oo = on_device(ids, oo)
        p_sp = eng.token_spans_units_device(d_ids.data_ptr(), d_oo.data_ptr(), n_docs, len(ids), CHAR, stream())
        sp = s["exp"][CHAR]
        rng = np.random.default_rng(8)
        ann_doc = np.sort(rng.integers(0, n_docs, 3000))
        ends = np.array([int(sp[int(oo[d]):int(oo[d + 1]), 1].max(initial=0)) for d in range(n_docs)])
        a0 = (rng.random(3000) * (ends[ann_doc] + 3)).astype(np.int64)
        a1 = a0 + (rng.integers(0, 12, 3000) * (rng.random(3000) < 0.8)).astype(np.int64)
        ann = np.stack([a0, a1], axis=1)
        p1, got = locate(tk, eng, p_sp, d_oo, n_docs, len(ids), ann_doc, ann)
        exp = locate_brute(sp.tolist(), oo, ann_doc.tolist(), ann.tolist())
        assert_spans(got, exp, "random")
        assert np.any(exp[:, 1] - exp[:, 0] > 1) and np.any(exp[:, 1] == exp[:, 0])
        # refusals: nothing is written, the earlier result stays readable, bad_ann names the first one
        for k, (bd, ba) in ((7, (n_docs, (0, 1))), (11, (3, (5, 4))), (0, (2 ** 32 - 1, (0, 0)))):
            doc2, ann2 = ann_doc.copy(), ann.copy()
            doc2[k], ann2[k] = bd, ba
            doc2[2000], ann2[2000] = n_docs + 9, (9, 1)               # a later bad one: the first is reported
            with pytest.raises(tk.TokenizerError) as e:
                locate(tk, eng, p_sp, d_oo, n_docs, len(ids), doc2, ann2)
            assert e.value.code == tk.TK_ERR_INVALID_ARG and e.value.bad_ann == k, str(e.value)
            assert np.array_equal(to_host(tk.DeviceView(p1, 2 * 3000, "<i4"), (3000, 2), np.uint32), got)
        # A == 0; and the result before it stays where it was
        p0, none = locate(tk, eng, p_sp, d_oo, n_docs, len(ids), [], [])
        assert none.shape == (0, 2)
        assert np.array_equal(to_host(tk.DeviceView(p1, 2 * 3000, "<i4"), (3000, 2), np.uint32), got)
        # no documents at all
        z = dev(np.zeros(1, np.uint64), np.uint64)
        locate(tk, eng, 0, z, 0, 0, [], [])
    finally:
        eng.close()


def test_buffers_stay_apart(tk, eng_bench, bench_vocab, sweep):
    """Byte spans, encode outputs and a window result are unchanged after a units call and a locate call."""
    s = sweep["bench"]
    n_docs = len(s["docs"])
    d_bytes, d_offs = dev(s["data"], np.uint8), dev(s["offs"], np.uint64)
    p_ids, p_oo, p_sp, n = eng_bench.encode_batch_device_spans(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, len(s["data"]), True, True,
                                                               tk.SPANS_CHECK_BYTES, stream())
    res = eng_bench.window_from_ids_device(p_ids, p_oo, n_docs, n, 16, 4, 0, 7, 1, 1, FIXED | SPANS, p_sp, stream())
    v = res.views()
    W, L = res.n_windows, res.row_len

    def snapshot():
        return [to_host(tk.DeviceView(p_ids, n, "<i4"), (n,), np.uint32).copy(), to_host(tk.DeviceView(p_oo, n_docs + 1, "<i8"), (n_docs + 1,), np.uint64).copy(),
                fetch_spans(tk, p_sp, n).copy(), to_host(v[0], (W, L), np.int32).copy(), to_host(v[6], (W, L, 2), np.uint32).copy()]

    before = snapshot()
    assert np.array_equal(before[0], s["ids"]) and np.array_equal(before[2].astype(np.int64), s["exp"][BYTE])
    p_u = eng_bench.token_spans_units_device(p_ids, p_oo, n_docs, n, tk.UNIT_UTF16, stream())
    ann_doc = np.arange(n_docs, dtype=np.uint32)
    ann = np.stack([np.zeros(n_docs, np.uint32), np.full(n_docs, 5, np.uint32)], axis=1)
    p_r, got = locate(tk, eng_bench, p_u, dev(s["oo"], np.uint64), n_docs, n, ann_doc, ann)
    assert len({p_ids, p_oo, p_sp, p_u, p_r}) == 5
    assert_spans(fetch_spans(tk, p_u, n), s["exp"][UTF16], "units")
    assert_spans(got, locate_brute(s["exp"][UTF16].tolist(), s["oo"], ann_doc.tolist(), ann.tolist()), "locate")
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a, b)


def test_many_short_documents_take_several_groups_per_wave(tk, eng_small, small_vocab):
    """More than 131 072 documents: the launch is capped at 512 blocks of 16 waves, so a wave takes a second group of 16 documents
    and starts it with fresh carries.  Documents of 0 to 3 byte tokens cut out of one text, so that characters are split across
    documents; exact against the restatement, and two successive calls agree, in both units."""
    v = small_vocab
    n_docs = 140_000
    rng = np.random.default_rng(21)
    lens = rng.integers(0, 4, n_docs)
    oo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    text = ("a\U0001f680é中b\U0001f680\U0001f680 z" * (int(oo[-1]) // 20 + 1)).encode()[:int(oo[-1])]
    ids = (np.frombuffer(text, np.uint8).astype(np.uint32) + 10)
    assert (n_docs + 15) // 16 > 512 * 16
    d_ids, d_oo = on_device(ids, oo)
    for u in (CHAR, UTF16, BYTE):
        exp = unit_spans_bytewise(ids, oo, v["tokens"], v["num_special"], u)
        runs = []
        for _ in range(2):
            p = eng_small.token_spans_units_device(d_ids.data_ptr(), d_oo.data_ptr(), n_docs, len(ids), u, stream())
            runs.append(fetch_spans(tk, p, len(ids)))
        assert_spans(runs[0], exp, ("first call", u))
        assert_spans(runs[1], runs[0], ("second call", u))


def unit_spans_byte_tokens(ids, oo, ns, unit):
    """The definition for ids that are specials or ONE-byte tokens (id - ns = the byte), with numpy over whole arrays: a token
    that is a character start begins at U of its own position, any other at U of the last start in front of it in its document
    (0 without one).  -> int64[n_ids, 2]."""
    ids, oo = np.asarray(ids, np.int64), np.asarray(oo, np.int64)
    body = ids >= ns
    b = np.where(body, ids - ns, 0)
    start = body & ((b & 0xC0) != 0x80)
    w = start.astype(np.int64) + ((unit == UTF16) & body & (b >= 0xF0)) if unit != BYTE else body.astype(np.int64)
    incl = np.cumsum(w)
    excl = incl - w
    doc = np.repeat(np.arange(len(oo) - 1), np.diff(oo))
    first = oo[:-1][doc]                                        # the first id of the id's document
    base = excl[np.minimum(oo[:-1], max(len(ids) - 1, 0))][doc] if len(ids) else excl
    idx = np.arange(len(ids))
    last = np.maximum.accumulate(np.where(start, idx, -1))      # the last start at or before the id
    lead = np.where(last >= first, excl[np.maximum(last, 0)], base)
    st = np.where(~body | start | (unit == BYTE), excl, lead) - base
    return np.stack([st, incl - base], axis=1)


def test_many_documents_of_many_steps(tk, eng_small, small_vocab):
    """The bench shape in small: more than 131 072 documents of about 100 ids (BOS / EOS included), so a group of 16 documents
    is about 25 steps of 64 ids and a wave takes a second group behind them: the multi-step carries AND the restart per group.
    Byte tokens of one mixed text cut at arbitrary bytes; exact against the definition, and a second call equals the first."""
    v = small_vocab
    ns = v["num_special"]
    n_docs = 135_000
    rng = np.random.default_rng(33)
    lens = rng.integers(60, 141, n_docs)
    lens[rng.integers(0, n_docs, 500)] = 0                      # a few documents without text
    total = int(lens.sum())
    unit_text = "the quick \U0001f680é中 brown\U0001f680\U0001f680 fox, 中文字符 jumps".encode()
    text = np.frombuffer((unit_text * (total // len(unit_text) + 1))[:total], np.uint8).astype(np.uint32) + ns
    oo = np.concatenate([[0], np.cumsum(lens + 2)]).astype(np.int64)
    ids = np.empty(int(oo[-1]), np.uint32)
    ids[oo[:-1]], ids[oo[1:] - 1] = 1, 2
    keep = np.ones(len(ids), bool)
    keep[oo[:-1]] = keep[oo[1:] - 1] = False
    ids[keep] = text
    assert (n_docs + 15) // 16 > 512 * 16 and len(ids) > 13_000_000
    # the whole-array restatement is the byte-wise one
    k = int(oo[3000])
    for u in UNITS:
        assert_spans(unit_spans_byte_tokens(ids[:k], oo[:3001], ns, u), unit_spans_bytewise(ids[:k], oo[:3001], v["tokens"], ns, u), ("restatements", u))
    d_ids, d_oo = on_device(ids, oo)
    for u in (CHAR, UTF16):
        exp = unit_spans_byte_tokens(ids, oo, ns, u)
        p = eng_small.token_spans_units_device(d_ids.data_ptr(), d_oo.data_ptr(), n_docs, len(ids), u, stream())
        first = fetch_spans(tk, p, len(ids)).copy()
        assert_spans(first, exp, ("first call", u))
        p = eng_small.token_spans_units_device(d_ids.data_ptr(), d_oo.data_ptr(), n_docs, len(ids), u, stream())
        assert np.array_equal(fetch_spans(tk, p, len(ids)), first), ("second call", u)
