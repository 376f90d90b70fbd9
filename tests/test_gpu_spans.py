"""Per-token byte spans on the GPU (include/tekken_hip.h tk_token_spans_device and the entries around it, csrc/tk_spans.hip)
against the numpy restatement of the definition in tests/test_spans_cpu.py -- per id, per document, never through a global sum."""
import json

import numpy as np
import pytest

import corpus
import helpers
import tk_oracle
from test_spans_cpu import expected_spans

pytestmark = pytest.mark.gpu


def tok_len_of(v):
    return np.array([len(t) for t in v["tokens"]], np.int64)


def pack(docs):
    offs = np.zeros(len(docs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(d) for d in docs])
    joined = b"".join(docs)
    return (np.frombuffer(joined, np.uint8).copy() if joined else np.zeros(0, np.uint8)), offs


def check_spans(v, data, offs, ids, oo, spans):
    """Every id: spans equal the restatement, the text under a span is the token's bytes, and the spans of every document tile it."""
    ns, tokens, tok_len = v["num_special"], v["tokens"], tok_len_of(v)
    ids = np.asarray(ids, np.int64)
    oo = np.asarray(oo, np.int64)
    offs = np.asarray(offs, np.int64)
    spans = np.asarray(spans, np.int64).reshape(len(ids), 2)
    exp = expected_spans(ids, oo, tok_len, ns).astype(np.int64)
    bad = np.nonzero(np.any(spans != exp, axis=1))[0]
    assert len(bad) == 0, ("first differing id", int(bad[0]), spans[bad[0]].tolist(), exp[bad[0]].tolist())
    doc_of = np.repeat(np.arange(len(oo) - 1), np.diff(oo))
    doc_len = np.diff(offs)
    # tiling: every document's first span starts at 0, each starts where the one before ends, the last ends at the length
    nonempty = np.diff(oo) > 0
    assert np.all(spans[oo[:-1][nonempty], 0] == 0)
    assert np.array_equal(spans[oo[1:][nonempty] - 1, 1], doc_len[nonempty])
    assert np.all(doc_len[~nonempty] == 0)
    same = doc_of[1:] == doc_of[:-1]
    assert np.array_equal(spans[1:, 0][same], spans[:-1, 1][same])
    # bytes: specials are empty, every other id covers exactly its token, and the text there is the token's bytes
    body = ids >= ns
    L = spans[:, 1] - spans[:, 0]
    assert np.all(L[~body] == 0)
    assert np.array_equal(L[body], tok_len[ids[body] - ns])
    gstart, lb = offs[doc_of[body]] + spans[body, 0], L[body]
    if lb.sum():
        pos = np.repeat(gstart - (np.cumsum(lb) - lb), lb) + np.arange(int(lb.sum()))
        want = np.frombuffer(b"".join(tokens[i - ns] for i in ids[body].tolist()), np.uint8)
        assert np.array_equal(data[pos], want)


def regression_docs():
    """The round-4 shapes: a CR / LF run behind a char the 2048-byte region start cuts (tests/test_gpu_parity.py has the story)."""
    rle = [(0x4e2d, 26), (0x663, 1), (0xe9, 28), (0x21, 3), (0x20, 13), (0x9, 17), (0x3000, 11), (0xd, 40), (0x9, 11), (0xd, 22),
           (0x27, 5), (0x663, 13), (0xff13, 32), (0x21, 13), (0x2d, 22), (0xd, 14), (0x4e2d, 16)]
    frag = "".join(chr(c) * n for c, n in rle).encode()
    at = frag.index(b"\r" * 40)
    docs = [(b"ab cd\n" * 800)[:2 * 1952 - 32 - at + 1 + shift] + frag for shift in range(-4, 4)]
    for ch in ("…", "　", "\U0001f680"):
        for k in range(1, len(ch.encode())):
            docs.append((b"xy z\n" * 800)[:1952 - 32 - k] + ch.encode() + b"\n" * 45 + b"\t\t next" + b" words" * 30)
    return docs


EDGE = [b"", b"a", b" ", b" \t \n  \t", b"\r\n" * 40 + b"\n\r\r\n" * 10 + b"x", ("中文字符" * 60).encode(),
        b"a" * 70000, b"q" * 65, b"x" * 200 + b" tail", b"ab" * 128, b" " * 100 + b"word", "\U0001f680".encode(),
        "é\U0001f680中".encode(), b"", b"\n"]


def sweep_docs():
    docs = []
    for kind, n, dl, sd in (("ascii", 150, 512, 1), ("mixed", 40, 2048, 2), ("zipf", 200, 0, 4)):
        d, o = corpus.generate(kind, n, dl, seed=corpus.BASE_SEED + sd)
        docs += [x for x in corpus.docs_of(d, o) if len(x) <= 20000]
    return docs[:60] + EDGE + docs[60:] + regression_docs() + [b""]


@pytest.fixture(scope="module")
def vocabs(test_vocab, bench_vocab):
    return {"test": test_vocab, "bench": bench_vocab}


def test_known_answer_small_vocab(tk, small_vocab):
    from test_host_tokenizer import model
    t = tk.Tekkenizer.from_json(json.dumps(model(small_vocab["tokens"])), device=0)
    orc = helpers.oracle_for(small_vocab)
    try:
        ids, spans = t.encode_with_offsets("hello world", True, True)
        # "hello" is a vocabulary key; " world" is one piece no merge can shorten: six byte tokens
        assert ids == orc.encode(b"hello world", True, True) == [1, 266, 42, 129, 121, 124, 118, 110, 2]
        assert spans == [(0, 0), (0, 5), (5, 6), (6, 7), (7, 8), (8, 9), (9, 10), (10, 11), (11, 11)]
        ids, spans = t.encode_with_offsets("\U0001f680")                  # byte fallback: four 1-byte spans inside one char
        assert ids == orc.encode("\U0001f680".encode()) and len(ids) == 4
        assert spans == [(0, 1), (1, 2), (2, 3), (3, 4)]
        # the kernel (through the tokenizer's engine context) gives the same
        got = t.encode_batch_with_offsets(["hello world", "\U0001f680", ""], True, True)
        assert got[0] == t.encode_with_offsets("hello world", True, True)
        assert got[1][1] == [(0, 0), (0, 1), (1, 2), (2, 3), (3, 4), (4, 4)]
        assert got[2] == ([1, 2], [(0, 0), (0, 0)])
    finally:
        t.close()


@pytest.mark.parametrize("vname", ["test", "bench"])
@pytest.mark.parametrize("mode", ["default", "json_pattern", "memo"])
def test_property_sweep(tk, vocabs, vname, mode):
    v = vocabs[vname]
    docs = sweep_docs()
    data, offs = pack(docs)
    orc = helpers.oracle_for(v)
    eng = tk.Engine(v["tokens"], v["num_special"], v["bos"], v["eos"], device=0)
    try:
        if mode == "json_pattern":
            orc.set_pattern(1)
            eng.set_pattern(1)
        if mode == "memo":
            eng.set_memo(24, 1)
        for bos, eos in ((False, False), (True, False), (False, True), (True, True)):
            eids, eoo = orc.encode_batch(data, offs, bos, eos, threads=8)
            for _ in range(2 if mode == "memo" else 1):          # memo: the second call reads what the first one filled in
                ids, oo, spans = eng.encode_batch_spans(data, offs, bos, eos, checks=tk.SPANS_CHECK_BYTES)
                assert np.array_equal(oo, eoo) and np.array_equal(ids, eids)
                assert spans.shape == (len(ids), 2) and spans.dtype == np.uint32
                check_spans(v, data, offs, ids, oo, spans)
        if mode == "memo":
            assert eng.memo_stats()["hits_total"] > 0
    finally:
        eng.close()


@pytest.fixture(scope="module")
def eng_bench(tk, bench_vocab):
    e = tk.Engine(bench_vocab["tokens"], bench_vocab["num_special"], bench_vocab["bos"], bench_vocab["eos"], device=0)
    yield e
    e.close()


def test_full_size_device_resident_with_bytes_check(tk, eng_bench, bench_vocab):
    """C2 (1 M x 512 B) through tk_encode_batch_device_spans with TK_SPANS_CHECK_BYTES; every document checked on the host."""
    import torch
    n_docs = 1_000_000
    data, offs = corpus.generate("ascii", n_docs, 512, seed=corpus.BASE_SEED + 1)
    d_bytes = torch.from_numpy(data).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    p_ids, p_oo, p_sp, n = eng_bench.encode_batch_device_spans(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, len(data), True, True,
                                                               checks=tk.CHECK_OFFSETS | tk.SPANS_CHECK_BYTES, stream=stream)
    ids = torch.as_tensor(tk.DeviceView(p_ids, n, "<i4"), device="cuda").cpu().numpy().view(np.uint32)
    oo = torch.as_tensor(tk.DeviceView(p_oo, n_docs + 1, "<i8"), device="cuda").cpu().numpy().astype(np.int64)
    spans = torch.as_tensor(tk.DeviceView(p_sp, 2 * n, "<i4"), device="cuda").cpu().numpy().view(np.uint32).reshape(n, 2)
    assert int(oo[-1]) == n
    ns = bench_vocab["num_special"]
    exp = expected_spans(ids, oo, tok_len_of(bench_vocab), ns)
    assert np.array_equal(spans, exp)
    # per document: BOS (0, 0), EOS (len, len), and the last body token ends at the document's length
    doc_len = np.diff(offs.astype(np.int64))
    first, last = oo[:-1], oo[1:] - 1
    assert np.all(spans[first] == 0)
    assert np.array_equal(spans[last, 0].astype(np.int64), doc_len) and np.array_equal(spans[last, 1].astype(np.int64), doc_len)
    assert np.array_equal(spans[last - 1, 1].astype(np.int64), doc_len)
    # a sample of documents: ids against the oracle, text under every span against the token bytes
    orc = helpers.oracle_for(bench_vocab)
    for lo in (0, 500_000, 999_000):
        hi = lo + 1000
        sub_offs = offs[lo:hi + 1] - offs[lo]
        sub = data[int(offs[lo]):int(offs[hi])]
        eids, eoo = orc.encode_batch(sub, sub_offs, True, True, threads=8)
        got = ids[int(oo[lo]):int(oo[hi])]
        assert np.array_equal(got, eids)
        check_spans(bench_vocab, sub, sub_offs, got, oo[lo:hi + 1] - oo[lo], spans[int(oo[lo]):int(oo[hi])])


def _device_case(tk, eng, data, offs, ids, oo, checks):
    import torch
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, np.uint32).view(np.int32)).cuda()
    d_oo = torch.from_numpy(np.asarray(oo, np.int64)).cuda()
    d_offs = torch.from_numpy(np.asarray(offs, np.int64)).cuda()
    d_bytes = torch.from_numpy(data).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    p = eng.token_spans_device(d_ids.data_ptr(), d_oo.data_ptr(), len(oo) - 1, len(ids), d_offs.data_ptr(), d_bytes.data_ptr(), checks,
                               stream)
    return torch.as_tensor(tk.DeviceView(p, 2 * len(ids), "<i4"), device="cuda").cpu().numpy().view(np.uint32).reshape(len(ids), 2)


def test_checks_catch_what_the_global_sum_misses(tk, test_vocab):
    v = test_vocab
    ns, tok_len = v["num_special"], tok_len_of(v)
    d, o = corpus.generate("ascii", 64, 512, seed=corpus.BASE_SEED + 11)
    data, offs = d, o
    eng = tk.Engine(v["tokens"], ns, v["bos"], v["eos"], device=0)
    try:
        ids, oo = eng.encode_batch(data, offs, True, True)
        ids, oo = ids.astype(np.uint32), oo.astype(np.int64)
        # clean ids: no error, spans as restated
        sp = _device_case(tk, eng, data, offs, ids, oo, tk.SPANS_CHECK_BYTES)
        check_spans(v, data, offs, ids, oo, sp)

        def global_sum(x):
            x = x.astype(np.int64)
            return int(tok_len[x[x >= ns] - ns].sum())

        # a fragment duplicated in document a and one removed from document b: the global byte sum does not move
        for a, b in ((5, 17), (40, 9)):
            x = ids[int(oo[b]) + 3]
            assert x >= ns
            lst = [ids[int(oo[k]):int(oo[k + 1])].tolist() for k in range(len(oo) - 1)]
            lst[b].pop(3)
            lst[a].insert(2, int(x))
            ids2 = np.array([i for doc in lst for i in doc], np.uint32)
            oo2 = np.concatenate([[0], np.cumsum([len(doc) for doc in lst])]).astype(np.int64)
            assert global_sum(ids2) == global_sum(ids) == len(data)
            for chk in (tk.SPANS_CHECK_COVER, tk.SPANS_CHECK_BYTES):
                with pytest.raises(tk.TokenizerError) as e:
                    _device_case(tk, eng, data, offs, ids2, oo2, chk)
                assert e.value.code == tk.TK_ERR_RUNTIME and e.value.bad_doc == min(a, b), str(e.value)
                assert "document %d" % min(a, b) in str(e.value)
            _device_case(tk, eng, data, offs, ids2, oo2, 0)             # no check asked: spans only, no error
        # one id replaced by another token of the same length: COVER passes, BYTES fails on that document
        doc = 23
        k = int(oo[doc]) + 4
        x = int(ids[k])
        same = [r + ns for r in np.nonzero(tok_len == tok_len[x - ns])[0] if r + ns != x]
        ids3 = ids.copy()
        ids3[k] = same[0]
        _device_case(tk, eng, data, offs, ids3, oo, tk.SPANS_CHECK_COVER)
        with pytest.raises(tk.TokenizerError) as e:
            _device_case(tk, eng, data, offs, ids3, oo, tk.SPANS_CHECK_BYTES)
        assert e.value.code == tk.TK_ERR_RUNTIME and e.value.bad_doc == doc, str(e.value)
        # an id outside the vocabulary
        ids4 = ids.copy()
        ids4[int(oo[30]) + 2] = ns + len(v["tokens"]) + 7
        for chk in (0, tk.SPANS_CHECK_BYTES):
            with pytest.raises(tk.TokenizerError) as e:
                _device_case(tk, eng, data, offs, ids4, oo, chk)
            assert e.value.code == tk.TK_ERR_RUNTIME and e.value.bad_doc == 30, str(e.value)
        # the context still works after the failures
        sp = _device_case(tk, eng, data, offs, ids, oo, tk.SPANS_CHECK_BYTES)
        check_spans(v, data, offs, ids, oo, sp)
    finally:
        eng.close()


def test_callers_ids_over_table_edges(tk):
    """The caller's ids over helpers.table_edge_vocab(33001), the text their concatenation: tokens of 16, 17, 254, 255, 256, 300
    and 5000 bytes (a length byte of 0xFF sends the kernel to the offsets), ranks on both sides of the LDS part of the length
    table.  With TK_SPANS_CHECK_BYTES the clean call passes, and one changed byte anywhere in a long token names its document."""
    v = helpers.table_edge_vocab(33001)
    ns, toks = v["num_special"], v["tokens"]
    a, z = ns + 0x61, ns + 0x7A
    longs = [ns + v["edge"][(n, f)] for n in (15, 16, 17, 254, 255, 256, 300) for f in ("ascii", "zh_cut", "zh_tail", "rocket")]
    longs += [ns + v["long"]] + [ns + r for r in sorted(v["hand"])] + [ns + r for r in sorted(v["high"])]
    targets = [v["edge"][(300, "ascii")], 32767, 32769]
    lists = [[a, z, ns + r, a] for r in targets]                          # (documents 0..2: the ones a byte is changed in)
    lists += [[t] for t in longs] + [[a, t, 1, z, t, 3] for t in longs] + [longs, longs[::-1], [], [3], [ns + r for r in range(32760, 32776)]]
    rng = np.random.default_rng(9)
    pool = np.array(longs + list(range(ns, ns + 256)) + list(range(ns + 32700, ns + 32800)) + [0, 3, 7])
    lists += [pool[rng.integers(0, len(pool), int(rng.integers(0, 150)))].tolist() for _ in range(40)]
    ids = np.array([i for x in lists for i in x], np.uint32)
    oo = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    data, offs = pack([b"".join(toks[i - ns] for i in x if i >= ns) for x in lists])
    eng = tk.Engine(toks, ns, v["bos"], v["eos"], device=0)
    try:
        for chk in (0, tk.SPANS_CHECK_COVER, tk.SPANS_CHECK_BYTES):
            check_spans(v, data, offs, ids, oo, _device_case(tk, eng, data, offs, ids, oo, chk))
        for doc, r in enumerate(targets):
            for pos in (0, 15, 16, 254, 299):
                if pos >= len(toks[r]):                                   # (rank 32767 holds 255 bytes)
                    continue
                changed = data.copy()
                changed[int(offs[doc]) + 2 + pos] ^= 0x01
                _device_case(tk, eng, changed, offs, ids, oo, tk.SPANS_CHECK_COVER)
                with pytest.raises(tk.TokenizerError) as e:
                    _device_case(tk, eng, changed, offs, ids, oo, tk.SPANS_CHECK_BYTES)
                assert e.value.code == tk.TK_ERR_RUNTIME and e.value.bad_doc == doc, (r, pos, str(e.value))
                assert "id index 2 " in str(e.value)
        check_spans(v, data, offs, ids, oo, _device_case(tk, eng, data, offs, ids, oo, tk.SPANS_CHECK_BYTES))
    finally:
        eng.close()


def test_encode_outputs_outlive_a_spans_call(tk, eng_bench, bench_vocab):
    """tk_token_spans_device on the d_ids / d_out_offsets the encode call returned leaves them valid and unchanged."""
    import torch
    docs = sweep_docs()
    data, offs = pack(docs)
    d_bytes = torch.from_numpy(data).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    p_ids, p_oo, n = eng_bench.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), len(docs), len(data), True, True, stream)
    p_sp = eng_bench.token_spans_device(p_ids, p_oo, len(docs), n, d_offs.data_ptr(), d_bytes.data_ptr(), tk.SPANS_CHECK_BYTES, stream)
    assert p_sp not in (p_ids, p_oo)
    ids = torch.as_tensor(tk.DeviceView(p_ids, n, "<i4"), device="cuda").cpu().numpy().view(np.uint32)
    oo = torch.as_tensor(tk.DeviceView(p_oo, len(docs) + 1, "<i8"), device="cuda").cpu().numpy().astype(np.uint64)
    sp = torch.as_tensor(tk.DeviceView(p_sp, 2 * n, "<i4"), device="cuda").cpu().numpy().view(np.uint32).reshape(n, 2)
    eids, eoo = helpers.oracle_for(bench_vocab).encode_batch(data, offs, True, True, threads=8)
    assert np.array_equal(oo, eoo) and np.array_equal(ids, eids)
    check_spans(bench_vocab, data, offs, ids, oo, sp)


def test_host_spans_equal_kernel_spans(tk, bench_vocab):
    """tk_tokenizer_encode_with_spans (host prefix sum) against the kernel on the same documents, small-path batches included."""
    t = tk.Tekkenizer.from_file(bench_vocab["path"], device=0)
    try:
        eng = t.engine()
        docs = [x.decode("utf-8") for x in sweep_docs() if len(x) < 20000]
        host = [t.encode_with_offsets(x, True, True) for x in docs]
        calls0 = eng.small_path_calls()
        for lo in range(0, len(docs), 200):                         # batches of <= 1024 documents / 64 KiB: the one-launch path
            chunk = docs[lo:lo + 200]
            sub, total = [], 0
            for x in chunk:
                if total + len(x.encode()) > 60000:
                    break
                sub.append(x)
                total += len(x.encode())
            assert t.encode_batch_with_offsets(sub, True, True) == host[lo:lo + len(sub)]
        assert eng.small_path_calls() > calls0
        assert t.encode_batch_with_offsets(docs, True, True) == host                                  # the batch pipeline
        assert [h[1] for h in host] == [s for _, s in t.encode_batch_with_offsets(docs, True, True, checks=tk.SPANS_CHECK_BYTES)]
    finally:
        t.close()
