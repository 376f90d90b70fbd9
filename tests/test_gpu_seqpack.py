"""Packed fixed-length training rows on the GPU (include/tekken_hip.h tk_seqpack_from_ids_device and the entries around it,
csrc/tk_seqpack.hip) against the plain-loop restatement of the definition in tests/test_seqpack_cpu.py -- element by element
over every output, never through a sum."""
import json

import numpy as np
import pytest

import helpers
from helpers import on_device, to_host
from test_gpu_spans import pack, sweep_docs
from test_seqpack_cpu import ALL, CU_SEQLENS, DROP_LAST, I64, POSITIONS, SEGMENTS, expected_packed

pytestmark = pytest.mark.gpu

TENSORS = ("input_ids", "position_ids", "segment_ids", "cu_seqlens")
COUNTS = ("n_rows", "n_used", "n_left", "n_segments", "max_seqlen")


def fetch(res):
    """SeqpackResult -> dict like expected_packed's."""
    dt = np.int64 if res.typestr == "<i8" else np.int32
    shape = (res.n_rows, res.row_len)
    v = res.views()
    out = {k: to_host(v[i], shape, dt) for i, k in enumerate(TENSORS[:3])}
    out["cu_seqlens"] = to_host(v[3], (res.n_segments + 1,), np.int32)
    out.update({k: getattr(res, k) for k in COUNTS})
    return out


def assert_same(got, exp, what=""):
    helpers.assert_same(got, exp, what, COUNTS, TENSORS)


def packed_of(eng, d_ids, d_oo, n_ids, seq_len, pad_id, flags):
    import torch
    res = eng.seqpack_from_ids_device(d_ids.data_ptr(), d_oo.data_ptr(), d_oo.numel() - 1, n_ids, seq_len, pad_id, flags,
                                      torch.cuda.current_stream().cuda_stream)
    return res, fetch(res)


@pytest.fixture(scope="module")
def vocabs(test_vocab, bench_vocab):
    return {"test": test_vocab, "bench": bench_vocab}


@pytest.fixture(scope="module")
def eng_bench(tk, bench_vocab):
    e = tk.Engine(bench_vocab["tokens"], bench_vocab["num_special"], bench_vocab["bos"], bench_vocab["eos"], device=0)
    yield e
    e.close()


@pytest.fixture()
def small_tok(tk, small_vocab):
    from test_host_tokenizer import model
    t = tk.Tekkenizer.from_json(json.dumps(model(small_vocab["tokens"], specials=("<unk>", "<s>", "</s>", "<pad>"))), device=0)
    yield t
    t.close()


HELLO = [1, 266, 42, 129, 121, 124, 118, 110, 2]   # "hello world" with BOS / EOS on the small vocabulary (tests/test_gpu_spans.py)


def test_known_answer_small_vocab(tk, small_tok):
    import torch
    t = small_tok
    P = t.pad_id()
    assert P == 3
    docs = ["hello world", "", "hello"]             # the stream: HELLO + [1, 2] + [1, 266, 2], 14 ids, documents at 0, 9, 11
    r = t.encode_batch_packed(docs, seq_len=4)
    assert r["input_ids"].tolist() == [[1, 266, 42, 129], [121, 124, 118, 110], [2, 1, 2, 1], [266, 2, P, P]]
    assert r["position_ids"].tolist() == [[0, 1, 2, 3], [0, 1, 2, 3], [0, 0, 1, 0], [0, 1, 0, 0]]
    assert r["segment_ids"].tolist() == [[1, 1, 1, 1], [1, 1, 1, 1], [1, 2, 2, 3], [1, 1, 0, 0]]
    assert r["cu_seqlens"].tolist() == [0, 4, 8, 9, 11, 12, 14]
    assert (r["max_seqlen"], r["n_rows"], r["n_used"], r["n_left"], r["n_segments"]) == (4, 4, 14, 0, 6)
    assert isinstance(r["input_ids"], torch.Tensor) and r["input_ids"].dtype == torch.int64
    r = t.encode_batch_packed(docs, seq_len=4, drop_last=True, dtype="int32", return_tensors="np")
    assert r["input_ids"].tolist() == [[1, 266, 42, 129], [121, 124, 118, 110], [2, 1, 2, 1]] and r["input_ids"].dtype == np.int32
    assert r["segment_ids"].tolist() == [[1, 1, 1, 1], [1, 1, 1, 1], [1, 2, 2, 3]]
    assert r["cu_seqlens"].tolist() == [0, 4, 8, 9, 11, 12] and (r["n_used"], r["n_left"], r["n_segments"]) == (12, 2, 5)
    r = t.encode_batch_packed(docs, seq_len=4, add_bos=False, add_eos=False)     # [266, 42, 129, 121, 124, 118, 110] + [] + [266]
    assert r["input_ids"].tolist() == [[266, 42, 129, 121], [124, 118, 110, 266]]
    assert r["position_ids"].tolist() == [[0, 1, 2, 3], [0, 1, 2, 0]] and r["segment_ids"].tolist() == [[1, 1, 1, 1], [1, 1, 1, 2]]
    assert r["cu_seqlens"].tolist() == [0, 4, 7, 8] and r["max_seqlen"] == 4
    r = t.encode_batch_packed(docs, seq_len=5, pad_id=77)
    assert r["input_ids"].tolist() == [[1, 266, 42, 129, 121], [124, 118, 110, 2, 1], [2, 1, 266, 2, 77]]
    assert r["position_ids"].tolist() == [[0, 1, 2, 3, 4], [0, 1, 2, 3, 0], [0, 0, 1, 2, 0]]
    assert r["segment_ids"].tolist() == [[1, 1, 1, 1, 1], [1, 1, 1, 1, 2], [1, 2, 2, 2, 0]]
    assert r["cu_seqlens"].tolist() == [0, 5, 9, 10, 11, 14] and r["max_seqlen"] == 5


# ---- made-up ids through tk_seqpack_from_ids_device ----

def made_up(first_len=None):
    """8 700 documents: 700 with up to 299 ids (80 of them empty, the first 3 and last 2 among them; one of 50 001 ids), a run of
    5 000 empty ones and a block of 3 000 one-id ones.  first_len: the ids of the first non-empty document."""
    rng = np.random.default_rng(29)
    counts = rng.integers(0, 300, 700)
    # 80 counts set to 0: the first 3, the last 2 and 75 drawn without replacement from the documents not given a length below
    pool = np.setdiff1d(np.arange(700), [0, 1, 2, 3, 4, 333, 698, 699])
    counts[rng.choice(pool, 75, replace=False)] = 0
    counts[:3] = 0
    counts[-2:] = 0
    counts[333] = 50_001
    counts[3] = first_len if first_len else 17
    counts[4] = 40                                        # (non-empty: with first_len = L it starts at the start of row 1)
    counts = np.concatenate([counts[:200], np.zeros(5000, np.int64), counts[200:500], np.ones(3000, np.int64), counts[500:]])
    oo = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ids = rng.integers(0, 2**31 - 1, int(oo[-1])).astype(np.uint32)
    return ids, oo


N_MADE_UP = int(made_up()[1][-1])
assert N_MADE_UP == int(made_up(64)[1][-1]) - 47          # (the variants differ in the first document alone)
ROW_LENS = (1, 3, 4, 5, 64, 127, 128, 2048, 8196, 50_000, N_MADE_UP, N_MADE_UP + 1)
P_MADE_UP = 5
_cases = {}


def case(L, drop):
    """(ids, oo, expected_packed of them) of one row length: computed once, shared, never changed."""
    key = (L, drop)
    if key not in _cases:
        ids, oo = made_up(L if L in (64, 128) else None)
        _cases[key] = (ids, oo, expected_packed(ids, oo, L, P_MADE_UP, ALL | (DROP_LAST if drop else 0)))
    return _cases[key]


def test_the_case_set_holds_what_it_is_for():
    """From expected_packed's results alone: the properties the kernels' branches need are in the made-up cases."""
    seen = set()
    for L in ROW_LENS:
        ids, oo, e = case(L, False)
        N, n = int(oo[-1]), np.diff(oo)
        if e["n_rows"] and int(e["segment_ids"].max(axis=1).max()) >= 3:
            seen.add("a row with 3 segments or more")
        first_row, last_row = oo[:-1][n > 0] // L, (oo[1:][n > 0] - 1) // L
        if np.any(last_row - first_row >= 2):
            seen.add("a document spread over 3 rows or more")
        cu = e["cu_seqlens"][:-1]
        doc_starts = set(oo[:-1][n > 0].tolist()) - {0}
        if any(s % L == 0 for s in doc_starts):
            assert sum(1 for s in cu.tolist() if s in doc_starts and s % L == 0) == sum(1 for s in doc_starts if s % L == 0)
            seen.add("a document start that coincides with a row start")
            if L in (64, 128):
                assert L in doc_starts
                seen.add("... constructed at L = %d" % L)
        if e["n_rows"] and np.any(e["segment_ids"][-1] == 0):
            seen.add("a padded last row")
        if N % L == 0:
            assert e["n_left"] == 0 and np.all(e["segment_ids"] > 0)
            seen.add("an exact fit")
        if case(L, True)[2]["n_left"] > 0:
            seen.add("ids left over with DROP_LAST")
        # a tile of 4 096 stream positions with more document starts than the 1 024 the kernel's LDS array holds, and one with none
        per_tile = np.bincount(oo[:-1][n > 0] // 4096, minlength=N // 4096 + 1)
        if per_tile.max() > 1024 and per_tile.min() == 0:
            seen.add("tiles for both forms of the search")
    assert seen == {"a row with 3 segments or more", "a document spread over 3 rows or more", "a document start that coincides with a row start",
                    "... constructed at L = 64", "... constructed at L = 128", "a padded last row", "an exact fit",
                    "ids left over with DROP_LAST", "tiles for both forms of the search"}


@pytest.mark.parametrize("L", ROW_LENS)
def test_from_ids_on_ids_encode_never_produced(tk, eng_bench, L):
    P = P_MADE_UP
    for drop in (False, True):
        ids, oo, exp = case(L, drop)
        d_ids, d_oo = on_device(ids, oo)
        flags = ALL | (DROP_LAST if drop else 0)
        res, got = packed_of(eng_bench, d_ids, d_oo, len(ids), L, P, flags)
        assert_same(got, exp, (L, drop))
        # int64 equals int32 value for value
        _, got64 = packed_of(eng_bench, d_ids, d_oo, len(ids), L, P, flags | I64)
        for k in TENSORS[:3]:
            assert got64[k].dtype == np.int64 and np.array_equal(got64[k], got[k].astype(np.int64)), (L, drop, k)
        assert np.array_equal(got64["cu_seqlens"], got["cu_seqlens"]) and got64["cu_seqlens"].dtype == np.int32
        assert all(got64[k] == got[k] for k in COUNTS)
        # each optional output alone deselected: its pointer is NULL, the others are unchanged
        for off, key in ((POSITIONS, "position_ids"), (SEGMENTS, "segment_ids"), (CU_SEQLENS, "cu_seqlens")):
            res1, got1 = packed_of(eng_bench, d_ids, d_oo, len(ids), L, P, flags & ~off)
            assert getattr(res1, key + "_ptr") is None and got1[key] is None
            assert_same(got1, {**exp, key: None}, (L, drop, "without", key))


# ---- the fused and host entries ----

@pytest.mark.parametrize("vname", ["test", "bench"])
def test_fused_entry_sweep(tk, vocabs, vname):
    import torch
    v = vocabs[vname]
    P = 7                                            # an id encode never emits (a special that is neither BOS nor EOS)
    assert P < v["num_special"] and P not in (v["bos"], v["eos"])
    docs = [x for x in sweep_docs() if len(x) < 70000]
    data, offs = pack(docs)
    D = len(docs)
    orc = helpers.oracle_for(v)
    eng = tk.Engine(v["tokens"], v["num_special"], v["bos"], v["eos"], device=0)
    d_bytes = torch.from_numpy(data).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    try:
        for i, (bos, eos) in enumerate(((False, False), (True, False), (False, True), (True, True))):
            eids, eoo = orc.encode_batch(data, offs, bos, eos, threads=8)
            for j, L in enumerate((64, 512, 2048)):
                flags = ALL | (I64 if (i + j) & 1 else 0) | (DROP_LAST if j == 1 else 0)
                p_ids, p_oo, n_ids, res = eng.encode_batch_device_seqpack(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), L, bos, eos,
                                                                          pad_id=P, flags=flags, checks=tk.CHECK_OFFSETS, stream=stream)
                ids = to_host(tk.DeviceView(p_ids, n_ids, "<i4"), (n_ids,), np.uint32)
                oo = to_host(tk.DeviceView(p_oo, D + 1, "<i8"), (D + 1,), np.uint64)
                assert np.array_equal(oo, eoo) and np.array_equal(ids, eids)
                assert_same(fetch(res), expected_packed(eids, eoo, L, P, flags), (vname, bos, eos, L))
    finally:
        eng.close()


def test_host_entry_equals_device_entry(tk, eng_bench, bench_vocab):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    small = sweep_docs()[:60] + [b"", b"a"]          # ASCII documents of 512 bytes: no piece that makes the one-launch kernel hand the batch back
    assert sum(len(x) for x in small) < 60000
    large = sweep_docs()
    P = 7
    for docs, is_small in ((small, True), (large, False)):
        data, offs = pack(docs)
        d_bytes = torch.from_numpy(data).cuda()
        d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
        for L, flags in ((64, ALL), (510, ALL | I64 | DROP_LAST), (2048, POSITIONS | I64)):
            calls0 = eng_bench.small_path_calls()
            host = eng_bench.encode_batch_seqpack(data, offs, L, True, True, pad_id=P, flags=flags)
            assert (eng_bench.small_path_calls() > calls0) == is_small
            _, _, _, res = eng_bench.encode_batch_device_seqpack(d_bytes.data_ptr(), d_offs.data_ptr(), len(docs), len(data), L, True, True,
                                                                 pad_id=P, flags=flags, stream=stream)
            dev = fetch(res)
            assert_same(host, dev, (is_small, L, flags))
    eids, eoo = helpers.oracle_for(bench_vocab).encode_batch(data, offs, True, True, threads=8)
    assert_same(dev, expected_packed(eids, eoo, 2048, P, POSITIONS | I64))


def test_outputs_outlive_each_other(tk, eng_bench, bench_vocab):
    import torch
    docs = [x for x in sweep_docs() if len(x) < 70000]
    data, offs = pack(docs)
    D = len(docs)
    d_bytes = torch.from_numpy(data).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    eng = eng_bench
    p_ids, p_oo, p_sp, n = eng.encode_batch_device_spans(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), True, True, stream=stream)
    dn = eng.dense_from_ids_device(p_ids, p_oo, D, n, max_length=128, pad_id=7, keep_head=1, keep_tail=1, flags=4 | 16, stream=stream)   # FIXED | MASK

    def snapshot():
        return (to_host(tk.DeviceView(p_ids, n, "<i4"), (n,), np.uint32).copy(), to_host(tk.DeviceView(p_oo, D + 1, "<i8"), (D + 1,), np.uint64).copy(),
                to_host(tk.DeviceView(p_sp, 2 * n, "<i4"), (2 * n,), np.uint32).copy(),
                to_host(tk.DeviceView(dn.ids_ptr, (D, 128), "<i4"), (D, 128), np.int32).copy(),
                to_host(tk.DeviceView(dn.mask_ptr, (D, 128), "|u1"), (D, 128), np.uint8).copy(),
                to_host(tk.DeviceView(dn.lengths_ptr, D, "<i4"), (D,), np.uint32).copy())

    before = snapshot()
    eids, eoo = helpers.oracle_for(bench_vocab).encode_batch(data, offs, True, True, threads=8)
    assert np.array_equal(before[0], eids) and np.array_equal(before[1], eoo)
    good = eng.seqpack_from_ids_device(p_ids, p_oo, D, n, 512, 7, ALL, stream)
    ptrs = {good.input_ids_ptr, good.position_ids_ptr, good.segment_ids_ptr, good.cu_seqlens_ptr, dn.ids_ptr, dn.mask_ptr, dn.lengths_ptr,
            p_ids, p_oo, p_sp}
    assert len(ptrs) == 10 and None not in ptrs and 0 not in ptrs
    exp = expected_packed(eids, eoo, 512, 7, ALL)
    assert_same(fetch(good), exp)
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a, b)
    # every case of step 8: refused, and the first packed result stays readable
    bad = [dict(seq_len=0, flags=ALL), dict(seq_len=2**31, flags=ALL), dict(seq_len=2**32 - 1, flags=0), dict(seq_len=512, flags=ALL | 32),
           dict(seq_len=512, flags=1 << 31), dict(seq_len=2**30, flags=0, n_ids=2**36 + 1),         # 65 rows of 2^30: beyond 2^36 elements
           dict(seq_len=2**30, flags=CU_SEQLENS, n_ids=2**31),                                       # n_used = 2^31 does not fit int32
           dict(seq_len=512, flags=ALL, n_docs=0)]                                                   # ids without a document
    for opt in bad:
        with pytest.raises(tk.TokenizerError) as e:
            eng.seqpack_from_ids_device(p_ids, p_oo, opt.get("n_docs", D), opt.get("n_ids", n), opt["seq_len"], 7, opt["flags"], stream)
        assert e.value.code == tk.TK_ERR_INVALID_ARG, (opt, str(e.value))
        assert_same(fetch(good), exp, ("the earlier result after", opt))
    with pytest.raises(tk.TokenizerError) as e:
        eng.encode_batch_device_seqpack(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), 0, True, True, stream=stream)
    assert e.value.code == tk.TK_ERR_INVALID_ARG
    with pytest.raises(tk.TokenizerError) as e:
        eng.encode_batch_seqpack(data, offs, 64, True, True, flags=64)
    assert e.value.code == tk.TK_ERR_INVALID_ARG
    assert_same(fetch(good), exp, "the earlier result after the fused entries' errors")


def test_empty_shapes(tk, eng_bench):
    import torch
    eng = eng_bench
    z1 = np.zeros(1, np.int64)
    for flags in (ALL, ALL | I64 | DROP_LAST, 0):
        for oo in (z1, np.zeros(6, np.int64)):                       # D = 0; all-empty documents
            d_ids, d_oo = on_device(np.zeros(0, np.uint32), oo)
            _, got = packed_of(eng, d_ids, d_oo, 0, 8, 9, flags)
            assert_same(got, expected_packed([], oo, 8, 9, flags), (flags, len(oo)))
        host = eng.encode_batch_seqpack(np.zeros(0, np.uint8), np.zeros(1, np.uint64), 8, True, True, pad_id=9, flags=flags)
        assert_same(host, expected_packed([], z1, 8, 9, flags), ("host", flags))
    rows = [[1, 20, 21, 22, 23, 24, 2], [1, 30, 2], [], [1, 40, 41, 42, 2]]
    oo = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    ids = np.array([i for r in rows for i in r], np.uint32)
    d_ids, d_oo = on_device(ids, oo)
    res, got = packed_of(eng, d_ids, d_oo, 15, 16, 9, ALL | DROP_LAST)          # N < L with DROP_LAST
    assert (res.n_rows, res.n_left, res.n_used, res.n_segments, res.max_seqlen) == (0, 15, 0, 0, 0) and got["cu_seqlens"].tolist() == [0]
    assert_same(got, expected_packed(ids, oo, 16, 9, ALL | DROP_LAST))
    for L, flags in ((4, ALL), (4, ALL | DROP_LAST), (5, ALL | I64), (7, ALL), (16, ALL), (1, ALL), (15, ALL)):   # the hand-made table
        _, got = packed_of(eng, d_ids, d_oo, 15, L, 9, flags)
        assert_same(got, expected_packed(ids, oo, L, 9, flags), (L, flags))


def test_tensors_from_encode_batch_packed(tk, bench_vocab):
    import torch
    t = tk.Tekkenizer.from_file(bench_vocab["path"], device=0)
    try:
        docs = [x.decode("utf-8") for x in sweep_docs()[:40]] + ["", "tail"]
        lists = t.encode_batch(docs, True, True)
        stream_ids = np.array([i for row in lists for i in row], np.int64)
        oo = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
        N = len(stream_ids)
        for dtype, tdt in (("int64", torch.int64), ("int32", torch.int32)):
            r = t.encode_batch_packed(docs, 256, dtype=dtype)
            R = -(-N // 256)
            assert set(r) == {"input_ids", "position_ids", "segment_ids", "cu_seqlens", "max_seqlen", "n_rows", "n_used", "n_left", "n_segments"}
            for k in TENSORS[:3]:
                assert r[k].dtype == tdt and tuple(r[k].shape) == (R, 256) and r[k].is_cuda and r[k].is_contiguous(), k
            assert r["cu_seqlens"].dtype == torch.int32 and tuple(r["cu_seqlens"].shape) == (r["n_segments"] + 1,) and r["cu_seqlens"].is_cuda
            assert (r["n_rows"], r["n_used"], r["n_left"]) == (R, N, 0)
            assert np.array_equal(r["input_ids"].flatten()[:r["n_used"]].cpu().numpy(), stream_ids)
            assert torch.all(r["input_ids"].flatten()[N:] == t.pad_id())
            keep = {k: r[k].cpu().numpy().copy() for k in TENSORS}
            t.encode_batch_packed(["something else entirely"] * 300, 64, dtype=dtype)      # copy=True survives the next call
            for k in TENSORS:
                assert np.array_equal(r[k].cpu().numpy(), keep[k]), k
            exp = expected_packed(stream_ids, oo, 256, t.pad_id(), ALL | (I64 if dtype == "int64" else 0))
            assert_same({**{k: keep[k] for k in TENSORS}, **{k: r[k] for k in COUNTS}}, exp, dtype)
            n = t.encode_batch_packed(docs, 256, dtype=dtype, return_tensors="np")
            assert_same(n, exp, ("np", dtype))
        r = t.encode_batch_packed(docs, 256, drop_last=True, return_position_ids=False, return_cu_seqlens=False, copy=False)
        assert r["position_ids"] is None and r["cu_seqlens"] is None and r["segment_ids"] is not None
        assert r["n_rows"] == N // 256 and r["n_left"] == N % 256 and tuple(r["input_ids"].shape) == (N // 256, 256)
        assert np.array_equal(r["input_ids"].flatten().cpu().numpy(), stream_ids[:r["n_used"]])
        with pytest.raises(tk.TokenizerError) as e:
            t.encode_batch_packed(docs, 0)
        assert e.value.code == tk.TK_ERR_INVALID_ARG
        with pytest.raises(tk.TokenizerError) as e:
            t.encode_batch_packed(docs, 16, dtype="int16")
        assert e.value.code == tk.TK_ERR_INVALID_ARG
    finally:
        t.close()
