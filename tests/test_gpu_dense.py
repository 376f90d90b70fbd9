"""Model-ready dense batches on the GPU (include/tekken_hip.h tk_dense_from_ids_device and the entries around it,
csrc/tk_dense.hip) against the numpy restatement of the definition in tests/test_dense_cpu.py -- element by element over the
whole tensor, never through a sum."""
import json

import numpy as np
import pytest

import corpus
import helpers
from helpers import on_device, to_host
from test_dense_cpu import FIXED, I64, MASK, PAD_LEFT, TRUNC_LEFT, expected_dense, expected_ragged
from test_gpu_spans import pack, sweep_docs

pytestmark = pytest.mark.gpu


def fetch(tk, res):
    """DenseResult -> dict like expected_dense's."""
    v_ids, v_mask, v_len = res.views()
    D, L = res.n_docs, res.row_len
    return {"dense": to_host(v_ids, (D, L), np.int64 if res.typestr == "<i8" else np.int32),
            "mask": to_host(v_mask, (D, L), np.uint8), "lengths": to_host(v_len, (D,), np.uint32),
            "row_len": L, "n_truncated": res.n_truncated}


def assert_same(got, exp, what=""):
    assert got["row_len"] == exp["row_len"], (what, got["row_len"], exp["row_len"])
    helpers.assert_array_same(got["dense"], exp["dense"], what)
    assert (got["mask"] is None) == (exp["mask"] is None), what
    if exp["mask"] is not None:
        assert np.array_equal(got["mask"], exp["mask"]), what
    assert np.array_equal(got["lengths"], exp["lengths"]), what
    assert got["n_truncated"] == exp["n_truncated"], what


def dense_of(tk, eng, ids, oo, **kw):
    import torch
    d_ids, d_oo = on_device(ids, oo)
    res = eng.dense_from_ids_device(d_ids.data_ptr(), d_oo.data_ptr(), len(oo) - 1, len(ids), stream=torch.cuda.current_stream().cuda_stream, **kw)
    return fetch(tk, res)


def ragged_of(tk, eng, dense, lengths, pad_id, pad_left):
    """tk_ragged_from_dense_device on a host array -> (ids uint32, offsets uint64)."""
    import torch
    D, L = dense.shape
    d = torch.from_numpy(np.ascontiguousarray(dense) if D * L else np.zeros(1, dense.dtype)).cuda()
    d_len = torch.from_numpy(np.asarray(lengths, np.uint32).view(np.int32)).cuda() if lengths is not None and D else None
    flags = (I64 if dense.dtype == np.int64 else 0) | (PAD_LEFT if pad_left else 0)
    p_ids, p_oo, n = eng.ragged_from_dense_device(d.data_ptr() if D * L else 0, D, L, flags, d_len.data_ptr() if d_len is not None else 0, pad_id,
                                                  torch.cuda.current_stream().cuda_stream)
    oo = to_host(tk.DeviceView(p_oo, D + 1, "<i8"), (D + 1,), np.uint64)
    assert int(oo[-1]) == n
    return to_host(tk.DeviceView(p_ids, n, "<i4"), (n,), np.uint32), oo


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
    r = t.encode_batch_padded(["hello world"], True, True)
    assert r["input_ids"].tolist() == [HELLO] and r["attention_mask"].tolist() == [[1] * 9] and r["n_truncated"] == 0
    r = t.encode_batch_padded(["hello world"], True, True, max_length=5)
    assert r["input_ids"].tolist() == [[1, 266, 42, 129, 2]] and r["n_truncated"] == 1 and r["lengths"].tolist() == [5]
    r = t.encode_batch_padded(["hello world"], True, True, max_length=5, truncation_side="left")
    assert r["input_ids"].tolist() == [[1, 124, 118, 110, 2]]
    r = t.encode_batch_padded(["hello world", ""], True, True, max_length=5, padding_side="left", padding="max_length", pad_to_multiple_of=4)
    assert r["input_ids"].tolist() == [[P, P, P, 1, 266, 42, 129, 2], [P, P, P, P, P, P, 1, 2]]
    assert r["attention_mask"].tolist() == [[0, 0, 0, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0, 1, 1]]
    assert r["lengths"].tolist() == [5, 2] and r["n_truncated"] == 1
    r = t.encode_batch_padded(["hello world", ""], True, True, padding_side="left", dtype="int32", return_tensors="np")
    assert r["input_ids"].tolist() == [HELLO, [P] * 7 + [1, 2]] and r["input_ids"].dtype == np.int32
    r = t.encode_batch_padded(["hello world", ""], False, False, max_length=4)           # no BOS / EOS: nothing is kept
    assert r["input_ids"].tolist() == [[266, 42, 129, 121], [P] * 4] and r["attention_mask"].tolist() == [[1] * 4, [0] * 4]
    assert isinstance(r["input_ids"], torch.Tensor)


def option_grid():
    """Between them: every flag, max_length 0 / 2 / 64 / 128 / 512, multiple_of, both element types."""
    return [dict(max_length=0, flags=MASK), dict(max_length=0, multiple_of=64, flags=PAD_LEFT),
            dict(max_length=2, flags=MASK | FIXED | I64), dict(max_length=2, flags=TRUNC_LEFT | PAD_LEFT | MASK),
            dict(max_length=64, flags=MASK | I64), dict(max_length=64, multiple_of=7, flags=TRUNC_LEFT | MASK),
            dict(max_length=128, flags=FIXED | MASK), dict(max_length=128, flags=PAD_LEFT | TRUNC_LEFT | I64 | MASK | FIXED),
            dict(max_length=512, multiple_of=64, flags=MASK), dict(max_length=512, flags=FIXED | PAD_LEFT | I64),
            dict(max_length=511, flags=FIXED | MASK | I64)]


@pytest.mark.parametrize("vname", ["test", "bench"])
def test_property_sweep(tk, vocabs, vname):
    import torch
    v = vocabs[vname]
    P = 7                                            # an id encode never emits (a special that is neither BOS nor EOS)
    assert P < v["num_special"] and P not in (v["bos"], v["eos"])
    docs = [x for x in sweep_docs() if len(x) < 70000]   # (without the one 70 000-byte document the max_length = 0 tensors stay small)
    data, offs = pack(docs)
    D = len(docs)
    orc = helpers.oracle_for(v)
    eng = tk.Engine(v["tokens"], v["num_special"], v["bos"], v["eos"], device=0)
    d_bytes = torch.from_numpy(data).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    try:
        for bos, eos in ((False, False), (True, False), (False, True), (True, True)):
            eids, eoo = orc.encode_batch(data, offs, bos, eos, threads=8)
            n = np.diff(eoo.astype(np.int64))
            for T in (64, 128, 512):
                share = float((n > T).mean())
                print("vocab %s bos %d eos %d max_length %d: share of truncated documents %.3f" % (vname, bos, eos, T, share))
                assert 0.1 < share < 0.9, (T, share)
            for opt in option_grid():
                if opt["max_length"] and bos + eos > opt["max_length"]:
                    continue
                p_ids, p_oo, n_ids, res = eng.encode_batch_device_dense(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), bos, eos,
                                                                        pad_id=P, checks=tk.CHECK_OFFSETS, stream=stream, **opt)
                ids = to_host(tk.DeviceView(p_ids, n_ids, "<i4"), (n_ids,), np.uint32)
                oo = to_host(tk.DeviceView(p_oo, D + 1, "<i8"), (D + 1,), np.uint64)
                assert np.array_equal(oo, eoo) and np.array_equal(ids, eids)
                exp = expected_dense(eids, eoo, opt["max_length"], opt.get("multiple_of", 0), P, int(bos), int(eos), opt["flags"])
                assert_same(fetch(tk, res), exp, (vname, bos, eos, opt))
                if opt["max_length"] in (64, 128, 512):
                    assert 0.1 < res.n_truncated / D < 0.9, (opt, res.n_truncated)
    finally:
        eng.close()


def test_from_ids_on_ids_encode_never_produced(tk, eng_bench):
    rng = np.random.default_rng(23)
    P = 5
    counts = rng.integers(0, 300, 700)
    counts[rng.integers(0, 700, 80)] = 0
    counts[333] = 50_001                                  # one very long document
    counts[:3] = 0
    counts[-2:] = 0
    oo = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ids = rng.integers(0, 2**31 - 1, int(oo[-1])).astype(np.uint32)
    grid = [dict(max_length=T, multiple_of=m, keep_head=h, keep_tail=t, flags=f)
            for T, m, h, t, f in ((0, 0, 3, 3, MASK), (0, 4, 0, 0, PAD_LEFT | MASK), (1, 0, 1, 1, MASK), (3, 0, 3, 3, TRUNC_LEFT | MASK),
                                  (3, 0, 0, 3, MASK), (100, 0, 2, 3, MASK), (100, 8, 3, 1, TRUNC_LEFT | PAD_LEFT | MASK),
                                  (101, 0, 1, 2, FIXED | MASK), (200, 0, 0, 0, FIXED | PAD_LEFT), (8192, 0, 3, 3, FIXED | MASK),
                                  (9001, 0, 3, 2, TRUNC_LEFT | MASK), (50_001, 0, 1, 1, MASK), (50_000, 0, 1, 1, PAD_LEFT))]
    for opt in grid:
        exp = expected_dense(ids, oo, pad_id=P, **opt)
        got = dense_of(tk, eng_bench, ids, oo, pad_id=P, **opt)
        assert_same(got, exp, opt)
        assert (got["mask"] is None) == (not opt["flags"] & MASK)
        # int32 and int64 give equal values
        got64 = dense_of(tk, eng_bench, ids, oo, pad_id=P, **{**opt, "flags": opt["flags"] | I64})
        assert got64["dense"].dtype == np.int64 and np.array_equal(got64["dense"], got["dense"].astype(np.int64))
        assert np.array_equal(got64["lengths"], got["lengths"]) and got64["n_truncated"] == got["n_truncated"]
    # without MASK out.mask is NULL
    import torch
    d_ids, d_oo = on_device(ids, oo)
    res = eng_bench.dense_from_ids_device(d_ids.data_ptr(), d_oo.data_ptr(), len(counts), len(ids), max_length=16, pad_id=P, flags=0,
                                          stream=torch.cuda.current_stream().cuda_stream)
    assert res.mask_ptr is None and res.views()[1] is None


def test_encode_and_spans_outputs_outlive_a_dense_call(tk, eng_bench, bench_vocab):
    import torch
    docs = sweep_docs()
    data, offs = pack(docs)
    D = len(docs)
    d_bytes = torch.from_numpy(data).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    p_ids, p_oo, p_sp, n = eng_bench.encode_batch_device_spans(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), True, True, stream=stream)

    def snapshot():
        return (to_host(tk.DeviceView(p_ids, n, "<i4"), (n,), np.uint32).copy(), to_host(tk.DeviceView(p_oo, D + 1, "<i8"), (D + 1,), np.uint64).copy(),
                to_host(tk.DeviceView(p_sp, 2 * n, "<i4"), (2 * n,), np.uint32).copy())

    before = snapshot()
    eids, eoo = helpers.oracle_for(bench_vocab).encode_batch(data, offs, True, True, threads=8)
    assert np.array_equal(before[0], eids) and np.array_equal(before[1], eoo)
    for opt in (dict(max_length=128, flags=FIXED | MASK), dict(max_length=0, flags=I64 | MASK | PAD_LEFT)):
        res = eng_bench.dense_from_ids_device(p_ids, p_oo, D, n, pad_id=7, keep_head=1, keep_tail=1, stream=stream, **opt)
        assert len({res.ids_ptr, res.mask_ptr, res.lengths_ptr, p_ids, p_oo, p_sp}) == 6
        got = fetch(tk, res)
        after = snapshot()
        for a, b in zip(before, after):
            assert np.array_equal(a, b)
        assert_same(got, expected_dense(eids, eoo, opt["max_length"], 0, 7, 1, 1, opt["flags"]), opt)
    p_ids2, p_oo2, n2 = eng_bench.ragged_from_dense_device(res.ids_ptr, D, res.row_len, I64 | PAD_LEFT, res.lengths_ptr, 7, stream)
    after = snapshot()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert n2 == n and p_ids2 != p_ids
    assert np.array_equal(to_host(tk.DeviceView(p_ids2, n2, "<i4"), (n2,), np.uint32), eids)


def test_errors_and_empty_shapes(tk, test_vocab):
    import torch
    v = test_vocab
    eng = tk.Engine(v["tokens"], v["num_special"], v["bos"], v["eos"], device=0)
    stream = torch.cuda.current_stream().cuda_stream
    try:
        rows = [[1, 20, 21, 22, 23, 24, 2], [1, 30, 2], [], [1, 40, 41, 42, 2]]
        oo = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        ids = np.array([i for r in rows for i in r], np.uint32)
        d_ids, d_oo = on_device(ids, oo)
        good = eng.dense_from_ids_device(d_ids.data_ptr(), d_oo.data_ptr(), 4, len(ids), max_length=5, pad_id=9, keep_tail=1, flags=MASK, stream=stream)
        exp = expected_dense(ids, oo, 5, 0, 9, 0, 1, MASK)
        assert_same(fetch(tk, good), exp)
        bad = [dict(max_length=2, keep_tail=3), dict(max_length=2, keep_head=3, flags=TRUNC_LEFT), dict(max_length=0, flags=FIXED),
               dict(max_length=5, flags=64), dict(max_length=0xFFFFFFFF, flags=FIXED),            # a row of 2^31 elements or more
               dict(max_length=0x7FFFFFF0, multiple_of=0x80000000, flags=FIXED)]          # rounded up to 2^31
        for opt in bad:
            with pytest.raises(tk.TokenizerError) as e:
                eng.dense_from_ids_device(d_ids.data_ptr(), d_oo.data_ptr(), 4, len(ids), pad_id=9, stream=stream, **opt)
            assert e.value.code == tk.TK_ERR_INVALID_ARG, (opt, str(e.value))
            assert_same(fetch(tk, good), exp, ("the earlier result after", opt))
        # 64 rows of 2^31 - 16 elements: beyond 2^36 elements (refused before anything is allocated)
        z64 = torch.zeros(65, dtype=torch.int64, device="cuda")
        with pytest.raises(tk.TokenizerError) as e:
            eng.dense_from_ids_device(d_ids.data_ptr(), z64.data_ptr(), 64, 0, max_length=0x7FFFFFF0, pad_id=9, flags=FIXED, stream=stream)
        assert e.value.code == tk.TK_ERR_INVALID_ARG, str(e.value)
        assert_same(fetch(tk, good), exp, "the earlier result after the size error")
        # (the head is not looked at when truncating on the right, nor the tail on the left)
        eng.dense_from_ids_device(d_ids.data_ptr(), d_oo.data_ptr(), 4, len(ids), max_length=2, keep_head=3, pad_id=9, stream=stream)
        eng.dense_from_ids_device(d_ids.data_ptr(), d_oo.data_ptr(), 4, len(ids), max_length=2, keep_tail=3, pad_id=9, flags=TRUNC_LEFT, stream=stream)
        # the fused entries: BOS + EOS must fit
        data, offs = pack([b"hello world", b""])
        d_bytes, d_offs = torch.from_numpy(data).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda()
        for kw in (dict(max_length=1), dict(max_length=0, flags=FIXED)):
            with pytest.raises(tk.TokenizerError) as e:
                eng.encode_batch_device_dense(d_bytes.data_ptr(), d_offs.data_ptr(), 2, len(data), True, True, stream=stream, **kw)
            assert e.value.code == tk.TK_ERR_INVALID_ARG
            with pytest.raises(tk.TokenizerError) as e:
                eng.encode_batch_dense(data, offs, True, True, **kw)
            assert e.value.code == tk.TK_ERR_INVALID_ARG
        got = eng.encode_batch_dense(data, offs, True, True, max_length=2, pad_id=9, flags=MASK)
        assert got[0].tolist() == [[v["bos"], v["eos"]]] * 2 and eng.last_n_truncated == 1
        # D = 0
        for opt in (dict(max_length=0, flags=MASK), dict(max_length=6, flags=FIXED | MASK | I64), dict(max_length=0, multiple_of=8)):
            e0 = expected_dense([], [0], pad_id=9, **opt)
            assert_same(dense_of(tk, eng, np.zeros(0, np.uint32), np.zeros(1, np.int64), pad_id=9, **opt), e0, opt)
            dense, mask, lengths = eng.encode_batch_dense(np.zeros(0, np.uint8), np.zeros(1, np.uint64), True, True, pad_id=9, **opt)
            assert dense.shape == e0["dense"].shape and dense.dtype == e0["dense"].dtype and lengths.shape == (0,)
        # all-empty documents: L = 0 in the longest mode, rows of pads with FIXED
        z = np.zeros(6, np.int64)
        for opt in (dict(max_length=0, multiple_of=8, flags=MASK), dict(max_length=7, flags=MASK), dict(max_length=4, flags=FIXED | MASK | PAD_LEFT)):
            assert_same(dense_of(tk, eng, np.zeros(0, np.uint32), z, pad_id=9, **opt), expected_dense([], z, pad_id=9, **opt), opt)
        flat, roo = ragged_of(tk, eng, np.zeros((0, 5), np.int32), None, 9, False)
        assert len(flat) == 0 and roo.tolist() == [0]
        flat, roo = ragged_of(tk, eng, np.zeros((3, 0), np.int64), None, 9, True)
        assert len(flat) == 0 and roo.tolist() == [0, 0, 0, 0]
        flat, roo = ragged_of(tk, eng, np.full((3, 8), 9, np.int32), None, 9, False)
        assert len(flat) == 0 and roo.tolist() == [0, 0, 0, 0]
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
        for opt in (dict(max_length=64, flags=MASK), dict(max_length=0, multiple_of=8, flags=PAD_LEFT | I64 | MASK),
                    dict(max_length=33, flags=FIXED | TRUNC_LEFT)):
            calls0 = eng_bench.small_path_calls()
            dense, mask, lengths = eng_bench.encode_batch_dense(data, offs, True, True, pad_id=P, **opt)
            assert (eng_bench.small_path_calls() > calls0) == is_small
            n_trunc = eng_bench.last_n_truncated
            _, _, _, res = eng_bench.encode_batch_device_dense(d_bytes.data_ptr(), d_offs.data_ptr(), len(docs), len(data), True, True, pad_id=P,
                                                               stream=stream, **opt)
            dev = fetch(tk, res)
            assert_same({"dense": dense, "mask": mask, "lengths": lengths, "row_len": dense.shape[1], "n_truncated": n_trunc}, dev, opt)
    eids, eoo = helpers.oracle_for(bench_vocab).encode_batch(data, offs, True, True, threads=8)
    assert_same(dev, expected_dense(eids, eoo, 33, 0, P, 1, 1, FIXED | TRUNC_LEFT))


def test_inverse(tk, eng_bench, bench_vocab):
    docs = [x for x in sweep_docs() if len(x) < 70000]
    data, offs = pack(docs)
    P = 7
    eids, eoo = helpers.oracle_for(bench_vocab).encode_batch(data, offs, True, True, threads=8)
    for flags in (0, PAD_LEFT, I64, I64 | PAD_LEFT):
        for m in (0, 4):
            got = dense_of(tk, eng_bench, eids, eoo, max_length=0, multiple_of=m, pad_id=P, flags=flags)
            for lengths in (got["lengths"], None):
                flat, roo = ragged_of(tk, eng_bench, got["dense"], lengths, P, bool(flags & PAD_LEFT))
                assert np.array_equal(roo, eoo) and np.array_equal(flat, eids), (flags, m, lengths is None)
        # after truncation: what the restatement gives for the truncated tensor
        for T, extra in ((64, 0), (128, TRUNC_LEFT), (3, 0)):
            got = dense_of(tk, eng_bench, eids, eoo, max_length=T, pad_id=P, keep_head=1, keep_tail=1, flags=flags | extra)
            for lengths in (got["lengths"], None):
                flat, roo = ragged_of(tk, eng_bench, got["dense"], lengths, P, bool(flags & PAD_LEFT))
                eflat, eroo = expected_ragged(got["dense"], lengths, P, bool(flags & PAD_LEFT))
                assert np.array_equal(roo, eroo) and np.array_equal(flat, eflat), (flags, T, lengths is None)
    # rows that hold pad_id inside and at the unpadded end, lengths longer than the row (clamped)
    rng = np.random.default_rng(3)
    dense = rng.integers(0, 4, (300, 37)).astype(np.int32)
    for pad_left in (False, True):
        flat, roo = ragged_of(tk, eng_bench, dense, None, 0, pad_left)
        eflat, eroo = expected_ragged(dense, None, 0, pad_left)
        assert np.array_equal(roo, eroo) and np.array_equal(flat, eflat)
        lens = rng.integers(0, 50, 300)
        flat, roo = ragged_of(tk, eng_bench, dense, lens, 0, pad_left)
        eflat, eroo = expected_ragged(dense, np.minimum(lens, 37), 0, pad_left)
        assert np.array_equal(roo, eroo) and np.array_equal(flat, eflat)


def test_padded_round_trip_through_the_tokenizer(tk, bench_vocab):
    import torch
    t = tk.Tekkenizer.from_file(bench_vocab["path"], device=0)
    try:
        P = t.pad_id()
        docs = [x.decode("utf-8") for x in sweep_docs() if len(x) < 20000]
        for kw in (dict(), dict(padding_side="left", dtype="int32", pad_to_multiple_of=8), dict(return_tensors="np")):
            r = t.encode_batch_padded(docs, True, True, **kw)
            side = kw.get("padding_side", "right")
            assert t.decode_batch_padded(r["input_ids"], padding_side=side) == docs
            assert t.decode_batch_padded(r["input_ids"], r["lengths"], padding_side=side) == docs
        # truncated, ASCII documents (the cut falls on character boundaries): decode_batch of the kept ids, policy Keep
        data, offs = corpus.generate("ascii", 300, 512, seed=corpus.BASE_SEED + 3)
        adocs = [x.decode("ascii") for x in corpus.docs_of(data, offs)]
        ragged = t.encode_batch(adocs, True, True)
        for side in ("right", "left"):
            r = t.encode_batch_padded(adocs, True, True, max_length=40, truncation_side=side, padding_side=side)
            assert r["n_truncated"] > 0
            kept = [x if len(x) <= 40 else (x[:39] + x[-1:] if side == "right" else x[:1] + x[-39:]) for x in ragged]
            assert [row[m.bool()].tolist() for row, m in zip(r["input_ids"].cpu(), r["attention_mask"].cpu())] == kept
            want = t.decode_batch(kept, tk.SpecialTokenPolicy.Keep)
            assert t.decode_batch_padded(r["input_ids"], policy=tk.SpecialTokenPolicy.Keep, padding_side=side) == want
            assert t.decode_batch_padded(r["input_ids"], r["lengths"], tk.SpecialTokenPolicy.Keep, padding_side=side) == want
        # an id outside the vocabulary: the error names the row, as decode_batch
        bad = r["input_ids"].clone()
        bad[17, 0 if side == "right" else -1] = t.vocab_size() + 5
        with pytest.raises(tk.TokenizerError) as e:
            t.decode_batch_padded(bad, padding_side=side)
        assert e.value.bad_doc == 17
        assert P not in [i for x in ragged for i in x]
    finally:
        t.close()


def test_padded_tensors_dtype_shape_device_and_copy(tk, small_tok):
    import torch
    t = small_tok
    P = t.pad_id()
    docs = ["hello world", "", "hello", "world hello world"]
    for dtype, tdt in (("int64", torch.int64), ("int32", torch.int32)):
        r = t.encode_batch_padded(docs, True, True, max_length=6, padding="max_length", dtype=dtype)
        ids, mask, lengths = r["input_ids"], r["attention_mask"], r["lengths"]
        assert ids.dtype == tdt and mask.dtype == torch.uint8 and lengths.dtype == torch.int32
        assert tuple(ids.shape) == (4, 6) and tuple(mask.shape) == (4, 6) and tuple(lengths.shape) == (4,)
        assert ids.is_cuda and mask.is_cuda and lengths.is_cuda and ids.device.index == 0 and ids.is_contiguous()
        keep = ids.clone()
        # copy=True results survive the next call on the tokenizer
        r2 = t.encode_batch_padded(["world"] * 9, True, True, max_length=6, padding="max_length", dtype=dtype)
        assert torch.equal(ids, keep) and r2["input_ids"].tolist() == [[1, 267, 2, P, P, P]] * 9
        assert ids[0].tolist() == [1, 266, 42, 129, 121, 2] and ids[1].tolist() == [1, 2, P, P, P, P] and lengths.tolist() == [6, 2, 3, 6]
        assert r["n_truncated"] == 2
        v = t.encode_batch_padded(docs, True, True, max_length=6, padding="max_length", dtype=dtype, copy=False)
        assert torch.equal(v["input_ids"], keep)            # a view of the context's buffer, read before the next call
    r = t.encode_batch_padded(docs, return_mask=False, return_tensors="np")
    assert r["attention_mask"] is None and r["input_ids"].dtype == np.int64 and r["input_ids"].shape == (4, 13)
    r = t.encode_batch_padded([], True, True)
    assert tuple(r["input_ids"].shape) == (0, 0) and r["n_truncated"] == 0
    r = t.encode_batch_padded(["", ""])
    assert tuple(r["input_ids"].shape) == (2, 0) and r["lengths"].tolist() == [0, 0]


def torch_dense_rows(ids, oo, r0, r1, L, lim, h, t, pad_id, trunc_left, pad_left, dtype):
    """The definition as a torch composition over rows [r0, r1) of the ragged device views: index arithmetic + torch.where."""
    import torch
    start = oo[r0:r1]
    n = oo[r0 + 1:r1 + 1] - start
    k = torch.clamp(n, max=lim) if lim else n
    col = torch.arange(L, device=ids.device, dtype=torch.int64)[None, :]
    j = col - ((L - k)[:, None] if pad_left else 0)
    kept = (j >= 0) & (j < k[:, None])
    split = h if trunc_left else lim - t
    src = torch.where(j < split, j, j + (n - k)[:, None]) if lim else j
    idx = torch.where(kept, start[:, None] + src, torch.zeros_like(src))
    dense = torch.where(kept, ids[idx].to(dtype), torch.full((), pad_id, dtype=dtype, device=ids.device))
    return dense, kept.to(torch.uint8), k.to(torch.int32), int((n > lim).sum()) if lim else 0


@pytest.mark.parametrize("shape", ["c2", "zipf"])
def test_full_size_against_the_torch_composition(tk, eng_bench, shape):
    import torch
    P = 7
    if shape == "c2":
        n_docs, opt = 1_000_000, dict(max_length=128, flags=FIXED | MASK)
        data, offs = corpus.generate("ascii", n_docs, 512, seed=corpus.BASE_SEED + 1)
    else:
        n_docs, opt = 500_000, dict(max_length=512, multiple_of=64, flags=MASK)
        data, offs = corpus.generate("zipf", n_docs, 0, seed=corpus.BASE_SEED + 1)
    d_bytes = torch.from_numpy(data).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    for i64 in (0, I64):
        flags = opt["flags"] | i64
        p_ids, p_oo, n, res = eng_bench.encode_batch_device_dense(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, len(data), True, True,
                                                                  max_length=opt["max_length"], multiple_of=opt.get("multiple_of", 0), pad_id=P,
                                                                  flags=flags, stream=stream)
        ids = torch.as_tensor(tk.DeviceView(p_ids, n, "<i4"), device="cuda")
        oo = torch.as_tensor(tk.DeviceView(p_oo, n_docs + 1, "<i8"), device="cuda")
        v_ids, v_mask, v_len = res.views()
        dense, mask, lengths = (torch.as_tensor(x, device="cuda") for x in (v_ids, v_mask, v_len))
        L, T = res.row_len, opt["max_length"]
        assert res.n_docs == n_docs and tuple(dense.shape) == (n_docs, L) and dense.dtype == (torch.int64 if i64 else torch.int32)
        longest = int((oo[1:] - oo[:-1]).max())
        assert L == (T if flags & FIXED else (min(longest, T) + 63) // 64 * 64)
        n_trunc, rows = 0, max(1, (64 << 20) // L)                     # (the int64 index of a chunk stays at 512 MB)
        for r0 in range(0, n_docs, rows):
            r1 = min(r0 + rows, n_docs)
            e_dense, e_mask, e_len, e_trunc = torch_dense_rows(ids, oo, r0, r1, L, T, 1, 1, P, False, False, dense.dtype)
            assert torch.equal(dense[r0:r1], e_dense), (shape, i64, r0)
            assert torch.equal(mask[r0:r1], e_mask) and torch.equal(lengths[r0:r1], e_len), (shape, i64, r0)
            n_trunc += e_trunc
            del e_dense, e_mask, e_len
        assert res.n_truncated == n_trunc and n_trunc < n_docs and (shape == "c2" or n_trunc > 0)
        # and back: the kept ids of every row, with the lengths and with the pad trim
        for d_len in (res.lengths_ptr, 0):
            p_r, p_ro, n_r = eng_bench.ragged_from_dense_device(res.ids_ptr, n_docs, L, i64, d_len, P, stream)
            r_oo = torch.as_tensor(tk.DeviceView(p_ro, n_docs + 1, "<i8"), device="cuda")
            r_ids = torch.as_tensor(tk.DeviceView(p_r, n_r, "<i4"), device="cuda")
            assert torch.equal(r_oo[1:] - r_oo[:-1], lengths.to(torch.int64)) and n_r == int(lengths.sum())
            assert torch.equal(r_ids.to(dense.dtype), dense[mask.bool()])
