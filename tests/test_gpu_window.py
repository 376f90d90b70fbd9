"""Overlapping windows for long documents on the GPU (include/tekken_hip.h tk_window_from_ids_device and the entries around it,
csrc/tk_window.hip) against the plain-loop restatement of the definition in tests/test_window_cpu.py -- element by element over
every output, never through a sum."""
import json

import numpy as np
import pytest

import helpers
from helpers import dev, on_device, to_host
from test_gpu_spans import pack, sweep_docs
from test_window_cpu import FIXED, I64, MASK, SPANS, expected_windows, refused_cases

pytestmark = pytest.mark.gpu

ARRAYS = ("input_ids", "mask", "lengths", "window_doc", "window_start", "doc_windows", "spans")
COUNTS = ("n_windows", "n_split", "row_len")


def fetch(res):
    """WindowResult -> dict like expected_windows's."""
    dt = np.int64 if res.typestr == "<i8" else np.int32
    W, L = res.n_windows, res.row_len
    v = res.views()
    return {"input_ids": to_host(v[0], (W, L), dt), "mask": to_host(v[1], (W, L), np.uint8), "lengths": to_host(v[2], (W,), np.uint32),
            "window_doc": to_host(v[3], (W,), np.uint32), "window_start": to_host(v[4], (W,), np.uint32),
            "doc_windows": to_host(v[5], (res.n_docs + 1,), np.uint64), "spans": to_host(v[6], (W, L, 2), np.uint32),
            "n_windows": W, "n_split": res.n_split, "row_len": L}


def assert_same(got, exp, what=""):
    helpers.assert_same(got, exp, what, COUNTS, ARRAYS)


def windows_of(eng, d_ids, d_oo, n_ids, T, s, h, t, m, pad_id, flags, d_spans=None):
    import torch
    res = eng.window_from_ids_device(d_ids.data_ptr(), d_oo.data_ptr(), d_oo.numel() - 1, n_ids, T, s, m, pad_id, h, t, flags,
                                     d_spans.data_ptr() if d_spans is not None else 0, torch.cuda.current_stream().cuda_stream)
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


def test_known_answer_small_vocab(tk, small_tok):
    import torch
    t = small_tok
    P = t.pad_id()
    assert P == 3
    # "hello world" with BOS / EOS: [1, 266, 42, 129, 121, 124, 118, 110, 2] (tests/test_gpu_spans.py), 9 ids, a body of 7; c = 4, step 3
    docs = ["hello world", "", "hello"]
    r = t.encode_batch_windows(docs, max_length=6, stride=1, add_bos=True, add_eos=True, return_offsets_mapping=True)
    assert r["input_ids"].tolist() == [[1, 266, 42, 129, 121, 2], [1, 121, 124, 118, 110, 2], [1, 2, P, P, P, P], [1, 266, 2, P, P, P]]
    assert r["attention_mask"].tolist() == [[1] * 6, [1] * 6, [1, 1, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0]]
    assert r["lengths"].tolist() == [6, 6, 2, 3] and r["overflow_to_sample_mapping"].tolist() == [0, 0, 1, 2]
    assert r["window_start"].tolist() == [1, 4, 1, 1] and r["doc_windows"].tolist() == [0, 2, 3, 4]
    assert (r["n_windows"], r["n_split"]) == (4, 1)
    assert r["offset_mapping"].tolist() == [[[0, 0], [0, 5], [5, 6], [6, 7], [7, 8], [11, 11]], [[0, 0], [7, 8], [8, 9], [9, 10], [10, 11], [11, 11]],
                                            [[0, 0]] * 6, [[0, 0], [0, 5], [5, 5], [0, 0], [0, 0], [0, 0]]]
    assert isinstance(r["input_ids"], torch.Tensor) and r["input_ids"].dtype == torch.int64
    # without BOS / EOS: [266, 42, 129, 121, 124, 118, 110] at c = 6, step 5; longest rows, int32, numpy
    r = t.encode_batch_windows(docs, max_length=6, stride=1, padding="longest", dtype="int32", return_tensors="np", pad_id=77)
    assert r["input_ids"].tolist() == [[266, 42, 129, 121, 124, 118], [118, 110, 77, 77, 77, 77], [77] * 6, [266, 77, 77, 77, 77, 77]]
    assert r["input_ids"].dtype == np.int32 and r["offset_mapping"] is None
    assert r["lengths"].tolist() == [6, 2, 0, 1] and r["window_start"].tolist() == [0, 5, 0, 0] and r["doc_windows"].tolist() == [0, 2, 3, 4]
    r = t.encode_batch_windows(["hello", ""], max_length=6, padding="longest", pad_to_multiple_of=4, return_attention_mask=False)
    assert r["input_ids"].tolist() == [[266, P, P, P], [P] * 4] and r["attention_mask"] is None and r["n_split"] == 0


# ---- made-up ids through tk_window_from_ids_device ----

def made_up(T):
    """8 600 documents: 600 with up to 299 ids (some empty, the first 3 and last 2 among them; one of 50 001 ids, one of exactly
    T and one of T + 1), a run of 5 000 empty ones and a block of 3 000 one-id ones."""
    rng = np.random.default_rng(31)
    counts = rng.integers(0, 300, 600)
    pool = np.setdiff1d(np.arange(600), [0, 1, 2, 3, 4, 333, 334, 335, 598, 599])
    counts[rng.choice(pool, 60, replace=False)] = 0
    counts[:3] = 0
    counts[-2:] = 0
    counts[3], counts[4] = T, T + 1
    counts[333], counts[334], counts[335] = 50_001, 0, 4 * T + 3       # an empty document between two split ones
    counts = np.concatenate([counts[:200], np.zeros(5000, np.int64), counts[200:500], np.ones(3000, np.int64), counts[500:]])
    oo = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ids = rng.integers(0, 2**31 - 1, int(oo[-1])).astype(np.uint32)
    return ids, oo


def short_docs():
    """Documents of at most 41 ids: the longest-row mode below T."""
    rng = np.random.default_rng(32)
    counts = rng.integers(0, 42, 300)
    counts[7] = 41
    oo = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return rng.integers(0, 2**31 - 1, int(oo[-1])).astype(np.uint32), oo


SHAPES = ((4, 0, 0, 0), (4, 1, 1, 1), (5, 2, 1, 1), (8, 5, 1, 1), (64, 16, 1, 1), (127, 0, 2, 3), (128, 32, 1, 1), (2048, 128, 1, 1))
P_MADE_UP = 5
_cases = {}


def case(shape, m, fixed=True, short=False):
    """(ids, oo, expected_windows of them) of one shape: computed once, shared, never changed."""
    key = (shape, m, fixed, short)
    if key not in _cases:
        T, s, h, t = shape
        ids, oo = short_docs() if short else made_up(T)
        _cases[key] = (ids, oo, expected_windows(ids, oo, T, s, h, t, m, P_MADE_UP, MASK | (FIXED if fixed else 0)))
    return _cases[key]


def test_the_case_set_holds_what_it_is_for():
    """From expected_windows's results alone: the properties the kernels' branches need are in the made-up cases."""
    seen = set()
    for shape in SHAPES:
        T, s, h, t = shape
        c = T - h - t
        ids, oo, e = case(shape, 0)
        dw, lens, wd = e["doc_windows"].astype(np.int64), e["lengths"].astype(np.int64), e["window_doc"]
        w = np.diff(dw)
        n = np.diff(oo)
        run, longest_run = 0, 0
        for x in w.tolist():
            run = run + 1 if x == 1 else 0
            longest_run = max(longest_run, run)
        if longest_run > 4096:
            seen.add("a run of more than 4 096 consecutive single-window documents")
        if w.max() > 4096:
            seen.add("a document with more than 4 096 windows")
        split = np.nonzero(w > 1)[0]
        last_body = lens[dw[split + 1] - 1] - h - t
        if np.any(last_body < c):
            seen.add("a last window shorter than c")
        if np.any(last_body == c):
            seen.add("a last window of exactly c")
        if np.any((w[:-2] > 1) & (n[1:-1] == 0) & (w[2:] > 1)):
            seen.add("an empty document between split ones")
        if e["row_len"] % 4 != 0:
            seen.add("L % 4 != 0")
        assert w[n == T].tolist() == [1] * int(np.sum(n == T)) and np.sum(n == T) >= 1 and np.all(w[n == T + 1] == 2) and np.sum(n == T + 1) >= 1
        assert np.array_equal(wd, np.repeat(np.arange(len(w)), w))
    assert seen == {"a run of more than 4 096 consecutive single-window documents", "a document with more than 4 096 windows",
                    "a last window shorter than c", "a last window of exactly c", "an empty document between split ones", "L % 4 != 0"}
    assert case((64, 16, 1, 1), 0, fixed=False, short=True)[2]["row_len"] == 41                          # below T: the longest document
    assert case((64, 16, 1, 1), 64, fixed=False, short=True)[2]["row_len"] == 64


def variants(eng, d_ids, d_oo, n_ids, shape, m, flags, got, what):
    """int64 equals int32 value for value; without the mask its pointer is NULL and the rest is unchanged."""
    T, s, h, t = shape
    _, got64 = windows_of(eng, d_ids, d_oo, n_ids, T, s, h, t, m, P_MADE_UP, flags | I64)
    assert got64["input_ids"].dtype == np.int64
    assert_same({**got64, "input_ids": got64["input_ids"].astype(np.int32)}, got, (what, "int64"))
    for f in (flags & ~MASK, (flags & ~MASK) | I64):
        res1, got1 = windows_of(eng, d_ids, d_oo, n_ids, T, s, h, t, m, P_MADE_UP, f)
        assert res1.mask_ptr is None and got1["mask"] is None
        assert_same({**got1, "input_ids": got1["input_ids"].astype(np.int32)}, {**got, "mask": None}, (what, "without the mask", f))


@pytest.mark.parametrize("shape", SHAPES)
def test_from_ids_on_ids_encode_never_produced(tk, eng_bench, shape):
    T, s, h, t = shape
    for m in (0, 64):
        ids, oo, exp = case(shape, m)
        d_ids, d_oo = on_device(ids, oo)
        for fixed in (True, False):                     # (a document of 50 001 ids: the longest-row mode gives the same rows)
            flags = MASK | (FIXED if fixed else 0)
            _, got = windows_of(eng_bench, d_ids, d_oo, len(ids), T, s, h, t, m, P_MADE_UP, flags)
            assert_same(got, exp, (shape, m, fixed))
        variants(eng_bench, d_ids, d_oo, len(ids), shape, m, flags, got, (shape, m))
    if T >= 64:                                         # every document below T: L is the longest document, then rounded
        for m in (0, 64):
            ids, oo, exp = case(shape, m, fixed=False, short=True)
            d_ids, d_oo = on_device(ids, oo)
            _, got = windows_of(eng_bench, d_ids, d_oo, len(ids), T, s, h, t, m, P_MADE_UP, MASK)
            assert_same(got, exp, (shape, m, "short documents"))
            variants(eng_bench, d_ids, d_oo, len(ids), shape, m, MASK, got, (shape, m, "short documents"))


@pytest.mark.parametrize("shape", [(5, 2, 1, 1), (8, 5, 1, 1), (64, 16, 1, 1), (127, 0, 2, 3)])
def test_spans_output_on_made_up_spans(tk, eng_bench, shape):
    T, s, h, t = shape
    ids, oo = made_up(T)
    g = np.arange(len(ids), dtype=np.uint64)
    sp = np.stack([(g * 2 + 1) & 0xFFFFFFFF, (g * 3 + 7) & 0xFFFFFFFF], axis=1).astype(np.uint32)   # index-derived: a wrong source index shows
    d_ids, d_oo = on_device(ids, oo)
    d_sp = dev(sp.reshape(-1), np.uint32)
    for m, flags in ((0, FIXED | SPANS | MASK), (4, SPANS | I64)):
        exp = expected_windows(ids, oo, T, s, h, t, m, P_MADE_UP, flags, sp)
        res, got = windows_of(eng_bench, d_ids, d_oo, len(ids), T, s, h, t, m, P_MADE_UP, flags, d_sp)
        assert res.spans_ptr is not None
        assert_same(got, exp, (shape, m, flags))


def long_row_docs():
    """(ids, oo, spans) of 14 documents around 9 001 ids -- shorter, exactly, one more, more than twice as many --, about 93 000
    ids, with made-up spans."""
    rng = np.random.default_rng(53)
    n = [3000, 20000, 0, 5, 9000, 9001, 10, 9002, 20000, 120, 4500, 8998, 1, 1]
    oo = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    ids = rng.integers(0, 2**31 - 1, int(oo[-1])).astype(np.uint32)
    g = np.arange(len(ids), dtype=np.uint64)
    sp = np.stack([(g * 2 + 1) & 0xFFFFFFFF, (g * 3 + 7) & 0xFFFFFFFF], axis=1).astype(np.uint32)   # index-derived: a wrong source index shows
    return ids, oo, sp


def test_row_longer_than_a_block_tile(tk, eng_bench):
    """T = 9 001: the units of one row are split over blockIdx.y, element by element (L = 9 001) and in units of 4 (L = 9 004)."""
    T, s = 9001, 100
    ids, oo, sp = long_row_docs()
    d_ids, d_oo = on_device(ids, oo)
    d_sp = dev(sp.reshape(-1), np.uint32)
    for m in (0, 4):
        for h, t in ((2, 3), (3, 2)):
            flags = FIXED | MASK | SPANS
            exp = expected_windows(ids, oo, T, s, h, t, m, P_MADE_UP, flags, sp)
            assert exp["row_len"] == T + 3 * (m == 4) and exp["lengths"].max() == T and exp["n_split"] > 0
            for fl in (flags, flags | I64):
                _, got = windows_of(eng_bench, d_ids, d_oo, len(ids), T, s, h, t, m, P_MADE_UP, fl, d_sp)
                assert_same({**got, "input_ids": got["input_ids"].astype(np.int32)}, exp, (m, h, t, fl))


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
            # the spans of this encoding, from tk_token_spans_device's own buffer
            p_ids, p_oo, p_sp, n = eng.encode_batch_device_spans(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), bos, eos, stream=stream)
            sp = to_host(tk.DeviceView(p_sp, 2 * n, "<i4"), (2 * n,), np.uint32).reshape(-1, 2).copy()
            for j, T in enumerate((64, 512, 2048)):
                flags = MASK | (I64 if (i + j) & 1 else 0) | (FIXED if j != 1 else 0) | (SPANS if j == i % 3 else 0)
                stride = (16, 128, 0)[j]
                p_ids, p_oo, n_ids, res = eng.encode_batch_device_window(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), T, stride, bos, eos,
                                                                         pad_id=P, flags=flags, checks=tk.CHECK_OFFSETS, stream=stream)
                ids = to_host(tk.DeviceView(p_ids, n_ids, "<i4"), (n_ids,), np.uint32)
                oo = to_host(tk.DeviceView(p_oo, D + 1, "<i8"), (D + 1,), np.uint64)
                assert np.array_equal(oo, eoo) and np.array_equal(ids, eids)
                assert_same(fetch(res), expected_windows(eids, eoo, T, stride, int(bos), int(eos), 0, P, flags, sp), (vname, bos, eos, T))
    finally:
        eng.close()


def host_as_expected(host):
    return {**host, "row_len": host["input_ids"].shape[1]}


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
        for T, s, m, flags in ((64, 16, 0, FIXED | MASK), (30, 7, 4, I64 | SPANS), (2048, 128, 0, FIXED | I64 | MASK | SPANS)):
            calls0 = eng_bench.small_path_calls()
            host = eng_bench.encode_batch_window(data, offs, T, s, True, True, multiple_of=m, pad_id=P, flags=flags)
            assert (eng_bench.small_path_calls() > calls0) == is_small
            _, _, _, res = eng_bench.encode_batch_device_window(d_bytes.data_ptr(), d_offs.data_ptr(), len(docs), len(data), T, s, True, True,
                                                                multiple_of=m, pad_id=P, flags=flags, stream=stream)
            dv = fetch(res)
            assert_same(host_as_expected(host), dv, (is_small, T, flags))
    eids, eoo = helpers.oracle_for(bench_vocab).encode_batch(data, offs, True, True, threads=8)
    exp = expected_windows(eids, eoo, 2048, 128, 1, 1, 0, P, FIXED | I64 | MASK)
    assert_same({**dv, "spans": None}, exp)


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
    pk = eng.seqpack_from_ids_device(p_ids, p_oo, D, n, 512, 7, 2 | 4 | 8, stream)                      # positions, segments, cu_seqlens
    R = pk.n_rows

    def snapshot():
        return (to_host(tk.DeviceView(p_ids, n, "<i4"), (n,), np.uint32).copy(), to_host(tk.DeviceView(p_oo, D + 1, "<i8"), (D + 1,), np.uint64).copy(),
                to_host(tk.DeviceView(p_sp, 2 * n, "<i4"), (2 * n,), np.uint32).copy(),
                to_host(tk.DeviceView(dn.ids_ptr, (D, 128), "<i4"), (D, 128), np.int32).copy(),
                to_host(tk.DeviceView(dn.mask_ptr, (D, 128), "|u1"), (D, 128), np.uint8).copy(),
                to_host(tk.DeviceView(dn.lengths_ptr, D, "<i4"), (D,), np.uint32).copy(),
                to_host(tk.DeviceView(pk.input_ids_ptr, (R, 512), "<i4"), (R, 512), np.int32).copy(),
                to_host(tk.DeviceView(pk.position_ids_ptr, (R, 512), "<i4"), (R, 512), np.int32).copy(),
                to_host(tk.DeviceView(pk.segment_ids_ptr, (R, 512), "<i4"), (R, 512), np.int32).copy(),
                to_host(tk.DeviceView(pk.cu_seqlens_ptr, pk.n_segments + 1, "<i4"), (pk.n_segments + 1,), np.int32).copy())

    before = snapshot()
    eids, eoo = helpers.oracle_for(bench_vocab).encode_batch(data, offs, True, True, threads=8)
    assert np.array_equal(before[0], eids) and np.array_equal(before[1], eoo)
    sp = before[2].reshape(-1, 2)
    flags = FIXED | MASK | SPANS
    good = eng.window_from_ids_device(p_ids, p_oo, D, n, 512, 128, 0, 7, 1, 1, flags, p_sp, stream)
    ptrs = {good.input_ids_ptr, good.mask_ptr, good.spans_ptr, good.lengths_ptr, good.window_doc_ptr, good.window_start_ptr, good.doc_windows_ptr,
            pk.input_ids_ptr, pk.position_ids_ptr, pk.segment_ids_ptr, pk.cu_seqlens_ptr, dn.ids_ptr, dn.mask_ptr, dn.lengths_ptr, p_ids, p_oo, p_sp}
    assert len(ptrs) == 17 and None not in ptrs and 0 not in ptrs
    exp = expected_windows(eids, eoo, 512, 128, 1, 1, 0, 7, flags, sp)
    assert_same(fetch(good), exp)
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a, b)
    # every case of step 8: refused, and the first window result stays readable (the offsets of the cases are read, never their ids)
    for what, _, oo, T, s, h, t, m, fl, _ in refused_cases():
        d_oo = dev(np.array(oo, np.uint64), np.uint64)
        real = len(oo) == D + 1 or what == "ids without a document"
        with pytest.raises(tk.TokenizerError) as e:
            eng.window_from_ids_device(p_ids, p_oo if real else d_oo.data_ptr(), 0 if what == "ids without a document" else len(oo) - 1,
                                       n if real else int(oo[-1]), T, s, m, 7, h, t, fl, 0, stream)
        assert e.value.code == tk.TK_ERR_INVALID_ARG, (what, str(e.value))
        assert_same(fetch(good), exp, ("the earlier result after", what))
    for bos, eos, T, s in ((True, True, 2, 0), (True, False, 1, 0), (True, True, 8, 6), (False, False, 0, 0)):
        with pytest.raises(tk.TokenizerError) as e:
            eng.encode_batch_device_window(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), T, s, bos, eos, stream=stream)
        assert e.value.code == tk.TK_ERR_INVALID_ARG, (bos, eos, T, s)
    with pytest.raises(tk.TokenizerError) as e:
        eng.encode_batch_window(data, offs, 64, 0, True, True, flags=64)
    assert e.value.code == tk.TK_ERR_INVALID_ARG
    assert_same(fetch(good), exp, "the earlier result after the fused entries' errors")


def test_empty_shapes(tk, eng_bench):
    eng = eng_bench
    z1 = np.zeros(1, np.int64)
    for flags in (MASK, FIXED | I64 | MASK, FIXED, 0):
        for m in (0, 8):
            for oo in (z1, np.zeros(6, np.int64)):                   # D = 0; all-empty documents
                d_ids, d_oo = on_device(np.zeros(0, np.uint32), oo)
                _, got = windows_of(eng, d_ids, d_oo, 0, 6, 1, 1, 1, m, 9, flags)
                assert_same(got, expected_windows([], oo, 6, 1, 1, 1, m, 9, flags), (flags, m, len(oo)))
        host = eng.encode_batch_window(np.zeros(0, np.uint8), np.zeros(1, np.uint64), 6, 1, True, True, pad_id=9, flags=flags)
        assert_same(host_as_expected(host), expected_windows([], z1, 6, 1, 1, 1, 0, 9, flags), ("host", flags))
    rows = [[1] + list(range(20, 30)) + [2], [1, 30, 2], [], [1] + list(range(40, 45)) + [2]]           # the worked example
    oo = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    ids = np.array([i for r in rows for i in r], np.uint32)
    d_ids, d_oo = on_device(ids, oo)
    res, got = windows_of(eng, d_ids, d_oo, len(ids), 6, 1, 1, 1, 0, 9, FIXED | MASK)
    assert got["input_ids"].tolist() == [[1, 20, 21, 22, 23, 2], [1, 23, 24, 25, 26, 2], [1, 26, 27, 28, 29, 2], [1, 30, 2, 9, 9, 9], [9] * 6,
                                         [1, 40, 41, 42, 43, 2], [1, 43, 44, 2, 9, 9]]
    assert got["window_doc"].tolist() == [0, 0, 0, 1, 2, 3, 3] and got["window_start"].tolist() == [1, 4, 7, 1, 0, 1, 4]
    assert got["lengths"].tolist() == [6, 6, 6, 3, 0, 6, 4] and got["doc_windows"].tolist() == [0, 3, 4, 5, 7] and res.n_split == 2
    for T, s, h, t, m, flags in ((4, 0, 0, 0, 0, FIXED), (4, 2, 0, 0, 0, MASK), (5, 2, 1, 1, 0, FIXED | I64), (8, 0, 2, 3, 0, MASK), (8, 0, 2, 3, 16, 0),
                                 (12, 3, 1, 1, 0, 0), (13, 3, 1, 1, 0, MASK), (3, 0, 1, 1, 0, FIXED | MASK), (1, 0, 0, 0, 0, MASK)):
        _, got = windows_of(eng, d_ids, d_oo, len(ids), T, s, h, t, m, 9, flags)
        assert_same(got, expected_windows(ids, oo, T, s, h, t, m, 9, flags), (T, s, h, t, m, flags))


def test_tensors_from_encode_batch_windows(tk, bench_vocab):
    import torch
    t = tk.Tekkenizer.from_file(bench_vocab["path"], device=0)
    try:
        docs = [x.decode("utf-8") for x in sweep_docs()[:40]] + ["", "tail"]
        lists = t.encode_batch(docs, True, True)
        ids = np.array([i for row in lists for i in row], np.int64)
        oo = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
        keys = {"input_ids", "attention_mask", "lengths", "overflow_to_sample_mapping", "window_start", "doc_windows", "offset_mapping",
                "n_windows", "n_split"}
        names = {"input_ids": "input_ids", "attention_mask": "mask", "lengths": "lengths", "overflow_to_sample_mapping": "window_doc",
                 "window_start": "window_start", "doc_windows": "doc_windows"}
        for dtype, tdt in (("int64", torch.int64), ("int32", torch.int32)):
            exp = expected_windows(ids, oo, 64, 16, 1, 1, 0, t.pad_id(), FIXED | MASK | (I64 if dtype == "int64" else 0))
            W = exp["n_windows"]
            assert exp["n_split"] > 0
            r = t.encode_batch_windows(docs, 64, 16, True, True, dtype=dtype)
            assert set(r) == keys and r["offset_mapping"] is None and (r["n_windows"], r["n_split"]) == (W, exp["n_split"])
            assert r["input_ids"].dtype == tdt and tuple(r["input_ids"].shape) == (W, 64) and r["input_ids"].is_cuda and r["input_ids"].is_contiguous()
            assert r["attention_mask"].dtype == torch.uint8 and tuple(r["attention_mask"].shape) == (W, 64) and r["attention_mask"].is_cuda
            for k in ("lengths", "overflow_to_sample_mapping", "window_start"):
                assert r[k].dtype == torch.int32 and tuple(r[k].shape) == (W,) and r[k].is_cuda, k
            assert r["doc_windows"].dtype == torch.int64 and tuple(r["doc_windows"].shape) == (len(docs) + 1,) and r["doc_windows"].is_cuda
            keep = {k: r[k].cpu().numpy().copy() for k in names}
            t.encode_batch_windows(["something else entirely"] * 300, 8, 2, dtype=dtype)      # copy=True survives the next call
            for k, e in names.items():
                assert np.array_equal(r[k].cpu().numpy(), keep[k]), k
                assert np.array_equal(keep[k], exp[e].astype(keep[k].dtype)), k
            n = t.encode_batch_windows(docs, 64, 16, True, True, dtype=dtype, return_tensors="np")
            for k, e in names.items():
                assert np.array_equal(n[k], exp[e].astype(n[k].dtype)) and n[k].shape == exp[e].shape, k
        r = t.encode_batch_windows(docs, 64, 16, True, True, padding="longest", pad_to_multiple_of=48, return_attention_mask=False,
                                   return_offsets_mapping=True, copy=False)
        assert r["attention_mask"] is None and tuple(r["input_ids"].shape) == (W, 96)
        assert r["offset_mapping"].dtype == torch.int32 and tuple(r["offset_mapping"].shape) == (W, 96, 2) and r["offset_mapping"].is_cuda
        assert np.array_equal(r["input_ids"][:, :64].cpu().numpy(), exp["input_ids"].astype(np.int64))
        with pytest.raises(tk.TokenizerError) as e:
            t.encode_batch_windows(docs, 0)
        assert e.value.code == tk.TK_ERR_INVALID_ARG
        with pytest.raises(tk.TokenizerError) as e:
            t.encode_batch_windows(docs, 2, 0, True, True)
        assert e.value.code == tk.TK_ERR_INVALID_ARG
        with pytest.raises(tk.TokenizerError) as e:
            t.encode_batch_windows(docs, 16, dtype="int16")
        assert e.value.code == tk.TK_ERR_INVALID_ARG
    finally:
        t.close()
