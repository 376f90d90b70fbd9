"""Whole documents packed into rows without cutting them on the GPU (include/tekken_hip.h tk_rowfit_from_ids_device and the
entries around it, csrc/tk_rowfit.hip) against the plain-loop restatement of the definition in tests/test_rowfit_cpu.py --
element by element over every output, never through a sum."""
import itertools
import json

import numpy as np
import pytest

import helpers
from helpers import dev, on_device, to_host
from test_gpu_spans import pack, sweep_docs
from test_rowfit_cpu import ALL, CU_SEQLENS, DOC_START, I64, IGN, LABELS, POSITIONS, SEGMENTS, expected_rowfit, random_lengths

pytestmark = pytest.mark.gpu

TENSORS = ("input_ids", "labels", "position_ids", "segment_ids", "cu_seqlens", "doc_start")
COUNTS = ("n_rows", "n_segments", "max_seqlen", "n_truncated", "n_pad")
P = 5            # the pad id of the made-up cases


def fetch(res):
    """RowfitResult -> dict like expected_rowfit's."""
    dt = np.int64 if res.typestr == "<i8" else np.int32
    shape = (res.n_rows, res.row_len)
    v = res.views()
    out = {"input_ids": to_host(v[0], shape, dt), "labels": to_host(v[1], shape, np.int32), "position_ids": to_host(v[2], shape, dt),
           "segment_ids": to_host(v[3], shape, dt), "cu_seqlens": to_host(v[4], (res.n_segments + 1,), np.int32),
           "doc_start": to_host(v[5], (res.n_docs,), np.uint64)}
    out.update({k: getattr(res, k) for k in COUNTS})
    return out


def assert_same(got, exp, what=""):
    helpers.assert_same(got, exp, what, COUNTS, TENSORS)


def ragged_of(lengths, seed=0):
    """Made-up ids (none is the pad id) and labels (negative values among them, none is the ignore index) of the given lengths."""
    rng = np.random.default_rng(1000 + seed)
    oo = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = int(oo[-1])
    ids = rng.integers(6, 2**31 - 1, n).astype(np.uint32)
    lab = rng.integers(-2**31, 2**31 - 1, n).astype(np.int32)
    lab[lab == IGN] = 0
    return ids, oo, lab


def fit_of(eng, ids, oo, lab, L, keep_tail, flags):
    import torch
    d_ids, d_oo = on_device(ids, oo)
    d_lab = torch.from_numpy(np.ascontiguousarray(lab if len(lab) else np.zeros(1, np.int32), np.int32)).cuda() if lab is not None else None
    res = eng.rowfit_from_ids_device(d_ids.data_ptr(), d_oo.data_ptr(), len(oo) - 1, len(ids), L, P, keep_tail, flags,
                                     d_lab.data_ptr() if d_lab is not None else 0, IGN, torch.cuda.current_stream().cuda_stream)
    return res, fetch(res)


def check_case(eng, lengths, L, keep_tail=0, seed=0, what=""):
    """Both element types against the definition; -> the expected result (of int32)."""
    ids, oo, lab = ragged_of(lengths, seed)
    exp = expected_rowfit(ids, oo, lab, L, P, IGN, keep_tail, ALL)
    _, got = fit_of(eng, ids, oo, lab, L, keep_tail, ALL)
    assert_same(got, exp, (what, L, keep_tail))
    _, got64 = fit_of(eng, ids, oo, lab, L, keep_tail, ALL | I64)        # int64 equals int32 value for value; labels stay int32
    for k in ("input_ids", "position_ids", "segment_ids"):
        assert got64[k].dtype == np.int64 and np.array_equal(got64[k], got[k].astype(np.int64)), (what, L, k)
    for k in ("labels", "cu_seqlens", "doc_start"):
        helpers.assert_array_same(got64[k], got[k], (what, L, k))
    assert all(got64[k] == got[k] for k in COUNTS)
    return exp


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
    from test_gpu_join import SPECIALS
    from test_host_tokenizer import model
    t = tk.Tekkenizer.from_json(json.dumps(model(small_vocab["tokens"], specials=SPECIALS)), device=0)
    yield t
    t.close()


HELLO = [1, 266, 42, 129, 121, 124, 118, 110, 2]   # "hello world" with BOS / EOS on the small vocabulary (tests/test_gpu_spans.py)


def test_known_answer_small_vocab(tk, small_tok):
    import torch
    t = small_tok
    Q = t.pad_id()
    assert Q == 3
    docs = ["hello world", "", "hello"]             # HELLO, [1, 2], [1, 266, 2]
    for dtype, rt in (("int64", "pt"), ("int32", "pt"), ("int64", "np"), ("int32", "np")):
        r = t.encode_batch_packed_whole(docs, seq_len=12, dtype=dtype, return_tensors=rt)
        assert r["input_ids"].tolist() == [HELLO + [1, 2, Q], [1, 266, 2] + [Q] * 9]
        assert r["position_ids"].tolist() == [[0, 1, 2, 3, 4, 5, 6, 7, 8, 0, 1, 0], [0, 1, 2] + [0] * 9]
        assert r["segment_ids"].tolist() == [[1] * 9 + [2, 2, 0], [1, 1, 1] + [0] * 9]
        assert r["cu_seqlens"].tolist() == [0, 9, 11, 12, 15, 24] and r["doc_start"].tolist() == [0, 9, 12] and r["labels"] is None
        assert (r["max_seqlen"], r["n_rows"], r["n_segments"], r["n_truncated"], r["n_pad"]) == (9, 2, 5, 0, 10)
        if rt == "pt":
            assert r["input_ids"].is_cuda and r["input_ids"].dtype == (torch.int64 if dtype == "int64" else torch.int32)
            assert r["cu_seqlens"].dtype == torch.int32 and r["doc_start"].dtype == torch.int64
        else:
            assert r["input_ids"].dtype == (np.int64 if dtype == "int64" else np.int32) and r["cu_seqlens"].dtype == np.int32
        # seq_len 4: "hello world" is truncated and keeps its EOS
        r = t.encode_batch_packed_whole(docs, seq_len=4, dtype=dtype, return_tensors=rt)
        assert r["input_ids"].tolist() == [[1, 266, 42, 2], [1, 2, Q, Q], [1, 266, 2, Q]] and r["n_truncated"] == 1
        assert r["cu_seqlens"].tolist() == [0, 4, 6, 8, 11, 12] and r["doc_start"].tolist() == [0, 4, 8] and r["max_seqlen"] == 4
    r = t.encode_batch_packed_whole(docs, seq_len=4, add_eos=False, pad_id=77, return_position_ids=False, return_doc_start=False)
    assert r["input_ids"].tolist() == [[1, 266, 42, 129], [1, 1, 266, 77]]            # no EOS: the truncated document simply ends
    assert r["position_ids"] is None and r["doc_start"] is None and r["segment_ids"].tolist() == [[1] * 4, [1, 2, 2, 0]]
    for bad in (dict(seq_len=0), dict(seq_len=8, dtype="int16")):
        with pytest.raises(tk.TokenizerError) as e:
            t.encode_batch_packed_whole(docs, **bad)
        assert e.value.code == tk.TK_ERR_INVALID_ARG


def test_known_answer_chat_packed(tk, small_tok):
    import torch
    t = small_tok
    chats = [[{"role": "system", "content": "be brief"}, {"role": "user", "content": "hello world"}, {"role": "assistant", "content": "hello"}],
             [{"role": "user", "content": "hello"}, {"role": "assistant", "content": "world hello"}], [],
             [{"role": "user", "content": "hello"}]]
    c = t.encode_chat(chats, return_tensors="np")
    for L in (64, 24, 8):
        for dtype in ("int64", "int32"):
            exp = expected_rowfit(c["input_ids"], c["offsets"], c["labels"], L, t.pad_id(), IGN, 0, ALL | (I64 if dtype == "int64" else 0))
            if dtype == "int64":
                exp["labels"] = exp["labels"].astype(np.int64)
            r = t.encode_chat_packed(chats, L, dtype=dtype)
            assert r["n_labelled"] == c["n_labelled"] and r["input_ids"].is_cuda and r["labels"].dtype == r["input_ids"].dtype
            got = {k: (r[k].cpu().numpy() if torch.is_tensor(r[k]) else r[k]) for k in r}
            got["doc_start"] = got["doc_start"].astype(np.uint64)
            assert_same(got, exp, (L, dtype))
            n = t.encode_chat_packed(chats, L, dtype=dtype, return_tensors="np")
            n["doc_start"] = n["doc_start"].astype(np.uint64)
            assert_same(n, exp, ("np", L, dtype))
    assert exp["n_truncated"] > 0 and exp["n_rows"] > 1                  # (L = 8 truncates; nothing is truncated at L = 64)
    r = t.encode_chat_packed(chats, 64)
    assert r["n_truncated"] == 0 and (r["labels"] != IGN).sum().item() == c["n_labelled"]
    r = t.encode_chat_packed([], 8)
    assert r["n_rows"] == 0 and tuple(r["input_ids"].shape) == (0, 8) and r["cu_seqlens"].tolist() == [0]


# ---- made-up ids through tk_rowfit_from_ids_device ----

@pytest.mark.parametrize("L", [1, 3, 4, 5, 8, 64, 4096])
def test_sweep_from_ids(tk, eng_bench, L):
    rng = np.random.default_rng(40 + L)
    residues = set()
    for D in (0, 1, 2, 63, 64, 65, 257, 4097):
        if D == 0:
            lengths = np.zeros(0, np.int64)
        elif L == 4096 and D > 257:
            lengths = rng.integers(0, 40, D)                              # (what the plain loops of the restatement can take)
            for special in (L, L + 1, 3 * L, L // 2 + 1, L - 17):         # ... with exact-fit, over-long and half-row documents among them
                lengths[rng.integers(0, D, 4)] = special
        else:
            lengths = random_lengths(rng, D, L)
        exp = check_case(eng_bench, lengths, L, int(rng.integers(0, L + 1)), D, ("sweep", D))
        residues |= {int(s) % 4 for s, n in zip(exp["doc_start"], lengths) if n > 0}
    assert L == 1 or residues == {0, 1, 2, 3}                             # document starts at every residue of 4, on both store paths


def test_every_subset_of_the_optional_outputs(tk, eng_bench):
    lengths = random_lengths(np.random.default_rng(7), 65, 8)
    ids, oo, lab = ragged_of(lengths, 7)
    full = expected_rowfit(ids, oo, lab, 8, P, IGN, 1, ALL)
    names = {POSITIONS: "position_ids", SEGMENTS: "segment_ids", CU_SEQLENS: "cu_seqlens", LABELS: "labels", DOC_START: "doc_start"}
    for k in range(len(names) + 1):
        for sub in itertools.combinations(names, k):
            flags = sum(sub)
            res, got = fit_of(eng_bench, ids, oo, lab, 8, 1, flags)
            exp = {**full, **{name: None for f, name in names.items() if not flags & f}}
            assert_same(got, exp, ("subset", flags))
            for f, name in names.items():
                assert (getattr(res, name + "_ptr") is None) == (not flags & f), (flags, name)


def test_length_mixes(tk, eng_bench):
    eng = eng_bench
    for L in (4, 5):
        exp = check_case(eng, [L] * 65, L, 0, 1, "all == L")
        assert exp["n_pad"] == 0 and exp["n_rows"] == 65 and exp["n_segments"] == 65
    for L, D in ((8, 4097), (3, 65), (4096, 3)):                         # every document a row of its own: the chain has D links
        exp = check_case(eng, [L // 2 + 1] * D, L, 0, 2, "all L // 2 + 1")
        assert exp["n_rows"] == D and exp["doc_start"].tolist() == [r * L for r in range(D)]
    exp = check_case(eng, [1] * 5000, 4096, 0, 3, "one-id documents")    # more than TKY_CAP starts in a tile
    assert exp["n_rows"] == 2 and exp["n_segments"] == 5001
    # runs of 70 or more empty documents at the front, in the middle, behind a full row and at the end
    z = [0] * 75
    exp = check_case(eng, z + [3, 2] + z + [3] + [8] + z + [5, 3] + z + [1] + z, 8, 0, 4, "runs of empty documents")
    assert exp["n_rows"] == 4 and exp["doc_start"][77 + 75 + 2] == 16 and exp["doc_start"][-1] == 25
    # sums that hit E[j] - E[i] == L exactly, and L + 1
    exp = check_case(eng, [3, 5, 3, 6, 4, 4, 1, 7, 1, 8, 8, 1] * 30, 8, 0, 5, "exact fits and misses by one")
    assert exp["n_rows"] == 241
    for L in (5, 8):
        for keep_tail in (0, 1, L):
            exp = check_case(eng, [2, L + 1, 3 * L, 1, L + 1, L, 3 * L] * 20, L, keep_tail, 6, "over-long documents")
            assert exp["n_truncated"] == 4 * 20
    for n in (1, 7, 8, 9):
        exp = check_case(eng, [n], 8, 1, 8, "one document alone")
        assert exp["n_rows"] == 1 and exp["n_truncated"] == (n > 8)
    for shapes in ([(8, 0)] * 2, [(64, 5), (8, 3), (4096, 40)], [(4096, 1), (3, 0), (64, 64)]):   # shrinking and growing, call after call
        for L, kt in shapes:
            check_case(eng, random_lengths(np.random.default_rng(L + kt), 129, L), L, kt, 9, "call after call")


def test_many_rows_at_the_widest_row(tk, eng_bench):
    """600 documents of L // 2 + 1 ids at L = 4096: a row each, 600 links of the chain (10 rounds) on the vector-store path.  The
    expected tensors follow from the definition without the element loops: row d is document d and 2047 pads."""
    L, D = 4096, 600
    n = L // 2 + 1
    ids, oo, lab = ragged_of([n] * D, 11)
    pad = np.arange(L) >= n
    exp = {"input_ids": np.where(pad, P, ids.reshape(D, n).astype(np.int32)[:, np.minimum(np.arange(L), n - 1)]).astype(np.int32),
           "labels": np.where(pad, IGN, lab.reshape(D, n)[:, np.minimum(np.arange(L), n - 1)]).astype(np.int32),
           "position_ids": np.tile(np.where(pad, 0, np.arange(L)), (D, 1)).astype(np.int32),
           "segment_ids": np.tile(np.where(pad, 0, 1), (D, 1)).astype(np.int32),
           "cu_seqlens": np.sort(np.concatenate([np.arange(D) * L, np.arange(D) * L + n, [D * L]])).astype(np.int32),
           "doc_start": (np.arange(D) * L).astype(np.uint64),
           "n_rows": D, "n_segments": 2 * D, "max_seqlen": n, "n_truncated": 0, "n_pad": D * (L - n)}
    _, got = fit_of(eng_bench, ids, oo, lab, L, 0, ALL)
    assert_same(got, exp, "600 rows of 4096")
    small = expected_rowfit(ids[:3 * n], oo[:4], lab[:3 * n], L, P, IGN, 0, ALL)       # the construction above against the restatement
    for k in TENSORS[:4]:
        assert np.array_equal(exp[k][:3], small[k]), k
    _, got64 = fit_of(eng_bench, ids, oo, lab, L, 0, ALL | I64)
    assert np.array_equal(got64["input_ids"], exp["input_ids"].astype(np.int64)) and np.array_equal(got64["labels"], exp["labels"])


def test_empty_shapes(tk, eng_bench):
    for flags in (ALL, ALL | I64, 0, LABELS):
        for oo in (np.zeros(1, np.int64), np.zeros(6, np.int64)):          # D = 0; all-empty documents
            _, got = fit_of(eng_bench, np.zeros(0, np.uint32), oo, None, 8, 0, flags)
            assert_same(got, expected_rowfit([], oo, None, 8, P, IGN, 0, flags), (flags, len(oo)))
        host = eng_bench.encode_batch_rowfit(np.zeros(0, np.uint8), np.zeros(1, np.uint64), 8, True, True, pad_id=P, flags=flags & ~LABELS)
        assert_same(host, expected_rowfit([], [0], None, 8, P, IGN, 0, flags & ~LABELS), ("host", flags))


# ---- the fused and host entries ----

@pytest.mark.parametrize("vname", ["test", "bench"])
def test_fused_and_host_entries(tk, vocabs, vname):
    import torch
    v = vocabs[vname]
    Q = 7                                            # an id encode never emits (a special that is neither BOS nor EOS)
    docs = [x for x in sweep_docs() if len(x) < 70000]
    data, offs = pack(docs)
    D = len(docs)
    orc = helpers.oracle_for(v)
    eng = tk.Engine(v["tokens"], v["num_special"], v["bos"], v["eos"], device=0)
    d_bytes = torch.from_numpy(data).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    flags0 = ALL & ~LABELS
    try:
        for i, (bos, eos, L) in enumerate(((True, True, 512), (False, True, 64), (True, False, 2048))):
            eids, eoo = orc.encode_batch(data, offs, bos, eos, threads=8)
            flags = flags0 | (I64 if i & 1 else 0)
            p_ids, p_oo, n_ids, res = eng.encode_batch_device_rowfit(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), L, bos, eos, pad_id=Q,
                                                                     keep_tail=int(eos), flags=flags, checks=tk.CHECK_OFFSETS, stream=stream)
            ids = to_host(tk.DeviceView(p_ids, n_ids, "<i4"), (n_ids,), np.uint32)
            oo = to_host(tk.DeviceView(p_oo, D + 1, "<i8"), (D + 1,), np.uint64)
            assert np.array_equal(oo, eoo) and np.array_equal(ids, eids)
            exp = expected_rowfit(eids, eoo, None, L, Q, IGN, int(eos), flags)
            assert_same(fetch(res), exp, (vname, bos, eos, L))
            assert exp["n_truncated"] > 0
            if vname == "bench":
                host = eng.encode_batch_rowfit(data, offs, L, bos, eos, pad_id=Q, keep_tail=int(eos), flags=flags)
                assert_same(host, exp, ("host", bos, eos, L))
        small = sweep_docs()[:60] + [b"", b"a"]      # the one-launch small path: its ids are mapped pinned memory
        data, offs = pack(small)
        calls0 = eng.small_path_calls()
        host = eng.encode_batch_rowfit(data, offs, 96, True, True, pad_id=Q, keep_tail=1, flags=flags0)
        assert eng.small_path_calls() > calls0
        eids, eoo = orc.encode_batch(data, offs, True, True, threads=8)
        assert_same(host, expected_rowfit(eids, eoo, None, 96, Q, IGN, 1, flags0), "host, small path")
        with pytest.raises(tk.TokenizerError) as e:  # text has no labels stream
            eng.encode_batch_rowfit(data, offs, 96, True, True, flags=LABELS)
        assert e.value.code == tk.TK_ERR_INVALID_ARG
        # ... and on the device entry that is refused before anything is encoded: the last encode's outputs are as they were
        p_ids, p_oo, n_ids = eng.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), D, d_bytes.numel(), True, True, stream=stream)
        before = to_host(tk.DeviceView(p_ids, n_ids, "<i4"), (n_ids,), np.uint32).copy()
        one = torch.from_numpy(np.array([0, 1], np.int64)).cuda()
        with pytest.raises(tk.TokenizerError) as e:
            eng.encode_batch_device_rowfit(d_bytes.data_ptr(), one.data_ptr(), 1, 1, 96, True, True, flags=LABELS, stream=stream)
        assert e.value.code == tk.TK_ERR_INVALID_ARG
        assert np.array_equal(to_host(tk.DeviceView(p_ids, n_ids, "<i4"), (n_ids,), np.uint32), before)
    finally:
        eng.close()


# ---- buffers and argument errors ----

def test_outputs_outlive_each_other_and_argument_errors(tk, eng_bench, bench_vocab):
    import torch
    docs = [x for x in sweep_docs() if len(x) < 70000][:120]
    data, offs = pack(docs)
    D = len(docs)
    d_bytes = torch.from_numpy(data).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    eng = eng_bench
    p_ids, p_oo, n = eng.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), True, True, stream=stream)
    dn = eng.dense_from_ids_device(p_ids, p_oo, D, n, max_length=128, pad_id=7, keep_head=1, keep_tail=1, flags=4 | 16, stream=stream)   # FIXED | MASK
    sp = eng.seqpack_from_ids_device(p_ids, p_oo, D, n, 512, 7, 2 | 4 | 8, stream)
    ctrl, pfl, conv = dev(np.full(D, 4, np.uint32), np.uint32), dev(np.arange(D) % 4, np.uint32), dev(np.arange(D + 1), np.uint64)
    jn = eng.join_from_ids_device(p_ids, p_oo, D, n, ctrl.data_ptr(), pfl.data_ptr(), conv.data_ptr(), D, IGN, 1, 0, stream)

    def snapshot():
        R = (sp.n_rows, 512)
        return (to_host(tk.DeviceView(p_ids, n, "<i4"), (n,), np.uint32).copy(), to_host(tk.DeviceView(p_oo, D + 1, "<i8"), (D + 1,), np.uint64).copy(),
                to_host(tk.DeviceView(dn.ids_ptr, (D, 128), "<i4"), (D, 128), np.int32).copy(),
                to_host(tk.DeviceView(dn.mask_ptr, (D, 128), "|u1"), (D, 128), np.uint8).copy(),
                to_host(tk.DeviceView(sp.input_ids_ptr, R, "<i4"), R, np.int32).copy(), to_host(tk.DeviceView(sp.position_ids_ptr, R, "<i4"), R, np.int32).copy(),
                to_host(tk.DeviceView(sp.segment_ids_ptr, R, "<i4"), R, np.int32).copy(),
                to_host(tk.DeviceView(sp.cu_seqlens_ptr, sp.n_segments + 1, "<i4"), (sp.n_segments + 1,), np.int32).copy(),
                to_host(tk.DeviceView(jn.ids_ptr, jn.n_ids, "<i4"), (jn.n_ids,), np.uint32).copy(),
                to_host(tk.DeviceView(jn.labels_ptr, jn.n_ids, "<i4"), (jn.n_ids,), np.int32).copy(),
                to_host(tk.DeviceView(jn.offsets_ptr, D + 1, "<i8"), (D + 1,), np.uint64).copy())

    before = snapshot()
    eids, eoo = helpers.oracle_for(bench_vocab).encode_batch(data, offs, True, True, threads=8)
    assert np.array_equal(before[0], eids) and np.array_equal(before[1], eoo)
    # the join's ids / labels / offsets straight into the rowfit pass
    good = eng.rowfit_from_ids_device(jn.ids_ptr, jn.offsets_ptr, D, jn.n_ids, 512, 7, 0, ALL, jn.labels_ptr, IGN, stream)
    ptrs = {good.input_ids_ptr, good.labels_ptr, good.position_ids_ptr, good.segment_ids_ptr, good.cu_seqlens_ptr, good.doc_start_ptr,
            dn.ids_ptr, dn.mask_ptr, sp.input_ids_ptr, sp.position_ids_ptr, sp.segment_ids_ptr, sp.cu_seqlens_ptr, jn.ids_ptr, jn.labels_ptr,
            jn.offsets_ptr, p_ids, p_oo}
    assert len(ptrs) == 17 and None not in ptrs and 0 not in ptrs
    exp = expected_rowfit(before[8], before[10], before[9], 512, 7, IGN, 0, ALL)
    assert_same(fetch(good), exp)
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a, b)
    # every case of step 9: refused with a message, and the first rowfit result stays readable
    half = 2**29 + 1
    three = dev(np.array([0, half, 2 * half, 3 * half]), np.uint64)      # three documents of L // 2 + 1 ids: 3 rows of 2^30
    many = dev(np.arange(66) * half, np.uint64)                           # 65 of them: beyond 2^36 elements
    bad = [dict(seq_len=0), dict(seq_len=2**31), dict(seq_len=2**32 - 1, flags=0), dict(seq_len=512, flags=ALL | 64), dict(seq_len=512, flags=1 << 31),
           dict(seq_len=512, keep_tail=513), dict(seq_len=512, labels=0), dict(seq_len=512, n_docs=0),
           dict(seq_len=2**30, flags=0, oo=many.data_ptr(), n_docs=65, n_ids=65 * half),
           dict(seq_len=2**30, flags=CU_SEQLENS, oo=three.data_ptr(), n_docs=3, n_ids=3 * half),
           dict(seq_len=512, n_ids=jn.n_ids - 1)]                         # offsets that do not end at n_ids
    mem0 = torch.cuda.mem_get_info()[0]
    for opt in bad:
        with pytest.raises(tk.TokenizerError) as e:
            eng.rowfit_from_ids_device(jn.ids_ptr, opt.get("oo", jn.offsets_ptr), opt.get("n_docs", D), opt.get("n_ids", jn.n_ids), opt["seq_len"], 7,
                                       opt.get("keep_tail", 0), opt.get("flags", ALL), opt.get("labels", jn.labels_ptr), IGN, stream)
        assert e.value.code == tk.TK_ERR_INVALID_ARG and len(str(e.value)) > 20, (opt, str(e.value))
        assert_same(fetch(good), exp, ("the earlier result after", opt))
    assert mem0 - torch.cuda.mem_get_info()[0] < 2**28                    # refused before any tensor of 2^30-element rows was allocated
    # the three-document case is valid without cu_seqlens only as far as memory goes: nothing here runs it
    with pytest.raises(tk.TokenizerError) as e:
        eng.encode_batch_device_rowfit(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), 0, True, True, stream=stream)
    assert e.value.code == tk.TK_ERR_INVALID_ARG
    with pytest.raises(tk.TokenizerError) as e:
        eng.encode_batch_rowfit(data, offs, 64, True, True, flags=64)
    assert e.value.code == tk.TK_ERR_INVALID_ARG
    assert_same(fetch(good), exp, "the earlier result after the fused entries' errors")
    for a, b in zip(before[2:], snapshot()[2:]):
        assert np.array_equal(a, b)


def test_parts_entry_equals_join_then_rowfit(tk, eng_bench):
    import torch
    eng = eng_bench
    stream = torch.cuda.current_stream().cuda_stream
    parts = [x for x in sweep_docs() if len(x) < 3000][:90]
    data, offs = pack(parts)
    n_parts, C = len(parts), 31
    ctrl = np.where(np.arange(n_parts) % 3 == 0, 4, 0xFFFFFFFF).astype(np.uint32)
    pf = (np.arange(n_parts) % 4).astype(np.uint32)
    conv = np.concatenate([[0, 0], np.sort(np.random.default_rng(3).integers(0, n_parts, C - 2)), [n_parts]]).astype(np.uint64)
    d_bytes, d_offs = torch.from_numpy(data).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda()
    d_ctrl, d_pf, d_conv = dev(ctrl, np.uint32), dev(pf, np.uint32), dev(conv, np.uint64)
    for L, flags in ((256, ALL), (1000, ALL | I64)):
        j, fit = eng.encode_parts_device_rowfit(d_bytes.data_ptr(), d_offs.data_ptr(), n_parts, len(data), d_ctrl.data_ptr(), d_pf.data_ptr(),
                                                d_conv.data_ptr(), C, L, P, 0, flags, IGN, 1, tk.CHECK_OFFSETS | tk.CHECK_PARTS, stream)
        jids = to_host(tk.DeviceView(j.ids_ptr, j.n_ids, "<i4"), (j.n_ids,), np.uint32)
        jlab = to_host(tk.DeviceView(j.labels_ptr, j.n_ids, "<i4"), (j.n_ids,), np.int32)
        joo = to_host(tk.DeviceView(j.offsets_ptr, C + 1, "<i8"), (C + 1,), np.uint64)
        host = eng.encode_parts_join(data, offs, ctrl, pf, conv, ignore_index=IGN, flags=1)
        assert np.array_equal(jids, host["ids"]) and np.array_equal(jlab, host["labels"]) and np.array_equal(joo, host["offsets"])
        exp = expected_rowfit(jids, joo, jlab, L, P, IGN, 0, flags)
        assert_same(fetch(fit), exp, ("parts", L))
        assert exp["n_rows"] > 1 and int((exp["labels"] != IGN).sum()) > 0
    with pytest.raises(tk.TokenizerError) as e:      # labels asked of a join that makes none: refused before anything runs
        eng.encode_parts_device_rowfit(d_bytes.data_ptr(), d_offs.data_ptr(), n_parts, len(data), d_ctrl.data_ptr(), d_pf.data_ptr(),
                                       d_conv.data_ptr(), C, 256, P, 0, ALL, IGN, 0, tk.CHECK_OFFSETS | tk.CHECK_PARTS, stream)
    assert e.value.code == tk.TK_ERR_INVALID_ARG and "TK_JOIN_LABELS" in str(e.value)
    assert_same(fetch(fit), exp, "the last result after the refused call")
