"""Sentence-pair rows on the GPU (include/tekken_hip.h tk_pair_from_ids_device and the entries around it, csrc/tk_pair.hip) against
the plain-loop restatement of the definition in tests/test_pair_cpu.py -- element by element over every output, never through a
sum."""
import json

import numpy as np
import pytest

import helpers
from helpers import dev, on_device, to_host
from test_gpu_spans import pack, sweep_docs
from test_pair_cpu import (ARRAYS, COUNTS, FIXED, I64, LONGEST_FIRST, MASK, ONLY_FIRST, ONLY_SECOND, OVERFLOW, SEQUENCE_IDS, SPANS, TYPE_IDS,
                           expected_pairs, ragged, refused_cases)

pytestmark = pytest.mark.gpu

EVERY = MASK | TYPE_IDS | SEQUENCE_IDS | SPANS
HEAD, SEP, TAIL = (1,), (2,), (2,)       # n_head = 1: the A run is misaligned against the 4-element units
PAD = 5


def fetch(res):
    """PairResult -> dict like expected_pairs's."""
    dt = np.int64 if res.typestr == "<i8" else np.int32
    W, L = res.n_windows, res.row_len
    v = res.views()
    out = {"input_ids": to_host(v[0], (W, L), dt), "spans": to_host(v[8], (W, L, 2), np.uint32),
           "pair_windows": to_host(v[9], (res.n_pairs + 1,), np.uint64)}
    for i, k in ((1, "mask"), (2, "type_ids"), (3, "sequence_ids")):
        out[k] = to_host(v[i], (W, L), np.uint8)
    for i, k in ((4, "lengths"), (5, "window_pair"), (6, "window_start"), (7, "second_start")):
        out[k] = to_host(v[i], (W,), np.uint32)
    out.update({k: getattr(res, k) for k in COUNTS})
    return out


def assert_same(got, exp, what=""):
    helpers.assert_same(got, exp, what, COUNTS, ARRAYS)


def select(exp, flags):
    """expected_pairs's result for all outputs, as it is for `flags`: int64 on request, an unselected output None."""
    out = dict(exp)
    if flags & I64:
        out["input_ids"] = exp["input_ids"].astype(np.int64)
    for f, k in ((MASK, "mask"), (TYPE_IDS, "type_ids"), (SEQUENCE_IDS, "sequence_ids"), (SPANS, "spans")):
        if not flags & f:
            out[k] = None
    return out


def pairs_of(eng, d_ids, d_oo, n_ids, T, strategy, s, F, m, flags, d_spans=None, lists=(HEAD, SEP, TAIL), pad=PAD):
    import torch
    res = eng.pair_from_ids_device(d_ids.data_ptr(), d_oo.data_ptr(), d_oo.numel() - 1, n_ids, T, strategy, s, F, m, pad, *lists, flags=flags,
                                   d_spans_ptr=d_spans.data_ptr() if d_spans is not None else 0, stream=torch.cuda.current_stream().cuda_stream)
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


# ---- known answers through Tekkenizer.encode_pairs ----

KEYS = {"input_ids", "attention_mask", "token_type_ids", "sequence_ids", "lengths", "overflow_to_sample_mapping", "window_start", "second_start",
        "pair_windows", "offset_mapping", "n_windows", "n_truncated", "n_split", "n_fixed_cut"}


def test_known_answers_small_vocab(tk, small_tok):
    import torch
    t = small_tok
    P = t.pad_id()
    assert P == 3 and t.bos_id() == 1 and t.eos_id() == 2
    # the first worked case of the definition: "hello" is [266], "hello world" [266, 42, 129, 121, 124, 118, 110]
    r = t.encode_pairs(["hello"], ["hello world"], 8, truncation="only_second", stride=1, return_overflowing_tokens=True, max_fixed=2,
                       sep=["</s>"], return_sequence_ids=True, return_offsets_mapping=True)
    assert set(r) == KEYS
    assert r["input_ids"].tolist() == [[1, 266, 2, 266, 42, 129, 121, 2], [1, 266, 2, 121, 124, 118, 110, 2]]
    assert r["window_start"].tolist() == [0, 3] and r["second_start"].tolist() == [3, 3] and r["overflow_to_sample_mapping"].tolist() == [0, 0]
    assert r["token_type_ids"].tolist() == [[0, 0, 0, 1, 1, 1, 1, 1]] * 2 and r["sequence_ids"].tolist() == [[255, 0, 255, 1, 1, 1, 1, 255]] * 2
    assert r["attention_mask"].tolist() == [[1] * 8] * 2 and r["lengths"].tolist() == [8, 8] and r["pair_windows"].tolist() == [0, 2]
    assert (r["n_windows"], r["n_truncated"], r["n_split"], r["n_fixed_cut"]) == (2, 1, 1, 0)
    assert r["offset_mapping"].tolist() == [[[0, 0], [0, 5], [0, 0], [0, 5], [5, 6], [6, 7], [7, 8], [0, 0]],
                                            [[0, 0], [0, 5], [0, 0], [7, 8], [8, 9], [9, 10], [10, 11], [0, 0]]]
    assert isinstance(r["input_ids"], torch.Tensor) and r["input_ids"].dtype == torch.int64 and r["input_ids"].is_cuda
    assert r["token_type_ids"].dtype == torch.uint8 and r["second_start"].dtype == torch.int32 and r["pair_windows"].dtype == torch.int64
    assert r["offset_mapping"].dtype == torch.int32 and tuple(r["offset_mapping"].shape) == (2, 8, 2)
    # the second: longest_first at T = 10, no sep; numpy, int32; a second pair that fits
    r = t.encode_pairs(["hello world", "hello"], ["hello world", ""], 10, dtype="int32", return_tensors="np")
    assert set(r) == KEYS and r["input_ids"].dtype == np.int32 and r["sequence_ids"] is None and r["offset_mapping"] is None
    assert r["input_ids"].tolist() == [[1, 266, 42, 129, 121, 266, 42, 129, 121, 2], [1, 266, 2] + [P] * 7]
    assert r["token_type_ids"].tolist() == [[0] * 5 + [1] * 5, [0, 0, 1] + [0] * 7] and r["attention_mask"].tolist() == [[1] * 10, [1] * 3 + [0] * 7]
    assert r["lengths"].tolist() == [10, 3] and r["second_start"].tolist() == [5, 2] and r["lengths"].dtype == np.int32
    assert (r["n_windows"], r["n_truncated"], r["n_split"], r["n_fixed_cut"]) == (2, 1, 0, 0) and r["pair_windows"].tolist() == [0, 1, 2]
    # padding "longest" with pad_to_multiple_of, explicit ids for the lists, a pad id of the caller's, views of the context's buffers
    for rt in ("pt", "np"):
        r = t.encode_pairs(["hello"], ["hello"], 64, truncation="only_first", padding="longest", pad_to_multiple_of=4, head=[1, 1], sep=(7,),
                           tail=(), pad_id=77, return_attention_mask=False, return_token_type_ids=False, return_tensors=rt, copy=False)
        assert r["input_ids"].tolist() == [[1, 1, 266, 7, 266, 77, 77, 77]] and r["attention_mask"] is None and r["token_type_ids"] is None
        assert r["second_start"].tolist() == [4] and r["lengths"].tolist() == [5]
    # offset_mapping in bytes and in code points for a pair with a two-byte character, against the spans of each text alone
    first, second = ["é", "hello"], ["hello é", "wé"]
    for unit in ("byte", "char"):
        alone = t.encode_batch_with_offsets([x for pair in zip(first, second) for x in pair], offsets_unit=unit)
        ids, oo = ragged([a[0] for a in alone])
        sp = np.array([s for a in alone for s in a[1]], np.uint32).reshape(-1, 2)
        exp = expected_pairs(ids, oo, 16, LONGEST_FIRST, 0, 0, 0, P, (1,), (), (2,), FIXED | I64 | SPANS, sp)
        for rt in ("pt", "np"):
            r = t.encode_pairs(first, second, 16, return_offsets_mapping=True, offsets_unit=unit, return_tensors=rt)
            assert r["input_ids"].tolist() == exp["input_ids"].tolist() and r["offset_mapping"].tolist() == exp["spans"].tolist(), (unit, rt)
    assert exp["input_ids"][0].tolist()[:8] == [1, 205, 179, 266, 42, 205, 179, 2]
    assert exp["spans"][0].tolist()[:8] == [[0, 0], [0, 1], [0, 1], [0, 5], [5, 6], [6, 7], [6, 7], [0, 0]]      # code points: both bytes of the e-acute cover it
    for bad in (dict(truncation="longest"), dict(dtype="int16"), dict(padding="left"), dict(return_tensors="tf"), dict(stride=1),
                dict(head=[1] * 5), dict(max_fixed=2 ** 32)):
        with pytest.raises(tk.TokenizerError) as e:
            t.encode_pairs(["hello"], ["hello"], 8, **bad)
        assert e.value.code == tk.TK_ERR_INVALID_ARG, bad
    with pytest.raises(tk.TokenizerError) as e:
        t.encode_pairs(["hello"], ["hello", "world"], 8)
    assert e.value.code == tk.TK_ERR_INVALID_ARG


# ---- made-up ids through tk_pair_from_ids_device ----

def made_up(cw):
    """5 600 pairs: 600 with sides of up to 299 ids (some empty on one side, the first 2 and last 2 on both; one side of 50 001
    ids; sides of exactly cw, cw + 1 and 4 * cw + 3 beside a one-id side, either way round) and a run of 5 000 pairs of one-id
    sides.  cw: the room of the windowed side beside a one-id fixed side."""
    rng = np.random.default_rng(51)
    n = rng.integers(0, 300, (600, 2))
    pool = np.arange(20, 597)
    n[rng.choice(pool, 40, replace=False), 0] = 0
    n[rng.choice(pool, 40, replace=False), 1] = 0
    n[[0, 1, 598, 599]] = 0
    n[5], n[6] = (1, 50_001), (50_001, 1)
    n[7], n[8], n[9] = (1, cw), (1, cw + 1), (1, 4 * cw + 3)
    n[10], n[11], n[12] = (cw, 1), (cw + 1, 1), (4 * cw + 3, 1)
    n[13] = (0, 4 * cw + 3)
    n = np.concatenate([n[:300], np.ones((5000, 2), np.int64), n[300:]])
    oo = np.concatenate([[0], np.cumsum(n.reshape(-1))]).astype(np.int64)
    ids = rng.integers(0, 2**31 - 1, int(oo[-1])).astype(np.uint32)
    return ids, oo


def made_up_spans(n_ids):
    g = np.arange(n_ids, dtype=np.uint64)
    return np.stack([(g * 2 + 1) & 0xFFFFFFFF, (g * 3 + 7) & 0xFFFFFFFF], axis=1).astype(np.uint32)   # index-derived: a wrong source index shows


def run_config(eng, ids, oo, T, strategy, s, F, m, flags, lists=(HEAD, SEP, TAIL), variants=True):
    """Every output against the restatement: all optional outputs at once, then int64 without any, then each one alone."""
    sp = made_up_spans(len(ids))
    exp = expected_pairs(ids, oo, T, strategy, s, F, m, PAD, *lists, flags | EVERY, sp)
    d_ids, d_oo = on_device(ids, oo)
    d_sp = dev(sp.reshape(-1), np.uint32)
    res, got = pairs_of(eng, d_ids, d_oo, len(ids), T, strategy, s, F, m, flags | EVERY, d_sp, lists)
    assert None not in (res.mask_ptr, res.type_ids_ptr, res.sequence_ids_ptr, res.spans_ptr)
    assert_same(got, exp, "every output")
    for fl in ((I64, MASK | I64, TYPE_IDS, SEQUENCE_IDS | I64, SPANS) if variants else (I64,)):
        res, got = pairs_of(eng, d_ids, d_oo, len(ids), T, strategy, s, F, m, flags | fl, d_sp if fl & SPANS else None, lists)
        assert_same(got, select(exp, fl), ("flags", fl))
    return exp


C64 = 64 - 3         # the room of the two texts at T = 64 under HEAD / SEP / TAIL
CONFIGS = [(LONGEST_FIRST, 0, 0, 0), (ONLY_FIRST, 0, 0, 0), (ONLY_SECOND, 0, 0, 0)] + \
          [(st, s, 8, OVERFLOW) for st in (ONLY_FIRST, ONLY_SECOND) for s in (0, 1, C64 - 8 - 1)]


@pytest.mark.parametrize("strategy,s,F,overflow", CONFIGS)
def test_from_ids_on_made_up_ids(tk, eng_bench, strategy, s, F, overflow):
    ids, oo = made_up(C64 - 1)
    exp = run_config(eng_bench, ids, oo, 64, strategy, s, F, 0, FIXED | overflow)
    # from the restatement's result alone: the case set holds what it is for
    w, n = np.diff(exp["pair_windows"].astype(np.int64)), np.diff(oo).reshape(-1, 2)
    v = n[:, 1] if strategy == ONLY_SECOND else n[:, 0]
    assert exp["n_pairs"] == 5600 and exp["row_len"] == 64
    if overflow:
        one_id_x = (n[:, 0] if strategy == ONLY_SECOND else n[:, 1]) == 1
        step = C64 - 1 - s
        for side, windows in ((C64 - 1, 1), (C64, 2), (4 * C64 - 1, 1 + -(-(3 * C64) // step))):     # cw, cw + 1, 4 * cw + 3
            assert np.sum(one_id_x & (v == side)) >= 1 and np.all(w[one_id_x & (v == side)] == windows), side
        assert w.max() > 4096 // (1 if s > 1 else 8)
        assert exp["n_split"] == int(np.sum(w > 1)) > 100 and exp["n_fixed_cut"] > 100
    else:
        assert np.all(w == 1) and exp["n_split"] == 0 and exp["n_truncated"] > 100
        assert exp["n_fixed_cut"] == (0 if strategy == LONGEST_FIRST else int(np.sum((n[:, 1] if strategy == ONLY_FIRST else n[:, 0]) > C64 - 1)))


# ---- shapes the fill kernel can get wrong ----

def test_rows_of_four_elements_over_one_id_pairs(tk, eng_bench):
    """L = 4: a block's row group holds 2 048 rows, more pairs than LDS has room for (TKY_CAP) over the 5 000 one-id pairs -- the
    global-memory form of the staging -- and fewer elsewhere."""
    ids, oo = made_up(3)
    none = ((), (), ())
    run_config(eng_bench, ids, oo, 4, LONGEST_FIRST, 0, 0, 0, FIXED, none)                       # all lists empty: c = 4
    run_config(eng_bench, ids, oo, 4, ONLY_SECOND, 1, 1, 0, FIXED | OVERFLOW, none, variants=False)
    run_config(eng_bench, ids, oo, 4, LONGEST_FIRST, 0, 0, 0, FIXED, ((1,), (), (2,)), variants=False)        # x = 2: c = 2
    run_config(eng_bench, ids, oo, 4, ONLY_FIRST, 0, 1, 0, OVERFLOW, ((1,), (), (2,)), variants=False)        # cw = 1, longest mode


def test_row_length_that_is_no_multiple_of_four(tk, eng_bench):
    ids, oo = made_up(37 - 3 - 1)
    run_config(eng_bench, ids, oo, 37, LONGEST_FIRST, 0, 0, 0, FIXED)
    exp = run_config(eng_bench, ids, oo, 37, ONLY_SECOND, 5, 8, 0, FIXED | OVERFLOW, variants=False)
    assert exp["row_len"] == 37 and exp["n_split"] > 100
    run_config(eng_bench, ids, oo, 37, ONLY_FIRST, 0, 0, 3, 0, variants=False)                    # longest mode, rounded to 39


def test_row_longer_than_a_block_tile(tk, eng_bench):
    """T = 9 001: the units of one row are split over blockIdx.y, element by element (L = 9 001) and in units of 4 (L = 9 004)."""
    rng = np.random.default_rng(52)
    n = [3000, 20000, 0, 5, 9000, 9000, 10, 8998, 20000, 120, 4500, 4499, 1, 1]
    oo = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    ids = rng.integers(0, 2**31 - 1, int(oo[-1])).astype(np.uint32)
    for m in (0, 4):
        for strategy, s, F, fl in ((LONGEST_FIRST, 0, 0, 0), (ONLY_SECOND, 50, 100, OVERFLOW), (ONLY_FIRST, 0, 4000, OVERFLOW)):
            exp = run_config(eng_bench, ids, oo, 9001, strategy, s, F, m, FIXED | fl, variants=False)
            assert exp["row_len"] == 9001 + 3 * (m == 4) and exp["lengths"].max() == 9001 and (exp["n_split"] > 0) == bool(fl)


def test_empty_shapes(tk, eng_bench):
    eng = eng_bench
    none = ((), (), ())
    for strategy in (LONGEST_FIRST, ONLY_FIRST, ONLY_SECOND):
        for flags in (0, FIXED, OVERFLOW if strategy else 0):
            for m in (0, 8):
                # P = 0; P = 1; all pairs empty: L = x in longest mode, 0 without a fixed id
                for ids, oo in (ragged([]), ragged([[11, 12, 13], [14] * 9]), ragged([[]] * 10)):
                    for lists in ((HEAD, SEP, TAIL), none):
                        exp = run_config(eng, ids.astype(np.uint32), oo, 8, strategy, 0, 0, m, flags, lists, variants=False)
                        if len(ids) == 0 and not flags & FIXED:
                            x = sum(len(l) for l in lists) if len(oo) > 1 else 0
                            assert exp["row_len"] == (-(-x // 8) * 8 if m else x) and exp["n_windows"] == (len(oo) - 1) // 2


# ---- the fused and host entries ----

def host_as_expected(host, P):
    return {**host, "row_len": host["input_ids"].shape[1], "n_pairs": P}


@pytest.mark.parametrize("vname", ["test", "bench"])
def test_fused_entries_on_real_text(tk, vocabs, vname):
    import torch
    v = vocabs[vname]
    P = 7                                            # an id encode never emits (a special that is neither BOS nor EOS)
    docs = [x for x in sweep_docs() if len(x) < 70000]
    docs = docs[:len(docs) // 2 * 2]
    small = sweep_docs()[:60] + [b"", b"a"]          # ASCII documents of 512 bytes: the one-launch small path of the host entry
    lists = ((v["bos"],), (v["eos"], v["bos"]), (v["eos"],))
    orc = helpers.oracle_for(v)
    eng = tk.Engine(v["tokens"], v["num_special"], v["bos"], v["eos"], device=0)
    stream = torch.cuda.current_stream().cuda_stream
    try:
        for parts, is_small in ((docs, False), (small, True)):
            data, offs = pack(parts)
            D = len(parts)
            d_bytes = torch.from_numpy(data if len(data) else np.zeros(1, np.uint8)).cuda()
            d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
            # each side encoded alone: no token spans the seam
            eids, eoo = orc.encode_batch(data, offs, False, False, threads=8)
            _, _, p_sp, n = eng.encode_batch_device_spans(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), False, False, stream=stream)
            sp = to_host(tk.DeviceView(p_sp, 2 * n, "<i4"), (2 * n,), np.uint32).reshape(-1, 2).copy()
            for T, strategy, s, F, m, flags in ((128, ONLY_SECOND, 16, 32, 0, FIXED | OVERFLOW | EVERY), (64, LONGEST_FIRST, 0, 0, 0, MASK | I64),
                                                (30, ONLY_FIRST, 3, 10, 4, OVERFLOW | I64 | TYPE_IDS | SPANS)):
                p_ids, p_oo, n_ids, res = eng.encode_pairs_device(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), T, strategy, s, F, m, P, *lists,
                                                                  flags=flags, checks=tk.CHECK_OFFSETS, stream=stream)
                ids = to_host(tk.DeviceView(p_ids, n_ids, "<i4"), (n_ids,), np.uint32)
                oo = to_host(tk.DeviceView(p_oo, D + 1, "<i8"), (D + 1,), np.uint64)
                assert np.array_equal(oo, eoo) and np.array_equal(ids, eids)
                dv = fetch(res)
                assert_same(dv, expected_pairs(eids, eoo, T, strategy, s, F, m, P, *lists, flags, sp), (vname, T, strategy))
                calls0 = eng.small_path_calls()
                host = eng.encode_pairs(data, offs, T, strategy, s, F, m, P, *lists, flags=flags)
                assert (eng.small_path_calls() > calls0) == is_small
                assert_same(host_as_expected(host, D // 2), dv, (vname, "host entry", T, strategy))
    finally:
        eng.close()


# ---- refusals ----

def test_refusals_leave_the_earlier_result_readable(tk, eng_bench):
    import torch
    eng = eng_bench
    stream = torch.cuda.current_stream().cuda_stream
    cases = refused_cases()
    ids, oo = cases[0][1], cases[0][2]
    d_ids, d_oo = on_device(ids.astype(np.uint32), oo)
    sp = made_up_spans(len(ids))
    d_sp = dev(sp.reshape(-1), np.uint32)
    flags = FIXED | OVERFLOW | EVERY
    exp = expected_pairs(ids, oo, 8, ONLY_SECOND, 1, 2, 0, PAD, HEAD, SEP, TAIL, flags, sp)
    good, got = pairs_of(eng, d_ids, d_oo, len(ids), 8, ONLY_SECOND, 1, 2, 0, flags, d_sp)
    assert_same(got, exp)
    for what, _, coo, T, strategy, s, F, m, head, sep, tail, fl in cases:
        real = len(coo) == len(oo) or what in ("ids without a part", "an odd part count")
        d_coo = d_oo if real else dev(np.array(coo, np.uint64), np.uint64)
        with pytest.raises(tk.TokenizerError) as e:
            eng.pair_from_ids_device(d_ids.data_ptr(), d_coo.data_ptr(), len(coo) - 1, len(ids) if real else int(coo[-1]), T, strategy, s, F, m, PAD,
                                     head, sep, tail, flags=fl, stream=stream)
        assert e.value.code == tk.TK_ERR_INVALID_ARG, (what, str(e.value))
        assert_same(fetch(good), exp, ("the earlier result after", what))
    # the fused entries: the options are refused before anything is encoded, an odd part count behind it
    data, offs = pack([b"hello", b"hello world", b"a"])
    d_bytes, d_offs = torch.from_numpy(data).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda()
    for n_parts, T, strategy, s, fl in ((2, 3, LONGEST_FIRST, 0, 0), (2, 8, 3, 0, 0), (2, 8, LONGEST_FIRST, 1, 0), (2, 8, ONLY_FIRST, 0, 128), (3, 8, ONLY_FIRST, 0, 0)):
        with pytest.raises(tk.TokenizerError) as e:
            eng.encode_pairs_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_parts, int(offs[n_parts]), T, strategy, s, 0, 0, PAD, HEAD, SEP, TAIL,
                                    flags=fl, stream=stream)
        assert e.value.code == tk.TK_ERR_INVALID_ARG, (n_parts, T, strategy, s, fl)
        with pytest.raises(tk.TokenizerError) as e:
            eng.encode_pairs(data[:int(offs[n_parts])], offs[:n_parts + 1], T, strategy, s, 0, 0, PAD, HEAD, SEP, TAIL, flags=fl)
        assert e.value.code == tk.TK_ERR_INVALID_ARG, (n_parts, T, strategy, s, fl)
    assert_same(fetch(good), exp, "the earlier result after the fused entries' errors")
