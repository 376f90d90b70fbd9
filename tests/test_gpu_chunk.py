"""Boundary-aware token-budget chunks on the GPU (include/tekken_hip.h tk_chunk_from_ids_device, tk_chunk_levels_device and the
entries around them, csrc/tk_chunk.hip) against the plain-loop restatement of the definition in tests/test_chunk_cpu.py -- element
by element over every output, never through a sum."""
import json

import numpy as np
import pytest

import helpers
from helpers import dev, on_device, to_host
from test_chunk_cpu import (ALL_LEVELS, BYTES, CUT_LAST, FIXED, I64, LINE, MASK, PARAGRAPH, SENTENCE, SPANS, TOKEN, WORD, expected_chunks,
                            expected_levels_batch, refused_cases)
from test_gpu_spans import pack, sweep_docs
from test_gpu_window import fetch as window_fetch
from test_gpu_window import long_row_docs, made_up

pytestmark = pytest.mark.gpu

ARRAYS = ("input_ids", "mask", "lengths", "window_doc", "window_start", "doc_windows", "spans", "cut_level", "chunk_bytes", "level_counts")
COUNTS = ("n_windows", "n_split", "row_len")
PAD = 5


def fetch(res):
    """ChunkResult -> dict like expected_chunks's."""
    dt = np.int64 if res.typestr == "<i8" else np.int32
    W, L = res.n_windows, res.row_len
    v = res.views()
    return {"input_ids": to_host(v[0], (W, L), dt), "mask": to_host(v[1], (W, L), np.uint8), "lengths": to_host(v[2], (W,), np.uint32),
            "window_doc": to_host(v[3], (W,), np.uint32), "window_start": to_host(v[4], (W,), np.uint32),
            "doc_windows": to_host(v[5], (res.n_docs + 1,), np.uint64), "spans": to_host(v[6], (W, L, 2), np.uint32),
            "cut_level": to_host(v[7], (W,), np.uint8), "chunk_bytes": to_host(v[8], (W, 2), np.uint32),
            "level_counts": to_host(v[9], (6,), np.uint64), "n_windows": W, "n_split": res.n_split, "row_len": L}


def assert_same(got, exp, what=""):
    helpers.assert_same(got, exp, what, COUNTS, ARRAYS)


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def chunks_of(eng, d_ids, d_oo, n_ids, d_lev, T, m, o, h, t, mo, flags, d_spans=None, pad_id=PAD):
    res = eng.chunk_from_ids_device(d_ids.data_ptr(), d_oo.data_ptr(), d_oo.numel() - 1, n_ids, d_lev.data_ptr() if d_lev is not None else 0, T, m, o,
                                    mo, pad_id, h, t, flags, d_spans.data_ptr() if d_spans is not None else 0, stream())
    return res, fetch(res)


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
    # every byte is a token but "hello" (266); with BOS / EOS c = 10 and min_length 5: the first chunk ends behind the sentence
    # (the break in front of "Three"), the second behind the empty line, and the third holds the rest
    docs = ["One two. Three\n\nhello five", "", "hello"]
    r = t.encode_batch_chunks(docs, max_length=12, add_bos=True, add_eos=True, return_offsets_mapping=True, return_text=True)
    assert r["input_ids"].tolist() == [[1, 89, 120, 111, 42, 126, 129, 121, 56, 42, 2, P], [1, 94, 114, 124, 111, 111, 20, 20, 2, P, P, P],
                                       [1, 266, 42, 112, 115, 128, 111, 2, P, P, P, P], [1, 2] + [P] * 10, [1, 266, 2] + [P] * 9]
    assert r["attention_mask"].tolist() == [[1] * n + [0] * (12 - n) for n in (11, 9, 8, 2, 3)]
    assert r["lengths"].tolist() == [11, 9, 8, 2, 3] and r["overflow_to_sample_mapping"].tolist() == [0, 0, 0, 1, 2]
    assert r["window_start"].tolist() == [1, 10, 17, 1, 1] and r["doc_windows"].tolist() == [0, 3, 4, 5]
    assert r["cut_level"].tolist() == [SENTENCE, PARAGRAPH, CUT_LAST, CUT_LAST, CUT_LAST]
    assert r["chunk_bytes"].tolist() == [[0, 9], [9, 16], [16, 26], [0, 0], [0, 5]] and r["level_counts"].tolist() == [0, 0, 0, 1, 0, 1]
    assert r["texts"] == ["One two. ", "Three\n\n", "hello five", "", "hello"] and (r["n_windows"], r["n_split"]) == (5, 1)
    assert r["offset_mapping"][1].tolist() == [[0, 0], [9, 10], [10, 11], [11, 12], [12, 13], [13, 14], [14, 15], [15, 16], [26, 26], [0, 0], [0, 0], [0, 0]]
    assert isinstance(r["input_ids"], torch.Tensor) and r["input_ids"].dtype == torch.int64 and r["cut_level"].dtype == torch.uint8
    # without BOS / EOS at the same budget of text ids (c = 10 again: max_length 10, min_length 5), longest rows, int32, numpy
    r = t.encode_batch_chunks(docs, max_length=10, padding="longest", dtype="int32", return_tensors="np", pad_id=77, return_text=True)
    assert r["input_ids"].tolist() == [[89, 120, 111, 42, 126, 129, 121, 56, 42, 77], [94, 114, 124, 111, 111, 20, 20, 77, 77, 77],
                                       [266, 42, 112, 115, 128, 111, 77, 77, 77, 77], [77] * 10, [266] + [77] * 9]
    assert r["input_ids"].dtype == np.int32 and r["offset_mapping"] is None and r["lengths"].tolist() == [9, 7, 6, 0, 1]
    assert r["window_start"].tolist() == [0, 9, 16, 0, 0] and r["cut_level"].tolist() == [SENTENCE, PARAGRAPH, CUT_LAST, CUT_LAST, CUT_LAST]
    assert r["chunk_bytes"].tolist() == [[0, 9], [9, 16], [16, 26], [0, 0], [0, 5]] and r["texts"] == ["One two. ", "Three\n\n", "hello five", "", "hello"]
    # only word breaks count: the sentence and the paragraph are word breaks like the others, and the LAST one in reach wins
    r = t.encode_batch_chunks(docs[:1], max_length=10, levels=("word",), return_tensors="np", return_text=True)
    assert r["texts"] == ["One two. ", "Three\n\nhello ", "five"] and r["cut_level"].tolist() == [WORD, WORD, CUT_LAST]
    # no kind of break counts: every cut is a token break at the budget, and the overlap starts at a token
    r = t.encode_batch_chunks(docs[:1], max_length=10, levels=(), min_length=4, overlap=3, return_tensors="np", return_text=True)
    assert r["texts"] == ["One two. T", ". Three\n\nhello", "\n\nhello five"] and r["cut_level"].tolist() == [TOKEN, TOKEN, CUT_LAST]
    assert r["window_start"].tolist() == [0, 7, 14]
    # an overlap of up to 4 ids snaps to the word break in front of the cut: the blank in front of "Three", the empty line
    r = t.encode_batch_chunks(docs[:1], max_length=10, overlap=4, return_tensors="np", return_text=True)
    assert r["texts"] == ["One two. ", " Three\n\n", "\n\nhello five"] and r["cut_level"].tolist() == [SENTENCE, PARAGRAPH, CUT_LAST]
    assert r["window_start"].tolist() == [0, 8, 14]
    with pytest.raises(tk.TokenizerError) as e:
        t.encode_batch_chunks(docs, 10, levels=("clause",))
    assert e.value.code == tk.TK_ERR_INVALID_ARG
    with pytest.raises(tk.TokenizerError) as e:
        t.encode_batch_chunks(docs, 10, overlap=5, min_length=5)
    assert e.value.code == tk.TK_ERR_INVALID_ARG
    with pytest.raises(tk.TokenizerError) as e:
        t.encode_batch_chunks(docs, 2, add_bos=True, add_eos=True)
    assert e.value.code == tk.TK_ERR_INVALID_ARG


# ---- made-up ids and levels through tk_chunk_from_ids_device ----

# (T, m, o, h, t): candidate ranges c - m + 1 of 1, 63, 64, 65 and 129; overlaps of 0, 1, 63 and 64; T = 6 and T = 512; T = 7 with
# multiple_of 0: L % 4 != 0
SHAPES = ((6, 4, 0, 1, 1), (6, 2, 1, 0, 0), (7, 3, 1, 0, 0), (512, 448, 63, 1, 1), (512, 449, 64, 0, 0), (512, 446, 1, 1, 1), (512, 382, 0, 1, 1),
          (512, 382, 64, 1, 1))
_cases = {}


def case(shape):
    """(ids, oo, lev, spans, expected_chunks of them) of one shape: computed once, shared, never changed."""
    if shape not in _cases:
        T, m, o, h, t = shape
        ids, oo = made_up(T)
        rng = np.random.default_rng(61)
        # strong breaks are rare, as in text: about half of the candidate ranges of 129 hold no paragraph break, so the scans go
        # through every block of a range, end early, and find their best in any block
        lev = rng.choice(6, len(ids), p=[0.3, 0.55, 0.1, 0.03, 0.015, 0.005]).astype(np.uint8)
        g = np.arange(len(ids), dtype=np.uint64)
        sp = np.stack([(g * 2 + 1) & 0xFFFFFFFF, (g * 3 + 7) & 0xFFFFFFFF], axis=1).astype(np.uint32)   # index-derived: a wrong source index shows
        _cases[shape] = (ids, oo, lev, sp, expected_chunks(ids, oo, lev, T, m, o, h, t, 0, PAD, FIXED | MASK | SPANS | BYTES, sp))
    return _cases[shape]


ROWS_TILE = 2048                   # csrc/tk_rows.h TKY_ROWS_TILE: units of a block's row group
OWNERS_CAP = 1024                  # csrc/tk_layout.h TKY_CAP: owners of a row group that LDS holds
UNSTAGED = (4, 2, 0, 0, 0)         # L = 4: one unit a row, ROWS_TILE rows a block
_unstaged = []


def unstaged_case():
    """(ids, oo, lev, spans, expected_chunks of them): 3 000 one-id documents between two split ones, at UNSTAGED."""
    if not _unstaged:
        T, m, o, h, t = UNSTAGED
        rng = np.random.default_rng(63)
        oo = np.concatenate([[0], np.cumsum([9] + [1] * 3000 + [9])]).astype(np.int64)
        ids = rng.integers(0, 2**31 - 1, int(oo[-1])).astype(np.uint32)
        lev = rng.integers(0, 6, len(ids)).astype(np.uint8)
        g = np.arange(len(ids), dtype=np.uint64)
        sp = np.stack([(g * 2 + 1) & 0xFFFFFFFF, (g * 3 + 7) & 0xFFFFFFFF], axis=1).astype(np.uint32)
        _unstaged.append((ids, oo, lev, sp, expected_chunks(ids, oo, lev, T, m, o, h, t, 0, PAD, FIXED | MASK | SPANS | BYTES, sp)))
    return _unstaged[0]


def most_owners_of_a_row_group(e):
    """The largest number of documents that start inside one row group of the fill, behind the group's first row: what
    TkyRowOwners stages unless it is more than OWNERS_CAP.  The shape is csrc/tk_rows.h tky_rows_shape's."""
    L, W = e["row_len"], e["n_windows"]
    units = L // 4 if L and L % 4 == 0 else max(L, 1)
    rb = ROWS_TILE // units if units <= ROWS_TILE else 1
    dw = e["doc_windows"].astype(np.int64)[:-1]
    return max((int(np.sum((dw > r0) & (dw < min(r0 + rb, W)))) for r0 in range(0, W, rb)), default=0)


def test_the_case_set_holds_what_it_is_for():
    """From expected_chunks's results alone.  The fill's unstaged branch (more than 1 024 documents start inside one row group)
    needs one unit a row, L = 4 or L = 1, which no shape of SHAPES has at any multiple_of the tests use: over made_up()'s block of
    3 000 one-id documents their most are 1 023 documents at L = 8 (T = 6 and 7 at multiple_of 4: 1 024 rows a block), 340 at
    L = 6, 291 at L = 7, 127 at L = 64 and 15 at L = 512, and no other test of this file has more (L = 16; L = 0 over 5 rows).  The
    window tests reach it with the same block at T = 4.  unstaged_case() is here for it."""
    seen = set()
    assert most_owners_of_a_row_group(unstaged_case()[4]) > OWNERS_CAP
    seen.add("a row group of more than 1 024 documents")
    for shape in SHAPES:
        T, m, o, h, t = shape
        ids, oo, lev, sp, e = case(shape)
        seen.add(("range", T - h - t - m + 1))
        seen.add(("overlap", o))
        n, w = np.diff(oo), np.diff(e["doc_windows"].astype(np.int64))
        assert np.all(w[n == T] == 1) and np.sum(n == T) >= 1 and np.all(w[n == T + 1] == 2) and np.sum(n == T + 1) >= 1
        assert n.max() == 50_001 and np.any((w[:-2] > 1) & (n[1:-1] == 0) & (w[2:] > 1)) and e["level_counts"].sum() == e["n_windows"] - len(n)
        if e["row_len"] % 4:
            seen.add("L % 4 != 0")
        if np.all(e["level_counts"] > 0):
            seen.add("a cut at every level")
        assert most_owners_of_a_row_group(e) <= OWNERS_CAP
    assert seen >= {("range", r) for r in (1, 63, 64, 65, 129)} | {("overlap", o) for o in (0, 1, 63, 64)} | {"L % 4 != 0", "a cut at every level",
                                                                                                             "a row group of more than 1 024 documents"}


@pytest.mark.parametrize("shape", SHAPES)
def test_walk_on_made_up_levels(tk, eng_bench, shape):
    T, m, o, h, t = shape
    ids, oo, lev, sp, exp = case(shape)
    d_ids, d_oo = on_device(ids, oo)
    d_lev, d_sp = dev(lev, np.uint8), dev(sp.reshape(-1), np.uint32)
    flags = FIXED | MASK | SPANS | BYTES
    _, got = chunks_of(eng_bench, d_ids, d_oo, len(ids), d_lev, T, m, o, h, t, 0, flags, d_sp)
    assert_same(got, exp, shape)
    # int64 equals int32 value for value; an unselected output is NULL and the rest is unchanged; longest rows; multiple_of
    for f, mo in ((flags | I64, 0), (FIXED | I64, 0), (MASK, 64), (BYTES, 0), (SPANS | I64, 4)):
        res, g = chunks_of(eng_bench, d_ids, d_oo, len(ids), d_lev, T, m, o, h, t, mo, f, d_sp if f & (SPANS | BYTES) else None)
        assert (res.mask_ptr is None) == (not f & MASK) and (res.spans_ptr is None) == (not f & SPANS) and (res.chunk_bytes_ptr is None) == (not f & BYTES)
        assert g["input_ids"].dtype == (np.int64 if f & I64 else np.int32) and g["row_len"] == -(-T // (mo or 1)) * (mo or 1)
        want = {**exp, "row_len": g["row_len"]}
        for k, bit in (("mask", MASK), ("spans", SPANS), ("chunk_bytes", BYTES)):
            if not f & bit:
                want[k] = None
        if mo:                                          # the rows of the FIXED case, and pads behind them
            L = g["row_len"]
            assert np.all(g["input_ids"][:, T:] == PAD) and (g["mask"] is None or not g["mask"][:, T:].any())
            g = {**g, "input_ids": g["input_ids"][:, :T], "mask": None if g["mask"] is None else g["mask"][:, :T],
                 "spans": None if g["spans"] is None else g["spans"][:, :T], "row_len": L}
        assert_same({**g, "input_ids": np.ascontiguousarray(g["input_ids"]).astype(np.int32)}, want, (shape, f, mo))


def test_split_documents_at_the_end_and_start_of_a_waves_group(tk, eng_bench):
    """70 000 documents, so that a wave of the walk takes 64: split documents as the 64th of a group, the 65th (the first of the
    next), both, and a whole group of them; unsplit ones of every length up to T between them."""
    rng = np.random.default_rng(62)
    T, m, o, h, t = 16, 6, 3, 1, 1
    n = np.zeros(70_000, np.int64)
    n[:2000] = rng.integers(0, T + 1, 2000)
    for d in (63, 64, 127, 192, 64 * 9 + 63, 64 * 9 + 64, 69_999 - 64, 69_999):
        n[d] = int(rng.integers(T + 1, 400))
    n[64 * 20:64 * 21] = rng.integers(T + 1, 120, 64)
    oo = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    ids = rng.integers(0, 2**31 - 1, int(oo[-1])).astype(np.uint32)
    lev = rng.integers(0, 6, len(ids)).astype(np.uint8)
    exp = expected_chunks(ids, oo, lev, T, m, o, h, t, 0, PAD, FIXED | MASK)
    assert exp["n_split"] == 8 + 64
    d_ids, d_oo = on_device(ids, oo)
    _, got = chunks_of(eng_bench, d_ids, d_oo, len(ids), dev(lev, np.uint8), T, m, o, h, t, 0, FIXED | MASK)
    assert_same(got, exp)


@pytest.mark.parametrize("shape", [(6, 1, 1, 1), (512, 128, 1, 1)])
def test_all_token_levels_equal_the_window_pass(tk, eng_bench, shape):
    T, o, h, t = shape
    ids, oo = made_up(T)
    d_ids, d_oo = on_device(ids, oo)
    c = T - h - t
    for level, m in ((TOKEN, c), (TOKEN, o + 1), (PARAGRAPH, (c + o + 1) // 2)):      # (any level, as long as all are equal; any valid m)
        d_lev = dev(np.full(len(ids), level, np.uint8), np.uint8)
        for flags in (FIXED | MASK, I64):
            _, got = chunks_of(eng_bench, d_ids, d_oo, len(ids), d_lev, T, m, o, h, t, 0, flags)
            w = eng_bench.window_from_ids_device(d_ids.data_ptr(), d_oo.data_ptr(), len(oo) - 1, len(ids), T, o, 0, PAD, h, t, flags, 0, stream())
            v = w.views()
            W, L = w.n_windows, w.row_len
            assert (got["n_windows"], got["n_split"], got["row_len"]) == (W, w.n_split, L)
            dt = np.int64 if flags & I64 else np.int32
            for k, view, shp, dty in (("input_ids", v[0], (W, L), dt), ("mask", v[1], (W, L), np.uint8), ("lengths", v[2], (W,), np.uint32),
                                      ("window_doc", v[3], (W,), np.uint32), ("window_start", v[4], (W,), np.uint32),
                                      ("doc_windows", v[5], (len(oo),), np.uint64)):
                helpers.assert_array_same(got[k], to_host(view, shp, dty), (shape, level, m, flags, k))
            split = np.diff(got["doc_windows"].astype(np.int64)) > 1
            assert got["level_counts"].tolist() == [int(got["n_windows"] - len(split)) if l == level else 0 for l in range(6)]


def test_more_documents_in_a_row_group_than_lds_holds(tk, eng_bench):
    """The fill's unstaged branch: rows of one unit, 2 048 a block, over one-id documents -- the first row group has more than
    1 024 of them and reads their starts from global memory, the last one stages its own."""
    T, m, o, h, t = UNSTAGED
    ids, oo, lev, sp, exp = unstaged_case()
    assert exp["row_len"] == 4 and exp["n_split"] == 2
    d_ids, d_oo = on_device(ids, oo)
    d_lev, d_sp = dev(lev, np.uint8), dev(sp.reshape(-1), np.uint32)
    for fl in (FIXED | MASK | SPANS | BYTES, FIXED | MASK | SPANS | BYTES | I64):
        _, got = chunks_of(eng_bench, d_ids, d_oo, len(ids), d_lev, T, m, o, h, t, 0, fl, d_sp)
        assert_same({**got, "input_ids": got["input_ids"].astype(np.int32)}, exp, fl)


def test_row_longer_than_a_block_tile(tk, eng_bench):
    """T = 9 001 through the chunk fill: the units of one row are split over blockIdx.y, element by element (L = 9 001) and in units
    of 4 (L = 9 004).  Every level TOKEN and min_length = c: the chunks are the windows at stride = overlap, and every output the
    two passes share is compared with the window pass's too, the spans among them."""
    T, o, h, t = 9001, 100, 2, 3
    ids, oo, sp = long_row_docs()
    lev = np.full(len(ids), TOKEN, np.uint8)
    d_ids, d_oo = on_device(ids, oo)
    d_lev, d_sp = dev(lev, np.uint8), dev(sp.reshape(-1), np.uint32)
    flags = FIXED | MASK | SPANS | BYTES
    for mo in (0, 4):
        exp = expected_chunks(ids, oo, lev, T, T - h - t, o, h, t, mo, PAD, flags, sp)
        assert exp["row_len"] == T + 3 * (mo == 4) and exp["lengths"].max() == T and exp["n_split"] > 0
        for fl in (flags, flags | I64):
            _, got = chunks_of(eng_bench, d_ids, d_oo, len(ids), d_lev, T, T - h - t, o, h, t, mo, fl, d_sp)
            assert_same({**got, "input_ids": got["input_ids"].astype(np.int32)}, exp, (mo, fl))
            wfl = fl & ~BYTES                           # (the two passes number FIXED, I64, MASK and SPANS alike)
            w = window_fetch(eng_bench.window_from_ids_device(d_ids.data_ptr(), d_oo.data_ptr(), len(oo) - 1, len(ids), T, o, mo, PAD, h, t, wfl,
                                                              d_sp.data_ptr(), stream()))
            assert (got["n_windows"], got["n_split"], got["row_len"]) == (w["n_windows"], w["n_split"], w["row_len"])
            for k in ("input_ids", "mask", "lengths", "window_doc", "window_start", "doc_windows", "spans"):
                helpers.assert_array_same(got[k], w[k], (mo, fl, k))


# ---- the levels kernel ----

def levels_of(tk, eng, docs, bos, eos, mask):
    """(ids, oo, spans [N, 2], the kernel's levels) of docs encoded on the device."""
    import torch
    data, offs = pack(docs)
    d_bytes = torch.from_numpy(data if len(data) else np.zeros(1, np.uint8)).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    D = len(docs)
    p_ids, p_oo, p_sp, n = eng.encode_batch_device_spans(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), bos, eos, stream=stream())
    p_lev = eng.chunk_levels_device(p_sp, p_oo, D, n, d_bytes.data_ptr(), d_offs.data_ptr(), len(data), mask, stream())
    oo = to_host(tk.DeviceView(p_oo, D + 1, "<i8"), (D + 1,), np.uint64).copy()
    sp = to_host(tk.DeviceView(p_sp, 2 * n, "<i4"), (2 * n,), np.uint32).reshape(-1, 2).copy()
    ids = to_host(tk.DeviceView(p_ids, n, "<i4"), (n,), np.uint32).copy()
    return ids, oo, sp, to_host(tk.DeviceView(p_lev, n, "|u1"), (n,), np.uint8).copy()


@pytest.mark.parametrize("mask", [ALL_LEVELS, (1 << WORD) | (1 << LINE)])
def test_levels_kernel_against_the_rules(tk, eng_bench, mask):
    blank = b" \t\n" * 40 + b"\n\n" + b" " * 30
    text = ("First sentence. Second one!  Third?\n\nA new paragraph\n  indented 3.14 and eé.\n" "你好。再见！好？是" "\n").encode()
    sets = ([x for x in sweep_docs() if len(x) < 70000],                                             # malformed UTF-8 among them
            [blank, b"", b"", text, b" ", b"\n", text * 9, b"", blank + text] + [b""] * 40 + [text[:k] for k in range(0, 60)] + [b""])
    for docs in sets:
        for bos, eos in ((True, True), (False, False)):
            ids, oo, sp, got = levels_of(tk, eng_bench, docs, bos, eos, mask)
            exp = expected_levels_batch(docs, oo, sp, mask)
            helpers.assert_array_same(got, exp, (len(docs), bos, eos, mask))
            if bos and mask == ALL_LEVELS:                          # ids at p == 0 and at p == len are token breaks
                first, last = oo[:-1].astype(np.int64), oo[1:].astype(np.int64) - 1
                assert np.all(got[first] == TOKEN) and np.all(got[last] == TOKEN)
    with pytest.raises(tk.TokenizerError) as e:
        levels_of(tk, eng_bench, [b"a b"], False, False, 64)
    assert e.value.code == tk.TK_ERR_INVALID_ARG
    with pytest.raises(tk.TokenizerError) as e:
        levels_of(tk, eng_bench, [b"a b"], False, False, ALL_LEVELS | 2)
    assert e.value.code == tk.TK_ERR_INVALID_ARG


# ---- the fused and host entries ----

def test_composite_on_generated_documents(tk, eng_bench):
    import torch
    docs = [x for x in sweep_docs() if len(x) < 70000][:300] + [b"", b"tail"]
    data, offs = pack(docs)
    D = len(docs)
    d_bytes = torch.from_numpy(data).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    eng = eng_bench
    for i, (bos, eos, T, m, o, mask) in enumerate(((True, True, 64, 32, 8, ALL_LEVELS), (False, False, 48, 20, 0, ALL_LEVELS & ~(1 << SENTENCE)),
                                                   (True, False, 512, 256, 64, ALL_LEVELS))):
        flags = MASK | BYTES | (I64 if i & 1 else 0) | (FIXED if i != 1 else 0) | (SPANS if i != 2 else 0)
        p_ids, p_oo, n_ids, res = eng.encode_batch_device_chunk(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), T, m, o, bos, eos, 0, 7, mask, flags,
                                                                tk.CHECK_OFFSETS, stream())
        got = fetch(res)
        ids = to_host(tk.DeviceView(p_ids, n_ids, "<i4"), (n_ids,), np.uint32).copy()
        oo = to_host(tk.DeviceView(p_oo, D + 1, "<i8"), (D + 1,), np.uint64).copy()
        # restatement over restatement: the spans of tk_token_spans_device, the levels of the rules, the chunks of the definition
        p2_ids, p2_oo, p_sp, n = eng.encode_batch_device_spans(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), bos, eos, stream=stream())
        assert n == n_ids
        sp = to_host(tk.DeviceView(p_sp, 2 * n, "<i4"), (2 * n,), np.uint32).reshape(-1, 2).copy()
        lev = expected_levels_batch(docs, oo, sp, mask)
        exp = expected_chunks(ids, oo, lev, T, m, o, int(bos), int(eos), 0, 7, flags, sp)
        assert exp["n_split"] > 0 and exp["level_counts"][WORD:].sum() > 0
        assert_same(got, exp, (bos, eos, T))
        host = eng.encode_batch_chunk(data, offs, T, m, o, bos, eos, False, 0, 7, mask, flags)
        assert_same({**host, "row_len": host["input_ids"].shape[1]}, exp, ("host", bos, eos, T))
        assert all(x >= 0 for x in eng.last_chunk_ms())
    # the one-launch small path: the kernels read text, ids and offsets in mapped pinned memory; the device entry gives the same
    small = sweep_docs()[:60] + [b"", b"a", b"One two. Three\n\nFour five"]
    data, offs = pack(small)
    d_bytes = torch.from_numpy(data).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    flags = FIXED | MASK | SPANS | BYTES
    calls0 = eng.small_path_calls()
    host = eng.encode_batch_chunk(data, offs, 24, 8, 3, True, True, False, 0, 7, ALL_LEVELS, flags)
    assert eng.small_path_calls() > calls0
    _, _, _, res = eng.encode_batch_device_chunk(d_bytes.data_ptr(), d_offs.data_ptr(), len(small), len(data), 24, 8, 3, True, True, 0, 7, ALL_LEVELS, flags,
                                                 0, stream())
    assert res.n_split >= 60
    assert_same({**host, "row_len": host["input_ids"].shape[1]}, fetch(res), "the small path")


def test_outputs_outlive_each_other_and_refusals(tk, eng_bench, bench_vocab):
    import torch
    docs = [x for x in sweep_docs() if len(x) < 70000]
    data, offs = pack(docs)
    D = len(docs)
    d_bytes = torch.from_numpy(data).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    eng, st = eng_bench, stream()
    p_ids, p_oo, p_sp, n = eng.encode_batch_device_spans(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), True, True, stream=st)
    wflags = 1 | 4 | 8                                                       # the window pass: FIXED | MASK | SPANS
    win = eng.window_from_ids_device(p_ids, p_oo, D, n, 512, 128, 0, 7, 1, 1, wflags, p_sp, st)
    W = win.n_windows

    def snapshot():
        return (to_host(tk.DeviceView(p_ids, n, "<i4"), (n,), np.uint32).copy(), to_host(tk.DeviceView(p_oo, D + 1, "<i8"), (D + 1,), np.uint64).copy(),
                to_host(tk.DeviceView(p_sp, 2 * n, "<i4"), (2 * n,), np.uint32).copy(),
                to_host(tk.DeviceView(win.input_ids_ptr, (W, 512), "<i4"), (W, 512), np.int32).copy(),
                to_host(tk.DeviceView(win.mask_ptr, (W, 512), "|u1"), (W, 512), np.uint8).copy(),
                to_host(tk.DeviceView(win.spans_ptr, (W, 512, 2), "<i4"), (W, 512, 2), np.uint32).copy(),
                to_host(tk.DeviceView(win.window_start_ptr, W, "<i4"), (W,), np.uint32).copy(),
                to_host(tk.DeviceView(win.doc_windows_ptr, D + 1, "<i8"), (D + 1,), np.uint64).copy())

    before = snapshot()
    ids, oo, sp = before[0], before[1], before[2].reshape(-1, 2)
    p_lev = eng.chunk_levels_device(p_sp, p_oo, D, n, d_bytes.data_ptr(), d_offs.data_ptr(), len(data), ALL_LEVELS, st)
    lev = to_host(tk.DeviceView(p_lev, n, "|u1"), (n,), np.uint8).copy()
    flags = FIXED | MASK | SPANS | BYTES
    good = eng.chunk_from_ids_device(p_ids, p_oo, D, n, p_lev, 512, 256, 64, 0, 7, 1, 1, flags, p_sp, st)
    ptrs = {good.input_ids_ptr, good.mask_ptr, good.spans_ptr, good.lengths_ptr, good.window_doc_ptr, good.window_start_ptr, good.doc_windows_ptr,
            good.cut_level_ptr, good.chunk_bytes_ptr, good.level_counts_ptr, p_lev, win.input_ids_ptr, win.mask_ptr, win.spans_ptr, win.lengths_ptr,
            win.window_doc_ptr, win.window_start_ptr, win.doc_windows_ptr, p_ids, p_oo, p_sp}
    assert len(ptrs) == 21 and None not in ptrs and 0 not in ptrs
    exp = expected_chunks(ids, oo, lev, 512, 256, 64, 1, 1, 0, 7, flags, sp)
    assert exp["n_split"] > 0
    assert_same(fetch(good), exp)
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a, b)
    # every refused case: TK_ERR_INVALID_ARG, and the first chunk result stays readable (the offsets of the cases are read, never
    # ids or levels behind them: no case that reaches the walk has a document to split)
    for what, _, coo, clev, T, m, o, h, t, mo, fl, on_device_too in refused_cases():
        if not on_device_too:
            continue
        real = len(coo) == 5 or what == "ids without a document"      # the cases over the four hand-made documents: any real ids do
        d_oo = dev(np.array(coo, np.uint64), np.uint64)
        with pytest.raises(tk.TokenizerError) as e:
            eng.chunk_from_ids_device(p_ids, d_oo.data_ptr(), 0 if what == "ids without a document" else len(coo) - 1,
                                      int(coo[-1]) if not real else 29 if len(coo) == 5 else n, 0 if clev is None else p_lev, T, m, o, mo, 7, h, t, fl, 0, st)
        assert e.value.code == tk.TK_ERR_INVALID_ARG, (what, str(e.value))
        assert_same(fetch(good), exp, ("the earlier result after", what))
    for bos, eos, T, m, o in ((True, True, 2, 1, 0), (True, False, 1, 1, 0), (True, True, 8, 7, 0), (True, True, 8, 3, 3), (False, False, 0, 1, 0),
                              (False, False, 8, 0, 0)):
        with pytest.raises(tk.TokenizerError) as e:
            eng.encode_batch_device_chunk(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), T, m, o, bos, eos, stream=st)
        assert e.value.code == tk.TK_ERR_INVALID_ARG, (bos, eos, T, m, o)
    with pytest.raises(tk.TokenizerError) as e:
        eng.encode_batch_device_chunk(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), 64, 32, 8, levels=1, stream=st)
    assert e.value.code == tk.TK_ERR_INVALID_ARG
    with pytest.raises(tk.TokenizerError) as e:
        eng.encode_batch_chunk(data, offs, 64, 32, 0, True, True, flags=64)
    assert e.value.code == tk.TK_ERR_INVALID_ARG
    assert_same(fetch(good), exp, "the earlier result after the fused entries' errors")
    # the composite entry encodes again and runs the spans pass into a buffer of its own: tk_token_spans_device's result and the
    # window result are as they were
    eng.encode_batch_device_chunk(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), 64, 32, 8, True, True, flags=SPANS | BYTES, stream=st)
    for a, b in zip(before[2:], snapshot()[2:]):
        assert np.array_equal(a, b)


def test_empty_shapes(tk, eng_bench):
    eng = eng_bench
    z1 = np.zeros(1, np.int64)
    zsp = dev(np.zeros(2, np.uint32), np.uint32)
    for flags in (MASK, FIXED | I64 | MASK | SPANS | BYTES, FIXED, BYTES):
        for mo in (0, 8):
            for oo in (z1, np.zeros(6, np.int64)):                   # D = 0; all-empty documents
                d_ids, d_oo = on_device(np.zeros(0, np.uint32), oo)
                _, got = chunks_of(eng, d_ids, d_oo, 0, None, 6, 2, 1, 1, 1, mo, flags, zsp, pad_id=9)
                sp = np.zeros((0, 2), np.uint32)
                assert_same(got, expected_chunks([], oo, [], 6, 2, 1, 1, 1, mo, 9, flags, sp), (flags, mo, len(oo)))
        host = eng.encode_batch_chunk(np.zeros(0, np.uint8), np.zeros(1, np.uint64), 6, 2, 1, True, True, pad_id=9, flags=flags)
        assert_same({**host, "row_len": host["input_ids"].shape[1]}, expected_chunks([], z1, [], 6, 2, 1, 1, 1, 0, 9, flags, np.zeros((0, 2), np.uint32)),
                    ("host", flags))
    # the hand-made walk of tests/test_chunk_cpu.py
    rows = [[1] + list(range(20, 30)) + [2], [1, 30, 2], []]
    oo = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    ids = np.array([i for r in rows for i in r], np.uint32)
    lev = np.array([1] + [1, 1, 2, 1, 1, 2, 1, 1, 1, 1] + [1] + [1, 1, 1], np.uint8)
    d_ids, d_oo = on_device(ids, oo)
    res, got = chunks_of(eng, d_ids, d_oo, len(ids), dev(lev, np.uint8), 6, 2, 1, 1, 1, 0, FIXED, pad_id=9)
    assert got["input_ids"].tolist() == [[1, 20, 21, 2, 9, 9], [1, 21, 22, 23, 24, 2], [1, 24, 25, 26, 27, 2], [1, 27, 28, 29, 2, 9], [1, 30, 2, 9, 9, 9], [9] * 6]
    assert got["window_start"].tolist() == [1, 2, 5, 8, 1, 0] and got["cut_level"].tolist() == [WORD, WORD, TOKEN, CUT_LAST, CUT_LAST, CUT_LAST]
    assert got["level_counts"].tolist() == [0, 1, 2, 0, 0, 0] and res.n_split == 1 and got["doc_windows"].tolist() == [0, 4, 5, 6]
    lev9 = np.array([1, 1, 1, 9, 1, 5, 1, 1, 1], np.uint8)                   # a level byte above 5 reads as 5
    d_ids, d_oo = on_device(np.arange(100, 109).astype(np.uint32), np.array([0, 9], np.int64))
    _, got = chunks_of(eng, d_ids, d_oo, 9, dev(lev9, np.uint8), 6, 3, 0, 0, 0, 0, FIXED)
    assert got["window_start"].tolist() == [0, 5] and got["cut_level"].tolist() == [PARAGRAPH, CUT_LAST] and got["level_counts"].tolist() == [0, 0, 0, 0, 0, 1]
