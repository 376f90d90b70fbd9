"""Masked-LM and span-corruption rows on the GPU (include/tekken_hip.h tk_noise_replace_device / tk_noise_spans_device and the entries
around them, csrc/tk_noise.hip) against the plain-loop restatement of the definition in tests/test_noise_cpu.py -- every output
and counter bit for bit, both modes, both units, drawn choices and given ones, at the shapes where the tiles of the kernels end."""
import ctypes
import json

import numpy as np
import pytest

import helpers
from helpers import dev, to_host
from test_noise_cpu import (ACCEPTED_SPANS, DESC, JOINED, NONE, ONE, REFUSED_REPLACE, REFUSED_SPANS, REPLACE_ARRAYS, REPLACE_COUNTS, S0, SELECTED,
                            SPANS_ARRAYS, SPANS_COUNTS, SPLIT, TOKEN, V, WORD, expected_noise_replace, expected_noise_spans, noise_opts, pack,
                            word_ids_of)

pytestmark = pytest.mark.gpu

BOTH = SPLIT | JOINED


@pytest.fixture(scope="module")
def eng(tk, test_vocab):
    assert (test_vocab["num_special"], test_vocab["num_special"] + len(test_vocab["tokens"])) == (S0, V)
    e = tk.Engine(test_vocab["tokens"], test_vocab["num_special"], test_vocab["bos"], test_vocab["eos"], device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def T(tk):
    return int(tk.lib().tk_noise_tile())


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def fetch_replace(res):
    v = res.views()
    out = {"input_ids": to_host(v[0], res.n_ids, np.uint32), "labels": to_host(v[1], res.n_ids, np.int32), "selected": to_host(v[2], res.n_ids, np.uint8)}
    out.update({k: getattr(res, k) for k in REPLACE_COUNTS})
    return out


def fetch_spans(res):
    v, D, n = res.views(), res.n_docs, res.n_inputs + res.n_targets
    shapes = (res.n_inputs, D + 1, res.n_targets, D + 1, n, D + 1, n)
    types = (np.uint32, np.uint64, np.uint32, np.uint64, np.uint32, np.uint64, np.int32)
    out = {k: to_host(x, s, t) for k, x, s, t in zip(SPANS_ARRAYS, v, shapes, types)}
    out.update({k: getattr(res, k) for k in SPANS_COUNTS})
    return out


def ptr(t, n=1):
    return t.data_ptr() if t is not None and n else 0


def run(eng, mode, ids, offs, o, word_ids=None, sel=None, what=""):
    """One device call over host arrays against the restatement; -> the expected dict."""
    d_ids, d_oo = dev(ids, np.uint32), dev(offs, np.uint64)
    d_w = None if word_ids is None else dev(word_ids, np.uint32)
    d_s = None if sel is None else dev(sel, np.uint8)
    call = eng.noise_replace_device if mode == "replace" else eng.noise_spans_device
    res = call(ptr(d_ids, len(ids)), d_oo.data_ptr(), len(offs) - 1, len(ids), 0 if d_w is None else d_w.data_ptr(),
               0 if d_s is None else d_s.data_ptr(), stream(), **o)
    if mode == "replace":
        exp = expected_noise_replace(ids, offs, o, word_ids, sel)
        helpers.assert_same(fetch_replace(res), exp, (what, o), REPLACE_COUNTS, REPLACE_ARRAYS)
    else:
        exp = expected_noise_spans(ids, offs, o, word_ids, sel)
        helpers.assert_same(fetch_spans(res), exp, (what, o), SPANS_COUNTS, SPANS_ARRAYS)
    return exp


def both_modes(eng, ids, offs, word_ids=None, sel=None, what="", spans_flags=(BOTH,), n_sentinels=100, **kw):
    """The same choice through replace mode and through spans mode; -> replace mode's expected dict."""
    r = run(eng, "replace", ids, offs, noise_opts(mask_q32=ONE // 2, random_q32=ONE // 4, mask_id=4, flags=SELECTED, **kw), word_ids, sel, what)
    for fl in spans_flags:
        run(eng, "spans", ids, offs, noise_opts(n_sentinels=n_sentinels, sentinel_first=100, final_id=2, flags=fl, **kw), word_ids, sel, what)
    return r


def ramp(n, salt=0, special_every=0):
    """n ordinary ids that tell where they came from; special_every: a special id at every such position."""
    x = (np.arange(n, dtype=np.int64) * 7 + salt) % (V - S0) + S0
    if special_every:
        x[special_every - 1::special_every] = 5
    return x.tolist()


def tile_docs(T):
    return [ramp(T - 1, 1), [], ramp(1, 2), ramp(T, 3), [], [], ramp(T + 1, 4, 97), ramp(1, 5), ramp(2 * T + 3, 6, 211), [], ramp(5, 7)]


# ---- the shapes ----

def test_no_document_and_no_id(eng):
    for docs in ([], [[], [], []]):
        ids, offs = pack(docs)
        r = run(eng, "replace", ids, offs, noise_opts(start_q32=ONE, mask_q32=ONE, flags=SELECTED))
        assert r["n_selected"] == 0
        for fl in (SPLIT, JOINED, BOTH):
            for fin in (NONE, 2):
                r = run(eng, "spans", ids, offs, noise_opts(start_q32=ONE, n_sentinels=3, final_id=fin, flags=fl))
                assert r["n_targets"] == (len(docs) if fin != NONE else 0)


@pytest.mark.parametrize("unit", [TOKEN, WORD])
def test_documents_around_the_tile_size_drawn(eng, T, unit):
    docs = tile_docs(T)
    ids, offs = pack(docs)
    w = word_ids_of(np.random.default_rng(3), docs) if unit == WORD else None
    for seed, span, sq in ((0, (1, 1), 1 << 29), (1, (1, 5), 1 << 28), (2, (3, 3), 1 << 27)):
        r = both_modes(eng, ids, offs, w, seed=seed, unit=unit, span_min=span[0], span_max=span[1], start_q32=sq, what="drawn")
        assert 0 < r["n_selected"] < len(ids)


def test_all_selected_and_none_selected(eng, T):
    docs = tile_docs(T)
    ids, offs = pack(docs)
    r = both_modes(eng, ids, offs, start_q32=ONE, span_max=2, spans_flags=(SPLIT, JOINED, BOTH))
    assert r["n_selected"] == int(np.sum(ids >= S0))
    r = both_modes(eng, ids, offs, start_q32=0)
    assert r["n_selected"] == 0 and np.array_equal(r["input_ids"], ids)
    both_modes(eng, ids, offs, sel=np.ones(len(ids), np.uint8))
    both_modes(eng, ids, offs, sel=np.zeros(len(ids), np.uint8))


def test_given_runs_on_tile_and_document_borders(eng, T):
    n = 3 * T + 7
    docs = [ramp(n, 1), ramp(T, 2), ramp(T, 3), ramp(9, 4)]
    ids, offs = pack(docs)
    sel = np.zeros(len(ids), np.uint8)
    sel[T - 3:T + 2] = 1                                # a run that crosses a tile border
    sel[2 * T - 4:2 * T] = 1                            # one that ends exactly at a border
    sel[3 * T:3 * T + 2] = 1                            # one that starts on a border
    sel[n - 2:n + 3] = 1                                # the document's last ids and the next one's first: two runs
    sel[n + T - 1:n + T + 1] = 1                        # the same with the document boundary on a tile border + 7
    sel[n + 2 * T - 1:n + 2 * T + 1] = 1
    sel[-1] = 1
    for n_sent in (100, 0, 1, 3):
        for fl, first in ((BOTH, 100), (BOTH | DESC, 300)):
            for fin in (2, NONE):
                r = run(eng, "spans", ids, offs, noise_opts(n_sentinels=n_sent, sentinel_first=first, final_id=fin, flags=fl), sel=sel)
        assert r["n_runs"] + r["n_runs_dropped"] == 10
    run(eng, "replace", ids, offs, noise_opts(mask_q32=ONE, mask_id=6999, flags=SELECTED), sel=sel)
    # documents that start on every tile border, selected at both ends
    docs = [ramp(T, i) for i in range(4)]
    ids, offs = pack(docs)
    sel = np.zeros(len(ids), np.uint8)
    for d in range(4):
        sel[d * T] = sel[d * T + T - 1] = 1
    r = run(eng, "spans", ids, offs, noise_opts(n_sentinels=1, sentinel_first=7, final_id=2, flags=BOTH), sel=sel)
    assert (r["n_runs"], r["n_runs_dropped"]) == (4, 4)


def test_spans_that_cross_tile_borders_the_halo(eng, T):
    docs = [ramp(2 * T + 3, 1, 131), ramp(T - 30, 2), ramp(40, 3), ramp(T + 1, 4)]
    ids, offs = pack(docs)
    for seed, lo, hi, sq in ((0, 64, 64, 1 << 27), (1, 1, 64, 1 << 28), (2, 40, 64, 1 << 27), (3, 2, 2, 3 << 30)):
        r = both_modes(eng, ids, offs, seed=seed, span_min=lo, span_max=hi, start_q32=sq, what="halo")
        s = r["selected"]
        assert any(s[b - 1] and s[b] for b in (T, 2 * T, 3 * T)), "no span crossed a border: the case shows nothing"


def test_word_units_whose_words_cross_tile_borders(eng, T):
    n = 2 * T + 50
    docs = [ramp(n, 1), ramp(T - 50 + 6, 2), ramp(20, 3)]
    ids, offs = pack(docs)
    w = np.concatenate([np.arange(len(d)) // 6 for d in docs]).astype(np.uint32)      # words of 6 ids: T is no multiple of 6
    w[ids < S0] = NONE
    w[5] = NONE
    for seed in (0, 1):
        r = both_modes(eng, ids, offs, w, seed=seed, unit=WORD, span_min=1, span_max=3, start_q32=1 << 31, what="words")
        s = r["selected"]
        assert any(s[b - 1] and s[b] and w[b - 1] == w[b] for b in (T, 2 * T))
    # word ids in any order are the caller's business: the definition is per id
    rng = np.random.default_rng(0)
    both_modes(eng, ids, offs, rng.integers(0, 50, len(ids)).astype(np.uint32), unit=WORD, span_max=64, start_q32=1 << 27)
    both_modes(eng, ids, offs, w, sel=np.ones(len(ids), np.uint8), unit=WORD)


def test_fewer_sentinels_than_the_runs_of_a_long_document(eng, T):
    docs = [ramp(2 * T + 100, 1), ramp(300, 2), [], ramp(T, 3)]
    ids, offs = pack(docs)
    for n_sent in (0, 1, 40):
        r = run(eng, "spans", ids, offs, noise_opts(start_q32=1 << 28, seed=4, span_max=3, n_sentinels=n_sent, sentinel_first=200, final_id=2, flags=BOTH))
        assert r["n_runs_dropped"] > 0 and r["n_runs"] <= 4 * n_sent
    run(eng, "spans", ids, offs, noise_opts(start_q32=1 << 28, seed=4, span_max=3, n_sentinels=40, sentinel_first=200, flags=SPLIT | DESC))


def test_many_short_and_empty_documents(eng):
    rng = np.random.default_rng(5)
    docs = [ramp(int(n), i, 5) for i, n in enumerate(rng.integers(0, 4, 3000))]       # more starts in a tile than LDS holds
    ids, offs = pack(docs)
    both_modes(eng, ids, offs, seed=1, span_max=2, start_q32=1 << 31)


def test_one_random_batch_of_200k_ids(eng):
    rng = np.random.default_rng(7)
    lens = rng.integers(0, 600, 600).tolist() + [15000]
    docs = []
    for n in lens:
        x = rng.integers(S0, V, n)
        x[rng.random(n) < 0.03] = 3
        docs.append(x.tolist())
    ids, offs = pack(docs)
    assert 150000 < len(ids) < 230000
    both_modes(eng, ids, offs, seed=11, span_min=1, span_max=3, start_q32=1 << 28, n_sentinels=20)
    w = word_ids_of(rng, docs)
    run(eng, "replace", ids, offs, noise_opts(start_q32=1 << 29, seed=12, unit=WORD, span_max=2, mask_q32=ONE, flags=SELECTED), w)


# ---- the entries from text ----

TEXTS = ["The quick brown fox jumps over the lazy dog. " * 40, "", "naïve café 中文 \U0001f680 tokens", "x", "def f(a, b):\n    return a + b\n" * 200]


@pytest.mark.parametrize("unit", [TOKEN, WORD])
def test_composites_equal_encode_words_and_the_ids_entry(tk, eng, unit):
    data, offs = tk.pack_docs([t.encode() for t in TEXTS])
    d_data, d_offs = dev(data, np.uint8), dev(offs, np.uint64)
    D = len(TEXTS)
    d_ids, d_oo, n, wres = eng.encode_batch_device_words(d_data.data_ptr(), d_offs.data_ptr(), D, len(data), True, True, 0, tk.CHECK_OFFSETS, stream())
    ids = to_host(tk.DeviceView(d_ids, n, "<i4"), (n,), np.uint32).copy()
    oo = to_host(tk.DeviceView(d_oo, D + 1, "<i8"), (D + 1,), np.uint64).copy()
    w = to_host(wres.views()[0], n, np.uint32).copy()
    o = noise_opts(start_q32=1 << 30, mask_q32=ONE // 2, random_q32=ONE // 4, seed=9, unit=unit, span_max=3, mask_id=4, flags=SELECTED)
    exp = run(eng, "replace", ids, oo, o, w if unit == WORD else None)
    assert 0 < exp["n_selected"] < n
    _, _, n2, res = eng.encode_batch_device_noise_replace(d_data.data_ptr(), d_offs.data_ptr(), D, len(data), True, True, tk.CHECK_OFFSETS, stream(), **o)
    assert n2 == n
    helpers.assert_same(fetch_replace(res), exp, "device composite", REPLACE_COUNTS, REPLACE_ARRAYS)
    hid, hoo, out = eng.encode_batch_noise_replace(data, offs, True, True, **o)
    assert np.array_equal(hid, ids) and np.array_equal(hoo, oo)
    helpers.assert_same(out, exp, "host entry", ("n_selected", "n_masked", "n_random"), REPLACE_ARRAYS)
    o = noise_opts(start_q32=1 << 30, seed=9, unit=unit, span_max=3, n_sentinels=10, sentinel_first=50, final_id=2, flags=BOTH)
    exp = run(eng, "spans", ids, oo, o, w if unit == WORD else None)
    _, _, _, res = eng.encode_batch_device_noise_spans(d_data.data_ptr(), d_offs.data_ptr(), D, len(data), True, True, tk.CHECK_OFFSETS, stream(), **o)
    helpers.assert_same(fetch_spans(res), exp, "device composite", SPANS_COUNTS, SPANS_ARRAYS)
    hid, hoo, out = eng.encode_batch_noise_spans(data, offs, True, True, **o)
    assert np.array_equal(hid, ids)
    helpers.assert_same(out, exp, "host entry", [k for k in SPANS_COUNTS if k != "n_docs"], SPANS_ARRAYS)
    # start_q32 == 0: bit for bit encode's ids
    d_ids, d_oo, n, res = eng.encode_batch_device_noise_replace(d_data.data_ptr(), d_offs.data_ptr(), D, len(data), True, True, 0, stream(),
                                                                **noise_opts(mask_q32=ONE, unit=unit))
    assert np.array_equal(to_host(res.views()[0], n, np.uint32), ids) and res.n_selected == 0
    assert np.array_equal(to_host(tk.DeviceView(d_ids, n, "<i4"), (n,), np.uint32), ids)
    assert eng.last_noise_ms()[0] > 0


def test_every_refusal_leaves_an_earlier_result_readable(tk, eng):
    L, vp = tk.lib(), ctypes.c_void_p
    ids, offs = pack([ramp(50, 1), ramp(30, 2)])
    d_ids, d_oo = dev(ids, np.uint32), dev(offs, np.uint64)
    good_r = noise_opts(start_q32=1 << 31, mask_q32=ONE, flags=SELECTED)
    good_s = noise_opts(start_q32=1 << 31, n_sentinels=9, sentinel_first=20, final_id=2, flags=BOTH)
    rep = eng.noise_replace_device(d_ids.data_ptr(), d_oo.data_ptr(), 2, len(ids), stream=stream(), **good_r)
    before_r = fetch_replace(rep)

    def rc(mode, o, ids_p=d_ids.data_ptr(), oo_p=d_oo.data_ptr(), out=True, n_docs=2):
        st = (tk._NoiseReplace if mode == "replace" else tk._NoiseSpans)()
        opts = tk._noise_opts(**o) if o is not None else None
        fn = getattr(L, "tk_noise_%s_device" % mode)
        return fn(eng._h, vp(ids_p), vp(oo_p), n_docs, len(ids), None, None, ctypes.byref(opts) if opts else None, vp(stream()),
                  ctypes.byref(st) if out else None)

    for kw in REFUSED_REPLACE:
        assert rc("replace", noise_opts(**kw)) == tk.TK_ERR_INVALID_ARG, kw
    for bad in (dict(o=None), dict(ids_p=None), dict(oo_p=None), dict(out=False), dict(n_docs=2 ** 32 - 16)):
        assert rc("replace", **dict(dict(o=good_r), **bad)) == tk.TK_ERR_INVALID_ARG, bad
        assert rc("spans", **dict(dict(o=good_s), **bad)) == tk.TK_ERR_INVALID_ARG, bad
    helpers.assert_same(fetch_replace(rep), before_r, "behind the refusals", REPLACE_COUNTS, REPLACE_ARRAYS)
    sp = eng.noise_spans_device(d_ids.data_ptr(), d_oo.data_ptr(), 2, len(ids), stream=stream(), **good_s)
    before_s = fetch_spans(sp)
    for kw in REFUSED_SPANS:
        assert rc("spans", noise_opts(**kw)) == tk.TK_ERR_INVALID_ARG, kw
    helpers.assert_same(fetch_spans(sp), before_s, "behind the refusals", SPANS_COUNTS, SPANS_ARRAYS)
    for kw in ACCEPTED_SPANS:
        assert rc("spans", noise_opts(**kw)) == tk.TK_OK, kw
    with pytest.raises(tk.TokenizerError) as e:
        eng.noise_spans_device(d_ids.data_ptr(), d_oo.data_ptr(), 2, len(ids), stream=stream(), **noise_opts(flags=SPLIT, final_id=S0))
    assert e.value.code == tk.TK_ERR_INVALID_ARG and "final_id" in str(e.value)
    # the composites refuse before anything is encoded: the ids of an earlier encode stay as they are
    data, offs = tk.pack_docs([b"some text to encode", b"and more"])
    d_data, d_offs = dev(data, np.uint8), dev(offs, np.uint64)
    with pytest.raises(tk.TokenizerError):
        eng.encode_batch_device_noise_replace(d_data.data_ptr(), d_offs.data_ptr(), 2, len(data), stream=stream(), **noise_opts(span_max=65))
    with pytest.raises(tk.TokenizerError):
        eng.encode_batch_noise_spans(data, offs, **noise_opts(flags=0))


# ---- the Tekkenizer methods ----

@pytest.fixture(scope="module")
def tkz(tk, small_vocab):
    from test_host_tokenizer import model
    specials = ("<unk>", "<s>", "</s>", "<pad>", "[INST]", "<X0>", "<X1>", "<X2>", "<X3>", "<X4>")
    t = tk.Tekkenizer.from_json(json.dumps(model(small_vocab["tokens"], specials=specials)), device=0)
    yield t
    t.close()


DOCS = ["hello world, hello again", "", "a much longer document than the others, so that the rows are padded: " + "word " * 30, "x"]


@pytest.mark.parametrize("unit", ["token", "word"])
def test_encode_batch_mlm_padded_equals_the_dense_pass_over_the_ragged_result(tk, tkz, unit):
    kw = dict(mlm_probability=0.3, unit=unit, span=(1, 2), seed=3, add_bos=True, add_eos=True, return_tensors="np")
    rag = tkz.encode_batch_mlm(DOCS, **kw)
    oo = rag["offsets"].tolist()
    enc = [tkz.encode(d, True, True) for d in DOCS]
    assert oo == np.concatenate([[0], np.cumsum([len(e) for e in enc])]).tolist()
    sel = rag["labels"] != -100
    flat = np.array([x for e in enc for x in e])
    assert 0 < rag["n_selected"] == int(sel.sum()) and np.array_equal(rag["labels"][sel], flat[sel]) and np.array_equal(rag["input_ids"][~sel], flat[~sel])
    assert np.all(flat[sel] >= tkz.num_special_tokens())
    masked = sel & (rag["input_ids"] == tkz.unk_id())
    assert rag["n_masked"] == int(masked.sum()) and rag["n_masked"] + rag["n_random"] <= rag["n_selected"]
    for max_length, side in ((None, "right"), (12, "right"), (12, "left")):
        pad = tkz.encode_batch_mlm(DOCS, padding="longest", max_length=max_length, truncation_side=side, **kw)
        eng = tkz.engine()
        d_ids, d_lab, d_oo = dev(rag["input_ids"], np.uint32), dev(rag["labels"].view(np.uint32), np.uint32), dev(rag["offsets"], np.uint64)
        fl = tk.DENSE_TRUNC_LEFT if side == "left" else 0
        N = len(flat)
        a = eng.dense_from_ids_device(d_ids.data_ptr(), d_oo.data_ptr(), len(DOCS), N, max_length, None, tkz.pad_id(), 1, 1,
                                      fl | tk.DENSE_I64 | tk.DENSE_MASK, stream()).tensors(True)
        b = eng.dense_from_ids_device(d_lab.data_ptr(), d_oo.data_ptr(), len(DOCS), N, max_length, None, (-100) & 0xFFFFFFFF, 1, 1, fl, stream()).tensors(True)
        assert np.array_equal(pad["input_ids"], a["ids"].cpu().numpy()) and np.array_equal(pad["attention_mask"], a["mask"].cpu().numpy())
        assert np.array_equal(pad["labels"], b["ids"].cpu().numpy().astype(np.int64)) and pad["labels"].dtype == np.int64
        assert pad["n_selected"] == rag["n_selected"] and pad["input_ids"].shape == pad["labels"].shape
    other = tkz.encode_batch_mlm(DOCS, **dict(kw, seed=4))
    assert not np.array_equal(other["labels"], rag["labels"])
    with pytest.raises(tk.TokenizerError):
        tkz.encode_batch_mlm(DOCS, unit="sentence")


def test_encode_batch_span_corruption_forms(tk, tkz):
    x0 = tkz.get_control_token("<X0>")
    kw = dict(noise_density=0.3, span=(1, 3), sentinels=(x0, 5, False), final="</s>", seed=1, return_tensors="np")
    r = tkz.encode_batch_span_corruption(DOCS, **kw)
    io, lo = r["input_offsets"].tolist(), r["label_offsets"].tolist()
    eos = tkz.eos_id()
    assert r["n_runs"] > 0 and r["n_inputs"] == io[-1] and r["n_targets"] == lo[-1]
    for d, doc in enumerate(DOCS):
        inp, tgt = r["input_ids"][io[d]:io[d + 1]].tolist(), r["labels"][lo[d]:lo[d + 1]].tolist()
        assert tgt[-1] == eos
        # undo the corruption: every sentinel of the inputs stands for the ids behind it in the targets
        hidden, cur = {}, None
        for x in tgt[:-1]:
            if x0 <= x < x0 + 5:
                cur = hidden.setdefault(x, [])
            else:
                cur.append(x)
        back = [y for x in inp for y in (hidden[x] if x0 <= x < x0 + 5 else [x])]
        assert back == tkz.encode(doc)
    j = tkz.encode_batch_span_corruption(DOCS, form="joined", **kw)
    jo = j["offsets"].tolist()
    for d in range(len(DOCS)):
        inp, tgt = r["input_ids"][io[d]:io[d + 1]].tolist(), r["labels"][lo[d]:lo[d + 1]].tolist()
        assert j["input_ids"][jo[d]:jo[d + 1]].tolist() == inp + tgt and j["labels"][jo[d]:jo[d + 1]].tolist() == [-100] * len(inp) + tgt
    p = tkz.encode_batch_span_corruption(DOCS, padding="longest", **kw)
    assert p["input_ids"].shape[0] == len(DOCS) and p["labels"].shape[0] == len(DOCS)
    for d in range(len(DOCS)):
        n, m = io[d + 1] - io[d], lo[d + 1] - lo[d]
        assert p["input_ids"][d, :n].tolist() == r["input_ids"][io[d]:io[d + 1]].tolist() and p["lengths"][d] == n
        assert p["labels"][d, :m].tolist() == r["labels"][lo[d]:lo[d + 1]].tolist() and np.all(p["labels"][d, m:] == -100)
    pj = tkz.encode_batch_span_corruption(DOCS, form="joined", padding="longest", **kw)
    assert pj["input_ids"].shape == pj["labels"].shape and pj["input_ids"].shape[1] == max(jo[d + 1] - jo[d] for d in range(len(DOCS)))
