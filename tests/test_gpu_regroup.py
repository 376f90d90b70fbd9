"""Documents selected, reordered and cut into batches on the GPU (include/tekken_hip.h tk_regroup_from_ids_device and the entries
around it, csrc/tk_regroup.hip) against the plain restatement of the definition in tests/test_regroup_cpu.py -- element by
element over every output, never through a sum.  Every case runs with all optional outputs on and again with none."""
import numpy as np
import pytest

import helpers
from helpers import dev, on_device, to_host
from test_gpu_spans import pack, sweep_docs
from test_regroup_cpu import (ALL, BATCH_OFFSETS, BATCH_ROWLEN, BATCHES, DESC, GROUPED, HAND_CASES, KEEP, LABELS, LENGTH, NB, PERM, SHUFFLE,
                              expected_regroup, opts)

pytestmark = pytest.mark.gpu

ARRAYS = ("ids", "offsets", "labels", "perm", "batch_offsets", "batch_rowlen")
COUNTS = ("n_docs", "n_ids", "n_masked", "n_short", "n_long", "n_batches", "n_oversize", "n_batch_pad")
TILE, CAP = 4096, 1024      # TKY_TILE, TKY_CAP (csrc/tk_layout.h)


def fetch(res):
    """RegroupResult -> dict like expected_regroup's."""
    v = res.views()
    out = {"ids": to_host(v[0], (res.n_ids,), np.uint32), "offsets": to_host(v[1], (res.n_docs + 1,), np.uint64),
           "labels": to_host(v[2], (res.n_ids,), np.int32), "perm": to_host(v[3], (res.n_docs,), np.uint32),
           "batch_offsets": to_host(v[4], (res.n_batches + 1,), np.uint64), "batch_rowlen": to_host(v[5], (res.n_batches,), np.uint32)}
    out.update({k: getattr(res, k) for k in COUNTS})
    return out


def assert_same(got, exp, what=""):
    helpers.assert_same(got, exp, what, COUNTS, ARRAYS)


class Ragged:
    """Made-up ids and labels of the given lengths, on the host and on the device (uploaded once a set)."""

    def __init__(self, lengths, seed=0):
        import torch
        rng = np.random.default_rng(2000 + seed)
        self.oo = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
        n = int(self.oo[-1])
        self.ids = rng.integers(0, 2**32 - 1, n, dtype=np.uint64).astype(np.uint32)
        self.lab = rng.integers(-2**31, 2**31 - 1, n).astype(np.int32)
        self.D = len(lengths)
        self.d_ids, self.d_oo = on_device(self.ids, self.oo)
        self.d_lab = torch.from_numpy(self.lab if n else np.zeros(1, np.int32)).cuda()


def regroup(eng, r, o, keep=None, labels=True):
    import torch
    d_keep = dev(np.asarray(keep, np.uint8), np.uint8) if keep is not None else None
    return eng.regroup_from_ids_device(r.d_ids.data_ptr(), r.d_oo.data_ptr(), r.D, len(r.ids), o["order"], o["min_length"], o["max_length"],
                                       o["seed"], o["window"], o["max_tokens"], o["max_docs"], o["flags"],
                                       r.d_lab.data_ptr() if labels else 0, d_keep.data_ptr() if d_keep is not None else 0,
                                       torch.cuda.current_stream().cuda_stream)


def check_case(eng, r, keep=None, what="", **kw):
    """All optional outputs on, then none (the counts of the batches stay); -> the expected result of the first."""
    o = opts(**kw)
    full = dict(o, flags=o["flags"] | (ALL if o["max_tokens"] else NB))
    exp = expected_regroup(r.ids, r.oo, r.lab, keep, full)
    assert_same(fetch(regroup(eng, r, full, keep)), exp, (what, kw, "all outputs"))
    bare = dict(o, flags=(o["flags"] & DESC) | (BATCHES if o["max_tokens"] else 0))
    exp0 = expected_regroup(r.ids, r.oo, None, keep, bare)
    assert all(exp0[k] is None for k in ARRAYS[2:]) and all(exp0[k] == exp[k] for k in COUNTS)
    assert_same(fetch(regroup(eng, r, bare, keep, labels=False)), exp0, (what, kw, "no optional output"))
    return exp


@pytest.fixture(scope="module")
def eng(tk, test_vocab):
    e = tk.Engine(test_vocab["tokens"], test_vocab["num_special"], test_vocab["bos"], test_vocab["eos"], device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def big():
    """70 000 documents of 0 .. 40 ids: several blocks a radix pass, long runs of equal keys."""
    return Ragged(np.random.default_rng(41).integers(0, 41, 70000).tolist(), 1)


@pytest.fixture(scope="module")
def big_plus():
    """... and one document of 70 000 ids among them: a digit above 16 bits."""
    n = np.random.default_rng(41).integers(0, 41, 70000).tolist()
    n[31337] = 70000
    return Ragged(n, 2)


# ---- edges ----

def test_edges(eng):
    for order in (KEEP, LENGTH, SHUFFLE, GROUPED):
        kw = dict(order=order, window=3, seed=5, max_tokens=16)
        assert check_case(eng, Ragged([]), what="D = 0", **kw)["n_docs"] == 0
        assert check_case(eng, Ragged([7]), what="D = 1", **kw)["n_batches"] == 1
        assert check_case(eng, Ragged([0]), what="D = 1, empty", **kw)["n_docs"] == 1
        assert check_case(eng, Ragged([3, 9, 2]), keep=[0, 0, 0], what="all dropped", **kw)["n_masked"] == 3
        assert check_case(eng, Ragged([3, 9, 2]), what="all dropped by length", min_length=10, **kw)["n_short"] == 3
    r = Ragged([0] * 5000)                             # all empty: one batch of 5000 through two levels of the pyramid
    for order in (KEEP, LENGTH, GROUPED):
        e = check_case(eng, r, what="all empty", order=order, window=64, max_tokens=8)
        assert e["n_batches"] == 1 and e["n_ids"] == 0
    assert check_case(eng, r, what="all empty, max_docs", max_tokens=8, max_docs=7)["n_batches"] == 715
    rng = np.random.default_rng(42)
    n = rng.integers(0, 30, 3000).tolist()
    r = Ragged(n, 3)
    keep = (rng.random(3000) < 0.5).astype(np.uint8)
    e = check_case(eng, r, keep=keep, what="keep alone")
    assert e["n_masked"] == int((keep == 0).sum()) and e["n_short"] == e["n_long"] == 0
    e = check_case(eng, r, what="min alone", min_length=10)
    assert e["n_short"] == sum(x < 10 for x in n) and e["n_long"] == 0
    e = check_case(eng, r, what="max alone", max_length=20)
    assert e["n_long"] == sum(x > 20 for x in n) and e["n_short"] == 0
    e = check_case(eng, r, keep=keep, what="all three", min_length=5, max_length=25, order=LENGTH, max_tokens=300)
    assert e["n_masked"] + e["n_short"] + e["n_long"] + e["n_docs"] == 3000 and min(e["n_short"], e["n_long"]) > 0


@pytest.mark.parametrize("case", range(len(HAND_CASES)), ids=[c[0] for c in HAND_CASES])
def test_hand_cases_on_the_device(eng, case):
    name, lengths, keep, kw = HAND_CASES[case]
    check_case(eng, Ragged(lengths), keep=keep, what=name, **kw)


# ---- the gather ----

def test_gather_ties_unstaged_tiles_and_documents_across_tiles(eng):
    rng = np.random.default_rng(43)
    zeros = rng.choice([0, 0, 0, 0, 1, 2, 5, 9], 6000).tolist()                      # ties in the new offsets
    ones = [1] * (CAP + 500) + [0] * 40 + [1] * 3000                                 # more than TKY_CAP starts inside one tile
    long_one = rng.integers(0, 9, 400).tolist()
    long_one[200] = 3 * TILE + 5                                                     # a document that spans tiles
    for name, lengths in (("zeros", zeros), ("ones", ones), ("long", long_one)):
        r = Ragged(lengths, 4)
        for order in (KEEP, SHUFFLE, LENGTH):
            e = check_case(eng, r, what=name, order=order, seed=9)
            assert e["n_ids"] == sum(lengths)
    assert max(ones) == 1 and sum(ones) > TILE


def test_gather_alignment_of_source_and_output(eng):
    # odd source offsets into an output aligned to 4: document 0 (3 ids) is dropped, the others start at 3, 11, 19 and land at 0, 8, 16
    e = check_case(eng, Ragged([3, 8, 8, 8, 2]), keep=[0, 1, 1, 1, 1], what="odd source")
    assert e["offsets"].tolist() == [0, 8, 16, 24, 26]
    # the reverse: sources at 0, 4, 12 land at 1, 5, 13 behind the one-id document
    e = check_case(eng, Ragged([4, 8, 8, 1]), what="odd output", order=LENGTH)
    assert e["perm"].tolist() == [3, 0, 1, 2] and e["offsets"].tolist() == [0, 1, 5, 13, 21]
    for shift in range(1, 4):                          # every residue of source and output start against each other
        for out_shift in range(4):
            lengths = [shift] + [out_shift] + [16, 5, 12, 7, 4]
            e = check_case(eng, Ragged(lengths, shift), keep=[0, 1, 1, 1, 1, 1, 1], what=("residues", shift, out_shift))
            assert e["n_ids"] == out_shift + 44


# ---- the sort ----

SORT_CASES = [dict(order=LENGTH), dict(order=LENGTH, flags=DESC), dict(order=SHUFFLE, seed=1), dict(order=SHUFFLE, seed=2, flags=DESC),
              dict(order=KEEP, flags=DESC)]
SORT_CASES += [dict(order=GROUPED, window=w, seed=1, flags=f) for w in (1, 7, 4096, 100000) for f in (0, DESC)]
SORT_CASES += [dict(order=GROUPED, window=4096, seed=2)]


@pytest.mark.parametrize("case", range(len(SORT_CASES)), ids=lambda i: "-".join("%s%s" % kv for kv in SORT_CASES[i].items()))
def test_sort_70000_documents(eng, big, case):
    e = check_case(eng, big, what="70 000", **SORT_CASES[case])
    assert e["n_docs"] == 70000
    if SORT_CASES[case]["order"] == LENGTH:            # long runs of equal keys: the order inside them is the documents'
        n = np.diff(big.oo.astype(np.int64))[e["perm"]]
        assert np.all(np.diff(n) <= 0 if SORT_CASES[case].get("flags") else np.diff(n) >= 0)
        same = np.diff(n) == 0
        assert same.sum() > 60000 and np.all(np.diff(e["perm"].astype(np.int64))[same] > 0)


@pytest.mark.parametrize("case", [0, 1, 2, 9, 10, 13], ids=lambda i: "-".join("%s%s" % kv for kv in SORT_CASES[i].items()))
def test_sort_with_a_digit_above_16_bits(eng, big_plus, case):
    kw = SORT_CASES[case]
    e = check_case(eng, big_plus, what="70 000 + one long", min_length=1, **kw)
    if kw["order"] == LENGTH:
        assert int(e["perm"][0 if kw.get("flags") else -1]) == 31337


# ---- the batches ----

@pytest.mark.parametrize("max_docs", [0, 1, 8])
def test_batches_of_70000_documents(eng, big, max_docs):
    e = check_case(eng, big, what="T = 512", max_tokens=512, max_docs=max_docs)
    assert e["n_oversize"] == 0 and e["n_batches"] > (1000 if max_docs != 1 else 69999)
    if max_docs:
        assert int(np.diff(e["batch_offsets"].astype(np.int64)).max()) == max_docs


@pytest.mark.parametrize("flags", [0, DESC])
def test_batches_in_length_order(eng, big, big_plus, flags):
    e = check_case(eng, big, what="LENGTH, T = 4096", order=LENGTH, flags=flags, max_tokens=4096)
    assert e["n_batch_pad"] < e["n_ids"] // 20         # what the order is for: almost no padding
    e = check_case(eng, big_plus, what="LENGTH, T = 4096, one oversize", order=LENGTH, flags=flags, max_tokens=4096)
    assert e["n_oversize"] == 1
    e = check_case(eng, big, what="one batch", max_tokens=2**40)
    assert e["n_batches"] == 1 and e["batch_rowlen"].tolist() == [40]


def test_dense_helper_over_every_batch(tk, eng):
    """The dense pass over offsets + first_doc with the same ids pointer: no rebasing (tk_dense.hip indexes ids[oo[d] + j])."""
    import torch
    r = Ragged(np.random.default_rng(44).integers(0, 41, 3000).tolist(), 5)
    o = opts(order=GROUPED, window=256, seed=3, max_tokens=512)
    res = regroup(eng, r, o)
    exp = expected_regroup(r.ids, r.oo, r.lab, None, o)
    assert_same(fetch(res), exp)
    ids, oo = exp["ids"].astype(np.int64), exp["offsets"].astype(np.int64)
    batches = list(res.batches())
    assert [b[0] for b in batches] + [res.n_docs] == exp["batch_offsets"].tolist() and [b[2] for b in batches] == exp["batch_rowlen"].tolist()
    assert len(batches) > 100
    PAD = 0xFFFFFFF
    for first, end, rowlen in batches:
        d = eng.dense_from_regroup_batch(res, first, end, pad_id=PAD, stream=torch.cuda.current_stream().cuda_stream)
        assert (d.n_docs, d.row_len) == (end - first, rowlen)
        rows = np.full((end - first, rowlen), PAD, np.int64)
        for k in range(first, end):
            rows[k - first, :oo[k + 1] - oo[k]] = ids[oo[k]:oo[k + 1]]
        got = to_host(d.views()[0], (end - first, rowlen), np.int32)
        helpers.assert_array_same(got.view(np.uint32).astype(np.int64), rows, ("batch", first, end))
    assert_same(fetch(res), exp, "the regroup result after the dense calls")


# ---- the entries ----

def test_fused_and_host_entries_and_what_comes_next(tk, eng, test_vocab):
    import torch
    from test_rowfit_cpu import expected_rowfit
    docs = [x for x in sweep_docs() if len(x) < 5000]
    assert len(docs) > 200
    data, offs = pack(docs)
    D = len(docs)
    d_bytes, d_offs = torch.from_numpy(data).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    p_ids, p_oo, n_ids = eng.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), True, True, stream=stream)
    eids = to_host(tk.DeviceView(p_ids, n_ids, "<i4"), (n_ids,), np.uint32).copy()
    eoo = to_host(tk.DeviceView(p_oo, D + 1, "<i8"), (D + 1,), np.uint64).copy()
    for kw in (dict(order=GROUPED, window=32, seed=11, min_length=3, max_length=900, max_tokens=4096, max_docs=64),
               dict(order=LENGTH, flags=DESC | PERM | BATCHES | BATCH_OFFSETS | BATCH_ROWLEN, max_tokens=2000), dict(order=SHUFFLE, seed=2, flags=0)):
        o = opts(**kw)
        o["flags"] &= ~LABELS
        exp = expected_regroup(eids, eoo, None, None, o)
        args = (o["order"], o["min_length"], o["max_length"], o["seed"], o["window"], o["max_tokens"], o["max_docs"], o["flags"])
        res = eng.regroup_from_ids_device(p_ids, p_oo, D, n_ids, *args, stream=stream)
        assert_same(fetch(res), exp, ("from_ids over encode's output", kw))
        q_ids, q_oo, m_ids, fused = eng.encode_batch_device_regroup(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), True, True, *args,
                                                                    checks=tk.CHECK_OFFSETS, stream=stream)
        assert m_ids == n_ids and np.array_equal(to_host(tk.DeviceView(q_ids, m_ids, "<i4"), (m_ids,), np.uint32), eids)
        assert_same(fetch(fused), exp, ("fused", kw))
        assert_same(eng.encode_batch_regroup(data, offs, True, True, False, *args), exp, ("host", kw))
    assert exp["n_docs"] == D and 0 < expected_regroup(eids, eoo, None, None, opts(min_length=3, max_length=900, flags=0))["n_docs"] < D
    small = docs[:40] + [b"", b"a"]                    # the one-launch small path: its ids are mapped pinned memory
    sdata, soffs = pack(small)
    calls0 = eng.small_path_calls()
    host = eng.encode_batch_regroup(sdata, soffs, True, True, False, LENGTH, 0, 0, 0, 0, 256, 0, ALL & ~LABELS)
    assert eng.small_path_calls() > calls0
    sids, soo = eng.encode_batch(sdata, soffs, True, True)
    assert_same(host, expected_regroup(sids, soo, None, None, opts(order=LENGTH, max_tokens=256, flags=ALL & ~LABELS)), "host, small path")
    # text has no labels stream: refused before anything is encoded, and the earlier results stay readable
    fused = eng.encode_batch_device_regroup(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), True, True, *args, stream=stream)[3]
    before = fetch(fused)                              # (the host calls above were regroup calls: the buffers are theirs since)
    assert_same(before, exp, "fused, again")
    for call in (lambda: eng.encode_batch_regroup(data, offs, True, True, False, KEEP, flags=LABELS),
                 lambda: eng.encode_batch_device_regroup(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), True, True, flags=LABELS, stream=stream)):
        with pytest.raises(tk.TokenizerError) as e:
            call()
        assert e.value.code == tk.TK_ERR_INVALID_ARG and "labels" in str(e.value)
    # every refusal of step 5: a message, nothing written
    short_oo = dev(np.array([0, 5, 9]), np.uint64)
    falling = dev(np.array([0, 9, 5, n_ids]), np.uint64)
    bad = [dict(order=4), dict(flags=64), dict(flags=1 << 31), dict(order=GROUPED, window=0), dict(flags=BATCHES, max_tokens=0),
           dict(flags=LABELS), dict(min_length=5, max_length=4), dict(n_docs=0), dict(n_docs=2**32), dict(oo=short_oo.data_ptr(), n_docs=2),
           dict(oo=falling.data_ptr(), n_docs=3)]
    for opt in bad:
        with pytest.raises(tk.TokenizerError) as e:
            eng.regroup_from_ids_device(p_ids, opt.get("oo", p_oo), opt.get("n_docs", D), n_ids, opt.get("order", KEEP), opt.get("min_length", 0),
                                        opt.get("max_length", 0), 0, opt.get("window", 0), opt.get("max_tokens", 0), 0, opt.get("flags", 0), 0, 0, stream)
        assert e.value.code == tk.TK_ERR_INVALID_ARG and len(str(e.value)) > 12, (opt, str(e.value))
        assert_same(fetch(fused), before, ("the earlier result after", opt))
    # what comes next: the result's ids / offsets through the rowfit pass and through decode
    K = fused.n_docs
    fit = eng.rowfit_from_ids_device(fused.ids_ptr, fused.offsets_ptr, K, fused.n_ids, 256, 7, 0, 0, 0, -100, stream)
    efit = expected_rowfit(exp["ids"], exp["offsets"], None, 256, 7, -100, 0, 0)
    assert (fit.n_rows, fit.n_pad, fit.n_truncated) == (efit["n_rows"], efit["n_pad"], efit["n_truncated"])
    helpers.assert_array_same(to_host(fit.views()[0], (fit.n_rows, 256), np.int32), efit["input_ids"], "rowfit over the regrouped ids")
    tb, to = eng.decode_batch_device(fused.ids_ptr, fused.offsets_ptr, K, fused.n_ids, stream=stream)
    to = to_host(to, (K + 1,), np.int64)
    tb = to_host(tb, (int(to[-1]),), np.uint8).tobytes()
    want = eng.decode_docs([eids[int(eoo[d]):int(eoo[d + 1])].tolist() for d in exp_perm(eids, eoo, o)])
    assert [tb[int(to[k]):int(to[k + 1])] for k in range(K)] == want


def exp_perm(eids, eoo, o):
    return expected_regroup(eids, eoo, None, None, dict(o, flags=PERM))["perm"].tolist()


def test_tokenizer_method(tk, small_vocab):
    import json
    from test_host_tokenizer import model
    t = tk.Tekkenizer.from_json(json.dumps(model(small_vocab["tokens"])), device=0)
    try:
        docs = ["hello world", "", "hello", "hello hello hello world", "a"]       # 9, 2, 3, ?, 3 ids with BOS / EOS
        n = [len(t.encode(d, True, True)) for d in docs]
        for rt in ("pt", "np"):
            r = t.encode_batch_regrouped(docs, order="length", add_bos=True, add_eos=True, max_tokens=12, return_tensors=rt)
            perm = sorted(range(5), key=lambda d: (n[d], d))
            assert np.asarray(r["perm"].cpu() if rt == "pt" else r["perm"]).tolist() == perm
            assert np.asarray(r["offsets"].cpu() if rt == "pt" else r["offsets"]).tolist() == np.concatenate([[0], np.cumsum([n[d] for d in perm])]).tolist()
            assert r["n_docs"] == 5 and r["n_ids"] == sum(n) and r["labels"] is None and r["n_batches"] >= 2
        r = t.encode_batch_regrouped(docs, order="keep", add_bos=True, add_eos=True, keep=[1, 0, 1, 0, 1], min_length=3)
        assert r["perm"].tolist() == [0, 2, 4] and (r["n_masked"], r["n_short"]) == (2, 0) and r["batch_offsets"] is None
        assert r["ids"].tolist()[:9] == [1, 266, 42, 129, 121, 124, 118, 110, 2]
        with pytest.raises(tk.TokenizerError):
            t.encode_batch_regrouped(docs, order="sorted")
    finally:
        t.close()
