"""Fill-in-the-middle rows on the GPU (include/tekken_hip.h tk_fim_split_device and the entries around it, csrc/tk_fim.hip) against
the plain-loop restatement of the definition in tests/test_fim_cpu.py -- element by element over every output and counter, for
both unit sizes, PSM, SPM and mixed, drawn and given cuts; then the composite entries and the Tekkenizer methods."""
import json

import numpy as np
import pytest

import helpers
from helpers import dev, to_host
from test_fim_cpu import (ARRAYS, BOS, COUNTS, EOS, LABEL_MIDDLE, MID, NO_CUT, NONE, ONE, PART_SRC, PRE, SNAP, SUF, expected_fim, fim_opts,
                          pack)
from test_rowfit_cpu import expected_rowfit

pytestmark = pytest.mark.gpu

HALF = 1 << 31
ORDERS = {"psm": 0, "spm": ONE, "mixed": HALF}
SIZES = (0, 1, 2, 3, 15, 16, 17, 31, 32, 33)
TKY_CAP = 1024                  # csrc/tk_layout.h: the documents of a tile that LDS holds


@pytest.fixture(scope="module")
def eng(tk, test_vocab):
    e = tk.Engine(test_vocab["tokens"], test_vocab["num_special"], test_vocab["bos"], test_vocab["eos"], device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def tiles(tk):
    return {1: int(tk.lib().tk_fim_tile(1)), 4: int(tk.lib().tk_fim_tile(4))}


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def cuts_array(cuts, D):
    return None if cuts is None else np.array(cuts, np.uint64).reshape(D, 2)


def fetch(res):
    """FimResult -> dict like expected_fim's."""
    v = res.views()
    P, D = res.n_parts, res.n_docs
    out = {"units": to_host(v[0], res.n_units, np.uint8 if res.unit_bytes == 1 else np.uint32),
           "part_offsets": to_host(v[1], P + 1, np.uint64), "part_ctrl": to_host(v[2], P, np.uint32), "part_flags": to_host(v[3], P, np.uint32),
           "conv_offsets": to_host(v[4], D + 1, np.uint64), "part_src": to_host(v[5], P, np.uint64),
           "cuts": to_host(v[6], (D, 2), np.uint64), "mode": to_host(v[7], D, np.uint8)}
    out.update({k: getattr(res, k) for k in COUNTS})
    return out


def assert_same(got, exp, what=""):
    """(the dict of a host entry carries the counts that the arrays' shapes do not say: no n_docs)"""
    helpers.assert_same(got, exp, what, [k for k in COUNTS if k in got], ARRAYS)
    assert set(COUNTS) - set(got) <= {"n_docs"}


def check(eng, docs, unit_bytes, cuts=None, what="", **kw):
    """The device split of docs (lists of units) against the restatement; -> (the expected dict, the FimResult, the input tensor)."""
    kw.setdefault("flags", (SNAP | PART_SRC) if unit_bytes == 1 else PART_SRC)
    dt = np.uint8 if unit_bytes == 1 else np.uint32
    data, offs = pack(docs, dt)
    c = cuts_array(cuts, len(docs))
    d, o = dev(data, dt), dev(offs, np.uint64)
    dc = None if c is None else dev(c.reshape(-1), np.uint64)
    opts = fim_opts(**kw)
    split = eng.fim_split_device if unit_bytes == 1 else eng.fim_split_ids_device
    res = split(d.data_ptr(), o.data_ptr(), len(docs), len(data), 0 if dc is None else dc.data_ptr(), stream=stream(), **opts)
    exp = expected_fim(data, offs, opts, c, unit_bytes)
    assert_same(fetch(res), exp, (what, unit_bytes, kw))
    return exp, res, d


def units_of(rng, n, unit_bytes):
    return rng.integers(0, 256 if unit_bytes == 1 else 6000, n).tolist()


def ramp(n, unit_bytes, salt=0):
    """n units that tell where they came from (ASCII for text, so the snap moves nothing)."""
    return ((np.arange(n) * 7 + salt) % (96 if unit_bytes == 1 else 5987) + (32 if unit_bytes == 1 else 1000)).tolist()


# ---- the shapes ----

@pytest.mark.parametrize("unit_bytes", [1, 4])
def test_no_document_and_no_unit(eng, unit_bytes):
    for kw in (dict(rate_q32=ONE), dict(rate_q32=0)):
        exp, res, _ = check(eng, [], unit_bytes, **kw)
        assert res.n_docs == 0 and res.n_parts == 0 and exp["conv_offsets"].tolist() == [0]
        exp, res, _ = check(eng, [[], [], []], unit_bytes, spm_q32=HALF, **kw)
        assert res.n_units == 0 and res.n_parts == 15 and res.n_transformed == 0
    exp, res, _ = check(eng, [[], []], unit_bytes, [(0, 0), (NO_CUT, 0)])
    assert exp["mode"].tolist() == [1, 0]


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("unit_bytes", [1, 4])
def test_small_documents_drawn_and_given(eng, unit_bytes, order):
    rng = np.random.default_rng(unit_bytes)
    docs = [ramp(n, unit_bytes, i) for i, n in enumerate(SIZES * 3)]
    for seed in (0, 1):
        exp, _, _ = check(eng, docs, unit_bytes, rate_q32=ONE, spm_q32=ORDERS[order], seed=seed, what="drawn")
        assert exp["n_transformed"] == len(docs) - 3 and exp["n_skipped"] == 3
    check(eng, docs, unit_bytes, rate_q32=HALF, spm_q32=ORDERS[order], seed=5, min_units=3, flags=PART_SRC | LABEL_MIDDLE, what="half")
    cuts = [(int(rng.integers(0, n + 2)), int(rng.integers(0, n + 2))) if i % 5 else (NO_CUT, 1) for i, n in enumerate(SIZES * 3)]
    check(eng, docs, unit_bytes, cuts, spm_q32=ORDERS[order], seed=2, flags=LABEL_MIDDLE, what="given")   # (no part_src: NULL)
    every = [[(lo, hi) for lo in range(n + 1) for hi in range(lo, n + 1)] for n in (2, 3, 17)]       # every pair of cuts of a few sizes
    for n, pairs in zip((2, 3, 17), every):
        check(eng, [ramp(n, unit_bytes, i) for i in range(len(pairs))], unit_bytes, pairs, spm_q32=ORDERS[order], what="every pair")


@pytest.mark.parametrize("order", ["psm", "spm"])
@pytest.mark.parametrize("unit_bytes", [1, 4])
def test_one_document_over_three_tiles_with_the_cuts_on_the_borders(eng, tiles, unit_bytes, order):
    T = tiles[unit_bytes]
    at = (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1)
    pairs = [(lo, hi) for lo in at[:3] for hi in at if hi >= lo]
    # every document is three whole tiles, so each starts on a border; then the same cuts in documents that start 5 units off
    docs = [ramp(3 * T, unit_bytes, i) for i in range(len(pairs))]
    check(eng, docs, unit_bytes, pairs, spm_q32=ORDERS[order])
    docs = [ramp(2 * T + 5, unit_bytes, i) for i in range(len(pairs))]
    check(eng, docs, unit_bytes, [(lo, min(hi, 2 * T + 5)) for lo, hi in pairs], spm_q32=ORDERS[order])
    # the SEAMS of the output on the borders: PSM puts S at lo and M at lo + n - hi, SPM puts P at n - hi
    n = 3 * T
    pairs = [(T + k, n - T + j) for k in (-1, 0, 1) for j in (-1, 0, 1)]
    check(eng, [ramp(n, unit_bytes, i) for i in range(len(pairs))], unit_bytes, pairs, spm_q32=ORDERS[order])


@pytest.mark.parametrize("unit_bytes", [1, 4])
def test_a_document_boundary_exactly_on_a_tile_border(eng, tiles, unit_bytes):
    T = tiles[unit_bytes]
    sizes = [T, T - 1, 1, T + 1, T - 1, 0, 0, T, 2 * T, 7]
    docs = [ramp(n, unit_bytes, i) for i, n in enumerate(sizes)]
    for order in ("psm", "spm", "mixed"):
        check(eng, docs, unit_bytes, rate_q32=ONE, spm_q32=ORDERS[order], seed=3)
    check(eng, docs, unit_bytes, [(1, n) for n in sizes], spm_q32=HALF)


@pytest.mark.parametrize("unit_bytes", [1, 4])
def test_more_tiny_documents_in_a_tile_than_lds_holds(eng, tiles, unit_bytes):
    rng = np.random.default_rng(9)
    n_docs = 2 * TKY_CAP + 200                          # 0..3 units each: all of them in the first tile
    docs = [ramp(int(n), unit_bytes, i) for i, n in enumerate(rng.integers(0, 4, n_docs))]
    assert sum(len(d) for d in docs) < tiles[unit_bytes]
    docs.append(ramp(tiles[unit_bytes] + 40, unit_bytes))           # ... and a tile that LDS does hold behind it
    docs += [ramp(2, unit_bytes, 1)] * 50
    for order in ("psm", "spm", "mixed"):
        exp, _, _ = check(eng, docs, unit_bytes, rate_q32=ONE, spm_q32=ORDERS[order], seed=1)
        assert exp["n_transformed"] > TKY_CAP


def test_multi_byte_text_with_cuts_drawn_inside_characters(eng):
    docs = [list(d) for d in helpers.random_unicode_docs(300, seed=3, max_len=90)] + [list(("中\U0001f680é" * 700).encode())]
    inside = 0
    for seed in (0, 1):
        exp, _, _ = check(eng, docs, 1, rate_q32=ONE, spm_q32=HALF, seed=seed)
        raw = expected_fim(*pack(docs), fim_opts(rate_q32=ONE, spm_q32=HALF, seed=seed, flags=0))
        inside += int(np.sum(raw["cuts"] != exp["cuts"]))
        po, u = exp["part_offsets"], exp["units"].tobytes()
        for p in range(len(po) - 1):
            u[int(po[p]):int(po[p + 1])].decode("utf-8")                    # every part is valid UTF-8
        check(eng, docs, 1, rate_q32=ONE, spm_q32=HALF, seed=seed, flags=PART_SRC)   # without the snap
    assert inside > 50                                  # the draws did land inside characters


def test_invalid_utf8(eng):
    rng = np.random.default_rng(4)
    docs = [units_of(rng, int(n), 1) for n in rng.integers(0, 70, 200)]
    docs += [[0x80] * n for n in (1, 2, 3, 4, 5, 6, 40)] + [[0x61] + [0x80] * 5 + [0x62], [0xF0, 0x9F], [0xC3]]
    check(eng, docs, 1, rate_q32=ONE, spm_q32=HALF, seed=8)
    check(eng, docs, 1, [(len(d) - 1 if d else 0, len(d)) for d in docs])   # a continuation byte at n - 1


@pytest.mark.parametrize("head,tail", [(h, t) for h in (0, 1, 2) for t in (0, 1, 2)])
def test_head_and_tail_of_stored_ids(eng, head, tail):
    docs = [ramp(n, 4, i) for i, n in enumerate(SIZES + (4, 5, 40, 64, 65))]
    exp, _, _ = check(eng, docs, 4, rate_q32=ONE, spm_q32=HALF, seed=6, head=head, tail=tail)
    assert exp["n_skipped"] == sum(len(d) < head + tail + 1 for d in docs)
    check(eng, docs, 4, [(1, 3)] * len(docs), spm_q32=HALF, head=head, tail=tail, flags=PART_SRC | LABEL_MIDDLE)


@pytest.mark.parametrize("order", ["psm", "spm"])
def test_source_and_destination_misaligned_by_every_distance(eng, order):
    # lo = 1 .. 15 and a middle of 1 .. 16 bytes: the suffix and the middle move by every distance mod 16
    docs, cuts = [], []
    for lo in range(1, 16):
        for m in (1, 2, 7, 8, 15, 16):
            docs.append(ramp(200 + lo, 1, lo))
            cuts.append((lo, lo + 32 + m))
    check(eng, docs, 1, cuts, spm_q32=ORDERS[order])
    check(eng, [ramp(67, 4, i) for i in range(12)], 4, [(k % 4 + 1, 20 + k) for k in range(12)], spm_q32=ORDERS[order])


def test_rate_zero_returns_the_callers_buffer(eng):
    docs = [ramp(n, 1, n) for n in SIZES]
    exp, res, d = check(eng, docs, 1, rate_q32=0, flags=SNAP | BOS | EOS | PART_SRC)
    assert res.units_ptr == d.data_ptr() and exp["n_transformed"] == 0
    _, res, d = check(eng, docs, 1, [(NO_CUT, 0)] * len(docs))
    assert res.units_ptr != d.data_ptr()               # (cuts were given: the pass copies without looking at them)


# ---- the composites ----

def text_docs():
    docs = [d for d in helpers.mixed_docs(12, 4, 12, 3000)]
    return docs + helpers.random_unicode_docs(30, seed=5)


def join_of(eng, tk, exp, labels=True):
    """Step 7: encode_parts_join over the restatement's parts."""
    return eng.encode_parts_join(exp["units"], exp["part_offsets"], exp["part_ctrl"], exp["part_flags"], exp["conv_offsets"],
                                 flags=tk.JOIN_LABELS if labels else 0)


def assert_join(j, want, what=""):
    v = j.views()
    helpers.assert_array_same(to_host(v[0], j.n_ids, np.uint32), want["ids"], (what, "ids"))
    helpers.assert_array_same(to_host(v[1], j.n_convs + 1, np.uint64), want["offsets"], (what, "offsets"))
    helpers.assert_array_same(to_host(v[2], j.n_ids, np.int32), want["labels"], (what, "labels"))
    assert (j.n_ids, j.n_ctrl, j.n_labelled) == (want["n_ids"], want["n_ctrl"], want["n_labelled"])


@pytest.mark.parametrize("flags", [SNAP | BOS | EOS, SNAP | BOS | EOS | LABEL_MIDDLE | PART_SRC])
def test_device_and_host_composites_equal_the_join_of_the_restatement(eng, tk, flags):
    docs = text_docs()
    data, offs = pack([list(d) for d in docs])
    d, o = dev(data, np.uint8), dev(offs, np.uint64)
    for kw in (dict(rate_q32=HALF, spm_q32=HALF, seed=1), dict(rate_q32=ONE, spm_q32=ONE, middle_id=NONE, seed=2)):
        opts = fim_opts(flags=flags, **kw)
        exp = expected_fim(data, offs, opts)
        want = join_of(eng, tk, exp)
        f, j = eng.encode_batch_device_fim(d.data_ptr(), o.data_ptr(), len(docs), len(data), join_flags=tk.JOIN_LABELS, checks=3, stream=stream(),
                                           **opts)
        assert_same(fetch(f), exp, "device composite")
        assert_join(j, want, "device composite")
        hj, hf = eng.encode_batch_fim(data, offs, join_flags=tk.JOIN_LABELS, validate_utf8=True, return_parts=True, **opts)
        assert_same(hf, exp, "host composite")
        for k in ("ids", "offsets", "labels"):
            helpers.assert_array_same(hj[k], want[k], ("host composite", k))
        assert exp["n_transformed"] > 10


def test_given_cuts_through_the_host_entry(eng, tk):
    docs = [b"def f(x):\n    return x + 1\n", "préfixe 中文 \U0001f680 suffixe".encode(), b"", b"untouched"]
    cuts = np.array([(10, 18), (4, 15), (0, 0), (NO_CUT, 0)], np.uint64)
    data, offs = pack([list(d) for d in docs])
    opts = fim_opts(spm_q32=ONE, middle_id=NONE, flags=SNAP | BOS | EOS | PART_SRC)
    exp = expected_fim(data, offs, opts, cuts)
    hj, hf = eng.encode_batch_fim(data, offs, cuts, join_flags=tk.JOIN_LABELS, return_parts=True, **opts)
    assert_same(hf, exp, "host, cuts given")
    want = join_of(eng, tk, exp)
    helpers.assert_array_same(hj["ids"], want["ids"], "ids")
    helpers.assert_array_same(hj["labels"], want["labels"], "labels")


def test_rate_zero_is_encode_bit_for_bit(eng, tk):
    docs = text_docs()
    data, offs = pack([list(d) for d in docs])
    d, o = dev(data, np.uint8), dev(offs, np.uint64)
    for add_bos, add_eos in ((True, True), (False, False), (True, False)):
        flags = SNAP | (BOS if add_bos else 0) | (EOS if add_eos else 0)
        f, j = eng.encode_batch_device_fim(d.data_ptr(), o.data_ptr(), len(docs), len(data), stream=stream(), **fim_opts(rate_q32=0, flags=flags))
        assert f.units_ptr == d.data_ptr() and f.n_transformed == 0
        got_ids, got_oo = to_host(j.views()[0], j.n_ids, np.uint32), to_host(j.views()[1], j.n_convs + 1, np.uint64)
        p_ids, p_oo, n = eng.encode_batch_device(d.data_ptr(), o.data_ptr(), len(docs), len(data), add_bos, add_eos, stream())
        ids = to_host(tk.DeviceView(p_ids, n, "<i4"), n, np.uint32)
        oo = to_host(tk.DeviceView(p_oo, len(docs) + 1, "<i8"), len(docs) + 1, np.uint64)
        helpers.assert_array_same(got_ids, ids, "ids")
        helpers.assert_array_same(got_oo, oo, "offsets")


def test_ids_composite(eng, tk):
    rng = np.random.default_rng(12)
    docs = [[1] + (rng.integers(1000, 6000, int(n))).tolist() + [2] for n in rng.integers(0, 80, 150)] + [[1], [], [7, 8, 9]]
    ids, offs = pack(docs, np.uint32)
    d, o = dev(ids, np.uint32), dev(offs, np.uint64)
    f, j = eng.fim_from_ids_device(d.data_ptr(), o.data_ptr(), len(docs), len(ids), stream=stream(), **fim_opts(rate_q32=0, head=1, tail=1))
    assert f.units_ptr == d.data_ptr() and j.n_ctrl == 0
    helpers.assert_array_same(to_host(j.views()[0], j.n_ids, np.uint32), ids, "rate 0: the input ids")
    helpers.assert_array_same(to_host(j.views()[1], len(docs) + 1, np.uint64), offs, "rate 0: the input offsets")
    opts = fim_opts(rate_q32=ONE, spm_q32=HALF, seed=4, head=1, tail=1, flags=LABEL_MIDDLE | PART_SRC)
    f, j = eng.fim_from_ids_device(d.data_ptr(), o.data_ptr(), len(docs), len(ids), join_flags=tk.JOIN_LABELS, stream=stream(), **opts)
    exp = expected_fim(ids, offs, opts, None, 4)
    assert_same(fetch(f), exp, "ids composite")
    want_ids, want_lab, want_oo = [], [], [0]           # the join, restated: a control id in front of every part that has one
    po = exp["part_offsets"]
    for p in range(exp["n_parts"]):
        c, fl = int(exp["part_ctrl"][p]), int(exp["part_flags"][p])
        seg = exp["units"][int(po[p]):int(po[p + 1])].tolist()
        if c != NONE:
            want_ids.append(c)
            want_lab.append(c if fl & 1 else -100)
        want_ids += seg
        want_lab += seg if fl & 2 else [-100] * len(seg)
        if p % 5 == 4:
            want_oo.append(len(want_ids))
    v = j.views()
    helpers.assert_array_same(to_host(v[0], j.n_ids, np.uint32), np.array(want_ids, np.uint32), "ids")
    helpers.assert_array_same(to_host(v[1], len(docs) + 1, np.uint64), np.array(want_oo, np.uint64), "offsets")
    helpers.assert_array_same(to_host(v[2], j.n_ids, np.int32), np.array(want_lab, np.int32), "labels")


def test_a_refused_call_leaves_the_earlier_result_readable(eng, tk):
    docs = [ramp(40, 1, i) for i in range(20)]
    exp, res, d = check(eng, docs, 1, rate_q32=ONE, spm_q32=HALF, seed=9)
    o = dev(pack(docs)[1], np.uint64)
    args = (d.data_ptr(), o.data_ptr(), len(docs), 800)
    for bad in (dict(flags=32), dict(rate_q32=ONE + 1), dict(spm_q32=ONE + 1), dict(head=1), dict(tail=2), dict(prefix_id=1000),
                dict(suffix_id=5000), dict(middle_id=0xFFFFFFFE)):
        with pytest.raises(tk.TokenizerError) as e:
            eng.fim_split_device(*args, stream=stream(), **fim_opts(**dict(dict(rate_q32=ONE), **bad)))
        assert e.value.code == tk.TK_ERR_INVALID_ARG, bad
    with pytest.raises(tk.TokenizerError) as e:
        eng.fim_split_device(*args, checks=64, stream=stream(), **fim_opts())
    assert e.value.code == tk.TK_ERR_INVALID_ARG
    with pytest.raises(tk.TokenizerError) as e:
        eng.fim_split_device(d.data_ptr(), o.data_ptr(), 2 ** 32 - 16, 800, stream=stream(), **fim_opts())
    assert e.value.code == tk.TK_ERR_INVALID_ARG
    with pytest.raises(tk.TokenizerError) as e:
        eng.fim_split_device(d.data_ptr(), 0, len(docs), 800, stream=stream(), **fim_opts())
    assert e.value.code == tk.TK_ERR_INVALID_ARG
    for bad in (dict(flags=BOS), dict(flags=EOS), dict(flags=64)):
        with pytest.raises(tk.TokenizerError) as e:
            eng.fim_split_ids_device(*args, stream=stream(), **fim_opts(**bad))
        assert e.value.code == tk.TK_ERR_INVALID_ARG, bad
    with pytest.raises(tk.TokenizerError) as e:           # the join's options are refused before the text is split
        eng.encode_batch_device_fim(*args, join_flags=8, stream=stream(), **fim_opts(rate_q32=ONE))
    assert e.value.code == tk.TK_ERR_INVALID_ARG
    assert_same(fetch(res), exp, "the earlier result")
    ms = eng.last_fim_ms()
    assert len(ms) == 2 and ms[0] > 0 and ms[1] > 0


# ---- the Tekkenizer methods ----

@pytest.fixture(scope="module")
def tkz(tk, small_vocab):
    from test_host_tokenizer import model
    specials = ("<unk>", "<s>", "</s>", "<pad>", "[INST]", "[PREFIX]", "[SUFFIX]", "[MIDDLE]")
    t = tk.Tekkenizer.from_json(json.dumps(model(small_vocab["tokens"], specials=specials)), device=0)
    yield t
    t.close()


def test_encode_fim_agrees_with_the_batch_call_at_given_cuts(tkz, tk):
    prefix, middle, suffix = "def add(a, b):\n    return ", "a + b", "\n\nprint(add(1, 2)) # é中"
    prompt = tkz.encode_fim(prefix, suffix)
    assert prompt == [1, 6] + tkz.encode(suffix) + [5] + tkz.encode(prefix)
    a = len(prefix.encode())
    r = tkz.encode_batch_fim([prefix + middle + suffix, "left alone"], cuts=[(a, a + len(middle.encode())), None])
    oo = r["offsets"].tolist()
    row = r["input_ids"][oo[0]:oo[1]].tolist()
    assert row == prompt + tkz.encode(middle) + [2]     # the prompt, then what the model is to produce
    assert r["input_ids"][oo[1]:oo[2]].tolist() == tkz.encode("left alone", True, True)
    assert r["mode"].tolist() == [tk.FIM_SPM, tk.FIM_NONE] and r["cuts"].tolist() == [[a, a + 5], [NO_CUT, NO_CUT]]
    assert (r["n_transformed"], r["n_spm"], r["n_skipped"]) == (1, 1, 0) and r["labels"].tolist() == r["input_ids"].tolist()
    m = tkz.encode_batch_fim([prefix + middle + suffix], cuts=[(a, a + 5)], format="psm_spm", spm_rate=0.0, train_on="middle")
    assert m["input_ids"].tolist() == [1, 5] + tkz.encode(prefix) + [6] + tkz.encode(suffix) + [7] + tkz.encode(middle) + [2]
    n_mid = len(tkz.encode(middle))
    assert m["labels"].tolist() == [-100] * (len(m["labels"]) - n_mid - 1) + tkz.encode(middle) + [2] and m["n_labelled"] == n_mid + 1
    pt = tkz.encode_batch_fim([prefix + middle + suffix, "left alone"], cuts=[(a, a + 5), None], return_tensors="pt")
    assert pt["input_ids"].cpu().tolist() == r["input_ids"].tolist() and pt["offsets"].cpu().tolist() == oo
    with pytest.raises(tk.TokenizerError):
        tkz.encode_batch_fim(["x"], format="nope")
    with pytest.raises(tk.TokenizerError):
        tkz.encode_batch_fim(["x"], fim_rate=1.5)


def test_drawn_rows_depend_on_the_seed_alone(tkz):
    docs = ["document number %d: " % i + "xy " * (i % 17) for i in range(64)]
    a, b, c = (tkz.encode_batch_fim(docs, fim_rate=0.5, seed=s) for s in (3, 3, 4))
    assert a["input_ids"].tolist() == b["input_ids"].tolist() and a["cuts"].tolist() == b["cuts"].tolist()
    assert a["mode"].tolist() != c["mode"].tolist() and 10 < a["n_transformed"] < 54       # 32 +- 5.5 sigma
    for d in range(len(docs)):                          # a row is a permutation of the plain row plus the two control ids
        row = a["input_ids"][int(a["offsets"][d]):int(a["offsets"][d + 1])].tolist()
        plain = tkz.encode(docs[d], True, True)
        assert sorted(row) == sorted(plain + ([5, 6] if a["mode"][d] else []))


def test_packed_rows_hold_exactly_the_joined_ids(tkz):
    docs = ["row %d " % i + "abc " * (i % 23) for i in range(40)] + ["", "é中\U0001f680" * 9]
    kw = dict(fim_rate=0.7, spm_rate=0.5, seed=11, format="psm_spm", train_on="middle")
    r = tkz.encode_batch_fim(docs, **kw)
    L = 96
    p = tkz.encode_batch_fim_packed(docs, L, dtype="int32", return_tensors="np", **kw)
    exp = expected_rowfit(r["input_ids"], r["offsets"], r["labels"], L, tkz.pad_id())
    for k in ("input_ids", "labels", "position_ids", "segment_ids", "cu_seqlens", "doc_start"):
        got = p[k].view(exp[k].dtype) if p[k].dtype != exp[k].dtype else p[k]
        helpers.assert_array_same(got, exp[k], k)
    for k in ("n_rows", "n_segments", "max_seqlen", "n_truncated", "n_pad"):
        assert p[k] == exp[k], k
    assert (p["n_transformed"], p["n_spm"], p["n_skipped"], p["n_labelled"]) == (r["n_transformed"], r["n_spm"], r["n_skipped"], r["n_labelled"])
    assert p["n_transformed"] > 15
