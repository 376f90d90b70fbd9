"""Masked-LM and span-corruption rows (include/tekken_hip.h tk_noise_replace_device / tk_noise_spans_device): the definition restated
with plain loops, id by id, hand-made cases of every rule, invariants on random inputs, the covered fraction against the rate
given to noise_start_q32, the header's values, the exported symbols, the shim's declarations and the binding's description of the
two structs."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from test_layout_binding_cpu import header_members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF
NONE = 0xFFFFFFFF               # TK_JOIN_NONE, TK_WORD_NONE
ONE = 1 << 32                   # a rate of 1 in q32
TOKEN, WORD = 0, 1
SELECTED, DESC, SPLIT, JOINED = 1, 2, 4, 8
SPAN_LIMIT = 64
S0, V = 1000, 7000              # tests/helpers.py small_trained_vocab: 1000 special ids, 6000 ranks
VALUES = {"TK_NOISE_UNIT_TOKEN": TOKEN, "TK_NOISE_UNIT_WORD": WORD, "TK_NOISE_SELECTED": SELECTED, "TK_NOISE_DESC": DESC,
          "TK_NOISE_SPLIT": SPLIT, "TK_NOISE_JOINED": JOINED, "TK_NOISE_SPAN_LIMIT": SPAN_LIMIT}
NEW_SYMBOLS = ["tk_noise_replace_device", "tk_noise_spans_device", "tk_encode_batch_device_noise_replace", "tk_encode_batch_device_noise_spans",
               "tk_encode_batch_noise_replace", "tk_encode_batch_noise_spans", "tk_free_noise_replace", "tk_free_noise_spans",
               "tk_last_noise_ms", "tk_noise_tile"]
REPLACE_ARRAYS = ("input_ids", "labels", "selected")
REPLACE_COUNTS = ("n_docs", "n_ids", "n_selected", "n_masked", "n_random")
SPANS_ARRAYS = ("inputs", "input_offsets", "targets", "target_offsets", "joined", "joined_offsets", "joined_labels")
SPANS_COUNTS = ("n_docs", "n_selected", "n_runs", "n_runs_dropped", "n_inputs", "n_targets")


def h(seed, d):
    """The regroup pass's hash, as the header states it at TK_REGROUP_ORDER_SHUFFLE."""
    x = (d * 0x9E3779B1 + seed) & M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def noise_opts(start_q32=0, mask_q32=0, random_q32=0, seed=0, unit=TOKEN, span_min=1, span_max=1, mask_id=3, n_sentinels=0, sentinel_first=0,
               final_id=NONE, flags=0, ignore_index=-100):
    return dict(start_q32=start_q32, mask_q32=mask_q32, random_q32=random_q32, seed=seed, unit=unit, span_min=span_min, span_max=span_max,
                mask_id=mask_id, n_sentinels=n_sentinels, sentinel_first=sentinel_first, final_id=final_id, flags=flags, ignore_index=ignore_index)


def check_opts(o, spans, have_words, have_sel, n_docs, num_special, vocab):
    """Step 5: what the entries refuse raises ValueError."""
    if o["flags"] & ~(SELECTED | DESC | SPLIT | JOINED):
        raise ValueError("flag")
    if o["unit"] not in (TOKEN, WORD):
        raise ValueError("unit")
    if not 1 <= o["span_min"] <= o["span_max"] <= SPAN_LIMIT:
        raise ValueError("span")
    if o["start_q32"] > ONE or o["mask_q32"] > ONE or o["random_q32"] > ONE or o["mask_q32"] + o["random_q32"] > ONE:
        raise ValueError("rate")
    if o["unit"] == WORD and not have_words and not have_sel:
        raise ValueError("word_ids")
    if not spans:
        if o["mask_id"] >= vocab:
            raise ValueError("mask_id")
    else:
        if not o["flags"] & (SPLIT | JOINED):
            raise ValueError("no output")
        if o["final_id"] != NONE and o["final_id"] >= num_special:
            raise ValueError("final_id")
        n, first = o["n_sentinels"], o["sentinel_first"]
        for k in ((0, n - 1) if n else ()):             # the two ends of the sentinels the options can produce
            s = first - k if o["flags"] & DESC else first + k
            if not 0 <= s < num_special:
                raise ValueError("sentinel")
    if n_docs >= 2 ** 32 - 16:
        raise ValueError("n_docs")


def covered(o, t0, t1, x):
    """Step 2 for one unit index."""
    q = x
    while q >= 0 and q > x - o["span_max"]:
        if h(t0, q & M32) < o["start_q32"]:
            ln = o["span_min"] + ((h(t1, q & M32) * (o["span_max"] - o["span_min"] + 1)) >> 32)
            if q + ln > x:
                return True
        q -= 1
    return False


def select(ids, offs, o, word_ids, sel, num_special):
    """Steps 1 and 2: selected(i) of every id, and (d, p) of every id."""
    s = [h(o["seed"] & M32, (0x4E4F4900 + k) & M32) for k in range(4)]
    chosen, where = [], []
    for d in range(len(offs) - 1):
        t = [h(s[k], d & M32) for k in range(4)]
        for i in range(offs[d], offs[d + 1]):
            p = i - offs[d]
            eligible = ids[i] >= num_special
            if o["unit"] == WORD and word_ids is not None:
                eligible = eligible and word_ids[i] != NONE
            if sel is not None:
                c = sel[i] != 0
            else:
                x = p if o["unit"] == TOKEN else word_ids[i]
                c = eligible and covered(o, t[0], t[1], x)
            chosen.append(bool(eligible and c))
            where.append((d, p, t))
    return chosen, where


def _lists(ids, offs, word_ids, sel):
    conv = lambda a: None if a is None else [int(x) for x in np.asarray(a).tolist()]   # noqa: E731
    return conv(ids), conv(offs), conv(word_ids), conv(sel)


def expected_noise_replace(ids, offs, opts, word_ids=None, sel=None, num_special=S0, vocab=V):
    """Steps 1-3 and 5: the result of tk_noise_replace_device as a dict of numpy arrays and counts, id by id."""
    o = noise_opts(**opts)
    ids, offs, word_ids, sel = _lists(ids, offs, word_ids, sel)
    D = len(offs) - 1
    check_opts(o, False, word_ids is not None, sel is not None, D, num_special, vocab)
    if any(offs[d + 1] - offs[d] >= 2 ** 32 - 1 for d in range(D)):
        raise ValueError("document length")
    chosen, where = select(ids, offs, o, word_ids, sel, num_special)
    out, lab = [], []
    n_mask = n_rand = 0
    for i in range(len(chosen)):
        d, p, t = where[i]
        v, lb = ids[i], o["ignore_index"]
        if chosen[i]:
            lb = ids[i]
            r = h(t[2], p & M32)
            if r < o["mask_q32"]:
                v = o["mask_id"]
                n_mask += 1
            elif r < o["mask_q32"] + o["random_q32"]:
                v = num_special + ((h(t[3], p & M32) * (vocab - num_special)) >> 32)
                n_rand += 1
        out.append(v)
        lab.append(lb)
    return {"input_ids": np.array(out, np.uint32), "labels": np.array(lab, np.int32),
            "selected": np.array(chosen, np.uint8) if o["flags"] & SELECTED else None,
            "n_docs": D, "n_ids": len(out), "n_selected": sum(chosen), "n_masked": n_mask, "n_random": n_rand}


def expected_noise_spans(ids, offs, opts, word_ids=None, sel=None, num_special=S0, vocab=V):
    """Steps 1, 2, 4 and 5: the result of tk_noise_spans_device, document by document and id by id."""
    o = noise_opts(**opts)
    ids, offs, word_ids, sel = _lists(ids, offs, word_ids, sel)
    D = len(offs) - 1
    check_opts(o, True, word_ids is not None, sel is not None, D, num_special, vocab)
    if any(offs[d + 1] - offs[d] >= 2 ** 32 - 2 - o["n_sentinels"] for d in range(D)):
        raise ValueError("document length")
    chosen, _ = select(ids, offs, o, word_ids, sel, num_special)
    inputs, targets, joined, jlab, io, to, jo = [], [], [], [], [0], [0], [0]
    n_sel = n_runs = n_drop = 0
    for d in range(D):
        inp, tgt, k, prev = [], [], -1, False           # k: the run the last selected id belongs to
        for i in range(offs[d], offs[d + 1]):
            if chosen[i]:
                if not prev:
                    k += 1
                    if k < o["n_sentinels"]:
                        s = o["sentinel_first"] - k if o["flags"] & DESC else o["sentinel_first"] + k
                        inp.append(s)
                        tgt.append(s)
                        n_runs += 1
                    else:
                        n_drop += 1
                if k < o["n_sentinels"]:
                    tgt.append(ids[i])
                    n_sel += 1
                else:
                    inp.append(ids[i])
            else:
                inp.append(ids[i])
            prev = chosen[i]
        if o["final_id"] != NONE:
            tgt.append(o["final_id"])
        inputs += inp
        targets += tgt
        joined += inp + tgt
        jlab += [o["ignore_index"]] * len(inp) + tgt
        io.append(len(inputs))
        to.append(len(targets))
        jo.append(len(joined))
    split, jn = o["flags"] & SPLIT, o["flags"] & JOINED
    return {"inputs": np.array(inputs, np.uint32) if split else None, "input_offsets": np.array(io, np.uint64) if split else None,
            "targets": np.array(targets, np.uint32) if split else None, "target_offsets": np.array(to, np.uint64) if split else None,
            "joined": np.array(joined, np.uint32) if jn else None, "joined_offsets": np.array(jo, np.uint64) if jn else None,
            "joined_labels": np.array(jlab, np.int64).astype(np.int32) if jn else None,
            "n_docs": D, "n_selected": n_sel, "n_runs": n_runs, "n_runs_dropped": n_drop, "n_inputs": len(inputs), "n_targets": len(targets)}


def pack(docs):
    offs = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
    return np.array([x for d in docs for x in d], np.uint32), offs


def sel_of(docs_marks):
    """Documents as strings of '.', 'x' (selected) -> the sel bytes."""
    return np.array([c == "x" for d in docs_marks for c in d], np.uint8)


def spans(docs, marks, **kw):
    kw.setdefault("flags", SPLIT | JOINED)
    ids, offs = pack(docs)
    return expected_noise_spans(ids, offs, noise_opts(**kw), sel=sel_of(marks))


def rows(r, what, offsets):
    o = r[offsets].tolist()
    return [r[what][o[d]:o[d + 1]].tolist() for d in range(len(o) - 1)]


# ---- hand-made cases ----

def test_the_t5_example():
    """'Thank you for inviting me to your party last week .' with 'for inviting' and 'last' hidden: words as ids."""
    words = "Thank you for inviting me to your party last week .".split()
    doc = [2000 + i for i in range(len(words))]
    X, Y, Z = 900, 899, 898                             # descending sentinels, as T5's <extra_id_0>, <extra_id_1>, ...
    r = spans([doc], ["..xx....x.."], n_sentinels=2, sentinel_first=X, final_id=Z, flags=SPLIT | JOINED | DESC)
    assert rows(r, "inputs", "input_offsets") == [[2000, 2001, X, 2004, 2005, 2006, 2007, Y, 2009, 2010]]
    assert rows(r, "targets", "target_offsets") == [[X, 2002, 2003, Y, 2008, Z]]
    assert rows(r, "joined", "joined_offsets") == [[2000, 2001, X, 2004, 2005, 2006, 2007, Y, 2009, 2010, X, 2002, 2003, Y, 2008, Z]]
    assert rows(r, "joined_labels", "joined_offsets") == [[-100] * 10 + [X, 2002, 2003, Y, 2008, Z]]
    assert (r["n_selected"], r["n_runs"], r["n_runs_dropped"], r["n_inputs"], r["n_targets"]) == (3, 2, 0, 10, 6)


def test_a_special_id_splits_a_run_and_is_never_selected():
    r = spans([[2000, 2001, 5, 2003, 2004]], ["xxxxx"], n_sentinels=4, sentinel_first=10)
    assert rows(r, "inputs", "input_offsets") == [[10, 5, 11]]
    assert rows(r, "targets", "target_offsets") == [[10, 2000, 2001, 11, 2003, 2004]]
    ids, offs = pack([[2000, 5, 2002]])
    m = expected_noise_replace(ids, offs, noise_opts(mask_q32=ONE, mask_id=7, flags=SELECTED), sel=np.ones(3, np.uint8))
    assert m["input_ids"].tolist() == [7, 5, 7] and m["labels"].tolist() == [2000, -100, 2002] and m["selected"].tolist() == [1, 0, 1]
    assert (m["n_selected"], m["n_masked"], m["n_random"]) == (2, 2, 0)


def test_runs_beyond_n_sentinels_are_dropped_and_count_as_not_selected():
    doc = [2000 + i for i in range(9)]
    r = spans([doc], ["x.xx.x..x"], n_sentinels=2, sentinel_first=20, final_id=1)
    assert rows(r, "inputs", "input_offsets") == [[20, 2001, 21, 2004, 2005, 2006, 2007, 2008]]
    assert rows(r, "targets", "target_offsets") == [[20, 2000, 21, 2002, 2003, 1]]
    assert (r["n_selected"], r["n_runs"], r["n_runs_dropped"]) == (3, 2, 2)
    r = spans([doc, []], ["x.xx.x..x", ""], n_sentinels=0, final_id=1)       # everything dropped
    assert rows(r, "inputs", "input_offsets") == [doc, []] and rows(r, "targets", "target_offsets") == [[1], [1]]
    assert (r["n_selected"], r["n_runs"], r["n_runs_dropped"]) == (0, 0, 4)
    r = spans([doc], ["x.xx.x..x"], n_sentinels=0)
    assert r["n_targets"] == 0 and r["targets"].shape == (0,)


def test_runs_at_the_ends_of_documents_do_not_join_and_empty_documents():
    a, b = [2000, 2001, 2002], [3000, 3001]
    r = spans([a, [], b, []], ["x.x", "", "xx", ""], n_sentinels=3, sentinel_first=30, final_id=2)
    assert rows(r, "inputs", "input_offsets") == [[30, 2001, 31], [], [30], []]
    assert rows(r, "targets", "target_offsets") == [[30, 2000, 31, 2002, 2], [2], [30, 3000, 3001, 2], [2]]
    assert r["joined_offsets"].tolist() == [0, 8, 9, 14, 15]
    r = spans([], [], n_sentinels=3, sentinel_first=30, final_id=2)
    assert r["input_offsets"].tolist() == [0] and r["n_inputs"] == 0 and r["n_targets"] == 0
    r = spans([a], ["..."], n_sentinels=3, sentinel_first=30)           # no kept run: the document, and nothing
    assert rows(r, "inputs", "input_offsets") == [a] and rows(r, "targets", "target_offsets") == [[]]


def test_split_alone_and_joined_alone():
    r = spans([[2000, 2001]], ["x."], n_sentinels=1, sentinel_first=4, flags=SPLIT)
    assert r["joined"] is None and r["joined_offsets"] is None and r["joined_labels"] is None and r["inputs"].tolist() == [4, 2001]
    r = spans([[2000, 2001]], ["x."], n_sentinels=1, sentinel_first=4, flags=JOINED, ignore_index=-1)
    assert r["inputs"] is None and r["target_offsets"] is None and r["joined"].tolist() == [4, 2001, 4, 2000]
    assert r["joined_labels"].tolist() == [-1, -1, 4, 2000]


def first_covering(seed, d, lo, hi, start_q32, n=200):
    """(x, covered flags of 0 .. n) for document d under the draws."""
    o = noise_opts(start_q32=start_q32, seed=seed, span_min=lo, span_max=hi)
    s = [h(seed, (0x4E4F4900 + k) & M32) for k in range(4)]
    t = [h(s[k], d) for k in range(4)]
    return [covered(o, t[0], t[1], x) for x in range(n)], t


def test_the_draws_cover_whole_spans_and_look_at_indices_only():
    """Hand check of step 2 on one document: every start q covers exactly q .. q + len(q) - 1, nothing else is covered, and a special
    id at a start position still starts the span (the ids behind it are selected)."""
    lo, hi, sq = 2, 4, 1 << 29
    cov, t = first_covering(7, 0, lo, hi, sq)
    want = [False] * 200
    for q in range(200):
        if h(t[0], q) < sq:
            ln = lo + ((h(t[1], q) * (hi - lo + 1)) >> 32)
            assert lo <= ln <= hi
            for x in range(q, min(q + ln, 200)):
                want[x] = True
    assert cov == want and any(cov) and not all(cov)
    q = next(q for q in range(1, 199) if h(t[0], q) < sq and not cov[q - 1])
    ids = [2000] * 200
    ids[q] = 5                                          # a special id on a start position
    r = expected_noise_replace(np.array(ids, np.uint32), [0, 200], noise_opts(start_q32=sq, seed=7, span_min=lo, span_max=hi, flags=SELECTED))
    assert r["selected"][q] == 0 and r["selected"][q + 1] == 1
    assert r["selected"].tolist() == [int(c and i != q) for i, c in enumerate(cov)]


def test_documents_draw_apart_and_two_seeds_share_no_draw():
    a, _ = first_covering(1, 0, 1, 3, 1 << 30)
    b, _ = first_covering(1, 1, 1, 3, 1 << 30)
    c, _ = first_covering(2, 0, 1, 3, 1 << 30)
    assert a != b and a != c and b != c
    seeds = [h(seed, (0x4E4F4900 + k) & M32) for seed in (1, 2) for k in range(4)]
    assert len(set(seeds)) == 8


def test_word_unit_selects_whole_words_and_leaves_word_none_alone():
    # words: [0 0] [1] NONE [2 2 2] [3]; the NONE id is ordinary (an id in front of the first word wraps to NONE too)
    ids = np.array([2000, 2001, 2002, 2003, 2004, 2005, 2006, 2007], np.uint32)
    w = np.array([0, 0, 1, NONE, 2, 2, 2, 3], np.uint32)
    for seed in range(20):
        o = noise_opts(start_q32=1 << 31, seed=seed, unit=WORD, span_min=1, span_max=2, flags=SELECTED)
        s = expected_noise_replace(ids, [0, 8], o, word_ids=w)["selected"].tolist()
        assert s[0] == s[1] and s[4] == s[5] == s[6] and s[3] == 0
        cov, _ = first_covering(seed, 0, 1, 2, 1 << 31, 4)
        assert [s[0], s[2], s[4], s[7]] == [int(c) for c in cov]
    with pytest.raises(ValueError):
        expected_noise_replace(ids, [0, 8], noise_opts(unit=WORD))
    # with sel the unit's word ids are not needed; an id whose word is NONE is still not eligible when they are given
    o = noise_opts(unit=WORD, flags=SELECTED)
    assert expected_noise_replace(ids, [0, 8], o, sel=np.ones(8, np.uint8))["n_selected"] == 8
    assert expected_noise_replace(ids, [0, 8], o, word_ids=w, sel=np.ones(8, np.uint8))["selected"].tolist() == [1, 1, 1, 0, 1, 1, 1, 1]


def test_mask_random_and_keep_follow_the_two_rates():
    ids = np.full(4000, 2000, np.uint32)
    o = noise_opts(start_q32=ONE, mask_q32=ONE // 2, random_q32=ONE // 4, mask_id=6999, seed=3)
    r = expected_noise_replace(ids, [0, 4000], o)
    assert r["n_selected"] == 4000 and np.all(r["labels"] == 2000)
    out = r["input_ids"]
    kept = int(np.sum(out == 2000))
    assert r["n_masked"] == int(np.sum(out == 6999)) and abs(r["n_masked"] / 4000 - 0.5) < 0.05
    assert abs(r["n_random"] / 4000 - 0.25) < 0.05 and abs(kept / 4000 - 0.25) < 0.05      # (5 sigma = 0.04)
    rnd = out[(out != 2000) & (out != 6999)]
    assert rnd.min() >= S0 and rnd.max() < V and len(set(rnd.tolist())) > 500              # a random replacement is never special
    # the sum of the rates at 2^32: nothing is kept
    r = expected_noise_replace(ids, [0, 4000], noise_opts(start_q32=ONE, mask_q32=ONE - 5, random_q32=5, seed=3))
    assert r["n_masked"] + r["n_random"] == 4000


def test_start_q32_zero_changes_nothing():
    ids, offs = pack([[1, 2000, 2001, 2], [], [1, 2]])
    r = expected_noise_replace(ids, offs, noise_opts(mask_q32=ONE, flags=SELECTED))
    assert r["input_ids"].tolist() == ids.tolist() and set(r["labels"].tolist()) == {-100} and r["n_selected"] == 0
    s = expected_noise_spans(ids, offs, noise_opts(n_sentinels=5, flags=SPLIT))
    assert s["inputs"].tolist() == ids.tolist() and s["input_offsets"].tolist() == offs.tolist() and s["n_targets"] == 0


REFUSED = [dict(flags=16), dict(unit=2), dict(span_min=0), dict(span_min=3, span_max=2), dict(span_max=65, span_min=1), dict(start_q32=ONE + 1),
           dict(mask_q32=ONE + 1), dict(mask_q32=ONE, random_q32=1), dict(unit=WORD)]
REFUSED_REPLACE = REFUSED + [dict(mask_id=V)]
REFUSED_SPANS = [dict(flags=SPLIT | 16), dict(flags=0), dict(flags=DESC)] + [dict(x, flags=x.get("flags", 0) | SPLIT) for x in REFUSED[1:]] + [
    dict(flags=SPLIT, final_id=S0), dict(flags=SPLIT, n_sentinels=2, sentinel_first=S0 - 1), dict(flags=SPLIT, n_sentinels=1, sentinel_first=S0),
    dict(flags=SPLIT | DESC, n_sentinels=3, sentinel_first=1), dict(flags=SPLIT | DESC, n_sentinels=1, sentinel_first=S0)]
ACCEPTED_SPANS = [dict(flags=SPLIT, n_sentinels=2, sentinel_first=S0 - 2), dict(flags=SPLIT | DESC, n_sentinels=2, sentinel_first=1),
                  dict(flags=JOINED, n_sentinels=0, sentinel_first=S0 + 5), dict(flags=SPLIT, final_id=S0 - 1)]


def test_what_the_entries_refuse_raises():
    ids, offs = pack([[2000, 2001]])
    for kw in REFUSED_REPLACE:
        with pytest.raises(ValueError):
            expected_noise_replace(ids, offs, noise_opts(**kw))
    for kw in REFUSED_SPANS:
        with pytest.raises(ValueError):
            expected_noise_spans(ids, offs, noise_opts(**kw))
    for kw in ACCEPTED_SPANS:
        expected_noise_spans(ids, offs, noise_opts(**kw))
    expected_noise_replace(ids, offs, noise_opts(mask_id=V - 1, mask_q32=ONE // 2, random_q32=ONE // 2, start_q32=ONE, span_max=64))


# ---- invariants on random inputs ----

def random_batch(rng, n_docs, max_len, p_special=0.1):
    docs = []
    for _ in range(n_docs):
        n = int(rng.integers(0, max_len + 1))
        docs.append([int(rng.integers(0, S0)) if rng.random() < p_special else int(rng.integers(S0, V)) for _ in range(n)])
    return docs


def word_ids_of(rng, docs):
    """Word ids as the words pass writes them: non-decreasing from 0 along a document, NONE on special ids and in front of the first."""
    out = []
    for d in docs:
        w = -1
        for i, x in enumerate(d):
            if x < S0:
                out.append(NONE)
                continue
            if w < 0 and rng.random() < 0.1 and i == 0:
                out.append(NONE)
                continue
            if w < 0 or rng.random() < 0.5:
                w += 1
            out.append(w)
    return np.array(out, np.uint32)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_invariants_of_spans_mode(seed):
    rng = np.random.default_rng(seed)
    S, n_sent = 500, [0, 2, 50][seed]                   # sentinels 500 .. 549; the documents' special ids lie below them
    docs = []
    for _ in range(40):                                 # every id once in its document, so that an id says where it came from
        n = int(rng.integers(0, 61))
        pool = rng.permutation(np.concatenate([rng.choice(500, 8, replace=False), S0 + rng.choice(V - S0, 60, replace=False)]))
        docs.append([int(x) for x in pool[:n]])
    ids, offs = pack(docs)
    o = noise_opts(start_q32=1 << 29, seed=seed, span_min=1, span_max=4, n_sentinels=n_sent, sentinel_first=S, final_id=2, flags=SPLIT | JOINED)
    r = expected_noise_spans(ids, offs, o)
    m = expected_noise_replace(ids, offs, dict(o, flags=SELECTED))
    sel = m["selected"]
    assert r["n_inputs"] + r["n_targets"] == len(ids) + 2 * r["n_runs"] + len(docs)
    inputs, targets = rows(r, "inputs", "input_offsets"), rows(r, "targets", "target_offsets")
    n_hidden = 0
    for d, doc in enumerate(docs):
        assert targets[d][-1] == 2
        a = [x for x in inputs[d] if not S <= x < S + 50]
        b = [x for x in targets[d][:-1] if not S <= x < S + 50]
        at = {x: i for i, x in enumerate(doc)}
        # both in the document's order, no id twice, together every id once
        assert [at[x] for x in a] == sorted(at[x] for x in a) and [at[x] for x in b] == sorted(at[x] for x in b)
        assert not set(a) & set(b) and sorted(a + b) == sorted(doc)
        assert all(sel[int(offs[d]) + at[x]] for x in b)
        sa, sb = [x for x in inputs[d] if S <= x < S + 50], [x for x in targets[d] if S <= x < S + 50]
        assert sa == sb == list(range(S, S + len(sa))) and len(sa) <= n_sent
        n_hidden += len(b)
    assert r["n_selected"] == n_hidden <= m["n_selected"] and (n_sent < 50 or n_hidden == m["n_selected"]) and m["n_selected"] > 0
    # sel given equals the draws reproduced
    again = expected_noise_spans(ids, offs, dict(o, start_q32=0), sel=sel)
    for k in SPANS_ARRAYS:
        assert np.array_equal(again[k], r[k]), k
    assert rows(r, "joined", "joined_offsets") == [i + t for i, t in zip(inputs, targets)]
    assert rows(r, "joined_labels", "joined_offsets") == [[-100] * len(i) + t for i, t in zip(inputs, targets)]


@pytest.mark.parametrize("unit", [TOKEN, WORD])
def test_invariants_of_replace_mode(unit):
    rng = np.random.default_rng(10 + unit)
    docs = random_batch(rng, 30, 80)
    ids, offs = pack(docs)
    w = word_ids_of(rng, docs)
    o = noise_opts(start_q32=1 << 30, mask_q32=ONE // 2, random_q32=ONE // 4, seed=5, unit=unit, span_min=1, span_max=3, mask_id=4, flags=SELECTED)
    r = expected_noise_replace(ids, offs, o, word_ids=w)
    sel = r["selected"].astype(bool)
    assert np.array_equal(r["labels"][sel], ids[sel].astype(np.int32)) and np.all(r["labels"][~sel] == -100)
    assert np.array_equal(r["input_ids"][~sel], ids[~sel]) and np.all(ids[sel] >= S0)
    changed = sel & (r["input_ids"] != ids) & (r["input_ids"] != 4)
    assert np.all(r["input_ids"][changed] >= S0) and r["n_selected"] == int(sel.sum()) and 0 < r["n_selected"] < len(ids)
    if unit == WORD:
        assert not np.any(sel[w == NONE])
    again = expected_noise_replace(ids, offs, dict(o, start_q32=0), word_ids=w, sel=r["selected"])
    for k in REPLACE_ARRAYS + REPLACE_COUNTS:
        assert np.array_equal(again[k], r[k]), k
    other = expected_noise_replace(ids, offs, dict(o, seed=6), word_ids=w)
    assert not np.array_equal(other["selected"], r["selected"])


# ---- the density ----

@pytest.mark.parametrize("rate", [0.15, 0.5])
@pytest.mark.parametrize("span", [(1, 1), (1, 5), (3, 3), (1, 64)])
def test_covered_fraction_is_the_rate_given_to_noise_start_q32(tk, span, rate):
    """One document of n = 2 * 10^5 positions.  A covered flag depends on at most span_max start draws and two flags are dependent
    only within 2 span_max - 1 positions, so Var(mean) <= (2 span_max - 1) p (1 - p) / n; the tolerance is 5 standard deviations of
    that bound (span (1, 64) at 0.5: 0.063; (1, 1): 0.0056), plus 2^-31 for the rounding of start_q32."""
    n = 200000
    sq = tk.noise_start_q32(rate, span[0], span[1])
    o = noise_opts(start_q32=sq, span_min=span[0], span_max=span[1])
    tol = 5.0 * math.sqrt((2 * span[1] - 1) * rate * (1 - rate) / n) + 2.0 ** -31
    for seed in (0, 1):
        s = [h(seed, (0x4E4F4900 + k) & M32) for k in range(2)]
        t0, t1 = h(s[0], 0), h(s[1], 0)
        # the definition's own note: covered(x) iff the largest q + len(q) over the starts q <= x lies behind x
        reach, n_cov = 0, 0
        for x in range(n):
            if h(t0, x) < sq:
                reach = max(reach, x + span[0] + ((h(t1, x) * (span[1] - span[0] + 1)) >> 32))
            n_cov += reach > x
        assert abs(n_cov / n - rate) <= tol, (n_cov / n, tol)
    # ... and that note against step 2 as written, on the head of the document
    o["seed"] = 1
    want = [covered(o, t0, t1, x) for x in range(3000)]
    reach, got = 0, []
    for x in range(3000):
        if h(t0, x) < sq:
            reach = max(reach, x + span[0] + ((h(t1, x) * (span[1] - span[0] + 1)) >> 32))
        got.append(reach > x)
    assert got == want


def test_noise_start_q32_ends_and_refusals(tk):
    assert tk.noise_start_q32(0.0, 1, 5) == 0 and tk.noise_start_q32(1.0, 3, 3) == ONE
    assert abs(tk.noise_start_q32(0.15) / ONE - 0.15) < 1e-9
    assert tk.noise_start_q32(0.15, 1, 5) < tk.noise_start_q32(0.15, 1, 1) and tk.noise_start_q32(0.3, 2, 4) > tk.noise_start_q32(0.15, 2, 4)
    for bad in ((1.5, 1, 1), (-0.1, 1, 1), (0.5, 0, 1), (0.5, 3, 2), (0.5, 1, 65)):
        with pytest.raises(tk.TokenizerError):
            tk.noise_start_q32(*bad)


# ---- the header, the shim, the library and the binding ----

def test_header_values_and_shim_declarations():
    hdr = open(os.path.join(ROOT, "include", "tekken_hip.h")).read()
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bfn\s+%s\s*\(" % name, ffi), name
    for name, value in VALUES.items():
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name
        assert re.search(r"\bconst %s\s*:\s*\w+\s*=\s*%d\s*;" % (name, value), ffi), name
    for st in ("tk_noise_opts", "tk_noise_replace", "tk_noise_spans"):
        assert re.search(r"typedef struct %s\b" % st, hdr), st
    for st in ("TkNoiseOpts", "TkNoiseReplace", "TkNoiseSpans"):
        assert re.search(r"\bstruct %s\b" % st, ffi), st
    assert "0x4E4F4900" in hdr
    assert "tk_noise_replace_device" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    fields = re.search(r"typedef struct tk_noise_opts\s*\{(.*?)\}", hdr, re.S).group(1)
    assert re.sub(r"\s+", " ", fields).strip() == ("uint64_t start_q32, mask_q32, random_q32; uint32_t seed, unit, span_min, span_max, mask_id, "
                                                   "n_sentinels, sentinel_first, final_id, flags; int32_t ignore_index;")


def test_python_constants_and_exported_symbols(tk):
    assert (tk.NOISE_UNIT_TOKEN, tk.NOISE_UNIT_WORD) == (TOKEN, WORD) and tk.NOISE_SPAN_LIMIT == SPAN_LIMIT
    assert (tk.NOISE_SELECTED, tk.NOISE_DESC, tk.NOISE_SPLIT, tk.NOISE_JOINED) == (SELECTED, DESC, SPLIT, JOINED)
    for name in NEW_SYMBOLS:
        assert hasattr(tk.lib(), name), name
    for name in ("noise_replace_device", "noise_spans_device", "encode_batch_device_noise_replace", "encode_batch_device_noise_spans",
                 "encode_batch_noise_replace", "encode_batch_noise_spans", "last_noise_ms"):
        assert hasattr(tk.Engine, name), name
    for name in ("encode_batch_mlm", "encode_batch_span_corruption"):
        assert hasattr(tk.Tekkenizer, name), name
    assert ctypes.sizeof(tk._NoiseOpts) == 64 and [f[0] for f in tk._NoiseOpts._fields_] == list(noise_opts())
    T = tk.lib().tk_noise_tile()                        # (no GPU needed: a constant of the build)
    assert T > 0 and T % 4 == 0


@pytest.mark.parametrize("name,arrays,counts", [("noise_replace", REPLACE_ARRAYS, REPLACE_COUNTS), ("noise_spans", SPANS_ARRAYS, SPANS_COUNTS)])
def test_result_classes_declare_the_header_structs(tk, name, arrays, counts):
    """tests/test_layout_binding_cpu.py's checks, for the two noise results."""
    R, members = {"noise_replace": tk.NoiseReplaceResult, "noise_spans": tk.NoiseSpansResult}[name], header_members(name)
    assert R.PASS == name
    assert [o[0] for o in R.OUTPUTS] == [m for m, ptr in members if ptr] == list(arrays)
    assert list(R.COUNTS) == [m for m, ptr in members if not ptr] == list(counts)
    assert [ptr for _, ptr in members] == sorted((ptr for _, ptr in members), reverse=True)
    assert ctypes.sizeof(R.STRUCT) == sum(ctypes.sizeof(ctypes.c_void_p) if ptr else 8 for _, ptr in members)
    assert [f[0] for f in R.STRUCT._fields_] == [m for m, _ in members]
    for (_, ptr), (_, ctype) in zip(members, R.STRUCT._fields_):
        assert ctype is (ctypes.c_void_p if ptr else ctypes.c_uint64)
    st = R.STRUCT()
    for i, (field, _) in enumerate(R.STRUCT._fields_):
        setattr(st, field, 0x1000 * (i + 1) if field in arrays else i + 2)
    optional = next(o[0] for o in R.OUTPUTS if o[4])
    setattr(st, optional, None)
    r = R(st)
    for (out, ts, shape, _, _), v in zip(R.OUTPUTS, r.views()):
        if out == optional:
            assert getattr(r, out + "_ptr") is None and v is None
            continue
        cai = v.__cuda_array_interface__
        assert cai["data"][0] == getattr(st, out) and cai["shape"] == tuple(shape(r)) and cai["typestr"] == ts
    for k in R.COUNTS:
        assert getattr(r, k) == getattr(st, k)
    assert set(r._counts()) == set(R.DICT_COUNTS) <= set(R.COUNTS)
