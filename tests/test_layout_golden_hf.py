"""The layout passes' HF-named outputs against tests/golden/layout_vectors_hf.json: values from a THIRD-PARTY engine.

Label: independent engine, different authors, NOT the reference.  tools/gen_golden_hf_layout.py records, from HuggingFace
`tokenizers` objects untouched, what the README names after HF: offset_mapping (characters, UTF-16 units), word_ids(), truncation
and padding (sides, pad_to_multiple_of), stride / overflowing windows / overflow_to_sample_mapping, text_pair with longest_first /
only_first / only_second, token_type_ids, sequence_ids, and special strings parsed out of text.  The kernels, the header's
definitions and the restatements of tests/test_*_cpu.py have one author; this file holds both to values of another.

CPU legs: every restatement (expected_dense, expected_windows, expected_pairs, unit_spans_bytewise / unit_spans_str,
expected_spans, expected_words, expected_specials + expected_parsed) over the ORACLE's ids of the fixture's texts -- first asserted
equal to HF's ids.  GPU legs: the Tekkenizer's composite entries from text, so encode, the pass and the copy-out are pinned.
Both legs bring their results into the fixture's shape and go through one comparison, `differences`; a perturbed fixture value
per section shows that it reports.

Where this project deliberately differs from HF the expected side is adjusted for exactly that field, each with the row of the
table in DESIGN.md section 2 ("Deviations from HuggingFace") that lists it:
  D1  the EOS offsets are (len, len) here, (0, 0) in HF;
  D2  byte offsets: HF has none finer than a character, the fixture's are derived from character offsets; a token that begins or
      ends inside a character is compared after widening to the characters it touches (every other token: exactly).
"""
import copy
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SECTIONS = ("offsets", "words", "dense", "windows", "pairs", "specials")
UNITS = ("byte", "char", "utf16")
ENCODING = {"byte": "utf-8", "char": "utf-32-le", "utf16": "utf-16-le"}
UNIT_BYTES = {"byte": 1, "char": 4, "utf16": 2}
SPECIAL_NAMES = ("<unk>", "<s>", "</s>", "<pad>", "[SEP]", "<<mk", "<<mk>>")
KEPT = 8      # the generator's MAX_KEPT_IDS: max_fixed of the only_* strategies (no kept side is longer, so nothing is cut by it)


@pytest.fixture(scope="module")
def hf():
    with open(os.path.join(HERE, "golden", "layout_vectors_hf.json")) as f:
        g = json.load(f)
    with open(os.path.join(HERE, "golden", "merge_vectors_hf.json")) as f:
        m = json.load(f)
    assert "NOT the reference" in g["label"] and "HuggingFace tokenizers" in g["label"] and "merge_vectors_hf.json" in g["label"]
    assert g["num_special"] == m["num_special"] and g["pattern"] == m["pattern"]
    assert g["n_excluded_outside_class"] * 20 <= g["n_texts"]
    for s in SECTIONS:
        assert g[s]["n_cases"] == len(g[s]["cases"]) > 0 and g[s]["n_skipped"] * 10 <= g[s]["n_cases"] + g[s]["n_skipped"], s
    assert g["pairs"]["n_pairs_skipped"] * 10 <= g["pairs"]["n_pairs"] + g["pairs"]["n_pairs_skipped"]
    sp = g["special_ids"]
    assert [sp[n] for n in SPECIAL_NAMES[1:]] == [1, 2, 3, 4, 5, 6] and g["specials"]["strings"] == ["<s>", "</s>", "[SEP]", "<pad>", "<<mk", "<<mk>>"]
    g["tokens"] = [bytes.fromhex(t) for t in m["tokens_hex"]]
    g["docs"] = [bytes.fromhex(t["text_hex"]) for t in g["texts"]]
    g["strs"] = [d.decode("utf-8") for d in g["docs"]]
    g["special_docs"] = [bytes.fromhex(c["text_hex"]) for c in g["specials"]["cases"]]
    return g


# ---- the one comparison of both legs ----

def differences(exp, got, path="", limit=5):
    """Where two nested structures of dicts, lists and numbers differ: a list of (path, expected, got), at most `limit`."""
    out = []

    def walk(e, g, p):
        if len(out) >= limit:
            return
        if isinstance(e, dict):
            if not isinstance(g, dict) or set(e) != set(g):
                out.append((p, sorted(e), sorted(g) if isinstance(g, dict) else type(g).__name__))
                return
            for k in e:
                walk(e[k], g[k], "%s.%s" % (p, k))
        elif isinstance(e, list):
            if not isinstance(g, list) or len(e) != len(g):
                out.append((p, "list of %d" % len(e), "list of %d" % len(g) if isinstance(g, list) else type(g).__name__))
                return
            for k in range(len(e)):
                walk(e[k], g[k], "%s[%d]" % (p, k))
        elif type(e) is not type(g) or e != g:
            out.append((p, e, g))

    walk(exp, got, path)
    return out


def assert_same(exp, got, what):
    bad = differences(exp, got, what)
    assert not bad, bad


# ---- the expected side: the fixture, with the listed deviations applied to exactly their fields ----

def length_in(text, unit):
    return len(text.encode(ENCODING[unit])) // UNIT_BYTES[unit]


def expected_of(hf, section):
    cases = copy.deepcopy(hf[section]["cases"])
    if section == "offsets":
        out = []
        for text, c in zip(hf["strs"], cases):
            for unit in UNITS:
                assert c[unit + "_sp"][-2:] == [0, 0]
                c[unit + "_sp"][-2:] = [length_in(text, unit)] * 2                        # D1: EOS is (len, len) here
            out.append(c)
        return out
    if section == "windows":
        out = []
        for c in cases:
            for row, d in zip(c["offsets"], c["sample"]):
                assert row[:2] == [0, 0] and row[-2:] == [0, 0]
                row[-2:] = [len(hf["strs"][d])] * 2                                          # D1, the EOS of every window
            out.append({k: c[k] for k in ("sample", "ids", "offsets", "mask_longest", "mask_fixed")})
        return out
    if section == "pairs":
        return [{k: c[k] for k in ("sample", "ids", "type_ids", "sequence_ids", "offsets", "attention_mask")} for c in cases]
    if section == "dense":
        return [{k: c[k] for k in ("ids", "attention_mask", "lengths")} for c in cases]
    if section == "specials":
        return [{"ids": c["ids"]} for c in cases]
    return cases


# ---- what both legs share to bring their results into the fixture's shape ----

def flat(spans):
    return [int(x) for p in spans for x in p]


def widened(doc, spans):
    """D2: byte spans widened to the characters they touch (a span on character boundaries, or an empty one, is unchanged)."""
    from test_spans_units_cpu import widened_bytes
    return [tuple(widened_bytes(doc, int(s), int(e))) if s < e else (int(s), int(e)) for s, e in spans]


def rows_of(a, lengths):
    return [a[r, :int(n)].tolist() for r, n in enumerate(lengths)]


def span_rows(sp, lengths):
    return [sp[r, :int(n)].reshape(-1).tolist() for r, n in enumerate(lengths)]


def ragged(rows):
    oo = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return np.array([i for r in rows for i in r], np.int64), oo


def pair_texts(hf, c):
    return [hf["strs"][a] for a, _ in c["pairs"]], [hf["strs"][b] for _, b in c["pairs"]]


# ---- the CPU legs: the restatements over the oracle's ids ----

@pytest.fixture(scope="module")
def orc(hf):
    import tk_oracle
    o = tk_oracle.Oracle(hf["tokens"], hf["num_special"], 1, 2)
    got = [o.encode(d, False, False) for d in hf["docs"]]
    for d, t, g in zip(hf["docs"], hf["texts"], got):
        assert g == t["ids"], ("the oracle's ids are not HF's", d[:60], t["ids"][:12], g[:12])
    return {"oracle": o, "plain": got, "sp": [[1] + g + [2] for g in got]}


def cpu_offsets(hf, orc):
    from test_spans_cpu import expected_spans
    from test_spans_units_cpu import BYTE, CHAR, UTF16, locate_brute, unit_spans_bytewise, unit_spans_str
    tok_len, ns = [len(t) for t in hf["tokens"]], hf["num_special"]
    out = [{} for _ in hf["docs"]]
    for key, rows in (("", orc["plain"]), ("_sp", orc["sp"])):
        ids, oo = ragged(rows)
        for unit, code in (("char", CHAR), ("utf16", UTF16)):
            a = unit_spans_bytewise(ids, oo, hf["tokens"], ns, code)
            b = unit_spans_str(ids, oo, hf["tokens"], ns, code)
            assert np.array_equal(a, b), "the two restatements disagree (%s)" % unit
            for d in range(len(out)):
                out[d][unit + key] = flat(a[oo[d]:oo[d + 1]])
        a = expected_spans(ids, oo, tok_len, ns)
        assert np.array_equal(a, unit_spans_bytewise(ids, oo, hf["tokens"], ns, BYTE))
        for d, doc in enumerate(hf["docs"]):
            out[d]["byte" + key] = flat(widened(doc, a[oo[d]:oo[d + 1]].tolist()))
    for d, text in enumerate(hf["strs"]):               # HF's char_to_token(c): the first id the range (c, c + 1) overlaps
        sp = out[d]["char"]
        r = locate_brute(list(zip(sp[::2], sp[1::2])), [0, len(sp) // 2], [0] * len(text), [(c, c + 1) for c in range(len(text))])
        assert np.all(r[:, 0] < r[:, 1])
        out[d]["char_to_token"] = r[:, 0].tolist()
    return out


def cpu_words(hf, orc):
    import tk_oracle
    from test_words_cpu import expected_words
    data = np.frombuffer(b"".join(hf["docs"]), np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(d) for d in hf["docs"]])]).astype(np.int64)
    out = [{} for _ in hf["docs"]]
    for key, rows in (("", orc["plain"]), ("_sp", orc["sp"])):
        ids, oo = ragged(rows)
        w = expected_words(ids, oo, hf["tokens"], hf["num_special"], data, offs, tk_oracle.split)
        dw = w["doc_words"].astype(np.int64)
        for d in range(len(out)):
            out[d]["word_ids" + key] = w["word_ids"][oo[d]:oo[d + 1]].tolist()
            out[d]["word_first" + key] = w["word_first"][dw[d]:dw[d + 1]].tolist()         # HF's word_to_tokens(w)[0]
    return out


def cpu_dense(hf, orc):
    from test_dense_cpu import FIXED, MASK, PAD_LEFT, TRUNC_LEFT, expected_dense
    ids, oo = ragged(orc["sp"])
    out = []
    for c in hf["dense"]["cases"]:
        flags = MASK | (FIXED if c["fixed"] else 0) | (PAD_LEFT if c["padding_side"] == "left" else 0) \
            | (TRUNC_LEFT if c["truncation_side"] == "left" else 0)
        e = expected_dense(ids, oo, c["max_length"], c["multiple_of"] or 0, hf["special_ids"]["<pad>"], 1, 1, flags)
        out.append({"ids": e["dense"].tolist(), "attention_mask": e["mask"].tolist(), "lengths": e["lengths"].tolist()})
    return out


def char_spans(hf, rows):
    from test_spans_units_cpu import CHAR, unit_spans_bytewise
    ids, oo = ragged(rows)
    return ids, oo, unit_spans_bytewise(ids, oo, hf["tokens"], hf["num_special"], CHAR)


def cpu_windows(hf, orc):
    from test_window_cpu import FIXED, MASK, SPANS, expected_windows
    ids, oo, spans = char_spans(hf, orc["sp"])
    out = []
    for c in hf["windows"]["cases"]:
        e = expected_windows(ids, oo, c["max_length"], c["stride"], 1, 1, 0, hf["special_ids"]["<pad>"], MASK | SPANS, spans)
        f = expected_windows(ids, oo, c["max_length"], c["stride"], 1, 1, 0, hf["special_ids"]["<pad>"], MASK | FIXED)
        out.append({"sample": e["window_doc"].tolist(), "ids": rows_of(e["input_ids"], e["lengths"]),
                    "offsets": span_rows(e["spans"], e["lengths"]), "mask_longest": e["mask"].tolist(), "mask_fixed": f["mask"].tolist()})
    return out


def cpu_pairs(hf, orc):
    import test_pair_cpu as P
    sp = hf["special_ids"]
    out = []
    for c in hf["pairs"]["cases"]:
        ids, oo, spans = char_spans(hf, [orc["plain"][i] for pair in c["pairs"] for i in pair])
        flags = P.FIXED | P.MASK | P.TYPE_IDS | P.SEQUENCE_IDS | P.SPANS | (P.OVERFLOW if c["overflow"] else 0)
        strategy = {"longest_first": P.LONGEST_FIRST, "only_first": P.ONLY_FIRST, "only_second": P.ONLY_SECOND}[c["strategy"]]
        e = P.expected_pairs(ids, oo, c["max_length"], strategy, c["stride"], KEPT if c["overflow"] else 0, 0, sp["<pad>"], [sp["<s>"]],
                             [sp["[SEP]"]], [sp["</s>"]], flags, spans)
        assert e["n_fixed_cut"] == 0
        n = e["lengths"]
        out.append({"sample": e["window_pair"].tolist(), "ids": rows_of(e["input_ids"], n), "type_ids": rows_of(e["type_ids"], n),
                    "sequence_ids": rows_of(e["sequence_ids"], n), "offsets": span_rows(e["spans"], n), "attention_mask": e["mask"].tolist()})
    return out


def cpu_specials(hf, orc):
    from test_specials_cpu import PARSE, TEXT, expected_parsed
    docs = hf["special_docs"]
    data = np.frombuffer(b"".join(docs), np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    strings = [s.encode() for s in SPECIAL_NAMES]
    ids, oo = expected_parsed(orc["oracle"], data, offs, strings, [TEXT] + [PARSE] * 6, False, False)
    return [{"ids": ids[int(oo[d]):int(oo[d + 1])].tolist()} for d in range(len(docs))]


CPU = {"offsets": cpu_offsets, "words": cpu_words, "dense": cpu_dense, "windows": cpu_windows, "pairs": cpu_pairs, "specials": cpu_specials}


@pytest.fixture(scope="module")
def cpu_got(hf, orc):
    return {s: CPU[s](hf, orc) for s in SECTIONS}


def test_generator_uses_only_the_third_party_engine():
    """Neither the oracle nor the package nor a restatement of the tests is imported by the generator: the recorded values are
    HuggingFace's.  What it takes from gen_golden_hf.py is the pattern, the byte alphabet and the class check."""
    src = open(os.path.join(HERE, "..", "tools", "gen_golden_hf_layout.py")).read()
    for banned in ("import tk_oracle", "tekken-rs_amd", "import synth_vocab", "import gen_golden_merge", "import helpers", "from test_",
                   "import test_", "oracle/"):
        assert banned not in src, banned
    assert "from tokenizers import" in src and "from gen_golden_hf import NUM_SPECIAL, PATTERN, bytes_to_unicode, in_class" in src


def test_fixture_has_the_cases_it_is_for(hf):
    """Empty and one-character texts, tokens inside a character, astral characters; every dense length, side and multiple; every
    window and pair parameter; pairs with equal sides over the budget and with an empty side; the special strings' placements."""
    ids = [t["ids"] for t in hf["texts"]]
    assert 35 <= len(ids) <= 50 and max(len(d) for d in hf["docs"]) <= 600
    assert [] in ids and sum(len(s) == 1 for s in hf["strs"]) >= 4
    assert any(any(ord(ch) >= 0x10000 for ch in s) for s in hf["strs"])
    inside = sum(1 for c in hf["offsets"]["cases"] for k in range(0, len(c["char"]) - 2, 2) if c["char"][k] == c["char"][k + 2])
    assert inside > 20, "tokens that begin inside a character"
    for c in hf["offsets"]["cases"]:                    # HF gives BOS and EOS (0, 0) and leaves the other offsets alone
        assert all(c[u + "_sp"] == [0, 0] + c[u] + [0, 0] for u in UNITS)
    D = hf["dense"]["cases"]
    assert {(c["max_length"], c["truncation_side"]) for c in D} == {(T, s) for T in (8, 13, 16) for s in ("right", "left")}
    assert {(c["multiple_of"], c["padding_side"], c["fixed"]) for c in D} == {(m, s, f) for m in (None, 4, 7) for s in ("right", "left") for f in (False, True)}
    assert [(c["max_length"], c["stride"]) for c in hf["windows"]["cases"]] == [(7, 2), (16, 0), (16, 5), (33, 8)]
    assert all(max(c["sample"].count(d) for d in set(c["sample"])) > 2 for c in hf["windows"]["cases"])
    P = hf["pairs"]["cases"]
    assert {(c["strategy"], c["max_length"], c["stride"]) for c in P} == \
        {(s, 20, 0) for s in ("longest_first", "only_first", "only_second")} | {(s, 41, 0) for s in ("longest_first",)} \
        | {(s, T, st) for s in ("only_first", "only_second") for T, st in ((20, 4), (41, 7))}
    for c in P:
        n = [(len(ids[a]), len(ids[b])) for a, b in c["pairs"]]
        assert any(a == 0 for a, _ in n) and any(b == 0 for _, b in n)
        if c["strategy"] != "longest_first":
            assert all((a if c["strategy"] == "only_second" else b) <= KEPT for a, b in n) and len(c["ids"]) > len(c["pairs"])
    assert any(a == b and a + b + 3 > 20 for c in P if c["strategy"] == "longest_first" for a, b in [(len(ids[x]), len(ids[y])) for x, y in c["pairs"]])
    S = hf["special_docs"]
    assert b"a <<mk>> b" in S and b"a <<mk b" in S and b"<<m" in S and b"<<mk<<mk>>" in S and any(d.startswith(b"<s>") and d.endswith(b"</s>") for d in S)


@pytest.mark.parametrize("section", SECTIONS)
def test_restatements_match_hf(hf, cpu_got, section):
    assert_same(expected_of(hf, section), cpu_got[section], section)


# ---- a leg that can fail: one recorded value perturbed in memory, per section and field ----

def _bump(lst, k, by=1):
    lst[k] += by


MUTATIONS = [
    ("offsets", "a character offset", lambda cs: _bump(next(c for c in cs if len(c["char"]) > 6)["char"], 5)),
    ("offsets", "a UTF-16 offset", lambda cs: _bump(next(c for c in cs if c["utf16"] != c["char"])["utf16_sp"], 4)),
    ("offsets", "a byte offset", lambda cs: _bump(next(c for c in cs if len(c["byte"]) > 6)["byte"], 2)),
    ("words", "a word id", lambda cs: _bump(next(c for c in cs if len(c["word_ids"]) > 3)["word_ids"], 3)),
    ("offsets", "a char_to_token", lambda cs: _bump(next(c for c in cs if len(c["char_to_token"]) > 3)["char_to_token"], 2)),
    ("words", "the first id of a word", lambda cs: _bump(next(c for c in cs if len(c["word_first_sp"]) > 2)["word_first_sp"], 1)),
    ("words", "the word of BOS", lambda cs: cs[0]["word_ids_sp"].__setitem__(0, 0)),
    ("dense", "an id", lambda cs: _bump(cs[3]["ids"][2], 1)),
    ("dense", "a mask element", lambda cs: cs[4]["attention_mask"][1].__setitem__(0, 1 - cs[4]["attention_mask"][1][0])),
    ("dense", "a length", lambda cs: _bump(cs[0]["lengths"], 0, -1)),
    ("windows", "a window's sample index", lambda cs: _bump(cs[0]["sample"], 1)),
    ("windows", "an id of an overlap", lambda cs: _bump(cs[2]["ids"][1], 1)),
    ("windows", "an offset", lambda cs: _bump(cs[3]["offsets"][0], 3)),
    ("windows", "a mask element", lambda cs: cs[1]["mask_longest"][0].__setitem__(0, 0)),
    ("pairs", "a type id", lambda cs: cs[0]["type_ids"][0].__setitem__(-1, 0)),
    ("pairs", "a sequence id", lambda cs: cs[1]["sequence_ids"][0].__setitem__(1, 1 - cs[1]["sequence_ids"][0][1])),
    ("pairs", "a row's sample index", lambda cs: _bump(cs[2]["sample"], 2)),
    ("pairs", "an id", lambda cs: _bump(cs[3]["ids"][0], 1)),
    ("pairs", "an offset", lambda cs: _bump(cs[4]["offsets"][0], 3)),
    ("specials", "a special id", lambda cs: cs[0]["ids"].__setitem__(0, 2)),
    ("specials", "an id", lambda cs: _bump(cs[3]["ids"], 0)),
]


@pytest.mark.parametrize("section,what,mutate", MUTATIONS, ids=["%s: %s" % m[:2] for m in MUTATIONS])
def test_a_perturbed_fixture_value_is_reported(hf, cpu_got, section, what, mutate):
    """The comparison both legs go through, on the fixture with one value changed: it must report it (a window's sample index also moves
    the EOS offsets of D1, which are the length of the sample's text)."""
    g = dict(hf)
    g[section] = copy.deepcopy(hf[section])
    mutate(g[section]["cases"])
    bad = differences(expected_of(g, section), cpu_got[section], section)
    assert 1 <= len(bad) <= 3 and bad[0][0].startswith(section), (what, bad)


# ---- the GPU legs: from text through the Tekkenizer's composite entries ----

@pytest.fixture(scope="module")
def tkz(tk, hf):
    from test_host_tokenizer import model
    t = tk.Tekkenizer.from_json(json.dumps(model(hf["tokens"], num_special=hf["num_special"], specials=SPECIAL_NAMES)), device=0)
    sp = hf["special_ids"]
    assert (t.bos_id(), t.eos_id(), t.pad_id()) == (sp["<s>"], sp["</s>"], sp["<pad>"])
    assert [t.get_control_token(n) for n in SPECIAL_NAMES] == list(range(7))
    yield t
    t.close()


@pytest.mark.gpu
def test_gpu_ids_match_hf(tkz, hf):
    assert_same([t["ids"] for t in hf["texts"]], tkz.encode_batch(hf["strs"]), "ids")


@pytest.mark.gpu
def test_gpu_offsets_match_hf(tkz, hf):
    got = [{} for _ in hf["docs"]]
    for key, sp in (("", False), ("_sp", True)):
        for unit in UNITS:
            r = tkz.encode_batch_with_offsets(hf["strs"], sp, sp, offsets_unit=unit)
            for d, (ids, spans) in enumerate(r):
                assert ids == [1] * sp + hf["texts"][d]["ids"] + [2] * sp
                got[d][unit + key] = flat(widened(hf["docs"][d], spans) if unit == "byte" else spans)
    r = tkz.encode_batch_with_alignment(hf["strs"], [[(c, c + 1) for c in range(len(s))] for s in hf["strs"]], offsets_unit="char")
    ao = r["ann_offsets"]
    for d in range(len(got)):
        got[d]["char_to_token"] = r["token_ranges"][ao[d]:ao[d + 1], 0].tolist()
    assert_same(expected_of(hf, "offsets"), got, "offsets")


@pytest.mark.gpu
def test_gpu_words_match_hf(tkz, hf):
    got = [{} for _ in hf["docs"]]
    for key, sp in (("", False), ("_sp", True)):
        r = tkz.encode_batch_with_words(hf["strs"], sp, sp)
        oo, dw = r["id_offsets"], r["doc_words"]
        for d in range(len(got)):
            assert r["ids"][oo[d]:oo[d + 1]].tolist() == [1] * sp + hf["texts"][d]["ids"] + [2] * sp
            got[d]["word_ids" + key] = r["word_ids"][oo[d]:oo[d + 1]].view(np.uint32).tolist()
            got[d]["word_first" + key] = r["word_first"][dw[d]:dw[d + 1]].tolist()
    assert_same(expected_of(hf, "words"), got, "words")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_gpu_dense_matches_hf(tkz, hf, dtype):
    got = []
    for c in hf["dense"]["cases"]:
        r = tkz.encode_batch_padded(hf["strs"], True, True, max_length=c["max_length"], padding="max_length" if c["fixed"] else "longest",
                                    truncation_side=c["truncation_side"], padding_side=c["padding_side"], pad_to_multiple_of=c["multiple_of"],
                                    dtype=dtype, return_tensors="np")
        assert r["input_ids"].dtype == np.dtype(dtype)
        got.append({"ids": r["input_ids"].tolist(), "attention_mask": r["attention_mask"].tolist(), "lengths": r["lengths"].tolist()})
    assert_same(expected_of(hf, "dense"), got, "dense")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_gpu_windows_match_hf(tkz, hf, dtype):
    got = []
    for c in hf["windows"]["cases"]:
        kw = dict(add_bos=True, add_eos=True, dtype=dtype, return_tensors="np")
        r = tkz.encode_batch_windows(hf["strs"], c["max_length"], c["stride"], padding="longest", return_offsets_mapping=True,
                                     offsets_unit="char", **kw)
        f = tkz.encode_batch_windows(hf["strs"], c["max_length"], c["stride"], padding="max_length", **kw)
        assert r["input_ids"].dtype == np.dtype(dtype) and f["input_ids"].shape[1] == c["max_length"]
        assert np.array_equal(f["input_ids"][:, :r["input_ids"].shape[1]], r["input_ids"]) and np.array_equal(f["lengths"], r["lengths"])
        got.append({"sample": r["overflow_to_sample_mapping"].tolist(), "ids": rows_of(r["input_ids"], r["lengths"]),
                    "offsets": span_rows(r["offset_mapping"], r["lengths"]), "mask_longest": r["attention_mask"].tolist(),
                    "mask_fixed": f["attention_mask"].tolist()})
    assert_same(expected_of(hf, "windows"), got, "windows")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_gpu_pairs_match_hf(tkz, hf, dtype):
    got = []
    for c in hf["pairs"]["cases"]:
        first, second = pair_texts(hf, c)
        r = tkz.encode_pairs(first, second, c["max_length"], truncation=c["strategy"], stride=c["stride"], return_overflowing_tokens=c["overflow"],
                             max_fixed=KEPT if c["overflow"] else None, sep=[hf["special_ids"]["[SEP]"]], padding="max_length", dtype=dtype,
                             return_sequence_ids=True, return_offsets_mapping=True, offsets_unit="char", return_tensors="np")
        assert r["input_ids"].dtype == np.dtype(dtype) and r["n_fixed_cut"] == 0
        n = r["lengths"]
        got.append({"sample": r["overflow_to_sample_mapping"].tolist(), "ids": rows_of(r["input_ids"], n), "type_ids": rows_of(r["token_type_ids"], n),
                    "sequence_ids": rows_of(r["sequence_ids"], n), "offsets": span_rows(r["offset_mapping"], n),
                    "attention_mask": r["attention_mask"].tolist()})
    assert_same(expected_of(hf, "pairs"), got, "pairs")


@pytest.mark.gpu
def test_gpu_specials_match_hf(tkz, hf):
    docs = [d.decode("utf-8") for d in hf["special_docs"]]
    r = tkz.encode_batch_with_specials(docs, allowed=SPECIAL_NAMES[1:])
    oo = r["id_offsets"]
    assert_same(expected_of(hf, "specials"), [{"ids": r["ids"][int(oo[d]):int(oo[d + 1])].tolist()} for d in range(len(docs))], "specials")
