"""Special-token strings parsed out of text on the GPU (include/tekken_hip.h tk_specials_split_device and the entries around it,
csrc/tk_specials.hip) against the plain-loop restatement of the definition in tests/test_specials_cpu.py -- element by element
over every output, through the three entries."""
import json

import numpy as np
import pytest

import helpers
from helpers import dev, to_host
from test_gpu_spans import pack, sweep_docs
from test_specials_cpu import BOS, EOS, PARSE, PART_SRC, RAISE, TEXT, SpecialRaise, expected_parsed, expected_specials

pytestmark = pytest.mark.gpu

ARRAYS = ("bytes", "part_offsets", "part_ctrl", "conv_offsets", "part_src")
COUNTS = ("n_parts", "n_bytes", "n_matches", "n_removed")
N_SPECIAL = 1000                # tests/helpers.py small_trained_vocab
LONG = b"{" + b"0123456789" * 25 + b"wxyz"            # 255 bytes: the longest string that can be matched
FILL = b"the quick red fox, 12 jumps over (lazy) dogs. "     # no string of either set


def tekken_like():
    """What a Tekken vocabulary has: control tokens and the <SPECIAL_n> fillers, a thousand strings behind two first bytes."""
    s = [b"<unk>", b"<s>", b"</s>", b"[INST]", b"[/INST]", b"[PREFIX]", b"[SUFFIX]", b"[MIDDLE]"]
    return s + [b"<SPECIAL_%d>" % i for i in range(len(s), N_SPECIAL)], None


def nasty():
    """Single bytes, prefixes of each other, overlapping pairs, a string that overlaps itself, equal strings, a TEXT string that is
    a prefix of a PARSE one, the longest string there can be, runs of 1 .. 17 of one byte; every other id has no string (TEXT)."""
    s = [b"#", b"ab", b"bc", b"aa", b"<a", b"<ab>", b"<a>", LONG, b"[X]", b"[X]", b"q", b"qr"] + [b"~" * l for l in range(1, 18)]
    modes = [PARSE] * len(s) + [TEXT] * (N_SPECIAL - len(s))
    modes[10] = TEXT
    return s + [b""] * (N_SPECIAL - len(s)), modes


SETS = {"tekken": tekken_like(), "nasty": nasty()}


@pytest.fixture(scope="module")
def eng(tk, test_vocab):
    e = tk.Engine(test_vocab["tokens"], test_vocab["num_special"], test_vocab["bos"], test_vocab["eos"], device=0)
    e.current = None
    yield e
    e.close()


@pytest.fixture(scope="module")
def T(tk):
    return int(tk.lib().tk_specials_tile())           # the candidate kernel's tile, from the library


def use(eng, name):
    """The engine with string set `name`: (strings, modes)."""
    if eng.current != name:
        eng.set_special_tokens(SETS[name][0])
        eng.current = name
    return SETS[name]


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def upload(docs):
    """(data, offs, uint8 tensor of exactly n_bytes or None, its pointer, offsets tensor)"""
    import torch
    data, offs = pack(docs)
    d = torch.from_numpy(data).cuda() if len(data) else None
    return data, offs, d, (d.data_ptr() if d is not None else 0), dev(offs, np.uint64)


def fetch(res):
    """SpecialsResult -> dict like expected_specials'."""
    v = res.views()
    out = {"bytes": to_host(v[0], res.n_bytes, np.uint8), "part_offsets": to_host(v[1], res.n_parts + 1, np.uint64),
           "part_ctrl": to_host(v[2], res.n_parts, np.uint32), "conv_offsets": to_host(v[3], res.n_docs + 1, np.uint64),
           "part_src": to_host(v[4], res.n_parts, np.uint64)}
    out.update({k: getattr(res, k) for k in COUNTS})
    return out


def assert_same(got, exp, what=""):
    helpers.assert_same(got, exp, what, COUNTS, ARRAYS)


def check_split(eng, name, docs, flags=PART_SRC, modes="set", what=""):
    """The device split of docs against the restatement; -> (the expected dict, the SpecialsResult, the text tensor)."""
    strings, m = use(eng, name)
    m = m if modes == "set" else modes
    data, offs, d, ptr, o = upload(docs)
    res = eng.split_specials_device(ptr, o.data_ptr(), len(docs), len(data), m, flags, 0, stream())
    exp = expected_specials(data, offs, strings, m, flags)
    assert_same(fetch(res), exp, what)
    return exp, res, d


def check_all(eng, orc, name, docs, add_bos=True, add_eos=True, modes="set", what=""):
    """... and the two composite entries: their parts against the restatement, their ids against step 5 through the oracle."""
    strings, m = use(eng, name)
    m = m if modes == "set" else modes
    flags = (BOS if add_bos else 0) | (EOS if add_eos else 0)
    for f in (flags, flags | PART_SRC):
        check_split(eng, name, docs, f, m, what)
    data, offs, d, ptr, o = upload(docs)
    exp = expected_specials(data, offs, strings, m, flags | PART_SRC)
    ids, oo = expected_parsed(orc, data, offs, strings, m, add_bos, add_eos)
    parts, j = eng.encode_batch_device_parsed(ptr, o.data_ptr(), len(docs), len(data), add_bos, add_eos, m, PART_SRC, checks=3, stream=stream())
    assert_same(fetch(parts), exp, (what, "device composite"))
    v = j.views()
    helpers.assert_array_same(to_host(v[0], j.n_ids, np.uint32), ids, (what, "ids"))
    helpers.assert_array_same(to_host(v[1], j.n_convs + 1, np.uint64), oo, (what, "offsets"))
    assert j.n_ctrl == exp["n_matches"] + len(docs) * (int(add_bos) + int(add_eos))
    hj, hp = eng.encode_batch_parsed(data, offs, add_bos, add_eos, m, PART_SRC, validate_utf8=True, return_parts=True)
    assert_same(hp, exp, (what, "host composite"))
    helpers.assert_array_same(hj["ids"], ids, (what, "host ids"))
    helpers.assert_array_same(hj["offsets"], oo, (what, "host offsets"))
    return exp


@pytest.fixture(scope="module")
def orc(test_vocab):
    return helpers.oracle_for(test_vocab)


def filler(n, salt=0):
    return (FILL * (n // len(FILL) + 2))[salt % len(FILL):][:n]


def at_tile_offsets(T, string, ks, tail=b" end"):
    """One document per k: the string begins k bytes in front of a tile boundary of the packed text."""
    docs, g = [], 0
    for k in ks:
        pad = (-(g + k)) % T + (T if (-(g + k)) % T < 300 else 0)   # (room for text in front of the string)
        doc = filler(pad, k) + string + tail
        assert (g + pad + k) % T == 0
        docs.append(doc)
        g += len(doc)
    return docs


# ---- tile boundaries of the candidate kernel ----

@pytest.mark.parametrize("name,string", [("tekken", b"[/INST]"), ("tekken", b"<SPECIAL_20>"), ("nasty", LONG)])
def test_a_match_straddles_a_tile_boundary_at_every_split_point(eng, T, name, string):
    docs = at_tile_offsets(T, string, range(len(string) + 1))
    exp, _, _ = check_split(eng, name, docs, BOS | PART_SRC)
    assert exp["n_matches"] == len(docs)


def test_a_match_cut_by_a_document_boundary_on_before_and_behind_a_tile_boundary(eng, T):
    s = b"[/INST]"
    docs = []
    for delta in (-1, 0, 1):                            # the documents' boundary relative to a tile boundary
        for cut in range(1, len(s)):
            g = sum(len(x) for x in docs)
            pad = (-(g + cut) + delta) % T + T
            docs += [filler(pad, cut) + s[:cut], s[cut:] + b" tail"]
            assert (g + pad + cut - delta) % T == 0
    exp, res, d = check_split(eng, "tekken", docs, EOS)
    assert exp["n_matches"] == 0 and res.bytes_ptr == d.data_ptr()


def test_an_overlap_cluster_crosses_a_tile_boundary(eng, T):
    rng = np.random.default_rng(3)
    cluster = bytes(rng.choice(np.frombuffer(b"aabbc<>#q", np.uint8), 96))
    docs = at_tile_offsets(T, cluster, (1, 17, 48, 95), tail=b"")
    exp, _, _ = check_split(eng, "nasty", docs)
    assert exp["n_matches"] > 60


def test_a_run_of_overlapping_candidates_is_one_long_chain(eng, T):
    _, modes = use(eng, "nasty")
    only_aa = [PARSE if i == 3 else TEXT for i in range(N_SPECIAL)]
    run = b"a" * (3 * T + 1)                            # 3T candidates, a chain of more than 1.5 T links
    exp, _, _ = check_split(eng, "nasty", [run], BOS | EOS, only_aa)
    assert exp["n_matches"] == (3 * T) // 2 and exp["bytes"].tobytes() == b"a"
    check_split(eng, "nasty", [b"xy", run, b"", run[:-1], b"aaa"], PART_SRC, only_aa)


def test_the_parity_of_a_run_does_not_leak_into_the_next_document(eng, T):
    only_aa = [PARSE if i == 3 else TEXT for i in range(N_SPECIAL)]
    for odd in (0, 1):
        docs = [filler(T - 40) + b"a" * (38 + odd), b"a" * 41, b"a", b"aa", b"a" * (T + 3)]
        exp, _, _ = check_split(eng, "nasty", docs, PART_SRC, only_aa)
        # every document starts its own walk at its own first byte
        assert exp["n_matches"] == (38 + odd) // 2 + 20 + 0 + 1 + (T + 3) // 2
        assert exp["part_src"][int(exp["conv_offsets"][1]) + 1] == len(docs[0]) + 2


# ---- hand-made documents through all three entries ----

def test_matches_at_the_edges_of_documents_and_of_the_buffer(eng, orc):
    docs = [b"<s>[INST] hi there [/INST]fine</s>",      # matches at the document's start and end, adjacent matches
            b"[INST]",                                  # a document that is one match
            b"", b"",                                   # empty documents between matching ones
            b"</s></s></s>",                            # nothing but matches: every text is empty
            b"plain text, no marker",
            b"a < b and c[3] > d <SPECIAL_9 <SPECIAL_99>x<SPECIAL_999><SPECIAL_1000>",
            b"tail [/INST]"]                            # a match in the last bytes of the buffer
    for bos, eos in ((True, True), (False, False), (True, False), (False, True)):
        exp = check_all(eng, orc, "tekken", docs, bos, eos)
    assert exp["n_matches"] == 11
    check_all(eng, orc, "tekken", docs[:-1] + [b"tail [/INS"])       # a proper prefix of a string as the buffer's last bytes
    check_all(eng, orc, "tekken", [b"<"], False, False)
    check_all(eng, orc, "nasty", [b"<ab>x<a>y<a", b"abcd", b"xbcd", b"aaaaa", b"[X]", b"q qr qqr", LONG, LONG[:-1], b"#" * 33, b"<ab"])


def test_no_document_and_no_byte(eng, orc):
    check_all(eng, orc, "tekken", [])
    check_all(eng, orc, "tekken", [b"", b"", b""])
    check_all(eng, orc, "tekken", [b""], False, False)


def test_an_empty_match_set_gives_the_text_back(eng, orc):
    docs = [b"<s>[INST] hi [/INST]", b"", b"x"]
    text = [TEXT] * N_SPECIAL
    exp = check_all(eng, orc, "tekken", docs, modes=text)
    assert exp["n_matches"] == 0 and exp["n_parts"] == 6
    _, res, d = check_split(eng, "tekken", docs, 0, text)
    assert res.bytes_ptr == d.data_ptr()                # not copied
    _, res, d = check_split(eng, "tekken", [b"no marker here", b"<SPECIAL_x>"], BOS)
    assert res.n_removed == 0 and res.bytes_ptr == d.data_ptr()
    _, res, d = check_split(eng, "tekken", [b"one <s> marker"], BOS)
    assert res.n_removed == 3 and res.bytes_ptr != d.data_ptr()


def test_every_flag_combination(eng):
    docs = [b"<s>a[INST]bc[/INST]", b"", b"</s>", b"d" * 100 + b"[MIDDLE]" + b"e" * 100]
    for flags in range(8):
        check_split(eng, "tekken", docs, flags)


def test_compaction_at_every_misalignment(eng):
    rng = np.random.default_rng(11)
    seg = lambda n: bytes(rng.choice(np.frombuffer(b"cdefghij klmnop", np.uint8), n))
    docs = [b"".join(b"~" * l + seg(64 + l) for l in range(1, 18))]      # removed lengths 1 .. 17 in front of segments of 64 bytes and more
    docs += [seg(5) + b"~" * l + seg(80) for l in range(1, 18)]
    exp, _, _ = check_split(eng, "nasty", docs)
    assert exp["n_removed"] == 2 * sum(range(1, 18))
    exp, _, _ = check_split(eng, "nasty", [b"cd~ef"])   # an output of fewer than 16 bytes
    assert exp["bytes"].tobytes() == b"cdef"
    check_split(eng, "nasty", [b"~" * 17 + b"c"])
    check_split(eng, "nasty", [b"~" * 17])              # nothing left


# ---- refusals ----

def test_raise_fails_the_call_and_leaves_the_earlier_result(tk, eng):
    strings, _ = use(eng, "tekken")
    good = [b"x<s>y", b"[INST]z"]
    exp, res, _ = check_split(eng, "tekken", good, BOS | PART_SRC)
    modes = [PARSE] * N_SPECIAL
    modes[4] = RAISE
    docs = [b"ok [INST]", b"", b"fine [/INS", b"bad 0123[/INST] and [/INST]", b"[/INST]"]
    data, offs, d, ptr, o = upload(docs)
    with pytest.raises(SpecialRaise) as want:
        expected_specials(data, offs, strings, modes, 0)
    assert (want.value.doc, want.value.pos, want.value.id) == (3, 8, 4)
    with pytest.raises(tk.TokenizerError) as e:
        eng.split_specials_device(ptr, o.data_ptr(), len(docs), len(data), modes, 0, 0, stream())
    assert e.value.code == tk.TK_ERR_SPECIAL_POLICY and e.value.bad_doc == 3
    assert "document 3" in str(e.value) and "byte 8" in str(e.value) and "id 4" in str(e.value)
    assert_same(fetch(res), exp, "the earlier result")
    with pytest.raises(tk.TokenizerError) as e:
        eng.encode_batch_parsed(data, offs, True, True, modes)
    assert e.value.code == tk.TK_ERR_SPECIAL_POLICY and e.value.bad_doc == 3
    modes[4] = TEXT                                     # the same text, the string left alone
    check_split(eng, "tekken", docs, 0, modes)


def test_every_invalid_argument(tk, eng, test_vocab):
    def refused(e, *a, **kw):
        with pytest.raises(tk.TokenizerError) as err:
            e.split_specials_device(*a, **kw)
        assert err.value.code == tk.TK_ERR_INVALID_ARG, str(err.value)
    exp, res, _ = check_split(eng, "tekken", [b"a<s>b"], BOS)
    data, offs, d, ptr, o = upload([b"a<s>b"])
    args = (ptr, o.data_ptr(), 1, len(data))
    fresh = tk.Engine(test_vocab["tokens"], test_vocab["num_special"], test_vocab["bos"], test_vocab["eos"], device=0)
    refused(fresh, *args)                               # no strings on the context
    fresh.close()
    refused(eng, *args, modes=[PARSE] * (N_SPECIAL - 1))
    refused(eng, *args, modes=[PARSE] * (N_SPECIAL - 1) + [3])
    refused(eng, *args, flags=8)
    refused(eng, *args, checks=4)
    refused(eng, ptr, 0, 1, len(data))
    strings, modes = use(eng, "nasty")
    refused(eng, *args)                                 # modes NULL: the empty strings are in the match set
    refused(eng, *args, modes=modes[:-1] + [PARSE])
    eng.set_special_tokens(strings[:-1] + [b"y" * 256])
    eng.current = None
    refused(eng, *args, modes=modes[:-1] + [RAISE])
    eng.split_specials_device(*args, modes=modes)       # ... and left alone where it is TEXT
    with pytest.raises(tk.TokenizerError) as err:       # checks: offsets that do not end at n_bytes, text that is not UTF-8
        eng.split_specials_device(ptr, o.data_ptr(), 1, len(data) - 1, modes, 0, tk.CHECK_OFFSETS)
    assert err.value.code == tk.TK_ERR_INVALID_ARG
    bad = upload([b"a\xffb"])
    with pytest.raises(tk.TokenizerError) as err:
        eng.split_specials_device(bad[3], bad[4].data_ptr(), 1, 3, modes, 0, tk.CHECK_UTF8)
    assert err.value.code == tk.TK_ERR_INVALID_UTF8
    with pytest.raises(tk.TokenizerError) as err:       # the composite entry refuses the join's options before it splits
        eng.encode_batch_device_parsed(*args, modes=modes, join_flags=64)
    assert err.value.code == tk.TK_ERR_INVALID_ARG


# ---- the encoding it defines ----

def test_without_a_match_the_joined_ids_are_encodes(tk, eng):
    docs = sweep_docs()
    scrubbed = [d.replace(b"[", b"(").replace(b"<", b"(") for d in docs]
    for name, batch, modes in (("tekken", docs, [TEXT] * N_SPECIAL), ("tekken", scrubbed, None)):
        use(eng, name)
        data, offs, d, ptr, o = upload(batch)
        for bos, eos in ((True, True), (False, False), (True, False), (False, True)):
            p_ids, p_oo, n = eng.encode_batch_device(ptr, o.data_ptr(), len(batch), len(data), bos, eos, stream())
            ids = to_host(tk.DeviceView(p_ids, n, "<i4"), n, np.uint32).copy()
            oo = to_host(tk.DeviceView(p_oo, len(batch) + 1, "<i8"), len(batch) + 1, np.uint64).copy()
            parts, j = eng.encode_batch_device_parsed(ptr, o.data_ptr(), len(batch), len(data), bos, eos, modes, stream=stream())
            assert parts.n_matches == 0 and parts.bytes_ptr == ptr
            v = j.views()
            helpers.assert_array_same(to_host(v[0], j.n_ids, np.uint32), ids, (bos, eos, "ids"))
            helpers.assert_array_same(to_host(v[1], j.n_convs + 1, np.uint64), oo, (bos, eos, "offsets"))


def test_round_trip_returns_the_ids(tk, eng, orc):
    """ids with one control id between any two encoded segments: decode(KEEP), then the parsed encode, gives them back."""
    use(eng, "tekken")
    rng = np.random.default_rng(29)
    texts = [d.replace(b"[", b"(").replace(b"<", b"(") for d in sweep_docs() if 0 < len(d) < 400][:120]
    ids, oo = [], [0]
    for d in range(80):
        for k in range(int(rng.integers(0, 6))):
            ids += [int(rng.integers(1, 60)) for _ in range(int(rng.integers(1, 3)))]
            if rng.integers(0, 4):
                ids += orc.encode(texts[int(rng.integers(0, len(texts)))], False, False)
        oo.append(len(ids))
    ids, oo = np.array(ids, np.uint32), np.array(oo, np.uint64)
    d_ids, d_oo = helpers.on_device(ids, oo)
    vb, vo = eng.decode_batch_device(d_ids.data_ptr(), d_oo.data_ptr(), 80, len(ids), tk.SpecialTokenPolicy.Keep, stream())
    nb = vb.__cuda_array_interface__["shape"][0]
    _, j = eng.encode_batch_device_parsed(vb.__cuda_array_interface__["data"][0], vo.__cuda_array_interface__["data"][0], 80, nb,
                                          False, False, None, checks=3, stream=stream())
    v = j.views()
    helpers.assert_array_same(to_host(v[0], j.n_ids, np.uint32), ids, "ids")
    helpers.assert_array_same(to_host(v[1], 81, np.uint64), oo, "offsets")


# ---- one seeded random sweep ----

@pytest.mark.parametrize("name", ["tekken", "nasty"])
def test_random_sweep(eng, orc, T, name):
    strings, modes = use(eng, name)
    rng = np.random.default_rng(101 if name == "tekken" else 103)
    usable = [i for i, s in enumerate(strings) if s and (modes is None or modes[i] != TEXT or i == 10)]
    plant = [strings[i] for i in usable[:40]] + [strings[i] for i in usable[-3:]]
    alphabet = np.frombuffer(b"abc<[q#~ xyz\n" if name == "nasty" else b"abc <[/S>] xyz\n_1I", np.uint8)
    docs = []
    for d in range(2000):
        n = int(rng.integers(0, 3 * T + 1)) if d % 12 == 0 else int(rng.integers(0, 160))
        doc = bytearray(rng.choice(alphabet, n).tobytes())
        for _ in range(int(rng.integers(0, 2 + n // 60))):
            s = plant[int(rng.integers(0, len(plant)))]
            at = int(rng.integers(0, n + 1))
            doc[at:at] = s if rng.integers(0, 5) else s[:int(rng.integers(1, len(s) + 1))]
        docs.append(bytes(doc[:3 * T]))
    m = [PARSE if modes is None or modes[i] != TEXT else TEXT for i in range(N_SPECIAL)]
    for i in usable[::3]:
        m[i] = TEXT                                     # mixed modes, without RAISE
    exp, _, _ = check_split(eng, name, docs, BOS | EOS | PART_SRC, m)
    assert exp["n_matches"] > 2000
    if name == "tekken":                                # ... and the encoding it defines, against the oracle
        data, offs, d, ptr, o = upload(docs)
        ids, oo = expected_parsed(orc, data, offs, strings, m, True, False)
        _, j = eng.encode_batch_device_parsed(ptr, o.data_ptr(), len(docs), len(data), True, False, m, stream=stream())
        v = j.views()
        helpers.assert_array_same(to_host(v[0], j.n_ids, np.uint32), ids, "ids")
        helpers.assert_array_same(to_host(v[1], j.n_convs + 1, np.uint64), oo, "offsets")


# ---- the Tekkenizer methods on known answers ----

def test_tokenizer_methods(tk, small_vocab):
    from test_host_tokenizer import model
    specials = ("<unk>", "<s>", "</s>", "<pad>", "[INST]", "[/INST]", "[SYSTEM_PROMPT]", "[/SYSTEM_PROMPT]")
    t = tk.Tekkenizer.from_json(json.dumps(model(small_vocab["tokens"], specials=specials)), device=0)
    try:
        text = "<s>[INST] hi [/INST]"
        hi = [10 + b for b in b" hi "]                  # (no merge of the small vocabulary applies: one token a byte)
        assert t.encode(" hi ") == hi
        assert t.encode_with_specials(text) == [1, 4] + hi + [5]
        assert t.encode_with_specials(text, True, True) == [1, 1, 4] + hi + [5, 2]
        assert t.encode_with_specials(text, allowed=()) == t.encode(text)
        assert t.encode_with_specials(text, allowed=("[INST]",)) == t.encode("<s>") + [4] + t.encode(" hi [/INST]")
        assert t.encode_with_specials("hello world", True) == t.encode("hello world", True)
        with pytest.raises(tk.TokenizerError) as e:
            t.encode_with_specials(text, allowed=(), disallowed="all")
        assert e.value.code == tk.TK_ERR_SPECIAL_POLICY
        with pytest.raises(tk.TokenizerError) as e:
            t.encode_with_specials(text, disallowed=("[/INST]",))
        assert e.value.code == tk.TK_ERR_SPECIAL_POLICY
        assert t.encode_with_specials("<s> hi", disallowed=("[/INST]",)) == [1] + hi[:3]
        with pytest.raises(tk.TokenizerError) as e:
            t.encode_with_specials(text, allowed=("[NOPE]",))
        assert e.value.code == tk.TK_ERR_TOKEN_NOT_FOUND
        with pytest.raises(ValueError):
            t.encode_with_specials(text, allowed=("[INST]",), disallowed=("[INST]",))
        with pytest.raises(ValueError):
            t.encode_with_specials(text, allowed="all", disallowed="all")
        r = t.encode_batch_with_specials([text, "", "hello</s>"], add_eos=True)
        assert r["ids"].tolist() == [1, 4] + hi + [5, 2, 2] + t.encode("hello") + [2, 2]
        assert r["id_offsets"].tolist() == [0, 8, 9, 12] and r["n_matches"] == 4
        assert t.encode(text) == t.encode_batch([text])[0]          # encode itself is what it was: the markers stay text
        assert 4 not in t.encode(text)
    finally:
        t.close()
