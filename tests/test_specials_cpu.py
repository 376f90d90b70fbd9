"""Special-token strings parsed out of text (include/tekken_hip.h tk_specials_split_device): the definition restated with a plain
per-byte loop, hand-made cases of every rule, a model of the chain that chooses among overlapping candidates against that loop, the
header's values, the exported symbols and the shim's declarations, and the binding's description of the struct."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_layout_binding_cpu import header_members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT, PARSE, RAISE = 0, 1, 2
BOS, EOS, PART_SRC = 1, 2, 4
NONE = 0xFFFFFFFF
MAXLEN = 255
VALUES = {"TK_SPECIAL_TEXT": TEXT, "TK_SPECIAL_PARSE": PARSE, "TK_SPECIAL_RAISE": RAISE, "TK_SPECIALS_BOS": BOS, "TK_SPECIALS_EOS": EOS,
          "TK_SPECIALS_PART_SRC": PART_SRC}
NEW_SYMBOLS = ["tk_specials_split_device", "tk_encode_batch_device_parsed", "tk_encode_batch_parsed", "tk_free_specials",
               "tk_last_specials_ms", "tk_specials_tile", "tk_tokenizer_encode_parsed"]


class SpecialRaise(Exception):
    """Step 3: the first RAISE match."""

    def __init__(self, doc, pos, sid):
        super().__init__("document %d, byte %d: id %d" % (doc, pos, sid))
        self.doc, self.pos, self.id = doc, pos, sid


def match_set(strings, modes):
    """Step 1: {string: the lowest id of A with these bytes}; ValueError for what the call refuses."""
    if modes is None:
        modes = [PARSE] * len(strings)
    if len(modes) != len(strings):
        raise ValueError("n_modes")
    if any(m not in (TEXT, PARSE, RAISE) for m in modes):
        raise ValueError("unknown mode")
    A = {}
    for i, (s, m) in enumerate(zip(strings, modes)):
        if m == TEXT:
            continue
        if not 1 <= len(s) <= MAXLEN:
            raise ValueError("string %d has %d bytes" % (i, len(s)))
        A.setdefault(bytes(s), i)
    return A, list(modes)


def doc_matches(doc, A):
    """Step 2 for one document: [(p, len, id)], leftmost-longest, non-overlapping."""
    out, p = [], 0
    lens = sorted({len(s) for s in A}, reverse=True)
    first = {s[0] for s in A}
    while p < len(doc):
        if doc[p] not in first:                         # (no string of A begins here: the loop below would find none)
            p += 1
            continue
        for l in lens:                                  # the longest first
            if p + l <= len(doc) and doc[p:p + l] in A:
                out.append((p, l, A[doc[p:p + l]]))
                p += l
                break
        else:
            p += 1
    return out


def expected_specials(data, offs, strings, modes, flags, bos=1, eos=2):
    """Steps 1-4: the result of tk_specials_split_device as a dict of numpy arrays and counts."""
    A, modes = match_set(strings, modes)
    raw = bytes(bytearray(data))
    offs = [int(x) for x in offs]
    D = len(offs) - 1
    text, poffs, ctrl, conv, src = bytearray(), [0], [], [0], []
    n_matches = n_removed = 0
    for d in range(D):
        doc = raw[offs[d]:offs[d + 1]]
        ms = doc_matches(doc, A) if A else []
        for p, l, i in ms:
            if modes[i] == RAISE:
                raise SpecialRaise(d, p, i)
        cuts = [(bos if flags & BOS else NONE, 0)] + [(i, p + l) for p, l, i in ms]
        ends = [p for p, _, _ in ms] + [len(doc)]
        for (cid, start), end in zip(cuts, ends):
            ctrl.append(cid)
            src.append(offs[d] + start)
            text += doc[start:end]
            poffs.append(len(text))
        if flags & EOS:
            ctrl.append(eos)
            src.append(offs[d + 1])
            poffs.append(len(text))
        conv.append(len(ctrl))
        n_matches += len(ms)
        n_removed += sum(l for _, l, _ in ms)
    return {"bytes": np.frombuffer(bytes(text), np.uint8).copy() if text else np.zeros(0, np.uint8),
            "part_offsets": np.array(poffs, np.uint64), "part_ctrl": np.array(ctrl, np.uint32), "conv_offsets": np.array(conv, np.uint64),
            "part_src": np.array(src, np.uint64) if flags & PART_SRC else None,
            "n_docs": D, "n_parts": len(ctrl), "n_bytes": len(text), "n_matches": n_matches, "n_removed": n_removed}


def expected_parsed(orc, data, offs, strings, modes, add_bos, add_eos, bos=1, eos=2):
    """Step 5: (ids, offsets) of the join of every document's parts, each text encoded alone by the oracle."""
    e = expected_specials(data, offs, strings, modes, (BOS if add_bos else 0) | (EOS if add_eos else 0), bos, eos)
    po, text = e["part_offsets"], e["bytes"].tobytes()
    ids, oo = [], [0]
    for d in range(e["n_docs"]):
        for p in range(int(e["conv_offsets"][d]), int(e["conv_offsets"][d + 1])):
            if e["part_ctrl"][p] != NONE:
                ids.append(int(e["part_ctrl"][p]))
            seg = text[int(po[p]):int(po[p + 1])]
            if seg:
                ids += orc.encode(seg, False, False)
        oo.append(len(ids))
    return np.array(ids, np.uint32), np.array(oo, np.uint64)


def split(docs, strings, modes=None, flags=0):
    data = b"".join(docs)
    offs = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
    return expected_specials(np.frombuffer(data, np.uint8), offs, strings, modes, flags)


def triples(docs, strings, modes=None):
    A, _ = match_set(strings, modes)
    return [doc_matches(d, A) for d in docs]


# ---- hand-made cases of every rule ----

def test_longest_wins_over_a_prefix():
    s = [b"<a", b"<ab>", b"<a>"]
    assert triples([b"x<ab>y<a>z<a"], s) == [[(1, 4, 1), (6, 3, 2), (10, 2, 0)]]
    assert triples([b"<ab"], s) == [[(0, 2, 0)]]        # the longer one does not fit: the prefix matches


def test_leftmost_wins_over_a_longer_later_one():
    assert triples([b"abcd"], [b"ab", b"bcd"]) == [[(0, 2, 0)]]
    assert triples([b"xbcd"], [b"ab", b"bcd"]) == [[(1, 3, 1)]]


def test_matches_do_not_overlap():
    assert triples([b"aaaaa"], [b"aa"]) == [[(0, 2, 0), (2, 2, 0)]]


def test_equal_strings_the_lower_id_stands_for_both():
    assert triples([b"[X]"], [b"q", b"[X]", b"[X]"]) == [[(0, 3, 1)]]
    assert triples([b"[X]"], [b"q", b"[X]", b"[X]"], [PARSE, TEXT, PARSE]) == [[(0, 3, 2)]]   # ... of the match set


def test_a_text_string_that_is_a_prefix_of_a_parsed_one():
    s, m = [b"<s", b"<s>"], [TEXT, PARSE]
    assert triples([b"<s<s>"], s, m) == [[(2, 3, 1)]]
    assert triples([b"<s<s>"], s, [TEXT, TEXT]) == [[]]


def test_raise_is_reported_at_the_first_document_and_position():
    s, m = [b"[A]", b"[B]"], [PARSE, RAISE]
    with pytest.raises(SpecialRaise) as e:
        split([b"[A]", b"x[A]yy[B][B]", b"[B]"], s, m)
    assert (e.value.doc, e.value.pos, e.value.id) == (1, 6, 1)
    assert split([b"[A]", b"[B"], s, m)["n_matches"] == 1


def test_a_match_cut_by_a_document_end_does_not_match():
    r = split([b"ab[IN", b"ST]cd"], [b"[INST]"])
    assert r["n_matches"] == 0 and r["bytes"].tobytes() == b"ab[INST]cd" and r["part_offsets"].tolist() == [0, 5, 10]


def test_parts_of_a_hand_made_batch():
    s = [b"<unk>", b"<s>", b"</s>", b"[INST]", b"[/INST]"]
    r = split([b"<s>[INST] hi [/INST]ok</s>", b"", b"[INST]", b"no"], s, None, BOS | EOS | PART_SRC)
    assert r["bytes"].tobytes() == b" hi okno"
    assert r["conv_offsets"].tolist() == [0, 6, 8, 11, 13]
    assert r["part_ctrl"].tolist() == [1, 1, 3, 4, 2, 2, 1, 2, 1, 3, 2, 1, 2]
    assert r["part_offsets"].tolist() == [0, 0, 0, 4, 6, 6, 6, 6, 6, 6, 6, 6, 8, 8]
    assert r["part_src"].tolist() == [0, 3, 9, 20, 26, 26, 26, 26, 26, 32, 32, 32, 34]
    assert (r["n_matches"], r["n_removed"], r["n_bytes"], r["n_parts"]) == (5, 26, 8, 13)
    r = split([b"<s>x", b""], s, [TEXT] * 5, 0)         # every mode TEXT: one part a document, the text as it is
    assert r["part_ctrl"].tolist() == [NONE, NONE] and r["part_offsets"].tolist() == [0, 4, 4] and r["part_src"] is None
    r = split([], s, None, BOS)
    assert r["conv_offsets"].tolist() == [0] and r["part_offsets"].tolist() == [0] and r["n_parts"] == 0


def test_every_invalid_argument_of_step_1():
    with pytest.raises(ValueError):
        split([b"x"], [b"a", b""])                      # an empty string in the match set
    with pytest.raises(ValueError):
        split([b"x"], [b"a", b"b" * 256])
    assert split([b"x"], [b"a", b"", b"b" * 256], [PARSE, TEXT, TEXT])["n_matches"] == 0
    assert split([b"b" * 255], [b"b" * 255])["n_matches"] == 1
    with pytest.raises(ValueError):
        split([b"x"], [b"a"], [PARSE, PARSE])
    with pytest.raises(ValueError):
        split([b"x"], [b"a"], [3])


# ---- the chain: next() and reachability by pointer doubling, as the device runs it ----

def chain_matches(pos, length):
    """The candidates (sorted by position, each inside its document) that the walk of step 2 emits: those reachable from
    candidate 0 under nxt(c) = the first candidate at or behind pos[c] + length[c].  A jump is (target, steps); `row` is the
    number of the match a candidate is."""
    n = len(pos)
    if n == 0:
        return []
    jump = [(int(np.searchsorted(pos, pos[c] + length[c], "left")), 1) for c in range(n)] + [(n, 0)]
    assert all(c < t <= n for c, (t, _) in enumerate(jump[:-1]))
    row = [0] + [None] * n
    rounds = 0
    while (1 << rounds) <= n:
        rounds += 1
    for _ in range(rounds):
        new = list(row)
        for v in range(n + 1):
            t, steps = jump[v]
            if row[v] is not None and steps:
                assert new[t] in (None, row[v] + steps)
                new[t] = row[v] + steps
        jump = [(jump[t][0], s + jump[t][1]) for t, s in jump]
        row = new
    marked = [c for c in range(n) if row[c] is not None]
    assert [row[c] for c in marked] == list(range(len(marked))) and row[n] == len(marked)
    return marked


def test_chain_model_against_the_plain_loop():
    rng = np.random.default_rng(5)
    for trial in range(300):
        n_docs = int(rng.integers(1, 5))
        lens = rng.integers(0, 40, n_docs)
        offs = np.concatenate([[0], np.cumsum(lens)])
        dense = trial % 3 == 0                           # every position a candidate: long chains
        cand = {}
        for d in range(n_docs):
            for p in range(int(offs[d]), int(offs[d + 1])):
                if dense or rng.integers(0, 3) == 0:
                    cand[p] = int(rng.integers(1, min(6, int(offs[d + 1]) - p) + 1))   # wholly inside its document
        pos = np.array(sorted(cand), np.int64)
        length = np.array([cand[p] for p in pos], np.int64)
        exp = []
        for d in range(n_docs):                         # the plain walk, one document at a time
            p = int(offs[d])
            while p < offs[d + 1]:
                if p in cand:
                    exp.append(p)
                    p += cand[p]
                else:
                    p += 1
        assert [int(pos[c]) for c in chain_matches(pos, length)] == exp, trial


def test_chain_on_the_run_that_makes_one_chain_of_every_second_candidate():
    n = 1001
    pos, length = np.arange(n - 1), np.full(n - 1, 2)   # "aa" in "a" * n
    assert chain_matches(pos, length) == list(range(0, n - 1, 2))
    assert [m[0] for m in triples([b"a" * n], [b"aa"])[0]] == list(range(0, n - 1, 2))


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
    assert re.search(r"typedef struct tk_specials_opts\b", hdr) and re.search(r"typedef struct tk_specials\b", hdr)
    assert re.search(r"\bstruct TkSpecialsOpts\b", ffi) and re.search(r"\bstruct TkSpecials\b", ffi)
    assert "tk_specials_split_device" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_python_constants_and_exported_symbols(tk):
    assert (tk.SPECIAL_TEXT, tk.SPECIAL_PARSE, tk.SPECIAL_RAISE) == (TEXT, PARSE, RAISE)
    assert (tk.SPECIALS_BOS, tk.SPECIALS_EOS, tk.SPECIALS_PART_SRC) == (BOS, EOS, PART_SRC)
    for name in NEW_SYMBOLS:
        assert hasattr(tk.lib(), name), name
    for name in ("split_specials_device", "encode_batch_device_parsed", "encode_batch_parsed", "last_specials_ms"):
        assert hasattr(tk.Engine, name), name
    for name in ("encode_with_specials", "encode_batch_with_specials"):
        assert hasattr(tk.Tekkenizer, name), name
    assert ctypes.sizeof(tk._SpecialsOpts) == 16          # a pointer and two uint32
    assert tk.lib().tk_specials_tile() % 16 == 0          # (no GPU needed: a constant of the build)


def test_result_class_declares_the_header_struct(tk):
    """tests/test_layout_binding_cpu.py's first check, for "specials"."""
    R, members = tk.SpecialsResult, header_members("specials")
    assert R.PASS == "specials"
    assert [o[0] for o in R.OUTPUTS] == [m for m, ptr in members if ptr]
    assert list(R.COUNTS) == [m for m, ptr in members if not ptr]
    assert [ptr for _, ptr in members] == sorted((ptr for _, ptr in members), reverse=True)
    assert ctypes.sizeof(R.STRUCT) == sum(ctypes.sizeof(ctypes.c_void_p) if ptr else 8 for _, ptr in members)
    assert [f[0] for f in R.STRUCT._fields_] == [m for m, _ in members]
    for (_, ptr), (_, ctype) in zip(members, R.STRUCT._fields_):
        assert ctype is (ctypes.c_void_p if ptr else ctypes.c_uint64)


def test_result_attributes_and_views_follow_the_declaration(tk):
    """... and its second: every output has a fixed type, as a join's (no I64 flag, no typestr)."""
    R = tk.SpecialsResult
    st = R.STRUCT()
    for i, (field, _) in enumerate(R.STRUCT._fields_):
        setattr(st, field, 0x1000 * (i + 1) if field in [o[0] for o in R.OUTPUTS] else i + 2)
    first_optional = next(o[0] for o in R.OUTPUTS if o[4])
    setattr(st, first_optional, None)
    r = R(st)
    assert R.I64 is None and not hasattr(r, "typestr") and hasattr(r, "n_docs")
    views = r.views()
    assert len(views) == len(R.OUTPUTS)
    for (out, typestr, shape, _, optional), v in zip(R.OUTPUTS, views):
        if out == first_optional:
            assert getattr(r, out + "_ptr") is None and v is None
            continue
        assert getattr(r, out + "_ptr") == getattr(st, out)
        cai = v.__cuda_array_interface__
        assert cai["data"][0] == getattr(st, out) and cai["shape"] == tuple(shape(r)) and cai["typestr"] == typestr
    for k in R.COUNTS:
        assert getattr(r, k) == getattr(st, k)
    assert set(r._counts()) == set(R.DICT_COUNTS) <= set(R.COUNTS)
