"""Chat batches (include/tekken_hip.h tk_join_from_ids_device), the parts that need no GPU: the plain-loop restatement of the
definition that tests/test_gpu_join.py checks the kernels against, the hand-made cases of the definition, the wave search on
arrays with ties, the Rust shim's declarations, and the host-only tokenizer."""
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["tk_join_from_ids_device", "tk_encode_parts_device_join", "tk_encode_parts_join", "tk_free_join"]
NONE = 0xFFFFFFFF
LABEL_CTRL, LABEL_TEXT = 1, 2
LABELS, PART_INDEX = 1, 2
ALL = LABELS | PART_INDEX
CHECK_PARTS = 16
DEFINES = {"TK_CHECK_PARTS": "16", "TK_JOIN_NONE": "0xFFFFFFFFu", "TK_PART_LABEL_CTRL": "1", "TK_PART_LABEL_TEXT": "2",
           "TK_JOIN_LABELS": "1", "TK_JOIN_PART_INDEX": "2"}
IGN = -100


def expected_joined(ids, id_offs, part_ctrl, part_flags, conv_offs, ignore_index=IGN, flags=ALL, num_special=None):
    """The definition, restated part by part with plain loops (no cumulative sum, no search).  -> dict(ids uint32 [N], offsets
    uint64 [C + 1], labels int32 [N] or None, part_index uint32 [N] or None, n_ids, n_ctrl, n_labelled).  part_flags None: all
    zero.  What the entries refuse with TK_ERR_INVALID_ARG raises ValueError; num_special: also check the control ids (the
    entries: TK_CHECK_PARTS, the host entry always)."""
    src = [int(x) for x in ids]
    oo = [int(x) for x in id_offs]
    ctrl = [int(x) for x in part_ctrl]
    conv = [int(x) for x in conv_offs]
    P, C = len(oo) - 1, len(conv) - 1
    pf = [0] * P if part_flags is None else [int(x) for x in part_flags]
    if flags & ~ALL:
        raise ValueError("unknown flag")
    if C < 0 or len(ctrl) != P or len(pf) != P:
        raise ValueError("array lengths")
    if conv[0] != 0:
        raise ValueError("conv_offsets[0] != 0: conversation 0")
    for c in range(C):
        if conv[c + 1] < conv[c]:
            raise ValueError("conv_offsets decrease: conversation %d" % c)
    if conv[C] != P:
        raise ValueError("conv_offsets end at %d, not at %d: conversation %d" % (conv[C], P, C))
    if num_special is not None:
        for p in range(P):
            if ctrl[p] != NONE and ctrl[p] >= num_special:
                raise ValueError("part %d: control id %d" % (p, ctrl[p]))
    out, lab, pidx, offsets = [], [], [], [0]
    n_ctrl = n_labelled = 0
    for c in range(C):
        for p in range(conv[c], conv[c + 1]):
            if ctrl[p] != NONE:
                out.append(ctrl[p])
                lab.append(ctrl[p] if pf[p] & LABEL_CTRL else ignore_index)
                pidx.append(p - conv[c])
                n_ctrl += 1
                n_labelled += 1 if pf[p] & LABEL_CTRL else 0
            for i in range(oo[p], oo[p + 1]):
                out.append(src[i])
                lab.append(src[i] if pf[p] & LABEL_TEXT else ignore_index)
                pidx.append(p - conv[c])
                n_labelled += 1 if pf[p] & LABEL_TEXT else 0
        offsets.append(len(out))
    return {"ids": np.array(out, np.uint32), "offsets": np.array(offsets, np.uint64),
            "labels": np.array(lab, np.int64).astype(np.int32) if flags & LABELS else None,
            "part_index": np.array(pidx, np.uint32) if flags & PART_INDEX else None,
            "n_ids": len(out), "n_ctrl": n_ctrl, "n_labelled": n_labelled}


def parts_table(convs):
    """convs: lists of (ctrl or None, [ids], flags) -> (ids, id_offs, part_ctrl, part_flags, conv_offs)."""
    ids, oo, ctrl, pf, conv = [], [0], [], [], [0]
    for parts in convs:
        for c, text, fl in parts:
            ids += text
            oo.append(len(ids))
            ctrl.append(NONE if c is None else c)
            pf.append(fl)
        conv.append(len(ctrl))
    return (np.array(ids, np.uint32), np.array(oo, np.uint64), np.array(ctrl, np.uint32), np.array(pf, np.uint32), np.array(conv, np.uint64))


# 6 conversations: an empty one first and last; a part with neither a control id nor text; a part with only a control id; each label
# bit alone (and both, and none)
TABLE = [[],
         [(1, [], 0), (3, [50, 51, 52], 0), (4, [], 0), (None, [60, 61], LABEL_TEXT), (2, [], LABEL_CTRL)],
         [(None, [], LABEL_CTRL | LABEL_TEXT), (None, [70], 0)],
         [(5, [80, 81], LABEL_CTRL), (6, [82], LABEL_TEXT), (7, [83, 84], LABEL_CTRL | LABEL_TEXT)],
         [(None, [], 0)],
         []]


def test_hand_made_table():
    e = expected_joined(*parts_table(TABLE))
    assert e["ids"].tolist() == [1, 3, 50, 51, 52, 4, 60, 61, 2, 70, 5, 80, 81, 6, 82, 7, 83, 84]
    assert e["offsets"].tolist() == [0, 0, 9, 10, 18, 18, 18]
    I = IGN
    assert e["labels"].tolist() == [I, I, I, I, I, I, 60, 61, 2, I, 5, I, I, I, 82, 7, 83, 84]
    assert e["part_index"].tolist() == [0, 1, 1, 1, 1, 2, 3, 3, 4, 1, 0, 0, 0, 1, 1, 2, 2, 2]
    assert (e["n_ids"], e["n_ctrl"], e["n_labelled"]) == (18, 7, 8)
    assert e["ids"].dtype == np.uint32 and e["offsets"].dtype == np.uint64 and e["labels"].dtype == np.int32 and e["part_index"].dtype == np.uint32
    # another ignore value; NULL part_flags; each output deselected; n_labelled is filled all the same
    assert expected_joined(*parts_table(TABLE), ignore_index=-1)["labels"].tolist()[:7] == [-1] * 6 + [60]
    ids, oo, ctrl, pf, conv = parts_table(TABLE)
    e0 = expected_joined(ids, oo, ctrl, None, conv)
    assert e0["labels"].tolist() == [I] * 18 and e0["n_labelled"] == 0 and e0["ids"].tolist() == e["ids"].tolist()
    e1 = expected_joined(ids, oo, ctrl, pf, conv, flags=0)
    assert e1["labels"] is None and e1["part_index"] is None and e1["n_labelled"] == 8
    assert expected_joined(ids, oo, ctrl, pf, conv, flags=LABELS)["part_index"] is None
    assert expected_joined(ids, oo, ctrl, pf, conv, flags=PART_INDEX)["labels"] is None


def test_hand_made_empty_shapes():
    z = np.zeros(0, np.uint32)
    e = expected_joined(z, [0], z, z, [0])                       # C == 0
    assert e["ids"].tolist() == [] and e["offsets"].tolist() == [0] and (e["n_ids"], e["n_ctrl"], e["n_labelled"]) == (0, 0, 0)
    e = expected_joined(z, [0], z, None, [0, 0, 0])              # P == 0, conversations without parts
    assert e["offsets"].tolist() == [0, 0, 0] and e["labels"].tolist() == []
    e = expected_joined(z, [0, 0, 0], [NONE, NONE], [3, 3], [0, 1, 2])   # parts with neither
    assert e["offsets"].tolist() == [0, 0, 0] and e["n_ids"] == 0
    e = expected_joined(z, [0, 0, 0], [4, NONE], [1, 0], [0, 2])         # a control id alone
    assert e["ids"].tolist() == [4] and e["labels"].tolist() == [4] and e["part_index"].tolist() == [0] and e["n_labelled"] == 1


def test_every_refused_case_raises():
    ids, oo, ctrl, pf, conv = parts_table(TABLE)
    expected_joined(ids, oo, ctrl, pf, conv, num_special=8)
    for flags in (4, ALL | 8, 1 << 31):
        with pytest.raises(ValueError):
            expected_joined(ids, oo, ctrl, pf, conv, flags=flags)
    P = len(ctrl)
    for bad in ([1] + conv.tolist()[1:], [0, 0, 5, 4, 10, 11, 11], conv.tolist()[:-1] + [P - 1], conv.tolist()[:-1] + [P + 1]):
        with pytest.raises(ValueError):
            expected_joined(ids, oo, ctrl, pf, bad)
    with pytest.raises(ValueError):                      # C == 0 with parts
        expected_joined(ids, oo, ctrl, pf, [0])
    with pytest.raises(ValueError) as e:                 # a control id of num_special
        expected_joined(ids, oo, ctrl, pf, conv, num_special=7)
    assert "part 9" in str(e.value)                      # (the part that carries 7)
    c2 = ctrl.copy()
    c2[3] = NONE - 1
    with pytest.raises(ValueError):
        expected_joined(ids, oo, c2, pf, conv, num_special=8)


def random_parts(rng, C, longest):
    convs = []
    for _ in range(C):
        parts = []
        for _ in range(int(rng.integers(0, 8))):
            n = int(rng.integers(0, longest)) if rng.integers(0, 4) else 0
            parts.append((int(rng.integers(0, 10)) if rng.integers(0, 3) else None, rng.integers(10, 1000, n).tolist(), int(rng.integers(0, 4))))
        convs.append(parts)
    return convs


def test_invariants_on_random_input():
    rng = np.random.default_rng(31)
    for case in range(40):
        ids, oo, ctrl, pf, conv = parts_table(random_parts(rng, int(rng.integers(1, 12)), int(rng.integers(1, 30))))
        e = expected_joined(ids, oo, ctrl, pf, conv, num_special=10)
        N = e["n_ids"]
        assert N == len(ids) + e["n_ctrl"] == int(e["offsets"][-1]) and e["n_ctrl"] == int(np.sum(ctrl != NONE))
        # the control positions, from the definition's own counts: in front of every part that has one
        is_ctrl = np.zeros(N, bool)
        at = 0
        for p in range(len(ctrl)):
            if ctrl[p] != NONE:
                is_ctrl[at] = True
                at += 1
            at += int(oo[p + 1] - oo[p])
        assert at == N
        assert np.array_equal(e["ids"][~is_ctrl], ids) and np.array_equal(e["ids"][is_ctrl], ctrl[ctrl != NONE])
        lab = e["labels"]
        assert np.all((lab == IGN) | (lab == e["ids"].astype(np.int64)))
        assert e["n_labelled"] == int(np.sum(lab != IGN))
        for c in range(len(conv) - 1):
            a, b = int(e["offsets"][c]), int(e["offsets"][c + 1])
            pi = e["part_index"][a:b].astype(np.int64)
            assert np.all(np.diff(pi) >= 0) and (b == a or pi[-1] < int(conv[c + 1] - conv[c]))


def test_wave_search_handles_ties():
    """The join kernel searches the parts' output starts, which repeat where a part has neither a control id nor text: the 64-ary
    search (tools/seqpack_model.py restates tky_wave_count_le) returns the count of entries <= key -- one past the LAST such
    entry -- on arrays with runs of equal entries, the ballot stays a prefix of the lanes, and it ends."""
    import bisect
    import seqpack_model
    rng = np.random.default_rng(32)
    for n in (1, 2, 63, 64, 65, 127, 4095, 4096, 4097, 100_000):
        for distinct in (1, 3, max(n // 50, 1), n):
            a = sorted(rng.integers(0, distinct, n).tolist())
            a[0] = 0
            keys = rng.integers(0, distinct + 1, 40).tolist() + [0, a[-1], a[-1] + 1, a[n // 2]]
            for key in keys:
                assert seqpack_model.wave_count_le(a, n, key) == bisect.bisect_right(a, key), (n, distinct, key)
    a = [0] * 5000 + [7] * 300 + [8] + [9] * 70_000        # runs far longer than 64 and 64^2
    for key in (0, 6, 7, 8, 9, 10):
        assert seqpack_model.wave_count_le(a, len(a), key) == bisect.bisect_right(a, key)


def test_kernel_model_against_the_definition():
    """tools/join_model.py restates the join kernels index by index (and asserts that every read and write stays inside its
    array and every element is written once): against the definition on the hand-made table and on random parts with long runs
    of empty and one-element parts, at tile sizes small enough that both forms of a tile's search, tiles without a start and
    every N % 4 occur."""
    import join_model
    rng = np.random.default_rng(33)
    forms, tails = set(), set()
    inputs = [parts_table(TABLE)]
    for case in range(24):
        convs = random_parts(rng, int(rng.integers(1, 12)), int(rng.integers(1, 120)))
        convs.insert(int(rng.integers(0, len(convs))), [(None, [], 3)] * 40 + [(7, [], 1)] * 30 + [(None, [5], 2)] * 30 + [(None, [], 0)] * 25)
        convs.append([(None, [9] * (case % 4), 2)])
        inputs.append(parts_table(convs))
    for ids, oo, ctrl, pf, conv in inputs:
        for tile, cap in ((16, 4), (64, 16), (4096, 1024)):
            e = expected_joined(ids, oo, ctrl, pf, conv)
            m = join_model.join_model(ids, oo, ctrl, pf, conv, IGN, tile=tile, cap=cap)
            forms |= m.pop("forms")
            tails.add(e["n_ids"] % 4)
            for k in ("n_ids", "n_ctrl", "n_labelled"):
                assert m[k] == e[k], k
            for k in ("ids", "offsets", "labels", "part_index"):
                assert m[k] == e[k].tolist(), (k, tile)
    assert forms == {"lds", "global", "one load", "walk"} and tails == {0, 1, 2, 3}


def test_new_symbols_declared_in_header_and_shim():
    hdr = open(os.path.join(ROOT, "include", "tekken_hip.h")).read()
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^(int|void)\s+%s\s*\(" % name, hdr, re.M), name
        assert re.search(r"\bfn\s+%s\s*\(" % name, ffi), name
    for name, value in DEFINES.items():
        assert re.search(r"#define %s %s\b" % (name, value), hdr), name
        m = re.search(r"\bconst %s\s*:\s*\w+\s*=\s*([0-9A-Fa-fx_]+)\s*;" % name, ffi)
        assert m and int(m.group(1).replace("_", ""), 0) == int(value.rstrip("u"), 0), name
    assert re.search(r"typedef struct tk_join_opts\b", hdr) and re.search(r"typedef struct tk_join\b", hdr)
    assert re.search(r"\bstruct TkJoinOpts\b", ffi) and re.search(r"\bstruct TkJoin\b", ffi)


def test_python_constants_match_the_header(tk):
    assert (tk.CHECK_PARTS, tk.JOIN_NONE, tk.PART_LABEL_CTRL, tk.PART_LABEL_TEXT, tk.JOIN_LABELS, tk.JOIN_PART_INDEX) \
        == (CHECK_PARTS, NONE, LABEL_CTRL, LABEL_TEXT, LABELS, PART_INDEX)
    for name in NEW_SYMBOLS:
        assert hasattr(tk.lib(), name), name
    for name in ("join_from_ids_device", "encode_parts_device_join", "encode_parts_join"):
        assert hasattr(tk.Engine, name), name
    for name in ("encode_conversations", "encode_chat", "encode_chat_padded"):
        assert hasattr(tk.Tekkenizer, name), name
    assert hasattr(tk, "JoinResult")


def test_host_only_tokenizer_has_no_chat_batches(tk, small_vocab):
    from test_host_tokenizer import model
    t = tk.Tekkenizer.from_json(json.dumps(model(small_vocab["tokens"])), device=-1)
    chat = [[{"role": "user", "content": "hello"}]]
    for call in (lambda: t.encode_conversations([[("<s>", "hello", False)]]), lambda: t.encode_conversations([], return_tensors="np"),
                 lambda: t.encode_chat(chat), lambda: t.encode_chat(chat, return_tensors="np"), lambda: t.encode_chat_padded(chat)):
        with pytest.raises(tk.TokenizerError) as e:
            call()
        assert e.value.code == tk.TK_ERR_NO_DEVICE
    t.close()
