"""Lossy batch decode on the GPU (tk_decode_batch_lossy / tk_decode_batch_device_lossy; csrc/tk_decode_lossy.hip) against the
restatement of tests/decode_lossy_cases.py, which tests/test_decode_lossy_cpu.py holds to python's own codec: text bytes, document
offsets, the number of U+FFFD and the first dirty document, under Ignore and Keep, through the host and the device entry.  The
vocabulary is helpers.table_edge_vocab: its 256 byte tokens reach any byte string."""
import numpy as np
import pytest

import decode_lossy_cases as lc
import helpers

pytestmark = pytest.mark.gpu

TILE = 4096              # TK_LOSSY_TILE: raw text bytes of a block
MAX_BLOCKS = 2048        # TK_LOSSY_MAX_BLOCKS: the grid cap of the repair kernels
POLICIES = (lc.IGNORE, lc.KEEP)
V = helpers.table_edge_vocab(33001)
NS = V["num_special"]
ROCKET = "\U0001f680".encode()
PATTERNS = [ROCKET, b"\xf0\x9f\x9a", b"\xe0\x80", b"\xed\xa0\x80", b"\xbf"]


@pytest.fixture(scope="module")
def eng(tk):
    e = tk.Engine(V["tokens"], NS, V["bos"], V["eos"], device=0)
    e.set_special_tokens(V["specials"])
    yield e
    e.close()


def codec_count(bs):
    return bs.decode("utf-8", "replace").count("\ufffd")


def byte_ids(bs):
    return [NS + x for x in bs]


def ascii_ids(n, k=0):
    """n bytes of ASCII text in few ids: the longest "ascii" edge token that still fits, then letters."""
    out = []
    for ln in sorted(helpers.EDGE_LENGTHS, reverse=True):
        while n >= ln:
            out.append(NS + V["edge"][(ln, "ascii")])
            n -= ln
    return out + [NS + 0x61 + (k + j) % 26 for j in range(n)]


def device_decode(eng, ids, oo, policy, errors):
    import torch
    d_ids = torch.from_numpy(np.ascontiguousarray(ids if len(ids) else np.zeros(1, np.uint32)).view(np.int32)).cuda()
    d_oo = torch.from_numpy(oo.astype(np.int64)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    v_b, v_o = eng.decode_batch_device(d_ids.data_ptr(), d_oo.data_ptr(), len(oo) - 1, len(ids), policy, st, errors=errors)
    offs = torch.as_tensor(v_o, device="cuda").cpu().numpy().astype(np.uint64)
    data = torch.as_tensor(v_b, device="cuda").cpu().numpy() if int(offs[-1]) else np.zeros(0, np.uint8)
    return data, offs, (v_b.__cuda_array_interface__["data"][0], v_o.__cuda_array_interface__["data"][0])


def compare(data, offs, ref, what):
    want_offs = np.zeros(len(ref[1]) + 1, np.uint64)
    want_offs[1:] = np.cumsum([len(t) for t in ref[1]])
    assert offs.shape == want_offs.shape, what
    bad = np.nonzero(offs != want_offs)[0]
    assert len(bad) == 0, (what, "first differing offset: document", int(bad[0]), int(offs[bad[0]]), int(want_offs[bad[0]]))
    want = np.frombuffer(b"".join(ref[1]), np.uint8)
    assert data.shape == want.shape, (what, data.shape, want.shape)
    bad = np.nonzero(data != want)[0]
    assert len(bad) == 0, (what, "first differing byte", int(bad[0]), "document", int(np.searchsorted(want_offs, bad[0], "right")) - 1,
                           int(data[bad[0]]), int(want[bad[0]]), len(bad))


def check(eng, docs, policy, what, ref=None):
    """One batch through both lossy entries against the restatement; returns the restatement's answer."""
    ref = ref or lc.reference(V, docs, policy)
    assert ref[0] == "ok", what
    ids, oo = lc.ragged(docs)
    data, offs = eng.decode_batch(ids, oo, policy, errors="replace")
    compare(data, offs, ref, (what, "host"))
    assert (eng.n_replaced, eng.first_bad_doc) == (ref[2], ref[3]), (what, "host")
    data, offs, _ = device_decode(eng, ids, oo, policy, "replace")
    compare(data, offs, ref, (what, "device"))
    assert (eng.n_replaced, eng.first_bad_doc) == (ref[2], ref[3]), (what, "device")
    stats = eng.last_decode_lossy()
    assert stats["n_replaced"] == ref[2] and stats["n_bad_docs"] == ref[4], what
    assert (stats["repair_launches"] > 0) == (ref[2] > 0), what
    return ref


@pytest.mark.parametrize("policy", POLICIES)
def test_where_strict_succeeds_nothing_is_added(tk, eng, policy):
    """Valid input: the strict entry's text and offsets, the strict entry's own device buffers, no kernel behind the strict pipeline."""
    clean = [ascii_ids(300, 1) + byte_ids("é中".encode()) + [1, NS + V["edge"][(16, "rocket")]], [], ascii_ids(5000), [2, 3], byte_ids(ROCKET)]
    batches = {"no documents": [], "all empty": [[] for _ in range(40)], "all ascii": [ascii_ids(n, n) for n in (1, 17, 4096, 4097, 300, 0, 9000)],
               "mixed": clean}
    for name, docs in batches.items():
        ids, oo = lc.ragged(docs)
        ref = check(eng, docs, policy, name)
        assert ref[2] == 0 and ref[3] is None
        s_data, s_offs = eng.decode_batch(ids, oo, policy)
        l_data, l_offs = eng.decode_batch(ids, oo, policy, errors="replace")
        assert np.array_equal(s_data, l_data) and np.array_equal(s_offs, l_offs), name
        _, _, strict_ptrs = device_decode(eng, ids, oo, policy, "strict")
        _, _, lossy_ptrs = device_decode(eng, ids, oo, policy, "replace")
        assert strict_ptrs == lossy_ptrs, name
        stats = eng.last_decode_lossy()
        assert stats["repair_launches"] == 0 and stats["repair_ms"] == 0.0 and stats["strict_ms"] > 0.0 or not docs, name
    with pytest.raises(tk.TokenizerError):
        eng.decode_batch(*lc.ragged(clean), policy, errors="ignore")


@pytest.mark.parametrize("policy", POLICIES)
def test_every_offset_of_a_tile_edge_and_of_a_step_edge(eng, policy):
    """A complete character, three truncated or ill-formed sequences and a lone continuation byte at offsets -4..+4 around the
    edges of a thread's 16 bytes, of the validate kernel's 256-byte step, of a wave's 1024 bytes and of the 4096-byte tile.  Every
    document is padded to whole tiles, so the edge is where the document says; a special id sits in front of some patterns."""
    docs = []
    for edge in (16, 256, 1024, TILE):
        for k in range(-4, 5):
            for j, pat in enumerate(PATTERNS):
                head = ascii_ids(edge + k, k + j)
                if (k + j) % 3 == 0:
                    head = head[:-1] + [3] + head[-1:]          # the empty special: a run start one letter in front of the pattern
                used = edge + k + len(pat)
                docs.append(head + byte_ids(pat) + ascii_ids(-used % TILE + TILE * (k & 1), j))
    ref = check(eng, docs, policy, "edges")
    assert ref[2] == 4 * 9 * sum(codec_count(p) for p in PATTERNS)   # (the ASCII around a pattern changes nothing)
    # ... and the same patterns at the very end of a document, the next document starting with a continuation byte
    docs = []
    for k in range(-4, 5):
        for pat in PATTERNS:
            docs += [ascii_ids(TILE + k - len(pat)) + byte_ids(pat), byte_ids(b"\x9a\x80") + ascii_ids(-(k + 2) % TILE)]
    check(eng, docs, policy, "edges at document ends")


def test_hard_boundaries(eng):
    """E2 82 | AC: two replacements, never the euro sign -- across a document boundary, a dropped special, every kept special."""
    a, b = byte_ids(b"\xe2\x82"), byte_ids(b"\xac")
    assert lc.decode_lossy(V, a + b, lc.IGNORE) == ("€".encode(), 0)
    for policy in POLICIES:
        ref = check(eng, [byte_ids(b"abcde") + a, b + byte_ids(b"abc")], policy, "document boundary")
        assert ref[1] == [b"abcde" + lc.REPL, lc.REPL + b"abc"] and ref[2] == 2
    ref = check(eng, [[]] + [a + [sp] + b for sp in range(NS)], lc.IGNORE, "dropped specials")
    assert ref[1][1:] == [lc.REPL * 2] * NS
    ref = check(eng, [a + [sp] + b + [sp] for sp in range(NS)] + [[]], lc.KEEP, "kept specials")
    assert ref[1][:-1] == [lc.REPL + s.encode() + lc.REPL + s.encode() for s in V["specials"]]


@pytest.mark.parametrize("policy", POLICIES)
def test_growth_and_bookkeeping(eng, policy):
    ref = check(eng, [byte_ids(b"\x80" * 5000)], policy, "5000 continuation bytes")
    assert ref[1] == [lc.REPL * 5000]
    ref = check(eng, [byte_ids(b"\xf0\x90\x80" * 2000)], policy, "2000 truncated prefixes")
    assert ref[1] == [lc.REPL * 2000]
    dirty = [byte_ids(b"ab\xc3"), byte_ids(b"\xa9 \xf0\x9f") + ascii_ids(40), byte_ids(b"\xff" * 70)]
    empties = [[], [], dirty[0], [], dirty[1], [], [], [], dirty[2], [], []]
    check(eng, empties, policy, "empty documents around dirty ones")
    check(eng, [dirty[2]] + [[] for _ in range(37)], policy, "trailing empty documents")
    # dirty documents and documents without a byte >= 0x80 interleaved: the emit kernel's groups of 16 are mixed
    mixed = []
    for d in range(70):
        mixed.append(ascii_ids(10 + 37 * d % 900, d) if d % 3 else ascii_ids(d) + byte_ids(PATTERNS[1 + d % 4]) + ascii_ids(2 * d))
    ref = check(eng, mixed, policy, "dirty and ascii documents interleaved")
    assert ref[3] == 0 and ref[2] == sum(codec_count(PATTERNS[1 + d % 4]) for d in range(0, 70, 3))


def test_second_sweep(eng):
    """More text than the grid cap times the tile (the smallest such batch): tiles of the second sweep, a dirty document among them."""
    per = 300 * 1024
    n_clean = MAX_BLOCKS * TILE // per + 1
    docs = [[NS + V["edge"][(300, "ascii")]] * 1024 for _ in range(n_clean)]
    docs.insert(1, byte_ids(b"x\xe4\xb8"))
    docs.append(ascii_ids(100) + byte_ids(b"\xf0\x9f\x9a\x80\xf0\x9f\x9a") + ascii_ids(5000) + byte_ids(b"\xc0"))
    docs.append(ascii_ids(7))
    assert (n_clean - 1) * per < MAX_BLOCKS * TILE < n_clean * per
    ref = check(eng, docs, lc.IGNORE, "second sweep")
    assert ref[2] == 3 and ref[3] == 1


@pytest.mark.parametrize("policy", POLICIES)
def test_random_documents(eng, policy):
    rng = np.random.default_rng(23 + policy)
    docs = lc.random_docs(V, rng, 2000, 300)
    ref = lc.reference(V, docs, policy)
    assert ref[4] > len(docs) // 4 and len(docs) - ref[4] > len(docs) // 6
    check(eng, docs, policy, "random", ref)


def test_errors_that_remain(tk, eng):
    """A special id under Raise and an id outside the vocabulary: the strict entry's code and bad_doc, dirty documents or not."""
    dirty = byte_ids(b"a\xc3")
    for docs, policy in (([dirty, ascii_ids(9), [NS + 97, 1], dirty], lc.RAISE),
                         ([ascii_ids(9), dirty, [], [NS + len(V["tokens"]) + 3] + dirty], lc.IGNORE),
                         ([dirty, [NS + len(V["tokens"])], [1]], lc.RAISE), ([[1], [NS + len(V["tokens"])]], lc.RAISE)):
        ids, oo = lc.ragged(docs)
        clean = [[NS + 97] if d is dirty else [i for i in d if i not in dirty[1:]] for d in docs]   # the same batch without the invalid bytes
        with pytest.raises(tk.TokenizerError) as strict:
            eng.decode_batch(*lc.ragged(clean), policy)
        ref = lc.reference(V, docs, policy)
        assert ref[0] == "err"
        for entry in ("host", "device"):
            with pytest.raises(tk.TokenizerError) as e:
                if entry == "host":
                    eng.decode_batch(ids, oo, policy, errors="replace")
                else:
                    device_decode(eng, ids, oo, policy, "replace")
            assert (e.value.code, e.value.kind, e.value.bad_doc) == (strict.value.code, strict.value.kind, strict.value.bad_doc) == \
                (strict.value.code, {"special": "SpecialTokenPolicy", "key": "Tokenizers"}[ref[2]], ref[1]), (docs, entry)
    # Raise without a special id decodes
    ref = check(eng, [dirty, ascii_ids(9)], lc.RAISE, "raise, no specials")
    assert ref[2] == 1
