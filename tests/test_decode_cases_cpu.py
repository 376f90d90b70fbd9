"""The case tables of tests/decode_cases.py against the plain-Python model of the emit kernel's bookkeeping in the same file: every
table reaches the steps, store classes and length sources it is there for (so the GPU tests cannot pass while missing their
target), and tk_oracle.decode_ref accepts the cases meant to be valid and rejects the others with the class meant."""
import pytest

import decode_cases as dc
import helpers
from decode_cases import IGNORE, KEEP, RAISE


@pytest.fixture(scope="module")
def v():
    return helpers.table_edge_vocab(33001)


def test_vocabulary_shape():
    for n in (32767, 32768, 33001):
        v = helpers.table_edge_vocab(n)
        toks = v["tokens"]
        assert len(toks) == n and toks[:256] == [bytes([b]) for b in range(256)]
        for (m, f), r in v["edge"].items():
            assert len(toks[r]) == m and r < 1000
        assert sorted({m for m, _ in v["edge"]}) == list(helpers.EDGE_LENGTHS)
        assert len(toks[v["long"]]) == 5000
        for r, m in {**v["hand"], **v["high"]}.items():
            assert len(toks[r]) == m and any(b >= 0x80 for b in toks[r]) and toks[r].decode("utf-8")
        assert all(2 <= len(toks[r]) <= 6 for r in range(1000, 32764))
    assert n % 4 == 1 and len(set(v["hand"].values())) == len(v["hand"]) == 8 and sorted(v["hand"]) == list(range(32764, 32772))
    assert (v["hand"][32767], v["hand"][32768]) == (255, 254) and v["hand"][32769] >= 255       # the split at 32768 changes a length
    assert [len(s.encode()) for s in v["specials"]] == [5, 3, 4, 0, 18, 16, 36, 300]
    # flavours: the cut ones end / begin inside a character
    zh = v["tokens"][v["edge"][(64, "zh_cut")]]
    assert zh[-1] == 0xE4 and v["tokens"][v["edge"][(65, "zh_tail")]][0] == 0xB8
    assert (zh + v["tokens"][v["edge"][(65, "zh_tail")]]).decode("utf-8") == "中" * 43


def test_model_on_a_hand_made_batch(v):
    ns = v["num_special"]
    a = ns + 0x61
    t64, t300 = ns + v["edge"][(64, "ascii")], ns + v["edge"][(300, "ascii")]
    docs = [[a] * 3, [], [t64] * 63 + [a] * 62 + [7]] + [[]] * 13 + [[t300] * 14, [ns + 32768, ns + 32767, 3, ns + 40000]]
    steps = dc.paths_of(v, docs, KEEP)
    assert [(s["group"], len(s["ids"]), s["residue"], s["span"], s["direct"]) for s in steps] == \
        [(0, 64, 0, 3 + 61 * 64, False), (0, 64, 3, 2 * 64 + 62, False), (0, 1, 1, 300, False), (1, 18, 1, 14 * 300 + 509, True)]
    assert (steps[0]["doc_starts"], steps[0]["empty_starts"], steps[0]["empty_at_end"]) == (3, 1, 13)
    assert steps[3]["classes"][-4:] == [("direct_blob", "global"), ("direct_blob", "fallback_lds"), ("special:0", "sp_offs"), ("oov", "none")]
    assert steps[2]["classes"] == [("special:17+", "sp_offs")] and steps[0]["classes"][0] == ("inline", "lds")
    assert dc.paths_of(v, docs, IGNORE)[2]["classes"] == [("special:dropped", "none")]
    # one byte more in the second step: 3 + 4093 does not fit behind the cursor's residue
    docs[2] = [t64] * 63 + [a] * 61 + [ns + v["edge"][(2, "ascii")]] + [7]
    assert [s["direct"] for s in dc.paths_of(v, docs, KEEP)][:2] == [False, False]
    docs[2] = [t64] * 3 + [a] * 58 + [t64] * 64
    s = dc.paths_of(v, docs, KEEP)
    assert (s[0]["residue"], s[0]["span"], s[0]["direct"], s[1]["residue"], s[1]["span"], s[1]["direct"]) == (0, 3 + 3 * 64 + 58, False, 1, 4096, True)


def valid(v, docs, policy):
    return dc.reference(v, docs, policy)[0] == "ok"


@pytest.mark.parametrize("policy", [IGNORE, KEEP, RAISE])
def test_table_a_reaches_both_sides_at_every_residue(v, policy):
    docs = dc.table_a(v, policy)
    assert len(docs) % dc.GROUP_DOCS == 0 and valid(v, docs, policy)
    steps = dc.paths_of(v, docs, policy)
    under_test = [s for s in steps if len(s["ids"]) == dc.STEP and s["span"] >= 4000]
    # every total at every residue, and so both sides of (cursor & 3) + span > 4096 at every residue
    assert {(s["residue"], s["span"]) for s in under_test} >= {(r, t) for r in range(4) for t in dc.TOTALS}
    for r in range(4):
        assert {s["direct"] for s in under_test if s["residue"] + s["span"] in (4096, 4097) and s["residue"] == r} == {False, True}
    assert all(s["direct"] == (s["residue"] + s["span"] > 4096) for s in steps)
    # the steps in front are full and of 61..64 (without specials 64..67) bytes
    assert {s["span"] for s in steps if s["span"] < 100 and len(s["ids"]) == dc.STEP} == ({61, 62, 63, 64} if policy != RAISE else {64, 65, 66, 67})
    got = dc.reached(steps)
    sp = {KEEP: ["special:0", "special:1-15", "special:16", "special:17+"], IGNORE: ["special:dropped"], RAISE: []}[policy]
    want = {("image", c, "lds") for c in ("inline", "blob16", "image_loop")} | {("direct", c, "lds") for c in ("direct_regs", "direct_blob")}
    want |= {("image", "image_loop", "fallback_lds"), ("direct", "direct_blob", "fallback_lds"), ("direct", "direct_blob", "fallback_global")}
    want |= {(p, c, "sp_offs" if policy == KEEP else "none") for p in ("image", "direct") for c in sp}
    assert got == want, (sorted(got - want), sorted(want - got))
    # document boundaries inside direct steps: several starts in one step, empty documents among them and at the group's end
    direct = [s for s in steps if s["direct"]]
    assert any(s["doc_starts"] >= 4 for s in direct) and any(s["empty_starts"] >= 2 for s in direct)
    assert any(s["empty_at_end"] >= 9 for s in direct) and any(s["empty_at_end"] == 0 for s in direct)
    # every store class INSIDE one direct step, and the 5000-byte token among 63 short ones
    full = {c for p, c, _ in want if p == "direct"}
    assert any({c for c, _ in s["classes"]} >= full for s in direct)
    ns = v["num_special"]
    assert sum(1 for s in direct if ns + v["long"] in s["ids"] and len(s["ids"]) == dc.STEP and s["span"] < 5600) == 2
    if policy == KEEP:
        assert any(s["ids"].count(7) == 13 and s["residue"] + s["span"] == 4097 for s in direct)


def test_table_a_without_its_64_byte_tokens_misses_the_boundary(v):
    """(What the check above is for: the same table over tokens of 63 and 65 bytes only no longer reaches every total.)"""
    ns = v["num_special"]
    t64 = {ns + v["edge"][(64, f)] for f in helpers.EDGE_FLAVOURS}
    docs = [[i for i in d if i not in t64] for d in dc.table_a(v, KEEP)]
    steps = [s for s in dc.paths_of(v, docs, KEEP) if len(s["ids"]) == dc.STEP and s["span"] >= 4000]
    assert not {(s["residue"], s["span"]) for s in steps} >= {(r, t) for r in range(4) for t in dc.TOTALS}


@pytest.mark.parametrize("n_ranks", [32767, 32768, 33001])
@pytest.mark.parametrize("policy", [IGNORE, KEEP, RAISE])
def test_table_b_reaches_every_length_source(n_ranks, policy):
    v = helpers.table_edge_vocab(n_ranks)
    docs = dc.table_b(v, policy)
    assert valid(v, docs, policy)
    steps = dc.paths_of(v, docs, policy)
    src = {c[1] for s in steps for c in s["classes"]}
    want = {"lds", "fallback_lds"} | ({"global", "fallback_global"} if n_ranks == 33001 else set()) | ({"sp_offs"} if policy == KEEP else {"none"} if policy == IGNORE else set())
    assert src == want
    ns, ids = v["num_special"], {i for d in docs for i in d}
    assert ids >= {ns + r for r in v["hand"]} | {ns + r for r in v["high"]} | {ns + v["long"]}
    assert n_ranks - 1 + ns in ids or n_ranks == 33001                      # the last rank of the table
    hand = [ns + r for r in sorted(v["hand"])]
    assert hand in docs and hand[::-1] in docs
    assert {len(v["tokens"][i - ns]) for i in ids if i >= ns} >= {254, 255, 256, 300, 5000}
    assert any(sum(len(d) for d in docs[g:g + 16]) > 256 for g in range(0, len(docs), 16))      # the unrolled loop of the group pass
    where = ("lds", "fallback_lds") + (("global", "fallback_global") if n_ranks == 33001 else ())
    assert dc.reached(steps) >= {(p, c, w) for p, c in (("image", "image_loop"), ("direct", "direct_blob")) for w in where}


@pytest.mark.parametrize("policy", [IGNORE, KEEP, RAISE])
def test_table_c_cases_are_what_they_say(v, policy):
    cases = dc.table_c(v, policy)
    seen = set()
    for name, docs, bad in cases:
        assert len(docs) == 40
        want = ("ok",) if bad is None else ("err", bad, "utf8")
        got = dc.reference(v, docs, policy)
        assert (got[0],) + tuple(got[1:] if got[0] == "err" else ()) == want, name
        # the document under test lies in ONE step, of the path the name says
        steps = [s for s in dc.paths_of(v, docs, policy) if s["group"] == 1]
        at = sum(len(d) for d in docs[16:21])
        assert at + len(docs[21]) + (len(docs[22]) if name.endswith("/end") else 0) <= dc.STEP
        assert steps[0]["direct"] == name.startswith("direct/"), name
        seen.add((name.split("/")[0], name.split("/")[-1]))
        if bad is not None:                                       # the valid twin of every invalid case
            assert (name.rsplit("/", 1)[0] + "/valid") in {c[0] for c in cases}
    kinds = {"valid", "end", "start"} | ({"special"} if policy != RAISE else set())
    assert seen == {(p, k) for p in ("image", "direct") for k in kinds}
    classes = {c[0] for name, docs, bad in cases for s in dc.paths_of(v, docs, policy) for c in s["classes"]}
    assert classes >= {"inline", "blob16", "image_loop", "direct_regs", "direct_blob"}


def test_table_d_offenders(v):
    batches = dc.table_d(v)
    firsts = set()
    for docs in batches[:-2]:
        assert 45 <= len(docs) <= 60
        kinds = []
        for d, ids in enumerate(docs):
            r = dc.reference(v, [ids], RAISE)
            if r[0] == "err":
                kinds.append(r[2])
                gap = 0
                while not docs[d - gap - 1]:
                    gap += 1
                assert gap in (1, 2, 17)
                firsts.add((r[2], gap))
        assert sorted(kinds) == ["key", "special", "utf8"]
        assert dc.reference(v, docs, RAISE)[2] == kinds[0] and dc.reference(v, docs, KEEP)[2] == [k for k in kinds if k != "special"][0]
    assert firsts == {(k, g) for k in ("key", "utf8", "special") for g in (1, 2, 17)}
    assert len({dc.reference(v, docs, RAISE)[1:] for docs in batches}) > 6
    for docs in batches[-2:]:
        n = len(docs) - 1 - (2 if not docs[-1] else 0)
        assert docs[n][-1] == v["num_special"] + len(v["tokens"]) and not docs[n - 1]
        assert dc.reference(v, docs, IGNORE) == ("err", n, "key")


def test_sweep_documents(v):
    docs = dc.sweep_docs(v)
    assert len(docs) == 20000 and max(len(d) for d in docs) <= 40 and min(len(d) for d in docs) == 0
    r = dc.reference(v, docs, KEEP)
    assert r[0] == "ok"
    multi = sum(1 for t in r[1] if any(b >= 0x80 for b in t))
    assert 20000 // 3 <= multi <= 20000 // 2
    assert all(docs[d] for d in (8191, 8192, 8193, 16383, 16384, 16385, 8197, 16393))
