"""Streaming decode on the GPU (tk_decode_stream_step_device / tk_decode_stream_step; the stream kernels of
csrc/tk_decode_lossy.hip) against the restatement of tests/decode_lossy_cases.py and against the bulk lossy entry: only complete
characters leave a step, the open tail waits in the state word, and any split of an id sequence into steps gives the lossy decode
of the whole sequence."""
import numpy as np
import pytest

import decode_lossy_cases as lc
import helpers

pytestmark = pytest.mark.gpu

V = helpers.table_edge_vocab(33001)
NS = V["num_special"]
ROCKET = "\U0001f680".encode()
POLICIES = (lc.IGNORE, lc.KEEP)


@pytest.fixture(scope="module")
def eng(tk):
    e = tk.Engine(V["tokens"], NS, V["bos"], V["eos"], device=0)
    e.set_special_tokens(V["specials"])
    yield e
    e.close()


def byte_ids(bs):
    return [NS + x for x in bs]


def states(stream):
    return [int(x) & 0xFFFFFFFF for x in stream.state.cpu().numpy().tolist()]


def step_and_check(stream, id_lists, policy, flags=0):
    """One step on the GPU against the restatement from the same states: texts and the new state words."""
    before = states(stream)
    want, new, _ = lc.stream_step(V, before, id_lists, policy, flags)
    got = stream.step(id_lists, flags)
    assert got == want, [(q, g, w) for q, (g, w) in enumerate(zip(got, want)) if g != w][:3]
    assert states(stream) == new
    return got


def test_rocket_one_byte_token_a_step(eng):
    for policy in POLICIES:
        s = eng.decode_stream(3, policy)
        out, seen = [], []
        for b in ROCKET:
            out.append(step_and_check(s, [[NS + b], [], [NS + 0x61]], policy))
            seen.append(states(s)[0])
        assert [o[0] for o in out] == [b"", b"", b"", ROCKET] and [o[2] for o in out] == [b"a"] * 4
        assert seen == [0x010000F0, 0x02009FF0, 0x039A9FF0, 0]
        assert s.finish() == [b"", b"", b""]


@pytest.mark.parametrize("policy", POLICIES)
def test_split_invariant_against_the_bulk_entry(eng, policy):
    """500 random sequences, each cut into 1..6 steps (some of them empty), specials included: the steps' texts plus the final
    flush are what the bulk lossy entry gives for the whole sequences -- and what the restatement gives."""
    rng = np.random.default_rng(5 + policy)
    seqs = lc.random_docs(V, rng, 500, 40)
    n_steps = 6
    plan = []
    for ids in seqs:
        k = int(rng.integers(1, n_steps + 1))
        cuts = sorted(int(c) for c in rng.integers(0, len(ids) + 1, k - 1))
        parts = [ids[a:b] for a, b in zip([0] + cuts, cuts + [len(ids)])]
        where = sorted(rng.choice(n_steps, k, replace=False).tolist())      # the steps the parts go to; the others are empty
        row = [[] for _ in range(n_steps)]
        for w, p in zip(where, parts):
            row[w] = p
        plan.append(row)
    s = eng.decode_stream(len(seqs), policy)
    got = [b""] * len(seqs)
    held = 0
    for j in range(n_steps):
        out = step_and_check(s, [row[j] for row in plan], policy)
        got = [g + o for g, o in zip(got, out)]
        held += sum(1 for x in states(s) if x)
    got = [g + o for g, o in zip(got, step_and_check(s, [[] for _ in seqs], policy, lc.STREAM_FINAL))]
    assert held > 50 and states(s) == [0] * len(seqs)
    want = eng.decode_docs(seqs, policy, errors="replace")
    ref = lc.reference(V, seqs, policy)
    assert ref[0] == "ok" and want == ref[1]
    assert got == want


@pytest.mark.parametrize("n_seqs", [0, 1, 63, 64, 65, 257])
def test_sequence_counts(eng, n_seqs):
    rng = np.random.default_rng(n_seqs)
    s = eng.decode_stream(n_seqs, lc.KEEP)
    total = [b""] * n_seqs
    whole = [[] for _ in range(n_seqs)]
    for _ in range(3):
        ids = [[int(rng.integers(0, NS)) if rng.random() < 0.1 else NS + int(rng.choice(lc.ALPHA24)) for _ in range(int(rng.integers(0, 5)))]
               for _ in range(n_seqs)]
        whole = [w + i for w, i in zip(whole, ids)]
        total = [t + o for t, o in zip(total, step_and_check(s, ids, lc.KEEP))]
    total = [t + o for t, o in zip(total, s.finish())]
    assert total == lc.reference(V, whole, lc.KEEP)[1] and states(s) == [0] * n_seqs


def test_flushes_and_slots(eng):
    open3 = byte_ids(ROCKET[:3])
    # an open prefix flushed by a special id, in front of the special's own string under Keep
    s = eng.decode_stream(2, lc.KEEP)
    assert step_and_check(s, [open3, byte_ids(b"\xe4")], lc.KEEP) == [b"", b""]
    assert step_and_check(s, [[6] + byte_ids(b"\x80"), [NS + 0xB8]], lc.KEEP) == [lc.REPL + V["specials"][6].encode() + lc.REPL, b""]
    assert step_and_check(s, [[], [NS + 0xAD]], lc.KEEP) == [b"", "中".encode()]
    # ... by a dropped special at the end of a step: nothing is held behind it
    s = eng.decode_stream(2, lc.IGNORE)
    assert step_and_check(s, [open3 + [1], open3], lc.IGNORE) == [lc.REPL, b""]
    assert states(s) == [0, lc.state_word(ROCKET[:3])]
    assert step_and_check(s, [[NS + 0x80], [NS + 0x80]], lc.IGNORE) == [lc.REPL, ROCKET]
    # ... by TK_STREAM_FINAL, in a step with ids and in one without; the state is zero after the final step
    s = eng.decode_stream(3, lc.IGNORE)
    assert step_and_check(s, [open3, byte_ids(b"a\xc3"), []], lc.IGNORE) == [b"", b"a", b""]
    assert step_and_check(s, [[], byte_ids(b"\xa9\xe2\x82"), byte_ids(b"\xf0")], lc.IGNORE, lc.STREAM_FINAL) == [lc.REPL, "é".encode() + lc.REPL, lc.REPL]
    assert states(s) == [0, 0, 0]
    # a slot zeroed in mid-stream starts fresh while its neighbours go on
    s = eng.decode_stream(3, lc.IGNORE)
    assert step_and_check(s, [open3, open3, open3], lc.IGNORE) == [b"", b"", b""]
    s.reset([1])
    assert states(s) == [lc.state_word(ROCKET[:3]), 0, lc.state_word(ROCKET[:3])]
    assert step_and_check(s, [[NS + 0x80]] * 3, lc.IGNORE) == [ROCKET, lc.REPL, ROCKET]
    s.reset()
    assert states(s) == [0, 0, 0]


def test_errors_leave_the_states_alone(tk, eng):
    """An id outside the vocabulary (a special id under Raise) in one sequence: the strict entry's code, bad_seq names the
    sequence, the state buffer is bit for bit what it was -- through the device entry and through the host entry."""
    oov = NS + len(V["tokens"]) + 1
    for bad_ids, policy in (([NS + 0x61, oov], lc.IGNORE), ([NS + 0x61, 2], lc.RAISE)):
        with pytest.raises(tk.TokenizerError) as strict:
            eng.decode_docs([bad_ids], policy)
        s = eng.decode_stream(70, policy)
        first = [byte_ids(ROCKET[:1 + q % 3]) for q in range(70)]
        step_and_check(s, first, policy)
        before = states(s)
        assert all(before)
        ids = [[NS + 0x9F] for _ in range(70)]
        ids[67] = bad_ids
        with pytest.raises(tk.TokenizerError) as e:
            s.step(ids)
        assert (e.value.code, e.value.bad_seq) == (strict.value.code, 67)
        assert states(s) == before
        host_state = np.array(before, np.uint32)
        with pytest.raises(tk.TokenizerError) as e:
            eng.decode_stream_step(host_state, ids, policy)
        assert (e.value.code, e.value.bad_seq) == (strict.value.code, 67) and host_state.tolist() == before
        # the same step without the offender goes through, on both entries, with the same answer
        ids[67] = [NS + 0x9F]
        want, new, _ = lc.stream_step(V, before, ids, policy)
        assert eng.decode_stream_step(host_state, ids, policy) == want and host_state.tolist() == new
        assert s.step(ids) == want and states(s) == new


def test_tokenizer_level(tk, small_vocab):
    """Tekkenizer: errors="replace" on decode_batch and decode_batch_padded, n_replaced, and a stream of str."""
    import json
    from test_host_tokenizer import model
    t = tk.Tekkenizer.from_json(json.dumps(model(small_vocab["tokens"])), device=0)
    ns = t.num_special_tokens()
    rows = [[1] + [ns + b for b in "hé".encode()] + [ns + 0xF0, ns + 0x9F], [ns + 0x80, ns + 0x61, 2]]
    with pytest.raises(tk.TokenizerError):
        t.decode_batch(rows)
    assert t.decode_batch(rows, errors="replace") == ["hé\ufffd", "\ufffda"] and t.n_replaced == 2
    assert t.decode_batch(rows, tk.SpecialTokenPolicy.Keep, errors="replace") == ["<s>hé\ufffd", "\ufffda</s>"]
    pad = np.full((2, 8), 0, np.int32)
    for r, row in enumerate(rows):
        pad[r, :len(row)] = row
    assert t.decode_batch_padded(pad, lengths=[len(r) for r in rows], pad_id=0, errors="replace") == ["hé\ufffd", "\ufffda"] and t.n_replaced == 2
    s = t.decode_stream(2)
    assert s.step([[ns + 0xF0], [ns + 0x68]]) == ["", "h"]
    assert s.step([[ns + 0x9F, ns + 0x9A], [ns + 0xC3]]) == ["", ""]
    assert s.step([[ns + 0x80, ns + 0x21], []]) == ["\U0001f680!", ""]
    assert s.finish() == ["", "\ufffd"] and not s.state.any()
    t.close()
