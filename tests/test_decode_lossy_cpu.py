"""Lossy UTF-8 decoding on the CPU: the restatement of tests/decode_lossy_cases.py against python's own codec, the split
invariant of the stream step, and csrc/tk_utf8_lossy.h -- the scalar step the repair and stream kernels run -- through a
stand-alone program built with the address and undefined-behaviour sanitizers, against the restatement on the same cases."""
import itertools
import os
import random
import subprocess

import pytest

import decode_lossy_cases as lc

HERE = os.path.dirname(os.path.abspath(__file__))


def codec(doc, starts=()):
    cuts = [0] + sorted({s for s in starts if 0 < s < len(doc)}) + [len(doc)]
    return b"".join(doc[a:b].decode("utf-8", "replace").encode() for a, b in zip(cuts, cuts[1:]))


def test_restatement_matches_the_codec_on_random_strings():
    rng = random.Random(7)
    n = dirty = 0
    for _ in range(60000):
        if rng.random() < 0.7:
            doc = bytes(rng.choice(lc.ALPHA24) for _ in range(rng.randint(0, 9)))
        else:                                            # (well-formed text, dirty only where a run start cuts a character)
            doc = "".join(rng.choice("aé中\U0001f680߿ࠀ\U0010ffff") for _ in range(rng.randint(0, 4))).encode()
        starts = [rng.randrange(len(doc) + 1) for _ in range(rng.choice([0, 0, 1, 2]))]
        want = codec(doc, starts)
        got, pend, nrep = lc.lossy_cut(doc, starts)
        assert got == want and pend == b"" and nrep == want.count(lc.REPL), (doc, starts)
        n += 1
        dirty += nrep > 0
    assert dirty > n // 4 and n - dirty > n // 6


def test_restatement_matches_the_codec_exhaustive_short():
    """every string of up to four bytes over the critical bytes, with and without a run start at every position"""
    for ln in (0, 1, 2, 3, 4):
        for t in itertools.product(lc.ALPHA12, repeat=ln):
            doc = bytes(t)
            for starts in ([],) + tuple([s] for s in range(1, ln)):
                assert lc.lossy_cut(doc, starts)[0] == codec(doc, starts), (doc, starts)
                # the hold-back: what is held is a truncated prefix, and text + U+FFFD-for-it is the whole answer
                text, pend, _ = lc.lossy_cut(doc, starts, hold=True)
                assert len(pend) <= 3 and text + (lc.REPL if pend else b"") == codec(doc, starts), (doc, starts)


def _vocab():
    toks = [bytes([b]) for b in range(256)] + ["🚀".encode(), "中".encode()[:2], "é".encode()]
    return {"tokens": toks, "num_special": 4, "specials": ["<unk>", "<s>", "", "é🚀"]}


def test_split_invariant():
    """Any split of an id sequence into steps (empty ones too): the steps' texts plus the final flush are the lossy decode of the
    whole sequence; specials under every policy."""
    v = _vocab()
    rng = random.Random(3)
    ns = v["num_special"]
    held = 0
    for it in range(6000):
        policy = it % 3
        n = rng.randint(0, 12)
        ids = [ns + (rng.choice(lc.ALPHA24) if rng.random() < 0.8 else rng.randrange(256, 259)) for _ in range(n)]
        if policy != lc.RAISE or it % 2:
            ids = [rng.randrange(ns) if rng.random() < 0.15 else i for i in ids]
        k = rng.randint(1, 5)
        cuts = sorted(rng.randint(0, n) for _ in range(k - 1))
        steps = [ids[a:b] for a, b in zip([0] + cuts, cuts + [n])]
        try:
            want, nrep = lc.decode_lossy(v, ids, policy)
        except ValueError as e:
            assert str(e) == "special" and policy == lc.RAISE
            with pytest.raises(ValueError):
                st = [0]
                for s in steps:
                    _, st, _ = lc.stream_step(v, st, [s], policy)
            continue
        st, got, r = [0], b"", 0
        for j, s in enumerate(steps):
            final = lc.STREAM_FINAL if j == len(steps) - 1 and it % 2 else 0
            t, st, rr = lc.stream_step(v, st, [s], policy, final)
            held += st[0] != 0
            got += t[0]
            r += rr
        t, st, rr = lc.stream_step(v, st, [[]], policy, lc.STREAM_FINAL)     # the final flush (nothing left after a final step)
        assert st == [0] and got + t[0] == want and r + rr == nrep, (ids, steps, policy)
    assert held > 300


def _program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lossy") / "utf8_lossy_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(HERE, "utf8_lossy_check.c")])
    return exe


def test_header_program_against_the_restatement(tmp_path_factory):
    exe = _program(tmp_path_factory)
    rng = random.Random(11)
    cases = []
    for ln in (0, 1, 2, 3):
        for t in itertools.product(lc.ALPHA12, repeat=ln):
            for starts in ([],) + tuple([s] for s in range(1, ln)):
                cases.append((bytes(t), list(starts)))
    good = ["a", "é", "中", "\U0001f680", "߿", "ࠀ", "퟿", "\U00010000", "\U0010ffff"]
    for _ in range(40000):
        k = rng.random()
        if k < 0.6:
            doc = bytes(rng.choice(lc.ALPHA24) for _ in range(rng.randint(0, 9)))
        else:
            doc = "".join(rng.choice(good) for _ in range(rng.randint(1, 8))).encode()
            if k < 0.8 and doc:
                i = rng.randrange(len(doc))
                doc = doc[:i] + bytes([rng.choice(lc.ALPHA24)]) + doc[i + 1:]
        cases.append((doc, [rng.randrange(len(doc) + 1) for _ in range(rng.choice([0, 0, 1, 2, 3]))]))
    d = tmp_path_factory.mktemp("lossy_io")
    fin, fout = str(d / "cases.txt"), str(d / "out.txt")
    with open(fin, "w") as f:
        for doc, starts in cases:
            f.write("%s %x\n" % (doc.hex() or "-", sum(1 << s for s in set(starts) if s < max(len(doc), 1))))
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    with open(fout) as f:
        lines = f.read().split("\n")[:-1]
    assert len(lines) == len(cases)
    unhex = lambda s: b"" if s == "-" else bytes.fromhex(s)
    n = dirty = 0
    for (doc, starts), line in zip(cases, lines):
        full, held, fed, state = line.split(" ")
        want = codec(doc, starts)
        w_full, _, nrep = lc.lossy_cut(doc, starts)
        w_held, pend, _ = lc.lossy_cut(doc, starts, hold=True)
        assert w_full == want
        assert unhex(full) == want, (doc, starts, line)
        assert unhex(held) == w_held and unhex(fed) == w_held, (doc, starts, line, w_held)
        assert int(state, 16) == lc.state_word(pend), (doc, starts, line)
        n += 1
        dirty += nrep > 0
    assert dirty > n // 4 and n - dirty > n // 6


# ---- the header, the shim and the binding ----
NEW_SYMBOLS = ["tk_decode_batch_lossy", "tk_decode_batch_device_lossy", "tk_decode_stream_step_device", "tk_decode_stream_step",
               "tk_last_decode_lossy_ms", "tk_last_decode_lossy_stats"]


def test_header_shim_and_binding_declare_the_entries(tk):
    import inspect
    import re
    root = os.path.dirname(HERE)
    hdr = open(os.path.join(root, "include", "tekken_hip.h")).read()
    ffi = open(os.path.join(root, "shim", "src", "ffi.rs")).read()
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bfn\s+%s\s*\(" % name, ffi), name
    assert re.search(r"#define TK_STREAM_FINAL 1\b", hdr) and re.search(r"\bconst TK_STREAM_FINAL\s*:\s*c_int\s*=\s*1\s*;", ffi)
    assert tk.STREAM_FINAL == lc.STREAM_FINAL == 1
    assert all(name in doc for name in NEW_SYMBOLS[:4])
    # errors= defaults to "strict" everywhere: today's callers see nothing new
    for fn in (tk.Engine.decode_batch, tk.Engine.decode_docs, tk.Engine.decode_batch_device, tk.Tekkenizer.decode_batch,
               tk.Tekkenizer.decode_batch_padded):
        assert inspect.signature(fn).parameters["errors"].default == "strict", fn
    assert all(hasattr(tk.DecodeStream, m) for m in ("step", "step_device", "finish", "reset")) and hasattr(tk.Tekkenizer, "decode_stream")
