"""What the lossy-decode tests share: a plain-Python restatement of lossy UTF-8 decoding of a run (substitution of maximal
subparts: python's bytes.decode("utf-8", "replace"), Rust's from_utf8_lossy), of the lossy decode of a document -- the grouping of
tk_oracle.decode_ref (reference src/tekkenizer.rs:463-560) with that rule in place of the UTF-8 error -- and of the stream step
with its hold-back.  tests/test_decode_lossy_cpu.py holds the restatement to python's codec; the GPU tests compare with it."""
import re

import numpy as np

IGNORE, KEEP, RAISE = 0, 1, 2
STREAM_FINAL = 1
REPL = b"\xef\xbf\xbd"
# the bytes where the rules change
ALPHA24 = [0x41, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF, 0xE0, 0xE1, 0xEC, 0xED, 0xEE, 0xEF, 0xF0, 0xF1,
           0xF3, 0xF4, 0xF5, 0xFF]
ALPHA12 = [0x41, 0x80, 0xA0, 0xBF, 0xC1, 0xC2, 0xE0, 0xED, 0xEF, 0xF0, 0xF4, 0xF5]


_NOT_ASCII = re.compile(rb"[\x80-\xff]")


def lead(b):
    """(what b begins: 1 ASCII, 0 nothing, 2..4 a sequence of that length; the bounds of the second byte)"""
    lo, hi = 0x80, 0xBF
    if b < 0x80:
        return 1, lo, hi
    if b < 0xC2 or b > 0xF4:
        return 0, lo, hi
    if b < 0xE0:
        return 2, lo, hi
    if b < 0xF0:
        return 3, (0xA0 if b == 0xE0 else lo), (0x9F if b == 0xED else hi)
    return 4, (0x90 if b == 0xF0 else lo), (0x8F if b == 0xF4 else hi)


def lossy_run(run, hold=False):
    """(lossy text of the run, the truncated prefix held back at its end -- only with hold --, U+FFFD written)"""
    out, i, n, nrep = bytearray(), 0, len(run), 0
    while i < n:
        b = run[i]
        need, lo, hi = lead(b)
        if need == 1:                                     # (a stretch of ASCII at once: the tests decode megabytes)
            m = _NOT_ASCII.search(run, i)
            j = m.start() if m else n
            out += run[i:j]
            i = j
            continue
        if need == 0:
            out += REPL
            nrep += 1
            i += 1
            continue
        m = 1
        while m < need and i + m < n and (lo if m == 1 else 0x80) <= run[i + m] <= (hi if m == 1 else 0xBF):
            m += 1
        if m == need:
            out += run[i:i + m]
        elif hold and i + m == n:
            return bytes(out), bytes(run[i:]), nrep
        else:
            out += REPL
            nrep += 1
        i += m
    return bytes(out), b"", nrep


def lossy_cut(doc, starts, hold=False):
    """A byte string cut at `starts` into runs, each lossy-decoded on its own (hold: only the last run holds back)."""
    cuts = [0] + sorted({s for s in starts if 0 < s < len(doc)}) + [len(doc)]
    out, pend, nrep = b"", b"", 0
    for k, (a, b) in enumerate(zip(cuts, cuts[1:])):
        t, pend, r = lossy_run(doc[a:b], hold and k == len(cuts) - 2)
        out += t
        nrep += r
    return out, pend, nrep


def _walk(v, ids, policy, pending, final):
    """The groups of decode_ref over `pending ++ ids`: (text, pending left, U+FFFD written); ValueError("special" / "key")."""
    ns, toks = v["num_special"], v["tokens"]
    out, nrep, run = [], 0, bytearray(pending)
    ids = list(ids)
    last_special = False
    for i in ids:
        if i < ns:
            if policy == RAISE:
                raise ValueError("special")
            t, _, r = lossy_run(run)                      # a special id (a dropped one too) closes the run
            out.append(t)
            nrep += r
            run = bytearray()
            if policy == KEEP:
                out.append(v["specials"][i].encode("utf-8"))
            last_special = True
        else:
            if i - ns >= len(toks):
                raise ValueError("key")
            run += toks[i - ns]
            last_special = False
    t, pend, r = lossy_run(run, hold=not final and not last_special)
    out.append(t)
    return b"".join(out), pend, nrep + r


def decode_lossy(v, ids, policy):
    """(lossy text of one document, U+FFFD written)"""
    t, _, r = _walk(v, ids, policy, b"", True)
    return t, r


def reference(v, id_lists, policy):
    """("ok", texts, n_replaced, first document with a replacement or None, documents with one), or ("err", first document that
    raises, what)."""
    out, nrep, first, dirty = [], 0, None, 0
    for d, ids in enumerate(id_lists):
        try:
            t, r = decode_lossy(v, ids, policy)
        except ValueError as e:
            return ("err", d, str(e))
        if r and first is None:
            first = d
        nrep += r
        dirty += r > 0
        out.append(t)
    return ("ok", out, nrep, first, dirty)


def state_word(pend):
    return sum(b << (8 * k) for k, b in enumerate(pend)) | (len(pend) << 24)


def state_bytes(word):
    n = (word >> 24) & 0xFF
    return bytes((word >> (8 * k)) & 0xFF for k in range(min(n, 3)))


def stream_step(v, states, id_lists, policy, flags=0):
    """One step over all sequences: (texts, new state words, U+FFFD written).  ValueError as decode_ref, states untouched."""
    texts, new, nrep = [], [], 0
    for st, ids in zip(states, id_lists):
        t, pend, r = _walk(v, ids, policy, state_bytes(int(st)), bool(flags & STREAM_FINAL))
        texts.append(t)
        new.append(state_word(pend))
        nrep += r
    return texts, new, nrep


def ragged(id_lists):
    oo = np.zeros(len(id_lists) + 1, np.uint64)
    if id_lists:
        oo[1:] = np.cumsum([len(x) for x in id_lists])
    return np.array([i for x in id_lists for i in x], np.uint32), oo


def random_docs(v, rng, n_docs, max_ids):
    """Documents of 0..max_ids ids over helpers.table_edge_vocab: three in ten clean (letters, whole characters, specials), the others
    byte tokens, edge tokens of up to 33 bytes (many end or begin inside a character) and specials."""
    V, NS = v, v["num_special"]
    edge = [V["edge"][k] for k in V["edge"] if k[0] <= 33]
    docs = []
    for d in range(n_docs):
        n = int(rng.integers(0, max_ids + 1))
        kind = rng.random()
        ids = []
        for _ in range(n):
            r = rng.random()
            if kind < 0.3:                                    # a clean document: letters, whole characters, specials
                ids.append(NS + 0x61 + int(rng.integers(0, 26)) if r < 0.8 else NS + V["edge"][(int(rng.choice([4, 8, 16])), "rocket")] if r < 0.95
                           else int(rng.integers(0, NS)))
            elif r < 0.5:
                ids.append(NS + int(rng.integers(0, 256)))
            elif r < 0.9:
                ids.append(NS + int(rng.choice(edge)))
            else:
                ids.append(int(rng.integers(0, NS)))
        docs.append(ids)
    return docs
