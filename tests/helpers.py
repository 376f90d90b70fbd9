"""Shared helpers of the test-suite."""
import functools
import os
import pickle
import random

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def small_trained_vocab(n_merges=3000, n_ranks=6000, seed=0x7E44E2):
    """256 bytes + BPE merges trained on a small synthetic sample, grown to n_ranks tokens."""
    import synth_vocab as sv
    cache = os.path.join(ROOT, "assets", "test_vocab_%d_%d.pkl" % (n_merges, n_ranks))
    if os.path.exists(cache):
        with open(cache, "rb") as f:
            return pickle.load(f)
    toks = sv.build_tokens(n_ranks, n_merges, 1500, 300, seed)
    v = {"tokens": toks, "num_special": 1000, "bos": 1, "eos": 2}
    os.makedirs(os.path.dirname(cache), exist_ok=True)
    with open(cache, "wb") as f:
        pickle.dump(v, f)
    return v


EDGE_LENGTHS = (2, 3, 4, 7, 8, 9, 14, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 254, 255, 256, 300)
EDGE_FLAVOURS = ("ascii", "mb", "zh_cut", "zh_tail", "e", "rocket")
EDGE_SPECIALS = ["<unk>", "<s>", "</s>", "", "[/AVAILABLE_TOOLS]", "0123456789abcdef", "é🚀" * 6, "x" * 300]
EDGE_LONG = 5000                 # the one token far beyond every one-byte length field
# ranks around the end of the LDS part of the decode kernels' one-byte length table (TKD_L8_LDS = 32768), pairwise different
# lengths: the last rank of the LDS part holds a token of 255 bytes (the 0xFF escape), the first rank behind it one of 254
EDGE_HAND = {32764: 16, 32765: 65, 32766: 33, 32767: 255, 32768: 254, 32769: 300, 32770: 17, 32771: 128}
EDGE_HIGH = {32780: 254, 32781: 255, 32782: 256, 32783: 300, 32784: EDGE_LONG}   # the longest tokens once more, above the split


def _edge_valid_mb(n, salt):
    """n bytes of valid UTF-8 that is not ASCII: ü, 中, 🚀 and a letter in rotation (from `salt`), each time the next that fits."""
    chars = ["ü".encode(), "中".encode(), "\U0001f680".encode(), bytes([0x61 + salt % 26])]
    out, k = b"", salt
    while len(out) < n:
        out += next(c for c in (chars[(k + j) % 4] for j in range(4)) if len(out) + len(c) <= n)
        k += 1
    return out


def _edge_token(n, flavour):
    zh, e, ro = "中".encode(), "é".encode(), "\U0001f680".encode()
    if flavour == "ascii":
        return (b" quick brown fox jumps over the lazy dog," * (n // 40 + 1))[:n]
    if flavour == "mb":
        return _edge_valid_mb(n, 0)
    if flavour == "zh_cut":                       # ends inside a character unless n is a multiple of three
        return (zh * (n // 3 + 1))[:n]
    if flavour == "zh_tail":                      # begins inside a character
        return (zh * (n // 3 + 2))[1:1 + n]
    return ((e if flavour == "e" else ro) * (n // 2 + 1))[:n]


def _edge_filler(r):
    """2..6 bytes, distinct for every rank: the rank in base 94 over '!'..'~'; every third rank of four bytes or more begins with é."""
    n, q = 2 + r % 5, r // 5
    lead = "é".encode() if r % 3 == 0 and n >= 4 else b""
    return lead + bytes(0x21 + (q // 94 ** j) % 94 for j in range(n - len(lead)))


@functools.lru_cache(maxsize=None)
def table_edge_vocab(n_ranks):
    """A made-up vocabulary for the edges of the decode, spans and words kernels' token tables (they read token bytes only: nothing
    is trained).  256 byte tokens; every length of EDGE_LENGTHS in every flavour of EDGE_FLAVOURS ("edge": (length, flavour) ->
    rank); one token of EDGE_LONG bytes ("long"); EDGE_HAND and EDGE_HIGH at their ranks ("mb" text, salted), as far as n_ranks
    reaches; every other rank short filler.  Specials: EDGE_SPECIALS (0, 16, 18, 36 and 300 bytes among them)."""
    tokens = [bytes([b]) for b in range(256)]
    edge = {}
    for n in EDGE_LENGTHS:
        for f in EDGE_FLAVOURS:
            edge[(n, f)] = len(tokens)
            tokens.append(_edge_token(n, f))
    long_rank = len(tokens)
    tokens.append(_edge_valid_mb(EDGE_LONG, 1))
    placed = {**EDGE_HAND, **EDGE_HIGH}
    assert n_ranks > len(tokens) and max(placed.values()) <= EDGE_LONG
    for r in range(len(tokens), n_ranks):
        tokens.append(_edge_valid_mb(placed[r], 2 + r % 20) if r in placed else _edge_filler(r))
    assert len(set(tokens)) == len(tokens) == n_ranks
    return {"tokens": tokens, "num_special": len(EDGE_SPECIALS), "bos": 1, "eos": 2, "specials": list(EDGE_SPECIALS), "edge": edge,
            "long": long_rank, "hand": {r: n for r, n in EDGE_HAND.items() if r < n_ranks},
            "high": {r: n for r, n in EDGE_HIGH.items() if r < n_ranks}}


EDGE_DOCS = [b"", b" ", b"\n", b"\t", b"   \n\t   ", "\U0001f680".encode(), b"a" * 1000, b"Hello\x00World",
             b"Line1\nLine2\rLine3\r\nLine4", b"a", b"ab", b"'s", b"x's", b" " * 70, b"\n" * 70 + b"x", b"z" * 64,
             b"z" * 65, b"q" * 63 + b" ", ("中" * 40).encode(), ("é" * 33).encode(), b"1" * 100,
             b"!" * 90 + b"\n\n", b"the " * 40, b"<s>[INST] hi [/INST]</s>"]


def mixed_docs(n_ascii=60, n_mixed=25, n_zipf=60, max_len=5000):
    import corpus
    docs = []
    d, o = corpus.generate("ascii", n_ascii, 512, seed=corpus.BASE_SEED + 1)
    docs += corpus.docs_of(d, o)
    d, o = corpus.generate("mixed", n_mixed, 2048, seed=corpus.BASE_SEED + 2)
    docs += corpus.docs_of(d, o)
    d, o = corpus.generate("zipf", n_zipf, seed=corpus.BASE_SEED + 4)
    docs += [x for x in corpus.docs_of(d, o) if len(x) <= max_len]
    return docs + list(EDGE_DOCS)


def random_unicode_docs(n, seed=7, max_len=120):
    alpha = ["a", "S", "s", "t", "r", "e", "l", "v", "m", "d", "x", "1", "2", "'", "!", " ", " ", "\n", "\r", "\t",
             "ſ", "é", "中", "٣", " ", " ", "　", "\U0001f680", "́", "\x00", "-"]
    rng = random.Random(seed)
    return ["".join(rng.choice(alpha) for _ in range(rng.randint(0, max_len))).encode("utf-8") for _ in range(n)]


def walked_lead_byte_docs():
    """Both sides of TKF_WALKCAP (672 lead bytes per region that the multi-byte walk of tk_flat_chunk_impl.h deals out over the lanes; more
    are walked lane by lane).  Two-byte chars that the range rules of tkf_classify do not cover -- Armenian letters (lead bytes D4 /
    D5), section and pilcrow signs, U+00A0 and U+0085 (lead C2), an NKo digit (lead DF) -- in a fixed mixed order, 600 .. 1024 of them
    per 2048-byte stretch, padded with "x "; every stretch three times over as one document, and twice over behind 31 ASCII letters."""
    chars = ["\u0531", "\u00a7", "\u0561", "\u00a0", "\u0540", "\u00b6", "\u0575", "\u0085", "\u07c1"]
    assert all(len(c.encode("utf-8")) == 2 for c in chars)
    docs = []
    for k in (600, 640, 671, 672, 673, 704, 900, 1024):
        s = "".join(chars[i % len(chars)] for i in range(k)).encode("utf-8")
        s += (b"x " * 1024)[:2048 - len(s)]
        assert len(s) == 2048
        docs += [s * 3, (b"abcdefghijklmnopqrstuvwxyzabcde" + s) * 2]
    return docs


def window_cut_docs():
    """A two-, three- and four-byte char that the END of the per-document path's first 64-byte window cuts, or just does not
    (tk_encode_impl.h step 1 trims the window to the last whole char, the slide starts the next window on it): the char behind
    61 .. 64 ASCII letters, then more of it and a CR LF behind a class-O char for the window after the slide."""
    return [b"a" * k + ch.encode("utf-8") + b" b " + ch.encode("utf-8") * 3 + b"\r\n x" for k in range(61, 65) for ch in ("é", "中", "\U0001f680")]


def oracle_for(v):
    import tk_oracle
    return tk_oracle.Oracle(v["tokens"], v["num_special"], v["bos"], v["eos"])


def starts_to_pieces(doc, starts):
    s = list(starts) + [len(doc)]
    return [doc[s[i]:s[i + 1]] for i in range(len(s) - 1)]


# ---- what the GPU tests of the layout passes share (test_gpu_dense / _seqpack / _join.py) ----

def to_host(view, shape, dtype):
    """A DeviceView as a numpy array of `shape` (an int: one dimension); an unselected output (None) stays None, and an empty
    tensor has nothing behind its pointer to look at."""
    import torch
    shape = shape if isinstance(shape, tuple) else (shape,)
    if view is None:
        return None
    if 0 in shape:
        return np.zeros(shape, dtype)
    return torch.as_tensor(view, device="cuda").cpu().numpy().view(dtype).reshape(shape)


def dev(a, dtype):
    """A host array on the device, seen as `dtype` (uint32 / uint64 go up as the signed type of the same width)."""
    import torch
    a = np.ascontiguousarray(a, dtype)
    if len(a) == 0:
        a = np.zeros(1, dtype)
    return torch.from_numpy(a.view({np.uint32: np.int32, np.uint64: np.int64, np.uint8: np.uint8}[dtype])).cuda()


def on_device(ids, oo):
    """Ragged ids and their offsets on the device."""
    return dev(ids, np.uint32), dev(oo, np.uint64)


def assert_array_same(got, exp, what=""):
    """Shape, dtype and every element; an unselected output is None on both sides."""
    assert (got is None) == (exp is None), what
    if exp is None:
        return
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype)
    bad = np.argwhere(got != exp)
    assert len(bad) == 0, (what, "first differing element", bad[0].tolist(), int(got[tuple(bad[0])]), int(exp[tuple(bad[0])]))


def assert_same(got, exp, what="", counts=(), arrays=()):
    """Two result dicts: the counts equal, the arrays element by element."""
    for k in counts:
        assert got[k] == exp[k], (what, k, got[k], exp[k])
    for k in arrays:
        assert_array_same(got[k], exp[k], (what, k))
