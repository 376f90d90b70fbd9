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
