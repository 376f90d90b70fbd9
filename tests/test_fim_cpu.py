"""Fill-in-the-middle rows (include/tekken_hip.h tk_fim_split_device): the definition restated with plain loops over units,
hand-made cases of every rule, invariants on random inputs, the hash and the draws against the binomial, the header's values, the
exported symbols, the shim's declarations and the binding's description of the struct."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_layout_binding_cpu import header_members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF
NONE = 0xFFFFFFFF
NO_CUT = 0xFFFFFFFFFFFFFFFF
SNAP, BOS, EOS, PART_SRC, LABEL_MIDDLE = 1, 2, 4, 8, 16
LABEL_CTRL, LABEL_TEXT = 1, 2
BOTH = LABEL_CTRL | LABEL_TEXT
ONE = 1 << 32                   # a rate of 1 in q32
PRE, SUF, MID = 5, 6, 7         # control ids of the hand-made cases
VALUES = {"TK_FIM_SNAP": SNAP, "TK_FIM_BOS": BOS, "TK_FIM_EOS": EOS, "TK_FIM_PART_SRC": PART_SRC, "TK_FIM_LABEL_MIDDLE": LABEL_MIDDLE}
NEW_SYMBOLS = ["tk_fim_split_device", "tk_fim_split_ids_device", "tk_encode_batch_device_fim", "tk_fim_from_ids_device",
               "tk_encode_batch_fim", "tk_free_fim", "tk_last_fim_ms", "tk_fim_tile"]
ARRAYS = ("units", "part_offsets", "part_ctrl", "part_flags", "conv_offsets", "part_src", "cuts", "mode")
COUNTS = ("n_docs", "n_parts", "n_units", "n_transformed", "n_spm", "n_skipped")


def h(seed, d):
    """The regroup pass's hash, as the header states it at TK_REGROUP_ORDER_SHUFFLE."""
    x = (d * 0x9E3779B1 + seed) & M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def draws(seed, d):
    """Step 2: (u_0, u_1, u_2, u_3) of document d."""
    return [h(h(seed & M32, (0x46494D00 + k) & M32), d & M32) for k in range(4)]


def fim_opts(rate_q32=0, spm_q32=0, seed=0, prefix_id=PRE, suffix_id=SUF, middle_id=MID, head=0, tail=0, min_units=0, flags=0):
    return dict(rate_q32=rate_q32, spm_q32=spm_q32, seed=seed, prefix_id=prefix_id, suffix_id=suffix_id, middle_id=middle_id, head=head,
                tail=tail, min_units=min_units, flags=flags)


def snap(body, c):
    """Step 3 for one cut, on bytes."""
    n = len(body)
    for _ in range(3):
        if not (0 < c < n and (body[c] & 0xC0) == 0x80):
            break
        c -= 1
    return c


def expected_fim(units, offs, opts, cuts=None, unit_bytes=1, num_special=1000, bos=1, eos=2):
    """Steps 1-6: the result of tk_fim_split_device (unit_bytes 1) / tk_fim_split_ids_device (4) as a dict of numpy arrays and
    counts, document by document.  What the entries refuse raises ValueError."""
    o = fim_opts(**opts)
    flags, head, tail = o["flags"], o["head"], o["tail"]
    text = unit_bytes == 1
    if flags & ~(SNAP | BOS | EOS | PART_SRC | LABEL_MIDDLE) or (not text and flags & (BOS | EOS)):
        raise ValueError("flags")
    if o["rate_q32"] > ONE or o["spm_q32"] > ONE:
        raise ValueError("rate")
    if text and (head or tail):
        raise ValueError("head / tail")
    if any(i != NONE and i >= num_special for i in (o["prefix_id"], o["suffix_id"], o["middle_id"])):
        raise ValueError("control id")
    src = [int(x) for x in np.asarray(units).tolist()]
    offs = [int(x) for x in offs]
    D = len(offs) - 1
    if D >= 2 ** 32 - 16:
        raise ValueError("n_docs")
    out, poffs, ctrl, pfl, psrc, cuts_out, mode = [], [], [], [], [], [], []
    n_tr = n_spm = n_skip = 0
    for d in range(D):
        start, end = offs[d], offs[d + 1]
        ln = end - start
        whole = ln >= head + tail                       # step 1
        hh, tt = (head, tail) if whole else (0, 0)
        body = src[start + hh:end - tt]
        n = len(body)
        u = draws(o["seed"], d)                         # step 2
        if cuts is not None:
            cand = int(cuts[d][0]) != NO_CUT
            ok = whole and n < 2 ** 32 - 1
            c = [min(int(cuts[d][0]), n), min(int(cuts[d][1]), n)]
        else:
            cand = u[0] < o["rate_q32"]
            ok = whole and n >= max(o["min_units"], 1) and n < 2 ** 32 - 1
            c = [(u[2] * (n + 1)) >> 32, (u[3] * (n + 1)) >> 32]
        tr = cand and ok
        n_skip += cand and not tr
        spm = tr and u[1] < o["spm_q32"]
        if tr and text and flags & SNAP:                # step 3
            c = [snap(body, c[0]), snap(body, c[1])]
        lo, hi = min(c), max(c)
        b0 = start + hh
        head_part = (o_bos(flags, bos) if text else NONE, src[start:b0], start)
        tail_part = (o_eos(flags, eos) if text else NONE, src[end - tt:end], end - tt)
        if not tr:                                      # step 4
            parts = [head_part, (NONE, body, b0), (NONE, [], b0 + n), (NONE, [], b0 + n), tail_part]
            fl = [BOTH] * 5
        else:
            P, M, S = (o["prefix_id"], body[:lo], b0), (o["middle_id"], body[lo:hi], b0 + lo), (o["suffix_id"], body[hi:], b0 + hi)
            assert P[1] + M[1] + S[1] == body
            parts = [head_part] + ([S, P, M] if spm else [P, S, M]) + [tail_part]
            fl = [0, 0, 0, LABEL_TEXT, BOTH] if flags & LABEL_MIDDLE else [BOTH] * 5   # step 5
        for (cid, seg, at), f in zip(parts, fl):
            poffs.append(len(out))
            ctrl.append(cid)
            pfl.append(f)
            psrc.append(at)
            out += seg
        assert len(out) == end                          # the document keeps its range
        n_tr += tr
        n_spm += spm
        cuts_out.append((lo, hi) if tr else (NO_CUT, NO_CUT))
        mode.append(2 if spm else 1 if tr else 0)
    poffs.append(len(out))
    dt = np.uint8 if text else np.uint32
    return {"units": np.array(out, dt), "part_offsets": np.array(poffs, np.uint64), "part_ctrl": np.array(ctrl, np.uint32),
            "part_flags": np.array(pfl, np.uint32), "conv_offsets": np.arange(0, 5 * D + 1, 5, dtype=np.uint64),
            "part_src": np.array(psrc, np.uint64) if flags & PART_SRC else None,
            "cuts": np.array(cuts_out, np.uint64).reshape(D, 2), "mode": np.array(mode, np.uint8),
            "n_docs": D, "n_parts": 5 * D, "n_units": len(out), "n_transformed": int(n_tr), "n_spm": int(n_spm), "n_skipped": int(n_skip)}


def o_bos(flags, bos):
    return bos if flags & BOS else NONE


def o_eos(flags, eos):
    return eos if flags & EOS else NONE


def pack(docs, dtype=np.uint8):
    offs = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
    flat = [x for d in docs for x in d]
    return np.array(flat, dtype), offs


def split_text(docs, cuts=None, **kw):
    kw.setdefault("flags", SNAP | PART_SRC)
    data, offs = pack(docs)
    return expected_fim(data, offs, fim_opts(**kw), cuts)


def split_ids(docs, cuts=None, **kw):
    kw.setdefault("flags", PART_SRC)
    ids, offs = pack(docs, np.uint32)
    return expected_fim(ids, offs, fim_opts(**kw), cuts, unit_bytes=4)


def texts(r, d=0):
    """The five part texts of document d."""
    po, u = r["part_offsets"], r["units"]
    return [bytes(u[int(po[5 * d + p]):int(po[5 * d + p + 1])].tolist()) if u.dtype == np.uint8
            else u[int(po[5 * d + p]):int(po[5 * d + p + 1])].tolist() for p in range(5)]


# ---- hand-made cases of every rule ----

def test_psm_and_spm_on_one_document():
    doc = b"0123456789"
    r = split_text([doc], [(3, 7)], spm_q32=0)
    assert texts(r) == [b"", b"012", b"789", b"3456", b""] and r["mode"].tolist() == [1]
    assert r["part_ctrl"].tolist() == [NONE, PRE, SUF, MID, NONE] and r["part_src"].tolist() == [0, 0, 7, 3, 10]
    assert r["units"].tobytes() == b"0127893456" and r["cuts"].tolist() == [[3, 7]]
    r = split_text([doc], [(7, 3)], spm_q32=ONE, flags=SNAP | BOS | EOS | PART_SRC)   # (the order of the two cuts does not matter)
    assert texts(r) == [b"", b"789", b"012", b"3456", b""] and r["mode"].tolist() == [2]
    assert r["part_ctrl"].tolist() == [1, SUF, PRE, MID, 2] and r["part_src"].tolist() == [0, 7, 0, 3, 10]
    assert r["units"].tobytes() == b"7890123456" and (r["n_transformed"], r["n_spm"], r["n_skipped"]) == (1, 1, 0)
    assert r["conv_offsets"].tolist() == [0, 5] and r["part_offsets"].tolist() == [0, 0, 3, 6, 10, 10]


def test_cuts_at_0_at_n_and_equal():
    doc = b"abcdef"
    for cut, parts in (((0, 0), [b"", b"", b"abcdef", b"", b""]), ((6, 6), [b"", b"abcdef", b"", b"", b""]),
                       ((0, 6), [b"", b"", b"", b"abcdef", b""]), ((2, 2), [b"", b"ab", b"cdef", b"", b""]),
                       ((4, 99), [b"", b"abcd", b"", b"ef", b""])):        # (a given cut is clamped to n)
        r = split_text([doc], [cut])
        assert texts(r) == parts, cut
        assert r["n_transformed"] == 1 and sorted(r["units"].tolist()) == sorted(doc)
    r = split_text([doc, b"", doc], [(NO_CUT, 3), (0, 0), (1, NO_CUT)])
    assert r["mode"].tolist() == [0, 1, 1] and r["cuts"].tolist() == [[NO_CUT, NO_CUT], [0, 0], [1, 6]]
    assert texts(r, 0) == [b"", doc, b"", b"", b""] and texts(r, 1) == [b""] * 5    # (an empty document with cuts given: transformed, all empty)
    assert r["part_src"][:5].tolist() == [0, 0, 6, 6, 6]


def test_snap_inside_2_3_and_4_byte_characters():
    two, three, four = "é".encode(), "中".encode(), "\U0001f680".encode()
    doc = b"a" + two + three + four + b"z"              # starts: 0 | 1 | 3 | 6 | 10
    starts = {0: 0, 1: 1, 2: 1, 3: 3, 4: 3, 5: 3, 6: 6, 7: 6, 8: 6, 9: 6, 10: 10, 11: 11}
    for c, s in starts.items():
        r = split_text([doc], [(c, 11)])
        assert r["cuts"].tolist() == [[s, 11]], c
        texts(r)[1].decode("utf-8")                     # the prefix ends on a character boundary
    r = split_text([doc], [(2, 8)], flags=0)            # without TK_FIM_SNAP the cuts stay where they are
    assert r["cuts"].tolist() == [[2, 8]]


def test_snap_stops_after_3_continuation_bytes_and_at_the_last_byte():
    doc = b"a" + b"\x80" * 5 + b"b"                     # invalid UTF-8: a run of 5 continuation bytes at 1..5
    assert split_text([doc], [(5, 7)])["cuts"].tolist() == [[2, 7]]     # 5 -> 4 -> 3 -> 2, and no further
    assert split_text([doc], [(3, 7)])["cuts"].tolist() == [[0, 7]]     # 3 -> 2 -> 1 -> 0
    assert split_text([doc], [(6, 7)])["cuts"].tolist() == [[6, 7]]     # 'b' is no continuation byte
    doc = b"ab\xc3\xa9"                                 # a continuation byte at n - 1
    assert split_text([doc], [(3, 4)])["cuts"].tolist() == [[2, 4]]     # c = n is never moved
    assert split_text([b"\x80\x80"], [(1, 1)])["cuts"].tolist() == [[0, 0]]
    assert split_text([b"\x80\x80"], [(0, 2)])["cuts"].tolist() == [[0, 2]]


def test_head_and_tail_stay_and_short_documents_are_left_alone():
    r = split_ids([[1, 10, 11, 12, 13, 2], [1, 2], [9], [1, 20, 2]], [(1, 3), (0, 0), (0, 1), (1, 1)], head=1, tail=1, spm_q32=ONE)
    assert texts(r, 0) == [[1], [13], [10], [11, 12], [2]] and r["units"][:6].tolist() == [1, 13, 10, 11, 12, 2]
    assert texts(r, 1) == [[1], [], [], [], [2]] and r["mode"][1] == 2            # n == 0 with cuts given: transformed, nothing to move
    assert texts(r, 2) == [[], [9], [], [], []] and r["mode"][2] == 0             # len < head + tail: never transformed, no head, no tail
    assert texts(r, 3) == [[1], [], [20], [], [2]]
    assert (r["n_transformed"], r["n_spm"], r["n_skipped"]) == (3, 3, 1)
    assert r["part_ctrl"][:5].tolist() == [NONE, SUF, PRE, MID, NONE] and r["part_ctrl"][10:15].tolist() == [NONE] * 5
    assert r["part_src"][:5].tolist() == [0, 4, 1, 2, 5]
    with pytest.raises(ValueError):
        split_text([b"abc"], head=1)                    # head / tail belong to the ids entries
    with pytest.raises(ValueError):
        split_ids([[1, 2]], flags=BOS)                  # ... and BOS / EOS to the text entries


def test_min_units_and_n_skipped():
    docs = [b"x" * n for n in (0, 1, 4, 5, 9)]
    r = split_text(docs, rate_q32=ONE, min_units=5)
    assert r["mode"].tolist() == [0, 0, 0, 1, 1] and (r["n_transformed"], r["n_skipped"]) == (2, 3)
    r = split_text(docs, rate_q32=ONE)                  # min_units 0 means 1: an empty document is never drawn
    assert r["mode"].tolist() == [0, 1, 1, 1, 1] and r["n_skipped"] == 1
    r = split_text(docs, rate_q32=0, min_units=5)       # no candidate, nothing skipped
    assert r["mode"].tolist() == [0] * 5 and r["n_skipped"] == 0 and r["n_transformed"] == 0
    r = split_text(docs, [(0, 0)] * 5, min_units=5)     # with cuts min_units plays no part
    assert r["mode"].tolist() == [1] * 5 and r["n_skipped"] == 0


def test_each_id_may_be_none_and_a_bad_id_is_refused():
    for k, name in enumerate(("prefix_id", "suffix_id", "middle_id")):
        r = split_text([b"abcdef"], [(2, 4)], **{name: NONE})
        want = [NONE, PRE, SUF, MID, NONE]
        want[1 + k] = NONE
        assert r["part_ctrl"].tolist() == want
        with pytest.raises(ValueError):
            split_text([b"abcdef"], [(2, 4)], **{name: 1000})
    r = split_text([b"abcdef"], [(2, 4)], spm_q32=ONE, middle_id=NONE)            # Mistral's format
    assert r["part_ctrl"].tolist() == [NONE, SUF, PRE, NONE, NONE] and texts(r) == [b"", b"ef", b"ab", b"cd", b""]
    for bad in (dict(rate_q32=ONE + 1), dict(spm_q32=ONE + 1), dict(flags=32)):
        with pytest.raises(ValueError):
            split_text([b"abc"], **bad)


def test_label_middle_flags():
    r = split_text([b"abcdef", b"xyz"], [(2, 4), (NO_CUT, 0)], flags=LABEL_MIDDLE | BOS | EOS)
    assert r["part_flags"].tolist() == [0, 0, 0, LABEL_TEXT, BOTH] + [BOTH] * 5   # an untransformed document stays fully labelled
    assert split_text([b"abcdef"], [(2, 4)])["part_flags"].tolist() == [BOTH] * 5


# ---- invariants on random inputs ----

def random_docs(rng, D, text):
    if text:
        alpha = ["a", "b", " ", "é", "中", "\U0001f680", "\n"]
        return ["".join(rng.choice(alpha, int(rng.integers(0, 40)))).encode() for _ in range(D)]
    return [rng.integers(0, 5000, int(rng.integers(0, 40))).tolist() for _ in range(D)]


@pytest.mark.parametrize("text", [True, False])
def test_invariants_on_random_input(text):
    rng = np.random.default_rng(11)
    for trial in range(40):
        D = int(rng.integers(0, 30))
        docs = random_docs(rng, D, text)
        head, tail = (0, 0) if text else (int(rng.integers(0, 3)), int(rng.integers(0, 3)))
        kw = dict(rate_q32=int(rng.integers(0, ONE + 1)), spm_q32=int(rng.integers(0, ONE + 1)), seed=trial, head=head, tail=tail,
                  min_units=int(rng.integers(0, 6)))
        cuts = None if trial % 3 else [(int(rng.integers(0, 50)), int(rng.integers(0, 50))) if rng.integers(0, 4) else (NO_CUT, 0) for _ in range(D)]
        r = (split_text if text else split_ids)(docs, cuts, **kw)
        data, offs = pack(docs, np.uint8 if text else np.uint32)
        po, u, ps = r["part_offsets"], r["units"], r["part_src"]
        assert r["n_units"] == len(data) and po[0] == 0 and po[-1] == len(data) and np.all(np.diff(po.astype(np.int64)) >= 0)
        for d in range(D):
            a, b = int(offs[d]), int(offs[d + 1])
            assert po[5 * d] == a and sorted(u[a:b].tolist()) == sorted(data[a:b].tolist())   # a permutation of its own range
            for p in range(5 * d, 5 * d + 5):           # part_src maps back
                n = int(po[p + 1] - po[p])
                assert u[int(po[p]):int(po[p + 1])].tolist() == data[int(ps[p]):int(ps[p]) + n].tolist()
            if r["mode"][d]:
                lo, hi = (int(x) for x in r["cuts"][d])
                assert b - a >= head + tail              # (a shorter document is never transformed)
                body = data[a + head:b - tail].tolist()
                t = texts(r, d)
                P, S = (t[2], t[1]) if r["mode"][d] == 2 else (t[1], t[2])
                assert list(P) + list(t[3]) + list(S) == body and len(P) == lo and len(P) + len(t[3]) == hi   # P + M + S == body
                if text:
                    for piece in (P, t[3], S):
                        piece.decode("utf-8")           # valid UTF-8 in, valid UTF-8 parts out
            else:
                assert u[a:b].tolist() == data[a:b].tolist()
        ident = (split_text if text else split_ids)(docs, None, **dict(kw, rate_q32=0))     # rate 0 is the identity
        assert ident["units"].tolist() == data.tolist() and ident["n_transformed"] == 0 and not ident["mode"].any()


# ---- the hash and the draws ----

def test_hash_literals_from_the_header_formula():
    assert [h(0, 0x46494D00 + k) for k in range(4)] == [0xB4B99A64, 0x128045EB, 0x63DDFAFF, 0x8414EC07]
    assert draws(0, 0) == [0xE2385C18, 0x75B0FF8E, 0x6A33B2EB, 0xEA6FCE3D]
    assert draws(0, 1) == [0x9724CA2C, 0x3C57CF80, 0xF43DA990, 0x78AB7713]
    assert draws(1, 0) == [0xF7522B6F, 0x3DDC53A8, 0x2EFA9FAD, 0x40BB1D52]
    assert draws(7, 12345) == [0xAE94321A, 0x51DC5A02, 0x25CBB9A6, 0x4AF23D4A]
    assert draws(0xFFFFFFFF, 0xFFFFFFEF) == [0x6A6D02F0, 0x64300F62, 0x94FBA5F5, 0x31A8B89A]


def test_epochs_share_no_draw():
    for e in list(range(64)) + [0xFFFFFFFE]:
        a = [h(e, 0x46494D00 + k) for k in range(4)]
        b = [h((e + 1) & M32, 0x46494D00 + k) for k in range(4)]
        assert all(x != y for x, y in zip(a, b)) and len(set(a)) == 4


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_draws_against_the_binomial(seed):
    """D = 4096 at p = 1/2: 5 sigma = 5 * sqrt(0.25 / 4096) = 0.039.  The mean of lo / n, the smaller of two uniform draws, is 1/3."""
    D, n = 4096, 1000
    data, offs = np.zeros(D * n, np.uint8), np.arange(D + 1, dtype=np.uint64) * n
    r = expected_fim(data, offs, fim_opts(rate_q32=1 << 31, spm_q32=1 << 31, seed=seed, flags=0))
    assert abs(r["n_transformed"] / D - 0.5) <= 0.04
    assert abs(r["n_spm"] / r["n_transformed"] - 0.5) <= 0.04
    tr = r["mode"] != 0
    assert abs(float(np.mean(r["cuts"][tr, 0].astype(np.float64) / n)) - 1 / 3) <= 0.03
    assert r["cuts"][tr].max() <= n and np.all(r["cuts"][tr, 0] <= r["cuts"][tr, 1])


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
    assert re.search(r"#define TK_FIM_NO_CUT \(~0ull\)", hdr) and re.search(r"\bconst TK_FIM_NO_CUT\s*:\s*u64\s*=\s*!0\s*;", ffi)
    assert re.search(r"typedef struct tk_fim_opts\b", hdr) and re.search(r"typedef struct tk_fim\b", hdr)
    assert re.search(r"\bstruct TkFimOpts\b", ffi) and re.search(r"\bstruct TkFim\b", ffi)
    assert "0x46494D00" in hdr
    assert "tk_fim_split_device" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    fields = re.search(r"typedef struct tk_fim_opts\s*\{(.*?)\}", hdr, re.S).group(1)
    assert re.sub(r"\s+", " ", fields).strip() == ("uint64_t rate_q32, spm_q32; uint32_t seed, prefix_id, suffix_id, middle_id, head, tail, "
                                                   "min_units, flags;")


def test_python_constants_and_exported_symbols(tk):
    assert (tk.FIM_SNAP, tk.FIM_BOS, tk.FIM_EOS, tk.FIM_PART_SRC, tk.FIM_LABEL_MIDDLE) == (SNAP, BOS, EOS, PART_SRC, LABEL_MIDDLE)
    assert tk.FIM_NO_CUT == NO_CUT and (tk.FIM_NONE, tk.FIM_PSM, tk.FIM_SPM) == (0, 1, 2)
    for name in NEW_SYMBOLS:
        assert hasattr(tk.lib(), name), name
    for name in ("fim_split_device", "fim_split_ids_device", "encode_batch_device_fim", "fim_from_ids_device", "encode_batch_fim", "last_fim_ms"):
        assert hasattr(tk.Engine, name), name
    for name in ("encode_batch_fim", "encode_batch_fim_packed", "encode_fim"):
        assert hasattr(tk.Tekkenizer, name), name
    assert ctypes.sizeof(tk._FimOpts) == 48 and [f[0] for f in tk._FimOpts._fields_] == list(fim_opts())
    L = tk.lib()                                        # (no GPU needed: constants of the build)
    assert L.tk_fim_tile(1) % 16 == 0 and L.tk_fim_tile(4) % 4 == 0 and L.tk_fim_tile(1) > 0 and L.tk_fim_tile(4) > 0
    assert L.tk_fim_tile(2) == 0
    assert tk.fim_q32(0.0) == 0 and tk.fim_q32(1.0) == ONE and tk.fim_q32(0.5) == 1 << 31 and tk.fim_q32(1 - 2.0 ** -40) == ONE
    with pytest.raises(tk.TokenizerError):
        tk.fim_q32(1.5)


def test_result_class_declares_the_header_struct(tk):
    """tests/test_layout_binding_cpu.py's first check, for "fim"."""
    R, members = tk.FimResult, header_members("fim")
    assert R.PASS == "fim"
    assert [o[0] for o in R.OUTPUTS] == [m for m, ptr in members if ptr] == list(ARRAYS)
    assert list(R.COUNTS) == [m for m, ptr in members if not ptr] == list(COUNTS)
    assert [ptr for _, ptr in members] == sorted((ptr for _, ptr in members), reverse=True)
    assert ctypes.sizeof(R.STRUCT) == sum(ctypes.sizeof(ctypes.c_void_p) if ptr else 8 for _, ptr in members)
    assert [f[0] for f in R.STRUCT._fields_] == [m for m, _ in members]
    for (_, ptr), (_, ctype) in zip(members, R.STRUCT._fields_):
        assert ctype is (ctypes.c_void_p if ptr else ctypes.c_uint64)


@pytest.mark.parametrize("unit_bytes,typestr", [(1, "|u1"), (4, "<i4")])
def test_result_attributes_and_views_follow_the_declaration(tk, unit_bytes, typestr):
    R = tk.FimResult
    st = R.STRUCT()
    for i, (field, _) in enumerate(R.STRUCT._fields_):
        setattr(st, field, 0x1000 * (i + 1) if field in ARRAYS else i + 2)
    st.part_src = None
    r = R(st, unit_bytes=unit_bytes)
    views = r.views()
    assert len(views) == len(R.OUTPUTS) and r.unit_bytes == unit_bytes
    for (out, ts, shape, _, optional), v in zip(R.OUTPUTS, views):
        if out == "part_src":
            assert optional and r.part_src_ptr is None and v is None
            continue
        assert not optional and getattr(r, out + "_ptr") == getattr(st, out)
        cai = v.__cuda_array_interface__
        assert cai["data"][0] == getattr(st, out) and cai["shape"] == tuple(shape(r))
        assert cai["typestr"] == (typestr if out == "units" else ts)
    assert views[6].__cuda_array_interface__["shape"] == (st.n_docs, 2)
    for k in R.COUNTS:
        assert getattr(r, k) == getattr(st, k)
    assert set(r._counts()) == set(R.DICT_COUNTS) <= set(R.COUNTS)
