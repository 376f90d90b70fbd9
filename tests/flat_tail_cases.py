"""Directed layouts for the bookkeeping tail of the flat path (csrc/tk_flat_tail_impl.h: firstdoc, wavefirst, todo, counts,
assemble) and what the tail has to make of them.  Plain numpy, no tokenizer: a layout is what the flat / merge / per-document
kernels would have left behind (chunk-dense ids with holes, per-chunk slot counts, per-document start ranks, flags, hole
counts, staging), built so that it is consistent, and `expected()` restates the definition of every output with plain loops.

Shared by tests/test_flat_tail_emu.py (the device source on the CPU wave emulator) and tests/flat_tail_worker.py (the
gfx950 kernels through the development build's tk_test_flat_tail)."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tekken-rs_amd", "csrc")


def _defines(path, prefix):
    """#define NAME <integer expression of earlier names> -> {NAME: value}"""
    out = {}
    for line in open(path):
        m = re.match(r"#define (%s\w+) (.+)" % prefix, line)
        if not m:
            continue
        expr = re.sub(r"/\*.*", "", m.group(2)).strip()
        expr = re.sub(r"\b(0x[0-9A-Fa-f]+|\d+)[uU]?[lL]*\b", r"\1", expr)
        try:
            out[m.group(1)] = int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(out)))
        except Exception:
            pass          # function-like macros
    return out


def _enum(path, prefix):
    out = {}
    for m in re.finditer(r"\b(%s\w+) = (\d+)" % prefix, open(path).read()):
        out[m.group(1)] = int(m.group(2))
    return out


_F = _defines(os.path.join(CSRC, "tk_flat_args.h"), "TKF_")
TKC = _enum(os.path.join(CSRC, "tk_counters.h"), "TKC_")
COMMIT, HL, STRIDE, HOLE = _F["TKF_COMMIT"], _F["TKF_HL"], _F["TKF_STRIDE"], _F["TKF_HOLE"]
NCTR = TKC["TKC_DEVICE_WORDS"]
GUARD_FILL = 0xDEADBEEF
ID_FILL = 0xA5A5A5A5          # out_ids before the tail runs
SENTINEL = 0x5E5E5E5E         # every other output before the tail runs
MAX_ID = (1 << 18) - 1


class Layout:
    """Documents are appended in order.  A document takes `segs[0]` slots of the chunk its first byte lies in (behind the
    slots of the documents before it), then ALL slots of the following chunks: segs[1], segs[2], ...  It ends `nbytes` bytes
    after its start, or (more than one segment, nbytes not given) `end_off` bytes into the chunk of its last segment."""

    def __init__(self, seed=0, add_bos=1, add_eos=1, bos=1, eos=MAX_ID, p_base=(1 << 33) + 12345):
        self.rng = np.random.RandomState(seed)
        self.add_bos, self.add_eos, self.bos, self.eos, self.p_base = add_bos, add_eos, bos, eos, p_base
        self.doc_offs = [0]
        self.rows = [[]]          # slots of every chunk so far (the last one is open)
        self.lstart, self.flags, self.holes, self.counts_in, self.staged = [], [], [], [], []
        self.miss_count = None
        self.n_chunks_override = None
        self.n_staging_override = None

    # ---- building ----
    def _open_chunk(self, c):
        while len(self.rows) <= c:
            self.rows.append([])

    def doc(self, segs=(0,), nbytes=None, end_off=1, holes="none", flag=0, staged=None, stale=None):
        segs = list(segs)
        b = self.doc_offs[-1]
        c = b // COMMIT
        assert c >= len(self.rows) - 1, "a document starts in a chunk that is already closed"
        n = sum(segs)
        if n == 0 and nbytes == 0 and len(segs) == 1:      # an empty document opens no chunk
            self.lstart.append(len(self.rows[c]) if c < len(self.rows) else 0)
        else:
            self._open_chunk(c)
            self.lstart.append(len(self.rows[c]))
        if callable(holes):
            hs = [bool(holes(i, n)) for i in range(n)]
        else:
            hs = {"none": lambda i: False, "all": lambda i: True, "alt": lambda i: i % 2 == 0, "alt1": lambda i: i % 2 == 1}[holes]
            hs = [hs(i) for i in range(n)]
        vals = [HOLE if h else int(v) for h, v in zip(hs, self.rng.randint(0, MAX_ID + 1, n))]
        if n % 2 and not hs[0]:
            vals[0] = MAX_ID
        k = 0
        for i, s in enumerate(segs):
            if n == 0 and nbytes == 0 and len(segs) == 1:
                break
            self._open_chunk(c + i)
            assert i == 0 or not self.rows[c + i], "a later segment starts a fresh chunk"
            self.rows[c + i] += vals[k:k + s]
            assert len(self.rows[c + i]) <= STRIDE, "more slots than a row of tmp holds"
            k += s
        self.holes.append(sum(1 for v in vals if v == HOLE))
        if nbytes is None:
            nbytes = 1 if len(segs) == 1 else (c + len(segs) - 1) * COMMIT + end_off - b
        e = b + nbytes
        assert e >= b and e // COMMIT >= c + len(segs) - 1, "the document ends before its last chunk"
        self.doc_offs.append(e)
        self.flags.append(1 if flag else 0)
        if flag:
            staged = [int(v) for v in self.rng.randint(0, MAX_ID + 1, 0 if staged is None else staged)]
            assert len(staged) <= nbytes + 2
            self.staged.append(staged)
            self.counts_in.append(len(staged) if stale is None else stale)
        else:
            self.staged.append(None)
            self.counts_in.append(SENTINEL)
        return len(self.flags) - 1

    def next_chunk(self):
        """a document without slots that ends at the first byte of the next chunk"""
        return self.doc(segs=(0, 0), end_off=0)

    def room(self):
        c = self.doc_offs[-1] // COMMIT
        return STRIDE - (len(self.rows[c]) if c < len(self.rows) else 0)

    # ---- the arrays ----
    def arrays(self):
        D = len(self.flags)
        n_bytes = self.doc_offs[-1]
        C = (n_bytes + COMMIT - 1) // COMMIT if self.n_chunks_override is None else self.n_chunks_override
        rows = self.rows[:C]
        assert all(not r for r in self.rows[C:]), "slots beyond the last chunk"
        rows += [[] for _ in range(C - len(rows))]
        a = {}
        a["n_docs"], a["n_bytes"], a["n_chunks"] = D, n_bytes, C
        a["doc_offs"] = np.array(self.doc_offs, np.uint64)
        a["kcount"] = np.array([len(r) for r in rows], np.uint32)
        tmp = np.full(C * STRIDE, GUARD_FILL, np.uint32)          # what the flat kernel never wrote is never read
        for c, r in enumerate(rows):
            tmp[c * STRIDE:c * STRIDE + len(r)] = r
        a["tmp"] = tmp
        a["lstart"] = np.array(self.lstart, np.uint32).reshape(D)
        a["flags"] = np.array(self.flags, np.uint32).reshape(D)
        a["holes"] = np.array(self.holes, np.uint32).reshape(D)
        a["counts_in"] = np.array(self.counts_in, np.uint32).reshape(D)
        ns = n_bytes + 2 * D if self.n_staging_override is None else self.n_staging_override
        st = np.full(ns, GUARD_FILL, np.uint32)
        for d, s in enumerate(self.staged):
            if s:
                o = self.doc_offs[d] + 2 * d
                st[o:o + len(s)] = s
        a["staging"] = st
        if self.miss_count is None:
            mc = self.rng.randint(0, 4, 4 * C).astype(np.uint32)
        else:
            mc = np.array(self.miss_count, np.uint32)
            assert mc.size == 4 * C
        a["miss_count"] = mc
        a["counters_in"] = (0xC0DE0000 + np.arange(NCTR)).astype(np.uint32)
        for k in ("add_bos", "add_eos", "bos", "eos", "p_base"):
            a[k] = getattr(self, k)
        return a


def expected(a, final_pass, long_recs):
    """What the tail must leave, from the definitions (the flat path's bookkeeping)."""
    D, C, n_bytes = a["n_docs"], a["n_chunks"], a["n_bytes"]
    offs = [int(x) for x in a["doc_offs"]]
    kc = [int(x) for x in a["kcount"]]
    P = [0]
    for k in kc:
        P.append(P[-1] + k)
    x = {}
    # first_doc[c]: documents that start below the chunk's loaded region
    x["first_doc"] = np.array([sum(1 for d in range(D) if offs[d] < max(c * COMMIT - HL, 0)) for c in range(C)], np.uint32).reshape(C)
    # wave_first[w]: the sub-queue that holds item 64 w (narrow classes: sub-queues 0 .. 2C-1, wide: 2C .. 4C-1, counted from the first wide item)
    mc = [int(v) for v in a["miss_count"]]

    def firsts(lo, hi):
        owner = []
        for e in range(lo, hi):
            owner += [e] * mc[e]
        return np.array(owner[::64], np.uint32).reshape(-1)
    x["wave_first"], x["wave_first_wide"] = firsts(0, 2 * C), firsts(2 * C, 4 * C)
    n_narrow = sum(mc[:2 * C])
    flagged = [d for d in range(D) if a["flags"][d]]
    x["todo"] = flagged
    x["maxlen"] = min(max([offs[d + 1] - offs[d] for d in flagged] or [0]), 0xFFFFFFFF)
    extra = (1 if a["add_bos"] else 0) + (1 if a["add_eos"] else 0)

    def G(i):
        return P[C] if offs[i] >= n_bytes else P[offs[i] // COMMIT] + int(a["lstart"][i])

    # global slot g (the P[c] + k-th: slot k of chunk c) -> its entry of tmp
    stream = [int(v) for c in range(C) for v in a["tmp"][c * STRIDE:c * STRIDE + kc[c]]]
    counts, docs_ids = [], []
    for d in range(D):
        if a["flags"][d]:
            if final_pass:
                n = min(int(a["counts_in"][d]), offs[d + 1] - offs[d] + 2)
                o = offs[d] + 2 * d
                docs_ids.append([int(v) for v in a["staging"][o:o + n]])
            else:
                n = int(a["counts_in"][d])     # left alone
                docs_ids.append(None)
            counts.append(n)
            continue
        g0, g1 = G(d), G(d + 1)
        assert g0 <= g1, "inconsistent layout"
        ids = [v for v in stream[g0:g1] if v != HOLE]
        assert len(ids) == g1 - g0 - int(a["holes"][d]), "inconsistent layout: holes[d]"
        ids = ([a["bos"]] if a["add_bos"] else []) + ids + ([a["eos"]] if a["add_eos"] else [])
        counts.append(g1 - g0 - int(a["holes"][d]) + extra)
        docs_ids.append(ids)
    x["counts"] = np.array(counts, np.uint32).reshape(D)
    oo = [0]
    for n in counts:
        oo.append(oo[-1] + n)
    x["out_offs"] = np.array(oo, np.uint64)
    x["total"] = oo[-1]
    x["n_flagged"] = 0 if final_pass else len(flagged)
    x["copied"] = bool(final_pass) or (not flagged and not long_recs)
    x["ids"] = np.array([v for ids in docs_ids for v in ids], np.uint32) if x["copied"] else None
    ctr = a["counters_in"].copy()
    ctr[:TKC["TKC_CLEARED"]] = 0
    ctr[TKC["TKC_MEMO_HITS"]] = 0
    ctr[TKC["TKC_LONG_RECS"]] = long_recs
    if C:
        ctr[TKC["TKC_NARROW_LEFT"]] = min(n_narrow, 0xFFFFFFFF)
    if D:
        ctr[TKC["TKC_TODO"]] = len(flagged)
        ctr[TKC["TKC_TODO_MAXLEN"]] = x["maxlen"]
        ctr[TKC["TKC_HANDED_BACK"]] = x["n_flagged"]
        ctr[TKC["TKC_TOTAL"]] = x["total"] & 0xFFFFFFFF
        ctr[TKC["TKC_TOTAL"] + 1] = x["total"] >> 32
    x["counters"] = ctr
    return x


# ---- running a layout through emu_flat_tail / tk_test_flat_tail ----
_u32p, _u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)


class TkTestTailCase(ctypes.Structure):           # csrc/tk_test_hooks.h
    _fields_ = [("n_docs", ctypes.c_uint64), ("n_bytes", ctypes.c_uint64), ("n_chunks", ctypes.c_uint64), ("p_base", ctypes.c_uint64),
                ("doc_offs", _u64p), ("kcount", _u32p), ("miss_count", _u32p), ("lstart", _u32p), ("flags", _u32p), ("holes", _u32p),
                ("tmp", _u32p), ("staging", _u32p), ("n_staging", ctypes.c_uint64), ("counters_in", _u32p),
                ("long_recs", ctypes.c_uint32), ("bos_id", ctypes.c_uint32), ("eos_id", ctypes.c_uint32),
                ("add_bos", ctypes.c_int32), ("add_eos", ctypes.c_int32), ("final_pass", ctypes.c_int32),
                ("out_cap", ctypes.c_uint64), ("n_wave_first", ctypes.c_uint64), ("n_wave_first_wide", ctypes.c_uint64),
                ("counts", _u32p), ("out_ids", _u32p), ("first_doc", _u32p), ("flags_cleared", _u32p), ("holes_cleared", _u32p),
                ("wave_first", _u32p), ("wave_first_wide", _u32p), ("todo", _u32p), ("out_offs", _u64p), ("counters_out", _u32p),
                ("err", ctypes.c_char_p), ("err_cap", ctypes.c_uint32)]


def _ptr(arr, ct):
    return arr.ctypes.data_as(ctypes.POINTER(ct))


def run_and_check(call, a, final_pass, long_recs, x=None):
    """call(pointer to TkTestTailCase) -> rc.  Raises AssertionError naming the first array that is not what expected() says."""
    x = x or expected(a, final_pass, long_recs)
    D, C = a["n_docs"], a["n_chunks"]
    cap = x["total"] + 8 if x["copied"] else 64     # (nothing may be written when the pass copies nothing)
    out = dict(counts=a["counts_in"].copy(), out_ids=np.full(cap, ID_FILL, np.uint32), first_doc=np.full(C, SENTINEL, np.uint32),
               flags_cleared=np.full(D + 1, SENTINEL, np.uint32), holes_cleared=np.full(D + 1, SENTINEL, np.uint32),
               wave_first=np.full(x["wave_first"].size, SENTINEL, np.uint32), wave_first_wide=np.full(x["wave_first_wide"].size, SENTINEL, np.uint32),
               todo=np.full(D, SENTINEL, np.uint32), out_offs=np.full(D + 1, SENTINEL, np.uint64), counters_out=np.zeros(NCTR, np.uint32))
    err = ctypes.create_string_buffer(512)
    t = TkTestTailCase()
    t.n_docs, t.n_bytes, t.n_chunks, t.p_base = D, a["n_bytes"], C, a["p_base"]
    t.doc_offs = _ptr(a["doc_offs"], ctypes.c_uint64)
    for k in ("kcount", "miss_count", "lstart", "flags", "holes", "tmp", "staging", "counters_in"):
        setattr(t, k, _ptr(a[k], ctypes.c_uint32))
    t.n_staging = a["staging"].size
    t.long_recs, t.bos_id, t.eos_id = long_recs, a["bos"], a["eos"]
    t.add_bos, t.add_eos, t.final_pass = a["add_bos"], a["add_eos"], final_pass
    t.out_cap, t.n_wave_first, t.n_wave_first_wide = cap, x["wave_first"].size, x["wave_first_wide"].size
    for k, v in out.items():
        setattr(t, k, _ptr(v, ctypes.c_uint64 if k == "out_offs" else ctypes.c_uint32))
    t.err = ctypes.cast(err, ctypes.c_char_p)
    t.err_cap = 512
    rc = call(ctypes.byref(t))
    assert rc == 0, "rc=%d: %s" % (rc, err.value.decode(errors="replace"))     # (a changed guard word ends here)

    def same(name, got, want):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape, "%s: %d entries, expected %d" % (name, got.size, want.size)
        if not np.array_equal(got, want):
            i = int(np.flatnonzero(got != want)[0])
            raise AssertionError("%s[%d] = %d, expected %d (%d entries differ)" % (name, i, int(got[i]), int(want[i]), int((got != want).sum())))
    same("first_doc", out["first_doc"], x["first_doc"])
    same("flags after the pre-pass", out["flags_cleared"], np.zeros(D + 1, np.uint32))
    same("holes after the pre-pass", out["holes_cleared"], np.zeros(D + 1, np.uint32))
    same("wave_first", out["wave_first"], x["wave_first"])
    same("wave_first_wide", out["wave_first_wide"], x["wave_first_wide"])
    same("counters", out["counters_out"], x["counters"])
    # the list as a set (the waves append with an atomic: any order between them), in document order inside a wave
    n = len(x["todo"])
    got = [int(v) for v in out["todo"][:n]]
    assert sorted(got) == x["todo"], "todo: %r, expected the documents %r" % (got[:20], x["todo"][:20])
    pos = {d: i for i, d in enumerate(got)}
    for d0, d1 in zip(x["todo"], x["todo"][1:]):
        if d0 // 64 == d1 // 64:
            assert pos[d1] == pos[d0] + 1, "todo: documents %d and %d of one wave are not neighbours in order" % (d0, d1)
    same("todo past n_todo", out["todo"][n:], np.full(D - n, SENTINEL, np.uint32))
    same("counts", out["counts"], x["counts"])
    same("out_offs", out["out_offs"], x["out_offs"])
    if x["copied"] and D:
        same("out_ids", out["out_ids"][:x["total"]], x["ids"])
        same("out_ids past the total", out["out_ids"][x["total"]:], np.full(8, ID_FILL, np.uint32))
    else:
        same("out_ids (nothing may be copied)", out["out_ids"], np.full(cap, ID_FILL, np.uint32))


# ---- the cases ----
def _small(L, n_docs, hi=20):
    """n_docs short documents of one byte each (a few longer ones, a few of them over a chunk boundary)"""
    end = len(L.flags) + n_docs
    while len(L.flags) < end:
        s = int(L.rng.randint(0, hi + 1))
        if len(L.flags) % 37 == 5:
            s = int(L.rng.choice([127, 128, 129, 200]))
        if s > L.room():
            L.next_chunk()                       # (one of the n_docs)
            continue
        L.doc(segs=(s,), holes=str(L.rng.choice(["none", "none", "alt", "alt1"])) if s else "none")


def case_single_chunk_counts():
    L = Layout(1)
    for s in list(range(131)) + [191, 192, 193, 255, 256, 257, 300, 513, 2000]:
        if s > L.room():
            L.next_chunk()
        L.doc(segs=(s,), holes="none" if s % 3 else "alt")
    return L


def case_two_chunks():
    L = Layout(2)
    for nf in (0, 1, 63, 64, 65, 127, 128):
        for rest in (1, 63, 64, 65, 127):
            if nf > L.room():
                L.next_chunk()
            L.doc(segs=(nf, rest))               # nf = 0 behind another document: rest == the next chunk's kcount only if nothing follows in it
            L.doc(segs=(3,))                     # the next chunk holds more than `rest`
    L.next_chunk()
    for nf, rest in ((0, 64), (1, 127), (64, 64), (100, 28), (100, 29), (127, 1), (128, 1)):
        L.doc(segs=(nf, rest, 0), end_off=0)     # rest == kcount of the next chunk exactly (the chunk after it starts empty)
    L.doc(segs=(5,))
    return L


def case_three_chunks():
    L = Layout(3)
    for a_, mid, b_ in ((10, 0, 10), (10, 1, 10), (0, 0, 5), (0, 1, 1), (60, 1, 60), (63, 0, 65), (1, 0, 1), (126, 1, 1), (5, 7, 1), (64, 63, 1)):
        if a_ > L.room():
            L.next_chunk()
        L.doc(segs=(a_, mid, b_))                # <= 128 slots, `rest` one more than the middle chunk holds: no two-segment copy
        L.doc(segs=(2,))
    L.doc(segs=(10, 0, 0, 0, 20))
    L.next_chunk()
    L.doc(segs=(500, 2000, STRIDE, 1, 700), holes="alt")       # thousands of slots over five chunks
    L.doc(segs=(300, STRIDE, 0, 1999, 1))
    L.doc(segs=(0, 50))                          # the first chunk contributes nothing
    L.doc(segs=(0, 0, 5))
    L.next_chunk()
    L.doc(segs=(0, 2000))
    L.doc(segs=(1,))
    return L


def case_holes():
    L = Layout(4)
    pats = ["none", "all", "alt", "alt1", lambda i, n: i in (0, 63, 64, 127, n - 1)]
    for segs in ((129,), (128,), (64,), (65,), (1,), (300,), (60, 40), (64, 64), (1, 127), (100, 400), (30, 0, 30), (64, 1, 63)):
        for p in pats + [lambda i, n, nf=segs[0]: i in (nf - 1, nf), lambda i, n, nf=segs[0]: i in (nf - 2, nf - 1), lambda i, n, nf=segs[0]: i in (nf, nf + 1)]:
            if segs[0] > L.room():
                L.next_chunk()
            L.doc(segs=segs, holes=p)
    return L


def case_empty_documents():
    L = Layout(5)
    for _ in range(5):
        L.doc(nbytes=0)                          # a run at the start
    _small(L, 9)
    for _ in range(70):
        L.doc(nbytes=0)                          # in the middle, over a wave boundary
    _small(L, 3)
    L.next_chunk()
    for _ in range(4):
        L.doc(nbytes=0)                          # at a chunk's first byte
    L.doc(segs=(7,))
    L.doc(segs=(12, 0), end_off=0)
    L.doc(nbytes=0)
    L.doc(segs=(1,))
    for _ in range(11):
        L.doc(nbytes=0)                          # trailing: doc_offs == n_bytes
    return L


def case_no_bytes():
    L = Layout(6)
    for _ in range(5):
        L.doc(nbytes=0)
    return L


def case_no_documents():
    return Layout(7)


def case_n_docs(n):
    L = Layout(100 + n)
    _small(L, n)
    return L


def case_flags(which, seed=8):
    L = Layout(seed)
    for d in range(200):
        f = {"none": False, "one": d == 70, "wave": 64 <= d < 128, "several": d % 3 == 0 or d >= 190}[which]
        n = int(L.rng.randint(1, 30))
        if n > L.room():
            L.next_chunk()
        L.doc(segs=(n,), nbytes=n, flag=f, staged=int(L.rng.randint(0, n + 3)) if f else None)
    return L


def case_flagged_final():
    L = Layout(9)
    for i, st in enumerate((0, 1, 64, 65, 1000, 3, 2)):
        L.doc(segs=(5,), nbytes=max(st, 3), flag=1, staged=st)
        L.doc(segs=(6 + i,), holes="alt")        # flagged and unflagged documents inside one group of eight
    L.doc(segs=(4,), nbytes=10, flag=1, staged=12, stale=13)            # a stale count above len + 2 is clamped
    L.doc(segs=(4,), nbytes=10, flag=1, staged=12, stale=0xFFFFFFF0)
    L.doc(segs=(0,), nbytes=0, flag=1, staged=2, stale=77)
    L.doc(segs=(9, 3))
    L.doc(segs=(130,), nbytes=200, flag=1, staged=150)
    L.doc(segs=(2,))
    return L


def case_bos_eos(add_bos, add_eos):
    L = Layout(10, add_bos=add_bos, add_eos=add_eos, bos=MAX_ID, eos=MAX_ID - 1)
    _small(L, 40)
    L.doc(segs=(100, 30))
    L.doc(segs=(100, 600, 3))
    L.doc(segs=(2,), nbytes=9, flag=1, staged=11)
    return L


def case_p_base(base):
    L = Layout(11, p_base=base)
    _small(L, 70)
    L.doc(segs=(50, 60))
    L.doc(segs=(50, 1, 60))
    return L


def case_firstdoc_boundaries():
    L = Layout(12)
    for c, off in ((1, -1), (2, 0), (3, 1), (4, -1), (4, 0), (4, 1)):    # document boundaries around c * COMMIT - HL
        L.doc(segs=(3,), nbytes=c * COMMIT - HL + off - L.doc_offs[-1])
    L.doc(segs=(1,), nbytes=10 * COMMIT + 17)                            # one document over many chunks
    L.doc(segs=(2,), nbytes=COMMIT - HL)
    L.doc(segs=(1,), nbytes=3 * COMMIT)                                  # the last document owns every chunk above its start
    return L


def case_firstdoc_few_documents():
    L = Layout(13)
    L.doc(segs=(4, 0, 0, 9))
    L.doc(segs=(1,), nbytes=5)
    L.doc(segs=(1,), nbytes=2 * COMMIT)
    return L


def case_wavefirst(which):
    L = Layout(14)
    L.doc(segs=(3, 0, 0, 2))                     # four chunks: sixteen sub-queues
    C = 4
    mc = {"empty": [0, 5, 0, 0, 70, 0, 0, 1] + [0, 0, 130, 0, 0, 0, 0, 3],
          "long": [200, 1, 0, 63, 0, 0, 64, 0] + [1, 0, 0, 200, 0, 0, 0, 0],
          "multiples": [64, 64, 128, 0, 0, 64, 0, 0] + [0, 128, 0, 0, 64, 0, 0, 64],
          "no_narrow": [0] * 8 + [3, 0, 100, 0, 0, 0, 65, 0],
          "no_wide": [3, 0, 100, 0, 0, 0, 65, 0] + [0] * 8,
          "none": [0] * 16}[which]
    assert len(mc) == 4 * C
    L.miss_count = mc
    return L


def case_todo_huge():
    """a handed-back document of 2^32 + 5 bytes: the longest-document word saturates.  (One chunk stands in for its two
    million: the tail looks at the chunks of the documents that start below n_bytes only.)"""
    L = Layout(15)
    L.doc(segs=(4,), nbytes=(1 << 32) + 5, flag=1, staged=3)
    for _ in range(3):
        L.doc(nbytes=0)
    L.n_chunks_override = 1
    L.n_staging_override = 16
    return L


def random_layout(seed):
    r = np.random.RandomState(1000 + seed)
    L = Layout(2000 + seed, add_bos=int(r.randint(2)), add_eos=int(r.randint(2)), p_base=int(r.choice([0, 7, (1 << 33) + 12345])))
    n_docs, max_chunks = int(r.choice([0, 1, 5, 20, 60, 64, 65, 130, 300])), int(r.randint(1, 7))
    n_docs = int(r.randint(0, n_docs + 1))
    flag_p = float(r.choice([0, 0, 0.02, 0.3]))
    for _ in range(n_docs):
        b = L.doc_offs[-1]
        left = max_chunks - 1 - b // COMMIT      # chunks the document may still move on
        if r.randint(10) == 0:
            L.doc(nbytes=0)
            continue
        nseg = 1 if left <= 0 or r.randint(10) < 7 else int(r.randint(2, min(left, 4) + 2))
        hi = int(r.choice([3, 30, 130, 300, 2000]))
        segs = [int(r.randint(0, min(hi, L.room()) + 1))] + [int(r.randint(0, min(hi, STRIDE) + 1)) * int(r.randint(4) > 0) for _ in range(nseg - 1)]
        nb = int(r.randint(1, 40)) if nseg == 1 and (b + 40) // COMMIT < max_chunks else (1 if nseg == 1 else None)
        f = bool(r.rand() < flag_p)
        L.doc(segs=segs, nbytes=nb, end_off=int(r.choice([0, 1, 5])) if segs[-1] == 0 else int(r.choice([1, 5])),
              holes=str(r.choice(["none", "none", "alt", "alt1", "all"])), flag=f,
              staged=int(r.randint(0, (nb if nb is not None else 50) + 3)) if f else None, stale=(0xFFFFFFFF if f and r.randint(5) == 0 else None))
    return L


def directed_cases():
    """(name, Layout) -- every one is run through the optimistic and the final pass (modes())."""
    yield "single_chunk_counts", case_single_chunk_counts()
    yield "two_chunks", case_two_chunks()
    yield "three_chunks", case_three_chunks()
    yield "holes", case_holes()
    yield "empty_documents", case_empty_documents()
    yield "no_bytes", case_no_bytes()
    yield "no_documents", case_no_documents()
    for n in (1, 7, 8, 9, 63, 64, 65, 127, 129, 257, 1025):
        yield "n_docs_%d" % n, case_n_docs(n)
    for w in ("none", "one", "wave", "several"):
        yield "flags_%s" % w, case_flags(w)
    yield "flagged_final", case_flagged_final()
    for b in (0, 1):
        for e in (0, 1):
            yield "bos%d_eos%d" % (b, e), case_bos_eos(b, e)
    yield "p_base_0", case_p_base(0)
    yield "p_base_2p33", case_p_base((1 << 33) + 12345)
    yield "firstdoc_boundaries", case_firstdoc_boundaries()
    yield "firstdoc_few_documents", case_firstdoc_few_documents()
    for w in ("empty", "long", "multiples", "no_narrow", "no_wide", "none"):
        yield "wavefirst_%s" % w, case_wavefirst(w)
    yield "todo_huge", case_todo_huge()


def modes(a):
    """(final_pass, long_recs): the optimistic pass alone and with long-piece records waiting (the second skip word), the final pass"""
    return [(0, 0), (0, 3), (1, 0)]


N_RANDOM = 300
