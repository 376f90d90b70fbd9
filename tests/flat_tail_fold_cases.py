"""Layouts for the FOLDED bookkeeping tail of the flat path (csrc/tk_flat_tail_impl.h: tkf_fold_apply_wave, tkf_counts_sums_wave,
tkf_assemble_fold_waves) on top of tests/flat_tail_cases.py: its directed and random layouts, and edges of the folded forms' own
tiles -- documents around a wave (64), a block of the counts kernel (4096) and two blocks; 5 n_chunks around a tile of the miss
side's block sums (2048); sub-queues empty / narrow only / wide only / both / 33..64 bytes only; totals beyond 2^32.

Shared by tests/test_flat_tail_fold_emu.py (the device source on the CPU wave emulator) and tests/flat_tail_fold_worker.py (the
gfx950 kernels through the development build's tk_test_flat_tail_fold).  What a run has to leave is flat_tail_cases.expected():
the folded forms and the pinned ones are both held to it, array for array, so they agree with each other."""
import numpy as np

import flat_tail_cases as ftc

N_DOCS_EDGES = (0, 1, 63, 64, 65, 4095, 4096, 4097, 8193)
N_CHUNKS_EDGES = (1, 409, 410, 820)           # 5 n_chunks = 5, 2045, 2050, 4100: below / above one and two tiles of 2048
QUEUES = ("empty", "narrow", "wide", "both", "long3")

# (fold, miss_max, doc_max) as tk_test_flat_tail_fold / emu_fold_tail take them: the folded forms wherever they can run; the
# bounds forced to 1, so that everything above one partial sum takes the three-kernel scans; and never (the pinned flow)
CONFIGS = ((1, 0, 0), (-1, 1, 1), (0, 0, 0))


def case_n_docs(n):
    L = ftc.Layout(300 + n)
    ftc._small(L, n)
    return L


def case_n_chunks(C, queues="both", seed=0):
    """a few documents, one of them over all the chunks in between, the last ones in chunk C - 1"""
    L = ftc.Layout(400 + C + seed)
    ftc._small(L, 6)
    if C > 1:
        L.doc(segs=(2,), nbytes=(C - 1) * ftc.COMMIT + 5 - L.doc_offs[-1])
    L.doc(segs=(4,), holes="alt")
    L.doc(segs=(70,))
    a = L.arrays()
    assert a["n_chunks"] == C, (a["n_chunks"], C)
    r = np.random.RandomState(500 + C + seed)
    mc = r.randint(0, 4, 4 * C).astype(np.uint32)
    mc[r.randint(0, 4 * C, 3)] = (64, 129, 200)[:3]
    lo = {"empty": (4 * C, 4 * C), "narrow": (0, 2 * C), "wide": (2 * C, 4 * C), "both": (0, 4 * C), "long3": (3 * C, 4 * C)}[queues]
    keep = np.zeros(4 * C, bool)
    keep[lo[0]:lo[1]] = True
    mc[~keep] = 0
    L.miss_count = [int(v) for v in mc]
    return L


def case_big_totals():
    """handed-back documents with counts near 2^31: the optimistic pass leaves them alone, so out_offs and the total pass 2^32
    (nothing is copied); p_base is 2^33 + 12345 as everywhere"""
    L = ftc.Layout(600)
    ftc._small(L, 70)
    for i in range(5):
        L.doc(segs=(3,), nbytes=9, flag=1, staged=4, stale=0x7FFFFFF0 + i)
        L.doc(segs=(5,))
    ftc._small(L, 70)
    return L


def edge_cases():
    for n in N_DOCS_EDGES:
        yield "n_docs_%d" % n, case_n_docs(n)
    for C in N_CHUNKS_EDGES:
        for q in QUEUES:
            yield "n_chunks_%d_%s" % (C, q), case_n_chunks(C, q)
    yield "big_totals", case_big_totals()


def case_many_docs(D=266300):
    """(arrays, expected) for D one-byte documents of 0 or 1 slots each, built and restated with numpy (the Layout's Python loops
    are per document): more than 64 blocks of 4096 documents, so the assembly's strided fold of the block sums runs a second round"""
    COMMIT, STRIDE, HL = ftc.COMMIT, ftc.STRIDE, ftc.HL
    C = (D + COMMIT - 1) // COMMIT
    d = np.arange(D, dtype=np.int64)
    s_d = (d % 3 != 0).astype(np.int64)
    chunk = d // COMMIT
    kcount = np.bincount(chunk, weights=s_d, minlength=C).astype(np.uint32)
    P = np.concatenate(([0], np.cumsum(kcount, dtype=np.int64)))
    before = np.cumsum(s_d) - s_d                              # slots of the stream before the document
    lstart = (before - P[chunk]).astype(np.uint32)
    vals = ((d * 2654435761) & ftc.MAX_ID).astype(np.uint32)
    tmp = np.full(C * STRIDE, ftc.GUARD_FILL, np.uint32)
    has = s_d == 1
    tmp[chunk[has] * STRIDE + lstart[has]] = vals[has]
    r = np.random.RandomState(77)
    a = dict(n_docs=D, n_bytes=D, n_chunks=C, doc_offs=np.arange(D + 1, dtype=np.uint64), kcount=kcount, tmp=tmp, lstart=lstart,
             flags=np.zeros(D, np.uint32), holes=np.zeros(D, np.uint32), counts_in=np.full(D, ftc.SENTINEL, np.uint32),
             staging=np.full(3 * D, ftc.GUARD_FILL, np.uint32), miss_count=r.randint(0, 4, 4 * C).astype(np.uint32),
             counters_in=(0xC0DE0000 + np.arange(ftc.NCTR)).astype(np.uint32), add_bos=1, add_eos=1, bos=1, eos=ftc.MAX_ID, p_base=(1 << 33) + 12345)
    x = {}
    x["first_doc"] = np.minimum(np.maximum(np.arange(C, dtype=np.int64) * COMMIT - HL, 0), D).astype(np.uint32)
    mc = a["miss_count"].astype(np.int64)
    x["wave_first"] = np.repeat(np.arange(2 * C), mc[:2 * C])[::64].astype(np.uint32)
    x["wave_first_wide"] = np.repeat(np.arange(2 * C, 4 * C), mc[2 * C:])[::64].astype(np.uint32)
    x["todo"], x["maxlen"], x["n_flagged"], x["copied"] = [], 0, 0, True
    counts = s_d + 2
    x["counts"] = counts.astype(np.uint32)
    oo = np.concatenate(([0], np.cumsum(counts))).astype(np.uint64)
    x["out_offs"], x["total"] = oo, int(oo[-1])
    ids = np.empty(x["total"], np.uint32)
    o = oo[:-1].astype(np.int64)
    ids[o] = 1
    ids[o[has] + 1] = vals[has]
    ids[o + counts - 1] = ftc.MAX_ID
    x["ids"] = ids
    ctr = a["counters_in"].copy()
    ctr[:ftc.TKC["TKC_CLEARED"]] = 0
    ctr[ftc.TKC["TKC_MEMO_HITS"]] = 0
    ctr[ftc.TKC["TKC_LONG_RECS"]] = 0
    ctr[ftc.TKC["TKC_NARROW_LEFT"]] = int(mc[:2 * C].sum())
    ctr[ftc.TKC["TKC_TODO"]] = ctr[ftc.TKC["TKC_TODO_MAXLEN"]] = ctr[ftc.TKC["TKC_HANDED_BACK"]] = 0
    ctr[ftc.TKC["TKC_TOTAL"]], ctr[ftc.TKC["TKC_TOTAL"] + 1] = x["total"] & 0xFFFFFFFF, x["total"] >> 32
    x["counters"] = ctr
    return a, x


def big_cases():
    """(name, arrays, expected or None): more than 64 partial sums on either side -- the strided parts of the folds run a second
    round only above 131 072 miss entries (26 215 chunks) or 262 144 documents.  For the GPU hook (the emulator would take minutes)."""
    yield "many_chunks_26300", case_n_chunks(26300, "both").arrays(), None
    a, x = case_many_docs()
    yield "many_docs_266300", a, x


def check(call3, a, final_pass, long_recs, configs=CONFIGS, x=None):
    """call3(t, fold, miss_max, doc_max) -> rc; every configuration against the one restatement"""
    x = x or ftc.expected(a, final_pass, long_recs)
    for fold, mm, dm in configs:
        try:
            ftc.run_and_check(lambda t: call3(t, fold, mm, dm), a, final_pass, long_recs, x=x)
        except AssertionError as e:
            raise AssertionError("fold=%d miss_max=%d doc_max=%d: %s" % (fold, mm, dm, e))
