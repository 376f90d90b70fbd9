"""The bookkeeping tail of the flat path -- csrc/tk_flat_tail_impl.h: firstdoc, wavefirst, todo, counts, assemble -- on the CPU
wave emulator against the plain restatement of tests/flat_tail_cases.py, on layouts made for it: every slot count around the
64 / 128 / 256 steps of the copies, documents over two, three and five chunks with empty chunks in between, holes at every
edge, empty documents, document counts around the wave / group-of-eight / block tails, handed-back documents in the
optimistic and in the final pass.  Every array the device source writes sits between guard words (emu_driver.cpp:
run_flat_tail), every array it reads is exactly as long as it has to be.  tests/test_gpu_flat_tail.py runs the same cases
through the gfx950 kernels."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emu"))
import emu  # noqa: E402
import flat_tail_cases as ftc  # noqa: E402


def _call():
    L = emu.lib()
    L.emu_flat_tail.restype = ctypes.c_int
    L.emu_flat_tail.argtypes = [ctypes.POINTER(ftc.TkTestTailCase)]
    return L.emu_flat_tail


def test_constants_are_the_headers():
    out = np.zeros(6, np.uint64)
    L = emu.lib()
    L.emu_flat_consts.restype = None
    L.emu_flat_consts(out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
    assert [int(v) for v in out] == [ftc.COMMIT, ftc.HL, ftc.STRIDE, ftc.HOLE, ftc.TKC["TKC_CLEARED"], ftc.NCTR]
    assert (ftc.COMMIT, ftc.HL) == (1952, 32)


DIRECTED = list(ftc.directed_cases())


@pytest.mark.parametrize("name,layout", DIRECTED, ids=[n for n, _ in DIRECTED])
def test_emu_flat_tail_directed(name, layout):
    a = layout.arrays()
    for final_pass, long_recs in ftc.modes(a):
        try:
            ftc.run_and_check(_call(), a, final_pass, long_recs)
        except AssertionError as e:
            raise AssertionError("%s, final_pass=%d, long-piece records=%d: %s" % (name, final_pass, long_recs, e))


def test_emu_flat_tail_directed_cover_what_they_claim():
    """the layouts reach the paths they are named for (a case that silently stopped doing so would test nothing)"""
    a = dict(DIRECTED)["three_chunks"].arrays()
    spans3 = 0
    for d in range(a["n_docs"]):
        c0, c1 = int(a["doc_offs"][d]) // ftc.COMMIT, int(a["doc_offs"][d + 1]) // ftc.COMMIT
        spans3 += c1 - c0 >= 2
    assert spans3 >= 12
    a = dict(DIRECTED)["todo_huge"].arrays()
    assert ftc.expected(a, 1, 0)["maxlen"] == 0xFFFFFFFF
    a = dict(DIRECTED)["flagged_final"].arrays()
    assert int(a["counts_in"].max()) > int(a["doc_offs"][-1]) + 2 * a["n_docs"]
    assert sorted(set(int(l.arrays()["n_docs"]) for n, l in DIRECTED if n.startswith("n_docs_"))) == [1, 7, 8, 9, 63, 64, 65, 127, 129, 257, 1025]


def test_emu_flat_tail_random_layouts():
    call = _call()
    for seed in range(ftc.N_RANDOM):
        a = ftc.random_layout(seed).arrays()
        flagged = bool(a["flags"].any())
        for final_pass, long_recs in ((0, 0), (1, 0)) if flagged or seed % 4 else ((0, 2), (1, 0)):
            try:
                ftc.run_and_check(call, a, final_pass, long_recs)
            except AssertionError as e:
                raise AssertionError("random layout %d, final_pass=%d, long-piece records=%d: %s" % (seed, final_pass, long_recs, e))
