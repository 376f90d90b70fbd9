"""The FOLDED bookkeeping tail of the flat path -- csrc/tk_flat_tail_impl.h: tkf_fold_apply_wave, tkf_counts_sums_wave,
tkf_assemble_fold_waves -- on the CPU wave emulator (tests/emu/emu_fold_driver.cpp).  Every directed and random layout of
tests/flat_tail_cases.py and the edges of tests/flat_tail_fold_cases.py, optimistic and final pass, in three configurations:
folded wherever it can run, the bounds forced to 1 (the three-kernel forms above one partial sum), and the pinned flow.  All
three are held to flat_tail_cases.expected() array for array (counts, out_offs, out_ids, wave_first*, the counters), so the
folded forms give exactly what the pinned bodies give; the folded miss_prefix is compared with the scan inside the driver.  Every
array the device source writes sits between guard words.  tests/test_gpu_flat_tail_fold.py runs the same through the kernels."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import flat_tail_cases as ftc  # noqa: E402
import flat_tail_fold_cases as ffc  # noqa: E402

_LIB = None


def _lib():
    """tests/emu/libtk_emu_fold.so, rebuilt when a source is newer"""
    global _LIB
    if _LIB is None:
        emu_dir, csrc = os.path.join(HERE, "emu"), os.path.join(ROOT, "tekken-rs_amd", "csrc")
        so = os.path.join(emu_dir, "libtk_emu_fold.so")
        srcs = [os.path.join(emu_dir, f) for f in ("emu_fold_driver.cpp", "tk_wave_emu.h")] + \
               [os.path.join(csrc, f) for f in ("tk_flat_tail_impl.h", "tk_flat_args.h", "tk_counters.h", "tk_test_hooks.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                                   "-shared", "-o", so, srcs[0]])
        _LIB = ctypes.CDLL(so)
        _LIB.emu_fold_tail.restype = ctypes.c_int
        _LIB.emu_fold_tail.argtypes = [ctypes.POINTER(ftc.TkTestTailCase), ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32]
        _LIB.emu_fold_wave_sums.restype = None
    return _LIB


def _call3(t, fold, mm, dm):
    return _lib().emu_fold_tail(t, fold, mm, dm)


def test_wave_sums_are_exact_in_64_bits():
    """the slices the 32-bit wave scan adds up: sums mod 2^64 of arbitrary values, the exclusive scan of values below 2^36"""
    rng = np.random.RandomState(5)
    for v in (np.zeros(64, np.uint64), np.full(64, 0xFFFFFFFFFFFFFFFF, np.uint64), np.full(64, (1 << 36) - 1, np.uint64),
              rng.randint(0, 1 << 63, 64, dtype=np.uint64) * np.uint64(2) + np.uint64(1), rng.randint(0, 1 << 32, 64, dtype=np.uint64)):
        out = np.zeros(65, np.uint64)
        _lib().emu_fold_wave_sums(v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
        low = [int(x) & ((1 << 36) - 1) for x in v]
        assert [int(x) for x in out[:64]] == [sum(low[:i]) for i in range(64)]
        assert int(out[64]) == sum(int(x) for x in v) % (1 << 64)


DIRECTED = list(ftc.directed_cases())
EDGES = list(ffc.edge_cases())


@pytest.mark.parametrize("name,layout", DIRECTED + EDGES, ids=[n for n, _ in DIRECTED] + ["edge_" + n for n, _ in EDGES])
def test_emu_fold_tail_directed_and_edges(name, layout):
    a = layout.arrays()
    for final_pass, long_recs in ftc.modes(a):
        try:
            ffc.check(_call3, a, final_pass, long_recs)
        except AssertionError as e:
            raise AssertionError("%s, final_pass=%d, long-piece records=%d: %s" % (name, final_pass, long_recs, e))


def test_emu_fold_edges_cover_what_they_claim():
    got = dict(EDGES)
    assert sorted(int(got["n_docs_%d" % n].arrays()["n_docs"]) for n in ffc.N_DOCS_EDGES) == sorted(ffc.N_DOCS_EDGES)
    for C in ffc.N_CHUNKS_EDGES:
        a = got["n_chunks_%d_long3" % C].arrays()
        assert a["n_chunks"] == C and a["miss_count"][:3 * C].sum() == 0 and a["miss_count"][3 * C:].sum() > 0
        assert got["n_chunks_%d_narrow" % C].arrays()["miss_count"][2 * C:].sum() == 0
        assert got["n_chunks_%d_empty" % C].arrays()["miss_count"].sum() == 0
    assert ftc.expected(got["big_totals"].arrays(), 0, 0)["total"] > 1 << 32
    # with the bounds at 1 both forms run: a case of one partial sum folds, the cases above it fall back
    assert (5 * 409 + 2047) // 2048 == 1 and (5 * 410 + 2047) // 2048 == 2 and (4096 + 4095) // 4096 == 1 and (4097 + 4095) // 4096 == 2


def test_emu_fold_tail_random_layouts():
    for seed in range(ftc.N_RANDOM):
        a = ftc.random_layout(seed).arrays()
        flagged = bool(a["flags"].any())
        for final_pass, long_recs in ((0, 0), (1, 0)) if flagged or seed % 4 else ((0, 2), (1, 0)):
            try:
                ffc.check(_call3, a, final_pass, long_recs, configs=ffc.CONFIGS[:2])
            except AssertionError as e:
                raise AssertionError("random layout %d, final_pass=%d, long-piece records=%d: %s" % (seed, final_pass, long_recs, e))
